// image_counts.h — periodic image counts of wrapped coordinates r [F][3][E], rebuilt on the device: the first step of
// mdhip_displacement_hist (displacement.hip) and of mdhip_self_relaxation (relaxation.hip). include/mdhip.h states the
// rule under mdhip_displacement_hist: n(0) = 0, n(f) = n(f-1) - 1 when d = x(f) - x(f-1) > L(f)/2, + 1 when
// d < -L(f)/2 (strict; a NaN shifts nothing); the callers form xu(f) = x(f) + (double)n(f) * L(f), unfused.
//
// Image counts never wait across workgroups. They take three launches over columns c = (axis, entity) of the
// F x 3E matrix, threads along c so that every load of [f][.] coalesces:
//   dp_image_kernel<false>  per (chunk of DP_CHUNK frames, column): the sum of the chunk's shifts, and the crossings
//   dp_chunk_scan_kernel    per column: exclusive scan of those sums over the chunks (a short serial loop)
//   dp_image_kernel<true>   per (chunk, column): the shifts again from the chunk's start value -> int32 n [F][3E]
// The n(f) are integers: the same whatever the chunking.
#pragma once
#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_CHUNK = 64;           // frames per chunk of the image-count passes
constexpr int DP_MAX_Y = 65535;

// Sum of the chunk's shifts per column (WRITE = false: tot[chunk][c], and the number of shifts into *crossings), or the
// image counts themselves from the scanned sums (WRITE = true: img[f][c]). Block (x, y): columns x * 256 .. (grid
// stride), chunk ch0 + y.
template <bool WRITE>
__global__ __launch_bounds__(DP_THREADS) void dp_image_kernel(const double *__restrict__ r,
                                                              const double *__restrict__ box, long long F,
                                                              long long E, long long ch0, int *__restrict__ tot,
                                                              int *__restrict__ img,
                                                              unsigned long long *__restrict__ crossings)
{
    __shared__ unsigned s_cross;
    const long long ncol = 3 * E;
    const long long ch = ch0 + blockIdx.y;
    const long long f0 = ch * DP_CHUNK, f1 = f0 + DP_CHUNK < F ? f0 + DP_CHUNK : F;
    unsigned n_cross = 0;
    if (!WRITE) {
        if (threadIdx.x == 0) s_cross = 0u;
        __syncthreads();
    }
    for (long long c = (long long)blockIdx.x * DP_THREADS + threadIdx.x; c < ncol;
         c += (long long)gridDim.x * DP_THREADS) {
        const int axis = (int)(c / E);
        int n = WRITE ? tot[ch * ncol + c] : 0;
        long long f = f0;
        double prev;
        if (f0 == 0) {
            prev = r[c];
            if (WRITE) img[c] = 0;
            f = 1;
        } else {
            prev = r[(f0 - 1) * ncol + c];
        }
#pragma unroll 8
        for (; f < f1; ++f) {
            const double x = r[f * ncol + c];
            const double half = 0.5 * box[f * 3 + axis];
            const double d = x - prev;
            const int s = d > half ? -1 : (d < -half ? 1 : 0);  // (a NaN compares false twice)
            n += s;
            if (WRITE)
                img[f * ncol + c] = n;
            else
                n_cross += s != 0;
            prev = x;
        }
        if (!WRITE) tot[ch * ncol + c] = n;
    }
    if (!WRITE) {
        for (int o = 32; o; o >>= 1) n_cross += __shfl_xor(n_cross, o);
        if ((threadIdx.x & 63) == 0 && n_cross) atomicAdd(&s_cross, n_cross);
        __syncthreads();
        if (threadIdx.x == 0 && s_cross) atomicAdd(crossings, (unsigned long long)s_cross);
    }
}

// tot[ch][c] <- sum of tot[0 .. ch - 1][c]: one lane per column.
__global__ __launch_bounds__(DP_THREADS) void dp_chunk_scan_kernel(int *__restrict__ tot, long long n_chunks,
                                                                   long long ncol)
{
    for (long long c = (long long)blockIdx.x * DP_THREADS + threadIdx.x; c < ncol;
         c += (long long)gridDim.x * DP_THREADS) {
        int run = 0;
        for (long long ch = 0; ch < n_chunks; ++ch) {
            const int t = tot[ch * ncol + c];
            tot[ch * ncol + c] = run;
            run += t;
        }
    }
}

// The three launches on the context's stream, for n_frames >= 2 and n_ent >= 1: box goes to the device (WS_BOX), the
// image counts to WS_AUX0 (WS_AUX1 holds the chunk sums), the number of shifts is added to *d_cross (a zeroed device
// word). `launches` counts what was launched.
inline int dp_image_counts(mdhip_ctx *ctx, const double *d_r, const double *box, long long n_frames, long long n_ent,
                           unsigned long long *d_cross, const double *&d_box, const int *&d_img, int &launches)
{
    int rc;
    const long long ncol = 3 * n_ent, n_chunks = (n_frames + DP_CHUNK - 1) / DP_CHUNK;
    MD_WS(d_b, double, WS_BOX, (size_t)n_frames * 24);
    if ((rc = mdhip_h2d_small(ctx, d_b, box, (size_t)n_frames * 24))) return rc;
    MD_WS(d_tot, int, WS_AUX1, (size_t)n_chunks * (size_t)ncol * 4);
    MD_WS(d_n, int, WS_AUX0, (size_t)n_frames * (size_t)ncol * 4);
    const unsigned gx = (unsigned)std::min<long long>((ncol + DP_THREADS - 1) / DP_THREADS, 65535);
    // grid.y holds at most 65535 chunks: longer trajectories go in slices
    for (long long c0 = 0; c0 < n_chunks; c0 += DP_MAX_Y, ++launches) {
        const unsigned gy = (unsigned)std::min<long long>(DP_MAX_Y, n_chunks - c0);
        hipLaunchKernelGGL(dp_image_kernel<false>, dim3(gx, gy), dim3(DP_THREADS), 0, ctx->stream, d_r, d_b, n_frames,
                           n_ent, c0, d_tot, (int *)nullptr, d_cross);
        MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(dp_chunk_scan_kernel, dim3(gx), dim3(DP_THREADS), 0, ctx->stream, d_tot, n_chunks, ncol);
    MD_HIP(hipGetLastError());
    ++launches;
    for (long long c0 = 0; c0 < n_chunks; c0 += DP_MAX_Y, ++launches) {
        const unsigned gy = (unsigned)std::min<long long>(DP_MAX_Y, n_chunks - c0);
        hipLaunchKernelGGL(dp_image_kernel<true>, dim3(gx, gy), dim3(DP_THREADS), 0, ctx->stream, d_r, d_b, n_frames,
                           n_ent, c0, d_tot, d_n, (unsigned long long *)nullptr);
        MD_HIP(hipGetLastError());
    }
    d_box = d_b;
    d_img = d_n;
    ctx->last_kernel = "dp_image_kernel";
    return MDHIP_OK;
}

}  // namespace
