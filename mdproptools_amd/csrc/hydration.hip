// hydration.hip — cation-water orientation cosines of hydration_number.get_hydration_number.
//
// Replaces the per-cation pandas merges of structural/hydration_number.py:13-99 of the reference: for each cation atom
// of each frame, the waters whose O lies within r_cut (single-wrap rsq, rdf_cn.py:36-58) and the cosine between
// d = cation - O (wrapped) and the water's v = (H1 + H2) - 2 O (raw coordinates, hydration_number.py:69-71):
//   cos = dot(d, v) / (|d| |v|),  dot = ((0 + dx vx) + dy vy) + dz vz,  |a| = sqrt((ax ax + ay ay) + az az)
// (numpy's sum / linalg.norm over three columns, hydration_number.py:28-32). Contraction is off in this file; f64
// sqrt and division compile to the correctly rounded sequences, so every cosine is numpy's double.
//
//  1. hy_water_kernel: one lane per (frame, water): the O planes and v planes [F][6][n_w]; v's H1 + H2 is pandas'
//     group sum, (0 + H1) + H2.
//  2. hy_search_kernel<COUNTS>: one block per (frame, tile of HY_TC cations, chunk of HY_CHUNK waters), grid-stride
//     over a flattened block index (no launch dimension grows with the frames). The lanes walk the chunk's O planes and
//     test each against every cation of the tile (wave-uniform coordinates) with the |d| form of the wrap (the same
//     rsq as d - sign(d) L; see clusters.hip). A hit is rare:
//       list mode: the water index is appended to the row (frame, cation); count stays exact past `cap` (the host then
//         re-runs the frames that overflowed with a larger cap);
//       counts mode: the cosine is computed at once; n_water, n_away (cos < cos_cut) per row and an exact histogram
//         (bin trunc((cos + 1) / w) clamped to n_bins - 1, NaN in no bin) kept per block in LDS, added to the global
//         uint64 bins once per block.
//  3. hy_row_kernel (list mode): one wave per row ranks the row's water indices (distinct) through LDS and writes each
//     index and its cosine at its rank: the waters in ascending molecule order, padded with -1 / NaN to `cap`.

#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

namespace {

constexpr int HY_THREADS = 256;
constexpr int HY_TC = 16;          // cations per block
constexpr int HY_CHUNK = 4096;     // waters per block (16 per lane)
constexpr int HY_MAX_CAP = 16384;  // the row pass stages a row in LDS (64 KB)
constexpr int HY_MAX_BINS = 4096;  // the counts pass keeps its histogram in LDS (32 KB)

// |d - sign(d) L| when d > L/2 or d < -L/2, else |d| (rdf_cn.py:50-55), as min(|d|, ||d| - L|): the same double
__device__ __forceinline__ double hy_wrap_abs(double d, double L)
{
    const double a = __builtin_fabs(d);
    return __builtin_fmin(a, __builtin_fabs(a - L));
}

// the signed wrap itself (the cosine needs the direction): d - sign(d) L when d > L/2 or d < -L/2
__device__ __forceinline__ double hy_wrap(double d, double L)
{
    const double h = 0.5 * L;
    return d > h ? d - L : (d < -h ? d + L : d);
}

__device__ __forceinline__ double hy_rsq(double cx, double cy, double cz, double x, double y, double z, double Lx,
                                         double Ly, double Lz)
{
    const double ax = hy_wrap_abs(cx - x, Lx);
    const double ay = hy_wrap_abs(cy - y, Ly);
    const double az = hy_wrap_abs(cz - z, Lz);
    return (ax * ax + ay * ay) + az * az;
}

// cosine of (cation - O, wrapped) and v of water w of the frame's planes p (ox oy oz vx vy vz, each n_w long)
__device__ __noinline__ double hy_cos(double cx, double cy, double cz, const double *__restrict__ p, long long n_w,
                                      long long w, double Lx, double Ly, double Lz)
{
    const double dx = hy_wrap(cx - p[w], Lx);
    const double dy = hy_wrap(cy - p[n_w + w], Ly);
    const double dz = hy_wrap(cz - p[2 * n_w + w], Lz);
    const double vx = p[3 * n_w + w], vy = p[4 * n_w + w], vz = p[5 * n_w + w];
    const double dot = ((0.0 + dx * vx) + dy * vy) + dz * vz;
    const double n1 = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
    const double n2 = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
    return dot / (n1 * n2);
}

__global__ __launch_bounds__(256) void hy_water_kernel(const double *__restrict__ xyz, long long n,
                                                       const int *__restrict__ waters, long long n_w, long long total,
                                                       double *__restrict__ wat)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long w = i % n_w, f = i / n_w;
        const long long a = waters[w];
        double *o = wat + (size_t)f * 6 * (size_t)n_w;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *pk = xyz + ((size_t)f * 3 + k) * (size_t)n;
            const double a0 = pk[a];
            o[k * n_w + w] = a0;
            o[(3 + k) * n_w + w] = ((0.0 + pk[a + 1]) + pk[a + 2]) - 2.0 * a0;
        }
    }
}

template <bool COUNTS>
__global__ __launch_bounds__(HY_THREADS) void hy_search_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ wat, long long n_w,
    const double *__restrict__ box, const int *__restrict__ cations, int n_c, double rc2, int cap, double cos_cut,
    double bin_w, int n_bins, long long n_tiles, long long n_chunks, long long n_blocks, int *__restrict__ idx,
    int *__restrict__ count, int *__restrict__ n_away, unsigned long long *__restrict__ hist)
{
    extern __shared__ unsigned long long s_hist[];
    if (COUNTS) {
        for (int b = threadIdx.x; b < n_bins; b += HY_THREADS) s_hist[b] = 0ull;
        __syncthreads();
    }
    for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const long long chunk = blk % n_chunks, rest = blk / n_chunks;
        const long long tile = rest % n_tiles, f = rest / n_tiles;
        const double *px = xyz + (size_t)f * 3 * (size_t)n, *py = px + n, *pz = py + n;
        const double *pw = wat + (size_t)f * 6 * (size_t)n_w;
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const int c0 = (int)tile * HY_TC;
        const int nc = n_c - c0 < HY_TC ? n_c - c0 : HY_TC;
        double cx[HY_TC], cy[HY_TC], cz[HY_TC];
#pragma unroll
        for (int k = 0; k < HY_TC; ++k) {
            const int ci = cations[k < nc ? c0 + k : c0];  // (a short last tile repeats its first cation; hits masked)
            cx[k] = px[ci];
            cy[k] = py[ci];
            cz[k] = pz[ci];
        }
        const long long w_end = (chunk + 1) * HY_CHUNK < n_w ? (chunk + 1) * HY_CHUNK : n_w;
        for (long long w = chunk * HY_CHUNK + threadIdx.x; w < w_end; w += HY_THREADS) {
            const double x = pw[w], y = pw[n_w + w], z = pw[2 * n_w + w];
            unsigned hits = 0;
#pragma unroll
            for (int k = 0; k < HY_TC; ++k)
                if (hy_rsq(cx[k], cy[k], cz[k], x, y, z, Lx, Ly, Lz) < rc2) hits |= 1u << k;
            hits &= (nc >= 32 ? ~0u : (1u << nc) - 1u);
            while (hits) {  // (rare: a few waters per cation in a whole frame)
                const int k = __builtin_ctz(hits);
                hits &= hits - 1u;
                const size_t row = (size_t)f * (size_t)n_c + (size_t)(c0 + k);
                if (COUNTS) {
                    const double c = hy_cos(cx[k], cy[k], cz[k], pw, n_w, w, Lx, Ly, Lz);
                    atomicAdd(&count[row], 1);
                    if (c < cos_cut) atomicAdd(&n_away[row], 1);
                    if (c == c) {
                        long long b = (long long)((c + 1.0) / bin_w);  // (truncates toward zero)
                        b = b < 0 ? 0 : (b >= n_bins ? n_bins - 1 : b);
                        atomicAdd(&s_hist[b], 1ull);
                    }
                } else {
                    const int slot = atomicAdd(&count[row], 1);
                    if (slot < cap) idx[row * (size_t)cap + (size_t)slot] = (int)w;
                }
            }
        }
    }
    if (COUNTS) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += HY_THREADS)
            if (s_hist[b]) atomicAdd(&hist[b], s_hist[b]);
    }
}

// One wave per row; LDS: the row [cap] (int).
__global__ __launch_bounds__(64) void hy_row_kernel(const double *__restrict__ xyz, long long n,
                                                    const double *__restrict__ wat, long long n_w,
                                                    const double *__restrict__ box, const int *__restrict__ cations,
                                                    int n_c, int *__restrict__ idx, const int *__restrict__ count,
                                                    double *__restrict__ cosv, long long n_rows, int cap)
{
    extern __shared__ int s_row[];
    const int lane = threadIdx.x;
    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const long long f = row / n_c;
        const int ci = cations[row % n_c];
        const double *px = xyz + (size_t)f * 3 * (size_t)n;
        const double *pw = wat + (size_t)f * 6 * (size_t)n_w;
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const double cx = px[ci], cy = px[n + ci], cz = px[2 * n + ci];
        int *r = idx + (size_t)row * (size_t)cap;
        double *o = cosv + (size_t)row * (size_t)cap;
        const int m = count[row] < cap ? count[row] : cap;
        __syncthreads();  // (the previous row's ranks have read s_row)
        for (int i = lane; i < m; i += 64) s_row[i] = r[i];
        __syncthreads();
        for (int i = lane; i < m; i += 64) {
            const int v = s_row[i];
            int rank = 0;
            for (int j = 0; j < m; ++j) rank += s_row[j] < v;
            r[rank] = v;
            o[rank] = hy_cos(cx, cy, cz, pw, n_w, v, Lx, Ly, Lz);
        }
        for (int i = m + lane; i < cap; i += 64) {
            r[i] = -1;
            o[i] = __builtin_nan("");
        }
    }
}

struct HyInputs {
    const double *xyz = nullptr, *box = nullptr;
    const int *cat = nullptr, *wat_idx = nullptr;
    double *wat = nullptr;
};

// What both entry points share: the checks and the staging of the inputs (no launch).
int hy_stage(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
             const double *box, int32_t n_cations, const int32_t *cations, int32_t n_waters, const int32_t *waters,
             HyInputs &in)
{
    MD_REQUIRE(n_atoms > 0, "cations without atoms");
    MD_REQUIRE(xyz && box && cations && (waters || n_waters == 0), "NULL array");
    MD_REQUIRE(n_atoms < (1ll << 31), "at most 2^31 - 1 atoms");
    for (int32_t c = 0; c < n_cations; ++c)
        MD_REQUIRE(cations[c] >= 0 && cations[c] < n_atoms, "cation %d: atom index %d out of range", (int)c,
                   (int)cations[c]);
    for (int32_t w = 0; w < n_waters; ++w)
        MD_REQUIRE(waters[w] >= 0 && (int64_t)waters[w] + 2 < n_atoms, "water %d: atoms %d..%d out of range", (int)w,
                   (int)waters[w], (int)waters[w] + 2);
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    in.xyz = (const double *)mdhip_stage(ctx, WS_XYZ_I, xyz, (size_t)n_frames * 3 * (size_t)n_atoms * 8,
                                         xyz_on_device, &rc);
    if (rc) return rc;
    MD_WS(d_box, double, WS_BOX, (size_t)n_frames * 3 * 8);
    if ((rc = mdhip_h2d_small(ctx, d_box, box, (size_t)n_frames * 3 * 8))) return rc;
    MD_WS(d_cat, int, WS_TYPE_I, (size_t)n_cations * 4);
    if ((rc = mdhip_h2d_small(ctx, d_cat, cations, (size_t)n_cations * 4))) return rc;
    in.box = d_box;
    in.cat = d_cat;
    if (n_waters == 0) return MDHIP_OK;
    MD_WS(d_widx, int, WS_TYPE_J, (size_t)n_waters * 4);
    if ((rc = mdhip_h2d_small(ctx, d_widx, waters, (size_t)n_waters * 4))) return rc;
    MD_WS(d_wat, double, WS_AUX1, (size_t)n_frames * 6 * (size_t)n_waters * 8);
    in.wat_idx = d_widx;
    in.wat = d_wat;
    return MDHIP_OK;
}

// Launches the water planes and the search (list or counts mode); the caller has zeroed the counters.
int hy_launch(mdhip_ctx *ctx, bool counts, int64_t n_frames, int64_t n_atoms, int32_t n_cations, int32_t n_waters,
              const HyInputs &in, double r_cut_sq, int32_t cap, double cos_cut, double bin_w, int32_t n_bins,
              int *d_idx, int *d_count, int *d_away, unsigned long long *d_hist)
{
    if (n_waters == 0) return MDHIP_OK;
    const size_t total = (size_t)n_frames * (size_t)n_waters;
    const unsigned wgrid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(hy_water_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, in.xyz, (long long)n_atoms,
                       in.wat_idx, (long long)n_waters, (long long)total, in.wat);
    MD_HIP(hipGetLastError());
    const long long n_tiles = (n_cations + HY_TC - 1) / HY_TC, n_chunks = (n_waters + HY_CHUNK - 1) / HY_CHUNK;
    const long long n_blocks = (long long)n_frames * n_tiles * n_chunks;
    const unsigned grid = (unsigned)std::min<long long>(n_blocks, (long long)ctx->cu_count * 64);
    if (counts)
        hipLaunchKernelGGL(hy_search_kernel<true>, dim3(grid), dim3(HY_THREADS), (size_t)n_bins * 8, ctx->stream,
                           in.xyz, (long long)n_atoms, in.wat, (long long)n_waters, in.box, in.cat, (int)n_cations,
                           r_cut_sq, (int)cap, cos_cut, bin_w, (int)n_bins, n_tiles, n_chunks, n_blocks, d_idx,
                           d_count, d_away, d_hist);
    else
        hipLaunchKernelGGL(hy_search_kernel<false>, dim3(grid), dim3(HY_THREADS), 0, ctx->stream, in.xyz,
                           (long long)n_atoms, in.wat, (long long)n_waters, in.box, in.cat, (int)n_cations, r_cut_sq,
                           (int)cap, cos_cut, bin_w, (int)n_bins, n_tiles, n_chunks, n_blocks, d_idx, d_count, d_away,
                           d_hist);
    MD_HIP(hipGetLastError());
    return MDHIP_OK;
}

}  // namespace

extern "C" {

int mdhip_hydration_cosines(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                            const double *box, int32_t n_cations, const int32_t *cations, int32_t n_waters,
                            const int32_t *waters, double r_cut_sq, int32_t cap, int32_t *idx, double *cosines,
                            int32_t *count)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_cations >= 0 && n_waters >= 0, "negative sizes");
    MD_REQUIRE(cap >= 1 && cap <= HY_MAX_CAP, "cap must be in [1, %d]", HY_MAX_CAP);
    if (n_frames == 0 || n_cations == 0) return cs.end();
    MD_REQUIRE(idx && cosines && count, "NULL array");
    HyInputs in;
    int rc;
    if ((rc = hy_stage(ctx, n_frames, n_atoms, xyz, xyz_on_device, box, n_cations, cations, n_waters, waters, in)))
        return rc;
    const size_t n_rows = (size_t)n_frames * (size_t)n_cations;
    MD_WS(d_count, int, WS_AUX0, n_rows * 4);
    MD_WS(d_idx, int, WS_OUT, n_rows * (size_t)cap * 4);
    MD_WS(d_cos, double, WS_OUT2, n_rows * (size_t)cap * 8);
    MD_HIP(hipMemsetAsync(d_count, 0, n_rows * 4, ctx->stream));
    KernelTimer timer(ctx, 3);
    ctx->last_kernel = "hy_search_kernel<false>";
    if ((rc = hy_launch(ctx, false, n_frames, n_atoms, n_cations, n_waters, in, r_cut_sq, cap, 0.0, 1.0, 1, d_idx,
                        d_count, nullptr, nullptr)))
        return rc;
    const unsigned row_grid = (unsigned)std::min<size_t>(n_rows, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(hy_row_kernel, dim3(row_grid), dim3(64), (size_t)cap * 4, ctx->stream, in.xyz,
                       (long long)n_atoms, in.wat, (long long)n_waters, in.box, in.cat, (int)n_cations, d_idx, d_count,
                       d_cos, (long long)n_rows, (int)cap);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, idx, d_idx, n_rows * (size_t)cap * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, cosines, d_cos, n_rows * (size_t)cap * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, count, d_count, n_rows * 4, 0))) return rc;
    cs.defer([timer]() {
        timer.collect();
        return MDHIP_OK;
    });
    return cs.end();
}

int mdhip_hydration_counts(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                           const double *box, int32_t n_cations, const int32_t *cations, int32_t n_waters,
                           const int32_t *waters, double r_cut_sq, double cos_cut, double bin_width, int32_t n_bins,
                           int32_t *n_water, int32_t *n_away, uint64_t *hist)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_cations >= 0 && n_waters >= 0, "negative sizes");
    MD_REQUIRE(n_bins >= 1 && n_bins <= HY_MAX_BINS, "n_bins must be in [1, %d]", HY_MAX_BINS);
    MD_REQUIRE(bin_width > 0.0, "bin_width must be positive");
    MD_REQUIRE(hist, "NULL array");
    memset(hist, 0, (size_t)n_bins * 8);
    if (n_frames == 0 || n_cations == 0) return cs.end();
    MD_REQUIRE(n_water && n_away, "NULL array");
    HyInputs in;
    int rc;
    if ((rc = hy_stage(ctx, n_frames, n_atoms, xyz, xyz_on_device, box, n_cations, cations, n_waters, waters, in)))
        return rc;
    const size_t n_rows = (size_t)n_frames * (size_t)n_cations;
    MD_WS(d_count, int, WS_AUX0, n_rows * 4);
    MD_WS(d_away, int, WS_AUX2, n_rows * 4);
    MD_WS(d_hist, unsigned long long, WS_HIST, (size_t)n_bins * 8);
    MD_HIP(hipMemsetAsync(d_count, 0, n_rows * 4, ctx->stream));
    MD_HIP(hipMemsetAsync(d_away, 0, n_rows * 4, ctx->stream));
    MD_HIP(hipMemsetAsync(d_hist, 0, (size_t)n_bins * 8, ctx->stream));
    KernelTimer timer(ctx, 2);
    ctx->last_kernel = "hy_search_kernel<true>";
    if ((rc = hy_launch(ctx, true, n_frames, n_atoms, n_cations, n_waters, in, r_cut_sq, 1, cos_cut, bin_width,
                        n_bins, nullptr, d_count, d_away, d_hist)))
        return rc;
    timer.stop();
    if ((rc = mdhip_result(cs, n_water, d_count, n_rows * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, n_away, d_away, n_rows * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, hist, d_hist, (size_t)n_bins * 8, 0))) return rc;
    cs.defer([timer]() {
        timer.collect();
        return MDHIP_OK;
    });
    return cs.end();
}

}  // extern "C"
