// density.hip — per-frame atom counts along one axis, measured from a surface: the hot loop of
// number_density.calc_number_density and of calc_density_profile.
//
// Replaces the per-type pandas selections and the Python `rho_part[i][k] += 1` loop of structural/number_density.py:
// 76-105 of the reference. Per frame, from the axis coordinate x [N] and a 16-bit code per atom (row field: which
// row of the result the atom counts in, or none; surface bit: the atom belongs to the surface):
//   lo, hi = min, max of x over the surface atoms (NaN coordinates skipped as pandas' min / max skip them; NaN, NaN
//            without one; -0.0 orders below +0.0 so that the pair does not depend on the reduction order)
//   REF_POS: s = x - lo; atoms with s < d:  b = s - (hi - lo)        number_density.py:87-96
//   REF_NEG: s = x - lo; atoms with s > d:  b = s                    number_density.py:97-105
//            k = trunc(b / w); -n_bins <= k < 0 counts in bin k + n_bins (the reference's Python indexing), k outside
//            [-n_bins, n_bins) counts in outside[f] and in no bin (the reference raises IndexError there)
//   PROFILE: s = x - origin (lo, hi or a value per frame); t = (s - s_lo) / w; bin trunc(t) when 0 <= t and
//            trunc(t) < n_bins, else outside[f] (NaN included); nothing wraps
// All in float64 with contraction off and true division: the bin index is numpy's. Counts are integers: every output
// is exact and independent of the launch geometry.
//
// Both passes (extent, then binning) need the frame's plane, and it should cross the memory fabric once:
//   frames of up to AP_CHUNK = 16 384 atoms: ap_frame_kernel, one workgroup per frame (64 .. 1024 threads), AP_ITEMS
//     atoms per lane held in registers between the passes, every load issued before the first use; the frame's
//     histogram lives in LDS and is STORED to the result (no atomics, no memset), or, when n_rows * n_bins exceeds
//     AP_LDS_WORDS, is added straight to the zeroed result in global memory;
//   larger frames: ap_extent_kernel (a partial extent per chunk of the frame; it loads the coordinates only where a
//     lane holds a surface atom) and ap_chunk_kernel (every workgroup folds its frame's partials, bins its chunk
//     into LDS and adds the non-zero bins to the zeroed result), launched for groups of frames of at most
//     AP_GROUP_BYTES, which the Infinity Cache holds between the two launches.
// Measured: DESIGN.md 4.10.

#include <algorithm>
#include <cmath>
#include <limits>

#include "ctx.h"

#pragma clang fp contract(off)

namespace {

constexpr int AP_ITEMS = 16;
constexpr int AP_THREADS = 1024;
constexpr int AP_CHUNK = AP_ITEMS * AP_THREADS;
constexpr int AP_BATCH = 8;  // split path: atoms per lane whose loads are in flight together
constexpr int AP_FRAME_WAVES = 5;  // waves per SIMD the one-workgroup kernel is compiled for (96 VGPRs): two workgroups of
                                 // up to 640 threads (10 240 atoms) share a CU, one loads while the other bins
constexpr int AP_LDS_WORDS = 15360;                 // 60 KB of uint32 bins per workgroup (two workgroups per CU)
constexpr size_t AP_GROUP_BYTES = (size_t)128 << 20;  // coordinate bytes between a frame's two passes (split path)
constexpr unsigned AP_SURFACE = MDHIP_AP_SURFACE, AP_ROW = MDHIP_AP_NONE;

struct ApParams {
    double bin_size;
    double dist;  // REF_*: dist_from_interface; PROFILE: s_lo
    int n_bins, n_rows;
    int origin_kind;  // PROFILE: 0 lo, 1 hi, 2 origin[f]
    int hist_lds;     // the frame's n_rows * n_bins words fit LDS
};

struct ApExtent {
    double lo, hi;  // +inf, -inf: no surface atom yet
};

__device__ __forceinline__ double ap_min(double a, double b)
{
    return (b < a || (b == a && __builtin_signbit(b))) ? b : a;
}
__device__ __forceinline__ double ap_max(double a, double b)
{
    return (b > a || (b == a && !__builtin_signbit(b))) ? b : a;
}

// The workgroup's extent (every lane gets it). s_red: 2 doubles per wave. One barrier inside, none after the reads.
__device__ __forceinline__ ApExtent ap_block_extent(ApExtent e, double *s_red)
{
    for (int o = 32; o; o >>= 1) {
        e.lo = ap_min(e.lo, __shfl_xor(e.lo, o));
        e.hi = ap_max(e.hi, __shfl_xor(e.hi, o));
    }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_red[2 * w] = e.lo;
        s_red[2 * w + 1] = e.hi;
    }
    __syncthreads();
    ApExtent r = {s_red[0], s_red[1]};
    for (int k = 1; k < nw; ++k) {
        r.lo = ap_min(r.lo, s_red[2 * k]);
        r.hi = ap_max(r.hi, s_red[2 * k + 1]);
    }
    if (r.lo > r.hi) r.lo = r.hi = __builtin_nan("");  // no surface atom
    return r;
}

// One atom into the frame's histogram (s_hist in LDS or g_hist in global memory); atoms without a bin into n_out.
template <int MODE>
__device__ __forceinline__ void ap_bin(double x, unsigned code, double lo, double range, double origin,
                                       const ApParams &p, unsigned *s_hist, unsigned *__restrict__ g_hist,
                                       unsigned &n_out)
{
    const unsigned row = code & AP_ROW;
    if (row >= (unsigned)p.n_rows) return;
    const double nb = (double)p.n_bins;
    int k;
    if constexpr (MODE == MDHIP_AP_PROFILE) {
        const double s = x - origin;
        const double t = (s - p.dist) / p.bin_size;
        if (!(t >= 0.0 && t < nb)) {
            ++n_out;
            return;
        }
        k = (int)t;
    } else {
        const double s = x - lo;
        double b;
        if constexpr (MODE == MDHIP_AP_REF_POS) {
            if (!(s < p.dist)) return;
            b = s - range;
        } else {
            if (!(s > p.dist)) return;
            b = s;
        }
        const double q = b / p.bin_size;
        if (!(q < nb && q > -(nb + 1.0))) {  // trunc(q) outside [-n_bins, n_bins)
            ++n_out;
            return;
        }
        k = (int)q;  // (truncates toward zero)
        if (k < 0) k += p.n_bins;
    }
    const size_t w = (size_t)row * (size_t)p.n_bins + (size_t)k;
    if (p.hist_lds)
        atomicAdd(&s_hist[w], 1u);
    else
        atomicAdd(&g_hist[w], 1u);
}

__device__ __forceinline__ double ap_origin(const ApParams &p, const ApExtent &e, const double *origin, long long f)
{
    return p.origin_kind == 0 ? e.lo : (p.origin_kind == 1 ? e.hi : origin[f]);
}

// One workgroup per frame of at most AP_ITEMS * blockDim.x atoms. LDS: the frame's histogram when p.hist_lds.
template <int MODE>
__global__ __launch_bounds__(AP_THREADS, AP_FRAME_WAVES) void ap_frame_kernel(const double *__restrict__ x, long long n,
                                                             const unsigned short *__restrict__ codes,
                                                             long long code_stride,
                                                             const double *__restrict__ origin, ApParams p,
                                                             unsigned *__restrict__ counts,
                                                             double *__restrict__ extent,
                                                             unsigned *__restrict__ outside)
{
    extern __shared__ unsigned s_hist[];
    __shared__ double s_red[2 * AP_THREADS / 64];
    __shared__ unsigned s_out;
    const int words = p.n_rows * p.n_bins;
    const long long f = blockIdx.x;
    const double *px = x + (size_t)f * (size_t)n;
    const unsigned short *pc = codes + (size_t)f * (size_t)code_stride;
    double xv[AP_ITEMS];
    unsigned cv[AP_ITEMS];
    // every load is issued before the first use: lanes past the end read the last atom and drop it
#pragma unroll
    for (int k = 0; k < AP_ITEMS; ++k) {
        const int i = k * (int)blockDim.x + (int)threadIdx.x;  // (< AP_CHUNK: 32-bit offsets from a uniform base)
        const int ii = i < (int)n ? i : (int)n - 1;
        xv[k] = px[ii];
        cv[k] = pc[ii];
    }
    ApExtent e = {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
#pragma unroll
    for (int k = 0; k < AP_ITEMS; ++k) {
        if (k * (int)blockDim.x + (int)threadIdx.x >= (int)n) cv[k] = AP_ROW;
        const bool surf = (cv[k] & AP_SURFACE) != 0;
        e.lo = surf ? ap_min(e.lo, xv[k]) : e.lo;
        e.hi = surf ? ap_max(e.hi, xv[k]) : e.hi;
    }
    if (p.hist_lds)
        for (int w = threadIdx.x; w < words; w += blockDim.x) s_hist[w] = 0u;
    if (threadIdx.x == 0) s_out = 0u;
    e = ap_block_extent(e, s_red);
    const double range = e.hi - e.lo, org = ap_origin(p, e, origin, f);
    unsigned *g_hist = counts + (size_t)f * (size_t)words;
    unsigned n_out = 0;
#pragma unroll
    for (int k = 0; k < AP_ITEMS; ++k) ap_bin<MODE>(xv[k], cv[k], e.lo, range, org, p, s_hist, g_hist, n_out);
    if (n_out) atomicAdd(&s_out, n_out);
    __syncthreads();
    if (p.hist_lds)
        for (int w = threadIdx.x; w < words; w += blockDim.x) g_hist[w] = s_hist[w];
    if (threadIdx.x == 0) {
        extent[2 * f] = e.lo;
        extent[2 * f + 1] = e.hi;
        outside[f] = s_out;
    }
}

// Split path, first launch: block b = (frame b / n_chunks, chunk b % n_chunks) -> partial[b] = its chunk's extent.
__global__ __launch_bounds__(AP_THREADS) void ap_extent_kernel(const double *__restrict__ x, long long n,
                                                              const unsigned short *__restrict__ codes,
                                                              long long code_stride, long long n_chunks,
                                                              long long chunk, double *__restrict__ partial)
{
    __shared__ double s_red[2 * AP_THREADS / 64];
    const long long f = blockIdx.x / n_chunks, c = blockIdx.x % n_chunks;
    const double *px = x + (size_t)f * (size_t)n;
    const unsigned short *pc = codes + (size_t)f * (size_t)code_stride;
    const long long i1 = (c + 1) * chunk < n ? (c + 1) * chunk : n;
    ApExtent e = {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
    // AP_BATCH atoms per lane at a time: the codes first (lanes past the end re-read the last atom and drop it), the
    // coordinates only where one of them is a surface atom, every load of a kind issued before the first use
    for (long long base = c * chunk; base < i1; base += (long long)AP_BATCH * AP_THREADS) {
        unsigned cv[AP_BATCH], any = 0;
#pragma unroll
        for (int u = 0; u < AP_BATCH; ++u) {
            const long long i = base + (long long)u * AP_THREADS + threadIdx.x;
            cv[u] = pc[i < i1 ? i : i1 - 1];
        }
#pragma unroll
        for (int u = 0; u < AP_BATCH; ++u) {
            if (base + (long long)u * AP_THREADS + threadIdx.x >= i1) cv[u] = AP_ROW;
            any |= cv[u];
        }
        if (any & AP_SURFACE) {
            double xv[AP_BATCH];
#pragma unroll
            for (int u = 0; u < AP_BATCH; ++u) {
                const long long i = base + (long long)u * AP_THREADS + threadIdx.x;
                xv[u] = px[i < i1 ? i : i1 - 1];
            }
#pragma unroll
            for (int u = 0; u < AP_BATCH; ++u) {
                const bool surf = (cv[u] & AP_SURFACE) != 0;
                e.lo = surf ? ap_min(e.lo, xv[u]) : e.lo;
                e.hi = surf ? ap_max(e.hi, xv[u]) : e.hi;
            }
        }
    }
    e = ap_block_extent(e, s_red);  // (NaN, NaN for a chunk without surface atoms: ap_min / ap_max skip them)
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = e.lo;
        partial[2 * (size_t)blockIdx.x + 1] = e.hi;
    }
}

// Split path, second launch (same block -> (frame, chunk) map): counts and outside were zeroed by the caller.
template <int MODE>
__global__ __launch_bounds__(AP_THREADS) void ap_chunk_kernel(const double *__restrict__ x, long long n,
                                                             const unsigned short *__restrict__ codes,
                                                             long long code_stride,
                                                             const double *__restrict__ origin, ApParams p,
                                                             long long n_chunks, long long chunk,
                                                             const double *__restrict__ partial,
                                                             unsigned *__restrict__ counts,
                                                             double *__restrict__ extent,
                                                             unsigned *__restrict__ outside)
{
    extern __shared__ unsigned s_hist[];
    __shared__ double s_red[2 * AP_THREADS / 64];
    __shared__ unsigned s_out;
    const int words = p.n_rows * p.n_bins;
    const long long f = blockIdx.x / n_chunks, c = blockIdx.x % n_chunks;
    ApExtent e = {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
    for (long long k = threadIdx.x; k < n_chunks; k += AP_THREADS) {
        e.lo = ap_min(e.lo, partial[2 * (size_t)(f * n_chunks + k)]);
        e.hi = ap_max(e.hi, partial[2 * (size_t)(f * n_chunks + k) + 1]);
    }
    if (p.hist_lds)
        for (int w = threadIdx.x; w < words; w += AP_THREADS) s_hist[w] = 0u;
    if (threadIdx.x == 0) s_out = 0u;
    e = ap_block_extent(e, s_red);
    const double range = e.hi - e.lo, org = ap_origin(p, e, origin, f);
    const double *px = x + (size_t)f * (size_t)n;
    const unsigned short *pc = codes + (size_t)f * (size_t)code_stride;
    unsigned *g_hist = counts + (size_t)f * (size_t)words;
    const long long i1 = (c + 1) * chunk < n ? (c + 1) * chunk : n;
    unsigned n_out = 0;
    for (long long base = c * chunk; base < i1; base += (long long)AP_BATCH * AP_THREADS) {
        double xv[AP_BATCH];
        unsigned cv[AP_BATCH];
#pragma unroll
        for (int u = 0; u < AP_BATCH; ++u) {  // (every load before the first use; past the end: the last atom, dropped)
            const long long i = base + (long long)u * AP_THREADS + threadIdx.x;
            xv[u] = px[i < i1 ? i : i1 - 1];
            cv[u] = pc[i < i1 ? i : i1 - 1];
        }
#pragma unroll
        for (int u = 0; u < AP_BATCH; ++u) {
            if (base + (long long)u * AP_THREADS + threadIdx.x >= i1) cv[u] = AP_ROW;
            ap_bin<MODE>(xv[u], cv[u], e.lo, range, org, p, s_hist, g_hist, n_out);
        }
    }
    if (n_out) atomicAdd(&s_out, n_out);
    __syncthreads();
    if (p.hist_lds)
        for (int w = threadIdx.x; w < words; w += AP_THREADS) {
            const unsigned v = s_hist[w];
            if (v) atomicAdd(&g_hist[w], v);
        }
    if (threadIdx.x == 0) {
        if (c == 0) {
            extent[2 * f] = e.lo;
            extent[2 * f + 1] = e.hi;
        }
        if (s_out) atomicAdd(&outside[f], s_out);
    }
}

template <int MODE>
int ap_launch(mdhip_ctx *ctx, int64_t n_frames, int64_t n, const double *d_x, const unsigned short *d_codes,
              long long code_stride, const double *d_origin, const ApParams &p, unsigned *d_counts, double *d_extent,
              unsigned *d_outside)
{
    const size_t words = (size_t)p.n_rows * (size_t)p.n_bins;
    const size_t lds = p.hist_lds ? words * 4 : 0;
    if (n <= AP_CHUNK) {
        const int threads = (int)std::min<int64_t>(AP_THREADS, std::max<int64_t>(64, ((n + AP_ITEMS - 1) / AP_ITEMS + 63) / 64 * 64));
        const unsigned grid = (unsigned)n_frames;  // (one workgroup per frame: checked below 2^31 by the caller)
        ctx->last_kernel = "ap_frame_kernel";
        ctx->last_launches = 1;
        hipLaunchKernelGGL(ap_frame_kernel<MODE>, dim3(grid), dim3(threads), lds, ctx->stream, d_x, (long long)n,
                           d_codes, code_stride, d_origin, p, d_counts, d_extent, d_outside);
        MD_HIP(hipGetLastError());
        return MDHIP_OK;
    }
    const long long chunk = AP_CHUNK, n_chunks = (n + chunk - 1) / chunk;
    const int64_t per_group = std::max<int64_t>(1, (int64_t)(AP_GROUP_BYTES / ((size_t)n * 8)));
    MD_WS(d_part, double, WS_PART, (size_t)std::min(per_group, n_frames) * (size_t)n_chunks * 16);
    ctx->last_kernel = "ap_chunk_kernel";
    ctx->last_launches = 0;
    for (int64_t f0 = 0; f0 < n_frames; f0 += per_group) {
        const int64_t nf = std::min(per_group, n_frames - f0);
        const unsigned grid = (unsigned)(nf * n_chunks);  // (about 128 MiB / 128 KiB chunks, or one frame's: < 2^17)
        const double *gx = d_x + (size_t)f0 * (size_t)n;
        const unsigned short *gc = d_codes + (size_t)f0 * (size_t)code_stride;
        hipLaunchKernelGGL(ap_extent_kernel, dim3(grid), dim3(AP_THREADS), 0, ctx->stream, gx, (long long)n, gc,
                           code_stride, n_chunks, chunk, d_part);
        MD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ap_chunk_kernel<MODE>, dim3(grid), dim3(AP_THREADS), lds, ctx->stream, gx, (long long)n,
                           gc, code_stride, d_origin ? d_origin + f0 : nullptr, p, n_chunks, chunk, d_part,
                           d_counts + (size_t)f0 * words, d_extent + 2 * (size_t)f0, d_outside + (size_t)f0);
        MD_HIP(hipGetLastError());
        ctx->last_launches += 2;
    }
    return MDHIP_OK;
}

}  // namespace

extern "C" {

int mdhip_axis_profile(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                       const uint16_t *codes, int codes_per_frame, int32_t n_rows, int mode, double bin_size,
                       double dist, int32_t n_bins, int origin_kind, const double *origin, uint32_t *counts,
                       double *extent, uint32_t *outside)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0, "negative sizes");
    MD_REQUIRE(n_atoms < (1ll << 31), "at most 2^31 - 1 atoms");
    MD_REQUIRE(mode == MDHIP_AP_REF_POS || mode == MDHIP_AP_REF_NEG || mode == MDHIP_AP_PROFILE, "unknown mode %d",
               mode);
    MD_REQUIRE(n_rows >= 1 && n_rows < (int32_t)MDHIP_AP_NONE, "n_rows must be in [1, %d]", (int)MDHIP_AP_NONE - 1);
    MD_REQUIRE(n_bins >= 1 && (int64_t)n_rows * n_bins < (1ll << 31), "n_bins must be positive, n_rows * n_bins < 2^31");
    MD_REQUIRE(bin_size > 0.0, "bin_size must be positive");
    MD_REQUIRE(dist == dist, "the distance is NaN");
    const bool given = mode == MDHIP_AP_PROFILE && origin_kind == 2;
    MD_REQUIRE(mode != MDHIP_AP_PROFILE || (origin_kind >= 0 && origin_kind <= 2), "origin_kind must be 0, 1 or 2");
    MD_REQUIRE(!given || origin, "origin_kind 2 needs an origin per frame");
    if (n_frames == 0) return cs.end();
    MD_REQUIRE(counts && extent && outside, "NULL array");
    const size_t words = (size_t)n_rows * (size_t)n_bins;
    MD_REQUIRE((size_t)n_frames * words < ((size_t)1 << 40), "result too large");
    if (n_atoms == 0) {
        memset(counts, 0, (size_t)n_frames * words * 4);
        memset(outside, 0, (size_t)n_frames * 4);
        for (int64_t i = 0; i < 2 * n_frames; ++i) extent[i] = std::numeric_limits<double>::quiet_NaN();
        return cs.end();
    }
    MD_REQUIRE(x && codes, "NULL array");
    MD_REQUIRE((n_frames * ((n_atoms + AP_CHUNK - 1) / AP_CHUNK)) < (1ll << 31), "too many frames of this size");
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const double *d_x =
        (const double *)mdhip_stage(ctx, WS_XYZ_I, x, (size_t)n_frames * (size_t)n_atoms * 8, x_on_device, &rc);
    if (rc) return rc;
    const size_t code_bytes = (size_t)(codes_per_frame ? n_frames : 1) * (size_t)n_atoms * 2;
    MD_WS(d_codes, unsigned short, WS_TYPE_I, code_bytes);
    if (code_bytes <= MD_SMALL_COPY_MAX) {
        if ((rc = mdhip_h2d_small(ctx, d_codes, codes, code_bytes))) return rc;
    } else {
        MD_HIP(hipMemcpyAsync(d_codes, codes, code_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    const double *d_origin = nullptr;
    if (given) {
        MD_WS(d_org, double, WS_AUX0, (size_t)n_frames * 8);
        if ((size_t)n_frames * 8 <= MD_SMALL_COPY_MAX) {
            if ((rc = mdhip_h2d_small(ctx, d_org, origin, (size_t)n_frames * 8))) return rc;
        } else {
            MD_HIP(hipMemcpyAsync(d_org, origin, (size_t)n_frames * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        d_origin = d_org;
    }
    MD_WS(d_counts, unsigned, WS_HIST, (size_t)n_frames * words * 4);
    MD_WS(d_extent, double, WS_OUT, (size_t)n_frames * 16);
    MD_WS(d_outside, unsigned, WS_MISC, (size_t)n_frames * 4);
    ApParams p;
    p.bin_size = bin_size;
    p.dist = dist;
    p.n_bins = n_bins;
    p.n_rows = n_rows;
    p.origin_kind = mode == MDHIP_AP_PROFILE ? origin_kind : 0;
    p.hist_lds = words <= (size_t)AP_LDS_WORDS;
    const bool split = n_atoms > AP_CHUNK;
    KernelTimer timer(ctx, 1);  // (the zeroing the launches need is part of the call's device time)
    if (split || !p.hist_lds) MD_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_frames * words * 4, ctx->stream));
    if (split) MD_HIP(hipMemsetAsync(d_outside, 0, (size_t)n_frames * 4, ctx->stream));
    const long long stride = codes_per_frame ? (long long)n_atoms : 0;
    switch (mode) {
    case MDHIP_AP_REF_POS:
        rc = ap_launch<MDHIP_AP_REF_POS>(ctx, n_frames, n_atoms, d_x, d_codes, stride, d_origin, p, d_counts, d_extent,
                                         d_outside);
        break;
    case MDHIP_AP_REF_NEG:
        rc = ap_launch<MDHIP_AP_REF_NEG>(ctx, n_frames, n_atoms, d_x, d_codes, stride, d_origin, p, d_counts, d_extent,
                                         d_outside);
        break;
    default:
        rc = ap_launch<MDHIP_AP_PROFILE>(ctx, n_frames, n_atoms, d_x, d_codes, stride, d_origin, p, d_counts, d_extent,
                                         d_outside);
    }
    if (rc) return rc;
    timer.stop();
    if ((rc = mdhip_result(cs, counts, d_counts, (size_t)n_frames * words * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, extent, d_extent, (size_t)n_frames * 16, 0))) return rc;
    if ((rc = mdhip_result(cs, outside, d_outside, (size_t)n_frames * 4, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
