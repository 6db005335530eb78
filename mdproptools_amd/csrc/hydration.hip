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
//  2. hy_search_kernel<COUNTS>: the sweep of shell_search.h, every cation against the O of every water of its frame
//     (the |d| form of the wrap: the same rsq as d - sign(d) L). What a hit (rare) does:
//       list mode: the water index is appended to the row (frame, cation) (shell::append);
//       counts mode: the cosine is computed at once; n_water, n_away (cos < cos_cut) per row and an exact histogram
//         (bin trunc((cos + 1) / w) clamped to n_bins - 1, NaN in no bin) kept per block in LDS, added to the global
//         uint64 bins once per block.
//  3. hy_row_kernel (list mode): the row pass of shell_search.h, one wave per row, writes each water index and its
//     cosine at its rank: the waters in ascending molecule order, padded with -1 / NaN to `cap`.

#include <algorithm>
#include <type_traits>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_search.h"

namespace {

constexpr int HY_MAX_BINS = 4096;  // the counts pass keeps its histogram in LDS (32 KB)

// cosine of (cation - O, wrapped) and v of water w of the frame's planes p (ox oy oz vx vy vz, each n_w long)
__device__ __noinline__ double hy_cos(double cx, double cy, double cz, const double *__restrict__ p, long long n_w,
                                      long long w, double Lx, double Ly, double Lz)
{
    const double dx = shell::wrap_signed(cx - p[w], Lx);
    const double dy = shell::wrap_signed(cy - p[n_w + w], Ly);
    const double dz = shell::wrap_signed(cz - p[2 * n_w + w], Lz);
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

// what a mode of the search writes
struct HyList {
    int cap;
    int *idx, *count;
};
struct HyCounts {
    double cos_cut, bin_w;
    int n_bins;
    int *count, *n_away;
    unsigned long long *hist;
};

template <bool COUNTS>
__global__ __launch_bounds__(shell::THREADS) void hy_search_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ wat, long long n_w,
    const double *__restrict__ box, const int *__restrict__ cations, int n_c, double rc2, shell::Grid g,
    std::conditional_t<COUNTS, HyCounts, HyList> o)
{
    extern __shared__ unsigned long long s_hist[];
    if constexpr (COUNTS) {
        for (int b = threadIdx.x; b < o.n_bins; b += shell::THREADS) s_hist[b] = 0ull;
        __syncthreads();
    }
    shell::sweep(xyz, n, cations, n_c, wat, 6, n_w, box, rc2, g,
                 [=](const shell::Row &r, size_t row, long long w) {
                     if constexpr (COUNTS) {
                         const double c = hy_cos(r.cx, r.cy, r.cz, wat + (size_t)r.f * 6 * (size_t)n_w, n_w, w, r.Lx,
                                                 r.Ly, r.Lz);
                         atomicAdd(&o.count[row], 1);
                         if (c < o.cos_cut) atomicAdd(&o.n_away[row], 1);
                         if (c == c) {
                             long long b = (long long)((c + 1.0) / o.bin_w);  // (truncates toward zero)
                             b = b < 0 ? 0 : (b >= o.n_bins ? o.n_bins - 1 : b);
                             atomicAdd(&s_hist[b], 1ull);
                         }
                     } else {
                         shell::append(o.count, o.idx, row, o.cap, (int)w);
                     }
                 });
    if constexpr (COUNTS) {
        __syncthreads();
        for (int b = threadIdx.x; b < o.n_bins; b += shell::THREADS)
            if (s_hist[b]) atomicAdd(&o.hist[b], s_hist[b]);
    }
}

// One wave per row; LDS: the row [cap] (int).
__global__ __launch_bounds__(64) void hy_row_kernel(const double *__restrict__ xyz, long long n,
                                                    const double *__restrict__ wat, long long n_w,
                                                    const double *__restrict__ box, const int *__restrict__ cations,
                                                    int n_c, int *__restrict__ idx, const int *__restrict__ count,
                                                    double *__restrict__ cosv, long long n_rows, int cap)
{
    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const shell::Row c = shell::row_of(xyz, n, box, cations, row / n_c, (int)(row % n_c));
        const double *pw = wat + (size_t)c.f * 6 * (size_t)n_w;
        int *r = idx + (size_t)row * (size_t)cap;
        double *o = cosv + (size_t)row * (size_t)cap;
        shell::rank_row(
            r, count[row], cap,
            [&](int rank, int v) {
                r[rank] = v;
                o[rank] = hy_cos(c.cx, c.cy, c.cz, pw, n_w, v, c.Lx, c.Ly, c.Lz);
            },
            [&](int i) {
                r[i] = -1;
                o[i] = __builtin_nan("");
            });
    }
}

struct HyInputs : shell::Inputs {
    const int *wat_idx = nullptr;
    double *wat = nullptr;
};

// What both entry points share: the checks and the staging of the inputs (no launch).
int hy_stage(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
             const double *box, int32_t n_cations, const int32_t *cations, int32_t n_waters, const int32_t *waters,
             HyInputs &in)
{
    int rc;
    if ((rc = shell::stage(ctx, "cation", n_frames, n_atoms, xyz, xyz_on_device, box, n_cations, cations, in)))
        return rc;
    MD_REQUIRE(waters || n_waters == 0, "NULL array");
    if ((rc = shell::check_indices(ctx, "water", n_waters, waters, 3, n_atoms))) return rc;
    if (n_waters == 0) return MDHIP_OK;
    MD_WS(d_widx, int, WS_TYPE_J, (size_t)n_waters * 4);
    if ((rc = mdhip_h2d_small(ctx, d_widx, waters, (size_t)n_waters * 4))) return rc;
    MD_WS(d_wat, double, WS_AUX1, (size_t)n_frames * 6 * (size_t)n_waters * 8);
    in.wat_idx = d_widx;
    in.wat = d_wat;
    return MDHIP_OK;
}

// Launches the water planes and the search (two launches); the caller has zeroed the counters. `lds`: the search's.
template <bool COUNTS, class Out>
int hy_launch(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, int32_t n_cations, int32_t n_waters,
              const HyInputs &in, double r_cut_sq, size_t lds, const Out &out)
{
    if (n_waters == 0) return MDHIP_OK;
    const size_t total = (size_t)n_frames * (size_t)n_waters;
    const unsigned wgrid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(hy_water_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, in.xyz, (long long)n_atoms,
                       in.wat_idx, (long long)n_waters, (long long)total, in.wat);
    MD_HIP(hipGetLastError());
    const shell::Grid g = shell::sweep_grid(ctx, n_frames, n_cations, n_waters);
    hipLaunchKernelGGL(hy_search_kernel<COUNTS>, dim3(g.grid), dim3(shell::THREADS), lds, ctx->stream, in.xyz,
                       (long long)n_atoms, in.wat, (long long)n_waters, in.box, in.centres, (int)n_cations, r_cut_sq,
                       g, out);
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
    shell::RowSet rs;
    int rc;
    if ((rc = shell::take_rows(ctx, n_frames, n_cations, cap, shell::MAX_CAP, rs))) return rc;
    if (rs.n_rows == 0) return cs.end();
    MD_REQUIRE(idx && cosines && count, "NULL array");
    HyInputs in;
    if ((rc = hy_stage(ctx, n_frames, n_atoms, xyz, xyz_on_device, box, n_cations, cations, n_waters, waters, in)))
        return rc;
    MD_WS(d_cos, double, WS_OUT2, rs.n_rows * (size_t)cap * 8);
    KernelTimer timer(ctx, 3);
    ctx->last_kernel = "hy_search_kernel<false>";
    if ((rc = hy_launch<false>(ctx, n_frames, n_atoms, n_cations, n_waters, in, r_cut_sq, 0,
                               HyList{(int)cap, rs.idx, rs.count})))
        return rc;
    hipLaunchKernelGGL(hy_row_kernel, dim3(rs.grid(ctx, 32)), dim3(64), (size_t)cap * 4, ctx->stream, in.xyz,
                       (long long)n_atoms, in.wat, (long long)n_waters, in.box, in.centres, (int)n_cations, rs.idx, rs.count,
                       d_cos, (long long)rs.n_rows, (int)cap);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, cosines, d_cos, rs.n_rows * (size_t)cap * 8, 0))) return rc;
    if ((rc = shell::row_results(cs, rs, idx, count))) return rc;
    return shell::finish(cs, timer);
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
    if ((rc = hy_launch<true>(ctx, n_frames, n_atoms, n_cations, n_waters, in, r_cut_sq, (size_t)n_bins * 8,
                              HyCounts{cos_cut, bin_width, (int)n_bins, d_count, d_away, d_hist})))
        return rc;
    timer.stop();
    if ((rc = mdhip_result(cs, n_water, d_count, n_rows * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, n_away, d_away, n_rows * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, hist, d_hist, (size_t)n_bins * 8, 0))) return rc;
    return shell::finish(cs, timer);
}

}  // extern "C"
