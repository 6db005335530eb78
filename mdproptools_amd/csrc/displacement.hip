// displacement.hip — histogram of the distance every entity travels over a fixed lag, over all time origins: the hot
// loop of Displacement.calc_dist / calc_van_hove (the self part of the van Hove function, G_s(r, t)).
//
// The reference's Displacement.calc_dist (dynamical/residence_time.py:211-254) is unfinished: it collects the WRAPPED
// x y z of the chosen atom types per frame and stops; the sketch behind it groups the frames into windows of one
// residence time. Here, for coordinates r [F][3][E] and jobs (group g, lag k, stride s):
//   image counts (box given: wrapped coordinates), per entity and axis: n(0) = 0, n(f) = n(f-1) - 1 when
//     d = x(f) - x(f-1) > L(f)/2, + 1 when d < -L(f)/2 (strict: the reference's single wrap, rdf_cn.py:44-57; a NaN
//     shifts nothing); xu(f) = x(f) + (double)n(f) * L(f), one product and one sum, unfused;
//   per origin t0 = 0, s, 2s, ... (t0 + k <= F - 1) and entity of g: d = xu(t0 + k) - xu(t0),
//     rsq = (dx dx + dy dy) + dz dz unfused, bin = trunc(sqrt(rsq) / bin_size) by comparison of rsq with the exact
//     edge table (mdhip_bin_edges), counted in hist[job][bin] when bin < nbins, else (NaN included) in overflow[job];
//   moments[job] = sum sqrt(rsq), sum rsq, sum rsq rsq over all windows of the job.
//
// The image counts are image_counts.h (three launches, shared with relaxation.hip): integers, the same whatever the
// chunking.
//
// Binning is one launch for all jobs (blockIdx.y = job, blockIdx.x = a run of `wpb` consecutive windows of the job,
// window w = origin * group size + entity, so that lanes run along the entities and small groups still fill a wave):
// a uint32 row per workgroup in LDS with LDS atomics when nbins <= DP_LDS_WORDS (wpb < 2^32, so no counter can wrap),
// flushed with 64-bit integer atomics; larger rows take the 64-bit atomics on the global row directly. Every
// workgroup writes its three partial moments (lane sums in window order, a fixed butterfly, the waves in order);
// dp_moment_kernel adds a job's partials in a fixed order. No float atomics: integers are exact and independent of
// the launch geometry, moments are reproducible for a given geometry. Measured: DESIGN.md 4.12.

#include "group_pairs.h"  // (its three argument checks; the kernels and the plan here are this file's own)
#include "image_counts.h"

#pragma clang fp contract(off)

namespace {

constexpr int DP_LDS_WORDS = 16128;    // uint32 bins of a job's row in LDS (63 KiB; 64 KiB per workgroup is the limit)
constexpr long long DP_MIN_WPB = 2048;  // windows per workgroup: at least 8 per lane ...
constexpr long long DP_BLOCKS = 4096;   // ... and at most this many workgroups per job

struct DpJob {
    long long e0, ng;     // the group's entities [e0, e0 + ng)
    long long n_win;      // origins * ng
    long long wpb, nblk;  // windows per workgroup, workgroups
    long long part0;      // first partial-moment slot of the job
    int lag, stride;
    int q, r;             // DP_THREADS = q * ng + r
};

// Block (x, y): windows [x * wpb, (x + 1) * wpb) of job job0 + y. Dynamic LDS: the job's row when LDS.
template <bool WRAP, bool LDS>
__global__ __launch_bounds__(DP_THREADS) void dp_bin_kernel(const double *__restrict__ r, const int *__restrict__ img,
                                                            const double *__restrict__ box, long long E,
                                                            const DpJob *__restrict__ jobs, int job0,
                                                            const double *__restrict__ edges, float gscale, int nbins,
                                                            unsigned long long *__restrict__ hist,
                                                            unsigned long long *__restrict__ overflow,
                                                            double *__restrict__ part)
{
    extern __shared__ unsigned s_hist[];
    __shared__ double s_red[3 * DP_THREADS / 64];
    __shared__ unsigned s_ovf;
    const int job = job0 + (int)blockIdx.y;
    const DpJob J = jobs[job];
    if ((long long)blockIdx.x >= J.nblk) return;  // (the whole workgroup: jobs of one launch differ in size)
    if (LDS)
        for (int w = threadIdx.x; w < nbins; w += DP_THREADS) s_hist[w] = 0u;
    if (threadIdx.x == 0) s_ovf = 0u;
    __syncthreads();
    unsigned long long *g_row = hist + (size_t)job * (size_t)nbins;
    const long long ncol = 3 * E;
    const long long w0 = (long long)blockIdx.x * J.wpb;
    const long long w1 = w0 + J.wpb < J.n_win ? w0 + J.wpb : J.n_win;
    const double top = edges[nbins];
    long long w = w0 + threadIdx.x;
    long long o = w / J.ng, e = w - o * J.ng;
    double s1 = 0.0, s2 = 0.0, s4 = 0.0;
    unsigned n_ovf = 0;
    for (; w < w1; w += DP_THREADS) {
        const long long t0 = o * J.stride, t1 = t0 + J.lag;
        const size_t a0 = (size_t)t0 * (size_t)ncol + (size_t)(J.e0 + e);
        const size_t a1 = (size_t)t1 * (size_t)ncol + (size_t)(J.e0 + e);
        double x0 = r[a0], y0 = r[a0 + E], z0 = r[a0 + 2 * E];
        double x1 = r[a1], y1 = r[a1 + E], z1 = r[a1 + 2 * E];
        if (WRAP) {
            const int i0 = img[a0], j0 = img[a0 + E], k0 = img[a0 + 2 * E];
            const int i1 = img[a1], j1 = img[a1 + E], k1 = img[a1 + 2 * E];
            const double *b0 = box + 3 * t0, *b1 = box + 3 * t1;
            x0 = x0 + (double)i0 * b0[0];
            y0 = y0 + (double)j0 * b0[1];
            z0 = z0 + (double)k0 * b0[2];
            x1 = x1 + (double)i1 * b1[0];
            y1 = y1 + (double)j1 * b1[1];
            z1 = z1 + (double)k1 * b1[2];
        }
        const double dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
        const double rsq = (dx * dx + dy * dy) + dz * dz;
        s1 += __builtin_sqrt(rsq);
        s2 += rsq;
        s4 += rsq * rsq;
        if (rsq < top) {
            const float g = __builtin_amdgcn_sqrtf((float)rsq) * gscale;  // a guess; the edges decide
            int k = g < (float)(nbins - 1) ? (int)g : nbins - 1;
            while (rsq < edges[k]) --k;       // edges[0] == 0 stops it
            while (rsq >= edges[k + 1]) ++k;  // rsq < edges[nbins] stops it
            if (LDS)
                atomicAdd(&s_hist[k], 1u);
            else
                atomicAdd(&g_row[k], 1ull);
        } else {
            ++n_ovf;  // bin >= nbins, or NaN
        }
        e += J.r;
        o += J.q;
        if (e >= J.ng) {
            e -= J.ng;
            ++o;
        }
    }
    // the workgroup's moments: a fixed butterfly inside every wave, then the waves in order
    for (int sh = 32; sh; sh >>= 1) {
        s1 += __shfl_xor(s1, sh);
        s2 += __shfl_xor(s2, sh);
        s4 += __shfl_xor(s4, sh);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_red[3 * wave] = s1;
        s_red[3 * wave + 1] = s2;
        s_red[3 * wave + 2] = s4;
    }
    if (n_ovf) atomicAdd(&s_ovf, n_ovf);
    __syncthreads();
    if (threadIdx.x < 3) {
        double a = s_red[threadIdx.x];
        for (int k = 1; k < DP_THREADS / 64; ++k) a += s_red[3 * k + threadIdx.x];
        part[3 * (size_t)(J.part0 + blockIdx.x) + threadIdx.x] = a;
    }
    if (threadIdx.x == 0 && s_ovf) atomicAdd(&overflow[job], (unsigned long long)s_ovf);
    if (LDS)
        for (int k = threadIdx.x; k < nbins; k += DP_THREADS) {
            const unsigned v = s_hist[k];
            if (v) atomicAdd(&g_row[k], (unsigned long long)v);
        }
}

// moments[job] <- the job's partials: lane t adds partials t, t + 256, ... in order, then a fixed tree over the lanes.
__global__ __launch_bounds__(DP_THREADS) void dp_moment_kernel(const DpJob *__restrict__ jobs, int job0,
                                                               const double *__restrict__ part,
                                                               double *__restrict__ moments)
{
    __shared__ double s_red[3][DP_THREADS];
    const int job = job0 + (int)blockIdx.x;
    const DpJob J = jobs[job];
    double a[3] = {0.0, 0.0, 0.0};
    for (long long b = threadIdx.x; b < J.nblk; b += DP_THREADS)
        for (int m = 0; m < 3; ++m) a[m] += part[3 * (size_t)(J.part0 + b) + m];
    for (int m = 0; m < 3; ++m) s_red[m][threadIdx.x] = a[m];
    __syncthreads();
    for (int w = DP_THREADS / 2; w; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int m = 0; m < 3; ++m) s_red[m][threadIdx.x] += s_red[m][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 3) moments[3 * (size_t)job + threadIdx.x] = s_red[threadIdx.x][0];
}

}  // namespace

extern "C" {

int mdhip_displacement_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                            const double *box, int n_groups, const int64_t *group_off, int n_jobs,
                            const int32_t *jobs, double bin_size, int32_t nbins, const double *edges,
                            uint64_t *hist, uint64_t *overflow, uint64_t *windows, double *moments,
                            uint64_t *crossings)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_ent >= 0 && n_groups >= 0 && n_jobs >= 0, "negative sizes");
    MD_REQUIRE(n_ent < (1ll << 40) && n_frames < (1ll << 40) && (n_ent == 0 || n_frames < (1ll << 40) / n_ent),
               "trajectory too large");
    MD_REQUIRE(nbins >= 1 && nbins <= (1 << 20), "nbins must be in [1, 2^20]");
    MD_REQUIRE(bin_size > 0.0 && bin_size < __builtin_inf(), "bin_size must be positive and finite");
    int rc;
    if ((rc = gp_check_groups(ctx, n_groups, group_off, n_ent))) return rc;
    MD_REQUIRE(n_jobs == 0 || (jobs && hist && overflow && windows && moments), "NULL array");
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 3 * (size_t)j;
        MD_REQUIRE(q[0] >= 0 && q[0] < n_groups, "job %d: group %d out of range", j, q[0]);
        MD_REQUIRE(q[1] >= 1 && (int64_t)q[1] <= n_frames - 1, "job %d: lag %d not in [1, n_frames - 1]", j, q[1]);
        MD_REQUIRE(q[2] >= 1, "job %d: stride %d must be positive", j, q[2]);
    }
    MD_REQUIRE((size_t)n_jobs * (size_t)nbins < ((size_t)1 << 34), "result too large");
    if ((rc = gp_check_edges(ctx, edges, nbins, n_jobs))) return rc;
    const bool wrap = box != nullptr && n_ent > 0 && n_frames >= 2;
    if (crossings) *crossings = 0;
    if (n_jobs == 0 && !(wrap && crossings)) return cs.end();
    MD_REQUIRE(n_ent == 0 || r, "NULL coordinates");

    // the jobs: windows, workgroups, partial-moment slots
    std::vector<DpJob> tab((size_t)n_jobs);
    long long n_part = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 3 * (size_t)j;
        DpJob &J = tab[(size_t)j];
        J.e0 = group_off[q[0]];
        J.ng = group_off[q[0] + 1] - J.e0;
        J.lag = q[1];
        J.stride = q[2];
        const long long n_orig = (n_frames - 1 - J.lag) / J.stride + 1;
        J.n_win = n_orig * J.ng;
        const long long even = ((J.n_win + DP_BLOCKS - 1) / DP_BLOCKS + DP_THREADS - 1) / DP_THREADS * DP_THREADS;
        J.wpb = std::max({DP_MIN_WPB, even, nbins <= DP_LDS_WORDS ? 4ll * nbins : 0ll});
        J.nblk = (J.n_win + J.wpb - 1) / J.wpb;
        J.part0 = n_part;
        J.q = J.ng ? (int)(DP_THREADS / J.ng) : 0;
        J.r = J.ng ? (int)(DP_THREADS % J.ng) : 0;
        n_part += J.nblk;
        windows[j] = (uint64_t)J.n_win;
    }
    std::vector<double> own;
    if (n_jobs && (rc = gp_edges(ctx, edges, own, bin_size, nbins))) return rc;

    MD_HIP(hipSetDevice(ctx->device));
    const size_t r_bytes = (size_t)n_frames * 3 * (size_t)n_ent * 8;
    const double *d_r = (const double *)mdhip_stage(ctx, WS_XYZ_I, r, r_bytes, r_on_device || r_bytes == 0, &rc);
    if (rc) return rc;
    MD_WS(d_misc, unsigned long long, WS_MISC, ((size_t)n_jobs + 1) * 8);  // overflow [J] | crossings
    unsigned long long *d_cross = d_misc + n_jobs;
    const double *d_box = nullptr;
    const int *d_img = nullptr;
    KernelTimer timer(ctx, 0);
    int launches = 0;
    MD_HIP(hipMemsetAsync(d_misc, 0, ((size_t)n_jobs + 1) * 8, ctx->stream));
    if (wrap) {
        if ((rc = dp_image_counts(ctx, d_r, box, n_frames, n_ent, d_cross, d_box, d_img, launches))) return rc;
    }
    unsigned long long *d_hist = nullptr;
    double *d_mom = nullptr;
    const size_t hist_bytes = (size_t)n_jobs * (size_t)nbins * 8;
    if (n_jobs) {
        MD_WS(d_jobs, DpJob, WS_AUX2, tab.size() * sizeof(DpJob));
        if ((rc = mdhip_h2d_small(ctx, d_jobs, tab.data(), tab.size() * sizeof(DpJob)))) return rc;
        MD_WS(d_edges, double, WS_TABLES, ((size_t)nbins + 1) * 8);
        if ((rc = mdhip_h2d_small(ctx, d_edges, edges, ((size_t)nbins + 1) * 8))) return rc;
        MD_WS(d_h, unsigned long long, WS_HIST, hist_bytes);
        MD_WS(d_part, double, WS_PART, std::max<size_t>((size_t)n_part, 1) * 24);
        MD_WS(d_m, double, WS_OUT, (size_t)n_jobs * 24);
        d_hist = d_h;
        d_mom = d_m;
        MD_HIP(hipMemsetAsync(d_hist, 0, hist_bytes, ctx->stream));
        const bool lds = nbins <= DP_LDS_WORDS;
        const size_t lds_b = lds ? (size_t)nbins * 4 : 0;
        const float gscale = (float)(1.0 / bin_size);
        // grid.y holds at most 65535 jobs: longer job lists go in slices (a job's workgroups are the same in any slice)
        for (int j0 = 0; j0 < n_jobs; j0 += DP_MAX_Y) {
            const int nj = std::min(DP_MAX_Y, n_jobs - j0);
            long long gx = 0;
            for (int j = j0; j < j0 + nj; ++j) gx = std::max(gx, tab[(size_t)j].nblk);
            if (gx > 0) {
                const dim3 grid((unsigned)gx, (unsigned)nj), block(DP_THREADS);
#define DP_BIN(W, L)                                                                                                  \
    hipLaunchKernelGGL((dp_bin_kernel<W, L>), grid, block, lds_b, ctx->stream, d_r, d_img, d_box, (long long)n_ent,  \
                       d_jobs, j0, d_edges, gscale, (int)nbins, d_hist, d_misc, d_part)
                if (wrap) {
                    if (lds) DP_BIN(true, true); else DP_BIN(true, false);
                } else {
                    if (lds) DP_BIN(false, true); else DP_BIN(false, false);
                }
#undef DP_BIN
                MD_HIP(hipGetLastError());
                ++launches;
            }
            hipLaunchKernelGGL(dp_moment_kernel, dim3((unsigned)nj), dim3(DP_THREADS), 0, ctx->stream, d_jobs, j0,
                               d_part, d_mom);
            MD_HIP(hipGetLastError());
            ++launches;
        }
        ctx->last_kernel = "dp_bin_kernel";
    }
    ctx->last_launches = launches;
    timer.stop();
    if (n_jobs) {
        if ((rc = mdhip_result(cs, hist, d_hist, hist_bytes, 0))) return rc;
        if ((rc = mdhip_result(cs, overflow, d_misc, (size_t)n_jobs * 8, 0))) return rc;
        if ((rc = mdhip_result(cs, moments, d_mom, (size_t)n_jobs * 24, 0))) return rc;
    }
    if (crossings && (rc = mdhip_result(cs, crossings, d_cross, 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
