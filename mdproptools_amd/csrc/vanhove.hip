// vanhove.hip — the distinct part of the van Hove function, G_d(r, t), before normalisation: for every time origin
// t0 the histogram of the distances between where the atoms of group a were at t0 and where the atoms of group b are
// at t0 + k (Displacement.calc_van_hove_distinct). The self part is displacement.hip.
//
// For WRAPPED coordinates r [F][3][E], box [F][3] and jobs (a, b, k, s), per origin t0 = 0, s, 2s, ... (t0 + k <= F - 1),
// i in a, j in b, j != i as entity indices:
//   d = r[t0+k][x][j] - r[t0][x][i] per axis, one shift by L = box[t0][x] iff |d| > L/2 (strict: the reference's single
//     wrap, rdf_cn.py:44-57), taken as the magnitude min(|d|, ||d| - L|) (wrap_abs, pair_common.h: the same number);
//   rsq = (dx dx + dy dy) + dz dz unfused; +1 in hist[job][bin] when rsq < edges[nbins], the bin by comparison of rsq
//     with the exact edge table (mdhip_bin_edges), else (NaN and +inf included) +1 in beyond[job].
//
// The sweep over the two groups — job plan, units, bin lookup, the beyond count, launch — is group_pairs.h; this file
// owns what a unit does. Which group lies along the lanes costs the kernel nothing: |d| does not know which end was
// subtracted and the box is that of t0 either way; only the two frames swap. The lane entity's coordinates and the edges
// of box[t0] stay in registers; the uniform entities come VH_U at a time through scalar loads: no vector load per pair.
// The cutoff compare comes first (at r_max = L/2 about half of all pairs fail it). A workgroup holds the job's row as
// uint32 in LDS (LDS atomics; at most 2^31 pairs: no word can wrap) when nbins <= VH_LDS_WORDS, flushed with 64-bit
// integer atomics; longer rows take 64-bit atomics on the global row. Integers only: no float atomics, the results do
// not depend on the launch geometry. Measured: DESIGN.md 4.12b.

#include "group_pairs.h"
#include "pair_common.h"

#pragma clang fp contract(off)

namespace {

using mdpair::wrap_abs;

constexpr int VH_THREADS = 256;
constexpr int VH_WAVES = VH_THREADS / 64;
constexpr int VH_U = 8;                       // uniform entities per batch of scalar loads
constexpr int VH_LDS_WORDS = 16128;           // uint32 bins of a job's row in LDS (63 KiB), as DP_LDS_WORDS
constexpr long long VH_JCHUNK = 1ll << 20;    // uniform entities per unit: 64 * 2^20 = 2^26 pairs at most
constexpr long long VH_BLOCKS = 4096;         // about this many workgroups per job at most
constexpr long long VH_MAX_PAIRS = 1ll << 31;  // pairs a workgroup bins between zeroing and flushing its row

// Dynamic LDS: the job's row when LDS.
template <bool LDS>
__global__ __launch_bounds__(VH_THREADS) void vh_pair_kernel(
    const double *__restrict__ r, const double *__restrict__ box, long long E, const GpJob *__restrict__ jobs, int job0,
    const double *__restrict__ edges, float gscale, float near, int nbins, unsigned long long *__restrict__ hist,
    unsigned long long *__restrict__ beyond)
{
    extern __shared__ unsigned s_hist[];
    __shared__ unsigned s_bey;
    const int job = job0 + (int)blockIdx.y;
    GpJob J;
    if (!gp_job(jobs, job, J)) return;
    if (LDS)
        for (int w = threadIdx.x; w < nbins; w += VH_THREADS) s_hist[w] = 0u;
    if (threadIdx.x == 0) s_bey = 0u;
    __syncthreads();
    unsigned long long *g_row = hist + (size_t)job * (size_t)nbins;
    const double top = edges[nbins];
    const float near2 = near + near;
    unsigned n_in = 0;  // the pairs this lane binned: the rest of its pairs are beyond r_max, or NaN

    auto tally = [&](double rsq, bool valid) {
        if (rsq < top && valid) {
            const int k = gp_bin(rsq, edges, gscale, near, near2, nbins);
            if (LDS)
                atomicAdd(&s_hist[k], 1u);
            else
                atomicAdd(&g_row[k], 1ull);
            ++n_in;
        }
    };

    const unsigned n_pairs = gp_walk<VH_WAVES, VH_JCHUNK>(J, [&](long long o, long long il, long long j0, int jlen, int self) {
        const long long t0 = o * J.stride;
        const long long fl = J.lanes_b ? t0 + J.lag : t0, fu = J.lanes_b ? t0 : t0 + J.lag;
        const double Lx = box[3 * t0], Ly = box[3 * t0 + 1], Lz = box[3 * t0 + 2];
        const size_t al = (size_t)fl * 3 * (size_t)E + (size_t)(J.l0 + il);
        const double xi = r[al], yi = r[al + E], zi = r[al + 2 * E];
        const double *__restrict__ px = r + (size_t)fu * 3 * (size_t)E + (size_t)(J.u0 + j0);
        const double *__restrict__ py = px + E, *__restrict__ pz = py + E;
        int jj = 0;
        for (; jj + VH_U <= jlen; jj += VH_U) {
            double xj[VH_U], yj[VH_U], zj[VH_U], rsq[VH_U];
#pragma unroll
            for (int q = 0; q < VH_U; ++q) xj[q] = px[jj + q], yj[q] = py[jj + q], zj[q] = pz[jj + q];
#pragma unroll
            for (int q = 0; q < VH_U; ++q) {
                const double ax = wrap_abs(xj[q] - xi, Lx);
                const double ay = wrap_abs(yj[q] - yi, Ly);
                const double az = wrap_abs(zj[q] - zi, Lz);
                rsq[q] = (ax * ax + ay * ay) + az * az;
            }
#pragma unroll
            for (int q = 0; q < VH_U; ++q) tally(rsq[q], jj + q != self);
        }
        for (; jj < jlen; ++jj) {
            const double ax = wrap_abs(px[jj] - xi, Lx);
            const double ay = wrap_abs(py[jj] - yi, Ly);
            const double az = wrap_abs(pz[jj] - zi, Lz);
            tally((ax * ax + ay * ay) + az * az, jj != self);
        }
    });
    unsigned n_bey[1] = {n_pairs - n_in};
    unsigned long long *const g_bey[1] = {beyond + job};
    gp_tail(n_bey, &s_bey, g_bey);
    if (LDS)
        for (int k = threadIdx.x; k < nbins; k += VH_THREADS) {
            const unsigned v = s_hist[k];
            if (v) atomicAdd(&g_row[k], (unsigned long long)v);
        }
}

}  // namespace

extern "C" {

int mdhip_van_hove_distinct(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                            const double *box, int n_groups, const int64_t *group_off, int n_jobs,
                            const int32_t *jobs, double bin_size, int32_t nbins, const double *edges, uint64_t *hist,
                            uint64_t *beyond, uint64_t *pairs)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    int rc;
    MD_REQUIRE(n_frames >= 0 && n_ent >= 0 && n_groups >= 0 && n_jobs >= 0, "negative sizes");
    MD_REQUIRE(n_ent < (1ll << 40) && n_frames < (1ll << 40) && (n_ent == 0 || n_frames < (1ll << 40) / n_ent),
               "trajectory too large");
    MD_REQUIRE(box, "NULL box: the distinct van Hove function needs wrapped coordinates and their box");
    MD_REQUIRE(nbins >= 1 && nbins <= (1 << 20), "nbins must be in [1, 2^20]");
    MD_REQUIRE(bin_size > 0.0 && bin_size < __builtin_inf(), "bin_size must be positive and finite");
    if ((rc = gp_check_groups(ctx, n_groups, group_off, n_ent))) return rc;
    MD_REQUIRE(n_jobs == 0 || (jobs && hist && beyond && pairs), "NULL array");
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 4 * (size_t)j;
        MD_REQUIRE(q[0] >= 0 && q[0] < n_groups && q[1] >= 0 && q[1] < n_groups, "job %d: group (%d, %d) out of range",
                   j, q[0], q[1]);
        MD_REQUIRE(q[2] >= 0 && (int64_t)q[2] <= n_frames - 1, "job %d: lag %d not in [0, n_frames - 1]", j, q[2]);
        MD_REQUIRE(q[3] >= 1, "job %d: stride %d must be positive", j, q[3]);
    }
    MD_REQUIRE((size_t)n_jobs * (size_t)nbins < ((size_t)1 << 34), "result too large");
    if ((rc = gp_check_edges(ctx, edges, nbins, n_jobs))) return rc;
    if (n_jobs == 0) return cs.end();
    MD_REQUIRE(n_ent == 0 || r, "NULL coordinates");

    const bool lds = nbins <= VH_LDS_WORDS;
    const GpRule rule = {VH_WAVES, VH_JCHUNK, VH_BLOCKS, VH_MAX_PAIRS, lds ? 8ll * nbins : 0};
    std::vector<GpJob> tab((size_t)n_jobs);
    std::vector<uint64_t> n_pairs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 4 * (size_t)j;
        const long long a0 = group_off[q[0]], b0 = group_off[q[1]];
        n_pairs[(size_t)j] = gp_plan(tab[(size_t)j], (n_frames - 1 - q[2]) / q[3] + 1, a0, group_off[q[0] + 1] - a0, b0,
                                     group_off[q[1] + 1] - b0, q[0] == q[1], rule);
        tab[(size_t)j].lag = q[2], tab[(size_t)j].stride = q[3];
    }
    for (int j = 0; j < n_jobs; ++j) MD_REQUIRE(tab[(size_t)j].nblk < (1ll << 31), "job %d: too many workgroups", j);
    std::copy(n_pairs.begin(), n_pairs.end(), pairs);
    std::vector<double> own;
    if ((rc = gp_edges(ctx, edges, own, bin_size, nbins))) return rc;
    const GpBand band = gp_band(nbins, bin_size);

    MD_HIP(hipSetDevice(ctx->device));
    const size_t r_bytes = (size_t)n_frames * 3 * (size_t)n_ent * 8;
    const double *d_r = (const double *)mdhip_stage(ctx, WS_XYZ_I, r, r_bytes, r_on_device || r_bytes == 0, &rc);
    if (rc) return rc;
    MD_WS(d_bey, unsigned long long, WS_MISC, (size_t)n_jobs * 8);
    GpTables d;
    if ((rc = gp_stage(ctx, box, n_frames, tab, edges, nbins, d))) return rc;
    const size_t hist_bytes = (size_t)n_jobs * (size_t)nbins * 8;
    MD_WS(d_hist, unsigned long long, WS_HIST, hist_bytes);
    KernelTimer timer(ctx, 0);
    MD_HIP(hipMemsetAsync(d_bey, 0, (size_t)n_jobs * 8, ctx->stream));
    MD_HIP(hipMemsetAsync(d_hist, 0, hist_bytes, ctx->stream));
    if ((rc = gp_launch(ctx, "vh_pair_kernel", timer, tab, [&](dim3 grid, int j0) {
        hipLaunchKernelGGL(lds ? vh_pair_kernel<true> : vh_pair_kernel<false>, grid, dim3(VH_THREADS),
                           lds ? (size_t)nbins * 4 : 0, ctx->stream, d_r, d.box, (long long)n_ent, d.jobs, j0, d.edges,
                           band.gscale, band.near, (int)nbins, d_hist, d_bey);
    }))) return rc;
    if ((rc = mdhip_result(cs, hist, d_hist, hist_bytes, 0))) return rc;
    if ((rc = mdhip_result(cs, beyond, d_bey, (size_t)n_jobs * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
