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
// One launch for all jobs (blockIdx.y = job; more than 65 535 jobs go in slices). Of a job's two groups one lies along
// the lanes and the other is swept as wave-uniform operands; which is which is the host's choice (the group that fills
// its tiles of 64 better goes on the lanes: 20 ions against 5000 solvent atoms put the solvent there), and costs the
// kernel nothing: |d| does not know which end was subtracted, and the box is that of t0 either way. A wave takes one
// unit at a time: (origin, tile of 64 lane entities, chunk of up to VH_JCHUNK uniform entities). The lane entity's
// three coordinates and the three edges of box[t0] stay in registers; the uniform entities come through uniform
// addresses on a const __restrict__ pointer, VH_U at a time, which the compiler turns into scalar loads: no vector
// load per pair. The cutoff compare comes first (at r_max = L/2 about half of all pairs fail it); the bin is a float
// guess with an exact guard band (as the pair sweeps, pair_plan.h): only a guess within the band of an integer walks
// the edge table. A workgroup owns a run of `upb` consecutive units of one job, its waves striding through them, and
// the job's row as uint32 in LDS (LDS atomics) when nbins <= VH_LDS_WORDS, flushed with 64-bit integer atomics;
// longer rows take 64-bit atomics on the global row. upb * 64 * VH_JCHUNK-or-less < 2^31 pairs per workgroup: no
// uint32 word can wrap. A lane counts its pairs (from the unit's sizes) and the pairs it binned; the difference is its
// share of beyond[job]: a butterfly, one LDS atomic per wave, one 64-bit atomic per workgroup. Groups are contiguous and ascending, so two different groups share no entity and the j != i
// test is right for every job: there is no same-group variant of the kernel. Integers only: no float atomics, the
// results do not depend on the launch geometry. Measured: DESIGN.md 4.12b.

#include <algorithm>
#include <cmath>
#include <vector>

#include "ctx.h"
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
constexpr int VH_MAX_Y = 65535;

struct VhJob {
    long long l0, nl;          // the entities along the lanes [l0, l0 + nl) ...
    long long u0, nu;          // ... and the wave-uniform ones [u0, u0 + nu)
    long long n_tiles, n_jc;   // tiles of 64 lane entities, chunks of VH_JCHUNK uniform entities
    long long n_units, upb, nblk;
    int lag, stride;
    int lane_late;             // 1: the lanes hold frame t0 + lag (group b), the uniform set frame t0 (group a)
};

// Block (x, y): units [x * upb, (x + 1) * upb) of job job0 + y. Dynamic LDS: the job's row when LDS.
template <bool LDS>
__global__ __launch_bounds__(VH_THREADS) void vh_pair_kernel(const double *__restrict__ r,
                                                             const double *__restrict__ box, long long E,
                                                             const VhJob *__restrict__ jobs, int job0,
                                                             const double *__restrict__ edges, float gscale,
                                                             float near, int nbins,
                                                             unsigned long long *__restrict__ hist,
                                                             unsigned long long *__restrict__ beyond)
{
    extern __shared__ unsigned s_hist[];
    __shared__ unsigned s_bey;
    const int job = job0 + (int)blockIdx.y;
    const VhJob J = jobs[job];
    if ((long long)blockIdx.x >= J.nblk) return;  // (the whole workgroup: jobs of one launch differ in size)
    if (LDS)
        for (int w = threadIdx.x; w < nbins; w += VH_THREADS) s_hist[w] = 0u;
    if (threadIdx.x == 0) s_bey = 0u;
    __syncthreads();
    unsigned long long *g_row = hist + (size_t)job * (size_t)nbins;
    const double top = edges[nbins];
    const float near2 = near + near;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long ua = (long long)blockIdx.x * J.upb;
    const long long ub = ua + J.upb < J.n_units ? ua + J.upb : J.n_units;
    unsigned n_pairs = 0, n_in = 0;  // this lane's pairs, and those of them it binned: the rest are beyond r_max, or NaN

    auto tally = [&](double rsq, bool valid) {
        if (rsq < top && valid) {
            const float g = __builtin_fmaf(__builtin_amdgcn_sqrtf((float)rsq), gscale, near);
            int k = (int)g;  // the bin, unless g is within the band above an integer: then the edges decide
            if (__builtin_amdgcn_fractf(g) < near2) {
                k = k < nbins - 1 ? k : nbins - 1;
                while (rsq < edges[k]) --k;       // edges[0] == 0 stops it
                while (rsq >= edges[k + 1]) ++k;  // rsq < edges[nbins] stops it
            }
            if (LDS)
                atomicAdd(&s_hist[k], 1u);
            else
                atomicAdd(&g_row[k], 1ull);
            ++n_in;
        }
    };

    for (long long u = ua + wave; u < ub; u += VH_WAVES) {
        const long long c = u % J.n_jc, ot = u / J.n_jc;
        const long long o = ot / J.n_tiles, tile = ot - o * J.n_tiles;
        const long long t0 = o * J.stride;
        const long long fl = J.lane_late ? t0 + J.lag : t0, fu = J.lane_late ? t0 : t0 + J.lag;
        const double Lx = box[3 * t0], Ly = box[3 * t0 + 1], Lz = box[3 * t0 + 2];
        const long long il = tile * 64 + lane;
        const long long j0 = c * VH_JCHUNK;
        const int jlen = (int)(J.nu - j0 < VH_JCHUNK ? J.nu - j0 : VH_JCHUNK);
        if (il >= J.nl) continue;
        const size_t al = (size_t)fl * 3 * (size_t)E + (size_t)(J.l0 + il);
        const double xi = r[al], yi = r[al + E], zi = r[al + 2 * E];
        // the uniform index that is this lane's own entity (none: outside [0, jlen))
        const long long self_ll = J.l0 + il - J.u0 - j0;
        const int self = self_ll >= 0 && self_ll < jlen ? (int)self_ll : -1;
        n_pairs += (unsigned)jlen - (self >= 0);
        const double *__restrict__ px = r + (size_t)fu * 3 * (size_t)E + (size_t)(J.u0 + j0);
        const double *__restrict__ py = px + E;
        const double *__restrict__ pz = py + E;
        int jj = 0;
        for (; jj + VH_U <= jlen; jj += VH_U) {
            double xj[VH_U], yj[VH_U], zj[VH_U], rsq[VH_U];
#pragma unroll
            for (int q = 0; q < VH_U; ++q) {
                xj[q] = px[jj + q];
                yj[q] = py[jj + q];
                zj[q] = pz[jj + q];
            }
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
    }
    unsigned n_bey = n_pairs - n_in;
    for (int sh = 32; sh; sh >>= 1) n_bey += __shfl_xor(n_bey, sh);
    if (lane == 0 && n_bey) atomicAdd(&s_bey, n_bey);
    __syncthreads();
    if (threadIdx.x == 0 && s_bey) atomicAdd(&beyond[job], (unsigned long long)s_bey);
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
    MD_REQUIRE(n_frames >= 0 && n_ent >= 0 && n_groups >= 0 && n_jobs >= 0, "negative sizes");
    MD_REQUIRE(n_ent < (1ll << 40) && n_frames < (1ll << 40) && (n_ent == 0 || n_frames < (1ll << 40) / n_ent),
               "trajectory too large");
    MD_REQUIRE(box, "NULL box: the distinct van Hove function needs wrapped coordinates and their box");
    MD_REQUIRE(nbins >= 1 && nbins <= (1 << 20), "nbins must be in [1, 2^20]");
    MD_REQUIRE(bin_size > 0.0 && bin_size < __builtin_inf(), "bin_size must be positive and finite");
    MD_REQUIRE(n_groups == 0 || group_off, "NULL group_off");
    for (int g = 0; g < n_groups; ++g)
        MD_REQUIRE(group_off[g] >= 0 && group_off[g] <= group_off[g + 1] && group_off[g + 1] <= n_ent,
                   "group_off must ascend within [0, n_ent] (group %d)", g);
    MD_REQUIRE(n_jobs == 0 || (jobs && hist && beyond && pairs), "NULL array");
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 4 * (size_t)j;
        MD_REQUIRE(q[0] >= 0 && q[0] < n_groups && q[1] >= 0 && q[1] < n_groups, "job %d: group (%d, %d) out of range",
                   j, q[0], q[1]);
        MD_REQUIRE(q[2] >= 0 && (int64_t)q[2] <= n_frames - 1, "job %d: lag %d not in [0, n_frames - 1]", j, q[2]);
        MD_REQUIRE(q[3] >= 1, "job %d: stride %d must be positive", j, q[3]);
    }
    MD_REQUIRE((size_t)n_jobs * (size_t)nbins < ((size_t)1 << 34), "result too large");
    if (edges && n_jobs) {  // (the kernel walks the table: it has to start at 0 and ascend)
        MD_REQUIRE(edges[0] == 0.0, "edges[0] must be 0");
        for (int k = 0; k < nbins; ++k) MD_REQUIRE(edges[k] <= edges[k + 1], "edges must ascend (bin %d)", k);
    }
    if (n_jobs == 0) return cs.end();
    MD_REQUIRE(n_ent == 0 || r, "NULL coordinates");

    // the jobs: which group lies along the lanes, units, workgroups
    const bool lds = nbins <= VH_LDS_WORDS;
    std::vector<VhJob> tab((size_t)n_jobs);
    std::vector<uint64_t> n_pairs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 4 * (size_t)j;
        VhJob &J = tab[(size_t)j];
        const long long a0 = group_off[q[0]], na = group_off[q[0] + 1] - a0;
        const long long b0 = group_off[q[1]], nb = group_off[q[1] + 1] - b0;
        J.lag = q[2];
        J.stride = q[3];
        const long long n_orig = (n_frames - 1 - J.lag) / J.stride + 1;
        n_pairs[(size_t)j] = (uint64_t)n_orig * ((uint64_t)na * (uint64_t)nb - (q[0] == q[1] ? (uint64_t)na : 0));
        // lanes: the group that wastes fewer lanes of its last tile (na / tiles(na) against nb / tiles(nb))
        const long long ta = (na + 63) / 64, tb = (nb + 63) / 64;
        J.lane_late = na * tb < nb * ta;
        J.l0 = J.lane_late ? b0 : a0;
        J.nl = J.lane_late ? nb : na;
        J.u0 = J.lane_late ? a0 : b0;
        J.nu = J.lane_late ? na : nb;
        J.n_tiles = (J.nl + 63) / 64;
        J.n_jc = (J.nu + VH_JCHUNK - 1) / VH_JCHUNK;
        J.n_units = n_orig * J.n_tiles * J.n_jc;
        J.upb = 1;
        J.nblk = 0;
        if (J.n_units > 0) {
            const long long per_unit = 64 * std::min(J.nu, VH_JCHUNK);  // pairs of one unit at most
            const long long even = (J.n_units + VH_BLOCKS - 1) / VH_BLOCKS;
            const long long amortise = lds ? (8ll * nbins + per_unit - 1) / per_unit : 0;  // zeroing and flushing a row
            J.upb = std::min(std::max({(long long)VH_WAVES, even, amortise}), VH_MAX_PAIRS / per_unit);
            J.nblk = (J.n_units + J.upb - 1) / J.upb;
        }
    }
    for (int j = 0; j < n_jobs; ++j)
        MD_REQUIRE(tab[(size_t)j].nblk < (1ll << 31), "job %d: too many workgroups", j);
    std::copy(n_pairs.begin(), n_pairs.end(), pairs);
    std::vector<double> own;
    if (!edges) {
        own.resize((size_t)nbins + 1);
        if (mdhip_bin_edges(bin_size, nbins, own.data()) != MDHIP_OK)
            return mdhip_fail(ctx, MDHIP_EINVAL, "no bin edges for bin_size %g", bin_size);
        edges = own.data();
    }
    // |error| of the f32 guess fma(sqrt((float)rsq), 1/bin_size, near), as pair_plan.h: relative 2.1e-7 of the bin number
    // plus half an ulp of the largest value each for the addend and the fma; near = 2 x that. A band of 1 or more (very
    // many bins) sends every pair to the table.
    const double ulp = std::ldexp(1.0, (int)std::floor(std::log2((double)nbins + 1.0)) - 23);
    const float near = (float)(2.0 * ((double)nbins * 2.1e-7 + ulp) + 1.0e-5);
    const float gscale = (float)(1.0 / bin_size);

    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const size_t r_bytes = (size_t)n_frames * 3 * (size_t)n_ent * 8;
    const double *d_r = (const double *)mdhip_stage(ctx, WS_XYZ_I, r, r_bytes, r_on_device || r_bytes == 0, &rc);
    if (rc) return rc;
    MD_WS(d_bey, unsigned long long, WS_MISC, (size_t)n_jobs * 8);
    MD_WS(d_box, double, WS_BOX, (size_t)n_frames * 24);
    if ((rc = mdhip_h2d_small(ctx, d_box, box, (size_t)n_frames * 24))) return rc;
    MD_WS(d_jobs, VhJob, WS_AUX2, tab.size() * sizeof(VhJob));
    if ((rc = mdhip_h2d_small(ctx, d_jobs, tab.data(), tab.size() * sizeof(VhJob)))) return rc;
    MD_WS(d_edges, double, WS_TABLES, ((size_t)nbins + 1) * 8);
    if ((rc = mdhip_h2d_small(ctx, d_edges, edges, ((size_t)nbins + 1) * 8))) return rc;
    const size_t hist_bytes = (size_t)n_jobs * (size_t)nbins * 8;
    MD_WS(d_hist, unsigned long long, WS_HIST, hist_bytes);
    KernelTimer timer(ctx, 0);
    int launches = 0;
    MD_HIP(hipMemsetAsync(d_bey, 0, (size_t)n_jobs * 8, ctx->stream));
    MD_HIP(hipMemsetAsync(d_hist, 0, hist_bytes, ctx->stream));
    const size_t lds_b = lds ? (size_t)nbins * 4 : 0;
    // grid.y holds at most 65535 jobs: longer job lists go in slices (a job's workgroups are the same in any slice)
    for (int j0 = 0; j0 < n_jobs; j0 += VH_MAX_Y) {
        const int nj = std::min(VH_MAX_Y, n_jobs - j0);
        long long gx = 0;
        for (int j = j0; j < j0 + nj; ++j) gx = std::max(gx, tab[(size_t)j].nblk);
        if (gx == 0) continue;
        const dim3 grid((unsigned)gx, (unsigned)nj), block(VH_THREADS);
        if (lds)
            hipLaunchKernelGGL(vh_pair_kernel<true>, grid, block, lds_b, ctx->stream, d_r, d_box, (long long)n_ent,
                               d_jobs, j0, d_edges, gscale, near, (int)nbins, d_hist, d_bey);
        else
            hipLaunchKernelGGL(vh_pair_kernel<false>, grid, block, 0, ctx->stream, d_r, d_box, (long long)n_ent,
                               d_jobs, j0, d_edges, gscale, near, (int)nbins, d_hist, d_bey);
        MD_HIP(hipGetLastError());
        ++launches;
    }
    ctx->last_kernel = "vh_pair_kernel";
    ctx->last_launches = launches;
    timer.stop();
    if ((rc = mdhip_result(cs, hist, d_hist, hist_bytes, 0))) return rc;
    if ((rc = mdhip_result(cs, beyond, d_bey, (size_t)n_jobs * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
