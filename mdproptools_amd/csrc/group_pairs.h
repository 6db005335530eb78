// group_pairs.h — the sweep over all pairs of two contiguous entity groups that mdhip_van_hove_distinct (vanhove.hip) and
// mdhip_vector_pair_hist (vector_pairs.hip) share: job record, unit plan, unit walker, bin lookup, counter tail, launch.
// One launch takes all jobs (blockIdx.y = job; more than 65 535 jobs go in slices). Of a job's two groups the one that
// fills its tiles of 64 better lies along the lanes (20 ions against 5000 solvent atoms put the solvent there); the other
// is swept as wave-uniform operands, through uniform addresses that the compiler turns into scalar loads. A wave takes
// one UNIT at a time: (origin, tile of 64 lane entities, chunk of uniform entities); a workgroup owns `upb` consecutive
// units of one job, its waves striding through them, and the job's row of bins between zeroing and flushing it:
// upb * (pairs of a unit) <= max_pairs, so that no word of the row can wrap. Frames, wrap, batch of uniform loads, payload,
// row layout and flush are each kernel's own. The host plan is arithmetic on plain values (no HIP header, no context), in the
// form of mol_tile.h: tests/native/group_pairs_plan_main.cpp walks it with g++ under sanitizers; the rest is for hipcc only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

// ---- host plan ------------------------------------------------------------------------------------------------------

struct GpJob {
    long long l0, nl;          // the entities along the lanes [l0, l0 + nl) ...
    long long u0, nu;          // ... and the wave-uniform ones [u0, u0 + nu)
    long long n_tiles, n_jc;   // tiles of 64 lane entities, chunks of uniform entities
    long long n_units, upb, nblk;
    int lag, stride;           // origin o is frame o * stride, the later end of a pair at that + lag (gp_plan: 0 and 1)
    int lanes_b;               // 1: the lanes hold group b, the uniform set group a
    int pad;
};

struct GpRule {
    int waves;                      // per workgroup: upb is at least this where max_pairs allows
    long long chunk, blocks;        // uniform entities per unit at most; about this many workgroups per job at most
    long long max_pairs, row_cost;  // pairs a workgroup bins between zeroing and flushing its row; what those two cost, in
};                                  // pairs: upb amortises it (0: the row is not the workgroup's)

// The plan of one job over n_orig origins, groups [a0, a0 + na) and [b0, b0 + nb) (`same`: one group, no pair i == i);
// returns its number of pairs. nblk can pass what a grid holds: the entry points refuse that.
inline uint64_t gp_plan(GpJob &J, long long n_orig, long long a0, long long na, long long b0, long long nb, bool same,
                        const GpRule &R)
{
    // lanes: the group that wastes fewer lanes of its last tile (na / tiles(na) against nb / tiles(nb)), in 128 bits
    const long long ta = (na + 63) / 64, tb = (nb + 63) / 64;
    J.lanes_b = (unsigned __int128)na * (unsigned __int128)tb < (unsigned __int128)nb * (unsigned __int128)ta;
    J.lag = 0, J.stride = 1, J.pad = 0;
    J.l0 = J.lanes_b ? b0 : a0, J.nl = J.lanes_b ? nb : na;
    J.u0 = J.lanes_b ? a0 : b0, J.nu = J.lanes_b ? na : nb;
    J.n_tiles = (J.nl + 63) / 64, J.n_jc = (J.nu + R.chunk - 1) / R.chunk;
    J.n_units = n_orig * J.n_tiles * J.n_jc;
    J.upb = 1, J.nblk = 0;
    if (J.n_units > 0) {
        const long long per_unit = 64 * std::min(J.nu, R.chunk);  // pairs of one unit at most
        const long long even = (J.n_units + R.blocks - 1) / R.blocks;
        const long long amortise = (R.row_cost + per_unit - 1) / per_unit;
        J.upb = std::min(std::max({(long long)R.waves, even, amortise}), R.max_pairs / per_unit);
        J.nblk = (J.n_units + J.upb - 1) / J.upb;
    }
    return (uint64_t)n_orig * ((uint64_t)na * (uint64_t)nb - (same ? (uint64_t)na : 0));
}

// The guard band of the f32 bin guess fma(sqrt((float)rsq), gscale, near), as pair_plan.h: |error| is relative 2.1e-7 of the bin
// number plus half an ulp of the largest value each for the addend and the fma; near = 2 x that. A band of 1 or more (very many
// bins) sends every pair to the edge table.
struct GpBand { float near, gscale; };
inline GpBand gp_band(int nbins, double bin_size)
{
    const double ulp = std::ldexp(1.0, (int)std::floor(std::log2((double)nbins + 1.0)) - 23);
    return {(float)(2.0 * ((double)nbins * 2.1e-7 + ulp) + 1.0e-5), (float)(1.0 / bin_size)};
}

}  // namespace

#ifdef __HIPCC__
#include "ctx.h"

namespace {

// ---- device part ----------------------------------------------------------------------------------------------------

// Block (x, y) works units [x * upb, (x + 1) * upb) of job job0 + y. False: the job has none for it, the whole workgroup returns.
__device__ __forceinline__ bool gp_job(const GpJob *__restrict__ jobs, int job, GpJob &J)
{
    return J = jobs[job], (long long)blockIdx.x < J.nblk;
}

// The wave's units: body(o, il, j0, jlen, self) for every lane that holds an entity — origin o, lane entity l0 + il, uniform
// entities u0 + j0 .. + jlen, of which number `self` is the lane's own (-1: none; two different groups share no entity, so one
// kernel serves every job). All but il and self are wave-uniform. Returns the lane's pairs, counted from the sizes.
template <int WAVES, long long CHUNK, class Body>
__device__ __forceinline__ unsigned gp_walk(const GpJob &J, Body body)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long ua = (long long)blockIdx.x * J.upb;
    const long long ub = ua + J.upb < J.n_units ? ua + J.upb : J.n_units;
    unsigned n_pairs = 0;
    for (long long u = ua + wave; u < ub; u += WAVES) {
        const long long c = u % J.n_jc, ot = u / J.n_jc;
        const long long o = ot / J.n_tiles, tile = ot - o * J.n_tiles;
        const long long il = tile * 64 + lane;
        const long long j0 = c * CHUNK;
        const int jlen = (int)(J.nu - j0 < CHUNK ? J.nu - j0 : CHUNK);
        if (il >= J.nl) continue;
        const long long self_ll = J.l0 + il - J.u0 - j0;
        const int self = self_ll >= 0 && self_ll < jlen ? (int)self_ll : -1;
        n_pairs += (unsigned)jlen - (self >= 0);
        body(o, il, j0, jlen, self);
    }
    return n_pairs;
}

// The bin of rsq < edges[nbins] by comparison with the exact edge table (mdhip_bin_edges); near2 = near + near.
__device__ __forceinline__ int gp_bin(double rsq, const double *__restrict__ edges, float gscale, float near,
                                      float near2, int nbins)
{
    const float g = __builtin_fmaf(__builtin_amdgcn_sqrtf((float)rsq), gscale, near);
    int k = (int)g;  // the bin, unless g is within the band above an integer: then the edges decide
    if (__builtin_amdgcn_fractf(g) < near2) {
        k = k < nbins - 1 ? k : nbins - 1;
        while (rsq < edges[k]) --k;       // edges[0] == 0 stops it
        while (rsq >= edges[k + 1]) ++k;  // rsq < edges[nbins] stops it
    }
    return k;
}

// N per-lane counters into N 64-bit totals: a butterfly, one LDS atomic per wave, one 64-bit atomic per workgroup. s_tot[N]
// is LDS zeroed before a barrier. Every thread calls this: its barrier also stands between the adds into an LDS row and the flush.
template <int N>
__device__ __forceinline__ void gp_tail(unsigned (&n)[N], unsigned *s_tot, unsigned long long *const (&total)[N])
{
    for (int sh = 32; sh; sh >>= 1)
        for (int k = 0; k < N; ++k) n[k] += __shfl_xor(n[k], sh);
    for (int k = 0; k < N; ++k)
        if ((threadIdx.x & 63) == 0 && n[k]) atomicAdd(&s_tot[k], n[k]);
    __syncthreads();
    for (int k = 0; k < N; ++k)
        if (threadIdx.x == 0 && s_tot[k]) atomicAdd(total[k], (unsigned long long)s_tot[k]);
}

// ---- host launch helpers --------------------------------------------------------------------------------------------

// The three checks that mdhip_displacement_hist makes as well. Groups: contiguous, ascending, inside a frame.
inline int gp_check_groups(mdhip_ctx *ctx, int n_groups, const int64_t *group_off, int64_t n_ent)
{
    MD_REQUIRE(n_groups == 0 || group_off, "NULL group_off");
    for (int g = 0; g < n_groups; ++g)
        MD_REQUIRE(group_off[g] >= 0 && group_off[g] <= group_off[g + 1] && group_off[g + 1] <= n_ent,
                   "group_off must ascend within [0, n_ent] (group %d)", g);
    return MDHIP_OK;
}

// A caller's edge table: the kernels walk it, so it has to start at 0 and ascend
inline int gp_check_edges(mdhip_ctx *ctx, const double *edges, int32_t nbins, int n_jobs)
{
    if (!edges || !n_jobs) return MDHIP_OK;
    MD_REQUIRE(edges[0] == 0.0, "edges[0] must be 0");
    for (int k = 0; k < nbins; ++k) MD_REQUIRE(edges[k] <= edges[k + 1], "edges must ascend (bin %d)", k);
    return MDHIP_OK;
}

// The caller's edges, or mdhip_bin_edges' own in `own`
inline int gp_edges(mdhip_ctx *ctx, const double *&edges, std::vector<double> &own, double bin_size, int32_t nbins)
{
    if (edges) return MDHIP_OK;
    own.resize((size_t)nbins + 1);
    if (mdhip_bin_edges(bin_size, nbins, own.data()) != MDHIP_OK)
        return mdhip_fail(ctx, MDHIP_EINVAL, "no bin edges for bin_size %g", bin_size);
    edges = own.data();
    return MDHIP_OK;
}

// box [F][3], the job table and edges [nbins + 1] on the device: WS_BOX, WS_AUX2, WS_TABLES
struct GpTables { double *box, *edges; GpJob *jobs; };
inline int gp_stage(mdhip_ctx *ctx, const double *box, int64_t n_frames, const std::vector<GpJob> &tab, const double *edges,
                    int32_t nbins, GpTables &d)
{
    int rc;
    if (!(d.box = (double *)mdhip_ws(ctx, WS_BOX, std::max<size_t>((size_t)n_frames * 24, 8)))) return MDHIP_ENOMEM;
    if ((rc = mdhip_h2d_small(ctx, d.box, box, (size_t)n_frames * 24))) return rc;
    if (!(d.jobs = (GpJob *)mdhip_ws(ctx, WS_AUX2, tab.size() * sizeof(GpJob)))) return MDHIP_ENOMEM;
    if ((rc = mdhip_h2d_small(ctx, d.jobs, tab.data(), tab.size() * sizeof(GpJob)))) return rc;
    if (!(d.edges = (double *)mdhip_ws(ctx, WS_TABLES, ((size_t)nbins + 1) * 8))) return MDHIP_ENOMEM;
    return mdhip_h2d_small(ctx, d.edges, edges, ((size_t)nbins + 1) * 8);
}

// launch(grid, job0) for every slice of 65 535 jobs (grid.y holds no more; a job's workgroups are the same in any slice), as
// wide as its largest job, unless that is 0; under `timer`; their number and `kernel` become last_launches / last_kernel.
template <class Launch>
inline int gp_launch(mdhip_ctx *ctx, const char *kernel, KernelTimer &timer, const std::vector<GpJob> &tab, Launch launch)
{
    constexpr int GP_MAX_Y = 65535;
    const int n_jobs = (int)tab.size();
    int launches = 0;
    for (int j0 = 0; j0 < n_jobs; j0 += GP_MAX_Y) {
        const int nj = std::min(GP_MAX_Y, n_jobs - j0);
        long long gx = 0;
        for (int j = j0; j < j0 + nj; ++j) gx = std::max(gx, tab[(size_t)j].nblk);
        if (gx == 0) continue;
        launch(dim3((unsigned)gx, (unsigned)nj), j0);
        MD_HIP(hipGetLastError());
        ++launches;
    }
    ctx->last_kernel = kernel, ctx->last_launches = launches;
    timer.stop();
    return MDHIP_OK;
}

}  // namespace
#endif  // __HIPCC__
