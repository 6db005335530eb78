// reorient.hip — molecular reorientation: molecule-fixed unit vectors and their first- and second-rank orientational
// time-correlation sums at every lag (dynamical/reorientation.py, class Reorientation; the reference has no such module).
//
// mdhip_axis_vectors: U[s][x][t] = the unit vector of series s (one molecule of one job) at frame t, from a weighted sum
//   of the differences between atoms of the molecule and its first atom (a bond: -1 / +1; a dipole: the charges). Tile,
//   job plan and launch are those of mol_tile.h, every job a class of its own; here: what a lane computes per
//   (molecule, frame).
//
// mdhip_orient_corr: sums[k][g] = sum over the series m of group g and the origins t of c and of c * c,
//   c = u_m(t) . u_m(t + k), with the geometry helpers of lag_tiles.h (tiles of 1024 lags, 4 per lane; time slabs; stages
//   of 128 steps with the window of the three components of ONE molecule in LDS). The inner loop: a lane keeps a sliding
//   window of 2 * 4 - 1 entries per component in registers, so that ONE LDS read per component and step feeds all four
//   of its lags, and u(t) (the same for every lane) arrives through uniform loads. The workgroup goes on to the next
//   molecule of its slab (OC_MS = 8 molecules of one group) with the accumulators carried along: the eight sums of a
//   lane stay in registers over slab x stage x step; the partial sums are per (molecule slab, time slab). A WAVE (256
//   lags) runs the steps up to the last origin of ITS smallest lag; those at which some of its lags have their partner
//   sample beyond the series — the last 255 at most — run the same blocks of four steps with c selected to zero for
//   such lags. Five FP64 operations per lag and step against three LDS reads per four lags: FP64-VALU bound (DESIGN
//   4.13b).
#include <algorithm>
#include <cmath>
#include <vector>

#include "call_tables.h"
#include "ctx.h"
#include "lag_tiles.h"
#include "mol_tile.h"

namespace {

// ---------------------------------------------------------------------------------------------
// axis vectors
// ---------------------------------------------------------------------------------------------

constexpr size_t AX_LDS = mt_tile_lds(3);
static_assert(AX_LDS <= 160 * 1024, "the tile must fit LDS");

struct AxJob {  // by position in the plan (= the job's number: nothing is pooled)
    long long series0;  // first series of the job
    int term0, n_terms;
};

__global__ __launch_bounds__(MT_THREADS) void axis_vectors_kernel(
    const double *__restrict__ x, const double *__restrict__ box, long long F, long long A,
    const MolClass *__restrict__ classes, int n_classes, const AxJob *__restrict__ jobs, const int *__restrict__ term_atom,
    const double *__restrict__ term_w, long long tile_base, long long ftile_base, double *__restrict__ U,
    unsigned long long *__restrict__ degenerate)
{
    extern __shared__ double s_u[];  // [3][MT_TM][MT_ROW]
    const MolTile t = mt_locate(classes, n_classes, tile_base, ftile_base, F);
    const AxJob job = jobs[t.cls.job0];
    mt_walk(t, degenerate + t.cls.job0, [&](long long a, long long f, int ff, unsigned long long &zeros) {
        double v[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double *__restrict__ plane = x + ((size_t)f * 3 + ax) * (size_t)A + a;
            const double xa = plane[0];
            const double L = box ? box[f * 3 + ax] : 0.0, half = L / 2;
            double acc = 0.0;
            for (int k = 0; k < job.n_terms; ++k) {
                double d = plane[term_atom[job.term0 + k]] - xa;
                if (box) d = mt_wrap(d, L, half);
                const double p = term_w[job.term0 + k] * d;
                acc = k == 0 ? p : acc + p;
            }
            v[ax] = acc;
        }
        const double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        double u[3];
        if (n2 == 0.0) {
            u[0] = u[1] = u[2] = 0.0;
            ++zeros;
        } else if (!(__builtin_fabs(n2) < __builtin_inf())) {
            u[0] = u[1] = u[2] = __builtin_nan("");
        } else {
            const double r = __builtin_sqrt(n2);
            u[0] = v[0] / r, u[1] = v[1] / r, u[2] = v[2] / r;
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) s_u[mt_at(ax, t.lane, ff)] = u[ax];
    });
    __syncthreads();
    mt_store<3>(t, s_u, job.series0, F, U);
}

// ---------------------------------------------------------------------------------------------
// orientational correlation sums
// ---------------------------------------------------------------------------------------------

using OC = lagt::OrientTiles;
constexpr int OC_THREADS = OC::THREADS, OC_LPT = OC::LPT, OC_TT = OC::TT, OC_ROW = OC::ROW;
constexpr int OC_MS = 8;                        // molecules per slab
constexpr int OC_MAX_GROUPS = 16;
constexpr long long OC_MAX_MSLABS = 32768;      // beyond that the slabs grow (OC_MS, 2 OC_MS, ...)
constexpr int OC_RESIDENT = 4;                  // workgroups per CU: at most 128 registers per lane (five would spill)
static_assert(OC_TT % OC_LPT == 0, "stages are whole blocks of OC_LPT steps");
static_assert((size_t)3 * OC_LPT * OC_ROW * 8 <= 160 * 1024, "the staged windows must fit LDS");

struct OcGroups {
    long long off[OC_MAX_GROUPS + 1];    // first series of every group
    long long slab0[OC_MAX_GROUPS + 1];  // first molecule slab of every group
};

// c = u(t) . u(t + k) from the origin values p and the window entries w
#define OC_DOT(PX, PY, PZ, WX, WY, WZ) __builtin_fma(PZ, WZ, __builtin_fma(PY, WY, (PX) * (WX)))

// partial[mslab][tslab][q][2] = sum over the molecules of the slab and the slab's time range of c, c * c at lag lag0 + q
__global__ __launch_bounds__(OC_THREADS, OC_RESIDENT) void orient_corr_kernel(const double *__restrict__ U, long long n,
                                                                 OcGroups groups, int n_groups, int ms, long long lag0,
                                                                 long long n_lags, int n_tiles, int n_tslabs,
                                                                 double *__restrict__ partial)
{
    __shared__ double s_w[3 * OC_LPT * OC_ROW];  // [3][OC_LPT][OC_ROW]
    const int tid = threadIdx.x;
    const int pair_id = blockIdx.x, tslab = blockIdx.y;
    const long long mslab = blockIdx.z;
    const int wave_lo = __builtin_amdgcn_readfirstlane(tid >> 6) * 64 * OC_LPT, wave_hi = wave_lo + 64 * OC_LPT;
    int g = 0;  // the last group whose first slab is not beyond this one (empty groups have none)
    while (g + 1 < n_groups && groups.slab0[g + 1] <= mslab) ++g;
    const long long m_lo = groups.off[g] + (mslab - groups.slab0[g]) * ms;
    const long long m_hi = m_lo + ms < groups.off[g + 1] ? m_lo + ms : groups.off[g + 1];

    for (int half = 0; half < 2; ++half) {
        const int tile = OC::tile_of(pair_id, half, n_tiles);
        if (half == 1 && tile == pair_id) break;  // the middle tile once
        const long long Q0 = OC::first_lag(tile), K0 = lag0 + Q0;
        if (Q0 >= n_lags) continue;
        long long t_lo, t_hi;
        OC::slab_range(n - K0, n_tslabs, tslab, t_lo, t_hi);
        double acc1[OC_LPT], acc2[OC_LPT];
#pragma unroll
        for (int j = 0; j < OC_LPT; ++j) acc1[j] = acc2[j] = 0.0;

        for (long long m = m_lo; m < m_hi; ++m) {
            const double *const Ux = U + (size_t)m * 3 * (size_t)n, *const Uy = Ux + n, *const Uz = Uy + n;
            for (long long T0 = t_lo; T0 < t_hi; T0 += OC_TT) {
                __syncthreads();
                // stage u[x][T0+K0 .. T0+K0+AW), zero beyond the series (such entries are never used: see `fast` and `ok`);
                // one bound test and one slot for the three components, not three lagt stages
                for (int i = tid; i < OC::AW; i += OC_THREADS) {
                    const long long at = T0 + K0 + i;
                    const int slot = (i % OC_LPT) * OC_ROW + i / OC_LPT;
                    const bool in = at < n;
                    s_w[slot] = in ? Ux[at] : 0.0;
                    s_w[OC_LPT * OC_ROW + slot] = in ? Uy[at] : 0.0;
                    s_w[2 * OC_LPT * OC_ROW + slot] = in ? Uz[at] : 0.0;
                }
                __syncthreads();
                const long long in_stage = OC::steps(t_hi, T0);
                // The steps of this WAVE (lags K0 + wave_lo .. K0 + wave_hi of the tile): those at which its smallest lag
                // still has its partner inside the series — the tile's time range is that of ITS smallest lag — and
                // none when all its lags lie beyond the requested ones (it only helps to stage then)
                const long long some = Q0 + wave_lo >= n_lags ? 0 : n - K0 - wave_lo - T0;
                const int tt_count = (int)(some <= 0 ? 0 : (some < in_stage ? some : in_stage));
                // ... and those at which EVERY lag of the wave has: T0 + tt + K0 + wave_hi - 1 <= n - 1. Both counts must
                // equal OC::fast_steps (lag_tiles.h has the rule and why): (n, K0, wave_lo + 1, T0, in_stage, 1) and
                // (n, K0, wave_hi, T0, tt_count, OC_LPT)
                const long long room = n - K0 - wave_hi - T0 + 1;
                const int fast = (int)(room <= 0 ? 0 : (room < tt_count ? room : tt_count)) & ~(OC_LPT - 1);
                const int blocks_end = tt_count & ~(OC_LPT - 1);
                int tt = 0;
                if (blocks_end > 0) {
                    // Lane window: entries OC_LPT tid + tt + j. A block of OC_LPT steps uses the entries j = 0 ..
                    // 2 OC_LPT - 2: the first OC_LPT - 1 are kept from the block before, the others are read here.
                    double w[3][2 * OC_LPT - 1];
#pragma unroll
                    for (int x = 0; x < 3; ++x)
#pragma unroll
                        for (int j = 0; j < OC_LPT - 1; ++j) w[x][j] = s_w[(x * OC_LPT + j) * OC_ROW + tid];
                    // GUARD: a lag whose partner sample does not exist adds c = 0 (selected, never multiplied: a NaN or an
                    // infinity at the origin must not reach it); `valid` = the entries of the lane's window that exist
#define OC_BLOCK(GUARD, VALID)                                                                                 \
    _Pragma("unroll") for (int s = 0; s < OC_LPT; ++s)                                                         \
    {                                                                                                          \
        const double px = Ux[T0 + tt + s], py = Uy[T0 + tt + s], pz = Uz[T0 + tt + s];                         \
        _Pragma("unroll") for (int j = 0; j < OC_LPT; ++j)                                                     \
        {                                                                                                      \
            double c = OC_DOT(px, py, pz, w[0][s + j], w[1][s + j], w[2][s + j]);                              \
            if (GUARD) c = s + j < (VALID) ? c : 0.0;                                                          \
            acc1[j] += c;                                                                                      \
            acc2[j] = __builtin_fma(c, c, acc2[j]);                                                            \
        }                                                                                                      \
    }
                    for (; tt < blocks_end; tt += OC_LPT) {
                        const int col = tid + tt / OC_LPT;
#pragma unroll
                        for (int x = 0; x < 3; ++x)
#pragma unroll
                            for (int s = 0; s < OC_LPT; ++s) {
                                const int e = OC_LPT - 1 + s;
                                w[x][e] = s_w[(x * OC_LPT + e % OC_LPT) * OC_ROW + col + e / OC_LPT];
                            }
                        if (tt < fast) {
                            OC_BLOCK(false, 0)
                        } else {
                            // the last steps of the wave's range, where only some of its lags still have a partner
                            const long long rest = n - T0 - K0 - (long long)OC_LPT * tid - tt;
                            const int valid = (int)(rest < 0 ? 0 : (rest < 2 * OC_LPT ? rest : 2 * OC_LPT));
                            OC_BLOCK(true, valid)
                        }
#undef OC_BLOCK
#pragma unroll
                        for (int x = 0; x < 3; ++x)
#pragma unroll
                            for (int j = 0; j < OC_LPT - 1; ++j) w[x][j] = w[x][j + OC_LPT];
                    }
                }
                // the up to OC_LPT - 1 steps behind the last whole block, one by one
                for (; tt < tt_count; ++tt) {
                    const double px = Ux[T0 + tt], py = Uy[T0 + tt], pz = Uz[T0 + tt];
#pragma unroll
                    for (int j = 0; j < OC_LPT; ++j) {
                        const int i = OC_LPT * tid + tt + j;
                        const int slot = (i % OC_LPT) * OC_ROW + i / OC_LPT;
                        const double c = OC_DOT(px, py, pz, s_w[slot], s_w[OC_LPT * OC_ROW + slot],
                                                s_w[2 * OC_LPT * OC_ROW + slot]);
                        if (T0 + K0 + i < n) {
                            acc1[j] += c;
                            acc2[j] = __builtin_fma(c, c, acc2[j]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < OC_LPT; ++j) {
            const long long q = OC::lane_lag(Q0, tid, j);
            if (q >= n_lags) continue;
            const size_t at = (((size_t)mslab * (size_t)n_tslabs + (size_t)tslab) * (size_t)n_lags + (size_t)q) * 2;
            partial[at] = acc1[j];
            partial[at + 1] = acc2[j];
        }
    }
}
#undef OC_DOT

// sums[lag0 + q][g][c] = the sum over the (molecule slab, time slab) partial sums of group g, in order
__global__ void orient_corr_finish_kernel(const double *__restrict__ partial, double *__restrict__ sums,
                                          OcGroups groups, int G, int n_tslabs, long long lag0, long long n_lags)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = n_lags * 2;
    if (idx >= row * G) return;
    const int g = (int)(idx / row);
    const long long r = idx - (long long)g * row;  // 2 q + c
    const long long s0 = groups.slab0[g] * n_tslabs, s1 = groups.slab0[g + 1] * n_tslabs;
    double s = 0.0;
    for (long long slab = s0; slab < s1; ++slab) s += partial[(size_t)slab * (size_t)row + (size_t)r];
    sums[((size_t)(lag0 + (r >> 1)) * G + g) * 2 + (size_t)(r & 1)] = s;
}

}  // namespace

extern "C" {

int mdhip_axis_vectors(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                       const double *box, int n_jobs, const int64_t *job_atom0, const int64_t *job_mols,
                       const int32_t *job_len, const int64_t *term_off, const int32_t *term_atom, const double *term_w,
                       double *U, int U_on_device, uint64_t *degenerate)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_jobs >= 1 && n_jobs <= (1 << 20), "n_jobs must be in [1, 2^20]");
    MD_REQUIRE(n_frames >= 1 && n_atoms >= 1, "n_frames and n_atoms must be positive");
    MD_REQUIRE(n_atoms < (1ll << 40) && n_frames < (1ll << 31) && n_frames < (1ll << 40) / n_atoms, "trajectory too large");
    MD_REQUIRE(x && job_atom0 && job_mols && job_len && term_off && term_atom && term_w && U && degenerate, "NULL array");
    MD_REQUIRE(term_off[0] == 0, "term_off must start at 0");
    const MolPlan plan = mol_plan(n_jobs, job_atom0, job_mols, job_len, n_atoms, n_frames, false, 1);
    std::vector<AxJob> jobs((size_t)n_jobs);
    for (int j = 0; j < plan.checked_jobs(); ++j) {
        const long long len = job_len[j], t0 = term_off[j], t1 = term_off[j + 1];
        MD_REQUIRE(t1 > t0 && t1 - t0 < len && t1 <= (1ll << 30), "job %d needs between 1 and job_len - 1 terms", j);
        if (int rc = mt_terms_ascend(ctx, j, term_atom, t0, t1, len)) return rc;
        jobs[(size_t)j] = {plan.series0[(size_t)j], (int)t0, (int)(t1 - t0)};
    }
    int rc;
    if ((rc = mt_plan_error(ctx, plan, n_atoms))) return rc;
    MolIo io;
    if ((rc = io.open(ctx, n_frames, n_atoms, x, x_on_device, box, U, U_on_device, plan.series))) return rc;
    const size_t n_terms = (size_t)term_off[n_jobs];
    const MolClass *d_cls;
    const AxJob *d_jobs;
    const double *d_w;
    const int *d_atom;
    unsigned long long *d_deg;
    CallTables tab;
    tab.add(plan.classes.data(), (size_t)n_jobs, &d_cls);
    tab.add(jobs.data(), (size_t)n_jobs, &d_jobs);
    tab.add(term_w, n_terms, &d_w);
    tab.add(term_atom, n_terms, &d_atom);
    tab.add_zeroed((size_t)n_jobs, &d_deg);
    if ((rc = upload_tables(ctx, tab, WS_TABLES))) return rc;
    MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(axis_vectors_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)AX_LDS));
    KernelTimer timer(ctx, 0);
    rc = mt_launch(ctx, "axis_vectors_kernel", timer, plan.tiles, n_frames, [&](dim3 grid, long long t0, long long ft0) {
        hipLaunchKernelGGL(axis_vectors_kernel, grid, dim3(MT_THREADS), AX_LDS, ctx->stream, io.x, io.box,
                           (long long)n_frames, (long long)n_atoms, d_cls, n_jobs, d_jobs, d_atom, d_w, t0, ft0, io.U.dev,
                           d_deg);
    });
    if (rc) return rc;
    if ((rc = io.U.deliver(cs))) return rc;
    if ((rc = mdhip_result(cs, degenerate, d_deg, (size_t)n_jobs * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

int mdhip_orient_corr(mdhip_ctx *ctx, int64_t n, int64_t n_series, const double *U, int U_on_device, int n_groups,
                      const int64_t *group_off, int64_t max_lag, double *sums, int sums_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_groups >= 1 && n_groups <= OC_MAX_GROUPS, "n_groups must be in [1, %d]", OC_MAX_GROUPS);
    MD_REQUIRE(n >= 1 && n < (1LL << 29), "series of 1 .. 2^29 samples are supported");
    MD_REQUIRE(max_lag >= 0 && max_lag <= n - 1, "max_lag must be in [0, n - 1]");
    MD_REQUIRE(n_series >= 0 && n_series < (1LL << 40) / n, "n_series must not be negative (and n_series * n below 2^40)");
    MD_REQUIRE(group_off && sums && (n_series == 0 || U), "NULL array");
    for (int g = 0; g < n_groups; ++g)
        MD_REQUIRE(group_off[g] >= 0 && group_off[g] <= group_off[g + 1] && group_off[g + 1] <= n_series,
                   "group_off must ascend within [0, n_series] (group %d)", g);
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const int G = n_groups;
    const long long n_lags_all = max_lag + 1;
    const size_t u_bytes = (size_t)n_series * 3 * (size_t)n * 8;
    const double *d_U = (const double *)mdhip_stage(ctx, WS_XYZ_I, U, u_bytes, U_on_device || u_bytes == 0, &rc);
    if (rc) return rc;
    const size_t out_b = (size_t)n_lags_all * G * 2 * 8;
    double *d_out = sums;
    if (!sums_on_device) {
        d_out = (double *)mdhip_ws(ctx, WS_OUT, out_b);
        if (!d_out) return MDHIP_ENOMEM;
    }
    // molecule slabs: OC_MS molecules of one group each; larger ones when there would be more than OC_MAX_MSLABS
    OcGroups groups;
    int ms = OC_MS;
    long long n_mslabs;
    for (;; ms *= 2) {
        n_mslabs = 0;
        for (int g = 0; g <= OC_MAX_GROUPS; ++g) {
            const int gg = g < G ? g : G;
            groups.off[g] = group_off[gg];
            groups.slab0[g] = n_mslabs;
            if (g < G) n_mslabs += (group_off[g + 1] - group_off[g] + ms - 1) / ms;
        }
        if (n_mslabs <= OC_MAX_MSLABS) break;
    }
    // time slabs when the molecule slabs alone do not fill the rounds (a workgroup of a paired short tile is done long
    // before one of a full tile, and the last round runs at the pace of the slowest); the lag range goes in chunks of
    // whole tiles, each pairing its own tiles. Every (slab, lag) of a chunk is written: nothing to clear.
    const long long M = std::max<long long>(n_mslabs, 1);
    const lagt::Plan pl = lagt::orient_plan(n, n_lags_all, n_mslabs, ctx->cu_count, lagt::PARTIAL_BUDGET);
    const int n_tslabs = pl.n_slabs;
    const long long chunk_lags = std::min<long long>(pl.chunk * OC::KT, n_lags_all);
    MD_WS(d_part, double, WS_PART, (size_t)(M * n_tslabs) * (size_t)chunk_lags * 2 * 8);
    KernelTimer timer(ctx, 0);
    int launches = 0;
    rc = lagt::run_chunks(
        ctx, n_lags_all, chunk_lags,
        [&](long long lag0, long long n_lags) {
            if (n_mslabs == 0) return MDHIP_OK;
            const int n_tiles = (int)OC::n_tiles(n_lags);
            const dim3 grid((unsigned)((n_tiles + 1) / 2), (unsigned)n_tslabs, (unsigned)n_mslabs);
            hipLaunchKernelGGL(orient_corr_kernel, grid, dim3(OC_THREADS), 0, ctx->stream, d_U, (long long)n, groups, G, ms,
                               lag0, n_lags, n_tiles, n_tslabs, d_part);
            ++launches;
            return MDHIP_OK;
        },
        [&](long long lag0, long long n_lags) {
            const unsigned fin = (unsigned)((n_lags * 2 * G + 255) / 256);
            hipLaunchKernelGGL(orient_corr_finish_kernel, dim3(fin), dim3(256), 0, ctx->stream, d_part, d_out, groups, G,
                               n_tslabs, lag0, n_lags);
            return MDHIP_OK;
        });
    if (rc) return rc;
    ctx->last_kernel = "orient_corr_kernel";
    ctx->last_launches = launches;
    timer.stop();
    if (!sums_on_device && (rc = mdhip_result(cs, sums, d_out, out_b, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
