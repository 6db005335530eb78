// collective.hip — Einstein-Helfand conductivity: collective charge displacements and their cross-displacement
// correlation at every lag (Conductivity.einstein / nernst, which the reference leaves as `pass`:
// dynamical/conductivity.py:399-403).
//
// mdhip_collective_displacement: P[g][x][t] = sum over the entities e of group g of c_e * (r[t][x][e] - r[0][x][e]).
//   One workgroup per (frame, axis, group): lane i adds the entities i, i + 256, ... of the group in order (the product
//   and the sum unfused), then a fixed tree over the 256 partial sums. One read of the trajectory: HBM-bound.
//
// mdhip_cross_msd: out[k][a][b] = sum_t sum_x (P[a][x][t+k] - P[a][x][t]) * (P[b][x][t+k] - P[b][x][t]) / (n - k).
//   Difference form throughout (subtract, then multiply): FP64-VALU bound, n * max_lag / 2 window positions with
//   3 G subtractions and 3 G (G + 1) / 2 fused multiply-adds each, with the geometry helpers of lag_tiles.h (tiles of 512
//   lags, 2 per lane; time slabs; stages of 128 steps with the windows of every series of the workgroup's groups in
//   LDS). The inner loop: a lane keeps a sliding window of two entries per series in registers, so that one LDS read
//   per series and step feeds both of its lags, and P[.][t] (the same for every lane) arrives through uniform loads.
//   ALL pair accumulators of a lane's lags stay in registers: one staged window feeds every group pair. Groups go in
//   tiles of four: up to four groups are one launch (10 pairs x 2 lags, twice that with the |term| sums); more groups
//   take one launch per pair of tiles (A <= B: the diagonal ones as above, the others all 16 pairs of 4 x 4 groups).
//   The finish kernel divides and mirrors. The steps at which some lag of a WAVE (128 lags) has its partner sample
//   beyond the series — the last 127 time origins of its lags at most — run in a predicated loop.
#include <algorithm>

#include "ctx.h"
#include "lag_tiles.h"

namespace {

// ---------------------------------------------------------------------------------------------
// collective displacement
// ---------------------------------------------------------------------------------------------

constexpr int CD_THREADS = 256;
constexpr int CD_MAX_GROUPS = 16;
constexpr long long CD_MAX_X = 1 << 20;  // frames per launch

struct CdGroups {
    long long off[CD_MAX_GROUPS + 1];
};

// Block (x, y, z): frame f0 + x, axis y, group z.
__global__ __launch_bounds__(CD_THREADS) void collective_kernel(const double *__restrict__ r,
                                                                const double *__restrict__ c, long long F,
                                                                long long E, long long f0, CdGroups groups,
                                                                double *__restrict__ P,
                                                                double *__restrict__ weighted)
{
    __shared__ double s_red[CD_THREADS];
    const long long f = f0 + blockIdx.x;
    const int axis = blockIdx.y, g = blockIdx.z;
    const long long e0 = groups.off[g], e1 = groups.off[g + 1];
    const double *__restrict__ now = r + ((size_t)f * 3 + axis) * (size_t)E;
    const double *__restrict__ first = r + (size_t)axis * (size_t)E;
    double *__restrict__ w = weighted ? weighted + ((size_t)f * 3 + axis) * (size_t)E : nullptr;
    double s = 0.0;
    for (long long e = e0 + threadIdx.x; e < e1; e += CD_THREADS) {
        const double v = c[e] * (now[e] - first[e]);
        if (w) w[e] = v;
        s += v;
    }
    s_red[threadIdx.x] = s;
    __syncthreads();
    for (int half = CD_THREADS / 2; half; half >>= 1) {
        if ((int)threadIdx.x < half) s_red[threadIdx.x] += s_red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) P[((size_t)g * 3 + axis) * (size_t)F + f] = s_red[0];
}

// ---------------------------------------------------------------------------------------------
// cross-displacement correlation
// ---------------------------------------------------------------------------------------------

using CM = lagt::CrossMsdTiles;
constexpr int CM_THREADS = CM::THREADS, CM_LPT = CM::LPT, CM_ROW = CM::ROW;
constexpr int CM_GT = 4;                         // groups per tile
constexpr int CM_MAX_GROUPS = 16;

// d <- the displacements of one lag from the window entries u and the origin values pt; acc += d_a * d_b per pair and axis
template <int NA, int NB, bool DIAG, bool ABS, int NS, int NP>
__device__ __forceinline__ void cm_accumulate(const double (&d)[NS], double (&acc)[NP], double (&acc_abs)[NP])
{
    int p = 0;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
        for (int b = DIAG ? a : 0; b < NB; ++b, ++p) {
            const int ia = 3 * a, ib = DIAG ? 3 * b : 3 * NA + 3 * b;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                acc[p] = __builtin_fma(d[ia + x], d[ib + x], acc[p]);
                if (ABS) acc_abs[p] = __builtin_fma(__builtin_fabs(d[ia + x]), __builtin_fabs(d[ib + x]), acc_abs[p]);
            }
        }
    }
}

// partial[slab][q][a][b] (a <= b, G x G rows) = sum over the slab's time range of sum_x d_a d_b at lag lag0 + q, for the
// groups ga0 .. ga0 + NA (a) and gb0 .. gb0 + NB (b; DIAG: the same groups, pairs a <= b only)
template <int NA, int NB, bool DIAG, bool ABS>
__global__ __launch_bounds__(CM_THREADS) void cross_msd_kernel(const double *__restrict__ P, long long n, int G,
                                                               int ga0, int gb0, long long lag0, long long n_lags,
                                                               int n_tiles, int n_slabs, double *__restrict__ partial,
                                                               double *__restrict__ partial_abs)
{
    constexpr int NS = 3 * (DIAG ? NA : NA + NB);
    constexpr int NP = DIAG ? NA * (NA + 1) / 2 : NA * NB;
    extern __shared__ double s_w[];  // [NS][2][CM_ROW]
    const int tid = threadIdx.x;
    const int pair_id = blockIdx.x, slab = blockIdx.y;
    const int wave_hi = (__builtin_amdgcn_readfirstlane(tid >> 6) + 1) * 64 * CM_LPT;
    // series s of the workgroup: the 3 NA series of tile A, then (unless DIAG) the 3 NB series of tile B
    const double *const Pa = P + (size_t)(3 * ga0) * (size_t)n, *const Pb = P + (size_t)(3 * gb0) * (size_t)n;
#define CM_SERIES(s) ((s) < 3 * NA ? Pa + (size_t)(s) * (size_t)n : Pb + (size_t)((s) - 3 * NA) * (size_t)n)

    for (int half = 0; half < 2; ++half) {
        const int tile = CM::tile_of(pair_id, half, n_tiles);
        if (half == 1 && tile == pair_id) break;  // the middle tile once
        const long long Q0 = CM::first_lag(tile), K0 = lag0 + Q0;
        if (Q0 >= n_lags) continue;
        long long t_lo, t_hi;
        CM::slab_range(n - K0, n_slabs, slab, t_lo, t_hi);
        double acc[CM_LPT][NP], acc_abs[CM_LPT][NP];
#pragma unroll
        for (int j = 0; j < CM_LPT; ++j)
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[j][p] = acc_abs[j][p] = 0.0;

        for (long long T0 = t_lo; T0 < t_hi; T0 += CM::TT) {
            __syncthreads();
            // (entries beyond the series are never used: see `fast` and `ok`)
#pragma unroll
            for (int s = 0; s < NS; ++s) CM::stage(s_w, s, CM_SERIES(s), T0 + K0, n, tid);
            __syncthreads();
            const int tt_count = (int)CM::steps(t_hi, T0);
            // steps at which every lag of this WAVE (lags K0 .. K0 + wave_hi of the tile at most) still has its partner:
            // these two lines must equal CM::fast_steps(n, K0, wave_hi, T0, tt_count, 4) (lag_tiles.h has the rule and why)
            const long long room = n - K0 - wave_hi - T0 + 1;
            const int fast = (int)(room <= 0 ? 0 : (room < tt_count ? room : tt_count)) & ~3;
            const double *base = s_w + tid;
            int tt = 0;
            if (fast > 0) {
                // Lane window: entries 2 tid + tt + j. Two steps use the entries j = 0, 1 (U0, U1) and j = 2 (V0); V0 and
                // V1 (j = 2, 3: the next two steps' U) are requested before the arithmetic. U and V swap roles every two
                // steps, so no register is ever moved.
                double wa0[NS], wa1[NS], wb0[NS], wb1[NS], d[NS], pt[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    wa0[s] = base[(2 * s) * CM_ROW];
                    wa1[s] = base[(2 * s + 1) * CM_ROW];
                }
#define CM_LAG(W, J)                                                                          \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) d[s] = W[s] - pt[s];                       \
    cm_accumulate<NA, NB, DIAG, ABS, NS, NP>(d, acc[J], acc_abs[J]);
#define CM_TWO_STEPS(U0, U1, V0, V1, TT)                                                      \
    {                                                                                         \
        const int col = ((TT) >> 1) + 1;                                                      \
        _Pragma("unroll") for (int s = 0; s < NS; ++s)                                        \
        {                                                                                     \
            V0[s] = base[(2 * s) * CM_ROW + col];                                             \
            V1[s] = base[(2 * s + 1) * CM_ROW + col];                                         \
        }                                                                                     \
        _Pragma("unroll") for (int s = 0; s < NS; ++s) pt[s] = CM_SERIES(s)[T0 + (TT)];       \
        CM_LAG(U0, 0)                                                                         \
        CM_LAG(U1, 1)                                                                         \
        _Pragma("unroll") for (int s = 0; s < NS; ++s) pt[s] = CM_SERIES(s)[T0 + (TT) + 1];   \
        CM_LAG(U1, 0)                                                                         \
        CM_LAG(V0, 1)                                                                         \
    }
                for (; tt < fast; tt += 4) {
                    CM_TWO_STEPS(wa0, wa1, wb0, wb1, tt)
                    CM_TWO_STEPS(wb0, wb1, wa0, wa1, tt + 2)
                }
#undef CM_TWO_STEPS
#undef CM_LAG
            }
            // the steps behind them, one by one: a lag whose partner sample does not exist adds nothing
            for (; tt < tt_count; ++tt) {
                double pt[NS], d[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) pt[s] = CM_SERIES(s)[T0 + tt];
#pragma unroll
                for (int j = 0; j < CM_LPT; ++j) {
                    const int i = 2 * tid + tt + j;
                    const bool ok = T0 + K0 + i < n;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        double w = s_w[CM::slot(i, s)];
                        asm volatile("" : "+v"(w));  // (the read itself is unconditional: one select, no branch per series)
                        d[s] = ok ? w - pt[s] : 0.0;
                    }
                    cm_accumulate<NA, NB, DIAG, ABS, NS, NP>(d, acc[j], acc_abs[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CM_LPT; ++j) {
            const long long q = CM::lane_lag(Q0, tid, j);
            if (q >= n_lags) continue;
            const size_t row = ((size_t)slab * (size_t)n_lags + (size_t)q) * (size_t)(G * G);
            int p = 0;
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int b = DIAG ? a : 0; b < NB; ++b, ++p) {
                    const size_t at = row + (size_t)(ga0 + a) * G + (size_t)(gb0 + b);
                    partial[at] = acc[j][p];
                    if (ABS) partial_abs[at] = acc_abs[j][p];
                }
        }
    }
#undef CM_SERIES
}

// out[lag0 + q][a][b] = (sum over the slabs, in order, of partial[slab][q][min(a, b)][max(a, b)]) / (n - (lag0 + q))
__global__ void cross_msd_finish_kernel(const double *__restrict__ partial, double *__restrict__ out, long long n,
                                        int G, long long lag0, long long n_lags, int n_slabs)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int GG = G * G;
    if (idx >= n_lags * GG) return;
    const long long q = idx / GG;
    const int ab = (int)(idx - q * GG), a = ab / G, b = ab - a * G;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const size_t at = (size_t)q * GG + (size_t)lo * G + hi;
    double s = 0.0;
    for (int r = 0; r < n_slabs; ++r) s += partial[(size_t)r * (size_t)n_lags * GG + at];
    out[(size_t)(lag0 + q) * GG + ab] = s / (double)(n - (lag0 + q));
}

template <int NA, int NB, bool DIAG, bool ABS>
int cm_launch(mdhip_ctx *ctx, dim3 grid, const double *d_P, long long n, int G, int ga0, int gb0, long long lag0,
              long long n_lags, int n_tiles, int n_slabs, double *d_part, double *d_part_abs)
{
    constexpr int NS = 3 * (DIAG ? NA : NA + NB);
    constexpr size_t lds_b = (size_t)NS * 2 * CM_ROW * 8;
    static_assert(lds_b <= 160 * 1024, "the staged windows must fit LDS");
    if (lds_b > 65536)
        MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(cross_msd_kernel<NA, NB, DIAG, ABS>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    hipLaunchKernelGGL((cross_msd_kernel<NA, NB, DIAG, ABS>), grid, dim3(CM_THREADS), lds_b, ctx->stream, d_P, n, G, ga0,
                       gb0, lag0, n_lags, n_tiles, n_slabs, d_part, d_part_abs);
    MD_HIP(hipGetLastError());
    return MDHIP_OK;
}

template <bool ABS>
int cm_launch_tiles(mdhip_ctx *ctx, dim3 grid, const double *d_P, long long n, int G, int ga0, int na, int gb0, int nb,
                    long long lag0, long long n_lags, int n_tiles, int n_slabs, double *d_part, double *d_part_abs)
{
#define CM_GO(NA, NB, DIAG)                                                                                          \
    return cm_launch<NA, NB, DIAG, ABS>(ctx, grid, d_P, n, G, ga0, gb0, lag0, n_lags, n_tiles, n_slabs, d_part,      \
                                        d_part_abs)
    if (ga0 == gb0) {
        switch (na) {
        case 1: CM_GO(1, 1, true);
        case 2: CM_GO(2, 2, true);
        case 3: CM_GO(3, 3, true);
        default: CM_GO(4, 4, true);
        }
    }
    // (A < B: tile A is a full one)
    switch (nb) {
    case 1: CM_GO(4, 1, false);
    case 2: CM_GO(4, 2, false);
    case 3: CM_GO(4, 3, false);
    default: CM_GO(4, 4, false);
    }
#undef CM_GO
}

}  // namespace

extern "C" {

int mdhip_collective_displacement(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                                  const double *weight, double scale, int n_groups, const int64_t *group_off,
                                  double *P, int P_on_device, double *weighted_dev)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_groups >= 1 && n_groups <= CD_MAX_GROUPS, "n_groups must be in [1, %d]", CD_MAX_GROUPS);
    MD_REQUIRE(n_frames >= 1 && n_ent >= 0, "n_frames must be positive, n_ent not negative");
    MD_REQUIRE(n_ent < (1ll << 40) && n_frames < (1ll << 31) && n_frames < (1ll << 40) / std::max<int64_t>(n_ent, 1),
               "trajectory too large");
    MD_REQUIRE(group_off && P && (n_ent == 0 || (r && weight)), "NULL array");
    for (int g = 0; g < n_groups; ++g)
        MD_REQUIRE(group_off[g] >= 0 && group_off[g] <= group_off[g + 1] && group_off[g + 1] <= n_ent,
                   "group_off must ascend within [0, n_ent] (group %d)", g);
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const size_t r_bytes = (size_t)n_frames * 3 * (size_t)n_ent * 8;
    const double *d_r = (const double *)mdhip_stage(ctx, WS_XYZ_I, r, r_bytes, r_on_device || r_bytes == 0, &rc);
    if (rc) return rc;
    // c_e = weight[e] * scale, formed once here
    MD_WS(d_c, double, WS_TABLES, std::max<size_t>((size_t)n_ent, 1) * 8);
    if (n_ent) {
        MD_PIN(h_c, double, (size_t)n_ent * 8);
        for (int64_t e = 0; e < n_ent; ++e) h_c[e] = weight[e] * scale;
        if ((rc = mdhip_copy_small(ctx, d_c, h_c, (size_t)n_ent * 8, hipMemcpyHostToDevice))) return rc;
    }
    CdGroups groups;
    for (int g = 0; g <= CD_MAX_GROUPS; ++g) groups.off[g] = group_off[g < n_groups ? g : n_groups];
    const size_t p_bytes = (size_t)n_groups * 3 * (size_t)n_frames * 8;
    double *d_P = P;
    if (!P_on_device) {
        d_P = (double *)mdhip_ws(ctx, WS_OUT, p_bytes);
        if (!d_P) return MDHIP_ENOMEM;
    }
    KernelTimer timer(ctx, 1);
    // entities that belong to no group weigh nothing
    if (weighted_dev && r_bytes && (group_off[0] != 0 || group_off[n_groups] != n_ent))
        MD_HIP(hipMemsetAsync(weighted_dev, 0, r_bytes, ctx->stream));
    // (a launch holds at most 2^32 threads along x: long trajectories go in slices of frames)
    for (long long f0 = 0; f0 < n_frames; f0 += CD_MAX_X) {
        const unsigned gx = (unsigned)std::min<long long>(CD_MAX_X, n_frames - f0);
        hipLaunchKernelGGL(collective_kernel, dim3(gx, 3, (unsigned)n_groups), dim3(CD_THREADS), 0, ctx->stream, d_r,
                           d_c, (long long)n_frames, (long long)n_ent, f0, groups, d_P, weighted_dev);
        MD_HIP(hipGetLastError());
    }
    ctx->last_kernel = "collective_kernel";
    timer.stop();
    if (!P_on_device && (rc = mdhip_result(cs, P, d_P, p_bytes, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

int mdhip_cross_msd(mdhip_ctx *ctx, int64_t n, int n_groups, const double *P, int P_on_device, int64_t max_lag,
                    double *out, double *abs_out, int out_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_groups >= 1 && n_groups <= CM_MAX_GROUPS, "n_groups must be in [1, %d]", CM_MAX_GROUPS);
    MD_REQUIRE(n >= 1 && n < (1LL << 29), "series of 1 .. 2^29 samples are supported");
    MD_REQUIRE(max_lag >= 0 && max_lag <= n - 1, "max_lag must be in [0, n - 1]");
    MD_REQUIRE(P && out, "NULL array");
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const int G = n_groups, GG = G * G;
    const bool want_abs = abs_out != nullptr;
    const long long n_lags_all = max_lag + 1;
    const double *d_P = (const double *)mdhip_stage(ctx, WS_XYZ_I, P, (size_t)G * 3 * (size_t)n * 8, P_on_device, &rc);
    if (rc) return rc;
    const size_t out_b = (size_t)n_lags_all * GG * 8;
    double *d_out = out, *d_abs = abs_out;
    if (!out_on_device) {
        d_out = (double *)mdhip_ws(ctx, WS_OUT, out_b);
        if (!d_out) return MDHIP_ENOMEM;
        if (want_abs) {
            d_abs = (double *)mdhip_ws(ctx, WS_OUT2, out_b);
            if (!d_abs) return MDHIP_ENOMEM;
        }
    }
    // the lag range goes in chunks of whole tiles, each pairing its own tiles; only a <= b is written
    const int n_gt = (G + CM_GT - 1) / CM_GT;
    const lagt::Plan pl = lagt::cross_msd_plan(n, n_lags_all, G, want_abs, ctx->cu_count, lagt::PARTIAL_BUDGET);
    const int n_slabs = pl.n_slabs;
    const long long chunk_lags = std::min<long long>(pl.chunk * CM::KT, n_lags_all);
    const size_t part_b = (size_t)n_slabs * (size_t)chunk_lags * GG * 8;
    MD_WS(d_part, double, WS_PART, part_b * (want_abs ? 2 : 1));
    double *d_part_abs = want_abs ? d_part + part_b / 8 : nullptr;
    KernelTimer timer(ctx, 0);
    int launches = 0;
    rc = lagt::run_chunks(
        ctx, n_lags_all, chunk_lags,
        [&](long long lag0, long long n_lags) {
            MD_HIP(hipMemsetAsync(d_part, 0, part_b * (want_abs ? 2 : 1), ctx->stream));  // (and only a <= b is written)
            const int n_tiles = (int)CM::n_tiles(n_lags);
            const dim3 grid((unsigned)((n_tiles + 1) / 2), (unsigned)n_slabs);
            for (int ta = 0; ta < n_gt; ++ta)
                for (int tb = ta; tb < n_gt; ++tb, ++launches) {
                    const int ga0 = ta * CM_GT, gb0 = tb * CM_GT;
                    const int na = std::min(CM_GT, G - ga0), nb = std::min(CM_GT, G - gb0);
                    const int err = want_abs ? cm_launch_tiles<true>(ctx, grid, d_P, n, G, ga0, na, gb0, nb, lag0, n_lags,
                                                                    n_tiles, n_slabs, d_part, d_part_abs)
                                            : cm_launch_tiles<false>(ctx, grid, d_P, n, G, ga0, na, gb0, nb, lag0, n_lags,
                                                                     n_tiles, n_slabs, d_part, d_part_abs);
                    if (err) return err;
                }
            return MDHIP_OK;
        },
        [&](long long lag0, long long n_lags) {
            const unsigned fin = (unsigned)((n_lags * GG + 255) / 256);
            hipLaunchKernelGGL(cross_msd_finish_kernel, dim3(fin), dim3(256), 0, ctx->stream, d_part, d_out, (long long)n,
                               G, lag0, n_lags, n_slabs);
            if (want_abs) {
                MD_HIP(hipGetLastError());
                hipLaunchKernelGGL(cross_msd_finish_kernel, dim3(fin), dim3(256), 0, ctx->stream, d_part_abs, d_abs,
                                   (long long)n, G, lag0, n_lags, n_slabs);
            }
            return MDHIP_OK;
        });
    if (rc) return rc;
    ctx->last_kernel = "cross_msd_kernel";
    ctx->last_launches = launches;
    timer.stop();
    if (!out_on_device) {
        if ((rc = mdhip_result(cs, out, d_out, out_b, 0))) return rc;
        if (want_abs && (rc = mdhip_result(cs, abs_out, d_abs, out_b, 0))) return rc;
    }
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
