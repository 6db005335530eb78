// lag_tiles.h — what the direct lag sweeps share — geometry helpers, a slab and chunk plan, a chunk loop: xcorr_direct_kernel (xcorr.hip), cross_msd_kernel (collective.hip)
// and orient_corr_kernel (reorient.hip) sum every lag of a time correlation directly, each with an inner loop of its
// own, inside ONE organisation:
//   - a workgroup owns a TILE of KT = THREADS * LPT consecutive lags, LPT per lane; tiles are paired (j, nT - 1 - j), the
//     middle one alone, so that every workgroup of a launch has the same amount of work;
//   - the origins [0, n - K0) of a tile (K0 its first lag) are cut into n_slabs time SLABS, the cuts multiples of ALIGN;
//     a slab goes in STAGES of TT steps, each with the window [T0 + K0, T0 + K0 + AW) of a series in LDS, transposed
//     ([i mod LPT][i div LPT], ROW doubles per row: the 64 lanes of a wave read consecutive doubles), zero beyond n;
//   - the slab sums go to a partial buffer that a second kernel adds in slab order (no float atomics); the host picks
//     the slab count from the resident workgroups and cuts the work into chunks whose partials fit a byte budget.
// The part above `#ifdef __HIPCC__` is plain C++17 integer arithmetic (no HIP header, no context), in the form of
// shell_gather.h: tests/native/lag_tiles_main.cpp walks it with g++ under sanitizers; the rest is for hipcc only.
#pragma once
#include <algorithm>
#include <cstddef>

#ifdef __HIPCC__
#define LT_HD __host__ __device__ __forceinline__
#else
#define LT_HD inline
#endif

namespace lagt {

// ---- host part: the slab and chunk plan -----------------------------------------------------------------------------

// Time slabs of a launch. Tiles are paired, so a launch ends with a partly filled last round of workgroups: `target`
// workgroups (rounds x resident per CU x CUs) keep that round a few percent. `per_slab`: the workgroups one slab adds;
// `time_cap`: slabs with a stage of their own; `hard_cap`: what the grid and the caller's layout allow; `forced` > 0
// replaces the estimate (opt_xcorr_tile), under the same caps.
inline int slab_count(long long target, long long per_slab, long long time_cap, long long hard_cap, int forced = 0)
{
    const long long want = forced > 0 ? forced : (target + per_slab - 1) / per_slab;
    return (int)std::max<long long>(1, std::min({want, time_cap, hard_cap}));
}

struct Plan {  // time slabs per launch, in [1, 65535]; units (lag tiles, or series pairs) per chunk, >= 1
    int n_slabs;
    long long chunk;
};

// `units` units whose partials take `unit_slab_b` bytes per unit and slab, under `budget` bytes: the units per chunk —
// one at least, whatever it takes — after (shrink_slabs) the slab count has come down to what one unit affords.
inline Plan fit(size_t unit_slab_b, long long n_slabs, long long units, size_t budget, bool shrink_slabs)
{
    if (shrink_slabs) n_slabs = std::max<long long>(1, std::min<long long>(n_slabs, (long long)(budget / unit_slab_b)));
    const long long chunk = std::max<long long>(1, std::min<long long>(units, (long long)(budget / (unit_slab_b * (size_t)n_slabs))));
    return {(int)n_slabs, chunk};
}

// units of the chunk that begins at unit u0
inline long long chunk_size(long long units, long long chunk, long long u0) { return chunk < units - u0 ? chunk : units - u0; }

// ---- geometry helpers of a kernel ----------------------------------------------------------------------------------

// THREADS lanes with LPT consecutive lags each, stages of TT steps, PAD window entries of prefetch behind them, ROW_PAD
// doubles between the transposed rows, slab cuts at multiples of ALIGN (a power of two).
template <int THREADS_, int LPT_, int TT_, int PAD, int ROW_PAD, int ALIGN>
struct Tiles {
    static constexpr int THREADS = THREADS_, LPT = LPT_, TT = TT_;
    static constexpr int KT = THREADS * LPT;       // lags per tile
    static constexpr int AW = TT + KT + PAD;       // window entries per series and stage
    static constexpr int ROW = AW / LPT + ROW_PAD;  // LPT transposed rows of ROW doubles per series
    static constexpr int LOG_LPT = LPT == 8 ? 3 : LPT == 4 ? 2 : LPT == 2 ? 1 : 0;
    static_assert(AW % LPT == 0 && (1 << LOG_LPT) == LPT && (ALIGN & (ALIGN - 1)) == 0, "whole rows, powers of two");

    static long long n_tiles(long long n_lags) { return (n_lags + KT - 1) / KT; }

    // Workgroup `pair_id` walks tile_of(pair_id, 0), then tile_of(pair_id, 1) unless that is the same (the middle) tile
    // again; a tile's first lag relative to lag0 is first_lag(tile), and a tile whose first lag is beyond the lags is
    // skipped. (The kernels spell out that `break` and `continue` themselves: a helper that returns the decision changes
    // the generated code, see profiles/lag_tiles_refactor_codegen.txt.)
    LT_HD static int tile_of(int pair_id, int half, int n_tiles) { return half == 0 ? pair_id : n_tiles - 1 - pair_id; }
    LT_HD static long long first_lag(int tile) { return (long long)tile * KT; }

    // origins [t_lo, t_hi) of slab `slab` of a tile with t_total = n - K0 origins (empty for the last slabs of a short tile)
    LT_HD static void slab_range(long long t_total, int n_slabs, int slab, long long &t_lo, long long &t_hi)
    {
        long long per = (t_total + n_slabs - 1) / n_slabs;
        per = (per + (ALIGN - 1)) & ~(long long)(ALIGN - 1);
        t_lo = (long long)slab * per;
        t_hi = t_lo + per < t_total ? t_lo + per : t_total;
    }

    // where window entry i of the series in row block `block` (LPT rows) lies; lane `tid` has entry LPT tid + e at slot(e) + tid
    LT_HD static int slot(int i, int block = 0) { return (LPT * block + (i & (LPT - 1))) * ROW + (i >> LOG_LPT); }

    // steps of the stage at T0 of a slab that ends at t_hi
    LT_HD static long long steps(long long t_hi, long long T0) { return t_hi - T0 < TT ? t_hi - T0 : TT; }

    // THE RULE of the unpredicated loops: of the first `count` steps of the stage at T0 of the tile at K0, those at which
    // the first `hi` lags of the tile all have their partner sample inside the series, T0 + tt + K0 + hi - 1 <= n - 1,
    // in whole blocks of `block` (a power of two) steps. cross_msd_kernel (hi = wave_hi, block 4) and orient_corr_kernel
    // (tt_count: hi = wave_lo + 1, block 1; fast: hi = wave_hi, block OC_LPT) type these two lines out — inlined, this
    // function changes their register allocation (same file) — and must equal it; tests/native/lag_tiles_main.cpp
    // checks the function, and that the kernels' expressions, restated there, equal it.
    LT_HD static int fast_steps(long long n, long long K0, int hi, long long T0, int count, int block)
    {
        const long long room = n - K0 - hi - T0 + 1;
        return (int)(room <= 0 ? 0 : (room < count ? room : count)) & ~(block - 1);
    }

    // lag j (0 .. LPT - 1) of lane `tid` in the tile at Q0; the lane stores those below n_lags
    LT_HD static long long lane_lag(long long Q0, int tid, int j) { return Q0 + (long long)tid * LPT + j; }

#ifdef __HIPCC__
    // one series' window [g0, g0 + AW) into row block `block` of `lds`, zero beyond the series; between two barriers
    __device__ __forceinline__ static void stage(double *lds, int block, const double *series, long long g0, long long n, int tid)
    {
        for (int i = tid; i < AW; i += THREADS) lds[slot(i, block)] = g0 + i < n ? series[g0 + i] : 0.0;
    }
#endif
};

// xcorr: two groups of prefetch behind the window; rows 4112 B apart, so that the 8 rows a staging store walks fall into
// different banks. cross_msd: one step of prefetch.
using XcorrTiles = Tiles<256, 8, 2016, 8 + 16, 3, 8>;
using CrossMsdTiles = Tiles<256, 2, 128, 2, 1, 2>;
using OrientTiles = Tiles<256, 4, 128, 0, 0, 1>;

// ---- the three plans ------------------------------------------------------------------------------------------------
// (their differences are measured choices of each kernel, or history; they decide the order of the slab sums and stay)

// xcorr_direct: units = series pairs (grid.z), 6 rounds of 4 resident workgroups; the pairs of a launch are estimated at
// 8 slabs first, since the slab count depends on them; the time cap counts from lag0.
inline Plan xcorr_plan(long long n, long long lag0, long long n_lags, int n_pairs, int cu_count, int forced, size_t budget)
{
    const long long blocks = (XcorrTiles::n_tiles(n_lags) + 1) / 2, pairs = std::min(n_pairs, 65535);
    const size_t slab_b = (size_t)n_lags * 8;
    const long long group = fit(slab_b, 8, pairs, budget, false).chunk;
    const int n_slabs = slab_count(6LL * cu_count * 4, blocks * group, (n - lag0 + XcorrTiles::TT - 1) / XcorrTiles::TT, 65535, forced);
    return fit(slab_b, n_slabs, group, budget, false);
}

// cross_msd: units = lag tiles of G x G sums (twice with the |term| sums), 6 rounds of 2 resident workgroups; the slabs
// come down to what one tile affords.
inline Plan cross_msd_plan(long long n, long long n_lags, int G, bool with_abs, int cu_count, size_t budget)
{
    using T = CrossMsdTiles;
    const long long tiles = T::n_tiles(n_lags);
    const int n_slabs = slab_count(6LL * cu_count * 2, (tiles + 1) / 2, (n + T::TT - 1) / T::TT, 65535);
    return fit((size_t)T::KT * G * G * 8 * (with_abs ? 2 : 1), n_slabs, tiles, budget, true);
}

// orient_corr: units = lag tiles of (c, c * c) per molecule slab (grid.z), 12 rounds of 4 resident workgroups; molecule
// slabs x time slabs stay within 65536.
inline Plan orient_plan(long long n, long long n_lags, long long n_mslabs, int cu_count, size_t budget)
{
    using T = OrientTiles;
    const long long tiles = T::n_tiles(n_lags), M = std::max<long long>(n_mslabs, 1);
    const int n_slabs = slab_count(12LL * 4 * cu_count, (tiles + 1) / 2 * M, (n + T::TT - 1) / T::TT, std::min(65535LL, 65536 / M));
    return fit((size_t)T::KT * 2 * 8 * (size_t)M, n_slabs, tiles, budget, false);
}

constexpr size_t PARTIAL_BUDGET = (size_t)1 << 30;  // what the three entry points pass

}  // namespace lagt

#ifdef __HIPCC__
#include "ctx.h"

namespace lagt {

// The chunk loop: for every chunk [u0, u0 + nu) of `units`, launch(u0, nu) — which first clears what its sums need
// cleared (a slab can be empty for short tiles) — then finish(u0, nu), on the call's stream.
template <class Launch, class Finish>
inline int run_chunks(mdhip_ctx *ctx, long long units, long long chunk, Launch launch, Finish finish)
{
    for (long long u0 = 0; u0 < units; u0 += chunk) {
        const long long nu = chunk_size(units, chunk, u0);
        int rc;
        if ((rc = launch(u0, nu))) return rc;
        MD_HIP(hipGetLastError());
        if ((rc = finish(u0, nu))) return rc;
        MD_HIP(hipGetLastError());
    }
    return MDHIP_OK;
}

}  // namespace lagt
#endif  // __HIPCC__
