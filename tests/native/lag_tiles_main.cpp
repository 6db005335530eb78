// lag_tiles_main.cpp — walks the host part of csrc/lag_tiles.h (the slab and chunk plans of xcorr_direct, mdhip_cross_msd
// and mdhip_orient_corr, and the geometry helpers of their kernels) over fixed edge tables and seeded random inputs;
// tests/test_lag_tiles_native_cpu.py builds it with g++ under -fsanitize=address,undefined. The header's host part is
// integer arithmetic only.
// Checked for every plan: it equals the formulas the three entry points used before the header existed, written out
// below as the reference; n_slabs in [1, 65535]; every grid dimension within its launch limit; the partial bytes of a
// chunk within the budget, or those of ONE unit (at one slab, where the plan may shrink the slabs) when that alone
// exceeds it; the chunks cover the units once, in order. For every geometry (the three real ones and a tiny one): every
// tile in exactly one (workgroup, half); every lag below n_lags in exactly one (tile, lane, j); the slab ranges of a tile
// partition [0, n - K0), with more slabs than stages and at K0 = n - 1 too; the stage slot map a bijection of the
// window entries into the row blocks; the steps of the stages of a slab add up to the slab; at every stage and for
// every wave the fast-step count (fast_steps) within the stage's steps, every fast step with its partner sample inside
// the series, and equal to the lines the kernels type out.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../mdproptools_amd/csrc/lag_tiles.h"

static long failures = 0, n_plans = 0, n_chunks = 0, n_many = 0, n_geoms = 0, n_ranges = 0, n_fast = 0;
static std::string what;
#define CHECK(cond)                                                                                    \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                              \
    } while (0)

using lagt::Plan;
typedef long long ll;

// ---- the parent's formulas ------------------------------------------------------------------------------------------

static Plan ref_xcorr(ll n, ll lag0, ll n_lags, int n_pairs, int cu, int forced, size_t budget)
{
    const int DX_KT = 2048, DX_TT = 2016;
    const int n_tiles = (int)((n_lags + DX_KT - 1) / DX_KT);
    const int n_blocks = (n_tiles + 1) / 2;
    const ll max_slabs = (n - lag0 + DX_TT - 1) / DX_TT;
    const size_t slab_b = (size_t)n_lags * 8;
    int group = (int)std::max<ll>(1, std::min<ll>(std::min(n_pairs, 65535), (ll)(budget / (slab_b * 8))));
    int n_slabs = forced > 0 ? forced : (int)((6LL * cu * 4 + (ll)n_blocks * group - 1) / ((ll)n_blocks * group));
    if (n_slabs > max_slabs) n_slabs = (int)max_slabs;
    if (n_slabs > 65535) n_slabs = 65535;
    if (n_slabs < 1) n_slabs = 1;
    group = (int)std::max<ll>(1, std::min<ll>(group, (ll)(budget / (slab_b * n_slabs))));
    return {n_slabs, group};
}

static Plan ref_cross_msd(ll n, ll n_lags_all, int G, bool want_abs, int cu, size_t budget)
{
    const int CM_KT = 512, CM_TT = 128, GG = G * G;
    const ll n_tiles_all = (n_lags_all + CM_KT - 1) / CM_KT;
    const ll blocks_all = (n_tiles_all + 1) / 2;
    ll n_slabs = (6LL * cu * 2 + blocks_all - 1) / blocks_all;
    n_slabs = std::max<ll>(1, std::min<ll>({n_slabs, (n + CM_TT - 1) / CM_TT, 65535}));
    const size_t tile_b = (size_t)CM_KT * GG * 8 * (want_abs ? 2 : 1);
    n_slabs = std::max<ll>(1, std::min<ll>(n_slabs, (ll)(budget / tile_b)));
    const ll chunk_tiles = std::max<ll>(1, std::min<ll>(n_tiles_all, (ll)(budget / (tile_b * n_slabs))));
    return {(int)n_slabs, chunk_tiles};
}

static Plan ref_orient(ll n, ll n_lags_all, ll n_mslabs, int cu, size_t budget)
{
    const int OC_KT = 1024, OC_TT = 128, OC_ROUNDS = 12, OC_RESIDENT = 4;
    const ll n_tiles_all = (n_lags_all + OC_KT - 1) / OC_KT;
    const ll blocks_all = (n_tiles_all + 1) / 2 * std::max<ll>(n_mslabs, 1);
    ll n_tslabs = ((ll)OC_ROUNDS * OC_RESIDENT * cu + blocks_all - 1) / blocks_all;
    n_tslabs = std::max<ll>(1, std::min<ll>({n_tslabs, (n + OC_TT - 1) / OC_TT, 65535, 65536 / std::max<ll>(n_mslabs, 1)}));
    const size_t tile_b = (size_t)OC_KT * 2 * 8 * (size_t)(std::max<ll>(n_mslabs, 1) * n_tslabs);
    const ll chunk_tiles = std::max<ll>(1, std::min<ll>(n_tiles_all, (ll)(budget / tile_b)));
    return {(int)n_tslabs, chunk_tiles};
}

// ---- what holds for every plan --------------------------------------------------------------------------------------

// `units` units in chunks of pl.chunk; unit_slab_b bytes per unit and slab; grid.x is gx(units of the chunk)
template <class GridX>
static void check_plan(const Plan &pl, const Plan &ref, ll units, size_t unit_slab_b, size_t budget, ll grid_z, GridX gx,
                       bool shrinks = false)
{
    ++n_plans;
    CHECK(pl.n_slabs == ref.n_slabs && pl.chunk == ref.chunk);
    CHECK(pl.n_slabs >= 1 && pl.n_slabs <= 65535 && pl.chunk >= 1 && pl.chunk <= std::max<ll>(units, 1));
    CHECK(grid_z <= 65535);
    const size_t chunk_b = unit_slab_b * (size_t)pl.n_slabs * (size_t)pl.chunk;
    CHECK(chunk_b <= budget || (pl.chunk == 1 && (!shrinks || pl.n_slabs == 1)));
    ll covered = 0, chunks = 0;
    for (ll u0 = 0; u0 < units; u0 += pl.chunk, ++chunks) {
        const ll nu = lagt::chunk_size(units, pl.chunk, u0);
        CHECK(u0 == covered && nu >= 1 && nu <= pl.chunk);
        CHECK(gx(nu) >= 1 && gx(nu) <= 0x7fffffffLL);
        covered += nu;
        if (chunks > 70000) break;  // (tiny budgets against many units: the cover is arithmetic from here on)
    }
    CHECK(covered == units || chunks > 70000);
    n_chunks += chunks;
    if (chunks > 3) ++n_many;
}

static void xcorr_case(ll n, ll lag0, ll n_lags, int n_pairs, int cu, int forced, size_t budget)
{
    char buf[200];
    snprintf(buf, sizeof buf, "xcorr n %lld lag0 %lld lags %lld pairs %d cu %d forced %d budget %zu", n, lag0, n_lags, n_pairs, cu, forced, budget);
    what = buf;
    const Plan pl = lagt::xcorr_plan(n, lag0, n_lags, n_pairs, cu, forced, budget);
    // units = series pairs (grid.z = pairs of a chunk); grid.x = the tile pairs, the same for every chunk
    const ll blocks = (lagt::XcorrTiles::n_tiles(n_lags) + 1) / 2;
    check_plan(pl, ref_xcorr(n, lag0, n_lags, n_pairs, cu, forced, budget), n_pairs, (size_t)n_lags * 8, budget, pl.chunk,
               [&](ll) { return blocks; });
}

static void cross_case(ll n, ll n_lags, int G, bool with_abs, int cu, size_t budget)
{
    char buf[200];
    snprintf(buf, sizeof buf, "cross_msd n %lld lags %lld G %d abs %d cu %d budget %zu", n, n_lags, G, (int)with_abs, cu, budget);
    what = buf;
    const Plan pl = lagt::cross_msd_plan(n, n_lags, G, with_abs, cu, budget);
    const size_t tile_b = (size_t)512 * G * G * 8 * (with_abs ? 2 : 1);
    check_plan(pl, ref_cross_msd(n, n_lags, G, with_abs, cu, budget), lagt::CrossMsdTiles::n_tiles(n_lags), tile_b, budget, 1,
               [&](ll tiles) { return (tiles + 1) / 2; }, true);
}

static void orient_case(ll n, ll n_lags, ll n_mslabs, int cu, size_t budget)
{
    char buf[200];
    snprintf(buf, sizeof buf, "orient n %lld lags %lld mslabs %lld cu %d budget %zu", n, n_lags, n_mslabs, cu, budget);
    what = buf;
    const Plan pl = lagt::orient_plan(n, n_lags, n_mslabs, cu, budget);
    const ll M = std::max<ll>(n_mslabs, 1);
    CHECK(M * pl.n_slabs <= 65536);
    check_plan(pl, ref_orient(n, n_lags, n_mslabs, cu, budget), lagt::OrientTiles::n_tiles(n_lags), (size_t)1024 * 16 * (size_t)M,
               budget, n_mslabs, [&](ll tiles) { return (tiles + 1) / 2; });
}

// ---- the geometry --------------------------------------------------------------------------------------------------

// The rule of the unpredicated loops (T::fast_steps) at one stage, for every wave of the workgroup: never more than the
// stage's steps, whole blocks, the partner sample of the wave's last lag inside the series at every fast step (the
// condition is monotone in tt: the first and the last fast step are looked at), no block more would fit; and the two
// lines of cross_msd_kernel and the four of orient_corr_kernel, restated here as they stand there, equal it.
template <class T>
static void check_fast_steps(ll n, ll K0, ll T0, int count)
{
    const int lanes = T::THREADS < 64 ? T::THREADS : 64;
    for (int w = 0; w < T::THREADS / lanes; ++w) {
        const int wave_lo = w * lanes * T::LPT, wave_hi = wave_lo + lanes * T::LPT;
        for (int block : {1, T::LPT, 4}) {
            const int f = T::fast_steps(n, K0, wave_hi, T0, count, block);
            ++n_fast;
            CHECK(f >= 0 && f <= count && f % block == 0);
            if (f > 0) CHECK(T0 + K0 + wave_hi - 1 <= n - 1 && T0 + (f - 1) + K0 + wave_hi - 1 <= n - 1);
            CHECK(f + block > count || T0 + (f + block - 1) + K0 + wave_hi - 1 > n - 1);
            const ll room = n - K0 - wave_hi - T0 + 1;  // cross_msd_kernel (block 4), orient_corr_kernel (block OC_LPT)
            CHECK(f == ((int)(room <= 0 ? 0 : (room < count ? room : count)) & ~(block - 1)));
        }
        const ll some = n - K0 - wave_lo - T0, in_stage = count;  // orient_corr_kernel's tt_count
        CHECK((int)(some <= 0 ? 0 : (some < in_stage ? some : in_stage)) == T::fast_steps(n, K0, wave_lo + 1, T0, count, 1));
    }
}

template <class T, int ALIGN>
static void walk_geometry(const char *name, int blocks, const std::vector<ll> &sizes)
{
    ++n_geoms;
    // the stage slot map: a bijection of (block, i < AW) into [0, blocks * LPT * ROW), rows never overlapping
    {
        what = std::string(name) + " slots";
        std::vector<char> seen((size_t)blocks * T::LPT * T::ROW, 0);
        for (int b = 0; b < blocks; ++b)
            for (int i = 0; i < T::AW; ++i) {
                const int s = T::slot(i, b);
                CHECK(s >= b * T::LPT * T::ROW && s < (b + 1) * T::LPT * T::ROW);
                if (s < 0 || s >= (int)seen.size()) continue;
                CHECK(!seen[(size_t)s]);
                seen[(size_t)s] = 1;
                CHECK(s == (b * T::LPT + i % T::LPT) * T::ROW + i / T::LPT);
            }
        // what lane tid reads for its lag j at step tt is window entry LPT tid + tt + j: inside the window
        CHECK(T::LPT * (T::THREADS - 1) + (T::TT - 1) + (T::LPT - 1) < T::AW);
    }
    for (ll n : sizes) {
        if (n < 1) continue;
        for (ll n_lags : {1LL, n / 2 + 1, n}) {
            for (ll lag0 : {0LL, n - n_lags}) {
                what = std::string(name) + " n " + std::to_string(n) + " lags " + std::to_string(n_lags) + " lag0 " + std::to_string(lag0);
                const int n_tiles = (int)T::n_tiles(n_lags), n_wg = (n_tiles + 1) / 2;
                // every tile in exactly one (workgroup, half), the middle one once
                std::vector<int> visits((size_t)n_tiles, 0);
                for (int wg = 0; wg < n_wg; ++wg)
                    for (int half = 0; half < 2; ++half) {
                        const int tile = T::tile_of(wg, half, n_tiles);
                        if (half == 1 && tile == wg) break;
                        CHECK(tile >= 0 && tile < n_tiles);
                        if (tile >= 0 && tile < n_tiles) ++visits[(size_t)tile];
                        CHECK(T::first_lag(tile) < n_lags);
                    }
                for (int t = 0; t < n_tiles; ++t) CHECK(visits[(size_t)t] == 1);
                // every lag below n_lags in exactly one (tile, lane, j), in order (the first and the last tile in full)
                for (int t : {0, n_tiles - 1}) {
                    ll expect = T::first_lag(t);
                    for (int tid = 0; tid < T::THREADS; ++tid)
                        for (int j = 0; j < T::LPT; ++j, ++expect) CHECK(T::lane_lag(T::first_lag(t), tid, j) == expect);
                    CHECK(expect == T::first_lag(t) + T::KT && (t < n_tiles - 1 || expect >= n_lags));
                }
                // the slab ranges of a tile partition [0, n - K0); the stages of a slab add up to it
                for (int t : {0, n_tiles / 2, n_tiles - 1}) {
                    const ll K0 = lag0 + T::first_lag(t), t_total = n - K0;
                    CHECK(t_total >= 1);
                    const ll stages = (t_total + T::TT - 1) / T::TT;
                    for (ll n_slabs : {1LL, 2LL, 3LL, stages, stages + 1, 2 * stages + 5, 65535LL}) {
                        if (n_slabs < 1 || n_slabs > 65535 || (n_slabs > 5000 && (t != 0 || lag0 != 0))) continue;
                        ll at = 0;
                        for (ll s = 0; s < n_slabs; ++s, ++n_ranges) {
                            ll t_lo, t_hi;
                            T::slab_range(t_total, (int)n_slabs, (int)s, t_lo, t_hi);
                            if (t_lo >= t_hi) {  // an empty slab: only behind the last origin
                                CHECK(at == t_total);
                                continue;
                            }
                            CHECK(t_lo == at && t_hi <= t_total && t_lo % ALIGN == 0);
                            at = t_hi;
                            ll sum = 0;
                            for (ll T0 = t_lo; T0 < t_hi; T0 += T::TT) {
                                const ll st = T::steps(t_hi, T0);
                                CHECK(st >= 1 && st <= T::TT);
                                sum += st;
                                if (n_slabs <= 5000) check_fast_steps<T>(n, K0, T0, (int)st);
                            }
                            CHECK(sum == t_hi - t_lo);
                        }
                        CHECK(at == t_total);
                    }
                }
            }
        }
    }
}

template <class T>
static std::vector<ll> gpu_test_sizes()
{
    const ll KT = T::KT, TT = T::TT;
    return {1, 2, TT - 1, TT + 1, KT - 1, KT + 1, KT + TT + 1, 2 * KT - 1, 2 * KT + 1, 3 * KT - 5};
}

int main(int argc, char **argv)
{
    const long n_random = argc > 1 ? atol(argv[1]) : 3000;
    const size_t GiB = (size_t)1 << 30;
    const ll n_max = (1LL << 29) - 1;

    // ---- plans: fixed edges
    for (int cu : {1, 256, 37})
        for (ll n : {1LL, 2LL, 127LL, 128LL, 129LL, 2015LL, 2016LL, 2017LL, 4097LL, 70001LL, 1LL << 20, n_max})
            for (size_t budget : {GiB, (size_t)1 << 20, (size_t)4096, (size_t)1 << 34}) {
                for (ll n_lags : {1LL, n / 3 + 1, n}) {
                    for (int pairs : {1, 3, 16, 65535, 70000})
                        for (int forced : {0, 1, 7, 100000})
                            for (ll lag0 : {0LL, (n - n_lags) / 2, n - n_lags}) xcorr_case(n, lag0, n_lags, pairs, cu, forced, budget);
                    for (int G : {1, 16})
                        for (bool with_abs : {false, true}) cross_case(n, n_lags, G, with_abs, cu, budget);
                    for (ll mslabs : {0LL, 1LL, 5LL, 32768LL}) orient_case(n, n_lags, mslabs, cu, budget);
                }
            }
    // the chunked Einstein case of tests/test_gpu_einstein.py: 3 lag tiles, 547 slabs cut to 512, one tile per chunk
    {
        what = "einstein 16 x 70001, 1101 lags, abs";
        const Plan pl = lagt::cross_msd_plan(70001, 1101, 16, true, 256, GiB);
        CHECK(lagt::CrossMsdTiles::n_tiles(1101) == 3 && pl.n_slabs == 512 && pl.chunk == 1);
        CHECK(lagt::slab_count(6LL * 256 * 2, 2, (70001 + 127) / 128, 65535) == 547);
    }

    // ---- plans: seeded random
    std::mt19937_64 rng(20240611);
    auto pick = [&](ll lo, ll hi) { return lo + (ll)(rng() % (unsigned long long)(hi - lo + 1)); };
    for (long k = 0; k < n_random; ++k) {
        const ll n = (k % 3 == 0) ? pick(1, 5000) : (k % 3 == 1) ? pick(1, 1 << 20) : pick(1, n_max);
        const ll n_lags = pick(1, n), lag0 = pick(0, n - n_lags);
        const int cu = (int)pick(1, 320);
        const size_t budget = (size_t)1 << pick(10, 34);
        xcorr_case(n, lag0, n_lags, (int)pick(1, 70000), cu, k % 4 == 0 ? (int)pick(1, 70000) : 0, budget);
        cross_case(n, n_lags, (int)pick(1, 16), k % 2 == 0, cu, budget);
        orient_case(n, n_lags, k % 5 == 0 ? 0 : pick(1, 32768), cu, budget);
    }

    // ---- the walker: the three real geometries at the sizes of the GPU tests, and a tiny one exhaustively
    walk_geometry<lagt::XcorrTiles, 8>("xcorr", 1, gpu_test_sizes<lagt::XcorrTiles>());
    walk_geometry<lagt::CrossMsdTiles, 2>("cross_msd", 24, gpu_test_sizes<lagt::CrossMsdTiles>());
    walk_geometry<lagt::OrientTiles, 1>("orient", 3, gpu_test_sizes<lagt::OrientTiles>());
    {
        typedef lagt::Tiles<4, 2, 4, 2, 1, 2> Tiny;  // tiles of 8 lags, stages of 4 steps
        std::vector<ll> all;
        for (ll n = 1; n <= 70; ++n) all.push_back(n);
        walk_geometry<Tiny, 2>("tiny", 3, all);
        typedef lagt::Tiles<2, 4, 8, 0, 0, 1> Tiny1;
        walk_geometry<Tiny1, 1>("tiny1", 2, all);
        typedef lagt::Tiles<2, 8, 16, 24, 3, 8> Tiny8;
        walk_geometry<Tiny8, 8>("tiny8", 1, all);
    }

    printf("plans %ld chunks %ld many_chunk_plans %ld geometries %ld slab_ranges %ld fast_steps %ld failures %ld\n", n_plans,
           n_chunks, n_many, n_geoms, n_ranges, n_fast, failures);
    return failures ? 1 : 0;
}
