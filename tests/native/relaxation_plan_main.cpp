// The host side of mdhip_self_relaxation (csrc/relaxation_plan.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_relaxation_plan_native_cpu.py. It includes nothing but that header.
//   cells:    for small (F, max_lag, stride), strides up to 2^63 - 1 included, every cell (origin index, lag) with t0 + lag <= F - 1 and lag <= max_lag is
//             met exactly once when the launches, their tiles, the lanes and the lanes' cells are walked the way the
//             kernel walks them, and no other cell is met; a tile that tile_empty names holds no cell
//   launches: every dimension in [1, 65535] at sizes up to 2^29 - 1 frames, the slices a partition of the tile ranges
//   guard:    origins[0] * size at 2^30 - 1 and 2^30, and sizes that would overflow a product
//   sinc:     against the long double sine at the switch points, around multiples of pi / 2 and at seeded random x in
//             [2^-12, 2^37): the largest error is printed and must be below 2^-34
// Prints "cells N launches N guard N sinc N sinc_err_log2 X below_far_log2 X failures N".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>

#include "../../mdproptools_amd/csrc/relaxation_plan.h"

static long long failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++failures <= 20) printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

// `stride` is the caller's, anything from 1 to 2^63 - 1: the entry point hands the plan and the kernel
// clamp_stride(F, stride), and the products below are the kernel's (UBSan watches them).
static long long walk_cells(long long F, long long max_lag, long long stride)
{
    const long long s = rx::clamp_stride(F, stride);
    CHECK(s >= 1 && s <= F && (stride > F - 1 || s == stride));
    std::map<std::pair<long long, long long>, int> seen;
    for (const rx::Launch &L : rx::launches(F, max_lag, s))
        for (long long by = 0; by < L.gy; ++by)
            for (long long bx = 0; bx < L.gx; ++bx) {
                const long long ot = L.ot0 + bx, kt = L.kt0 + by;
                const bool empty = rx::tile_empty(F, max_lag, s, ot, kt);
                for (int lane = 0; lane < rx::THREADS; ++lane) {
                    const long long oi = ot * rx::TO + rx::lane_origin(lane);
                    const long long k0 = kt * rx::TK + rx::lane_lag(lane, 0);
                    const int nv = rx::n_cells(F, max_lag, oi * s, k0);
                    CHECK(!(empty && nv > 0));
                    for (int c = 0; c < nv; ++c) {
                        CHECK(kt * rx::TK + rx::lane_lag(lane, c) == k0 + c);
                        ++seen[{oi, k0 + c}];
                    }
                }
            }
    long long want = 0;
    for (long long k = 0; k <= max_lag; ++k) {
        const long long no = rx::origins(F, k, s);
        long long brute = 0;
        for (long long t0 = 0; t0 <= F - 1 - k; t0 = stride <= F - 1 - t0 ? t0 + stride : F) ++brute;  // (the caller's stride)
        CHECK(no == brute && no == rx::origins(F, k, stride));
        for (long long oi = 0; oi < no; ++oi) {
            auto it = seen.find({oi, k});
            CHECK(it != seen.end() && it->second == 1);
        }
        want += no;
    }
    CHECK((long long)seen.size() == want);
    return want;
}

int main()
{
    long long cells = 0, n_launch = 0, n_guard = 0, n_sinc = 0;
    // ---- cells
    const long long Fs[] = {1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 95, 96, 97, 128, 129, 161, 200};
    for (long long F : Fs) {
        const long long lags[] = {0, 1, 7, 8, 9, 62, 63, 64, 65, (F - 1) / 2, F - 2, F - 1};
        const long long strides[] = {1, 2, 3, 7, 31, 32, 33, F - 1, F, F + 5, 1ll << 40, 1ll << 58, 1ll << 61,
                                     (1ll << 62) + 1, 0x7fffffffffffffffll};
        for (long long K : lags)
            for (long long s : strides)
                if (K >= 0 && K <= F - 1 && s >= 1) cells += walk_cells(F, K, s);
    }
    // ---- launches
    const long long bigF[] = {1, 2, 64, 65, 2097120, 2097121, 2097153, 4194240, 4194241, 4194305, 100000000, rx::MAX_FRAMES};
    for (long long F : bigF) {
        const long long lags[] = {0, 1, 63, 64, F / 2, F - 1};
        const long long strides[] = {1, 2, 1000, F};
        for (long long K : lags)
            for (long long s : strides) {
                if (K > F - 1) continue;
                const auto Ls = rx::launches(F, K, s);
                CHECK(!Ls.empty());
                const long long n_kt = K / rx::TK + 1;
                long long kt_next = 0, ot_next = 0, n_ot = 0;
                for (size_t i = 0; i < Ls.size(); ++i) {
                    const rx::Launch &L = Ls[i];
                    CHECK(L.gx >= 1 && L.gx <= 65535 && L.gy >= 1 && L.gy <= 65535);
                    if (L.ot0 == 0) {  // a new slice of lag tiles
                        CHECK(ot_next == n_ot);
                        CHECK(L.kt0 == kt_next);
                        kt_next = L.kt0 + L.gy;
                        n_ot = (rx::origins(F, L.kt0 * rx::TK, s) + rx::TO - 1) / rx::TO;
                        ot_next = 0;
                    }
                    CHECK(L.ot0 == ot_next);
                    ot_next += L.gx;
                    // the widest lag tile of the slice is its first: nothing beyond n_ot holds a cell
                    CHECK(rx::tile_empty(F, K, s, n_ot, L.kt0));
                    ++n_launch;
                }
                CHECK(kt_next == n_kt && ot_next == n_ot);
            }
    }
    CHECK(rx::launches(2097121, 0, 1).size() == 2);       // 65536 origin tiles
    CHECK(rx::launches(4194241, 4194240, 4194241).size() == 2);  // 65536 lag tiles of one origin
    // ---- guard
    {
        const long long G = 1ll << 30;
        CHECK(rx::guard_ok(1, 1, G - 1) && !rx::guard_ok(1, 1, G));
        CHECK(rx::guard_ok(32768, 1, 32767) && !rx::guard_ok(32768, 1, 32768));
        CHECK(rx::guard_ok(32768, 2, 65535) && !rx::guard_ok(32768, 2, 65536));   // 16384 origins
        CHECK(rx::guard_ok(32769, 2, 65535 - 4) && !rx::guard_ok(32769, 2, 65536));  // 16385 origins
        CHECK(rx::guard_ok(rx::MAX_FRAMES, 1, 2) && !rx::guard_ok(rx::MAX_FRAMES, 1, 3));
        CHECK(rx::guard_ok(rx::MAX_FRAMES, rx::MAX_FRAMES, G - 1));
        CHECK(!rx::guard_ok(rx::MAX_FRAMES, 1, (1ll << 62)));   // (a product would overflow)
        CHECK(rx::guard_ok(1000, 1, 0));
        for (long long F = 1; F < 3000; F += 7)
            for (long long s = 1; s < 40; s += 3) {
                const long long o = rx::origins(F, 0, s), edge = (G - 1) / o;
                CHECK(o * edge < G && o * (edge + 1) >= G);
                CHECK(rx::guard_ok(F, s, edge) && !rx::guard_ok(F, s, edge + 1));
                ++n_guard;
            }
    }
    // ---- sinc
    long double worst = 0.0L, worst_in = 0.0L;  // over every x, and below the far cut
    auto probe = [&](double x) {
        const long double want = x == 0.0 ? 1.0L : sinl((long double)x) / (long double)x;
        const long double err = fabsl((long double)rx::sinc(x) - want);
        if (err > worst) worst = err;
        if (x < rx::SINC_FAR && err > worst_in) worst_in = err;
        ++n_sinc;
    };
    CHECK(rx::sinc(0.0) == 1.0);
    CHECK(rx::sinc(INFINITY) == 0.0 && rx::sinc(rx::SINC_FAR) == 0.0);
    const double edges[] = {0.0, 1e-300, 1e-20, rx::SINC_NEAR, rx::SINC_FAR, 0.7853981633974483, 1.5707963267948966,
                            3.141592653589793, 6.283185307179586, 100.0, 1e5, 1e9};
    for (double e : edges) {
        probe(e);
        probe(std::nextafter(e, 0.0));
        probe(std::nextafter(e, 1e300));
    }
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> expo(-12.0, 37.0), unit(0.0, 1.0);
    for (int i = 0; i < 2000000; ++i) probe(std::exp2(expo(rng)));
    for (int i = 0; i < 500000; ++i) probe(100.0 * unit(rng));                  // what the GPU tests use
    for (long long m = 1; m < 200000; ++m) {                                    // around the multiples of pi / 4
        const double c = 0.7853981633974483 * (double)m * (m % 7 == 0 ? 1000.0 : 1.0);
        probe(c);
        probe(std::nextafter(c, 0.0));
        probe(c * (1.0 + 1e-9));
    }
    const double log2_err = worst > 0.0L ? (double)log2l(worst) : -1074.0;
    const double log2_in = worst_in > 0.0L ? (double)log2l(worst_in) : -1074.0;
    CHECK(worst < 0x1p-34L);
    CHECK(worst_in < 0x1p-43L);  // (what the header derives for the polynomial branch)
    printf("cells %lld launches %lld guard %lld sinc %lld sinc_err_log2 %.2f below_far_log2 %.2f failures %lld\n", cells,
           n_launch, n_guard, n_sinc, log2_err, log2_in, failures);
    return failures ? 1 : 0;
}
