// relaxation_plan.h — the tile geometry, launch split, size guard and sinc evaluation of mdhip_self_relaxation
// (relaxation.hip). Plain C++17, no HIP: tests/native/relaxation_plan_main.cpp includes nothing but this header.
//
// A workgroup of THREADS lanes owns a TILE of TO origins x TK lags of one group. Lane l holds origin o = l % TO of the
// tile and the CELLS consecutive lags (l / TO) * CELLS + c, c = 0 .. CELLS - 1: the 32 lanes of half a wave hold the 32
// origins of one run of lags, so that a lag's sum over origins is a shuffle reduction inside half a wave. Tile
// (ot, kt): origin indices ot * TO + o (frame t0 = index * stride), lags kt * TK + kl. A cell exists when
// lag <= max_lag and t0 + lag <= n_frames - 1.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define RX_HD __host__ __device__
#else
#define RX_HD
#endif

namespace rx {

constexpr int THREADS = 256;
constexpr int TO = 32;                       // origins of a tile
constexpr int CELLS = 8;                     // cells of a lane: consecutive lags of one origin
constexpr int LAG_RUNS = THREADS / TO;       // 8 runs of CELLS lags
constexpr int TK = LAG_RUNS * CELLS;         // 64 lags of a tile
constexpr int EB = 16;                       // entities of a stage
constexpr int ORG_W = TO + 1;                // LDS row of the origin frames (odd: the transposing stores spread over the banks)
constexpr int WIN = TO + TK - 1;             // LDS row of the partner frames: 95, odd
constexpr int LDS_DOUBLES = 3 * EB * (ORG_W + WIN);  // 6144 doubles = 48 KiB: three workgroups per CU
constexpr int MAX_Y = 65535;
constexpr int MAX_GROUPS = 16, MAX_Q = 4;
constexpr long long MAX_FRAMES = (1ll << 29) - 1;
constexpr long long GUARD = 1ll << 30;       // origins[0] * group size stays below this

// origins of lag k: t0 = 0, s, 2s, ... with t0 + k <= F - 1
RX_HD inline long long origins(long long F, long long k, long long s) { return k <= F - 1 ? (F - 1 - k) / s + 1 : 0; }

// The stride the plan and the kernel work with. Any stride beyond F - 1 leaves the one origin t0 = 0, so F stands for
// all of them: with s <= F < 2^29 every product (origin index) * s of the plan and the kernel stays below 2^35, where a
// caller's stride near 2^63 would overflow it.
RX_HD inline long long clamp_stride(long long F, long long s) { return s < F ? s : F; }

// origins[0] * size < 2^30 (no overflow: size may be anything below 2^63). With the 2^32 unit |fs| <= 2^30 * 2^32 =
// 2^62 < 2^63, and count2 <= origins * size^2 < 2^60.
inline bool guard_ok(long long F, long long s, long long size) { return size <= (GUARD - 1) / origins(F, 0, s); }

// lane, cell -> origin and lag inside the tile
RX_HD inline int lane_origin(int lane) { return lane % TO; }
RX_HD inline int lane_lag(int lane, int c) { return lane / TO * CELLS + c; }

// Cells of a lane that exist: c < n_cells (they are the lane's first). t0: the lane's origin frame, k0: its first lag.
RX_HD inline int n_cells(long long F, long long max_lag, long long t0, long long k0)
{
    const long long last = max_lag < F - 1 - t0 ? max_lag : F - 1 - t0;  // the largest lag of this origin
    const long long n = last - k0 + 1;
    return n < 0 ? 0 : n > CELLS ? CELLS : (int)n;
}

// A tile is skipped when not even its first cell exists.
RX_HD inline bool tile_empty(long long F, long long max_lag, long long s, long long ot, long long kt)
{
    return kt * TK > max_lag || ot * TO * s + kt * TK > F - 1;
}

// One launch: grid (gx origin tiles from ot0 on, gy lag tiles from kt0 on, groups). No launch dimension passes 65535:
// longer origin and lag ranges go in slices. A slice is as wide as its first lag tile needs (the widest of the slice).
struct Launch {
    long long ot0, kt0;
    unsigned gx, gy;
};
inline std::vector<Launch> launches(long long F, long long max_lag, long long s)
{
    std::vector<Launch> out;
    const long long n_kt = max_lag / TK + 1;
    for (long long kt0 = 0; kt0 < n_kt; kt0 += MAX_Y) {
        const long long n_ot = (origins(F, kt0 * TK, s) + TO - 1) / TO;
        for (long long ot0 = 0; ot0 < n_ot; ot0 += MAX_Y)
            out.push_back({ot0, kt0, (unsigned)std::min<long long>(MAX_Y, n_ot - ot0),
                           (unsigned)std::min<long long>(MAX_Y, n_kt - kt0)});
    }
    return out;
}

// ---- sinc(x) = sin(x) / x for x >= 0 (or +inf), within 2^-34 absolute of the real sinc of the double x ------------
//   x >= 2^36 (+inf too): 0. |sinc(x)| <= 1 / x <= 2^-36.
//   x <  2^-8 (the switch point): 1 + x2 (-1/6 + x2 / 120), x2 = x * x. The series alternates with falling terms, so
//             what is left out is below x^6 / 5040 <= 2^-48 / 5040 < 2^-60; three roundings of values <= 1 add
//             less than 2^-51. Exactly 1 at x = 0.
//   else:     n = rint(x * 2/pi) (by the 1.5 * 2^52 addition, whose low bits are n), r = x - n * pi/2 with pi/2 as
//             the sum of two doubles (two fused multiply-adds: each rounds a value below 1, <= 2^-54; what the two
//             doubles leave of pi/2, below 2^-107, times n < 2^36: 2^-71), so |r| < pi/4 + 2^-15 is within 2^-52 of
//             the real reduced argument. sin r and cos r from their Taylor polynomials of degree 13 and 14 (Horner in
//             r * r, fused multiply-adds): the first terms left out are r^15 / 15! < 2^-45 and r^16 / 16! < 2^-49 at
//             |r| <= 0.79, Horner's roundings below 2^-51. The quadrant n mod 4 picks the polynomial and the sign:
//             |value - sin x| < 2^-44. One division by x: for n = 0 every error above is relative to r = x (the sine
//             polynomial is r times a series), so the quotient is within 2^-44; for n >= 1, x > pi/4 and the
//             quotient's error is below 2^-44 * 4/pi + 2^-53 < 2^-43.
// 2^-43 is well inside the 2^-34 that include/mdhip.h promises; tests/native/relaxation_plan_main.cpp measures it
// against the long double sine.
constexpr double SINC_FAR = 68719476736.0;   // 2^36
constexpr double SINC_NEAR = 0.00390625;     // 2^-8

RX_HD inline double sinc(double x)
{
    if (!(x < SINC_FAR)) return 0.0;
    const double x2 = x * x;
    if (x < SINC_NEAR) return 1.0 + x2 * (-1.0 / 6.0 + x2 * (1.0 / 120.0));
    constexpr double magic = 6755399441055744.0;       // 1.5 * 2^52
    constexpr double two_over_pi = 0.63661977236758138;
    constexpr double pio2_hi = 1.5707963267948966;      // the double nearest pi/2
    constexpr double pio2_lo = 6.123233995736766e-17;   // pi/2 - pio2_hi
    const double t = __builtin_fma(x, two_over_pi, magic);
    const double n = t - magic;
    uint64_t bits;
    memcpy(&bits, &t, 8);
    const unsigned quad = (unsigned)bits;               // n mod 2^32: n < 2^36 sits in the low bits of t
    double r = __builtin_fma(-n, pio2_hi, x);
    r = __builtin_fma(-n, pio2_lo, r);
    const double r2 = r * r;
    double sn = 1.0 / 6227020800.0;
    sn = __builtin_fma(sn, r2, -1.0 / 39916800.0);
    sn = __builtin_fma(sn, r2, 1.0 / 362880.0);
    sn = __builtin_fma(sn, r2, -1.0 / 5040.0);
    sn = __builtin_fma(sn, r2, 1.0 / 120.0);
    sn = __builtin_fma(sn, r2, -1.0 / 6.0);
    sn = __builtin_fma(sn * r2, r, r);
    double cs = -1.0 / 87178291200.0;
    cs = __builtin_fma(cs, r2, 1.0 / 479001600.0);
    cs = __builtin_fma(cs, r2, -1.0 / 3628800.0);
    cs = __builtin_fma(cs, r2, 1.0 / 40320.0);
    cs = __builtin_fma(cs, r2, -1.0 / 720.0);
    cs = __builtin_fma(cs, r2, 1.0 / 24.0);
    cs = __builtin_fma(cs, r2, -0.5);
    cs = __builtin_fma(cs, r2, 1.0);
    const double v = (quad & 1u) ? cs : sn;
    return ((quad & 2u) ? -v : v) / x;
}

}  // namespace rx
