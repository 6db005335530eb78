// group_pairs_plan_main.cpp — walks the unit plan of csrc/group_pairs.h (the host-only part: which of a job's two groups
// lies along the lanes, its tiles, chunks and units, how many units a workgroup takes, the guard band) over fixed tables
// and seeded random jobs; tests/test_group_pairs_plan_native_cpu.py builds it with g++ under -fsanitize=address,undefined.
// g++ sees nothing of the header's device and launch parts.
// Two rule records, those of mdhip_van_hove_distinct (2^31 pairs per workgroup, a row of 8 nbins or none) and of
// mdhip_vector_pair_hist (2^29, 32 nbins), each with chunks of 3, 64 and 2^20 uniform entities. Checked for every job:
// the lanes rule and the matching ends; n_tiles, n_jc, n_units; nblk * upb >= n_units > (nblk - 1) * upb; no word of a
// row can wrap (upb * 64 * min(nu, chunk) <= max_pairs); upb >= waves where that allows; the pair count; and, for small
// jobs, by decoding every unit as the kernels do, that each (origin, lane entity, uniform entity) is visited exactly once
// and the pair of an entity with itself never.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../mdproptools_amd/csrc/group_pairs.h"

static long failures = 0, n_jobs = 0, n_lanes_b = 0, n_same = 0, n_empty = 0, n_chunked = 0, n_capped = 0, n_walked = 0, n_limit = 0;
static std::string what;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                \
    } while (0)

typedef unsigned __int128 u128;
static const long long WALK_MAX = 150000;  // (origin, i, j) triples of a job that is decoded unit by unit

static GpRule rule_vh(int nbins, long long chunk) { return {4, chunk, 4096, 1ll << 31, nbins <= 16128 ? 8ll * nbins : 0}; }
static GpRule rule_vp(int nbins, long long chunk) { return {4, chunk, 4096, 1ll << 29, 32ll * nbins}; }

static void check(long long n_orig, long long a0, long long na, long long b0, long long nb, const GpRule &R)
{
    const bool same = a0 == b0 && na == nb;
    char buf[200];
    snprintf(buf, sizeof buf, "origins %lld a (%lld, %lld) b (%lld, %lld) chunk %lld max_pairs %lld row %lld", n_orig, a0,
             na, b0, nb, R.chunk, R.max_pairs, R.row_cost);
    what = buf;
    GpJob J;
    const uint64_t pairs = gp_plan(J, n_orig, a0, na, b0, nb, same, R);
    ++n_jobs, n_same += same;
    // the lanes rule, and the ends that go with it
    const long long ta = na / 64 + (na % 64 != 0), tb = nb / 64 + (nb % 64 != 0);
    const bool lanes_b = (u128)na * (u128)tb < (u128)nb * (u128)ta;
    n_lanes_b += lanes_b;
    CHECK(J.lanes_b == (int)lanes_b && J.lag == 0 && J.stride == 1 && J.pad == 0);
    CHECK(J.l0 == (lanes_b ? b0 : a0) && J.nl == (lanes_b ? nb : na) && J.u0 == (lanes_b ? a0 : b0) && J.nu == (lanes_b ? na : nb));
    // units
    CHECK(J.n_tiles == (lanes_b ? tb : ta));
    CHECK(J.n_jc == J.nu / R.chunk + (J.nu % R.chunk != 0));
    CHECK((u128)J.n_units == (u128)n_orig * (u128)J.n_tiles * (u128)J.n_jc);
    n_chunked += J.n_jc > 1;
    // workgroups
    const long long per_unit = 64 * std::min(J.nu, R.chunk);
    CHECK(J.upb >= 1);
    if (J.n_units > 0) {
        CHECK((u128)J.nblk * (u128)J.upb >= (u128)J.n_units && (u128)J.n_units > (u128)(J.nblk - 1) * (u128)J.upb);
        CHECK((u128)J.upb * (u128)per_unit <= (u128)R.max_pairs);  // no uint32 or int64 word of a row can wrap
        if (R.max_pairs / per_unit >= R.waves) CHECK(J.upb >= R.waves);
        n_capped += J.upb == R.max_pairs / per_unit && (J.n_units + R.blocks - 1) / R.blocks > J.upb;
    } else {
        CHECK(J.nblk == 0);
        ++n_empty;
    }
    CHECK(pairs == (uint64_t)((u128)n_orig * ((u128)na * (u128)nb - (same ? (u128)na : 0))));
    // coverage: every unit of every workgroup and wave, decoded as gp_walk does
    if (failures || J.n_units == 0 || (u128)n_orig * (u128)na * (u128)nb > (u128)WALK_MAX) return;
    ++n_walked;
    std::vector<unsigned char> seen((size_t)(n_orig * J.nl * J.nu), 0);
    uint64_t visited = 0;
    for (long long blk = 0; blk < J.nblk; ++blk) {
        const long long ua = blk * J.upb, ub = std::min(ua + J.upb, J.n_units);
        uint64_t in_block = 0;
        for (int wave = 0; wave < R.waves; ++wave)
            for (long long u = ua + wave; u < ub; u += R.waves) {
                const long long c = u % J.n_jc, ot = u / J.n_jc;
                const long long o = ot / J.n_tiles, tile = ot - o * J.n_tiles;
                const long long j0 = c * R.chunk;
                const int jlen = (int)(J.nu - j0 < R.chunk ? J.nu - j0 : R.chunk);
                CHECK(o >= 0 && o < n_orig && tile >= 0 && tile < J.n_tiles && j0 < J.nu && jlen >= 1);
                for (int lane = 0; lane < 64; ++lane) {
                    const long long il = tile * 64 + lane;
                    if (il >= J.nl) continue;
                    const long long self_ll = J.l0 + il - J.u0 - j0;
                    const int self = self_ll >= 0 && self_ll < jlen ? (int)self_ll : -1;
                    for (int jj = 0; jj < jlen; ++jj)
                        if (jj != self) ++seen[(size_t)((o * J.nl + il) * J.nu + j0 + jj)], ++in_block;
                }
            }
        CHECK(in_block <= (uint64_t)R.max_pairs);
        visited += in_block;
    }
    long wrong = 0;
    for (long long o = 0; o < n_orig; ++o)
        for (long long i = 0; i < J.nl; ++i)
            for (long long j = 0; j < J.nu; ++j)
                wrong += seen[(size_t)((o * J.nl + i) * J.nu + j)] != (J.l0 + i != J.u0 + j);
    CHECK(wrong == 0);
    const bool disjoint = a0 + na <= b0 || b0 + nb <= a0 || na == 0 || nb == 0;
    if (same || disjoint) CHECK(visited == pairs);
}

static void check_rules(long long n_orig, long long a0, long long na, long long b0, long long nb, bool small_chunks)
{
    for (int nbins : {1, 4096, 16128, 16129})
        for (long long chunk : {3ll, 64ll, 1ll << 20}) {
            if (chunk != 1ll << 20 && !small_chunks) continue;
            check(n_orig, a0, na, b0, nb, rule_vh(nbins, chunk));
            if (nbins <= 4096) check(n_orig, a0, na, b0, nb, rule_vp(nbins, chunk));
        }
}

int main(int argc, char **argv)
{
    const long long sizes[] = {0, 1, 63, 64, 65, 128, 1ll << 20, (1ll << 20) + 1};
    for (long long n_orig : {0ll, 1ll, 70001ll})
        for (long long na : sizes) {
            check_rules(n_orig, 7, na, 7, na, true);  // a is b
            for (long long nb : sizes) {
                check_rules(n_orig, 0, na, na, nb, true);       // a | b
                check_rules(n_orig, nb + 5, na, 2, nb, true);  // b, a gap, a
            }
        }
    check_rules(2, 0, 65, 60, 70, true);  // two groups of different calls that share entities: i == j is still no pair
    {  // the entry points' limits: n_ent < 2^40, n_frames * n_ent < 2^40
        const long long top = (1ll << 40) - 1;
        check_rules(1, 0, top, 0, top, false);
        check_rules(1, 0, top - 64, top - 64, 64, false);
        check_rules(1, 0, 64, 64, top - 64, false);
        check_rules(1, 0, 1ll << 39, 1ll << 39, (1ll << 39) - 1, false);
        check_rules(1ll << 39, 0, 1, 1, 1, false);
        check_rules((1ll << 33) - 1, 0, 64, 64, 64, false);
        check_rules((1ll << 19) - 1, 0, 1ll << 20, 1ll << 20, (1ll << 20) + 1, false);
        n_limit += 7;
    }
    const int n_random = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20261020);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    const long long small[] = {0, 1, 2, 5, 63, 64, 65, 100, 127, 128, 129, 130, 200};
    const int bins[] = {1, 32, 4096, 16128, 16129};
    for (int k = 0; k < n_random; ++k) {
        const bool large = k % 5 == 0;
        long long na = small[pick(0, 12)], nb = small[pick(0, 12)];
        long long n_orig = pick(0, 4);
        if (large) {
            if (pick(0, 1)) na = pick(1, 3) * (1ll << 20) + pick(-2, 2);
            else nb = pick(1, 3) * (1ll << 20) + pick(-2, 2);
            n_orig = pick(0, 100000);
        }
        const long long a0 = pick(0, 9), b0 = k % 3 == 0 ? a0 : a0 + na + pick(0, 3);
        if (k % 3 == 0) nb = na;
        const int nbins = bins[pick(0, 4)];
        const long long chunk = large ? 1ll << 20 : (pick(0, 2) == 0 ? 3 : pick(0, 1) ? 64 : 1ll << 20);
        if (k % 2 == 0 && nbins <= 4096) check(n_orig, a0, na, b0, nb, rule_vp(nbins, chunk));
        else check(n_orig, a0, na, b0, nb, rule_vh(nbins, chunk));
        if (k % 4 == 1) check(n_orig, b0, nb, a0, na, rule_vh(nbins, chunk));  // the same two groups the other way round
    }
    {  // the guard band: twice the error bound of the guess, and the scale
        for (int nbins : {1, 32, 4096, 16129, 1 << 20}) {
            const GpBand b = gp_band(nbins, 0.25);
            int e = 0;
            while ((1ll << (e + 1)) <= (long long)nbins + 1) ++e;  // floor(log2(nbins + 1))
            what = "band";
            CHECK(b.gscale == 4.0f && b.near == (float)(2.0 * (nbins * 2.1e-7 + std::ldexp(1.0, e - 23)) + 1.0e-5));
            CHECK(b.near > 0.0f && (nbins > 4096 || b.near < 0.01f));
        }
    }
    printf("jobs %ld lanes_b %ld same %ld empty %ld chunked %ld capped %ld walked %ld limit %ld failures %ld\n", n_jobs,
           n_lanes_b, n_same, n_empty, n_chunked, n_capped, n_walked, n_limit, failures);
    return failures ? 1 : 0;
}
