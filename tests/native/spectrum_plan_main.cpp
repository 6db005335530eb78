// spectrum_plan_main.cpp — walks the row table and the batches of csrc/spectrum_plan.h (which row of the time-major copy an
// entity of mdhip_velocity_spectrum owns, and which rows a batch holds) over fixed tables and seeded random ones;
// tests/test_spectrum_plan_native_cpu.py builds it with g++ under -fsanitize=address,undefined. The header is host
// arithmetic only.
// Checked for every accepted table: the rows of an axis are a permutation of the grouped entities, ascending with the
// entity inside each group, the groups one after the other from row0; entities of group -1 have no row; the cuts are
// consecutive entity ranges that begin and end at a grouped entity and hold every grouped entity exactly once; the rows of
// a batch (one axis of a cut) are whole series, a permutation of 0 .. rows - 1 in the order (group, entity), every group a
// contiguous segment; a batch stays within the byte bound unless it holds ONE row and is as large as the bound allows
// unless it is the last. Every invalid table is refused with its rule, the first offending entity named, and holds no
// batch.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../mdproptools_amd/csrc/spectrum_plan.h"

static long failures = 0, n_plans = 0, n_rejected = 0, n_batches = 0, n_rows = 0;
static std::string what;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                \
    } while (0)

struct Table {
    std::vector<int32_t> group;
    int G = 1;
    int64_t F = 1, L = 4, max_lag = 0;
    int buffers = 1;
    long long bound = 1ll << 32;
};

static bool lengths_ok(const Table &t)
{
    return t.F >= 1 && t.L >= 4 && t.L < (1ll << 30) && (t.L & (t.L - 1)) == 0 && t.max_lag >= 0 && t.max_lag <= t.F - 1 &&
           t.L >= t.F + t.max_lag;
}

static void check(const Table &t, const char *name)
{
    const long long E = (long long)t.group.size();
    char buf[160];
    snprintf(buf, sizeof buf, "%s: E %lld G %d F %lld L %lld lag %lld", name, E, t.G, (long long)t.F, (long long)t.L,
             (long long)t.max_lag);
    what = buf;
    const SpPlan pl = spectrum_plan(t.F, E, t.G, t.group.data(), t.L, t.max_lag, t.buffers, t.bound);
    ++n_plans;
    int want = SP_PLAN_OK;
    long long bad = -1;
    if (t.G < 1 || t.G > SP_MAX_GROUPS) want = SP_PLAN_GROUPS;
    else if (!lengths_ok(t)) want = SP_PLAN_LENGTH;
    else
        for (long long e = 0; e < E && bad < 0; ++e)
            if (t.group[(size_t)e] < -1 || t.group[(size_t)e] >= t.G) want = SP_PLAN_ENTITY, bad = e;
    CHECK(pl.error == want && pl.bad_entity == bad);
    if (want != SP_PLAN_OK) {
        ++n_rejected;
        CHECK(pl.cuts.empty() && pl.n_batches() == 0);
        return;
    }
    if (pl.error != SP_PLAN_OK) return;
    // the row table
    CHECK((long long)pl.ent_row.size() == E);
    std::vector<long long> count((size_t)t.G, 0), owner;
    long long grouped = 0;
    for (long long e = 0; e < E; ++e) grouped += t.group[(size_t)e] >= 0;
    CHECK(pl.n_rows == grouped && pl.rows_total() == 3 * grouped);
    owner.assign((size_t)grouped, -1);
    for (long long e = 0; e < E; ++e) {
        const int g = t.group[(size_t)e];
        const long long r = pl.ent_row[(size_t)e];
        if (g < 0) {
            CHECK(r == -1);
            continue;
        }
        CHECK(r == pl.groups.row0[g] + count[(size_t)g]);  // ascending with the entity inside its group
        ++count[(size_t)g];
        CHECK(r >= 0 && r < grouped);
        if (r < 0 || r >= grouped) return;
        CHECK(owner[(size_t)r] == -1);  // a permutation: no row twice
        owner[(size_t)r] = e;
    }
    long long at = 0;
    for (int g = 0; g <= SP_MAX_GROUPS; ++g) {
        CHECK(pl.groups.row0[g] == at);
        if (g < t.G) at += count[(size_t)g];
    }
    CHECK(at == grouped);
    // the cuts: consecutive entity ranges, every grouped entity in exactly one; a batch is one axis of a cut
    CHECK(pl.row_bytes == (t.F + (long long)t.buffers * t.L) * 8);
    const long long per = std::max<long long>(1, std::min<long long>(SP_MAX_BATCH_ROWS, t.bound / pl.row_bytes));
    long long next_e = 0, rows_seen = 0, largest = 0;
    std::vector<long long> covered((size_t)t.G, 0);
    for (size_t c = 0; c < pl.cuts.size(); ++c) {
        const SpCut &cut = pl.cuts[c];
        n_batches += 3;
        CHECK(cut.e_lo >= next_e && cut.e_lo < cut.e_hi && cut.e_hi <= E);
        if (!(cut.e_lo >= next_e && cut.e_lo < cut.e_hi && cut.e_hi <= E)) return;
        for (long long e = next_e; e < cut.e_lo; ++e) CHECK(t.group[(size_t)e] < 0);  // nothing grouped between two cuts
        CHECK(t.group[(size_t)cut.e_lo] >= 0 && t.group[(size_t)(cut.e_hi - 1)] >= 0);
        next_e = cut.e_hi;
        CHECK(cut.rows >= 1 && (cut.rows == 1 || cut.rows * pl.row_bytes <= t.bound) && cut.rows <= SP_MAX_BATCH_ROWS);
        CHECK(cut.rows == per || c + 1 == pl.cuts.size());  // as long as the bound allows, unless it is the last
        largest = std::max(largest, cut.rows);
        // the buffer rows: a permutation of 0 .. rows - 1, group after group, ascending with the entity inside a group
        std::vector<long long> in_cut((size_t)t.G, 0);
        std::vector<char> taken((size_t)cut.rows, 0);
        long long grouped_here = 0;
        for (long long e = cut.e_lo; e < cut.e_hi; ++e) {
            const int g = t.group[(size_t)e];
            if (g < 0) continue;
            ++grouped_here;
            const long long r = pl.ent_row[(size_t)e] + cut.shift.add[g];
            CHECK(r == cut.seg[g] + in_cut[(size_t)g]);
            ++in_cut[(size_t)g];
            CHECK(r >= 0 && r < cut.rows);
            if (r < 0 || r >= cut.rows) return;
            CHECK(!taken[(size_t)r]);
            taken[(size_t)r] = 1;
        }
        CHECK(grouped_here == cut.rows);
        long long seg_at = 0;
        for (int g = 0; g <= SP_MAX_GROUPS; ++g) {
            CHECK(cut.seg[g] == seg_at);
            if (g < t.G) seg_at += in_cut[(size_t)g], covered[(size_t)g] += in_cut[(size_t)g];
        }
        CHECK(seg_at == cut.rows);
        rows_seen += cut.rows;
        n_rows += 3 * cut.rows;
    }
    for (long long e = next_e; e < E; ++e) CHECK(t.group[(size_t)e] < 0);
    CHECK(rows_seen == grouped && pl.max_rows == largest && pl.n_batches() == 3 * (long long)pl.cuts.size());
    CHECK((grouped == 0) == pl.cuts.empty());
    for (int g = 0; g < t.G; ++g) CHECK(covered[(size_t)g] == count[(size_t)g]);
}

int main(int argc, char **argv)
{
    {  // interleaved types inside molecules, some entities in no group, a group without entities
        Table t;
        t.G = 4, t.F = 700, t.L = 2048, t.max_lag = 699;
        for (int e = 0; e < 130; ++e) t.group.push_back(e % 7 == 3 ? -1 : (e % 3 == 0 ? 0 : 3));
        for (long long bound : {1ll << 20, 1ll << 32, 1ll, 21984ll, 2 * 21984ll - 1, 2 * 21984ll}) {
            t.bound = bound;
            check(t, "interleaved");
            t.buffers = 2;
            check(t, "interleaved, packed");
            t.buffers = 1;
        }
    }
    {  // nothing grouped, nothing at all, one entity
        Table t;
        t.G = 2, t.F = 5, t.L = 16, t.max_lag = 4;
        check(t, "no entity");
        t.group = {-1, -1, -1};
        check(t, "no grouped entity");
        t.group = {1};
        check(t, "one entity");
        t.G = 16, t.group = {15, 0, 15, -1, 7};
        check(t, "sixteen groups");
    }
    {  // the lengths: equality of F + max_lag and L, one more lag, no power of two, either end of the range
        Table t;
        t.G = 1, t.group = {0, 0, 0}, t.F = 724, t.max_lag = 300, t.L = 1024;
        check(t, "equality");
        t.max_lag = 301;
        check(t, "one lag too many");
        t.max_lag = 724;
        check(t, "max_lag = F");
        t.max_lag = -1;
        check(t, "max_lag < 0");
        t.max_lag = 0, t.L = 1000;
        check(t, "no power of two");
        t.L = 2, t.F = 1;
        check(t, "L = 2");
        t.L = 4;
        check(t, "L = 4");
        t.L = 1ll << 30;
        check(t, "L = 2^30");
        t.L = 1ll << 29, t.F = 0;
        check(t, "no frame");
        t.F = (1ll << 28) + 1, t.max_lag = (1ll << 28) - 1;
        check(t, "long series");
    }
    {  // refused: the group count, and a bad entity at the front, in the middle, at the end, and two of them
        Table t;
        t.F = 8, t.L = 16, t.max_lag = 7;
        for (int e = 0; e < 9; ++e) t.group.push_back(e % 3);
        for (int G : {0, -1, 17, 2}) {
            t.G = G;
            check(t, "group count");
        }
        t.G = 3;
        for (int at : {0, 4, 8})
            for (int32_t v : {-2, 3, 1 << 30}) {
                Table u = t;
                u.group[(size_t)at] = v;
                check(u, "one bad entity");
                u.group[8] = -5;
                check(u, "two bad entities");
            }
    }
    const int n_random = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20261021);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    for (int k = 0; k < n_random; ++k) {
        Table t;
        t.G = (int)pick(1, 16);
        const long long sizes[] = {0, 1, 2, 63, 64, 65, 130, 1000, 22000};
        const long long E = sizes[pick(0, 8)];
        const int style = (int)pick(0, 2);
        for (long long e = 0; e < E; ++e)
            t.group.push_back(style == 0 ? (int32_t)pick(-1, t.G - 1) : style == 1 ? (int32_t)(e % t.G) : (int32_t)(e * t.G / E));
        t.F = pick(1, 3000);
        t.max_lag = pick(0, t.F - 1);
        t.L = 4;
        while (t.L < t.F + t.max_lag) t.L *= 2;
        if (k % 3 == 0) t.L *= 2;
        t.buffers = (int)pick(1, 2);
        t.bound = k % 5 == 0 ? pick(1, 1ll << 16) : pick(1ll << 16, 1ll << 26);
        if (k % 7 == 0) {  // something that must be refused
            switch (pick(0, 4)) {
            case 0: t.G = pick(0, 1) ? 0 : 17; break;
            case 1: t.L /= 2; break;  // (refused where that falls below F + max_lag or 4; accepted otherwise)
            case 2: t.max_lag = t.F; break;
            case 3: t.L += 1; break;
            default:
                if (E) t.group[(size_t)pick(0, E - 1)] = pick(0, 1) ? -2 : t.G;
                break;
            }
        }
        check(t, "random");
    }
    printf("plans %ld rejected %ld batches %ld rows %ld failures %ld\n", n_plans, n_rejected, n_batches, n_rows, failures);
    return failures ? 1 : 0;
}
