// mol_plan_main.cpp — walks the job plan of csrc/mol_tile.h (the host-only part: which class a job of mdhip_axis_vectors or
// mdhip_dihedral_angles joins, where its series and the class's molecule tiles start) over fixed tables and seeded
// random ones; tests/test_mol_plan_native_cpu.py builds it with g++ under -fsanitize=address,undefined. g++ sees
// nothing of the header's device and launch parts.
// Fixed tables: jobs without molecules at the front, in the middle and at the end; keys (atom0, mols, len) repeated
// with others in between (A, B, A); a class that fills to a lowered max_class_jobs and opens again; 63 / 64 / 65 / 128
// molecules. Checked for every table, pooled and not: every job stands at exactly one position, the positions of a
// class are contiguous, in call order and of one key; the classes come in the order of their first job and are what a
// plain search through the classes so far gives; tile0 advances by ceil(mols / 64) exactly; series0 is the prefix sum
// of job_mols in call order; without pooling every job is a class of its own, at its own position; a rejected table
// names the FIRST offending job and its rule.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../mdproptools_amd/csrc/mol_tile.h"

static long failures = 0, n_plans = 0, n_rejected = 0, n_reopened = 0;
static std::string what;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                \
    } while (0)

struct Table {
    std::vector<int64_t> atom0, mols;
    std::vector<int32_t> len;
    int64_t n_atoms = 0, n_frames = 1;
    void add(int64_t a0, int64_t m, int32_t l) { atom0.push_back(a0), mols.push_back(m), len.push_back(l); }
};

static bool in_range(const Table &t, int j)
{
    const long long len = t.len[j], mols = t.mols[j], a0 = t.atom0[j];
    return len >= 1 && mols >= 0 && a0 >= 0 && a0 <= t.n_atoms && mols <= (t.n_atoms - a0) / len;
}

static void check(const Table &t, bool pool, int max_class_jobs, const char *name)
{
    const int J = (int)t.mols.size();
    char buf[160];
    snprintf(buf, sizeof buf, "%s: %d jobs, pool %d, max %d", name, J, (int)pool, max_class_jobs);
    what = buf;
    const MolPlan pl = mol_plan(J, t.atom0.data(), t.mols.data(), t.len.data(), t.n_atoms, t.n_frames, pool, max_class_jobs);
    ++n_plans;
    // what must be refused, and at which job
    int bad_range = -1, bad_result = -1;
    long long sum = 0;
    for (int j = 0; j < J && bad_range < 0; ++j) {
        if (!in_range(t, j)) bad_range = j;
        else if ((sum += t.mols[j]) >= (1ll << 40) / t.n_frames && bad_result < 0) bad_result = j;
    }
    if (bad_range >= 0) {
        ++n_rejected;
        CHECK(pl.error == MOL_PLAN_RANGE && pl.bad_job == bad_range && pl.checked_jobs() == bad_range);
        return;
    }
    if (bad_result >= 0) {
        ++n_rejected;
        CHECK(pl.error == MOL_PLAN_RESULT && pl.bad_job == bad_result && pl.checked_jobs() == J);
        return;
    }
    CHECK(pl.error == MOL_PLAN_OK && pl.bad_job == -1 && pl.checked_jobs() == J);
    CHECK((int)pl.order.size() == J && (int)pl.series0.size() == J);
    if (pl.error != MOL_PLAN_OK || (int)pl.order.size() != J || (int)pl.series0.size() != J) return;
    // series0: the prefix sum in call order
    long long series = 0;
    for (int j = 0; j < J; ++j) {
        CHECK(pl.series0[(size_t)j] == series);
        series += t.mols[j];
    }
    CHECK(pl.series == series);
    // the classes a plain search gives: a job joins the LAST class of its key unless that is full
    std::vector<std::vector<int>> want;
    for (int j = 0; j < J; ++j) {
        int c = -1;
        if (pool)
            for (int k = (int)want.size() - 1; k >= 0 && c < 0; --k) {
                const int j0 = want[(size_t)k][0];
                if (t.atom0[j0] == t.atom0[j] && t.mols[j0] == t.mols[j] && t.len[j0] == t.len[j]) c = k;
            }
        if (c >= 0 && (int)want[(size_t)c].size() >= max_class_jobs) c = -1, ++n_reopened;
        if (c < 0) want.emplace_back(), c = (int)want.size() - 1;
        want[(size_t)c].push_back(j);
    }
    CHECK(pl.classes.size() == want.size());
    if (!pool) CHECK((int)pl.classes.size() == J);
    if (pl.classes.size() != want.size()) return;
    std::vector<int> seen((size_t)J, 0);
    long long tile = 0;
    int pos = 0;
    for (size_t c = 0; c < want.size(); ++c) {
        const MolClass &cl = pl.classes[c];
        const int j0 = want[c][0];
        CHECK(cl.atom0 == t.atom0[j0] && cl.mols == t.mols[j0] && cl.len == t.len[j0] && cl.pad == 0);
        CHECK(cl.job0 == pos && cl.n_jobs == (int)want[c].size() && cl.n_jobs >= 1 && cl.n_jobs <= (pool ? max_class_jobs : 1));
        CHECK(cl.tile0 == tile);
        tile += cl.mols / MT_TM + (cl.mols % MT_TM != 0);
        if (cl.job0 != pos || cl.n_jobs != (int)want[c].size()) return;
        for (int k = 0; k < cl.n_jobs; ++k, ++pos) {
            const int j = pl.order[(size_t)pos];
            CHECK(j == want[c][(size_t)k]);  // (call order inside the class, the classes in the order of their first job)
            CHECK(j >= 0 && j < J);
            if (j < 0 || j >= J) return;
            ++seen[(size_t)j];
            CHECK(t.atom0[j] == cl.atom0 && t.mols[j] == cl.mols && t.len[j] == cl.len);
            if (!pool) CHECK(j == pos);
        }
    }
    CHECK(pos == J && pl.tiles == tile);
    for (int j = 0; j < J; ++j) CHECK(seen[(size_t)j] == 1);
}

static void check_all(const Table &t, const char *name)
{
    check(t, false, 1, name);
    for (int cap : {1, 2, 3, 1 << 16}) check(t, true, cap, name);
}

int main(int argc, char **argv)
{
    {  // jobs without molecules at the front, in the middle and at the end; A, B, A
        Table t;
        t.n_atoms = 1000, t.n_frames = 65;
        t.add(0, 0, 4), t.add(0, 65, 4), t.add(260, 0, 4), t.add(260, 1, 4), t.add(0, 65, 4), t.add(264, 0, 3);
        check_all(t, "empty jobs");
        Table u;
        u.n_atoms = 264, u.n_frames = 65;
        u.add(0, 65, 4), u.add(260, 0, 4), u.add(260, 1, 4);
        check_all(u, "(65, 0, 1)");
    }
    {  // a class that fills and opens again, other keys in between
        Table t;
        t.n_atoms = 64 * 5 + 128 * 2, t.n_frames = 3;
        for (int k = 0; k < 7; ++k) {
            t.add(0, 64, 5);
            if (k % 3 == 1) t.add(320, 128, 2);
        }
        check_all(t, "fill and reopen");
    }
    {  // molecule counts about the tile
        Table t;
        t.n_atoms = 4096, t.n_frames = 130;
        for (int64_t m : {63, 64, 65, 128, 1, 0, 640}) t.add(3, m, 6);
        check_all(t, "63 / 64 / 65 / 128");
    }
    {  // rejected: each rule at the first, a middle and the last job, and two at once
        const int64_t bad[][3] = {{0, 5, 0}, {0, -1, 3}, {-1, 2, 3}, {101, 0, 3}, {98, 2, 2}, {0, 34, 3}};
        for (const auto &b : bad)
            for (int at : {0, 2, 4}) {
                Table t;
                t.n_atoms = 100, t.n_frames = 7;
                for (int j = 0; j < 5; ++j) t.add(j, 3, 4);
                t.atom0[(size_t)at] = b[0], t.mols[(size_t)at] = b[1], t.len[(size_t)at] = (int32_t)b[2];
                check_all(t, "one bad job");
                t.len[4] = 0;
                check_all(t, "two bad jobs");
            }
        Table t;  // series * n_frames reaches 2^40 with job 2
        t.n_atoms = 1ll << 30, t.n_frames = 1 << 12;
        t.add(0, (1 << 26), 4), t.add(0, (1 << 27), 8), t.add(5, (1 << 26), 8), t.add(0, 1, 1);
        check_all(t, "result too large");
        t.mols[2] -= 1;
        check_all(t, "result just fits");
        t.mols[2] += 1, t.atom0[3] = t.n_atoms;  // (job 3 runs past the frame: that is reported, as the entry points do)
        check_all(t, "too large and out of range");
    }
    const int n_random = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20261020);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    for (int k = 0; k < n_random; ++k) {
        Table t;
        t.n_frames = k % 11 == 0 ? pick(1, (1ll << 31) - 1) : pick(1, 300);
        // a few molecule types one after the other; jobs draw from them, so that keys repeat
        const int n_types = (int)pick(1, 5);
        const long long counts[] = {0, 1, 63, 64, 65, 128, 129, 1000};
        std::vector<long long> a0, m, l;
        long long atoms = 0;
        for (int ty = 0; ty < n_types; ++ty) {
            a0.push_back(atoms), m.push_back(counts[pick(0, 7)]), l.push_back(pick(1, 9));
            atoms += m.back() * l.back();
        }
        t.n_atoms = atoms + pick(0, 3) + (atoms == 0);
        const int J = (int)pick(1, 40);
        for (int j = 0; j < J; ++j) {
            const size_t ty = (size_t)pick(0, n_types - 1);
            t.add(a0[ty], m[ty], (int32_t)l[ty]);
        }
        if (k % 7 == 0) {  // one or two jobs that must be refused
            for (int r = 0; r < 1 + k % 2; ++r) {
                const size_t j = (size_t)pick(0, J - 1);
                switch (pick(0, 3)) {
                case 0: t.len[j] = (int32_t)pick(-1, 0); break;
                case 1: t.mols[j] = -pick(1, 5); break;
                case 2: t.atom0[j] = t.n_atoms + pick(1, 9); break;
                default: t.mols[j] = t.n_atoms + 1; break;
                }
            }
        }
        check(t, false, 1, "random");
        check(t, true, k % 3 == 0 ? (int)pick(1, 4) : 1 << 16, "random");
    }
    printf("plans %ld rejected %ld reopened %ld failures %ld\n", n_plans, n_rejected, n_reopened, failures);
    return failures ? 1 : 0;
}
