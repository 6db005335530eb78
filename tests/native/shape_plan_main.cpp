// shape_plan_main.cpp — walks the run plan of csrc/shape_plan.h (which molecules a workgroup of mdhip_mol_shape owns, and
// which form of the kernel works them) over fixed tables and seeded random ones; tests/test_shape_plan_native_cpu.py
// builds it with g++ under -fsanitize=address,undefined. The header is host arithmetic only.
// Fixed tables: 255 / 256 / 257 molecules of 3 atoms (runs end at the molecule limit), 64 / 65 molecules of 16 atoms (at
// the atom limit), lengths 1, 1024 and 1025 (the last stage, the first walk), jobs without molecules at the front, in
// the middle and at the end. Checked for every table: the runs of a job are contiguous, ascending and cover its
// molecules exactly once; no run crosses a job; a staged run holds at most SH_MOLS molecules and SH_CAP atoms and is as
// long as those limits allow unless it is the job's last; walk runs hold the jobs longer than SH_CAP; series0 is the
// prefix sum of job_mols; a rejected table names the FIRST offending job and its rule and holds no run; the mass sums
// are the index-order sums.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../mdproptools_amd/csrc/shape_plan.h"

static long failures = 0, n_plans = 0, n_rejected = 0, n_walk = 0, n_runs = 0;
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

static void check(const Table &t, const char *name)
{
    const int J = (int)t.mols.size();
    char buf[160];
    snprintf(buf, sizeof buf, "%s: %d jobs", name, J);
    what = buf;
    const ShPlan pl = shape_plan(J, t.atom0.data(), t.mols.data(), t.len.data(), t.n_atoms, t.n_frames);
    ++n_plans;
    int bad_range = -1, bad_result = -1;
    long long sum = 0, runs = 0;
    for (int j = 0; j < J && bad_range < 0; ++j) {
        if (!in_range(t, j)) {
            bad_range = j;
            break;
        }
        sum += t.mols[j];
        const long long per = t.len[j] > SH_CAP ? SH_MOLS : std::min<long long>(SH_MOLS, SH_CAP / t.len[j]);
        runs += (t.mols[j] + per - 1) / per;
        if ((sum >= (1ll << 40) / t.n_frames || runs >= SH_MAX_RUNS) && bad_result < 0) bad_result = j;
    }
    if (bad_range >= 0 || bad_result >= 0) {
        ++n_rejected;
        if (bad_range >= 0) CHECK(pl.error == MOL_PLAN_RANGE && pl.bad_job == bad_range && pl.checked_jobs() == bad_range);
        else CHECK(pl.error == MOL_PLAN_RESULT && pl.bad_job == bad_result && pl.checked_jobs() == J);
        CHECK(pl.staged.empty() && pl.walk.empty());
        return;
    }
    CHECK(pl.error == MOL_PLAN_OK && pl.bad_job == -1 && pl.checked_jobs() == J && (int)pl.series0.size() == J);
    if (pl.error != MOL_PLAN_OK || (int)pl.series0.size() != J) return;
    long long series = 0;
    for (int j = 0; j < J; ++j) {
        CHECK(pl.series0[(size_t)j] == series);
        series += t.mols[j];
    }
    CHECK(pl.series == series);
    CHECK((long long)(pl.staged.size() + pl.walk.size()) == runs);
    // every list: job after job, the runs of a job ascending from 0 without gap or overlap
    std::vector<long long> covered((size_t)J, 0);
    for (int list = 0; list < 2; ++list) {
        const std::vector<ShRun> &rs = list ? pl.walk : pl.staged;
        int last_job = -1;
        for (size_t k = 0; k < rs.size(); ++k, ++n_runs) {
            const ShRun &r = rs[k];
            CHECK(r.job >= 0 && r.job < J && r.job >= last_job);
            if (r.job < 0 || r.job >= J) return;
            last_job = r.job;
            const long long len = t.len[r.job], mols = t.mols[r.job];
            CHECK((len > SH_CAP) == (list == 1));
            CHECK(r.nm >= 1 && r.nm <= SH_MOLS && r.m0 == covered[(size_t)r.job] && r.m0 + r.nm <= mols);
            const long long per = sh_run_mols(len);
            if (!list) CHECK((long long)r.nm * len <= SH_CAP && per * len <= SH_CAP && ((per + 1) * len > SH_CAP || per == SH_MOLS));
            CHECK(r.nm == per || r.m0 + r.nm == mols);  // (only a job's last run is short)
            CHECK(t.atom0[r.job] + (r.m0 + r.nm) * len <= t.n_atoms);
            covered[(size_t)r.job] += r.nm;
            n_walk += list;
        }
    }
    for (int j = 0; j < J; ++j) CHECK(covered[(size_t)j] == t.mols[j]);
}

static void check_sums(std::mt19937_64 &rng)
{
    what = "mass sums";
    std::vector<int32_t> len = {1, 3, 16, 1025};
    std::vector<int64_t> off = {0};
    std::vector<double> w;
    for (int32_t l : len) {
        for (int k = 0; k < l; ++k) w.push_back(1.0 + (double)(rng() % 1000) / 7.0);
        off.push_back((int64_t)w.size());
    }
    const std::vector<double> sums = shape_mass_sums((int)len.size(), len.data(), off.data(), w.data());
    CHECK(sums.size() == len.size());
    for (size_t j = 0; j < len.size(); ++j) {
        double m = 0.0;
        for (int64_t k = off[j]; k < off[j + 1]; ++k) m += w[(size_t)k];
        CHECK(sums[j] == m);
    }
}

// frame slices: within gridDim.y and the frames; at most SH_FRAMES frames per workgroup unless gridDim.y is full; enough
// (run, slice) pairs for 16 workgroups per compute unit where the frames allow it
static void check_slices()
{
    what = "frame slices";
    for (long long runs : {1ll, 2ll, 300ll, 391ll, 4096ll, 4097ll, SH_MAX_RUNS - 1})
        for (long long frames : {1ll, 2ll, 15ll, 16ll, 17ll, 65ll, 300ll, 65535ll, 65536ll, 131071ll, 16 * 65535ll, 16 * 65535ll + 1, (1ll << 31) - 1})
            for (int cu : {1, 64, 256}) {
                const long long g = shape_frame_slices(runs, frames, cu), top = std::min(frames, SH_MAX_GRID_Y);
                CHECK(g >= 1 && g <= top);
                CHECK(g == top || (frames + g - 1) / g <= SH_FRAMES);
                CHECK(g == top || g * runs >= 16ll * cu);
            }
}

int main(int argc, char **argv)
{
    check_slices();
    {
        Table t;
        int64_t a = 0;
        for (int64_t m : {255, 256, 257, 1, 0, 513}) t.add(a, m, 3), a += 3 * m;
        for (int64_t m : {64, 65, 63, 128}) t.add(a, m, 16), a += 16 * m;
        t.n_atoms = a, t.n_frames = 65;
        check(t, "either side of the stage");
    }
    {
        Table t;
        int64_t a = 0;
        for (int32_t l : {1, 1024, 1025, 1023, 513, 512, 5, 4, 2000}) t.add(a, 300, l), a += 300ll * l;
        t.n_atoms = a + 3, t.n_frames = 3;
        check(t, "lengths about the stage");
    }
    {
        Table t;
        t.n_atoms = 1000, t.n_frames = 65;
        t.add(0, 0, 4), t.add(0, 65, 4), t.add(260, 0, 4), t.add(260, 1, 4), t.add(0, 0, 2000), t.add(264, 0, 3);
        check(t, "empty jobs");
    }
    {  // rejected: each rule at the first, a middle and the last job, and two at once
        const int64_t bad[][3] = {{0, 5, 0}, {0, -1, 3}, {-1, 2, 3}, {101, 0, 3}, {98, 2, 2}, {0, 34, 3}};
        for (const auto &b : bad)
            for (int at : {0, 2, 4}) {
                Table t;
                t.n_atoms = 100, t.n_frames = 7;
                for (int j = 0; j < 5; ++j) t.add(j, 3, 4);
                t.atom0[(size_t)at] = b[0], t.mols[(size_t)at] = b[1], t.len[(size_t)at] = (int32_t)b[2];
                check(t, "one bad job");
                t.len[4] = 0;
                check(t, "two bad jobs");
            }
        Table t;  // series * n_frames reaches 2^40 with job 2
        t.n_atoms = 1ll << 30, t.n_frames = 1 << 12;
        t.add(0, (1 << 26), 4), t.add(0, (1 << 27), 8), t.add(5, (1 << 26), 8), t.add(0, 1, 1);
        check(t, "result too large");
        Table u;  // the runs reach 2^22 with job 1
        u.n_atoms = 1ll << 34, u.n_frames = 1;
        u.add(0, (SH_MAX_RUNS - 3) * 10 - 5, 100), u.add(0, 21, 100), u.add(0, 0, 1);
        check(u, "too many runs");
        u.mols[1] = 11;
        check(u, "runs just fit");
    }
    const int n_random = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20261021);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    check_sums(rng);
    for (int k = 0; k < n_random; ++k) {
        Table t;
        t.n_frames = k % 11 == 0 ? pick(1, (1ll << 31) - 1) : pick(1, 300);
        const long long counts[] = {0, 1, 63, 64, 65, 255, 256, 257, 1000};
        const long long lens[] = {1, 2, 3, 4, 5, 7, 16, 100, 341, 342, 512, 513, 1024, 1025, 3000};
        const int J = (int)pick(1, 12);
        long long atoms = 0;
        for (int j = 0; j < J; ++j) {
            const long long m = counts[pick(0, 8)], l = lens[pick(0, 14)];
            t.add(atoms, m, (int32_t)l);
            atoms += m * l;
        }
        t.n_atoms = atoms + pick(0, 3) + (atoms == 0);
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
        check(t, "random");
    }
    printf("plans %ld rejected %ld walk %ld runs %ld failures %ld\n", n_plans, n_rejected, n_walk, n_runs, failures);
    return failures ? 1 : 0;
}
