// lag_plan_main.cpp — walks the work tables of csrc/lag_plan.h (the host-only plan of the full-lag MSD paths) over the
// shapes given in a file (tests/test_lag_plan_native_cpu.py writes tests/lag_plan_cases.py there) and over seeded random
// shapes; the test builds it under -fsanitize=address,undefined. Per line of the file:
//   F E max_lag G off[0..G] variant w1 w12_min_f fft_kernel direct residue overlap batch_mb batched_fuse
// Checked for every shape and for cu_count 16, 128, 256, 304: every column of a non-empty segment is covered exactly once
// by the items and no other column is; seg_off / batch_off are monotone and end at the item count; a staged plan has one
// stage per item and hands out exactly cu_count / 16 clusters; a residue fold lies inside its batch and max_items bounds
// its rows.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../mdproptools_amd/csrc/lag_plan.h"

using namespace lagplan;

static long failures = 0;
static std::string what;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                \
    } while (0)

struct Shape {
    long long F, E, max_lag, G;
    std::vector<int64_t> off;
    LagOptions opt;
};

static long counts[5];

static void check(const Shape &s, int cu_count, const LagLds &need, bool aligned)
{
    LagDevice dev;
    dev.cu_count = cu_count;
    dev.lds_max = 160 * 1024;
    dev.need = need;
    dev.part_cus0 = lag_part_cus0(cu_count);
    LagProblem p;
    p.F = s.F;
    p.E = s.E;
    p.max_lag = (int)s.max_lag;
    p.G = s.G;
    p.group_off = s.off.data();
    p.r_aligned16 = aligned;
    p.two_pass_ok = lag_pow2_length(s.F + s.max_lag) >= 2048;
    const LagPlan pl = lag_choose(dev, s.opt, p);
    char buf[256];
    snprintf(buf, sizeof buf, "F %lld E %lld lag %lld G %lld cu %d path %d src %d", s.F, s.E, s.max_lag, s.G, cu_count, pl.path, pl.src);
    what = buf;
    CHECK(pl.path >= LAG_W1 && pl.path <= LAG_BATCHED);
    ++counts[pl.path];
    const long long cols = 3 * s.E, S = 3 * s.G;
    std::vector<int> want((size_t)cols, 0), got((size_t)cols, 0);
    long long nonempty = 0;
    lag_segments(s.E, s.G, s.off.data(), 0, cols, [&](long long, long long lo, long long hi) {
        nonempty += hi > lo;
        for (long long c = lo; c < hi; ++c) ++want[(size_t)c];
    });
    CHECK(pl.path == LAG_POW2 || pl.path == LAG_W12 || (pl.n_batches >= 1 && pl.n_batches * pl.nb0 >= cols));
    if (pl.path == LAG_POW2 || pl.path == LAG_W12) {
        std::vector<LagItem> items;
        std::vector<LagStage> stages;
        std::vector<int> seg_off;
        const int given = lag_fused_items(pl, cu_count, s.E, s.G, s.off.data(), items, stages, seg_off);
        CHECK(pl.m >= 3 && pl.m <= FT_MAX_M);
        CHECK((int)seg_off.size() == S + 1 && seg_off[0] == 0 && seg_off[(size_t)S] == (int)items.size());
        for (long long q = 0; q < S; ++q) CHECK(seg_off[(size_t)q] <= seg_off[(size_t)q + 1]);
        std::vector<int> row_seen(items.size(), 0);
        if (pl.src != 0) {
            CHECK(nonempty >= 1 && nonempty <= pl.n_clusters);
            CHECK(given == cu_count / 16 && (long long)items.size() == 16LL * given);
        }
        if (pl.staged()) CHECK(stages.size() == items.size());
        else CHECK(stages.empty());
        for (size_t i = 0; i < items.size(); ++i) {
            const LagItem &it = items[i];
            CHECK(it.row >= 0 && it.row < (int)items.size());
            if (it.row < 0 || it.row >= (int)items.size()) continue;
            ++row_seen[(size_t)it.row];
            if (pl.src != 1) CHECK(it.row == (int)i);
            // the segment that owns the row
            long long seg = 0;
            while (seg + 1 < S && seg_off[(size_t)seg + 1] <= it.row) ++seg;
            const long long a = seg / s.G, g = seg % s.G, lo = a * s.E + s.off[(size_t)g], hi = a * s.E + s.off[(size_t)g + 1];
            if (pl.staged()) {
                const LagStage &st = stages[i];
                CHECK(st.k == (int)(i % 16) && st.cluster == (int)(i / 16) && st.lo == lo && st.hi == hi && it.step == 1);
                CHECK(it.c_lo >= 0 && it.c_lo <= it.c_hi && 16 * it.c_hi <= cols + 15);
                for (long long T = it.c_lo; T < it.c_hi; ++T) {
                    const long long col = 16 * T + st.k;
                    if (col >= st.lo && col < st.hi && col < cols) ++got[(size_t)col];
                }
            } else {
                CHECK(it.step == (pl.src == 1 ? 16 : 1) && it.c_lo <= it.c_hi && (it.c_lo == it.c_hi || (it.c_lo >= lo && it.c_hi <= hi)));
                for (long long col = it.c_lo; col < it.c_hi && col < cols && col >= 0; col += it.step) ++got[(size_t)col];
            }
        }
        for (int r : row_seen) CHECK(r == 1);
        CHECK(got == want);
    } else if (pl.path != LAG_BATCHED) {
        const LagResidueItems r = lag_residue_items(pl, dev, s.E, s.G, s.off.data());
        CHECK((long long)r.batch_off.size() == pl.n_batches + 1 && r.batch_off[0] == 0 && r.batch_off.back() == (int)r.items.size());
        size_t fi = 0;
        for (long long b = 0; b < pl.n_batches; ++b) {
            const long long c_first = b * pl.nb0, nb = std::min(pl.nb0, cols - c_first);
            CHECK(nb >= 0 && r.batch_off[(size_t)b] <= r.batch_off[(size_t)b + 1]);
            int rows = 0;
            for (; fi < r.folds.size() && r.folds[fi].batch == b; ++fi) {
                const LagFold &f = r.folds[fi];
                CHECK(f.seg >= 0 && f.seg < S && f.c_n >= 1 && f.c_lo >= c_first && f.c_lo + f.c_n <= c_first + nb);
                CHECK(f.first == rows && f.count >= 1 && f.first + f.count <= r.max_items);
                CHECK((f.c_n + 64 * TSQ_TILES - 1) / (64 * TSQ_TILES) <= r.max_tiles);
                rows += f.count;
            }
            CHECK(rows == r.batch_off[(size_t)b + 1] - r.batch_off[(size_t)b] && rows <= r.max_items);
            for (int i = r.batch_off[(size_t)b]; i < r.batch_off[(size_t)b + 1]; ++i) {
                const LagItem &it = r.items[(size_t)i];
                CHECK(it.step == 1 && it.row == i - r.batch_off[(size_t)b] && it.c_lo >= 0 && it.c_lo < it.c_hi && it.c_hi <= nb);
                for (long long col = std::max(0LL, it.c_lo); col < it.c_hi && c_first + col < cols; ++col) ++got[(size_t)(c_first + col)];
            }
        }
        CHECK(fi == r.folds.size());
        CHECK(got == want);
    }
}

int main(int argc, char **argv)
{
    std::vector<Shape> shapes;
    if (argc > 1) {
        FILE *fh = fopen(argv[1], "r");
        if (!fh) return 2;
        Shape s;
        while (fscanf(fh, "%lld %lld %lld %lld", &s.F, &s.E, &s.max_lag, &s.G) == 4) {
            if (s.G < 1 || s.G > 1000) return 2;
            s.off.assign((size_t)s.G + 1, 0);
            for (auto &o : s.off) {
                long long v;
                if (fscanf(fh, "%lld", &v) != 1) return 2;
                o = v;
            }
            LagOptions &o = s.opt;
            if (fscanf(fh, "%d %d %d %d %d %d %d %d %d", &o.variant, &o.w1, &o.w12_min_f, &o.fft_kernel, &o.direct, &o.residue,
                       &o.overlap, &o.batch_mb, &o.batched_fuse) != 9)
                return 2;
            shapes.push_back(s);
        }
        fclose(fh);
    }
    const size_t n_file = shapes.size();
    std::mt19937_64 rng(12345);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    const int n_random = argc > 2 ? atoi(argv[2]) : 3000;
    for (int k = 0; k < n_random; ++k) {
        Shape s;
        const long long fmax[] = {40, 1600, 3100, 6200, 8300, 12400, 24700, 30000};
        s.F = pick(2, fmax[pick(0, 7)]);
        s.E = pick(1, k % 3 ? 300 : 40);
        s.max_lag = k % 4 ? s.F - 1 : pick(0, s.F - 1);
        s.G = pick(1, 24);
        s.off.resize((size_t)s.G + 1);
        for (auto &o : s.off) o = pick(0, k % 5 ? s.E : std::min<long long>(s.E, 3));  // (few distinct values: empty groups)
        std::sort(s.off.begin(), s.off.end());
        if (k % 7 == 0) s.off.front() = 0, s.off.back() = s.E;
        LagOptions &o = s.opt;
        o.variant = k % 11 == 0 ? 4 : 3;
        o.w1 = k % 13 != 0;
        o.w12_min_f = k % 17 == 0 ? 0 : 1536;
        o.fft_kernel = k % 3 == 0 ? (int)pick(0, 3) : 3;
        o.direct = k % 2 == 0 ? (int)pick(-1, 3) : -1;
        o.residue = k % 5 == 0 ? (int)pick(0, 2) : 1;
        o.overlap = k % 6 == 0 ? (int)pick(0, 2) : 0;
        o.batch_mb = k % 4 == 0 ? (int)pick(1, 64) : 4096;
        o.batched_fuse = (int)pick(0, 2);
        shapes.push_back(s);
    }
    const int cus[] = {16, 128, 256, 304};
    LagLds fits, tight;  // every kernel fits | the 12 288-point, the third power-of-two and the residue kernels do not
    tight.w12 = tight.residue = (size_t)1 << 20;
    for (auto &v : tight.f3) v = (size_t)1 << 20;
    for (size_t i = 0; i < shapes.size(); ++i)
        for (int cu : cus) {
            check(shapes[i], cu, fits, true);
            if (i % 4 == 0) check(shapes[i], cu, tight, true);
            if (i % 8 == 1) check(shapes[i], cu, fits, false);
        }
    printf("shapes %zu (%zu from the file) paths w1 %ld pow2 %ld w12 %ld residue %ld batched %ld failures %ld\n", shapes.size(), n_file,
           counts[0], counts[1], counts[2], counts[3], counts[4], failures);
    return failures ? 1 : 0;
}
