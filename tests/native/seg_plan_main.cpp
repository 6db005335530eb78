// seg_plan_main.cpp — walks the plans of csrc/seg_plan.h (the host-only decision of the per-molecule COM and charge-flux
// calls) over the cases given in a file (tests/test_seg_plan_native_cpu.py writes the tables of tests/segment_exact.py
// there, under every option set of its CONFIGS) and over seeded random tables; the test builds it under
// -fsanitize=address,undefined. Per line of the file:
//   flux seg_frame seg_cap seg_vec seg_gy n_attr n_frames n_seg size[0..n_seg)
// and per line one line "pick <kernel name>" comes out, which the test holds against segment_exact.expected_kernel.
// Checked for every plan and for cu_count 16, 128, 256, 304: every segment lies in exactly one run and the runs are in
// order; a run holds at most `cap` atoms and `max_segs` segments; a SegRun's a0 / na are the offsets of its run; the
// grid is what the kernels are launched with (1 <= gy <= 65535); the name is the instance (form, cap, threads) says; the
// walk form is chosen exactly when a segment exceeds 1024 atoms; seg_sums equals a plain index-order loop bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "../../mdproptools_amd/csrc/seg_plan.h"

static long failures = 0;
static std::string what;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                \
    } while (0)

struct Case {
    int flux = 0, n_attr = 3;
    long long n_frames = 1;
    SegOptions opt;
    std::vector<int64_t> off;  // [n_seg + 1]
};

static long counts[3];

static const char *check(const Case &c, int cu_count)
{
    const int64_t n_seg = (int64_t)c.off.size() - 1, *off = c.off.data();
    const long long n_frames = c.n_frames;
    const SegPlan pl = seg_plan(c.opt, cu_count, n_seg, off, c.n_attr, n_frames, c.flux != 0);
    char buf[256];
    snprintf(buf, sizeof buf, "flux %d frame %d cap %d gy %d K %d F %lld M %lld N %lld cu %d form %d", c.flux, c.opt.frame, c.opt.cap,
             c.opt.gy, c.n_attr, n_frames, (long long)n_seg, (long long)off[n_seg], cu_count, pl.form);
    what = buf;
    long long longest = 0;
    for (int64_t s = 0; s < n_seg; ++s) longest = std::max<long long>(longest, off[s + 1] - off[s]);
    CHECK(pl.form == SEG_WALK || pl.form == SEG_STAGED || pl.form == SEG_FRAME);
    if (pl.form < SEG_WALK || pl.form > SEG_FRAME) return pl.name;
    ++counts[pl.form];
    CHECK((pl.form == SEG_WALK) == (longest > 1024));
    CHECK(pl.gy >= 1 && pl.gy <= 65535);
    CHECK(pl.vec == c.opt.vec);
    const char *fl = c.flux ? "true" : "false";
    char name[96];
    if (pl.form == SEG_WALK) {
        CHECK(pl.blocks.empty() && pl.runs.empty());
        CHECK(pl.gx == (unsigned)((n_seg + 255) / 256) && pl.threads == 256);
        CHECK(pl.gy == (unsigned)std::min<long long>(n_frames, 4096) && pl.n_steps == n_frames);
        CHECK(strcmp(pl.name, c.flux ? "mol_flux_kernel" : "segment_com_kernel") == 0);
        return pl.name;
    }
    // the stage: what the options ask for where it holds the longest segment, else 1024
    const bool picked = c.opt.cap == 0 && c.opt.frame != 0;
    if (picked) CHECK(pl.cap == 1024 || (pl.cap == 512 && longest <= 512));
    else CHECK(pl.cap == ((c.opt.cap == 256 || c.opt.cap == 512) && longest <= c.opt.cap ? c.opt.cap : 1024));
    CHECK(pl.max_segs() == (pl.cap == 256 ? 64 : 256));
    CHECK((pl.form == SEG_FRAME) == (c.opt.frame != 0 && pl.cap != 256));
    CHECK(pl.threads == (pl.form == SEG_STAGED && pl.cap == 256 ? 64 : 256));
    CHECK(pl.gx == pl.blocks.size() && !pl.blocks.empty());
    long long next = 0;
    for (const SegBlock &b : pl.blocks) {
        CHECK(b.s0 == next && b.s1 > b.s0 && b.s1 <= n_seg);
        if (b.s0 != next || b.s1 <= b.s0 || b.s1 > n_seg) return pl.name;
        CHECK(b.s1 - b.s0 <= pl.max_segs() && off[b.s1] - off[b.s0] <= pl.cap);
        next = b.s1;
    }
    CHECK(next == n_seg);
    if (pl.form == SEG_FRAME) {
        CHECK(pl.runs.size() == pl.blocks.size());
        for (size_t i = 0; i < pl.runs.size() && i < pl.blocks.size(); ++i) {
            const SegRun &r = pl.runs[i];
            const SegBlock &b = pl.blocks[i];
            CHECK(r.s0 == b.s0 && r.s1 == b.s1 && r.a0 == off[b.s0] && r.na == off[b.s1] - off[b.s0] && r.pad_ == 0);
        }
        CHECK(pl.n_steps == n_frames * ((c.n_attr + 2) / 3));
        CHECK(pl.gy == (unsigned)std::min<long long>(pl.n_steps, 65535));
        snprintf(name, sizeof name, "segment_frame_kernel<%s, %d>", fl, pl.cap);
    } else {
        CHECK(pl.runs.empty() && pl.n_steps == n_frames && pl.gy <= n_frames);
        const long long nb = (long long)pl.blocks.size();
        const long long want = std::max<long long>((16LL * cu_count + nb - 1) / nb, n_frames / 10);
        const long long lim = std::min<long long>(n_frames, 65535);
        CHECK(pl.gy == (c.opt.gy > 0 ? std::min<long long>(lim, c.opt.gy) : std::max<long long>(1, std::min(lim, want))));
        snprintf(name, sizeof name, "segment_staged_kernel<%s, %d, %d>", fl, pl.cap, pl.threads);
    }
    CHECK(strcmp(pl.name, name) == 0);
    return pl.name;
}

// seg_sums against a plain loop, with and without charges
static void check_sums(const Case &c, std::mt19937_64 &rng)
{
    const int64_t n_seg = (int64_t)c.off.size() - 1, *off = c.off.data();
    std::uniform_real_distribution<double> um(1.0, 40.0);
    std::normal_distribution<double> nq(0.0, 1.0);
    std::vector<double> m((size_t)off[n_seg]), q(m.size()), sums, want_m((size_t)n_seg), want_q((size_t)n_seg);
    for (size_t a = 0; a < m.size(); ++a) m[a] = um(rng), q[a] = nq(rng);
    for (int64_t s = 0; s < n_seg; ++s) {
        double sm = 0.0, sq = 0.0;
        for (int64_t a = off[s]; a < off[s + 1]; ++a) sm += m[(size_t)a];
        for (int64_t a = off[s]; a < off[s + 1]; ++a) sq += q[(size_t)a];
        want_m[(size_t)s] = sm;
        want_q[(size_t)s] = sq;
    }
    what = "seg_sums";
    sums = seg_sums(n_seg, off, m.data(), q.data());
    CHECK(sums.size() == 2 * (size_t)n_seg);
    if (sums.size() == 2 * (size_t)n_seg) {
        CHECK(memcmp(sums.data(), want_m.data(), (size_t)n_seg * 8) == 0);
        CHECK(memcmp(sums.data() + n_seg, want_q.data(), (size_t)n_seg * 8) == 0);
    }
    sums = seg_sums(n_seg, off, m.data(), nullptr);
    CHECK(sums.size() == (size_t)n_seg && memcmp(sums.data(), want_m.data(), sums.size() * 8) == 0);
}

int main(int argc, char **argv)
{
    const int cus[] = {16, 128, 256, 304};
    std::mt19937_64 rng(20261019);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    size_t n_file = 0;
    if (argc > 1) {
        FILE *fh = fopen(argv[1], "r");
        if (!fh) return 2;
        Case c;
        long long n_seg;
        while (fscanf(fh, "%d %d %d %d %d %d %lld %lld", &c.flux, &c.opt.frame, &c.opt.cap, &c.opt.vec, &c.opt.gy, &c.n_attr, &c.n_frames,
                      &n_seg) == 8) {
            if (n_seg < 1 || n_seg > 100000) return 2;
            c.off.assign((size_t)n_seg + 1, 0);
            for (long long s = 0; s < n_seg; ++s) {
                long long v;
                if (fscanf(fh, "%lld", &v) != 1 || v < 1) return 2;
                c.off[(size_t)s + 1] = c.off[(size_t)s] + v;
            }
            const char *name = nullptr;
            for (int cu : cus) {
                const char *n = check(c, cu);
                what += " (the kernel must not depend on the CU count)";
                CHECK(!name || strcmp(n, name) == 0);
                name = n;
            }
            printf("pick %s\n", name);
            if (n_file++ % 16 == 0) check_sums(c, rng);
        }
        fclose(fh);
    }
    const int n_random = argc > 2 ? atoi(argv[2]) : 3000;
    for (int k = 0; k < n_random; ++k) {
        Case c;
        // segment sizes 1 .. 1100, mostly small; runs of one-atom segments around the 64 / 256 segments-per-run limits
        const long long smax[] = {1, 4, 16, 40, 255, 257, 511, 513, 1023, 1025, 1100};
        const long long top = smax[pick(0, 10)], pieces = pick(1, 12);
        c.off.assign(1, 0);
        for (long long p = 0; p < pieces; ++p) {
            const bool ones = k % 3 == 0 && p % 2 == 0;
            const long long n = ones ? (p % 4 ? 256 : 64) + pick(-2, 2) : pick(1, 60);
            for (long long s = 0; s < n; ++s) {
                // (a table whose top size is large holds a few large segments among small ones)
                const long long len = ones ? 1 : top > 40 && pick(0, 9) ? pick(1, 8) : pick(1, top);
                c.off.push_back(c.off.back() + len);
            }
        }
        const int caps[] = {0, 0, 256, 512, 1024, 100};
        c.opt.cap = caps[pick(0, 5)];
        c.opt.frame = (int)pick(0, 1);
        c.opt.vec = (int)pick(0, 1);
        c.opt.gy = k % 4 == 0 ? (int)pick(1, 5) : k % 29 == 0 ? 70000 : 0;
        c.flux = (int)pick(0, 1);
        c.n_attr = c.flux ? 3 : (int)pick(1, 7);
        c.n_frames = k % 17 == 0 ? pick(60000, 200000) : pick(1, 300);
        for (int cu : cus) check(c, cu);
        if (k % 8 == 0) check_sums(c, rng);
    }
    printf("plans %zu (%zu from the file) forms walk %ld staged %ld frame %ld failures %ld\n", (n_file + (size_t)n_random) * 4, n_file,
           counts[0], counts[1], counts[2], failures);
    return failures ? 1 : 0;
}
