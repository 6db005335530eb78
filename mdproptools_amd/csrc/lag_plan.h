// lag_plan.h — which spectral path one full-lag MSD call takes and the work tables of that path, decided from the
// problem's shape alone.
//
// Everything here is host arithmetic on plain values (two device limits, the lag_* options, the shape, the group
// offsets): no HIP header, no context, no device call. msd_fft.hip (the only includer inside the library) launches
// what lag_choose() returns; mdhip_lag_plan answers from the same function on a machine without a GPU, and
// tests/native/lag_plan_main.cpp walks the item tables under sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lagplan {

// The kernels' geometry as far as the decision reads it (msd_fft.hip asserts each against the kernels' own constant)
constexpr int W12_NW = 12, W12_SUB = 512, W12_N = W12_NW * W12_SUB, W12_UN = 4;  // msd_fft_w12.h
constexpr int FT_THREADS = 512, FT_MAX_M = 13, F3_MIN_M = 12, ST_UNITS = 8;      // the power-of-two kernels
constexpr int TSQ_TILES = 8;                                                     // transpose_centre64_sq_kernel

// LDS bytes the kernels need, from their own *_lds_bytes (msd_fft.hip: lag_lds_needs)
struct LagLds {
    size_t ft[FT_MAX_M + 1] = {}, f2[FT_MAX_M + 1] = {}, f3[FT_MAX_M + 1] = {};  // by m = log2 N
    size_t w12 = 0, w1 = 0, residue = 0;
};

struct LagDevice {
    int cu_count = 256;
    size_t lds_max = 65536;
    LagLds need;
    int part_cus0 = 0;  // CUs of the larger of the two CU-partitioned streams (lag_overlap); 0: there are none
};

// (as mdhip_part_streams splits the chip: every fourth group of 8 CUs goes to the streaming side)
inline int lag_part_cus0(int cu_count)
{
    if (cu_count < 64 || cu_count % 32 != 0) return 0;
    int n = 0;
    for (int i = 0; i < cu_count; ++i) n += (i / 8) % 4 != 3;
    return n;
}

// the context's lag_* options that the decision reads (defaults as ctx.h)
struct LagOptions {
    int variant = 3, w1 = 1, w12_min_f = 1536, fft_kernel = 3, direct = -1, residue = 1, overlap = 0, batch_mb = 4096,
        batched_fuse = 2;
};

struct LagProblem {
    long long F = 0, E = 0;
    int max_lag = 0;
    long long G = 0;
    const int64_t *group_off = nullptr;  // [G + 1]
    bool r_aligned16 = true;             // the trajectory's device address (16-byte loads of the staged kernels)
    bool two_pass_ok = false;            // fft_pow2.hip has a two-pass plan for the batched path's padded length
};

enum LagPath { LAG_W1 = 0, LAG_POW2 = 1, LAG_W12 = 2, LAG_RESIDUE = 3, LAG_BATCHED = 4 };
enum LagResidueKernel { RK_W1_1 = 1, RK_W1_2 = 2, RK_W1_3 = 3, RK_W12R_4 = 4, RK_W12P_SHARE = 5, RK_W12P_FOLD_W12O = 6 };

struct LagPlan {
    int path = LAG_BATCHED;
    bool too_long = false;  // batched: the padded length is beyond the transforms (the call fails)
    long long L = 0;        // padded length
    int m = 0;              // fused: the power of two at or above (F + max_lag) / 2; N = 2^m for the power-of-two kernels
    // fused (LAG_POW2 | LAG_W12)
    int gen = 0;            // LAG_POW2: 1 msd_power_lds_kernel, 2 _lds2_, 3 _lds3_
    int src = 0;            // 0 the transposed copy, 1 the trajectory as it is, 2 / 3 the clusters' staging rings
    int src_opt = 0;        // the option behind `src` (3 reaches the kernel as a negative row count)
    int Fc = 0;             // rows per cluster member
    int units = 0;          // staged: 16-byte units a lane moves per tile (w12: 4; power of two: 5, or 8 beyond 320 rows)
    int n_clusters = 0;
    int QR = 0, QR2 = 0, JJ = 0, QE = 0;  // the template instance: gen 1 | gen 2 | gen 3 (JJ, QE) | w12 (QE, SH)
    bool SH = false;
    // residue (LAG_W1 | LAG_RESIDUE)
    int short_d2 = 0;  // LAG_W1: padded length / 1024
    int D = 0;         // 4 | 8
    bool packed = false;
    int residue_kernel = 0;
    bool want_overlap = false, overlap = false;  // (overlap: wanted, and at least three batches)
    // batched
    int fuse = 0;  // 0 | 1 | 2
    // batches of whole series (residue, batched)
    long long n_batches = 1, nb0 = 0;
    const char *name = "";  // what mdhip_last_kernel_name reports after the call

    bool staged() const { return src >= 2; }
    bool w12() const { return path == LAG_W12; }
};

// The (axis, group) segments s = 3 G: fn(s, lo, hi) with the segment's columns [lo, hi) of the [F][3 E] matrix clipped
// to the batch [c_first, c_first + nb); hi <= lo: the batch holds nothing of it.
template <class Fn>
inline void lag_segments(long long E, long long G, const int64_t *group_off, long long c_first, long long nb, Fn &&fn)
{
    for (long long s = 0; s < 3 * G; ++s) {
        const long long a = s / G, g = s % G;
        const long long lo = std::max(c_first, a * E + (long long)group_off[g]);
        const long long hi = std::min(c_first + nb, a * E + (long long)group_off[g + 1]);
        fn(s, lo, hi);
    }
}

inline long long lag_pow2_length(long long n)
{
    long long L = 2;
    while (L < n) L <<= 1;
    return L;
}

// The single place that decides. `opt.direct` = 0 forces the transposed copy (the repeat after a stalled ring).
inline LagPlan lag_choose(const LagDevice &dev, const LagOptions &opt, const LagProblem &p)
{
    LagPlan pl;
    const long long F = p.F, E = p.E, G = p.G, max_lag = p.max_lag, cols = 3 * E;
    const bool spectral = opt.variant != 4;  // (4: the batched transforms whatever the length)

    // batches of whole series of the residue-class paths, `row_len` doubles each
    auto residue = [&](int short_d2) {
        pl.path = short_d2 ? LAG_W1 : LAG_RESIDUE;
        pl.short_d2 = short_d2;
        // D = 4: padded length 24 576, the series as they are; D = 8: 49 152, the series folded once by the transposition
        pl.D = short_d2 ? 4 : (F <= 2LL * W12_N && F + max_lag <= 4LL * W12_N) ? 4 : 8;  // (short: as D = 4 in what follows)
        pl.L = short_d2 ? 1024LL * short_d2 : (long long)pl.D * W12_N;
        // lag_residue 1 (default): two transforms per series (the even frequencies packed, the odd ones as class 1); 2: three
        // classes (0, 1, 2), nothing packed — the first form of the kernel, kept for A/B
        pl.packed = opt.residue != 2 || pl.D == 8;
        pl.residue_kernel = short_d2 ? short_d2 : !pl.packed ? RK_W12R_4 : pl.D == 4 ? RK_W12P_SHARE : RK_W12P_FOLD_W12O;
        pl.name = short_d2 ? "msd_power_w1_kernel"
                  : pl.D == 8 ? "msd_power_w12p_kernel + msd_power_w12o_kernel"
                  : pl.packed ? "msd_power_w12p_kernel"
                              : "msd_power_w12r_kernel";
        const long long row_len = pl.D == 4 ? F : 4LL * W12_N;  // doubles per series of the time-major copy
        // `lag_overlap`: two CU-masked streams, two buffers, at least three batches (msd_fft.hip: lag_msd_fft_residue)
        const bool want_overlap = opt.overlap != 0 && !short_d2 &&
                                  (cols * row_len * 8 >= (512LL << 20) || opt.overlap >= 2 /* tests: whatever the size */) &&
                                  dev.part_cus0 > 0;
        long long nb_max = std::max<long long>(1, ((long long)opt.batch_mb << 20) / (row_len * 8) / (want_overlap ? 2 : 1));
        if (want_overlap)
            nb_max = std::min(nb_max, std::max<long long>(opt.overlap >= 2 ? 1 : 4LL * dev.cu_count, (cols + 5) / 6));
        pl.n_batches = std::max<long long>(1, (cols + nb_max - 1) / nb_max);
        pl.nb0 = (cols + pl.n_batches - 1) / pl.n_batches;
        pl.want_overlap = want_overlap;
        pl.overlap = want_overlap && pl.n_batches >= 3;
        return pl;
    };

    // The fused LDS kernels: N = 2^m points, or (w12) 6144 = 12 x 512 with padded length 12 288
    auto fused = [&](int m, bool w12) {
        pl.path = w12 ? LAG_W12 : LAG_POW2;
        pl.m = m;
        const long long N = w12 ? (long long)W12_N : 1LL << m;
        pl.L = 2 * N;
        pl.name = w12 ? "msd_power_w12_kernel" : "msd_power_lds_kernel";
        // round-3 kernel (conflict-free layout, bilinear spectrum accumulation): N = 2^m a multiple of the block size
        const bool v2 = !w12 && opt.fft_kernel != 0 && m >= 9 && dev.need.f2[m] <= dev.lds_max;
        // second step of round 3 (first pass from registers, wave-private sub-transforms): lag_fft_kernel >= 2
        const bool v3 = !w12 && opt.fft_kernel >= 2 && m >= F3_MIN_M && dev.need.f3[m] <= dev.lds_max;
        pl.gen = w12 ? 0 : v3 ? 3 : v2 ? 2 : 1;
        // `lag_direct` 1: the third kernel reads the trajectory as it is, [F][3 E], no transposed copy. Needs the blocks in
        // whole clusters of 16 per XCD: 128 | cu_count.
        // `lag_direct` 2 (default) / 3: no transposed copy either, the clusters of 16 blocks transpose their own tiles inside
        // the kernel through a small ring: any 16 blocks, rows per member Fc = F / 16 rounded up to whole 128-byte lines.
        pl.n_clusters = dev.cu_count / 16;
        constexpr int LAG_DIRECT_DEFAULT = 2;  // where the series come from when the option is -1
        pl.src_opt = opt.direct >= 0 ? opt.direct : LAG_DIRECT_DEFAULT;
        pl.Fc = (int)((((F + 15) / 16) + 15) / 16 * 16);
        bool staged = (v3 || w12) && (pl.src_opt == 2 || pl.src_opt == 3) && dev.cu_count % 16 == 0 && pl.n_clusters >= 1 &&
                      (w12 ? pl.Fc <= 16 * (W12_NW / 2) * W12_UN
                           : pl.Fc <= 64 * ST_UNITS && (pl.Fc <= 64 * 5 || (m == 13 && F <= 8192))) &&  // (eight units: the N = 8192 kernels only)
                      cols >= 16 * (long long)pl.n_clusters &&
                      (unsigned long long)pl.Fc * (unsigned long long)cols * 8ull < 0xFFFFF000ull &&  // (a member's rows: one buffer)
                      p.r_aligned16;  // (16-byte loads of column pairs where the column count is even)
        bool direct = staged || (v3 && pl.src_opt == 1 && dev.cu_count % 128 == 0 && cols >= 16 * (long long)pl.n_clusters);
        if (direct) {
            // whole clusters go to segments (lag_fused_items: every non-empty segment at least one): a shape with more
            // non-empty segments than clusters — or none at all — keeps the transposed path
            long long nonempty = 0;
            lag_segments(E, G, p.group_off, 0, cols, [&](long long, long long lo, long long hi) { nonempty += hi > lo; });
            if (nonempty < 1 || nonempty > pl.n_clusters) {
                staged = direct = false;
                pl.src_opt = 0;
            }
        }
        pl.src = staged ? pl.src_opt : direct ? 1 : 0;
        // the template instance
        if (w12) {
            const int qe = std::max(4, (int)(((F + 1) / 2 + W12_SUB - 1) / W12_SUB));  // first-pass inputs that hold data: 4 .. 6
            pl.SH = F < 6 * W12_SUB;  // (1536 <= F < 3072)
            pl.QE = pl.SH || qe <= 4 ? 4 : qe == 5 ? 5 : 6;
            pl.units = staged ? W12_UN : 0;
        } else if (v3) {
            const long long s0 = N >> 3;
            const int qe = (int)(((F + 1) / 2 + s0 - 1) / s0);  // <= 8
            if (staged && pl.Fc > 64 * 5) {  // (eight staging units per lane and tile: rows per member beyond 320, F > 5120)
                pl.units = 8;
                pl.JJ = 2;
                pl.QE = qe <= 3 ? 3 : 4;
            } else {
                pl.units = staged ? 5 : 0;
                pl.JJ = s0 > FT_THREADS ? 2 : 1;
                pl.QE = qe <= 3 ? 3 : qe <= 4 ? 4 : 8;
            }
        } else if (v2) {
            // QR2 = sample pairs per lane: ceil(ceil(F / 2) / 512) <= N / 512 = 16 (16: F > N, only with max_lag < F - 1)
            const int qr2 = (int)(((F + 1) / 2 + FT_THREADS - 1) / FT_THREADS);
            pl.QR2 = qr2 <= 3 ? std::max(qr2, 1) : qr2 <= 5 ? 5 : qr2 <= 8 ? 8 : 16;
        } else {
            const int qr = (int)((F + FT_THREADS - 1) / FT_THREADS);
            pl.QR = qr <= 2 ? std::max(qr, 1) : qr <= 4 ? 4 : qr <= 8 ? 8 : qr <= 10 ? 10 : qr <= 12 ? 12 : qr <= 16 ? 16 : qr <= 24 ? 24 : 32;
        }
        return pl;
    };

    // round 6: trajectories below msd_power_w12_kernel's range, one wave per series (msd_fft_w12r.h): padded length 1024 / 2048 / 3072
    // (the residue-class host path launches its transposition and folds per (axis, group) segment: with many groups the
    // block-wide kernels, which take every segment in one launch, stay the faster choice for calls of a millisecond)
    if (spectral && opt.w1 != 0 && F + max_lag <= 3072 && F <= 1536 && F >= 2 && G <= 16 &&
        (F < std::max(3 * W12_SUB, opt.w12_min_f) || opt.w12_min_f <= 0 || F + max_lag <= 2048) && dev.need.w1 <= dev.lds_max)
        return residue((int)((F + max_lag + 1023) / 1024));
    if (spectral) {
        // fused LDS path when the padded series fits: L = power of two >= max(16, F + max_lag)
        int m = 3;
        while ((2LL << m) < F + max_lag) ++m;
        // round 5: padded length 12288 = 3 * 2^12 where 16384 would be the next power of two (msd_fft_w12.h)
        // round 6: the same kernel for 2048 < F + max_lag <= 8192 (m == 11, 12) from `lag_w12_min_f` frames on (default 1536,
        // the SHORT instance's lower limit): its twelve register-resident 512-point sub-transforms cost less per series than
        // the power-of-two kernels' 2048- and 4096-point transforms through LDS although it transforms 1.5-3 x the points
        // (tools/lag_sizes.py, profiles/r06_lag_sizes_ab.txt: E = 50 000, full lag, F = 1536 3.77 vs 3.78 ms, 2048 3.62 vs
        // 4.06, 3000 3.79 vs 5.43, 4096 4.02 vs 7.01)
        const bool w12_long = m == 13 && F >= 6 * W12_SUB;
        const bool w12_short = (m == 12 || m == 11) && F >= std::max(3 * W12_SUB, opt.w12_min_f) && opt.w12_min_f > 0;
        if (opt.fft_kernel >= 3 && (w12_long || w12_short) && F + max_lag <= 2 * W12_N && (F + 1) / 2 <= 6 * W12_SUB &&
            dev.need.w12 <= dev.lds_max)
            return fused(m, true);
        if (m <= FT_MAX_M && dev.need.ft[m] <= dev.lds_max) return fused(m, false);
    }
    // round 6: 16 384 < F + max_lag <= 24 576 (F <= 12 288) in residue classes of a 4 x 6144-point transform, F + max_lag <=
    // 49 152 (F <= 24 576) of an 8 x 6144-point one: no transform pass through HBM
    if (spectral && opt.residue != 0 && F + max_lag <= 8LL * W12_N && F <= 4LL * W12_N && dev.need.residue <= dev.lds_max)
        return residue(0);

    // the batched transforms (fft_pow2.hip). `lag_batched_fuse` 1: the first pass reads the centred series where the
    // transposition left them and the column sums are taken from the packed transform; 2 (default): the transform in two
    // passes, the second one fused with the column sums
    pl.path = LAG_BATCHED;
    pl.name = "lag_msd_fft";
    pl.L = lag_pow2_length(F + max_lag);
    pl.too_long = pl.L >= (1LL << 30);
    if (pl.too_long) return pl;
    const long long L = pl.L, K = L / 2 + 1;
    pl.fuse = opt.batched_fuse == 0 ? 0 : opt.batched_fuse >= 2 && p.two_pass_ok ? 2 : 1;
    // batches of whole series: (padded copy | centred series) + the transform buffers (+ spectrum) <= ~4 GiB
    const long long per_series = pl.fuse == 2 ? F * 8 + L * 8 : pl.fuse == 1 ? F * 8 + 2 * L * 8 : 2 * L * 8 + K * 16;
    const long long nb_max = std::max<long long>(1, std::min<long long>(((long long)opt.batch_mb << 20) / per_series, (1LL << 31) / K));
    pl.n_batches = std::max<long long>(1, (cols + nb_max - 1) / nb_max);
    pl.nb0 = (cols + pl.n_batches - 1) / pl.n_batches;
    return pl;
}

// One block's share of the series (FftItem of msd_fft.hip, field for field)
struct LagItem {
    long long c_lo, c_hi;  // series c_lo, c_lo + step, ... < c_hi of one segment
    int step;              // 1: a contiguous range; 16: one column of every 16-column tile (the direct-read kernel)
    int row;               // row of Qpart / Ppart the block writes (rows of one segment are consecutive)
};
// What a member of a staging cluster needs beside its item, whose c_lo / c_hi are the cluster's range of 16-column TILES
// (FftStage of msd_fft.hip)
struct LagStage {
    long long lo, hi;  // the segment's columns [lo, hi): a member whose column 16 T + k lies outside transforms zeros
    int k, cluster;    // member 0 .. 15: column 16 T + k of every tile; rows [k Fc, (k + 1) Fc) are its staging share
};

// Work items of the fused kernels: every non-empty segment gets a share of ~one block per CU, each a contiguous series
// range — or, where the series are read in place (src != 0), whole clusters of 16 blocks that walk the segment's
// 16-column tiles (aligned to 16 columns of the [F][cols] matrix = one 128-byte line per row), member k taking column
// 16 T + k. seg_off [3 G + 1]: the segments' first rows. -> the clusters given (src != 0: == pl.n_clusters).
inline int lag_fused_items(const LagPlan &pl, int cu_count, long long E, long long G, const int64_t *group_off,
                           std::vector<LagItem> &items, std::vector<LagStage> &stages, std::vector<int> &seg_off)
{
    const long long S = 3 * G, cols = 3 * E;
    items.clear();
    stages.clear();
    seg_off.assign((size_t)S + 1, 0);
    if (pl.src == 0) {
        lag_segments(E, G, group_off, 0, cols, [&](long long s, long long lo, long long hi) {
            const long long n = hi - lo;
            seg_off[(size_t)s] = (int)items.size();
            if (n <= 0) return;
            long long k = (n * cu_count + cols / 2) / cols;
            k = std::max<long long>(1, std::min(k, n));
            for (long long q = 0; q < k; ++q) items.push_back({lo + n * q / k, lo + n * (q + 1) / k, 1, (int)items.size()});
        });
        seg_off[(size_t)S] = (int)items.size();
        return 0;
    }
    // clusters per segment by largest remainder (every non-empty segment at least one: lag_choose has seen to it that
    // there are between one and n_clusters of them, so both loops below find a segment and end at n_clusters)
    const int n_clusters = pl.n_clusters;
    std::vector<long long> seg_n((size_t)S), seg_lo((size_t)S);
    std::vector<int> seg_c((size_t)S, 0);
    int given = 0;
    lag_segments(E, G, group_off, 0, cols, [&](long long s, long long lo, long long hi) {
        seg_lo[(size_t)s] = lo;
        seg_n[(size_t)s] = std::max(0LL, hi - lo);
        if (hi > lo) given += seg_c[(size_t)s] = std::max<int>(1, (int)((hi - lo) * n_clusters / cols));
    });
    while (given > n_clusters) {  // (the floor of 1 can overshoot when many segments are tiny)
        long long best = -1;
        for (long long s = 0; s < S; ++s)
            if (seg_c[s] > 1 && (best < 0 || seg_n[s] * seg_c[best] < seg_n[best] * seg_c[s])) best = s;
        if (best < 0) break;
        --seg_c[best];
        --given;
    }
    while (given > 0 && given < n_clusters) {  // the segment with the most columns per cluster takes the next one
        long long best = -1;
        for (long long s = 0; s < S; ++s)
            if (seg_n[s] > 0 && (best < 0 || seg_n[s] * seg_c[best] > seg_n[best] * seg_c[s])) best = s;
        ++seg_c[best];
        ++given;
    }
    // rows (= Qpart / Ppart rows, consecutive per segment): cluster q, member k -> row 16 q + k
    std::vector<LagItem> rows;
    for (long long s = 0; s < S; ++s) {
        seg_off[(size_t)s] = (int)rows.size();
        if (seg_c[s] == 0) continue;
        const long long lo = seg_lo[s], hi = lo + seg_n[s];
        const long long t0 = lo / 16, t1 = (hi + 15) / 16, nt = t1 - t0;
        for (int q = 0; q < seg_c[s]; ++q) {
            const long long ta = t0 + nt * q / seg_c[s], tb = t0 + nt * (q + 1) / seg_c[s];
            for (int k = 0; k < 16; ++k) {
                if (pl.staged()) {
                    // block 16 q + k = member k of cluster q (no placement assumption); c_lo / c_hi = the cluster's tiles
                    stages.push_back({lo, hi, k, (int)(rows.size() / 16)});
                    rows.push_back({ta, tb, 1, (int)rows.size()});
                } else {
                    long long c0 = 16 * ta + k, c1 = 16 * tb;  // columns 16 T + k, ta <= T < tb, inside [lo, hi)
                    while (c0 < lo) c0 += 16;
                    c1 = std::min(c1, hi);
                    rows.push_back({c0, std::max(c0, c1), 16, (int)rows.size()});
                }
            }
        }
    }
    seg_off[(size_t)S] = (int)rows.size();
    if (pl.staged() || given != n_clusters || n_clusters % 8 != 0) {
        items = rows;
        return given;
    }
    // src 1 (128 | cu_count): block b runs on XCD b % 8, dispatch round b / 8: the 16 members of a cluster are the
    // blocks of one XCD in 16 consecutive rounds
    items.resize(rows.size());
    for (int b = 0; b < (int)rows.size(); ++b) {
        const int xcd = b % 8, round = b / 8;
        const int q = (round / 16) * 8 + xcd, k = round % 16;
        items[(size_t)b] = rows[(size_t)q * 16 + k];
    }
    return given;
}

// The residue-class paths, batch by batch: every (segment, batch) overlap gets its share of ~one block per CU
struct LagFold {
    long long batch, seg, c_lo, c_n;  // the segment's columns inside the batch
    int first, count;                 // its rows of the blocks' partial spectra
};
struct LagResidueItems {
    std::vector<LagItem> items;   // c_lo / c_hi relative to the batch's first column; row: within the batch
    std::vector<LagFold> folds;   // in batch order
    std::vector<int> batch_off;   // [n_batches + 1] into items
    int max_items = 0;            // rows of partial spectra a batch writes at most
    long long max_tiles = 1;      // tiles of 64 x TSQ_TILES columns a fold's transposition has at most
};
inline LagResidueItems lag_residue_items(const LagPlan &pl, const LagDevice &dev, long long E, long long G, const int64_t *group_off)
{
    LagResidueItems r;
    const long long cols = 3 * E;
    r.batch_off.assign((size_t)pl.n_batches + 1, 0);
    for (long long b = 0; b < pl.n_batches; ++b) {
        const long long c_first = b * pl.nb0, nb = std::min(pl.nb0, cols - c_first);
        // (CUs the transform kernel of batch b runs on: it is given one workgroup per CU)
        const long long cus = pl.overlap && b + 1 < pl.n_batches ? dev.part_cus0 : dev.cu_count;
        r.batch_off[(size_t)b] = (int)r.items.size();
        int row = 0;
        lag_segments(E, G, group_off, c_first, nb, [&](long long s, long long lo, long long hi) {
            if (lo >= hi) return;
            const long long n = hi - lo;
            long long k = (n * cus + nb / 2) / nb;
            k = std::max<long long>(1, std::min(k, n));
            r.folds.push_back({b, s, lo, n, row, (int)k});
            r.max_tiles = std::max(r.max_tiles, (n + 64 * TSQ_TILES - 1) / (64 * TSQ_TILES));
            for (long long q = 0; q < k; ++q) r.items.push_back({lo - c_first + n * q / k, lo - c_first + n * (q + 1) / k, 1, row++});
        });
        r.max_items = std::max(r.max_items, row);
    }
    r.batch_off[(size_t)pl.n_batches] = (int)r.items.size();
    return r;
}

}  // namespace lagplan
