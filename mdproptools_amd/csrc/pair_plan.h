// pair_plan.h — what one batch of the pair-histogram path will run, decided from the problem's shape alone.
//
// pair_plan() is pure host arithmetic on sizes, box lengths, the context's options and two device limits (cu_count,
// lds_max): it makes no device call and touches no workspace, so the same function answers mdhip_pair_plan on a
// machine without a GPU. pair_hist.hip (the only includer; this header shares its compile flags, contraction off —
// the band floats below feed the exactness argument of the packed sweep) stages, launches and collects
// from the plan.
#pragma once
#include "pair_common.h"

namespace mdpair {

struct PairProblem {
    int64_t n_frames;
    int64_t ni, nj;
    const double *d_xi, *d_xj;  // device
    const int *d_ti, *d_tj;     // device compact type index
    int64_t ti_fs, tj_fs;
    const double *d_box;        // device [F][3]
    const double *h_box;        // host   [F][3]
    bool tri;
    int n_ti, n_tj;
    std::vector<int> cls;  // [n_ti][n_tj] -> class id (< n_cls; any number of classes: the device sees pass-local bytes)
    int n_cls;
    // displaced ordered rows (displace_rows, pair_hist.hip): row of (ti, tj) = disp_a[ti] + disp_b[tj]; disp_rows == 0: none found
    std::vector<int> disp_a, disp_b, disp_cls;  // disp_cls[row] -> class id (-1: no type pair lands there)
    int disp_rows = 0;
    int nbins;
    const double *edges;  // host [nbins+1]
    double rc2;
    float gscale;
    double bin_size;  // RDF: the reference's bin_size (0 for CN edge tables)
    int per_frame;
    // frame-summed RDF outputs kept on the device (mdhip_rdf_atomic_dev): full | part | overflow, accumulated by
    // derive_rdf_kernel straight from the row sums when the batch runs as one scalar-j pass; otherwise the batch
    // comes back as host class histograms like every other call and the caller adds them in
    unsigned long long *dev_out = nullptr;
    int n_rel = 0;
    const int *rel_cls = nullptr;   // host [n_rel]
    const int *rel_mult = nullptr;  // host [n_rel]
    // coordination numbers from the same sweep (mdhip_rdf_cn_atomic): one cutoff^2 per class (0: none). The bins of
    // the histogram are exact, so only the pairs of the bin that holds a class's cutoff (its split bin) need the exact
    // comparison: Hsplit counts those that are inside. Only the packed-f32 sweep does this — a batch that cannot run
    // it returns CN_UNFUSED and the caller runs a separate CN job
    int n_cn = 0;                             // != 0: on
    const double *cn_c2_cls = nullptr;        // host [n_cls]
    std::vector<uint64_t> *Hsplit = nullptr;  // out: [F|1][n_cls] pairs of the split bin with rsq < cutoff^2
    // Host-resident coordinates staged batch by batch (pair_hist_run): h_xi / h_xj are the caller's arrays, d_xi / d_xj
    // the (still empty) device buffers for all frames; the copy of batch k+1 runs on ctx->copy_stream while batch k is
    // swept. nullptr: the coordinates are on the device already.
    const double *h_xi = nullptr, *h_xj = nullptr;
};
constexpr int CN_UNFUSED = 1;  // (positive: not an error code of the ABI)
constexpr int SPLIT_BATCH = 2;  // a block may have wrapped a 32-bit LDS word: run the batch again in halves

struct PairPlan {
    int nTi = 0, nTj = 0;  // tiles per frame of either set
    // which kernel
    bool mode_cn = false;  // CN edge table: a few sorted cutoffs^2, bins found by counting
    bool fast = false;     // table-free binning with an exact guard band (else: the edge-table kernel)
    bool cull = false;     // spatial pre-pass
    bool sj = false;       // scalar-j sweep; sj_mode as sj_kernel's (pair_common.h), -1 for the LDS-tile kernels
    bool persist = false;  // ... on a resident grid with per-XCD work counters
    int sj_mode = -1;
    bool ordered = false, displaced = false, big = false;  // ordered rows: plain | displaced, one 16-wave block per CU
    bool pk = false, pk_rows = false, cut_guard = false;   // packed-f32 sweep: with class rows, cutoff inside a bin
    int cls_per_pass = 0, n_pass = 0;
    int ord_rows = 0, ord_maxb = 0;
    const std::vector<int> *row_cls = nullptr;  // ordered row -> class (the problem's disp_cls or cls)
    // the error bands the kernels' exactness rests on
    float near_ord = 0.f, near_pk_f = 0.f, s_cap = 0.f, rc2hi = 0.f, cut_lo = 0.f;
    int rel_block = 0;  // != 0: the packed sweep's f32 records are wanted (relative to their tile's centre)
    // geometry (the scalar-j grid is sized at the launch, from the kernel's occupancy)
    int jsplit = 1, blocks_per_frame = 0, fpb = 1, slots = 1;
    long long grid = 0;
    unsigned guard_tiles = 0;
    // the packed table buffer: edges | class table per pass | CN tables | displaced A, B | (16-aligned) row map
    bool one_sum = false;    // one scalar-j pass, frame-summed: the row sums sit behind the flag words
    bool map_rides = false;  // ... and the row map of derive_rdf_kernel rides behind the tables
    int sj_rows1 = 0, cn_rows = 0;
    size_t edges_b = 0, cls_b = 0, cn_off = 0, cn_fw = 0, disp_off = 0, disp_b = 0, tab_al = 0, map_b = 0, rows1_b = 0;
    // the launch
    PairKernel kern = nullptr;
    const char *kname = "";
    int bs = 0;               // threads per block
    std::vector<size_t> lds;  // histogram bytes of every pass (the scalar-j launch adds its guard word)

    int pass_c0(int pass) const { return pass * cls_per_pass; }
    int pass_nc(int pass, int n_cls) const { return std::min(n_cls - pass_c0(pass), cls_per_pass); }
};

// Fills `pl` for one batch of frames. -> MDHIP_OK, MDHIP_ELIMIT (error text set), or CN_UNFUSED when coordination
// numbers were asked for and the batch does not run as one packed sweep.
inline int pair_plan(mdhip_ctx *ctx, const PairProblem &p, PairPlan &pl)
{
    const int64_t F = p.n_frames;
    const int nTi = pl.nTi = (int)((p.ni + TILE - 1) / TILE);
    const int nTj = pl.nTj = (int)((p.nj + TILE - 1) / TILE);

    // kernel variant: 0 = reference-shaped loops with an edge-table lookup per pair (always used for CN
    // edge tables, gscale == 0); 1 = fast kernel (table-free binning with an exact guard band)
    const bool mode_cn = pl.mode_cn = !(p.gscale > 0.f);
    // The table-free bin guess of the fast kernels indexes a row of nbins + 1 words: that is enough exactly when
    // nbins = int(r_cut / bin_size) as the reference computes it (rdf_cn.py:169); a caller that passes fewer bins
    // gets the edge-table kernel, which clamps.
    const bool bins_ok = mode_cn || !(p.bin_size > 0.0) || std::sqrt(p.rc2) / p.bin_size < (double)p.nbins + 1.0 - 1e-9;
    const bool fast = pl.fast = ctx->opt_rdf_variant == 1 && bins_ok && (mode_cn ? p.nbins <= 64 : p.nbins <= 100000);

    // share of tile pairs within reach of each other (first frame's box): decides the culling and the slices per list
    double est;
    {
        const double V = p.h_box[0] * p.h_box[1] * p.h_box[2];
        const double edge = 0.5 * (std::cbrt((double)TILE * V / (double)p.ni) +
                                   std::cbrt((double)TILE * V / (double)p.nj));
        const double reach = std::sqrt(p.rc2) + 0.8 * edge;
        est = 4.18879 * reach * reach * reach / V;
    }
    // spatial culling: worth it when the cutoff sphere is a small part of the box (atoms x sites: scalar-j
    // kernel only)
    bool &cull = pl.cull;
    if (fast && nTi >= 8 && nTi <= 65535 && nTj <= 65535 && ctx->opt_rdf_cull != 0 &&
        (p.tri || (ctx->opt_rdf_sj != 0 && nTj >= 2)))
        cull = ctx->opt_rdf_cull == 1 || est < 1.5;  // measured: still +5 % at est = 1.08 (BASELINE C2)
    const bool sj = pl.sj = cull && ctx->opt_rdf_sj != 0;  // wave-independent sweep with scalar loads of the j atoms
    pl.persist = sj && !p.per_frame && ctx->opt_rdf_sj != 2;

    // classes per pass limited by LDS (keep >= 2 blocks per CU when possible)
    const size_t lds_cap = ctx->lds_max > 0 ? ctx->lds_max : 65536;
    const size_t fixed = fast ? lds_bytes_fast(p.nbins, 0, p.n_ti, p.n_tj) : lds_bytes(p.nbins, 0, p.n_ti, p.n_tj);
    const size_t row_b = fast ? (size_t)(p.nbins + 1) * 4 : (size_t)p.nbins * 4;
    if (fixed + row_b > lds_cap)
        return mdhip_fail(ctx, MDHIP_ELIMIT, "pair_hist: %d bins do not fit LDS (%zu B)", p.nbins,
                          lds_cap);
    const size_t budget = lds_cap / 2 > fixed + row_b ? lds_cap / 2 : lds_cap;
    int &cls_per_pass = pl.cls_per_pass = (int)((budget - fixed) / row_b);
    if (cls_per_pass > p.n_cls) cls_per_pass = p.n_cls;
    if (cls_per_pass > 250) cls_per_pass = 250;

    // Ordered-pair rows (MODE 2 / 3 of the scalar-j kernel): one LDS row per (ti, tj) addressed without a table —
    // the row offset rides in the addend of the bin guess. Needs all n_ti^2 rows in LDS and all classes in one pass:
    // at >= 4 blocks of 4 waves per CU for the all-f64 sweep, at 3 blocks of 8 waves (6 waves per SIMD) for the
    // packed-f32 sweep, whose blocks share one histogram among 8 waves.
    // Row layout of the ordered modes: plain (row = ti * n_tj + tj) unless that does not fit the packed sweep's third of
    // LDS and the displaced layout of displace_rows (row = A[ti] + B[tj], classes never mixed in a row) does.
    // (class rows of the packed sweep: as many classes per pass as fit a third of LDS)
    int pk_cls_fit = 0;
    for (int nc = std::min(p.n_cls, 250); nc >= 1; --nc)
        if (lds_bytes_sj_pk_rows(p.nbins, nc, p.n_ti, p.n_tj, p.n_cn) <= lds_cap / 3 - 512) {
            pk_cls_fit = nc;
            break;
        }
    int &ord_rows = pl.ord_rows = p.n_ti * p.n_tj, &ord_maxb = pl.ord_maxb = p.n_tj - 1;
    bool &displaced = pl.displaced, &big = pl.big;
    {
        const size_t third = lds_cap / 3 - 512, whole = lds_cap - 1024;
        const bool have_disp = p.disp_rows > 0 && p.disp_rows < ord_rows && ctx->opt_rdf_disp != 0;
        auto use_disp = [&]() {
            displaced = true;
            ord_rows = p.disp_rows;
            ord_maxb = *std::max_element(p.disp_b.begin(), p.disp_b.end());
        };
        if (lds_bytes_sj_pk(p.nbins, ord_rows, p.n_cn) <= third) {
            if (have_disp && ctx->opt_rdf_disp == 2) use_disp();  // (A/B: whenever it has fewer rows)
        } else if (have_disp && lds_bytes_sj_pk(p.nbins, p.disp_rows, p.n_cn) <= third) {
            use_disp();
        } else if (p.n_cn == 0 && ctx->opt_rdf_big != 0 && lds_cap >= 160 * 1024 && pk_cls_fit < p.n_cls) {
            // neither fits a third of LDS, and the class rows would need several passes (all classes in ONE pass of class rows
            // measured faster than this: 3.12 against 3.37 ms at C1's shape): ONE 16-wave block per CU with the whole LDS for
            // its histogram (BIG, pair_sj.hip) — every pair of nine types named is 81 rows, 130 KB — on whichever layout has
            // fewer rows
            const int rows_small = have_disp ? p.disp_rows : ord_rows;
            if (lds_bytes_sj_pk(p.nbins, rows_small, 0, true) <= whole) {
                big = true;
                if (have_disp) use_disp();
            }
        }
    }
    pl.row_cls = displaced ? &p.disp_cls : &p.cls;
    const size_t ord_b = lds_bytes_sj_ordered(p.nbins, ord_rows);
    const bool ord_base = sj && !mode_cn && ctx->opt_rdf_rows != 0 &&
                          p.n_cls <= 250 && (double)(ord_maxb + 1) * (p.nbins + 1) < 65536.0;
    bool &ordered = pl.ordered = ord_base && ord_b <= lds_cap / 4;
    // Packed-f32 classification (MODE 3-6 of the scalar-j kernel, header in pair_sj.hip) when the error band is
    // narrow: with the ordered rows when they fit a third of LDS (3 blocks of 8 waves per CU), else with class rows
    // and their row table (any number of types). The cutoff on a bin edge lets the band of that edge decide in/out
    // of the cutoff; a cutoff inside the last bin has its own band tested per pair (cut_guard).
    bool &pk = pl.pk, &pk_rows = pl.pk_rows, &cut_guard = pl.cut_guard;
    float &s_cap = pl.s_cap, &rc2hi = pl.rc2hi, &near_pk_f = pl.near_pk_f, &cut_lo = pl.cut_lo, &near_ord = pl.near_ord;
    int &rel_block = pl.rel_block;
    if (sj && !mode_cn && p.n_cls <= 250 && ctx->opt_rdf_pk != 0 && p.bin_size > 0.0) {
        const bool fits_ordered = ord_base && (big || lds_bytes_sj_pk(p.nbins, ord_rows, p.n_cn) <= lds_cap / 3 - 512);
        // class rows: as many classes per pass as fit a third of LDS. Round 6: when they do not all fit (every pair of nine
        // types named: 45 classes x 401 words = 72 KB) the packed sweep runs in SEVERAL passes over the pairs instead of
        // leaving the call to the all-f64 class-row kernel — C1's atoms with all 45 relations: 14.5 -> 6.3 ms per 200 frames
        // (`bench.py --shape C1full`); coordination numbers from the same sweep need one pass (else: two sweeps, as before)
        // (at least 8 classes per pass: with rows so long that fewer fit, the f64 kernel's half-of-LDS passes are as few)
        const bool fits_rows = pk_cls_fit >= p.n_cls || (pk_cls_fit >= 8 && p.n_cn == 0 && ctx->opt_rdf_pk_passes != 0);
        const double r_cut = std::sqrt(p.rc2);
        const double cpos = r_cut / p.bin_size, K = std::floor(cpos + 0.5);
        double l_max = 0.0, v_max = 0.0;
        for (int64_t f = 0; f < F; ++f) {
            const double *b = p.h_box + 3 * f;
            l_max = std::max(l_max, std::max(b[0], std::max(b[1], b[2])));
            v_max = std::max(v_max, b[0] * b[1] * b[2]);
        }
        // tile edge of the sparser of the two sets (atoms x sites: the sites)
        const double edge = std::cbrt((double)TILE * v_max / (double)std::min(p.ni, p.nj));
        const double cap = r_cut + 3.5 * edge;
        // (the guess carries tj * row_len with ordered rows, nothing with class rows)
        const double err = pk_error_bound(r_cut, p.bin_size, p.nbins, fits_ordered ? ord_maxb + 1 : 1, cap, l_max);
        const double u = std::ldexp(1.0, -24);
        const double near_pk = 2.0 * err + 4.5 * u * (p.nbins + 1) + 2.0e-5;
        const bool on_edge = std::fabs(cpos - K) <= 1e-6 && (K == (double)p.nbins || K == (double)p.nbins + 1.0);
        if ((fits_ordered || fits_rows) && (on_edge || std::floor(cpos) == (double)p.nbins) && near_pk <= 0.02 &&
            std::isfinite(l_max)) {
            pk = true;
            pk_rows = !fits_ordered;
            ordered = fits_ordered;
            cut_guard = !on_edge;
            // sqrt(rsq32) < cut_lo  =>  sqrt(rsq) < cut_lo + err * bin_size < r_cut: inside the cutoff for certain
            cut_lo = std::nextafterf((float)(r_cut - 1.1 * err * p.bin_size), 0.f);
            // the f32 records are relative to the centre of their whole tile (64-atom blocks bought a little f32
            // precision for 4x the per-block work: measured slower in round 2, retired in round 4)
            rel_block = TILE;
            near_pk_f = (float)near_pk;
            s_cap = (float)cap;
            // every pair with rsq < r_cut^2 has sqrt(rsq32) <= r_cut + err * bin_size
            const double r_hi = r_cut + err * p.bin_size;
            rc2hi = std::nextafterf((float)(r_hi * r_hi * (1.0 + 2.0 * u)), std::numeric_limits<float>::infinity());
            if (pk_rows) {  // all classes in one pass when they fit, else balanced passes of at most pk_cls_fit classes
                const int np = (p.n_cls + pk_cls_fit - 1) / pk_cls_fit;
                cls_per_pass = (p.n_cls + np - 1) / np;
            }
        }
    }
    big = big && pk && ordered && ctx->opt_rdf_pk != 2;  // (only the packed ordered sweep has the 16-wave instance)
    if (p.n_cn > 0 && (!pk || ctx->opt_rdf_pk == 2)) return CN_UNFUSED;
    if (ordered) {
        cls_per_pass = p.n_cls;
        // |error| of the f32 guess g = fma(sqrt((float)rsq), 1/ddr, near + tj*row_len): relative 2^-25 (conversion,
        // halved by the root) + 2^-23 (v_sqrt_f32, 1 ulp) + 2^-24 (rounded 1/ddr) = 2.1e-7 of the bin number, plus
        // half an ulp of the largest value each for the rounding of the addend and of the fma. near = 2 x that.
        const double maxg = (double)(ord_maxb + 1) * (p.nbins + 1) + 1.0;  // the addend carries B[tj] * row_len only
        const double ulp = std::ldexp(1.0, (int)std::floor(std::log2(maxg)) - 23);
        near_ord = (float)(2.0 * ((double)p.nbins * 2.1e-7 + ulp) + 1.0e-5);
        near_ord = std::max(near_ord, near_pk_f);  // one band for the f32 guess of either sweep
    }
    const int n_pass = pl.n_pass = (p.n_cls + cls_per_pass - 1) / cls_per_pass;

    // geometry
    int max_list = p.tri ? tri_shifts(nTi, 0) : nTj;
    int &jsplit = pl.jsplit = ctx->opt_rdf_jsplit;
    if (jsplit <= 0) {
        const int64_t want = (int64_t)ctx->cu_count * 48;  // ~12 blocks per CU slot: short tail
        const int64_t base = (int64_t)nTi * F;
        jsplit = (int)((want + base - 1) / base);
    }
    if (jsplit > max_list) jsplit = max_list;
    if (cull && jsplit > 4) jsplit = 4;
    // scalar-j kernels: items are (frame, tile, wave, slice); 4 slices measured best at C2 and C3, for the persistent
    // grid and for per-frame output alike (with one slice a 100k-atom frame has only two items per resident wave)
    if (sj && ctx->opt_rdf_jsplit <= 0) {
        // ... when the lists are long. A short reach (coordination cutoffs: a handful of neighbour tiles per tile) leaves
        // a slice one tile or none, and every item pays its set-up (counter, boxes, context) for it: round 4 measured
        // 4.72 -> 2.93 ms per 64 C3 frames for CN alone with ONE slice (tools/ab_pair.py rdf_jsplit=4,2,1 C3 cn).
        // Expected list length: the share of tile pairs within reach (as for the culling decision above) x tiles / 2.
        const double share = std::min(1.0, est);
        const double list_est = share * (double)nTj * (p.tri ? 0.5 : 1.0);
        jsplit = std::min(list_est >= 12.0 ? 4 : list_est >= 6.0 ? 2 : 1, max_list);
    }
    if (jsplit < 1) jsplit = 1;
    const int blocks_per_frame = pl.blocks_per_frame = nTi * jsplit;
    // frames per block (fast kernel, frame-summed output): as many as keeps >= `want` blocks in flight
    int &fpb = pl.fpb = 1;
    if (fast && !p.per_frame) {
        fpb = ctx->opt_rdf_fpb;
        if (fpb <= 0) {
            const int64_t want = (int64_t)ctx->cu_count * 24;
            fpb = (int)(((int64_t)blocks_per_frame * F) / want);
        }
        if (fpb < 1) fpb = 1;
        if (fpb > 64) fpb = 64;
    }
    const int64_t fgroups = (F + 8LL * fpb - 1) / (8LL * fpb);
    const int64_t grid = pl.grid = fgroups * 8 * blocks_per_frame;
    if (grid > 0x7fffffffLL)
        return mdhip_fail(ctx, MDHIP_ELIMIT, "pair_hist: grid of %lld blocks is too large",
                          (long long)grid);
    pl.slots = p.per_frame ? 1 : ctx->opt_rdf_slots;
    // one neighbour tile adds at most 64 x 256 to any one word of a block: 2^32 / 2^14 tiles, with margin
    pl.guard_tiles = ctx->opt_rdf_guard > 0 ? (unsigned)ctx->opt_rdf_guard : 250000u;

    // device tables
    pl.edges_b = (size_t)(p.nbins + 2) * 8;  // + a +inf sentinel after the last edge
    // CN tables of the scalar-j rows (one pass, all rows): word index of every row's split bin | cutoff^2 per row
    pl.cn_rows = p.n_cn ? (ordered ? ord_rows : p.n_cls + 1) : 0;
    pl.cn_fw = ((size_t)pl.cn_rows + 1) & ~size_t(1);
    const size_t cn_b = p.n_cn ? (pl.cn_fw + 2 * (size_t)pl.cn_rows) * 4 : 0;
    pl.cls_b = ((size_t)p.n_ti * p.n_tj + 63) & ~size_t(63);
    // edges and the class table of every pass: one pinned staging buffer, one H2D copy
    // (displaced rows: A | B as ints behind the CN tables, for pack_w of the sort pre-pass)
    pl.cn_off = pl.edges_b + (size_t)n_pass * pl.cls_b;
    pl.disp_off = (pl.cn_off + cn_b + 7) & ~size_t(7);
    pl.disp_b = ordered && displaced ? ((size_t)p.n_ti + p.n_tj) * 4 : 0;
    const size_t tab_b = pl.disp_off + pl.disp_b + 8;
    // The common case of the scalar-j sweep — one class pass, frame-summed rows — needs two more small things that a
    // C2 step paid a copy / a fill of their own for (round 5: ~12 us each with the gaps around them): the row map of
    // derive_rdf_kernel (results left on the device) rides behind the tables in the same copy, and the row sums sit
    // behind the flag words so that ONE fill empties both.
    pl.one_sum = sj && n_pass == 1 && !p.per_frame;
    pl.sj_rows1 = ordered ? ord_rows : p.n_cls + 1;
    pl.rows1_b = pl.one_sum ? (size_t)pl.sj_rows1 * (size_t)(p.nbins + 1 + (p.n_cn ? 1 : 0)) * 8 : 0;
    pl.map_rides = pl.one_sum && p.dev_out != nullptr;
    pl.tab_al = (tab_b + 15) & ~size_t(15);
    pl.map_b = pl.map_rides ? ((size_t)pl.sj_rows1 + 2 * (size_t)p.n_rel) * 4 : 0;

    // the launch: one kernel instance for every pass, its histogram bytes by the classes of the pass
    pl.sj_mode = !sj ? -1 : pk && ctx->opt_rdf_pk != 2 ? (pk_rows ? 5 : 3) + (cut_guard ? 1 : 0) : ordered ? 2 : mode_cn ? 1 : 0;
    const bool big_launch = big && pl.sj_mode >= 3 && pl.sj_mode <= 4;
    pl.bs = sj ? sj_block_threads(pl.sj_mode, big_launch) : TILE;
    pl.kern = sj ? sj_kernel(pl.sj_mode, pl.persist, p.n_cn > 0, big_launch, &pl.kname)
                 : dense_kernel(fast, p.tri, mode_cn, fast && cull, &pl.kname);
    pl.lds.resize(n_pass);
    for (int pass = 0; pass < n_pass; ++pass) {
        const int nc = pl.pass_nc(pass, p.n_cls);
        pl.lds[pass] = pk_rows ? lds_bytes_sj_pk_rows(p.nbins, nc, p.n_ti, p.n_tj, p.n_cn)
                       : pk    ? lds_bytes_sj_pk(p.nbins, ord_rows, p.n_cn, big)
                       : ordered ? ord_b
                       : sj    ? lds_bytes_sj(p.nbins, nc, p.n_ti, p.n_tj, mode_cn)
                       : fast ? lds_bytes_fast(p.nbins, nc, p.n_ti, p.n_tj)
                              : lds_bytes(p.nbins, nc, p.n_ti, p.n_tj);
    }
    return MDHIP_OK;
}

}  // namespace mdpair
