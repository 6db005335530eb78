// pair_hist.hip — all-pairs minimum-image distance histogramming for gfx950 (R1-R5).
//
// Replaces structural/rdf_cn.py:35-162 of the reference (_calc_rsq, _remove_outliers, _rdf_loop,
// _cn_loop, _rdf_mol_loop, _cn_mol_loop). One kernel family serves all four loops:
//
//   H[class(type_i, type_j)][bin(rsq)] += 1      for every in-cutoff pair, exactly once
//
// where `bin` is a comparison of rsq against a host-made table of exact edges and `class` is a small
// table lookup. The reference's outputs are integer-linear in H (see derive_* below), so the kernel
// never sees the relation list. RDF uses the edges of trunc(sqrt(rsq)/ddr); CN uses the sorted
// distinct cutoffs^2 as edges.
//
// Bit-exactness: rsq is built from exactly-rounded IEEE double ops in the reference's order,
// with contraction off for this whole translation unit:
//   d = head - other; if |d| > L/2: d -= sign(d)*L; rsq = (dx*dx + dy*dy) + dz*dz
// The wrap is evaluated as  a = |d|;  a' = min(a, |a - L|)  which selects the same double:
//   |d - sign(d)L| == | |d| - L |  (rounding is sign-symmetric), and for a > L/2 the real value
//   |a - L| < a while for a <= L/2 it is >= a; rounding to nearest is monotone and `a` is itself a
//   double, so the comparison of the rounded value against `a` falls the same way (ties give equal
//   values). Only a^2 enters rsq, so the lost sign is irrelevant.
//
// Kernels live in their own translation units (shared types: pair_common.h):
//   pair_sj.hip     scalar-j kernel — the default of the spatially culled sweep (one i atom per lane, j atoms
//                   through scalar loads, wrap decisions hoisted per (wave box, group box), persistent grid)
//   pair_cull.hip   the spatial pre-pass: Hilbert sort, bounding boxes, neighbour-tile lists
//   pair_dense.hip  LDS-tile kernels: dense half-shell sweep for small frames, the edge-table kernel of the
//                   first commit (A/B baseline, fallback for > 64 CN cutoffs)
// This file: relations -> classes (classify), batching (batch_parts, run_parts), one batch as plan -> stage_tables ->
// cull_prepass -> launch_pass -> collect_* (pair_hist_run_batch; the plan itself — kernel variant, row layout, error
// bands, launch geometry, table offsets — is pair_plan.h: pure arithmetic, no device), rows -> outputs, the C-ABI.
#include <map>
#include <mutex>
#include <optional>

#include "pair_plan.h"

using namespace mdpair;

namespace {

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

// Row displacement for the ordered-pair rows. The table-free sweep adds to word A[ti] + B[tj] + bin — the lane holds
// A[ti] rows as its base, the j atom's record carries B[tj] rows in the addend of the bin guess — and the plain layout
// A = ti * n_tj, B = tj needs n_ti * n_tj rows: 36 rows x 401 words for the reference's own example (9 atom types, five
// relations naming five of them -> 6 type indices), which does not fit the third of LDS a block may use, and sent
// that shape to the class-row kernels (a row-table lookup per pair: 1.47x per pair). But rows only
// have to be distinct where CLASSES are: two ordered type pairs may share a row whenever they belong to the same class
// (their counts are added up at the flush anyway) — above all the many pairs that no relation names. So: find
// integers A, B with  A[i] + B[j] == A[k] + B[l]  =>  cls(i, j) == cls(k, l),  minimising max A + max B + 1. Greedy,
// type by type (A[k] and B[k] together, smallest resulting row count first), over a few orders; 15 rows instead of 36
// for the example above. The kernels are unchanged: they see A and B through the records (pack_w) and row_mul.
// Cached per class table (the search costs ~1 ms, at most DISPLACE_BUDGET candidates plus one attempt; a drop-in run
// repeats the same relations for every batch).
struct DispKey {
    int n_ti, n_tj;
    std::vector<int> cls;
    bool operator<(const DispKey &o) const
    {
        if (n_ti != o.n_ti) return n_ti < o.n_ti;
        if (n_tj != o.n_tj) return n_tj < o.n_tj;
        return cls < o.cls;
    }
};
struct DispVal {
    std::vector<int> a, b, row_cls;
    int rows = 0;
};

static int displace_greedy(int n_ti, int n_tj, const std::vector<int> &cls, const std::vector<int> &order, int give_up,
                           std::vector<int> &A, std::vector<int> &B, std::vector<int> &row_cls, uint64_t &trials)
{
    const int n = std::max(n_ti, n_tj);
    A.assign(n_ti, -1);
    B.assign(n_tj, -1);
    row_cls.assign((size_t)2 * give_up + 2, -1);
    std::vector<int> done;  // type indices placed so far
    int max_a = 0, max_b = 0;
    std::vector<int> touched;
    for (int step = 0; step < n; ++step) {
        const int k = order[step];
        const bool has_a = k < n_ti, has_b = k < n_tj;
        int best_r = 1 << 30, best_s = 0, best_a = -1, best_b = -1;
        const int lim = give_up;
        for (int ai = 0; ai < (has_a ? lim : 1); ++ai) {
            for (int bi = 0; bi < (has_b ? lim : 1); ++bi) {
                const int ma = has_a ? std::max(max_a, ai) : max_a, mb = has_b ? std::max(max_b, bi) : max_b;
                const int r = ma + mb + 1, sc = ai + bi;
                ++trials;
                if (r >= give_up) break;  // (bi only grows)
                if (r > best_r || (r == best_r && sc >= best_s)) continue;
                // consistent with every row written so far, and with itself?
                bool ok = true;
                touched.clear();
                auto put = [&](int row, int c) {
                    if (row_cls[row] >= 0) {
                        if (row_cls[row] != c) ok = false;
                    } else {
                        row_cls[row] = c;
                        touched.push_back(row);
                    }
                };
                if (has_a && has_b) put(ai + bi, cls[(size_t)k * n_tj + k]);
                for (size_t q = 0; q < done.size() && ok; ++q) {
                    const int u = done[q];
                    if (has_a && u < n_tj) put(ai + B[u], cls[(size_t)k * n_tj + u]);
                    if (ok && has_b && u < n_ti) put(A[u] + bi, cls[(size_t)u * n_tj + k]);
                }
                for (int row : touched) row_cls[row] = -1;
                if (!ok) continue;
                best_r = r;
                best_s = sc;
                best_a = ai;
                best_b = bi;
            }
        }
        if (best_r >= give_up) return 0;
        if (has_a) {
            A[k] = best_a;
            max_a = std::max(max_a, best_a);
        }
        if (has_b) {
            B[k] = best_b;
            max_b = std::max(max_b, best_b);
        }
        if (has_a && has_b) row_cls[best_a + best_b] = cls[(size_t)k * n_tj + k];
        for (int u : done) {
            if (has_a && u < n_tj) row_cls[best_a + B[u]] = cls[(size_t)k * n_tj + u];
            if (has_b && u < n_ti) row_cls[A[u] + best_b] = cls[(size_t)u * n_tj + k];
        }
        done.push_back(k);
    }
    const int rows = max_a + max_b + 1;
    row_cls.resize(rows);
    return rows;
}

constexpr uint64_t DISPLACE_BUDGET = 2500000;  // (ai, bi) candidates per table, checked between attempts
// -> rows of the best displaced layout found (0: none with fewer rows than the plain layout, or too many types to try)
static int displace_rows(int n_ti, int n_tj, const std::vector<int> &cls, std::vector<int> &A, std::vector<int> &B,
                         std::vector<int> &row_cls)
{
    static std::mutex mu;
    static std::map<DispKey, DispVal> cache;
    const int plain = n_ti * n_tj;
    if (plain <= 4 || n_ti > 24 || n_tj > 24) return 0;
    DispKey key{n_ti, n_tj, cls};
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = cache.find(key);
        if (it != cache.end()) {
            A = it->second.a;
            B = it->second.b;
            row_cls = it->second.row_cls;
            return it->second.rows;
        }
    }
    const int n = std::max(n_ti, n_tj);
    DispVal best;
    std::vector<int> order(n), a, b, rc;
    for (int k = 0; k < n; ++k) order[k] = k;
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    uint64_t trials = 0;  // (ai, bi) candidates looked at so far, over all attempts
    for (int attempt = 0; attempt < 400; ++attempt) {
        if (attempt == 1) std::reverse(order.begin(), order.end());
        if (attempt >= 2)
            for (int k = n - 1; k > 0; --k) {  // a fixed pseudo-random shuffle: the same layout on every rank and run
                lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
                std::swap(order[k], order[(size_t)((lcg >> 33) % (uint64_t)(k + 1))]);
            }
        const int give_up = best.rows ? best.rows : plain;  // only strictly better layouts
        const int rows = displace_greedy(n_ti, n_tj, cls, order, give_up, a, b, rc, trials);
        if (rows > 0 && (best.rows == 0 || rows < best.rows)) {
            best.rows = rows;
            best.a = a;
            best.b = b;
            best.row_cls = rc;
        }
        if (trials > DISPLACE_BUDGET) break;  // a fixed amount of work, not of time: the layout never depends on the machine's load
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        if (cache.size() > 256) cache.clear();
        cache[key] = best;
    }
    A = best.a;
    B = best.b;
    row_cls = best.row_cls;
    return best.rows;
}

// what the host half of a batch's passes accumulates (shared with the completion step of a deferred batch)
struct BatchAcc {
    double total_ms = 0.0, prep_ms = 0.0;
    int launches = 0;
    unsigned long long ov = 0;
    bool prep_timed = false;
    KernelTimer prep;
    explicit BatchAcc(const KernelTimer &t) : prep(t) {}
};

// One batch between plan and results: the staged tables, the flag words, and where the results go.
struct Batch {
    const PairProblem &p;
    const PairPlan &pl;
    std::vector<uint64_t> &H;
    size_t out_frames;
    unsigned char *d_tab = nullptr, *h_tab = nullptr;  // the packed table buffer (PairPlan's offsets), device | pinned
    unsigned long long *d_misc = nullptr;              // flag words [8] | row sums (one_sum)
    std::shared_ptr<BatchAcc> acc;
};

// One launched pass: its classes [c0, c0 + nc), its rows on the device, its timer.
struct Pass {
    int pass, c0, nc;
    int sj_rows, cn_len, sj_words;       // scalar-j: rows of the block histograms, split counters per row, words
    size_t words;                        // dense: words of the pass's class histograms
    unsigned long long *d_rows = nullptr, *d_hist = nullptr;
    std::optional<KernelTimer> timer;
};

// Writes the plan's packed table buffer — edges | class table of every pass | CN tables | displaced A, B | row map —
// into pinned memory and sends it to the device in ONE small copy. -> the displaced-row tables as the sort pre-pass
// wants them, and the reach of the split bins.
static int stage_tables(mdhip_ctx *ctx, Batch &b, RowDisp &disp_i, RowDisp &disp_j, float &cn_reach)
{
    const PairProblem &p = b.p;
    const PairPlan &pl = b.pl;
    const std::vector<int> &row_cls = *pl.row_cls;
    MD_WS(d_tab, unsigned char, WS_TABLES, pl.tab_al + pl.map_b);
    MD_PIN(h_tab, unsigned char, pl.tab_al + pl.map_b + 32);
    double *e = reinterpret_cast<double *>(h_tab);
    std::copy(p.edges, p.edges + p.nbins + 1, e);
    e[p.nbins + 1] = std::numeric_limits<double>::infinity();
    if (p.n_cn) {
        int *fl = reinterpret_cast<int *>(h_tab + pl.cn_off);
        double *c2r = reinterpret_cast<double *>(fl + pl.cn_fw);
        std::fill(fl, fl + pl.cn_fw, -1);
        double reach = 0.0;
        for (int r = 0; r < pl.cn_rows; ++r) {
            const int cl = pl.ordered ? row_cls[r] : (r < p.n_cls ? r : -1);
            const double c2 = cl >= 0 ? p.cn_c2_cls[cl] : 0.0;
            c2r[r] = c2;
            if (!(c2 > 0.0)) continue;
            // split bin kc: edges[kc] <= c2 < edges[kc + 1]; none when the cutoff sits exactly on an edge
            const int kc = (int)(std::upper_bound(p.edges, p.edges + p.nbins + 1, c2) - p.edges) - 1;
            if (p.edges[kc] == c2) continue;
            fl[r] = r * (p.nbins + 1) + kc;
            const double top = kc + 1 <= p.nbins ? std::sqrt(p.edges[kc + 1]) : std::sqrt(p.rc2);
            reach = std::max(reach, std::min(top, std::sqrt(p.rc2)));
        }
        cn_reach = (float)((reach + 1e-3) * 1.00001);
    }
    for (int pass = 0; pass < pl.n_pass; ++pass) {
        const int c0 = pl.pass_c0(pass), nc = pl.pass_nc(pass, p.n_cls);
        unsigned char *t = h_tab + pl.edges_b + (size_t)pass * pl.cls_b;
        for (size_t k = 0; k < (size_t)p.n_ti * p.n_tj; ++k) {
            const int c = p.cls[k];  // (pass-local ids are < 250: they fit the byte, 0xFF = other pass)
            t[k] = (c >= c0 && c < c0 + nc) ? (unsigned char)(c - c0) : 0xFF;
        }
    }
    if (pl.disp_b) {
        int *h_d = reinterpret_cast<int *>(h_tab + pl.disp_off);
        std::copy(p.disp_a.begin(), p.disp_a.end(), h_d);
        std::copy(p.disp_b.begin(), p.disp_b.end(), h_d + p.n_ti);
        const int *d_d = reinterpret_cast<const int *>(d_tab + pl.disp_off);
        // atom-atom: one sorted set plays both roles (low word A, addend B); atoms x sites: the i set's addend and the j
        // set's low word are never read
        disp_i.lo = d_d;
        disp_i.hi = p.tri ? d_d + p.n_ti : d_d;
        disp_j.lo = disp_j.hi = d_d + p.n_ti;
    }
    if (pl.map_rides) {
        int *h_map = reinterpret_cast<int *>(h_tab + pl.tab_al);
        for (int r = 0; r < pl.sj_rows1; ++r) h_map[r] = pl.ordered ? row_cls[r] : (r < p.n_cls ? r : -1);
        for (int kl = 0; kl < p.n_rel; ++kl) {
            h_map[pl.sj_rows1 + kl] = p.rel_cls[kl];
            h_map[pl.sj_rows1 + p.n_rel + kl] = p.rel_mult[kl];
        }
    }
    b.d_tab = d_tab;
    b.h_tab = h_tab;
    return mdhip_copy_small(ctx, d_tab, h_tab, pl.tab_al + pl.map_b, hipMemcpyHostToDevice);
}

// The culled path's pre-pass — Hilbert sort, tile boxes, neighbour-tile lists; once, shared by all class passes —
// under a timer of its own. Points `a` at the sorted copies.
static int cull_prepass(mdhip_ctx *ctx, Batch &b, const RowDisp &disp_i, const RowDisp &disp_j, PairArgs &a)
{
    const PairProblem &p = b.p;
    const PairPlan &pl = b.pl;
    const int64_t F = p.n_frames;
    const int nTi = pl.nTi, nTj = pl.nTj;
    const long long N = p.ni;
    const bool want_soa = !pl.sj;  // only the LDS-tile kernel (atom-atom) reads the SoA copy
    MD_WS(d_l, unsigned short, WS_LIST, (size_t)F * nTi * (p.tri ? nTi : nTj) * 2);
    MD_WS(d_lc, int, WS_LISTCNT, (size_t)F * nTi * 4);
    KernelTimer ptimer(ctx, 1, true);  // second event pair: collected with the pair kernel's
    SortedSet si, sj_set;
    const int slot_i[5] = {WS_SORT_AOS, WS_BBOX, WS_GSPH, WS_WSPH, WS_GSPH4};
    // (the bin-guess addend near + type * row_len and the tile-relative f32 records belong to the j set)
    const float near = pl.ordered ? pl.near_ord : 0.f;
    const int row_len = pl.ordered ? p.nbins + 1 : 0;
    int rc = cull_prepare_set(ctx, F, p.d_xi, p.d_ti, (long long)p.ti_fs, p.d_box, N, nTi, p.n_ti, near, row_len, disp_i,
                              want_soa, pl.pk && p.tri ? pl.rel_block : 0, pl.pk_rows ? 1 : 0, pl.pk ? 1 : 0, slot_i, si);
    if (rc) return rc;
    if (p.tri) {
        sj_set = si;
    } else {
        const int slot_j[5] = {WS_SORT_AOS_J, WS_BBOX_J, WS_GSPH_J, WS_WSPH_J, WS_GSPH4_J};
        rc = cull_prepare_set(ctx, F, p.d_xj, p.d_tj, (long long)p.tj_fs, p.d_box, p.nj, nTj, p.n_ti, near, row_len, disp_j,
                              false, pl.pk ? pl.rel_block : 0, pl.pk_rows ? 1 : 0, pl.pk ? 1 : 0, slot_j, sj_set);
        if (rc) return rc;
    }
    launch_cull_lists(ctx->stream, p.tri, F, si.bbox, sj_set.bbox, nTi, nTj, p.d_box, p.rc2 * (1.0 + 1e-9) + 1e-9, d_l,
                      d_lc);
    ptimer.stop();
    MD_HIP(hipGetLastError());
    b.acc = std::make_shared<BatchAcc>(ptimer);
    b.acc->prep_timed = true;
    a.gsph = sj_set.gs;    // 8-atom boxes of the j set (LDS-tile kernel)
    a.gsph4 = sj_set.gs4;  // 4-atom boxes of the j set (scalar-j kernel)
    a.wsph = si.ws;        // 64-atom boxes of the i set
    if (want_soa) {
        a.xi = a.xj = si.sx;
        a.ti = a.tj = si.st;
        a.ti_fs = a.tj_fs = N;
    }
    a.list = d_l;
    a.list_cnt = d_lc;
    a.aos = si.aos;
    a.aos_j = sj_set.aos;
    a.rel = sj_set.rel;
    a.cen = sj_set.cen;
    return MDHIP_OK;
}

// Everything of the kernel's arguments that is the same for every pass (the inputs as the caller gave them:
// cull_prepass redirects them to the sorted copies).
static PairArgs batch_args(const Batch &b, float cn_reach)
{
    const PairProblem &p = b.p;
    const PairPlan &pl = b.pl;
    PairArgs a{};
    a.xi = p.d_xi;
    a.xj = p.d_xj;
    a.ti = p.d_ti;
    a.tj = p.d_tj;
    a.ti_fs = p.ti_fs;
    a.tj_fs = p.tj_fs;
    a.reach = (float)((std::sqrt(p.rc2) + 1e-3) * 1.00001);
    a.tri = p.tri ? 1 : 0;
    a.box = p.d_box;
    a.edges = reinterpret_cast<const double *>(b.d_tab);
    a.overflow = b.d_misc;
    a.ni = p.ni;
    a.nj = p.nj;
    a.rc2 = p.rc2;
    a.gscale = p.gscale;
    a.n_ti = p.n_ti;
    a.n_tj = p.n_tj;
    a.row_mul = pl.ordered && pl.displaced ? 1 : p.n_tj;
    a.n_rows_ord = pl.ord_rows;
    a.nbins = p.nbins;
    a.n_frames = (int)p.n_frames;
    a.nTi = pl.nTi;
    a.nTj = pl.nTj;
    a.jsplit = pl.jsplit;
    a.blocks_per_frame = pl.blocks_per_frame;
    a.per_frame = p.per_frame;
    a.slots = pl.slots;
    a.fpb = pl.fpb;
    a.near = pl.pk_rows ? pl.near_pk_f : pl.near_ord;
    a.s_cap = pl.s_cap;
    a.rc2hi = pl.rc2hi;
    a.cut_lo = pl.cut_lo;
    a.n_cn = p.n_cn;
    a.cn_tab = reinterpret_cast<const unsigned *>(b.d_tab + pl.cn_off);
    a.cn_reach = cn_reach;
    a.work = reinterpret_cast<unsigned *>(b.d_misc + 4);
    return a;
}

// Launches one class pass (and, for the scalar-j kernels, the merge of the blocks' histogram slices) under ps.timer.
// The scalar-j grid is sized here: it needs the kernel's occupancy on this device.
static int launch_pass(mdhip_ctx *ctx, const Batch &b, PairArgs a, Pass &ps)
{
    const PairProblem &p = b.p;
    const PairPlan &pl = b.pl;
    const int64_t F = p.n_frames;
    const bool sj = pl.sj;
    const size_t acc_frames = p.per_frame ? (size_t)F : (size_t)pl.slots;
    MD_WS(d_hist, unsigned long long, WS_HIST, (acc_frames + 1) * ps.words * 8);
    // (the scalar-j kernels keep their histograms in LDS and store them to their own slices: nothing of theirs is
    // added to d_hist, so it need not be emptied for them — one fill less per call)
    if (!sj) MD_HIP(hipMemsetAsync(d_hist, 0, acc_frames * ps.words * 8, ctx->stream));
    ps.d_hist = d_hist;
    a.cls = b.d_tab + pl.edges_b + (size_t)ps.pass * pl.cls_b;
    a.hist = d_hist;
    a.n_cls = ps.nc;
    const size_t lds = pl.lds[ps.pass];
    if (sj) {
        a.guard_off = (unsigned)((lds + 15) & ~size_t(15));
        a.guard_tiles = pl.guard_tiles;
    }
    const size_t lds_launch = sj ? ((lds + 15) & ~size_t(15)) + 16 : lds;
    const int bs = pl.bs, wpb = bs / 64;  // independent waves per block (scalar-j kernels)
    ctx->last_kernel = pl.kname;
    if (lds_launch > 65536)
        MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pl.kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_launch));
    long long launch_grid = pl.grid;
    if (sj) {
        int per_cu = 0;
        MD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(pl.kern), bs,
                                                            lds_launch));
        if (per_cu < 1) per_cu = 1;
        const long long capacity = (long long)per_cu * ctx->cu_count;
        // blocks' worth of wave items per frame (a frame has nTi * 4 * jsplit wave items)
        const long long block_items = ((long long)pl.nTi * 4 * pl.jsplit + wpb - 1) / wpb;
        a.fpb = 1;
        if (pl.persist) {
            // (beside another call: room for the pre-pass of the call after this one, see LANE_FREE_BLOCKS)
            const long long room = mdhip_beside_another(ctx) && capacity >= 8LL * LANE_FREE_BLOCKS ? LANE_FREE_BLOCKS : 0;
            launch_grid = std::min(capacity - room, F * block_items + 8);
            launch_grid = (launch_grid + 7) / 8 * 8;
            // (the work counters: the first pass finds them empty, d_misc was zeroed whole at the top of the batch)
            if (ps.pass > 0) MD_HIP(hipMemsetAsync(b.d_misc + 4, 0, 32, ctx->stream));
        } else {
            // per-frame output: as many blocks per frame as keeps one resident set busy, each flushing once
            // blocks per frame: few frames in flight per XCD (their records should stay in its 4 MB L2: 32 B per
            // atom per frame), every wave still left with a few items to draw
            const long long cap_xcd = std::max<long long>(1, capacity / 8);
            const long long frames_xcd = (F + 7) / 8;
            const long long in_flight = std::max<long long>(1, std::min<long long>(frames_xcd, ctx->opt_rdf_inflight));
            long long bpf = std::max<long long>(1, cap_xcd / in_flight);
            bpf = std::min(bpf, std::max<long long>(1, block_items / 2));
            // every block stores one copy of its LDS histogram: keep that workspace within ~2 GiB
            while (bpf > 8 && (double)(((F + 7) / 8) * 8 * bpf) * (double)lds > 2147483648.0) bpf /= 2;
            a.blocks_per_frame = (int)bpf;
            launch_grid = ((F + 7) / 8) * 8 * bpf;
            MD_WS(d_work, unsigned, WS_WORK, (size_t)F * 4);
            MD_HIP(hipMemsetAsync(d_work, 0, (size_t)F * 4, ctx->stream));
            a.work = d_work;
        }
        // every block stores its LDS histogram into its own slice; a merge kernel adds them up
        MD_WS(d_sl, unsigned, WS_SLICES, (size_t)launch_grid * ps.sj_words * 4);
        if (pl.one_sum && pl.rows1_b == (size_t)ps.sj_words * 8) {
            ps.d_rows = b.d_misc + 8;  // (emptied with the flag words at the top of the batch)
        } else {
            ps.d_rows = (unsigned long long *)mdhip_ws(ctx, WS_ROWS, b.out_frames * (size_t)ps.sj_words * 8);
            if (!ps.d_rows) return MDHIP_ENOMEM;
            if (!p.per_frame) MD_HIP(hipMemsetAsync(ps.d_rows, 0, (size_t)ps.sj_words * 8, ctx->stream));
        }
        a.slices = d_sl;
    }
    ps.timer.emplace(ctx);
    hipLaunchKernelGGL(pl.kern, dim3((unsigned)launch_grid), dim3(bs), lds_launch, ctx->stream, a);
    if (sj) {
        const unsigned gy = p.per_frame ? (unsigned)F : (unsigned)std::min<long long>(64, launch_grid);
        launch_merge_slices(ctx->stream, a.slices, ps.sj_words, launch_grid, p.per_frame, a.blocks_per_frame, gy, ps.d_rows);
    }
    ps.timer->stop();
    MD_HIP(hipGetLastError());
    return MDHIP_OK;
}

// the launch's flags (pinned): [0] deferred pairs lost, [1] work-loop assertion, [2] overflow guard
static int check_flags(mdhip_ctx *ctx, const uint64_t *hlost)
{
    if (hlost[2]) return SPLIT_BATCH;
    if (hlost[0] || hlost[1])
        return mdhip_fail(ctx, MDHIP_EHIP, "pair_hist: internal check failed (%llu deferred pairs lost, work loop %llu)",
                          (unsigned long long)hlost[0], (unsigned long long)hlost[1]);
    return MDHIP_OK;
}

static void collect_times(BatchAcc &acc, const KernelTimer &timer)
{
    acc.total_ms += timer.collect();
    ++acc.launches;
    if (acc.prep_timed) {  // the pre-pass ran ahead of the first pass on the same stream: its events are complete
        acc.prep_ms = acc.prep.collect();
        acc.prep_timed = false;
    }
}

// Collector 1 — results stay on the device: rows -> full | part | overflow by derive_rdf_kernel (added to dev_out; the
// row map came with the tables: map_rides); only the flag words come back. -> the pass's host half in `fin`.
static int collect_device(mdhip_ctx *ctx, const Batch &b, const Pass &ps, std::function<int()> &fin)
{
    const PairProblem &p = b.p;
    const PairPlan &pl = b.pl;
    if (!pl.map_rides || ps.sj_rows != pl.sj_rows1)
        return mdhip_fail(ctx, MDHIP_EHIP, "pair_hist: internal: the row map of the device-resident path is missing");
    const int *d_map = reinterpret_cast<const int *>(b.d_tab + pl.tab_al);
    launch_derive_rdf(ctx->stream, ps.d_rows, ps.sj_rows, p.nbins, d_map, p.n_rel, d_map + ps.sj_rows,
                      d_map + ps.sj_rows + p.n_rel, b.d_misc + 3, p.dev_out);
    MD_HIP(hipGetLastError());
    uint64_t *hlost = reinterpret_cast<uint64_t *>(b.h_tab + pl.tab_al + ((pl.map_b + 7) & ~size_t(7)));
    const int rcc = mdhip_copy_small(ctx, hlost, b.d_misc + 1, 24, hipMemcpyDeviceToHost);
    if (rcc) return rcc;
    fin = [ctx, acc = b.acc, timer = *ps.timer, hlost]() {
        const int rcf = check_flags(ctx, hlost);
        if (rcf) return rcf;
        collect_times(*acc, timer);
        return (int)MDHIP_OK;
    };
    return MDHIP_OK;
}

// Collector 2 — scalar-j rows: D2H of the row sums (pinned staging), then rows -> classes, the split counters and the
// overflow words on the host. -> the pass's host half in `fin`.
static int collect_sj_rows(mdhip_ctx *ctx, const Batch &b, const Pass &ps, std::function<int()> &fin)
{
    const PairProblem &p = b.p;
    const PairPlan &pl = b.pl;
    const size_t out_frames = b.out_frames, sj_words = (size_t)ps.sj_words;
    MD_PIN(hall, uint64_t, (out_frames * sj_words + 16) * 8);
    uint64_t *hrows = hall + 8;
    uint64_t *hlost = hrows + out_frames * sj_words;  // [0] queue overflow, [1] work-loop assertion
    if (ps.d_rows == b.d_misc + 8 && out_frames == 1) {
        // the row sums sit behind the flag words (one_sum): flags and rows leave in ONE copy
        hlost = hall + 1;
        const int rcc = mdhip_copy_small(ctx, hall, b.d_misc, (8 + sj_words) * 8, hipMemcpyDeviceToHost);
        if (rcc) return rcc;
    } else {
        int rcc = mdhip_copy_small(ctx, hrows, ps.d_rows, out_frames * sj_words * 8, hipMemcpyDeviceToHost);
        if (!rcc) rcc = mdhip_copy_small(ctx, hlost, b.d_misc + 1, 24, hipMemcpyDeviceToHost);
        if (rcc) return rcc;
    }
    std::vector<uint64_t> *Hp = &b.H, *Hsplit = p.Hsplit;
    fin = [ctx, acc = b.acc, timer = *ps.timer, hrows, hlost, Hp, Hsplit, out_frames, sj_words, sj_rows = ps.sj_rows,
           cn_len = ps.cn_len, ordered = pl.ordered, nc = ps.nc, c0 = ps.c0, n_cls_all = p.n_cls, nbins_all = p.nbins,
           cls = pl.ordered ? *pl.row_cls : std::vector<int>()]() {
        const int rcf = check_flags(ctx, hlost);
        if (rcf) return rcf;
        collect_times(*acc, timer);
        const int row_len = nbins_all + 1;
        for (size_t fr = 0; fr < out_frames && cn_len; ++fr)
            for (int r = 0; r < sj_rows; ++r) {
                const uint64_t *src = hrows + fr * sj_words + (size_t)sj_rows * row_len + (size_t)r;
                const int cl = ordered ? cls[r] : (r < nc ? c0 + r : -1);
                if (cl >= 0) (*Hsplit)[fr * n_cls_all + cl] += src[0];
            }
        for (size_t fr = 0; fr < out_frames; ++fr)
            for (int r = 0; r < sj_rows; ++r) {
                const uint64_t *src = hrows + fr * sj_words + (size_t)r * row_len;
                acc->ov += src[nbins_all];
                // ordered rows (ti, tj) -> class of the unordered pair; class rows of this pass -> c0 + r, the
                // extra row holds the pairs whose class belongs to another pass
                const int cl = ordered ? (int)cls[r] : (r < nc ? c0 + r : -1);
                if (cl < 0) continue;
                uint64_t *dst = &(*Hp)[(fr * n_cls_all + cl) * nbins_all];
                for (int k = 0; k < nbins_all; ++k) dst[k] += src[k];
            }
        return (int)MDHIP_OK;
    };
    return MDHIP_OK;
}

// Collector 3 — dense slots (LDS-tile and edge-table kernels): reduce the replicas, D2H (pinned staging) into the right
// class rows behind a stream sync; the overflow word rides along with the last pass.
static int collect_dense(mdhip_ctx *ctx, Batch &b, const Pass &ps)
{
    const PairProblem &p = b.p;
    const PairPlan &pl = b.pl;
    const size_t out_frames = b.out_frames, words = ps.words;
    const bool last = ps.pass == pl.n_pass - 1;
    unsigned long long *d_final = ps.d_hist;
    if (!p.per_frame && pl.slots > 1) {
        d_final = ps.d_hist + (size_t)pl.slots * words;
        launch_reduce_slots(ctx->stream, ps.d_hist, d_final, (int)words, pl.slots);
        MD_HIP(hipGetLastError());
    }
    MD_PIN(tmp, uint64_t, (out_frames * words + 1) * 8);
    MD_HIP(hipMemcpyAsync(tmp, d_final, out_frames * words * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (last) MD_HIP(hipMemcpyAsync(tmp + out_frames * words, b.d_misc, 8, hipMemcpyDeviceToHost, ctx->stream));
    MD_HIP(mdhip_stream_wait(ctx));
    if (last) b.acc->ov = tmp[out_frames * words];  // (d_misc[0] accumulates over the passes)
    collect_times(*b.acc, *ps.timer);
    for (size_t fr = 0; fr < out_frames; ++fr)
        memcpy(&b.H[(fr * p.n_cls + ps.c0) * p.nbins], &tmp[fr * words], words * 8);
    return MDHIP_OK;
}

// Runs the kernel over one batch of frames (in several passes when the class rows do not fit LDS) and
// returns the class histograms on the host: H [F|1][n_cls][nbins], overflow count. The sequence: pair_plan ->
// stage_tables -> cull_prepass -> per pass: launch_pass, one of the three collectors.
// `defer` (an asynchronous call's scope, or nullptr): when the batch runs as ONE scalar-j pass, its host half — flag
// check, timer read-out, folding the row sums into H — is left as a completion step of that call instead of being done
// behind a stream sync here; H, *overflow, p.Hsplit and *redo must then outlive the call (they are parts of the entry
// point's heap state). A launch that raised the overflow guard sets *redo there (nothing else is touched) instead of
// returning SPLIT_BATCH. Everything else (class passes, the dense kernels) completes inside, as before.
int pair_hist_run_batch(mdhip_ctx *ctx, const PairProblem &p, std::vector<uint64_t> &H, uint64_t *overflow,
                        CallScope *defer = nullptr, bool *redo = nullptr)
{
    const size_t out_frames = p.per_frame ? (size_t)p.n_frames : 1;
    H.assign(out_frames * p.n_cls * p.nbins, 0);
    if (p.Hsplit) p.Hsplit->assign(out_frames * p.n_cls, 0);
    *overflow = 0;
    if (p.n_frames == 0 || p.ni == 0 || p.nj == 0) return MDHIP_OK;

    PairPlan pl;
    int rc = pair_plan(ctx, p, pl);
    if (rc) return rc;
    Batch b{p, pl, H, out_frames};
    RowDisp disp_i, disp_j;
    float cn_reach = 0.f;
    rc = stage_tables(ctx, b, disp_i, disp_j, cn_reach);
    if (rc) return rc;
    MD_WS(d_misc, unsigned long long, WS_MISC, 64 + pl.rows1_b);
    MD_HIP(hipMemsetAsync(d_misc, 0, 64 + pl.rows1_b, ctx->stream));
    b.d_misc = d_misc;
    PairArgs args = batch_args(b, cn_reach);
    if (pl.cull) {
        rc = cull_prepass(ctx, b, disp_i, disp_j, args);
        if (rc) return rc;
    }
    // (total_ms: the pair kernel alone; the culling pre-pass is reported separately)
    if (!b.acc) b.acc = std::make_shared<BatchAcc>(KernelTimer(ctx, 1, true));
    // the end of the batch: what the passes found goes to the caller and to the context's registers
    auto finalize = [ctx, acc = b.acc, overflow, n_pass = pl.n_pass]() {
        // with several passes every in-cutoff overflow pair is seen once per pass
        *overflow = acc->ov / (uint64_t)n_pass;
        ctx->last_ms = acc->total_ms;
        ctx->last_launches = acc->launches;
        ctx->last_aux_ms = acc->prep_ms;
        return MDHIP_OK;
    };
    for (int pass = 0; pass < pl.n_pass; ++pass) {
        const int nc = pl.pass_nc(pass, p.n_cls);
        const int sj_rows = pl.ordered ? pl.ord_rows : nc + 1;
        const int cn_len = p.n_cn ? 1 : 0;  // one split counter per row, behind all histogram rows
        Pass ps{pass, pl.pass_c0(pass), nc, sj_rows, cn_len, sj_rows * (p.nbins + 1 + cn_len), (size_t)nc * p.nbins};
        rc = launch_pass(ctx, b, args, ps);
        if (rc) return rc;
        if (!pl.sj) {
            rc = collect_dense(ctx, b, ps);
            if (rc) return rc;
            continue;
        }
        std::function<int()> fin;
        rc = p.dev_out && pl.one_sum ? collect_device(ctx, b, ps, fin) : collect_sj_rows(ctx, b, ps, fin);
        if (rc) return rc;
        // the pass's host half: a completion step of an asynchronous call's one pass, else behind a stream sync now
        if (defer != nullptr && pl.n_pass == 1) {
            defer->defer([fin, finalize, redo]() {
                const int rcf = fin();
                if (rcf == SPLIT_BATCH) {
                    *redo = true;
                    return (int)MDHIP_OK;
                }
                return rcf ? rcf : finalize();
            });
            return MDHIP_OK;
        }
        MD_HIP(mdhip_stream_wait(ctx));
        rc = fin();
        if (rc) return rc;
    }
    return finalize();
}

// Copies the frames [f0, f0 + n) of the host-resident inputs of `p` to their device buffers on the copy stream and
// records `ev` behind them.
static int stage_batch_async(mdhip_ctx *ctx, const PairProblem &p, int64_t f0, int64_t n, hipEvent_t ev)
{
    // (pageable sources through the context's page-locked ring: mdhip_h2d_any — the halves alternate with the batches)
    const int half = ev == ctx->copy_ev[1] ? 1 : 0;
    if (p.h_xi) {
        const int rc = mdhip_h2d_any(ctx, const_cast<double *>(p.d_xi) + (size_t)f0 * 3 * p.ni, p.h_xi + (size_t)f0 * 3 * p.ni,
                                     (size_t)n * 3 * p.ni * 8, ctx->copy_stream, half);
        if (rc) return rc;
    }
    if (p.h_xj) {
        const int rc = mdhip_h2d_any(ctx, const_cast<double *>(p.d_xj) + (size_t)f0 * 3 * p.nj, p.h_xj + (size_t)f0 * 3 * p.nj,
                                     (size_t)n * 3 * p.nj * 8, ctx->copy_stream, half);
        if (rc) return rc;
    }
    MD_HIP(hipEventRecord(ev, ctx->copy_stream));
    return MDHIP_OK;
}

// The batches [f0, f0 + n) of F frames: the culled path's workspace (sorted copy, keys, cell counts, boxes,
// neighbour-tile lists) stays within ~2 GiB and a launch's grid.y within 65535. `staged` (host-resident coordinates):
// a shorter first batch lets the sweep start early. Pure arithmetic (mdhip_pair_plan counts launches with it).
static std::vector<std::pair<int64_t, int64_t>> batch_parts(const mdhip_ctx *ctx, int64_t F, int64_t ni, bool staged)
{
    const int64_t nT = (ni + TILE - 1) / TILE;
    const double per_frame_b = 54.0 * (double)ni + 4.0 * MORTON_CELLS + 2.0 * (double)nT * (double)nT + 1024.0;
    int64_t batch = (int64_t)(2147483648.0 / per_frame_b);
    if (batch < 1) batch = 1;
    if (batch > 32768) batch = 32768;
    // whole rounds of the spatial sort, which runs one block per frame and CU (its cell counters fill the LDS): 367 C3
    // frames a batch sorted in two rounds of 1.1 ms where 256 take one
    if (batch > ctx->cu_count && ctx->cu_count > 0) batch = batch / ctx->cu_count * ctx->cu_count;
    if (ctx->opt_rdf_batch > 0) batch = ctx->opt_rdf_batch;
    std::vector<std::pair<int64_t, int64_t>> parts;
    int64_t f0 = 0;
    if (staged && F >= 32) {
        // first batch: a quarter of the frames (whole multiples of 8: frames are dealt to the 8 XCDs). Its sweep has
        // to last as long as the copy of the rest — the sweep consumes frames ~3.7x slower than PCIe delivers them
        // at C2 and at C3 size (61 against 230 frames per ms at 10k atoms) — or the second sweep waits for data
        // (a sixth measured 3.94 ms per C2 step with a 0.18 ms stall)
        int64_t b0 = std::max<int64_t>(8, (F / 4) / 8 * 8);
        b0 = std::min(b0, batch);
        parts.emplace_back(0, b0);
        f0 = b0;
    }
    for (; f0 < F; f0 += batch) parts.emplace_back(f0, std::min<int64_t>(batch, F - f0));
    return parts;
}

// Whether an asynchronous atom-atom call may be on the device BESIDE the pair call issued before it — on the other lane,
// with that lane's own set of everything the pre-pass writes, the sweep reads and the call returns (ctx.h). The rule
// (include/mdhip.h): its frames are ONE batch of batch_parts (staged = false: the deferred path of an asynchronous call
// stages host-resident frames whole), and two sets of what such a batch asks for fit the device. A call of several
// batches fills the ~2 GiB its batches are bounded by, completes batch by batch inside the entry point anyway, and a
// second set must not make its batches smaller: it runs alone on the context's stream, as every other call does — and
// so does a call beside whose set a second one finds no room. The need is batch_parts' own estimate plus the staging
// buffer of host-resident frames; the free memory is asked for only when a call is larger than any checked before.
static bool pair_overlap_ok(mdhip_ctx *ctx, int64_t F, int64_t n, int on_device)
{
    if (F < 1 || n < 2 || F >= (1LL << 31) || n >= (1LL << 31)) return false;
    if (batch_parts(ctx, F, n, false).size() != 1) return false;
    const int64_t nT = (n + TILE - 1) / TILE;
    const double need = (54.0 * (double)n + 4.0 * MORTON_CELLS + 2.0 * (double)nT * (double)nT + 1024.0) * (double)F +
                        (on_device ? 0.0 : 24.0 * (double)n * (double)F);
    if (need <= ctx->lane_fit_bytes) return true;
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if ((double)free_b < 2.5 * need) return false;  // (both sets may still have to grow to this size, with their slack)
    ctx->lane_fit_bytes = need;
    return true;
}

static int pair_hist_run_range(mdhip_ctx *ctx, const PairProblem &p, int64_t f0, int64_t n, std::vector<uint64_t> &H,
                               uint64_t *overflow, std::vector<uint64_t> *Hsplit, CallScope *defer = nullptr,
                               bool *redo = nullptr);

// Runs the parts [first, first + second) of the frames [f0, f0 + n) one after the other and merges them — the batches of
// a call, or the halves of a batch that raised the overflow guard: the parts' class histograms and split counts go into
// the whole's, per frame or added up, and the timing registers of the context add up. `before(k)` runs ahead of part k.
template <class Before>
static int run_parts(mdhip_ctx *ctx, const PairProblem &p, const std::vector<std::pair<int64_t, int64_t>> &parts, int64_t f0,
                     int64_t n, std::vector<uint64_t> &H, uint64_t *overflow, std::vector<uint64_t> *Hsplit, Before before)
{
    const size_t row = (size_t)p.n_cls * p.nbins, row_cn = (size_t)p.n_cls;
    H.assign((p.per_frame ? (size_t)n : 1) * row, 0);
    if (Hsplit) Hsplit->assign((p.per_frame ? (size_t)n : 1) * row_cn, 0);
    *overflow = 0;
    double ms = 0.0, aux = 0.0;
    int launches = 0;
    std::vector<uint64_t> part, part_cn;
    for (size_t k = 0; k < parts.size(); ++k) {
        int rc = before(k);
        if (rc) return rc;
        uint64_t ov = 0;
        rc = pair_hist_run_range(ctx, p, parts[k].first, parts[k].second, part, &ov, Hsplit ? &part_cn : nullptr);
        if (rc) return rc;
        *overflow += ov;
        ms += ctx->last_ms;
        aux += ctx->last_aux_ms;
        launches += ctx->last_launches;
        const size_t at = (size_t)(parts[k].first - f0);
        if (p.per_frame)
            std::copy(part.begin(), part.end(), H.begin() + at * row);
        else
            for (size_t q = 0; q < row; ++q) H[q] += part[q];
        if (Hsplit) {
            if (p.per_frame)
                std::copy(part_cn.begin(), part_cn.end(), Hsplit->begin() + at * row_cn);
            else
                for (size_t q = 0; q < row_cn; ++q) (*Hsplit)[q] += part_cn[q];
        }
    }
    ctx->last_ms = ms;
    ctx->last_aux_ms = aux;
    ctx->last_launches = launches;
    return MDHIP_OK;
}

// The frames [f0, f0 + n) of `p` (their coordinates are on the device): one batch, or — when a block's 32-bit histogram
// words might wrap — halves of it, recursively. Results as pair_hist_run_batch's.
static int pair_hist_run_range(mdhip_ctx *ctx, const PairProblem &p, int64_t f0, int64_t n, std::vector<uint64_t> &H,
                               uint64_t *overflow, std::vector<uint64_t> *Hsplit, CallScope *defer, bool *redo)
{
    PairProblem q = p;
    q.h_xi = q.h_xj = nullptr;
    q.Hsplit = Hsplit;
    q.n_frames = n;
    q.d_xi = p.d_xi + (size_t)f0 * 3 * p.ni;
    q.d_xj = p.d_xj + (size_t)f0 * 3 * p.nj;
    q.d_ti = p.d_ti + (size_t)f0 * p.ti_fs;
    q.d_tj = p.d_tj + (size_t)f0 * p.tj_fs;
    q.d_box = p.d_box + (size_t)f0 * 3;
    q.h_box = p.h_box + (size_t)f0 * 3;
    const int rc1 = pair_hist_run_batch(ctx, q, H, overflow, defer, redo);
    if (rc1 != SPLIT_BATCH) return rc1;
    if (n == 1)
        return mdhip_fail(ctx, MDHIP_ELIMIT, "pair_hist: one frame can overflow the 32-bit block histograms "
                                              "(%lld x %lld atoms)", (long long)p.ni, (long long)p.nj);
    // (device-resident sums, dev_out, are left untouched by a flagged launch)
    const int64_t half = (n + 1) / 2;
    return run_parts(ctx, p, {{f0, half}, {f0 + half, n - half}}, f0, n, H, overflow, Hsplit, [](size_t) { return 0; });
}

// Runs the batches of batch_parts and merges them.
// Host-resident coordinates (p.h_xi): the batches are also the unit of the host-to-device staging — the copy of batch
// k + 1 is issued on the copy stream before batch k is swept, so that it runs under that sweep (page-locked sources:
// a DMA the host does not wait for; pageable sources: the runtime stages them synchronously, so the copy simply comes
// first, as without this scheme).
// `defer` / `redo`: see pair_hist_run_batch — used when the frames are ONE batch whose coordinates are on the device.
int pair_hist_run(mdhip_ctx *ctx, const PairProblem &p, std::vector<uint64_t> &H, uint64_t *overflow,
                  CallScope *defer = nullptr, bool *redo = nullptr)
{
    const int64_t F = p.n_frames;
    const bool staged = p.h_xi || p.h_xj;
    const std::vector<std::pair<int64_t, int64_t>> parts = batch_parts(ctx, F, p.ni, staged);
    if (staged) {
        const int rc = stage_batch_async(ctx, p, parts[0].first, parts[0].second, ctx->copy_ev[0]);
        if (rc) return rc;
    }
    if (parts.size() == 1 && !staged) return pair_hist_run_range(ctx, p, 0, F, H, overflow, p.Hsplit, defer, redo);
    return run_parts(ctx, p, parts, 0, F, H, overflow, p.Hsplit, [&](size_t k) {
        if (!staged) return (int)MDHIP_OK;
        // this batch's frames must have landed before the launch stream touches them; the next batch's copy goes
        // out now, ahead of this batch's kernels
        MD_HIP(hipStreamWaitEvent(ctx->stream, ctx->copy_ev[k & 1], 0));
        if (k + 1 < parts.size())
            return stage_batch_async(ctx, p, parts[k + 1].first, parts[k + 1].second, ctx->copy_ev[(k + 1) & 1]);
        return (int)MDHIP_OK;
    });
}

// labels -> compact indices 0..T-1 (sorted unique labels)
void compact_labels(const int32_t *lab, size_t n, std::vector<int32_t> &uniq, std::vector<int32_t> &idx)
{
    idx.resize(n);
    uniq.clear();
    if (n == 0) return;
    int32_t lo = lab[0], hi = lab[0];
    for (size_t k = 1; k < n; ++k) {
        lo = lab[k] < lo ? lab[k] : lo;
        hi = lab[k] > hi ? lab[k] : hi;
    }
    const int64_t span = (int64_t)hi - (int64_t)lo + 1;
    if (span <= (1 << 20)) {  // the usual case (LAMMPS types 1..T): one presence table, O(n)
        std::vector<int32_t> slot((size_t)span, -1);
        for (size_t k = 0; k < n; ++k) slot[(size_t)(lab[k] - lo)] = 0;
        int32_t next = 0;
        for (int64_t v = 0; v < span; ++v)
            if (slot[(size_t)v] == 0) {
                slot[(size_t)v] = next++;
                uniq.push_back((int32_t)(lo + v));
            }
        for (size_t k = 0; k < n; ++k) idx[k] = slot[(size_t)(lab[k] - lo)];
        return;
    }
    uniq.assign(lab, lab + n);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    for (size_t k = 0; k < n; ++k)
        idx[k] = (int32_t)(std::lower_bound(uniq.begin(), uniq.end(), lab[k]) - uniq.begin());
}

int find_label(const std::vector<int32_t> &uniq, int32_t lab)
{
    auto it = std::lower_bound(uniq.begin(), uniq.end(), lab);
    return (it != uniq.end() && *it == lab) ? (int)(it - uniq.begin()) : -1;
}

// Only labels that some relation names need histogram rows of their own: every other label shares ONE index (its
// pairs all belong to the class "no relation asks for this"). Shrinks the type count the kernels see — e.g. a
// 9-type electrolyte with relations over 3 types runs with 4 — which is what decides whether the table-free
// ordered-row layout (and with it the packed-f32 sweep) fits LDS. `col` = the relation column that refers to this
// atom set (-1: both, the triangular case). uniq: sorted distinct labels (in) -> named labels (out); idx: remapped.
int merge_unnamed_labels(std::vector<int32_t> &uniq, std::vector<int32_t> &idx, int n_rel, const int32_t *rel, int col)
{
    std::vector<int32_t> named;
    std::vector<int32_t> rank(uniq.size(), -1);
    for (size_t k = 0; k < uniq.size(); ++k) {
        bool hit = false;
        for (int kl = 0; kl < n_rel && !hit; ++kl)
            hit = (col != 1 && rel[2 * kl] == uniq[k]) || (col != 0 && rel[2 * kl + 1] == uniq[k]);
        if (hit) {
            rank[k] = (int32_t)named.size();
            named.push_back(uniq[k]);
        }
    }
    const int32_t other = (int32_t)named.size();
    const bool has_other = named.size() < uniq.size();
    for (auto &v : idx) v = rank[(size_t)v] >= 0 ? rank[(size_t)v] : other;
    uniq.swap(named);
    return (int)uniq.size() + (has_other ? 1 : 0);
}

// Relations -> classes. Triangular: unordered type pairs {a,b}; rectangular: ordered (atom type,
// site type). rel_cls[kl] = class id, or -1 when a label does not occur in the data (the reference
// then counts nothing); the last class collects every pair no relation asks for.
// ui / uj hold the labels that have an index of their own (0 .. size-1); n_ti / n_tj may be one larger: the
// index shared by all labels no relation names (merge_unnamed_labels).
void build_classes(bool tri, const std::vector<int32_t> &ui, const std::vector<int32_t> &uj, int n_ti, int n_tj,
                   int n_rel, const int32_t *rel, std::vector<int> &cls, std::vector<int> &rel_cls,
                   int &n_cls)
{
    std::vector<int> map((size_t)n_ti * n_tj, -1);
    rel_cls.assign(n_rel, -1);
    int next = 0;
    for (int kl = 0; kl < n_rel; ++kl) {
        const int a = find_label(ui, rel[2 * kl]);
        const int b = find_label(uj, rel[2 * kl + 1]);
        if (a < 0 || b < 0) continue;
        int &slot = map[(size_t)a * n_tj + b];
        if (slot < 0) {
            slot = next++;
            if (tri) map[(size_t)b * n_tj + a] = slot;
        }
        rel_cls[kl] = slot;
    }
    n_cls = next + 1;
    cls.resize((size_t)n_ti * n_tj);
    for (size_t k = 0; k < cls.size(); ++k) cls[k] = map[k] < 0 ? next : map[k];
}

struct RelJob {
    bool tri;
    int64_t F, ni, nj;
    const double *xi, *xj;  // host|dev
    int xi_dev, xj_dev;
    const int32_t *lab_i;  // host labels [ni] or [F][ni]
    int64_t lab_i_fs;
    const int32_t *lab_j;  // host labels [nj] (rectangular only)
    const double *box;     // host [F][3]
    int n_rel;
    const int32_t *rel;
    int nbins;
    const double *edges;  // host [nbins+1]
    double rc2;
    float gscale;
    double bin_size;
    int per_frame;
    unsigned long long *dev_out = nullptr;  // see PairProblem::dev_out
    const double *cn_rc2 = nullptr;           // mdhip_rdf_cn_atomic: coordination cutoff^2 per relation, host [n_rel]
    std::vector<uint64_t> *Hsplit = nullptr;  // see PairProblem::Hsplit
    std::vector<double> *cn_c2_cls = nullptr; // out: the cutoff^2 of every class
};

// Labels -> compact type indices -> classes -> displaced rows: the part of a job that needs no device, shared by
// run_job and mdhip_pair_plan. Fills p.tri, n_ti, n_tj, cls, n_cls and the displaced layout; idx_i / idx_j are the
// compact type columns (lab_j: rectangular only).
static int classify(mdhip_ctx *ctx, bool tri, const int32_t *lab_i, size_t n_lab_i, const int32_t *lab_j, size_t n_lab_j,
                    int n_rel, const int32_t *rel, PairProblem &p, std::vector<int> &rel_cls, std::vector<int32_t> &idx_i,
                    std::vector<int32_t> &idx_j)
{
    std::vector<int32_t> ui, uj;
    compact_labels(lab_i, n_lab_i, ui, idx_i);
    if (!tri) compact_labels(lab_j, n_lab_j, uj, idx_j);
    const int n_ti = merge_unnamed_labels(ui, idx_i, n_rel, rel, tri ? -1 : 0);
    const int n_tj = tri ? n_ti : merge_unnamed_labels(uj, idx_j, n_rel, rel, 1);
    if ((size_t)n_ti * (size_t)n_tj > 16384)
        return mdhip_fail(ctx, MDHIP_ELIMIT, "too many distinct types named by relations (%d x %d)", n_ti, n_tj);
    p.tri = tri;
    build_classes(tri, ui, tri ? ui : uj, n_ti, n_tj, n_rel, rel, p.cls, rel_cls, p.n_cls);
    p.n_ti = n_ti;
    p.n_tj = n_tj;
    if (ctx->opt_rdf_disp != 0) p.disp_rows = displace_rows(n_ti, n_tj, p.cls, p.disp_a, p.disp_b, p.disp_cls);
    return MDHIP_OK;
}

// One coordination cutoff^2 per class (0: none) from one per relation; false: relations that name the same pair of
// types with different cutoffs (such a call takes two sweeps).
static bool class_cutoffs(int n_rel, const std::vector<int> &rel_cls, const double *cn_rc2, int n_cls, std::vector<double> &c2)
{
    c2.assign(n_cls, 0.0);
    std::vector<char> seen(n_cls, 0);
    for (int kl = 0; kl < n_rel; ++kl) {
        const int cl = rel_cls[kl];
        if (cl < 0) continue;
        const double v = cn_rc2[kl] > 0.0 ? cn_rc2[kl] : 0.0;
        if (seen[cl] && c2[cl] != v) return false;
        seen[cl] = 1;
        c2[cl] = v;
    }
    return true;
}

// Stages everything, runs the kernel and returns class histograms + the relation->class map.
// `defer` / `redo`: see pair_hist_run_batch (H, rel_cls, *overflow, j.Hsplit and *redo then live in the entry point's
// heap state; what a deferred step needs from this function's locals is copied into it).
int run_job(mdhip_ctx *ctx, const RelJob &j, std::vector<uint64_t> &H, std::vector<int> &rel_cls,
            int &n_cls, uint64_t *overflow, CallScope *defer = nullptr, bool *redo = nullptr)
{
    std::vector<int32_t> idx_i, idx_j;
    PairProblem p;
    int rc = classify(ctx, j.tri, j.lab_i, j.lab_i_fs ? (size_t)j.F * j.ni : (size_t)j.ni, j.lab_j, (size_t)j.nj, j.n_rel,
                      j.rel, p, rel_cls, idx_i, idx_j);
    if (rc) return rc;
    n_cls = p.n_cls;
    std::vector<int> rel_mult(j.n_rel, 1);
    if (j.dev_out) {
        for (int kl = 0; kl < j.n_rel; ++kl) rel_mult[kl] = (j.tri && j.rel[2 * kl] == j.rel[2 * kl + 1]) ? 2 : 1;
        p.dev_out = j.dev_out;
        p.n_rel = j.n_rel;
        p.rel_cls = rel_cls.data();
        p.rel_mult = rel_mult.data();
    }

    // Host-resident coordinates are staged batch by batch under the sweeps (pair_hist_run); the guard drains the copy
    // stream on every way out, so that no copy still reads the caller's arrays after this call has returned.
    struct CopyGuard {
        mdhip_ctx *c;
        bool on = true;
        ~CopyGuard()
        {
            if (on && c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
        }
    } copy_guard{ctx};
    const bool overlap = ctx->opt_h2d_overlap != 0 && (!j.xi_dev || (!j.tri && !j.xj_dev));
    if (overlap && !ctx->copy_stream) {
        MD_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        MD_HIP(hipEventCreateWithFlags(&ctx->copy_ev[0], hipEventDisableTiming));
        MD_HIP(hipEventCreateWithFlags(&ctx->copy_ev[1], hipEventDisableTiming));
        for (auto &lane_ev : ctx->stage_ev)
            for (auto &e : lane_ev) MD_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // An ASYNCHRONOUS atom-atom call on host-resident frames: the whole trajectory is copied on the copy stream into the
    // staging buffer the call before this one does not use — i.e. under that call's kernels — and the sweep then runs as
    // on resident frames (one batch, its host half deferred). Calls that alternate between the lanes are double-buffered
    // by that alone (each lane's set has a WS_XYZ_I); calls that stay on one lane alternate between its two buffers. A
    // buffer is written again behind the event of the last kernels that read it, on whichever lane they ran. The caller's
    // array is read until the call completes (the contract of the *_async entry points; a pageable source is staged by the
    // runtime before hipMemcpyAsync returns).
    int stage_buf = -1;
    if (ctx->completing > 0 && (!j.xi_dev || (!j.tri && !j.xj_dev)))
        MD_HIP(mdhip_stream_wait(ctx));  // a re-run from a completion step: the staging buffers may feed queued kernels
    if (overlap && !j.xi_dev && j.tri && defer != nullptr) {
        const int lane = ctx->lane;
        if (mdhip_top_call(ctx)->exclusive) {  // (a call made from a completion step is its own top: exclusive)
            stage_buf = ctx->stage_flip[lane];
            ctx->stage_flip[lane] ^= 1;
        } else {
            stage_buf = 0;
        }
        const size_t xb = (size_t)j.F * 3 * j.ni * 8;
        double *d_x = (double *)mdhip_ws(ctx, stage_buf ? WS_XYZ_I2 : WS_XYZ_I, xb);
        if (!d_x) return MDHIP_ENOMEM;
        if (ctx->stage_used[lane][stage_buf]) MD_HIP(hipStreamWaitEvent(ctx->copy_stream, ctx->stage_ev[lane][stage_buf], 0));
        {
            const int rch = mdhip_h2d_any(ctx, d_x, j.xi, xb, ctx->copy_stream, lane ^ stage_buf);
            if (rch) return rch;
        }
        MD_HIP(hipEventRecord(ctx->copy_ev[0], ctx->copy_stream));
        MD_HIP(hipStreamWaitEvent(ctx->stream, ctx->copy_ev[0], 0));
        p.d_xi = d_x;
        copy_guard.on = false;
    } else if (overlap && !j.xi_dev) {
        MD_WS(d_x, double, WS_XYZ_I, (size_t)j.F * 3 * j.ni * 8);
        // (a workspace buffer that was just re-allocated may still be read by nothing: mdhip_ws synchronised the stream)
        p.d_xi = d_x;
        p.h_xi = j.xi;
    } else {
        p.d_xi = (const double *)mdhip_stage(ctx, WS_XYZ_I, j.xi, (size_t)j.F * 3 * j.ni * 8, j.xi_dev, &rc);
        if (rc) return rc;
    }
    // compact types of both sets and the box lengths: one pinned staging buffer (owned by the context, so the
    // asynchronous copies need no sync before this function's vectors go away)
    const size_t ti_b = (idx_i.size() * 4 + 63) & ~size_t(63), tj_b = (idx_j.size() * 4 + 63) & ~size_t(63);
    const size_t box_b = (size_t)j.F * 3 * 8;
    MD_PIN(h_in, unsigned char, ti_b + tj_b + box_b);
    memcpy(h_in, idx_i.data(), idx_i.size() * 4);
    memcpy(h_in + ti_b, idx_j.data(), idx_j.size() * 4);
    memcpy(h_in + ti_b + tj_b, j.box, box_b);
    // ONE copy for the three tables (round 5: three copies cost a C2 step ~12 us each, the gaps between a copy and the
    // kernels around it included): types of set i | types of set j | box lengths, behind each other in one buffer
    MD_WS(d_in, unsigned char, WS_TYPE_I, ti_b + tj_b + box_b);
    {
        const int rcc = mdhip_copy_small(ctx, d_in, h_in, ti_b + tj_b + box_b, hipMemcpyHostToDevice);
        if (rcc) return rcc;
    }
    int *d_ti = reinterpret_cast<int *>(d_in);
    p.d_ti = d_ti;
    p.ti_fs = j.lab_i_fs;
    if (j.tri) {
        p.d_xj = p.d_xi;
        p.d_tj = p.d_ti;
        p.tj_fs = p.ti_fs;
        p.nj = j.ni;
    } else {
        if (overlap && !j.xj_dev) {
            MD_WS(d_xjw, double, WS_XYZ_J, (size_t)j.F * 3 * j.nj * 8);
            p.d_xj = d_xjw;
            p.h_xj = j.xj;
        } else {
            p.d_xj = (const double *)mdhip_stage(ctx, WS_XYZ_J, j.xj, (size_t)j.F * 3 * j.nj * 8, j.xj_dev, &rc);
            if (rc) return rc;
        }
        p.d_tj = reinterpret_cast<int *>(d_in + ti_b);
        p.tj_fs = 0;
        p.nj = j.nj;
    }
    p.d_box = reinterpret_cast<double *>(d_in + ti_b + tj_b);
    p.h_box = j.box;
    p.n_frames = j.F;
    p.ni = j.ni;
    p.nbins = j.nbins;
    p.edges = j.edges;
    p.rc2 = j.rc2;
    p.gscale = j.gscale;
    p.bin_size = j.bin_size;
    p.per_frame = j.per_frame;
    if (j.cn_rc2) {
        if (!class_cutoffs(j.n_rel, rel_cls, j.cn_rc2, n_cls, *j.cn_c2_cls)) return CN_UNFUSED;
        p.n_cn = 1;
        p.cn_c2_cls = j.cn_c2_cls->data();
        p.Hsplit = j.Hsplit;
    }
    rc = pair_hist_run(ctx, p, H, overflow, defer, redo);
    if (stage_buf >= 0 && (rc == MDHIP_OK || rc == CN_UNFUSED)) {
        MD_HIP(hipEventRecord(ctx->stage_ev[ctx->lane][stage_buf], ctx->stream));  // behind the last kernels that read the buffer
        ctx->stage_used[ctx->lane][stage_buf] = true;
    }
    return rc;
}

// CN: edges are the sorted distinct positive cutoffs^2; rank[kl] = number of bins below relation kl's cutoff.
void cn_edges(int n_rel, const double *rc2, std::vector<double> &edges, std::vector<int> &rank)
{
    std::vector<double> q;
    for (int kl = 0; kl < n_rel; ++kl)
        if (rc2[kl] > 0.0) q.push_back(rc2[kl]);
    std::sort(q.begin(), q.end());
    q.erase(std::unique(q.begin(), q.end()), q.end());
    edges.assign(1, 0.0);
    edges.insert(edges.end(), q.begin(), q.end());
    rank.assign(n_rel, 0);
    for (int kl = 0; kl < n_rel; ++kl)
        if (rc2[kl] > 0.0)
            rank[kl] = (int)(std::lower_bound(q.begin(), q.end(), rc2[kl]) - q.begin()) + 1;
}

int check_common(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const void *xyz, const void *type,
                 const void *box, int n_rel, const void *rel)
{
    if (!ctx) return MDHIP_EINVAL;
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0, "negative sizes");
    MD_REQUIRE(n_frames == 0 || n_atoms == 0 || (xyz && type && box), "NULL input array");
    MD_REQUIRE(n_rel >= 0 && (n_rel == 0 || rel), "bad relation table");
    MD_REQUIRE(n_frames < (1LL << 31) && n_atoms < (1LL << 31), "sizes exceed 2^31");
    return MDHIP_OK;
}

}  // namespace

extern "C" {

double mdhip_pk_error_bound(double r_cut, double bin_size, int nbins, int n_rows, double s_cap, double l_max)
{
    return pk_error_bound(r_cut, bin_size, nbins, n_rows, s_cap, l_max);
}

int mdhip_row_displacement(int n_ti, int n_tj, const int32_t *cls, int32_t *a, int32_t *b, int32_t *row_cls, int *n_rows)
{
    if (n_ti < 1 || n_tj < 1 || !cls || !a || !b || !row_cls || !n_rows) return MDHIP_EINVAL;
    std::vector<int> c(cls, cls + (size_t)n_ti * n_tj), va, vb, vr;
    for (int v : c)
        if (v < 0) return MDHIP_EINVAL;
    const int rows = displace_rows(n_ti, n_tj, c, va, vb, vr);
    *n_rows = rows;
    if (rows > 0) {
        std::copy(va.begin(), va.end(), a);
        std::copy(vb.begin(), vb.end(), b);
        std::copy(vr.begin(), vr.end(), row_cls);
    }
    return MDHIP_OK;
}

// What an atom-atom entry point keeps on the heap while its batch may still be in flight (asynchronous calls): the
// class histograms the batch's completion step fills, and what the entry point's own step needs to turn them into the
// reference's outputs.
struct PairState {
    std::vector<uint64_t> H, Hsplit;
    std::vector<int> rel_cls;
    std::vector<double> c2_cls, edges;
    std::vector<int32_t> rel;
    int n_cls = 0;
    uint64_t ov = 0;
    bool redo = false;  // the launch raised the overflow guard of the 32-bit block histograms: run again, synchronously
};

// The call's own copy of the bin edges: the caller's, or (NULL) the exact edges of trunc(sqrt(rsq) / bin_size).
static const double *own_edges(std::vector<double> &store, const double *edges, double bin_size, int nbins)
{
    if (edges) {
        store.assign(edges, edges + nbins + 1);
    } else {
        store.resize((size_t)nbins + 1);
        mdhip_bin_edges(bin_size, nbins, store.data());
    }
    return store.data();
}

static void atomic_job(RelJob &j, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device, const int32_t *type,
                       int64_t type_frame_stride, const double *box, int n_rel, const int32_t *rel, double r_cut_sq,
                       double bin_size, int nbins, const double *edges, int per_frame)
{
    j.tri = true;
    j.F = n_frames;
    j.ni = j.nj = n_atoms;
    j.xi = xyz;
    j.xi_dev = on_device;
    j.lab_i = type;
    j.lab_i_fs = type_frame_stride;
    j.box = box;
    j.n_rel = n_rel;
    j.rel = rel;
    j.nbins = nbins;
    j.edges = edges;
    j.rc2 = r_cut_sq;
    j.gscale = bin_size > 0.0 ? (float)(1.0 / bin_size) : 0.f;
    j.bin_size = bin_size;
    j.per_frame = per_frame;
}

// ... and of atoms x sites (rectangular: ordered (atom type, site type) classes, one type column for all frames)
static void sites_job(RelJob &j, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device, const int32_t *type,
                      int64_t n_sites, const double *sites, int sites_on_device, const int32_t *site_type, const double *box,
                      int n_rel, const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                      int per_frame)
{
    atomic_job(j, n_frames, n_atoms, xyz, xyz_on_device, type, 0, box, n_rel, rel, r_cut_sq, bin_size, nbins, edges, per_frame);
    j.tri = false;
    j.nj = n_sites;
    j.xj = sites;
    j.xj_dev = sites_on_device;
    j.lab_j = site_type;
}

// Class rows Hf [n_cls][nbins] of one output frame -> the reference's atom-atom outputs (either may be NULL):
// full[bin] += 2 per pair (rdf_cn.py:85-86); part [n_rel][nbins]: the relation's class row, +1 per unordered {a,b}
// pair, +2 when a == b — ASSIGNED (a relation whose labels do not occur: zeros), or with `add` added to what is there.
static void rows_to_outputs(const uint64_t *Hf, int n_cls, int nbins, int n_rel, const int32_t *rel,
                            const std::vector<int> &rel_cls, uint64_t *full, uint64_t *part, bool add)
{
    for (int c = 0; c < n_cls && full; ++c)
        for (int b = 0; b < nbins; ++b) full[b] += 2 * Hf[(size_t)c * nbins + b];
    for (int kl = 0; kl < n_rel && part; ++kl) {
        uint64_t *dst = part + (size_t)kl * nbins;
        if (rel_cls[kl] < 0) {
            if (!add) std::fill(dst, dst + nbins, (uint64_t)0);
            continue;
        }
        const uint64_t mult = rel[2 * kl] == rel[2 * kl + 1] ? 2 : 1;
        const uint64_t *row = Hf + (size_t)rel_cls[kl] * nbins;
        for (int b = 0; b < nbins; ++b) dst[b] = (add ? dst[b] : 0) + mult * row[b];
    }
}

int mdhip_rdf_atomic(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                     int on_device, const int32_t *type, int64_t type_frame_stride,
                     const double *box, int n_rel, const int32_t *rel, double r_cut_sq,
                     double bin_size, int nbins, const double *edges, int per_frame,
                     uint64_t *hist_full, uint64_t *hist_part, uint64_t *overflow)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    int rc = check_common(ctx, n_frames, n_atoms, xyz, type, box, n_rel, rel);
    if (rc) return rc;
    MD_REQUIRE(nbins >= 1 && bin_size > 0.0, "nbins and bin_size must be positive");
    MD_REQUIRE(type_frame_stride == 0 || type_frame_stride == n_atoms,
               "type_frame_stride must be 0 or n_atoms");
    MD_REQUIRE(hist_full && (n_rel == 0 || hist_part), "NULL output");
    MD_HIP(hipSetDevice(ctx->device));
    const size_t out_frames = per_frame ? (size_t)n_frames : 1;
    std::fill(hist_full, hist_full + out_frames * nbins, (uint64_t)0);
    if (n_rel) std::fill(hist_part, hist_part + out_frames * n_rel * nbins, (uint64_t)0);
    if (overflow) *overflow = 0;
    if (n_frames == 0 || n_atoms < 2) return cs.end();

    auto st = std::make_shared<PairState>();
    RelJob j{};
    atomic_job(j, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq, bin_size, nbins,
               own_edges(st->edges, edges, bin_size, nbins), per_frame);
    st->rel.assign(rel, rel + 2 * (size_t)n_rel);
    rc = run_job(ctx, j, st->H, st->rel_cls, st->n_cls, &st->ov, cs.async() ? &cs : nullptr, &st->redo);
    if (rc) return rc;
    cs.defer([=]() {
        if (st->redo)  // (xyz, type, box are the caller's: valid and unchanged until the call has completed)
            return mdhip_rdf_atomic(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel,
                                    st->rel.data(), r_cut_sq, bin_size, nbins, st->edges.data(), per_frame, hist_full,
                                    hist_part, overflow);
        if (overflow) *overflow = st->ov;
        for (size_t f = 0; f < out_frames; ++f)
            rows_to_outputs(&st->H[f * st->n_cls * nbins], st->n_cls, nbins, n_rel, st->rel.data(), st->rel_cls,
                            hist_full + f * nbins, n_rel ? hist_part + f * n_rel * nbins : nullptr, false);
        return (int)MDHIP_OK;
    });
    return cs.end();
}

int mdhip_rdf_atomic_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                         const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                         const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                         uint64_t *out_dev)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    int rc = check_common(ctx, n_frames, n_atoms, xyz, type, box, n_rel, rel);
    if (rc) return rc;
    MD_REQUIRE(nbins >= 1 && bin_size > 0.0, "nbins and bin_size must be positive");
    MD_REQUIRE(type_frame_stride == 0 || type_frame_stride == n_atoms, "type_frame_stride must be 0 or n_atoms");
    MD_REQUIRE(out_dev, "NULL output");
    MD_HIP(hipSetDevice(ctx->device));
    const size_t words = (size_t)(1 + n_rel) * nbins + 1;
    MD_HIP(hipMemsetAsync(out_dev, 0, words * 8, ctx->stream));
    if (n_frames == 0 || n_atoms < 2) return cs.end();
    auto st = std::make_shared<PairState>();
    RelJob j{};
    atomic_job(j, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq, bin_size, nbins,
               own_edges(st->edges, edges, bin_size, nbins), 0);
    j.dev_out = reinterpret_cast<unsigned long long *>(out_dev);
    st->rel.assign(rel, rel + 2 * (size_t)n_rel);
    rc = run_job(ctx, j, st->H, st->rel_cls, st->n_cls, &st->ov, cs.async() ? &cs : nullptr, &st->redo);
    if (rc) return rc;
    cs.defer([=]() {
        if (st->redo)  // (device-resident sums are left untouched by a flagged launch)
            return mdhip_rdf_atomic_dev(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel,
                                        st->rel.data(), r_cut_sq, bin_size, nbins, st->edges.data(), out_dev);
        // batches that did not run as one scalar-j pass (small frames, class passes) came back as host class
        // histograms: add them in (rare path; a D2H / H2D round trip of the output words)
        const std::vector<uint64_t> &H = st->H;
        bool any = st->ov != 0;
        for (size_t k = 0; k < H.size() && !any; ++k) any = H[k] != 0;
        if (!any) return (int)MDHIP_OK;
        CallScope fix(ctx);
        MD_PIN(out, uint64_t, words * 8);
        MD_HIP(hipMemcpyAsync(out, out_dev, words * 8, hipMemcpyDeviceToHost, ctx->stream));
        MD_HIP(mdhip_stream_wait(ctx));
        rows_to_outputs(H.data(), st->n_cls, nbins, n_rel, st->rel.data(), st->rel_cls, out, out + nbins, true);  // ADDED
        out[words - 1] += st->ov;
        MD_HIP(hipMemcpyAsync(out_dev, out, words * 8, hipMemcpyHostToDevice, ctx->stream));
        return fix.end();
    });
    return cs.end();
}

// A finished array of counts goes to the caller: host memory at once, device memory through a copy of its own.
static int deliver_counts(mdhip_ctx *ctx, const uint64_t *src, size_t n, uint64_t *dst, int dst_on_device)
{
    if (!dst_on_device) {
        if (dst != src) memcpy(dst, src, n * 8);
        return MDHIP_OK;
    }
    return mdhip_deliver_to_device(ctx, dst, src, n * 8);
}

// The first condition of the one-sweep route: something to do, and no coordination cutoff beyond r_cut.
static bool cn_within_r_cut(int64_t n_frames, int64_t n_atoms, int n_rel, const double *cn_r_cut_sq, double r_cut_sq)
{
    bool fused = n_rel > 0 && n_frames > 0 && n_atoms >= 2;
    for (int kl = 0; kl < n_rel && fused; ++kl) fused = !(cn_r_cut_sq[kl] > r_cut_sq);
    return fused;
}
constexpr int CN_PK_BINS = 64;  // bins of the coarse histogram mdhip_cn_atomic's cutoffs ride on (option cn_pk)

// One sweep for the histograms AND the coordination counts. hist_full / hist_part / overflow may be
// NULL (coordination counts only: mdhip_cn_atomic runs its cutoffs through here with a coarse 64-bin histogram whose
// cutoff is the largest coordination cutoff). Returns MDHIP_OK, an error, or CN_UNFUSED when this call has to take the
// two-sweep route (a cutoff beyond r_cut, two cutoffs for one class, a geometry the packed sweep does not take).
// The work is issued into the caller's scope `cs`; its host half is a completion step of that call. cn: host, or
// device memory (cn_on_device; frame-summed only).
static int fused_rdf_cn(CallScope &cs, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                        const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                        const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                        const double *cn_r_cut_sq, int per_frame, uint64_t *hist_full, uint64_t *hist_part,
                        uint64_t *overflow, uint64_t *cn, int cn_on_device)
{
    mdhip_ctx *ctx = cs.ctx;
    if (!cn_within_r_cut(n_frames, n_atoms, n_rel, cn_r_cut_sq, r_cut_sq)) return CN_UNFUSED;
    MD_HIP(hipSetDevice(ctx->device));
    const size_t out_frames = per_frame ? (size_t)n_frames : 1;
    auto st = std::make_shared<PairState>();
    RelJob j{};
    atomic_job(j, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq, bin_size, nbins,
               own_edges(st->edges, edges, bin_size, nbins), per_frame);
    st->rel.assign(rel, rel + 2 * (size_t)n_rel);
    auto cuts = std::make_shared<std::vector<double>>(cn_r_cut_sq, cn_r_cut_sq + n_rel);
    j.cn_rc2 = cuts->data();
    j.Hsplit = &st->Hsplit;
    j.cn_c2_cls = &st->c2_cls;
    const int rc = run_job(ctx, j, st->H, st->rel_cls, st->n_cls, &st->ov, cs.async() ? &cs : nullptr, &st->redo);
    if (rc != MDHIP_OK) return rc;  // an error, or CN_UNFUSED
    cs.defer([=]() {
        if (st->redo) {
            // the same sweep again, inside a synchronous call of its own (which halves the batch where it has to)
            CallScope again(ctx);
            const int rc2 = fused_rdf_cn(again, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel,
                                         st->rel.data(), r_cut_sq, bin_size, nbins, st->edges.data(), cuts->data(),
                                         per_frame, hist_full, hist_part, overflow, cn, cn_on_device);
            if (rc2 != MDHIP_OK)
                return rc2 == CN_UNFUSED ? mdhip_fail(ctx, MDHIP_EHIP, "pair_hist: the one-sweep path refused its own re-run") : rc2;
            return again.end();
        }
        const std::vector<uint64_t> &H = st->H, &Hsplit = st->Hsplit;
        const double *use_edges = st->edges.data();
        const int32_t *rl = st->rel.data();
        const int n_cls = st->n_cls;
        if (overflow) *overflow = st->ov;
        if (hist_full) std::fill(hist_full, hist_full + out_frames * nbins, (uint64_t)0);
        std::vector<uint64_t> cn_host(cn_on_device ? out_frames * (size_t)n_rel : 0);
        uint64_t *cn_out = cn_on_device ? cn_host.data() : cn;
        for (size_t f = 0; f < out_frames; ++f) {
            const uint64_t *Hf = &H[f * n_cls * nbins];
            rows_to_outputs(Hf, n_cls, nbins, n_rel, rl, st->rel_cls, hist_full ? hist_full + f * nbins : nullptr,
                            hist_part ? hist_part + f * n_rel * nbins : nullptr, false);
            for (int kl = 0; kl < n_rel; ++kl) {
                uint64_t s = 0;
                const uint64_t mult = rl[2 * kl] == rl[2 * kl + 1] ? 2 : 1;
                if (st->rel_cls[kl] >= 0) {
                    const int cl = st->rel_cls[kl];
                    const uint64_t *row = Hf + (size_t)cl * nbins;
                    const double c2 = st->c2_cls[cl];
                    if (c2 > 0.0) {
                        // bins below the split bin are inside the cutoff (exact edges); the split bin's share was
                        // counted by the exact chain (a cutoff inside the overflow bin, index nbins: all bins plus
                        // the overflow pairs below the cutoff)
                        const int kc = (int)(std::upper_bound(use_edges, use_edges + nbins + 1, c2) - use_edges) - 1;
                        for (int b = 0; b < kc && b < nbins; ++b) s += row[b];
                        s += Hsplit[f * n_cls + cl];
                    }
                }
                cn_out[f * n_rel + kl] = mult * s;
            }
        }
        return deliver_counts(ctx, cn_out, out_frames * (size_t)n_rel, cn, cn_on_device);
    });
    return MDHIP_OK;
}

static int cn_atomic_impl(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                          const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                          const int32_t *rel, const double *r_cut_sq, int per_frame, uint64_t *cn, int cn_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    int rc = check_common(ctx, n_frames, n_atoms, xyz, type, box, n_rel, rel);
    if (rc) return rc;
    MD_REQUIRE(n_rel == 0 || (r_cut_sq && cn), "NULL cutoff or output");
    MD_REQUIRE(type_frame_stride == 0 || type_frame_stride == n_atoms,
               "type_frame_stride must be 0 or n_atoms");
    MD_REQUIRE(!cn_on_device || !per_frame, "a device result buffer holds the frame-summed counts");
    MD_HIP(hipSetDevice(ctx->device));
    const size_t out_frames = per_frame ? (size_t)n_frames : 1;
    rc = mdhip_zero_result(ctx, cn, out_frames * (size_t)n_rel * 8, cn_on_device);
    if (rc) return rc;
    if (n_frames == 0 || n_atoms < 2 || n_rel == 0) return cs.end();
    std::vector<double> edges;
    std::vector<int> rank;
    cn_edges(n_rel, r_cut_sq, edges, rank);
    const int nbins = (int)edges.size() - 1;
    if (nbins == 0) return cs.end();
    if (ctx->opt_cn_pk != 0) {
        // Option cn_pk (default): the packed-f32 sweep with a coarse histogram whose cutoff is the largest coordination
        // cutoff; the counts are the exact bins below each class's split bin plus the split-bin pairs the exact chain
        // finds inside — the same integers as the f64 edge-table kernel below, which is the route for
        // everything the packed sweep does not take (small frames, two cutoffs for one class, ...) and for cn_pk = 0.
        const double c_max = std::sqrt(edges.back());
        const int nb = CN_PK_BINS;
        rc = fused_rdf_cn(cs, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel,
                          edges.back(), c_max / nb, nb, nullptr, r_cut_sq, per_frame, nullptr, nullptr, nullptr, cn,
                          cn_on_device);
        if (rc == MDHIP_OK) return cs.end();
        if (rc != CN_UNFUSED) return rc;
    }
    RelJob j{};
    atomic_job(j, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, edges.back(), 0.0, nbins,
               edges.data(), per_frame);
    std::vector<uint64_t> H;
    std::vector<int> rel_cls;
    int n_cls = 0;
    uint64_t ov = 0;
    rc = run_job(ctx, j, H, rel_cls, n_cls, &ov);  // (edge-table kernel: completes inside)
    if (rc) return rc;
    std::vector<uint64_t> cn_host(out_frames * (size_t)n_rel, 0);
    for (size_t f = 0; f < out_frames; ++f)
        for (int kl = 0; kl < n_rel; ++kl) {
            if (rel_cls[kl] < 0) continue;
            const uint64_t mult = rel[2 * kl] == rel[2 * kl + 1] ? 2 : 1;
            const uint64_t *row = &H[(f * n_cls + rel_cls[kl]) * nbins];
            uint64_t s = 0;
            for (int b = 0; b < rank[kl]; ++b) s += row[b];
            cn_host[f * n_rel + kl] = mult * s;
        }
    if (cn_on_device) {
        rc = mdhip_h2d_small(ctx, cn, cn_host.data(), cn_host.size() * 8);
        if (rc) return rc;
    } else {
        memcpy(cn, cn_host.data(), cn_host.size() * 8);
    }
    return cs.end();
}

int mdhip_rdf_cn_atomic(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                        const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                        const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                        const double *cn_r_cut_sq, int per_frame, uint64_t *hist_full, uint64_t *hist_part,
                        uint64_t *overflow, uint64_t *cn)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    int rc = check_common(ctx, n_frames, n_atoms, xyz, type, box, n_rel, rel);
    if (rc) return rc;
    MD_REQUIRE(nbins >= 1 && bin_size > 0.0, "nbins and bin_size must be positive");
    MD_REQUIRE(type_frame_stride == 0 || type_frame_stride == n_atoms, "type_frame_stride must be 0 or n_atoms");
    MD_REQUIRE(hist_full && (n_rel == 0 || (hist_part && cn_r_cut_sq && cn)), "NULL output or cutoff array");
    rc = fused_rdf_cn(cs, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq,
                      bin_size, nbins, edges, cn_r_cut_sq, per_frame, hist_full, hist_part, overflow, cn, 0);
    if (rc == MDHIP_OK) return cs.end();
    if (rc != CN_UNFUSED) return rc;
    // this call does not run as one packed sweep — two sweeps (calls of their own, complete on return), same integers
    rc = mdhip_rdf_atomic(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq,
                          bin_size, nbins, edges, per_frame, hist_full, hist_part, overflow);
    if (rc) return rc;
    rc = cn_atomic_impl(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel,
                        cn_r_cut_sq, per_frame, cn, 0);
    if (rc) return rc;
    return cs.end();
}

int mdhip_cn_atomic(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                    int on_device, const int32_t *type, int64_t type_frame_stride,
                    const double *box, int n_rel, const int32_t *rel, const double *r_cut_sq,
                    int per_frame, uint64_t *cn)
{
    return cn_atomic_impl(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq,
                          per_frame, cn, 0);
}

int mdhip_cn_atomic_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                        const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                        const int32_t *rel, const double *r_cut_sq, uint64_t *cn_dev)
{
    if (!ctx) return MDHIP_EINVAL;
    MD_REQUIRE(n_rel == 0 || cn_dev, "NULL output");
    return cn_atomic_impl(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq, 0,
                          cn_dev, 1);
}

/* ---- asynchronous twins (results complete after mdhip_sync / mdhip_wait; inputs must stay valid until then) ---- */
int mdhip_rdf_atomic_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                           const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                           const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                           int per_frame, uint64_t *hist_full, uint64_t *hist_part, uint64_t *overflow)
{
    if (!ctx) return MDHIP_EINVAL;
    AsyncCall mark(ctx, pair_overlap_ok(ctx, n_frames, n_atoms, on_device));
    return mdhip_rdf_atomic(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq,
                            bin_size, nbins, edges, per_frame, hist_full, hist_part, overflow);
}

int mdhip_rdf_atomic_dev_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                               const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                               const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                               uint64_t *out_dev)
{
    if (!ctx) return MDHIP_EINVAL;
    AsyncCall mark(ctx, pair_overlap_ok(ctx, n_frames, n_atoms, on_device));
    return mdhip_rdf_atomic_dev(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq,
                                bin_size, nbins, edges, out_dev);
}

int mdhip_rdf_cn_atomic_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                              const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                              const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *edges,
                              const double *cn_r_cut_sq, int per_frame, uint64_t *hist_full, uint64_t *hist_part,
                              uint64_t *overflow, uint64_t *cn)
{
    if (!ctx) return MDHIP_EINVAL;
    AsyncCall mark(ctx, pair_overlap_ok(ctx, n_frames, n_atoms, on_device));
    return mdhip_rdf_cn_atomic(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq,
                               bin_size, nbins, edges, cn_r_cut_sq, per_frame, hist_full, hist_part, overflow, cn);
}

int mdhip_cn_atomic_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int on_device,
                          const int32_t *type, int64_t type_frame_stride, const double *box, int n_rel,
                          const int32_t *rel, const double *r_cut_sq, int per_frame, uint64_t *cn, int cn_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    AsyncCall mark(ctx, pair_overlap_ok(ctx, n_frames, n_atoms, on_device));
    return cn_atomic_impl(ctx, n_frames, n_atoms, xyz, on_device, type, type_frame_stride, box, n_rel, rel, r_cut_sq,
                          per_frame, cn, cn_on_device ? 1 : 0);
}

int mdhip_rdf_sites(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                    int xyz_on_device, const int32_t *type, int64_t n_sites, const double *sites,
                    int sites_on_device, const int32_t *site_type, const double *box, int n_rel,
                    const int32_t *rel, double r_cut_sq, double bin_size, int nbins,
                    const double *edges, int per_frame, uint64_t *hist_part, uint64_t *overflow)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);  // (atoms x sites: completes inside)
    int rc = check_common(ctx, n_frames, n_atoms, xyz, type, box, n_rel, rel);
    if (rc) return rc;
    MD_REQUIRE(n_sites >= 0 && n_sites < (1LL << 31), "bad n_sites");
    MD_REQUIRE(n_frames == 0 || n_sites == 0 || (sites && site_type), "NULL site arrays");
    MD_REQUIRE(nbins >= 1 && bin_size > 0.0, "nbins and bin_size must be positive");
    MD_REQUIRE(n_rel == 0 || hist_part, "NULL output");
    MD_HIP(hipSetDevice(ctx->device));
    const size_t out_frames = per_frame ? (size_t)n_frames : 1;
    if (n_rel) std::fill(hist_part, hist_part + out_frames * n_rel * nbins, (uint64_t)0);
    if (overflow) *overflow = 0;
    if (n_frames == 0 || n_atoms == 0 || n_sites == 0 || n_rel == 0) return cs.end();
    std::vector<double> edge_store;
    RelJob j{};
    sites_job(j, n_frames, n_atoms, xyz, xyz_on_device, type, n_sites, sites, sites_on_device, site_type, box, n_rel, rel,
              r_cut_sq, bin_size, nbins, own_edges(edge_store, edges, bin_size, nbins), per_frame);
    std::vector<uint64_t> H;
    std::vector<int> rel_cls;
    int n_cls = 0;
    uint64_t ov = 0;
    rc = run_job(ctx, j, H, rel_cls, n_cls, &ov);
    if (rc) return rc;
    if (overflow) *overflow = ov;
    for (size_t f = 0; f < out_frames; ++f)
        for (int kl = 0; kl < n_rel; ++kl) {
            if (rel_cls[kl] < 0) continue;
            memcpy(hist_part + (f * n_rel + kl) * nbins, &H[(f * n_cls + rel_cls[kl]) * nbins],
                   (size_t)nbins * 8);
        }
    return cs.end();
}

int mdhip_cn_sites(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz,
                   int xyz_on_device, const int32_t *type, int64_t n_sites, const double *sites,
                   int sites_on_device, const int32_t *site_type, const double *box, int n_rel,
                   const int32_t *rel, const double *r_cut_sq, int per_frame, uint64_t *cn)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);  // (atoms x sites: completes inside)
    int rc = check_common(ctx, n_frames, n_atoms, xyz, type, box, n_rel, rel);
    if (rc) return rc;
    MD_REQUIRE(n_sites >= 0 && n_sites < (1LL << 31), "bad n_sites");
    MD_REQUIRE(n_frames == 0 || n_sites == 0 || (sites && site_type), "NULL site arrays");
    MD_REQUIRE(n_rel == 0 || (r_cut_sq && cn), "NULL cutoff or output");
    MD_HIP(hipSetDevice(ctx->device));
    const size_t out_frames = per_frame ? (size_t)n_frames : 1;
    std::fill(cn, cn + out_frames * n_rel, (uint64_t)0);
    if (n_frames == 0 || n_atoms == 0 || n_sites == 0 || n_rel == 0) return cs.end();
    std::vector<double> edges;
    std::vector<int> rank;
    cn_edges(n_rel, r_cut_sq, edges, rank);
    const int nbins = (int)edges.size() - 1;
    if (nbins == 0) return cs.end();
    RelJob j{};
    sites_job(j, n_frames, n_atoms, xyz, xyz_on_device, type, n_sites, sites, sites_on_device, site_type, box, n_rel, rel,
              edges.back(), 0.0, nbins, edges.data(), per_frame);
    std::vector<uint64_t> H;
    std::vector<int> rel_cls;
    int n_cls = 0;
    uint64_t ov = 0;
    rc = run_job(ctx, j, H, rel_cls, n_cls, &ov);
    if (rc) return rc;
    for (size_t f = 0; f < out_frames; ++f)
        for (int kl = 0; kl < n_rel; ++kl) {
            if (rel_cls[kl] < 0) continue;
            const uint64_t *row = &H[(f * n_cls + rel_cls[kl]) * nbins];
            uint64_t s = 0;
            for (int b = 0; b < rank[kl]; ++b) s += row[b];
            cn[f * n_rel + kl] = s;
        }
    return cs.end();
}

int mdhip_pair_plan(const mdhip_ctx *ctx, int op, int64_t n_frames, int64_t n_atoms, const int32_t *type, int64_t n_type,
                    int64_t n_sites, const int32_t *site_type, int64_t n_site_type, const double *box, int n_rel,
                    const int32_t *rel, double r_cut_sq, double bin_size, int nbins, const double *cn_r_cut_sq, int per_frame,
                    int result_on_device, int xyz_on_device, int cu_count, int64_t lds_bytes, int n_opt,
                    const char *const *opt_key, const int *opt_value, char *text, int text_cap, int32_t *info)
{
    if (!text || text_cap < 1 || !info || op < MDHIP_PLAN_RDF || op > MDHIP_PLAN_RDF_CN) return MDHIP_EINVAL;
    if (n_frames < 0 || n_atoms < 0 || n_sites < 0 || n_type < 0 || n_rel < 0 || (n_rel && !rel)) return MDHIP_EINVAL;
    if (n_frames && n_atoms && (!type || !box)) return MDHIP_EINVAL;
    if (op != MDHIP_PLAN_RDF && (n_rel && !cn_r_cut_sq)) return MDHIP_EINVAL;
    if (op != MDHIP_PLAN_CN && !(nbins >= 1 && bin_size > 0.0)) return MDHIP_EINVAL;
    if (op == MDHIP_PLAN_RDF_CN && site_type) return MDHIP_EINVAL;
    mdhip_ctx c = ctx ? *ctx : mdhip_ctx();  // (a copy: options and limits only — nothing below touches a device)
    if (cu_count > 0) c.cu_count = cu_count;
    if (lds_bytes > 0) c.lds_max = (size_t)lds_bytes;
    text[0] = 0;
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[1] = -1;
    auto fail = [&](int code) {
        info[0] = code;
        snprintf(text, (size_t)text_cap, "%s", c.err.c_str());
        return (int)MDHIP_OK;
    };
    for (int k = 0; k < n_opt; ++k)
        if (const int rc = mdhip_set_option(&c, opt_key[k], opt_value[k])) return fail(rc);
    const bool tri = site_type == nullptr;
    if (n_frames == 0 || (tri ? n_atoms < 2 : n_atoms == 0 || n_sites == 0 || n_rel == 0)) return MDHIP_OK;  // nothing runs
    if (op == MDHIP_PLAN_CN && n_rel == 0) return MDHIP_OK;

    PairProblem p{};
    std::vector<int> rel_cls;
    std::vector<int32_t> idx_i, idx_j;
    if (const int rc = classify(&c, tri, type, (size_t)n_type, site_type, (size_t)n_site_type, n_rel, rel, p, rel_cls, idx_i, idx_j))
        return fail(rc);
    p.ni = n_atoms;
    p.nj = tri ? n_atoms : n_sites;
    p.per_frame = per_frame;
    if (result_on_device && op == MDHIP_PLAN_RDF && tri) {  // (mdhip_rdf_atomic_dev; the plan asks only whether it is set)
        static unsigned long long somewhere;
        p.dev_out = &somewhere;
        p.n_rel = n_rel;
    }
    const bool staged = c.opt_h2d_overlap != 0 && !xyz_on_device;  // (as a synchronous call stages host-resident frames)
    const auto parts = batch_parts(&c, n_frames, n_atoms, staged);
    std::vector<double> c2;
    // one sweep of all batches -> MDHIP_OK (info and text describe it), CN_UNFUSED, or an error
    auto sweep = [&](double rc2, double bsz, int nb, const double *cuts) {
        p.rc2 = rc2;
        p.bin_size = bsz;
        p.gscale = bsz > 0.0 ? (float)(1.0 / bsz) : 0.f;
        p.nbins = nb;
        p.n_cn = 0;
        if (cuts) {
            if (!class_cutoffs(n_rel, rel_cls, cuts, p.n_cls, c2)) return (int)CN_UNFUSED;
            p.n_cn = 1;
            p.cn_c2_cls = c2.data();
        }
        info[3] = 0;
        for (size_t k = 0; k < parts.size(); ++k) {
            PairPlan pl;
            p.n_frames = parts[k].second;
            p.h_box = box + 3 * parts[k].first;
            if (const int rc = pair_plan(&c, p, pl)) return rc;
            info[3] += pl.n_pass;
            if (k) continue;  // (the first batch is the one described)
            info[1] = pl.sj_mode;
            info[2] = pl.n_pass;
            info[4] = pl.ordered ? pl.ord_rows : 0;
            info[5] = pl.ordered && pl.displaced;
            info[6] = pl.big;
            info[7] = pl.pk && pl.sj_mode >= 3;
            snprintf(text, (size_t)text_cap, "%s", pl.kname);
        }
        return (int)MDHIP_OK;
    };
    int rc;
    if (op == MDHIP_PLAN_RDF) {
        rc = sweep(r_cut_sq, bin_size, nbins, nullptr);
    } else if (op == MDHIP_PLAN_RDF_CN) {
        rc = cn_within_r_cut(n_frames, n_atoms, n_rel, cn_r_cut_sq, r_cut_sq) ? sweep(r_cut_sq, bin_size, nbins, cn_r_cut_sq)
                                                                             : (int)CN_UNFUSED;
        if (rc == CN_UNFUSED) {  // two sweeps: the RDF's is the one described
            rc = sweep(r_cut_sq, bin_size, nbins, nullptr);
            if (rc == MDHIP_OK) rc = CN_UNFUSED;
        }
    } else {
        std::vector<double> edges;
        std::vector<int> rank;
        cn_edges(n_rel, cn_r_cut_sq, edges, rank);
        const int nb = (int)edges.size() - 1;
        if (nb == 0) return MDHIP_OK;
        rc = CN_UNFUSED;
        if (tri && c.opt_cn_pk != 0 && cn_within_r_cut(n_frames, n_atoms, n_rel, cn_r_cut_sq, edges.back()))
            rc = sweep(edges.back(), std::sqrt(edges.back()) / CN_PK_BINS, CN_PK_BINS, cn_r_cut_sq);
        if (rc == CN_UNFUSED) rc = sweep(edges.back(), 0.0, nb, nullptr);
    }
    if (rc < 0) return fail(rc);
    info[0] = rc;
    return MDHIP_OK;
}

}  // extern "C"
