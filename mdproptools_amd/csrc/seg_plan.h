// seg_plan.h — which segment kernel one per-molecule COM or charge-flux call runs, its tables and its grid, decided
// from the segment table's shape alone.
//
// Everything here is host arithmetic on plain values (the CU count, the seg_* options, the segment offsets, the plane
// and frame counts): no HIP header, no context, no device call. segment_com.hip (the only includer inside the
// library) launches what seg_plan() returns; tests/native/seg_plan_main.cpp walks the tables under sanitizers.
// An unnamed namespace, as the kernels of segment_com.hip that take SegBlock / SegRun: their symbols keep their names.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

// A run of whole segments [s0, s1) that fits one block's LDS stage (segment_staged_kernel)
struct SegBlock {
    long long s0, s1;
};
// The same with the run's atom range [a0, a0 + na) (segment_frame_kernel)
struct SegRun {
    long long s0, s1, a0;
    int na, pad_;
};
constexpr int SC_CAP_MAX = 1024;  // atoms per block stage (CAP of the kernels: 1024, 512 or 256)
constexpr int SC_PLANES = 3;      // attribute planes staged together (x, y, z): one barrier pair per frame

// Runs of whole segments with <= SC_CAP atoms and <= 256 segments each; false when a segment is longer.
inline bool build_seg_blocks(int64_t n_seg, const int64_t *seg_off, std::vector<SegBlock> &blocks, int SC_CAP = SC_CAP_MAX,
                             int max_segs = 256)
{
    blocks.clear();
    int64_t s0 = 0;
    while (s0 < n_seg) {
        int64_t s1 = s0;
        while (s1 < n_seg && s1 - s0 < max_segs && seg_off[s1 + 1] - seg_off[s0] <= SC_CAP) ++s1;
        if (s1 == s0) return false;  // segment s0 alone exceeds the LDS stage
        blocks.push_back({(long long)s0, (long long)s1});
        s0 = s1;
    }
    return true;
}

// Stage size of the by-frame kernel for a segment table (round 5; measured at C4 size, tools/ab_seg_cap.py): 1024 atoms per
// block unless that leaves the block's second phase — one lane per (segment, plane) sum, 256 lanes a round — mostly idle
// rounds (10-atom molecules: 102 segments x 3 planes = 306 sums = two rounds for 1.2 rounds' worth: 0.515 -> 0.478 ms with
// 512-atom stages) or the stage mostly empty (3-atom molecules: the 256-segment limit fills 768 of 1024: 0.722 -> 0.69).
// Molecules of 4, 16, 40 atoms and mixes of them keep 1024 (512: 2-7 % slower).
inline int pick_seg_cap(int64_t n_seg, const int64_t *seg_off, int n_attr, std::vector<SegBlock> &blocks)
{
    if (!build_seg_blocks(n_seg, seg_off, blocks, SC_CAP_MAX, 256)) {
        blocks.clear();  // (a segment longer than the stage: the caller takes the one-lane-per-segment kernel)
        return SC_CAP_MAX;
    }
    const int planes = n_attr < SC_PLANES ? n_attr : SC_PLANES;
    double rounds = 0.0, tasks = 0.0, atoms = 0.0;
    for (const SegBlock &b : blocks) {
        const double t = (double)planes * (double)(b.s1 - b.s0);
        rounds += std::ceil(t / 256.0);
        tasks += t;
        atoms += (double)(seg_off[b.s1] - seg_off[b.s0]);
    }
    const bool idle_rounds = rounds > (double)blocks.size() && rounds * 256.0 > 1.5 * tasks;
    const bool empty_stage = atoms < 0.85 * (double)SC_CAP_MAX * (double)blocks.size() && blocks.size() > 1;
    if (!(idle_rounds || empty_stage)) return SC_CAP_MAX;
    std::vector<SegBlock> half;
    if (!build_seg_blocks(n_seg, seg_off, half, 512, 256)) return SC_CAP_MAX;
    blocks.swap(half);
    return 512;
}

// Sums that do not depend on the frame, on the host in index order from 0.0: sums[s] = the mass sum of segment s and,
// where there are charges, sums[n_seg + s] = its charge sum. They are mdhip_segment_com's seg_mass / seg_q, the by-frame
// COM kernel's seg_msum and (the charge sums times charge_conv) the by-frame flux kernel's table.
inline std::vector<double> seg_sums(int64_t n_seg, const int64_t *seg_off, const double *atom_mass, const double *atom_q)
{
    std::vector<double> sums((size_t)n_seg * (atom_q ? 2 : 1));
    for (int64_t s = 0; s < n_seg; ++s) {
        double m = 0.0, q = 0.0;
        for (int64_t a = seg_off[s]; a < seg_off[s + 1]; ++a) {
            m += atom_mass[a];
            if (atom_q) q += atom_q[a];
        }
        sums[(size_t)s] = m;
        if (atom_q) sums[(size_t)(n_seg + s)] = q;
    }
    return sums;
}

// the context's seg_* options in this order (defaults as ctx.h)
struct SegOptions {
    int cap = 0, frame = 1, gy = 0, vec = 1;
};

// walk: one lane per (segment, frame) in global memory (segment_com_kernel | mol_flux_kernel); staged:
// segment_staged_kernel, a block loops over the frames of its slice; by frame: segment_frame_kernel
enum SegForm { SEG_WALK = 0, SEG_STAGED = 1, SEG_FRAME = 2 };

struct SegPlan {
    int form = SEG_WALK;
    int cap = SC_CAP_MAX;          // atoms per block stage: 256 | 512 | 1024
    int threads = 256;             // per block (64: the wave-private staged form of cap 256)
    int vec = 1;                   // staged: 16-byte loads when alignment allows
    std::vector<SegBlock> blocks;  // staged and by frame: the runs
    std::vector<SegRun> runs;      // by frame: the runs with their atom ranges
    unsigned gx = 0, gy = 1;       // the grid
    long long n_steps = 0;         // by frame: (frame, plane group) steps; otherwise the frames
    const char *name = "";         // what mdhip_last_kernel_name reports after the call

    int max_segs() const { return cap == 256 ? 64 : 256; }  // segments per run at most
};

// The single place that decides. n_attr = 3 for the flux (its steps are then the frames).
inline SegPlan seg_plan(const SegOptions &opt, int cu_count, int64_t n_seg, const int64_t *seg_off, int n_attr,
                        int64_t n_frames, bool flux)
{
    SegPlan pl;
    pl.vec = opt.vec;
    // default: four waves share a 1024-atom stage; seg_cap = 256 selects the wave-private form (one wave per block,
    // 256-atom stage, no block barrier that costs anything) — measured 0.61 against 0.635 of HBM spec at C4 shape, so
    // the two barriers per step are not what limits this kernel
    pl.cap = opt.cap == 512 ? 512 : opt.cap == 256 ? 256 : SC_CAP_MAX;
    bool staged;
    if (opt.cap == 0 && opt.frame != 0) {  // (default: by the shape of the segment table)
        pl.cap = pick_seg_cap(n_seg, seg_off, n_attr, pl.blocks);
        staged = !pl.blocks.empty();
    } else {
        staged = build_seg_blocks(n_seg, seg_off, pl.blocks, pl.cap, pl.max_segs());
        if (!staged && pl.cap != SC_CAP_MAX) {  // (a stage too small for a segment: 1024)
            pl.cap = SC_CAP_MAX;
            staged = build_seg_blocks(n_seg, seg_off, pl.blocks, pl.cap, pl.max_segs());
        }
        staged = staged && !pl.blocks.empty();  // (no segment at all: no run, as pick_seg_cap)
    }
    pl.n_steps = n_frames;
    if (!staged) {
        pl.blocks.clear();
        pl.gx = (unsigned)((n_seg + 255) / 256);
        pl.gy = (unsigned)std::min<int64_t>(n_frames, 4096);
        pl.name = flux ? "mol_flux_kernel" : "segment_com_kernel";
        return pl;
    }
    pl.gx = (unsigned)pl.blocks.size();
    if (opt.frame != 0 && pl.cap != 256) {  // (cap 256 is the staged kernel whatever seg_frame says)
        pl.form = SEG_FRAME;
        for (const SegBlock &b : pl.blocks)
            pl.runs.push_back({b.s0, b.s1, (long long)seg_off[b.s0], (int)(seg_off[b.s1] - seg_off[b.s0]), 0});
        pl.n_steps = (long long)n_frames * ((n_attr + SC_PLANES - 1) / SC_PLANES);
        pl.gy = (unsigned)std::min<long long>(pl.n_steps, 65535);
        pl.name = pl.cap == 512 ? (flux ? "segment_frame_kernel<true, 512>" : "segment_frame_kernel<false, 512>")
                                : (flux ? "segment_frame_kernel<true, 1024>" : "segment_frame_kernel<false, 1024>");
        return pl;
    }
    pl.form = SEG_STAGED;
    pl.threads = pl.cap == 256 ? 64 : 256;
    // frame slices: at least enough (block, slice) pairs to fill the chip several times over, and short runs of
    // ~10 frames per block (measured at C4 shape: 82 slices 0.57 of HBM spec, 512 slices 0.63, 1250 slices 0.60)
    int64_t want = ((int64_t)cu_count * 16 + (int64_t)pl.blocks.size() - 1) / (int64_t)pl.blocks.size();
    want = std::max<int64_t>(want, n_frames / 10);
    pl.gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_frames, std::min<int64_t>(want, 65535)));
    if (opt.gy > 0) pl.gy = (unsigned)std::min<int64_t>(std::min<int64_t>(n_frames, 65535), opt.gy);
    pl.name = pl.cap == 256   ? (flux ? "segment_staged_kernel<true, 256, 64>" : "segment_staged_kernel<false, 256, 64>")
              : pl.cap == 512 ? (flux ? "segment_staged_kernel<true, 512, 256>" : "segment_staged_kernel<false, 512, 256>")
                              : (flux ? "segment_staged_kernel<true, 1024, 256>" : "segment_staged_kernel<false, 1024, 256>");
    return pl;
}

}  // namespace
