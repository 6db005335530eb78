// mol_tile.h — what the four calls over JOBS OF MOLECULES share: mdhip_axis_vectors (reorient.hip), mdhip_dihedral_angles
// (dihedrals.hip), mdhip_mol_moments (moments.hip) and mdhip_mol_shape (mol_shape.hip, through shape_plan.h). A JOB
// covers job_mols molecules of job_len atoms from atom job_atom0 on and yields one series per molecule; the trajectory
// is frame-major [F][3][A].
// All four: the job walk (mol_jobs: the range rule, series0, the 2^40 result rule), its refusal texts (mt_plan_error),
//   the call's arrays on the device (MolIo), where a result is written and how it reaches the caller (MolOut) and the
//   single wrap (mt_wrap). Moments and shape besides: the launch loop of their per-(frame, job) totals
//   (mt_launch_totals). Axis vectors and moments: the ascent rule of a term list (mt_terms_ascend).
// Axis vectors, dihedrals and moments work the tile below under mt_launch (shape has runs of its own: shape_plan.h);
// the first two write series U[s][.][t], time-major [S][3][F], through the LDS tile (mt_store). The device tables of
// all four are packed by call_tables.h.
// The tile: a workgroup owns MT_TM = 64 molecules x MT_TF = 64 frames. Lane = molecule while reading (consecutive lanes
//   read atoms one molecule apart, every fetched line is used by the neighbouring terms and lanes), the finished
//   components go through an LDS tile ([C][64][64 + 1], conflict-free both ways), lane = frame while writing (512
//   contiguous bytes per wave and row). 16 waves per workgroup keep four frames x three axes x the named atoms of loads
//   in flight per lane. One read of the lines that hold named atoms, one write of U: HBM-bound.
// The plan: jobs over the same molecules (same first atom, count and length) may be pooled into a CLASS, whose tiles one
//   workgroup works job after job: the lines of a tile come from HBM once and from the caches for the other jobs.
//   Molecule tiles are numbered class after class; a workgroup finds its class through `tile0`.
// The host plan is arithmetic on plain values (no HIP header, no context), in the form of seg_plan.h:
// tests/native/mol_plan_main.cpp includes this header with g++ and walks it under sanitizers. The device walker and the
// launch helpers are for hipcc only. What a kernel computes per (molecule, frame) stays in its own file. An unnamed
// namespace, as the kernels that take MolClass: their symbols keep their names.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <numeric>
#include <tuple>
#include <vector>

namespace {

constexpr int MT_TM = 64;          // molecules per tile
constexpr int MT_TF = 64;          // frames per tile
constexpr int MT_WAVES = 16;
constexpr int MT_THREADS = 64 * MT_WAVES;
constexpr int MT_ROW = MT_TF + 1;  // doubles per (component, molecule) row of the LDS tile
constexpr long long MT_MAX_GRID = 65535;
constexpr size_t mt_tile_lds(int comps) { return (size_t)comps * MT_TM * MT_ROW * 8; }  // bytes of a tile of `comps` components

// ---- host plan ------------------------------------------------------------------------------------------------------

struct MolClass {
    long long atom0, mols, tile0;  // first atom, molecules, first molecule tile of the class
    int len, job0, n_jobs, pad;    // atoms per molecule; its jobs stand at the positions job0 .. job0 + n_jobs
};

// RANGE: job `bad_job` does not lie inside the n_atoms atoms of a frame; RESULT: with it the series times n_frames reach 2^40
enum MolPlanError { MOL_PLAN_OK = 0, MOL_PLAN_RANGE, MOL_PLAN_RESULT };

// The job walk of every plan: where the series of each job start, and the FIRST job that breaks a rule.
struct MolJobs {
    std::vector<long long> series0;  // first series of every job, in call order
    long long series = 0;
    int error = MOL_PLAN_OK, bad_job = -1;  // the FIRST offending job
    // the jobs whose own checks an entry point makes before it reports `error` (RESULT comes behind every job's checks)
    int checked_jobs() const { return error == MOL_PLAN_RANGE ? bad_job : (int)series0.size(); }
};

// Walks the jobs in call order into `w` and stops at the first one out of RANGE. fits(j, atom0, mols, len) sees every
// job in range and says whether the plan's own result rule still holds with it (true where there is none); the first
// job at which it does not, or with which the series times n_frames reach 2^40, is the RESULT error — the walk goes on
// behind it, since a later job out of range is reported first.
template <class Fits>
inline void mol_jobs(MolJobs &w, int n_jobs, const int64_t *job_atom0, const int64_t *job_mols, const int32_t *job_len,
                     int64_t n_atoms, int64_t n_frames, Fits fits)
{
    w.series0.resize((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const long long len = job_len[j], mols = job_mols[j], a0 = job_atom0[j];
        if (!(len >= 1 && mols >= 0 && a0 >= 0 && a0 <= n_atoms && mols <= (n_atoms - a0) / len)) {
            w.error = MOL_PLAN_RANGE, w.bad_job = j;
            return;
        }
        w.series0[(size_t)j] = w.series;
        w.series += mols;
        const bool fit = fits(j, a0, mols, len);
        if (w.error == MOL_PLAN_OK && (w.series >= (1ll << 40) / n_frames || !fit)) w.error = MOL_PLAN_RESULT, w.bad_job = j;
    }
}

struct MolPlan : MolJobs {
    std::vector<MolClass> classes;  // in the order of their first job
    std::vector<int> order;         // order[p] = the job (call order) at position p: class after class, call order inside
    long long tiles = 0;
};

// pool = false: every job is a class of its own. pool = true: jobs with equal (atom0, mols, len) share a class until it
// holds max_class_jobs; the next such job opens another one. What only a family knows about a job (the terms of an axis
// vector; the quadruple and histogram row of a dihedral) goes into a table of that family, by position.
inline MolPlan mol_plan(int n_jobs, const int64_t *job_atom0, const int64_t *job_mols, const int32_t *job_len,
                        int64_t n_atoms, int64_t n_frames, bool pool, int max_class_jobs)
{
    MolPlan pl;
    std::vector<int> class_of((size_t)n_jobs);
    std::map<std::tuple<long long, long long, long long>, int> open;  // (atom0, mols, len) -> the class still taking jobs
    mol_jobs(pl, n_jobs, job_atom0, job_mols, job_len, n_atoms, n_frames, [&](int j, long long a0, long long mols, long long len) {
        int &c = class_of[(size_t)j] = -1;
        const auto it = pool ? open.find(std::make_tuple(a0, mols, len)) : open.end();
        if (it != open.end() && pl.classes[(size_t)it->second].n_jobs < max_class_jobs) c = it->second;
        if (c < 0) {
            c = (int)pl.classes.size();
            pl.classes.push_back({a0, mols, 0, (int)len, 0, 0, 0});
            if (pool) open.insert_or_assign(std::make_tuple(a0, mols, len), c);
        }
        ++pl.classes[(size_t)c].n_jobs;
        return true;
    });
    if (pl.error != MOL_PLAN_OK) return pl;
    int first = 0;
    for (MolClass &c : pl.classes) {
        c.tile0 = pl.tiles, c.job0 = first;
        pl.tiles += (c.mols + MT_TM - 1) / MT_TM;
        first += c.n_jobs;
    }
    pl.order.resize((size_t)n_jobs);
    std::iota(pl.order.begin(), pl.order.end(), 0);
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](int a, int b) { return class_of[(size_t)a] < class_of[(size_t)b]; });
    return pl;
}

}  // namespace

#ifdef __HIPCC__
#include "ctx.h"

namespace {

// ---- device walker --------------------------------------------------------------------------------------------------

// What block (x, y) of a launch works: molecule tile tile_base + x (over all classes), frame tile ftile_base + y
struct MolTile {
    MolClass cls;
    long long m0, f0;  // first molecule (inside the class) and first frame of the tile
    int nm, nf, lane, wave;  // molecules and frames in it; the thread's lane and wave
};

__device__ __forceinline__ MolTile mt_locate(const MolClass *__restrict__ classes, int n_classes, long long tile_base,
                                             long long ftile_base, long long F)
{
    const long long tile = tile_base + blockIdx.x;
    int lo = 0, hi = n_classes - 1;  // the last class whose first tile is not beyond this one (classes without molecules have none)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (classes[mid].tile0 <= tile) lo = mid;
        else hi = mid - 1;
    }
    MolTile t;
    t.cls = classes[lo];
    t.m0 = (tile - t.cls.tile0) * MT_TM;
    t.nm = (int)(t.cls.mols - t.m0 < MT_TM ? t.cls.mols - t.m0 : MT_TM);
    t.f0 = (ftile_base + blockIdx.y) * MT_TF;
    t.nf = (int)(F - t.f0 < MT_TF ? F - t.f0 : MT_TF);
    t.lane = threadIdx.x & 63, t.wave = threadIdx.x >> 6;
    return t;
}

// One job's pass over the tile, lane = molecule and wave = frame: body(a, f, ff, zeros) for the lane's molecule (first
// atom a) at the frames f = f0 + ff of its wave; it counts in `zeros` where the molecule has no direction, and the
// lane's count is added to *degenerate (64-bit integer atomic, once per lane).
template <class Body>
__device__ __forceinline__ void mt_walk(const MolTile &t, unsigned long long *degenerate, Body body)
{
    if (t.lane >= t.nm) return;
    const long long a = t.cls.atom0 + (t.m0 + t.lane) * t.cls.len;
    unsigned long long zeros = 0;
    for (int ff = t.wave; ff < t.nf; ff += MT_WAVES) body(a, t.f0 + ff, ff, zeros);
    if (zeros) atomicAdd(degenerate, zeros);
}

// The single wrap of the reference (rdf_cn.py:50-55) of a difference d against the edge L, half = L / 2: strict on both
// sides — a difference of exactly half an edge stays — and applied once; a NaN (in d or in the box) shifts nothing.
__device__ __forceinline__ double mt_wrap(double d, double L, double half)
{
    if (d > half) d -= L;
    else if (d < -half) d += L;
    return d;
}

// where component `comp` of molecule `mol` at frame `ff` of the tile stands in the LDS tile [C][MT_TM][MT_ROW]
__device__ __forceinline__ int mt_at(int comp, int mol, int ff) { return (comp * MT_TM + mol) * MT_ROW + ff; }

// The finished tile to U[series0 + m0 ..][3][F], lane = frame; of the three rows of a series the first C come from the
// tile, the others are zeros. Every thread of the block calls it, behind the barrier that follows the fill.
template <int C>
__device__ __forceinline__ void mt_store(const MolTile &t, const double *s_u, long long series0, long long F,
                                         double *__restrict__ U)
{
    for (int row = t.wave; row < 3 * t.nm; row += MT_WAVES) {
        const int mol = row / 3, comp = row - 3 * mol;
        if (t.lane < t.nf)
            U[((size_t)(series0 + t.m0 + mol) * 3 + comp) * (size_t)F + (size_t)(t.f0 + t.lane)] =
                C == 3 || comp < C ? s_u[mt_at(comp, mol, t.lane)] : 0.0;
    }
}

// ---- host launch helpers --------------------------------------------------------------------------------------------

// what the job walk refused, in the words of the entry points
inline int mt_plan_error(mdhip_ctx *ctx, const MolJobs &pl, int64_t n_atoms)
{
    MD_REQUIRE(pl.error != MOL_PLAN_RANGE, "job %d runs past the %lld atoms of a frame", pl.bad_job, (long long)n_atoms);
    MD_REQUIRE(pl.error != MOL_PLAN_RESULT, "result too large");
    return MDHIP_OK;
}

// the rule that the term lists of axis vectors and moments share: the atoms [t0, t1) of job j's list
inline int mt_terms_ascend(mdhip_ctx *ctx, int j, const int32_t *atom, long long t0, long long t1, long long len)
{
    for (long long k = t0; k < t1; ++k)
        MD_REQUIRE(atom[k] >= 1 && atom[k] < len && (k == t0 || atom[k] > atom[k - 1]),
                   "job %d: the terms' atoms must ascend strictly within [1, job_len)", j);
    return MDHIP_OK;
}

// Where a kernel writes a result of `bytes` bytes: the caller's buffer when that is on the device, else workspace
// `slot`, from where deliver() sends it to the caller's once the kernel has run. Nothing asked for (dst == NULL):
// nowhere (dev stays null), unless `needed` says that the kernel must write it somewhere anyway — a later kernel of
// the call reads it back; that workspace copy is delivered to nobody.
struct MolOut {
    double *dev = nullptr;
    int open(mdhip_ctx *ctx, int slot, double *dst, int dst_on_device, size_t bytes_, bool needed = false)
    {
        bytes = bytes_;
        if (dst && dst_on_device) dev = dst;
        else host = dst;
        if (dev || !(dst || needed)) return MDHIP_OK;
        dev = (double *)mdhip_ws(ctx, slot, std::max<size_t>(bytes, 8));
        return dev ? MDHIP_OK : MDHIP_ENOMEM;
    }
    int deliver(CallScope &cs) const { return host ? mdhip_result(cs, host, dev, bytes, 0) : MDHIP_OK; }

private:
    double *host = nullptr;  // the caller's buffer, when the result has to be copied out to it
    size_t bytes = 0;
};

// A call's arrays on the context's device: x [F][3][A] (staged into WS_XYZ_I unless it is there), box [F][3] (host or NULL, into
// WS_BOX) and the series U [series][3][F] in WS_OUT unless the caller's buffer is on the device. U == NULL: no series.
struct MolIo {
    const double *x = nullptr, *box = nullptr;
    MolOut U;
    int open(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x_, int x_on_device, const double *box_,
             double *U_, int U_on_device, long long series)
    {
        MD_HIP(hipSetDevice(ctx->device));
        int rc;
        x = (const double *)mdhip_stage(ctx, WS_XYZ_I, x_, (size_t)n_frames * 3 * (size_t)n_atoms * 8, x_on_device, &rc);
        if (rc) return rc;
        if (box_) {
            MD_WS(d_b, double, WS_BOX, (size_t)n_frames * 3 * 8);
            if ((rc = mdhip_h2d_small(ctx, d_b, box_, (size_t)n_frames * 3 * 8))) return rc;
            box = d_b;
        }
        return U.open(ctx, WS_OUT, U_, U_on_device, (size_t)series * 3 * (size_t)n_frames * 8);
    }
};

// launch(grid, t0, ft0) for every piece of the tiles x frame tiles grid — launch dimensions stay within 65 535, so more
// tiles go in several launches — under `timer`; their number and `kernel` become the call's last_launches / last_kernel.
template <class Launch>
inline int mt_launch(mdhip_ctx *ctx, const char *kernel, KernelTimer &timer, long long tiles, int64_t n_frames, Launch launch)
{
    const long long f_tiles = (n_frames + MT_TF - 1) / MT_TF;
    int launches = 0;
    for (long long t0 = 0; t0 < tiles; t0 += MT_MAX_GRID)
        for (long long ft0 = 0; ft0 < f_tiles; ft0 += MT_MAX_GRID, ++launches) {
            launch(dim3((unsigned)std::min(MT_MAX_GRID, tiles - t0), (unsigned)std::min(MT_MAX_GRID, f_tiles - ft0)), t0, ft0);
            MD_HIP(hipGetLastError());
        }
    ctx->last_kernel = kernel;
    ctx->last_launches = launches;
    timer.stop();
    return MDHIP_OK;
}

// launch(grid, f0, j0) for every piece of the frames x jobs grid of a totals kernel (block (x, y): frame f0 + x, job
// j0 + y): frames in slices of 2^20 along x, jobs in slices of 65535 along y. Returns the number of launches, or the
// (negative) code of the launch that failed.
constexpr long long MT_TOTALS_MAX_X = 1 << 20;
constexpr int MT_TOTALS_MAX_Y = 65535;
template <class Launch>
inline int mt_launch_totals(mdhip_ctx *ctx, int64_t n_frames, int n_jobs, Launch launch)
{
    int launches = 0;
    for (long long f0 = 0; f0 < n_frames; f0 += MT_TOTALS_MAX_X)
        for (int j0 = 0; j0 < n_jobs; j0 += MT_TOTALS_MAX_Y, ++launches) {
            launch(dim3((unsigned)std::min<long long>(MT_TOTALS_MAX_X, n_frames - f0), (unsigned)std::min(MT_TOTALS_MAX_Y, n_jobs - j0)),
                   f0, j0);
            MD_HIP(hipGetLastError());
        }
    return launches;
}

}  // namespace
#endif  // __HIPCC__
