// shell_search.h — the per-centre shell search and what its eight consumers do around it. For each centre atom of each
// frame, the sweep hands every candidate point within r_cut under the reference's single-wrap rsq (rdf_cn.py:44-57) to
// a functor. All eight check and stage their inputs with stage and end their entry points with finish; all but sdf.hip
// run the sweep itself. The first three include this header alone; the other five, whose candidates are a list of the
// caller's, include shell_gather.h (which includes this one) and take from it the packed integer tables (IntTable,
// upload_ints), the candidate planes (planes_room, gather) and, where named below, shares_an_atom, excluded, cand_xyz:
//   clusters.hip        every atom a candidate; capped rows of molecules (append, RowSet); rank_row puts them in order
//   configurations.hip  every atom a candidate; capped rows of (molecule, word) records; row_of in its hit,
//                       rank_row_keyed
//   hydration.hip       the water O (check_indices) as candidates, gathered by its own hy_water_kernel (six planes,
//                       with a derived vector); wrap_signed for the cosines; capped rows, row_of and rank_row in its
//                       row pass; its counts mode keeps no rows (plain counters)
//   angles.hip          capped rows; wrap_signed; row_of in its pair pass; shares_an_atom, excluded and cand_xyz in
//                       the search, cand_xyz in the pair pass; finish with the search's aux timer
//   bond_order.hip      capped rows; row_of, wrap_signed and rsq again in its row pass, which ranks a row by
//                       (rsq, atom) itself; shares_an_atom and excluded in the search, cand_xyz in the row pass; finish
//                       with the search's aux timer
//   sdf.hip             a sweep of its own on this header's tile and chunk decomposition (Grid, sweep_grid, rsq,
//                       wrap_signed): hits go through a queue in LDS, and the self / same-molecule test reads the
//                       centres' molecules from LDS, so it keeps its own form of `excluded`; shares_an_atom; no rows
//   aggregates.hip      no rows (a union-find per frame); the hit is tested by node, not by atom or molecule; cand_xyz
//                       for the class pair's own cutoff; its node tables are generated segments of the IntTable
//   hbonds.hip          no rows (counters, or presence_table.h); excluded and cand_xyz in hb_walk
// The reference's arithmetic is unfused: an including .hip puts `#pragma clang fp contract(off)` AHEAD of this include
// (it has to be in force where wrap_abs / wrap_signed / rsq are instantiated). residence.hip (rt_wrap_abs) and
// pair_common.h (wrap_abs) keep copies of the wrap: the committed counter runs are tied to those files byte for byte.
#pragma once

#include <algorithm>

#include "ctx.h"

namespace shell {

constexpr int THREADS = 256;
constexpr int TC = 16;          // centres per block
constexpr int CHUNK = 4096;     // candidates per block (16 per lane)
constexpr int MAX_CAP = 16384;  // the row pass stages a row in LDS (64 KB)

// |d - sign(d) L| when d > L/2 or d < -L/2, else |d| (rdf_cn.py:50-55), as a = |d|; min(a, |a - L|): the same double.
// |d - sign(d) L| == ||d| - L| (rounding is sign-symmetric); for a > L/2 the real |a - L| < a and for a <= L/2 it is
// >= a, rounding to nearest is monotone and `a` is itself a double, so the rounded value compares against `a` the
// same way (d == +-L/2 exactly gives L/2 either way). Only the square enters rsq, so the lost sign is irrelevant.
__device__ __forceinline__ double wrap_abs(double d, double L)
{
    const double a = __builtin_fabs(d);
    return __builtin_fmin(a, __builtin_fabs(a - L));
}

// rdf_cn.py:56: dx ** 2 + dy ** 2 + dz ** 2, left to right, unfused; d = centre - candidate (only |d| enters)
__device__ __forceinline__ double rsq(double cx, double cy, double cz, double x, double y, double z, double Lx,
                                      double Ly, double Lz)
{
    const double ax = wrap_abs(cx - x, Lx);
    const double ay = wrap_abs(cy - y, Ly);
    const double az = wrap_abs(cz - z, Lz);
    return (ax * ax + ay * ay) + az * az;
}

// the signed wrap itself (a cosine needs the direction): d - sign(d) L when d > L/2 or d < -L/2
__device__ __forceinline__ double wrap_signed(double d, double L)
{
    const double h = 0.5 * L;
    return d > h ? d - L : (d < -h ? d + L : d);
}

// A row: centre c (atom ci) of frame f, with the frame's three coordinate planes [n], its box edges and the centre's
// coordinates. Plain pointers and doubles: it lives in registers and is never handed to a call that is not inlined.
struct Row {
    long long f;
    int c, ci;
    const double *px, *py, *pz;
    double Lx, Ly, Lz, cx, cy, cz;
};

__device__ __forceinline__ Row row_of(const double *__restrict__ xyz, long long n, const double *__restrict__ box,
                                      const int *__restrict__ centres, long long f, int c)
{
    Row r;
    r.f = f, r.c = c, r.ci = centres[c];
    r.px = xyz + (size_t)f * 3 * (size_t)n, r.py = r.px + n, r.pz = r.py + n;
    r.Lx = box[3 * f], r.Ly = box[3 * f + 1], r.Lz = box[3 * f + 2];
    r.cx = r.px[r.ci], r.cy = r.py[r.ci], r.cz = r.pz[r.ci];
    return r;
}

// The capped append: v goes to the next slot of idx[row][cap]. Returns the slot, or -1 when the row is full: count[row]
// stays exact past `cap` (every hit adds to it), which is how the host learns that a row overflowed and by how much, and
// runs it again with a larger cap.
__device__ __forceinline__ int append(int *__restrict__ count, int *__restrict__ idx, size_t row, int cap, int v)
{
    const int slot = atomicAdd(&count[row], 1);
    if (slot >= cap) return -1;
    idx[row * (size_t)cap + (size_t)slot] = v;
    return slot;
}

// the sweep's steps (host: sweep_grid) and the blocks that share them
struct Grid {
    long long n_tiles, n_chunks, n_blocks;
    unsigned grid;
};

// The sweep of a whole block: one step per (frame, tile of TC centres, chunk of CHUNK candidates), grid-stride over a
// flattened block index (no launch dimension grows with the frames). Centres: atoms centres[0 .. n_c) of the planes
// xyz[f][3][n]; candidates: the first three of the planes cand[f][cand_planes][n_cand]. The tile's centre coordinates
// are wave-uniform loads; the lanes walk the chunk on coalesced planes and test each candidate against every centre
// of the tile, strictly rsq < rc2. Per hit (rare): hit(the centre's Row, row = f * n_c + centre, candidate).
template <class Hit>
__device__ __forceinline__ void sweep(const double *__restrict__ xyz, long long n, const int *__restrict__ centres,
                                      int n_c, const double *__restrict__ cand, int cand_planes, long long n_cand,
                                      const double *__restrict__ box, double rc2, const Grid &g, Hit hit)
{
    for (long long blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const long long chunk = blk % g.n_chunks, rest = blk / g.n_chunks;
        const long long tile = rest % g.n_tiles, f = rest / g.n_tiles;
        const int c0 = (int)tile * TC;
        const int nc = n_c - c0 < TC ? n_c - c0 : TC;
        const Row r0 = row_of(xyz, n, box, centres, f, c0);  // (the frame's planes and box; centre k = 0)
        const double *qx = cand + (size_t)f * (size_t)cand_planes * (size_t)n_cand, *qy = qx + n_cand,
                     *qz = qy + n_cand;
        double cx[TC], cy[TC], cz[TC];
#pragma unroll
        for (int k = 0; k < TC; ++k) {
            const int ci = centres[k < nc ? c0 + k : c0];  // (a short last tile repeats its first centre; hits masked)
            cx[k] = r0.px[ci];
            cy[k] = r0.py[ci];
            cz[k] = r0.pz[ci];
        }
        const long long a_end = (chunk + 1) * CHUNK < n_cand ? (chunk + 1) * CHUNK : n_cand;
        for (long long a = chunk * CHUNK + threadIdx.x; a < a_end; a += THREADS) {
            const double x = qx[a], y = qy[a], z = qz[a];
            unsigned hits = 0;
#pragma unroll
            for (int k = 0; k < TC; ++k)
                if (rsq(cx[k], cy[k], cz[k], x, y, z, r0.Lx, r0.Ly, r0.Lz) < rc2) hits |= 1u << k;
            hits &= (nc >= 32 ? ~0u : (1u << nc) - 1u);
            while (__builtin_expect(hits != 0, 0)) {  // (rare: a few candidates per centre in a whole frame)
                const int k = __builtin_ctz(hits);
                hits &= hits - 1u;
                hit(row_of(xyz, n, box, centres, f, c0 + k), (size_t)f * (size_t)n_c + (size_t)(c0 + k), a);
            }
        }
    }
}

// The row pass of one wave: the n = min(count, cap) distinct ints of r[] are staged in LDS (the launch's dynamic LDS:
// cap ints) and each is ranked; emit(rank, value) for every value, then pad(i) for i in [n, cap).
template <class Emit, class Pad>
__device__ __forceinline__ void rank_row(const int *r, int count, int cap, Emit emit, Pad pad)
{
    extern __shared__ int s_row[];
    const int lane = threadIdx.x, n = count < cap ? count : cap;
    __syncthreads();  // (the previous row's ranks have read s_row)
    for (int i = lane; i < n; i += 64) s_row[i] = r[i];
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const int v = s_row[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += s_row[j] < v;
        emit(rank, v);
    }
    for (int i = n + lane; i < cap; i += 64) pad(i);
}

// The keyed sibling of rank_row, for rows of (molecule, 64-bit word) records ranked by (type, word, molecule): the
// n = min(count, cap) records load(i) -> (type, molecule, word) are staged in LDS (the launch's dynamic LDS: cap
// records of 16 bytes, {word, type << 32 | molecule}) and each is ranked; the molecules are distinct and not negative,
// so the keys are distinct. emit(rank, molecule, word) for every record, then pad(i) for i in [n, cap).
constexpr int MAX_KEYED_CAP = 4096;  // 64 KB of LDS

template <class Load, class Emit, class Pad>
__device__ __forceinline__ void rank_row_keyed(int count, int cap, Load load, Emit emit, Pad pad)
{
    extern __shared__ unsigned long long s_keyed[];
    const int lane = threadIdx.x, n = count < cap ? count : cap;
    __syncthreads();  // (the previous row's ranks have read s_keyed)
    for (int i = lane; i < n; i += 64) {
        int type, mol;
        unsigned long long word;
        load(i, type, mol, word);
        s_keyed[2 * i] = word;
        s_keyed[2 * i + 1] = ((unsigned long long)(unsigned)type << 32) | (unsigned)mol;
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const unsigned long long w = s_keyed[2 * i], tm = s_keyed[2 * i + 1];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned long long wj = s_keyed[2 * j], tmj = s_keyed[2 * j + 1];
            const unsigned tj = (unsigned)(tmj >> 32), t = (unsigned)(tm >> 32);
            rank += tj != t ? tj < t : (wj != w ? wj < w : tmj < tm);
        }
        emit(rank, (int)(unsigned)tm, w);
    }
    for (int i = n + lane; i < cap; i += 64) pad(i);
}

struct Inputs {  // on the device
    const double *xyz = nullptr, *box = nullptr;
    const int *centres = nullptr;
};

// A table of atom indices from the caller: entry k names the atoms idx[k] .. idx[k] + span - 1.
inline int check_indices(mdhip_ctx *ctx, const char *noun, int32_t n, const int32_t *idx, int span, int64_t n_atoms)
{
    for (int32_t k = 0; k < n; ++k) {
        const bool ok = idx[k] >= 0 && (int64_t)idx[k] + span - 1 < n_atoms;
        if (span > 1)
            MD_REQUIRE(ok, "%s %d: atoms %d..%d out of range", noun, (int)k, (int)idx[k], (int)idx[k] + span - 1);
        MD_REQUIRE(ok, "%s %d: atom index %d out of range", noun, (int)k, (int)idx[k]);
    }
    return MDHIP_OK;
}

// What every entry point checks and stages (no launch); `noun` names a centre in the error texts.
inline int stage(mdhip_ctx *ctx, const char *noun, int64_t n_frames, int64_t n_atoms, const double *xyz,
                 int xyz_on_device, const double *box, int32_t n_centres, const int32_t *centres, Inputs &in)
{
    MD_REQUIRE(n_atoms > 0, "%ss without atoms", noun);
    MD_REQUIRE(xyz && box && centres, "NULL array");
    MD_REQUIRE(n_atoms < (1ll << 31), "at most 2^31 - 1 atoms");
    int rc;
    if ((rc = check_indices(ctx, noun, n_centres, centres, 1, n_atoms))) return rc;
    MD_HIP(hipSetDevice(ctx->device));
    in.xyz = (const double *)mdhip_stage(ctx, WS_XYZ_I, xyz, (size_t)n_frames * 3 * (size_t)n_atoms * 8,
                                         xyz_on_device, &rc);
    if (rc) return rc;
    MD_WS(d_box, double, WS_BOX, (size_t)n_frames * 3 * 8);
    if ((rc = mdhip_h2d_small(ctx, d_box, box, (size_t)n_frames * 3 * 8))) return rc;
    MD_WS(d_cen, int, WS_TYPE_I, (size_t)n_centres * 4);
    in.box = d_box;
    in.centres = d_cen;
    return mdhip_h2d_small(ctx, d_cen, centres, (size_t)n_centres * 4);
}

inline Grid sweep_grid(const mdhip_ctx *ctx, int64_t n_frames, int32_t n_centres, int64_t n_cand)
{
    const long long n_tiles = (n_centres + TC - 1) / TC, n_chunks = (n_cand + CHUNK - 1) / CHUNK;
    const long long n_blocks = (long long)n_frames * n_tiles * n_chunks;
    return {n_tiles, n_chunks, n_blocks, (unsigned)std::min<long long>(n_blocks, (long long)ctx->cu_count * 64)};
}

// The rows of a capped call on the device: count [n_rows] (WS_AUX0), zeroed, and the row buffer idx [n_rows][cap]
// (WS_OUT).
struct RowSet {
    size_t n_rows = 0;
    int cap = 0;
    int *count = nullptr, *idx = nullptr;
    // blocks of a row pass: one row at a time each, `per_cu` of them on a CU
    unsigned grid(const mdhip_ctx *ctx, int per_cu) const { return (unsigned)std::min(n_rows, (size_t)ctx->cu_count * per_cu); }
};

// Checks `cap` against the caller's limit (`why`: what the limit is for, appended to the error text) and takes the
// buffers; a call without rows takes none.
inline int take_rows(mdhip_ctx *ctx, int64_t n_frames, int32_t n_centres, int32_t cap, int max_cap, RowSet &rs,
                     const char *why = "")
{
    MD_REQUIRE(cap >= 1 && cap <= max_cap, "cap must be in [1, %d]%s", max_cap, why);
    rs.n_rows = (size_t)n_frames * (size_t)n_centres;
    rs.cap = (int)cap;
    if (rs.n_rows == 0) return MDHIP_OK;
    MD_HIP(hipSetDevice(ctx->device));
    MD_WS(d_count, int, WS_AUX0, rs.n_rows * 4);
    MD_WS(d_idx, int, WS_OUT, rs.n_rows * (size_t)cap * 4);
    MD_HIP(hipMemsetAsync(d_count, 0, rs.n_rows * 4, ctx->stream));
    rs.count = d_count;
    rs.idx = d_idx;
    return MDHIP_OK;
}

// Queues the rows' results: idx (unless the caller has no use for the rows themselves: nullptr) and count.
inline int row_results(CallScope &cs, const RowSet &rs, int32_t *idx, int32_t *count)
{
    int rc;
    if (idx && (rc = mdhip_result(cs, idx, rs.idx, rs.n_rows * (size_t)rs.cap * 4, 0))) return rc;
    return mdhip_result(cs, count, rs.count, rs.n_rows * 4, 0);
}

// The end of an entry point whose launches ran under `timer` (and some of them under `aux`, whose time becomes the
// call's aux time): the times are read when the call completes.
inline int finish(CallScope &cs, const KernelTimer &timer, const KernelTimer *aux = nullptr)
{
    if (aux) cs.defer([a = *aux]() { return a.ctx->last_aux_ms = a.collect(), MDHIP_OK; });
    return mdhip_end_timed(cs, timer);
}

}  // namespace shell
