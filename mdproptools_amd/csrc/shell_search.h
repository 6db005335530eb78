// shell_search.h — the per-centre shell search that clusters.hip and hydration.hip share: for each centre atom of each
// frame, every candidate point within r_cut under the reference's single-wrap rsq (rdf_cn.py:44-57), handed to a
// functor; and the row pass that puts what a row collected in ascending order.
// The reference's arithmetic is unfused: an including .hip puts `#pragma clang fp contract(off)` AHEAD of this include
// (it has to be in force where wrap_abs / rsq are instantiated). residence.hip (rt_wrap_abs) and pair_common.h
// (wrap_abs) keep copies of the wrap: the committed counter runs are tied to those files byte for byte.
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

// the sweep's steps (host: sweep_grid) and the blocks that share them
struct Grid {
    long long n_tiles, n_chunks, n_blocks;
    unsigned grid;
};

// The sweep of a whole block: one step per (frame, tile of TC centres, chunk of CHUNK candidates), grid-stride over a
// flattened block index (no launch dimension grows with the frames). Centres: atoms centres[0 .. n_c) of the planes
// xyz[f][3][n]; candidates: the first three of the planes cand[f][cand_planes][n_cand]. The tile's centre coordinates
// are wave-uniform loads; the lanes walk the chunk on coalesced planes and test each candidate against every centre
// of the tile, strictly rsq < rc2. Per hit (rare): hit(f, row = f * n_c + centre, candidate, cx, cy, cz, Lx, Ly, Lz).
template <class Hit>
__device__ __forceinline__ void sweep(const double *__restrict__ xyz, long long n, const int *__restrict__ centres,
                                      int n_c, const double *__restrict__ cand, int cand_planes, long long n_cand,
                                      const double *__restrict__ box, double rc2, const Grid &g, Hit hit)
{
    for (long long blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const long long chunk = blk % g.n_chunks, rest = blk / g.n_chunks;
        const long long tile = rest % g.n_tiles, f = rest / g.n_tiles;
        const double *px = xyz + (size_t)f * 3 * (size_t)n, *py = px + n, *pz = py + n;
        const double *qx = cand + (size_t)f * (size_t)cand_planes * (size_t)n_cand, *qy = qx + n_cand,
                     *qz = qy + n_cand;
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const int c0 = (int)tile * TC;
        const int nc = n_c - c0 < TC ? n_c - c0 : TC;
        double cx[TC], cy[TC], cz[TC];
#pragma unroll
        for (int k = 0; k < TC; ++k) {
            const int ci = centres[k < nc ? c0 + k : c0];  // (a short last tile repeats its first centre; hits masked)
            cx[k] = px[ci];
            cy[k] = py[ci];
            cz[k] = pz[ci];
        }
        const long long a_end = (chunk + 1) * CHUNK < n_cand ? (chunk + 1) * CHUNK : n_cand;
        for (long long a = chunk * CHUNK + threadIdx.x; a < a_end; a += THREADS) {
            const double x = qx[a], y = qy[a], z = qz[a];
            unsigned hits = 0;
#pragma unroll
            for (int k = 0; k < TC; ++k)
                if (rsq(cx[k], cy[k], cz[k], x, y, z, Lx, Ly, Lz) < rc2) hits |= 1u << k;
            hits &= (nc >= 32 ? ~0u : (1u << nc) - 1u);
            while (__builtin_expect(hits != 0, 0)) {  // (rare: a few candidates per centre in a whole frame)
                const int k = __builtin_ctz(hits);
                hits &= hits - 1u;
                const int ci = centres[c0 + k];
                hit(f, (size_t)f * (size_t)n_c + (size_t)(c0 + k), a, px[ci], py[ci], pz[ci], Lx, Ly, Lz);
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

// What every entry point checks and stages (no launch); `noun` names a centre in the error texts.
inline int stage(mdhip_ctx *ctx, const char *noun, int64_t n_frames, int64_t n_atoms, const double *xyz,
                 int xyz_on_device, const double *box, int32_t n_centres, const int32_t *centres, Inputs &in)
{
    MD_REQUIRE(n_atoms > 0, "%ss without atoms", noun);
    MD_REQUIRE(xyz && box && centres, "NULL array");
    MD_REQUIRE(n_atoms < (1ll << 31), "at most 2^31 - 1 atoms");
    for (int32_t c = 0; c < n_centres; ++c)
        MD_REQUIRE(centres[c] >= 0 && centres[c] < n_atoms, "%s %d: atom index %d out of range", noun, (int)c,
                   (int)centres[c]);
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
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

// The end of an entry point whose launches ran under `timer`: the time is read when the call completes.
inline int finish(CallScope &cs, const KernelTimer &timer)
{
    cs.defer([timer]() {
        timer.collect();
        return MDHIP_OK;
    });
    return cs.end();
}

}  // namespace shell
