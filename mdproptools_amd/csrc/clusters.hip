// clusters.hip — solvation-shell search and per-molecule force sums for cluster extraction.
//
// Replaces the per-centre pair work of structural/cluster_analysis.py:47-235 of the reference (get_clusters): for each
// centre atom of each frame, the molecules that have an atom within r_cut (cluster_analysis.py:127-142), and the
// per-molecule force sums the cluster filter thresholds (cluster_analysis.py:146-152). Everything else a cluster needs
// (row order, the force filter, the boundary shift, the text) is per-cluster bookkeeping on the host
// (mdproptools_amd/structural/cluster_analysis.py).
//
//  1. shell_hits_kernel: one block per (frame, tile of SH_TC centres, chunk of SH_CHUNK atoms), grid-stride over a
//     flattened block index (no launch dimension grows with the frames). The tile's centre coordinates are
//     wave-uniform loads; the lanes walk the chunk's atoms on coalesced planes and test each against every centre of
//     the tile with the reference's single-wrap rsq (rdf_cn.py:44-57, contraction off). A hit is rare. It is counted
//     for its molecule only when it is the molecule's FIRST hit in id order: the atoms before it in the same molecule
//     (molecules are contiguous id ranges) are tested again, and any earlier hit means another lane counts the
//     molecule. So every shell molecule is appended exactly once — count[f][c] is the true number of shell molecules
//     even when it exceeds the row's capacity `cap` (the host then re-runs those frames with a larger one).
//  2. shell_sort_kernel: one wave per (frame, centre) row puts the row's molecule indices in ascending order (a rank
//     sort through LDS: the values are distinct) and pads the row to `cap` with -1.
//  3. mol_kahan_kernel: one lane per (frame, attribute, molecule), the compensated sum of pandas' groupby().sum() over
//     the molecule's atoms in id order.

#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_TC = 16;       // centres per block
constexpr int SH_CHUNK = 4096;  // atoms per block (16 per lane)
constexpr int SH_MAX_CAP = 16384;  // the sort stages a row in LDS (64 KB)

__device__ __forceinline__ double sh_wrap_abs(double d, double L)
{
    // |d - copysign(L, d)| when d > L/2 or d < -L/2, else |d| (rdf_cn.py:50-55), as min(|d|, ||d| - L|): the same
    // double — see residence.hip / pair_hist.hip for the equivalence (d == +-L/2 exactly gives L/2 either way)
    const double a = __builtin_fabs(d);
    return __builtin_fmin(a, __builtin_fabs(a - L));
}

// rdf_cn.py:56: dx ** 2 + dy ** 2 + dz ** 2, left to right, unfused; d = centre - atom (only |d| enters)
__device__ __forceinline__ double sh_rsq(double cx, double cy, double cz, double x, double y, double z, double Lx,
                                         double Ly, double Lz)
{
    const double ax = sh_wrap_abs(cx - x, Lx);
    const double ay = sh_wrap_abs(cy - y, Ly);
    const double az = sh_wrap_abs(cz - z, Lz);
    return (ax * ax + ay * ay) + az * az;
}

// Atom a of frame plane p* is within the cutoff of centre row `row` (coordinates c*): append its molecule unless an
// atom before it in the same molecule is within the cutoff too (that atom's lane appends it).
__device__ __noinline__ void sh_hit(const double *__restrict__ px, const double *__restrict__ py,
                                    const double *__restrict__ pz, const int *__restrict__ mol_of, long long a,
                                    double cx, double cy, double cz, double Lx, double Ly, double Lz, double rc2,
                                    int cap, size_t row, int *__restrict__ mols, int *__restrict__ count)
{
    const int m = mol_of[a];
    for (long long b = a - 1; b >= 0 && mol_of[b] == m; --b)
        if (sh_rsq(cx, cy, cz, px[b], py[b], pz[b], Lx, Ly, Lz) < rc2) return;
    const int slot = atomicAdd(&count[row], 1);
    if (slot < cap) mols[row * (size_t)cap + (size_t)slot] = m;
}

__global__ __launch_bounds__(SH_THREADS) void shell_hits_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ box, const int *__restrict__ centres,
    int n_c, const int *__restrict__ mol_of, double rc2, int cap, long long n_tiles, long long n_chunks,
    long long n_blocks, int *__restrict__ mols, int *__restrict__ count)
{
    for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const long long chunk = blk % n_chunks, rest = blk / n_chunks;
        const long long tile = rest % n_tiles, f = rest / n_tiles;
        const double *px = xyz + (size_t)f * 3 * (size_t)n, *py = px + n, *pz = py + n;
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const int c0 = (int)tile * SH_TC;
        const int nc = n_c - c0 < SH_TC ? n_c - c0 : SH_TC;
        double cx[SH_TC], cy[SH_TC], cz[SH_TC];
#pragma unroll
        for (int k = 0; k < SH_TC; ++k) {
            const int ci = centres[k < nc ? c0 + k : c0];  // (a short last tile repeats its first centre; hits masked)
            cx[k] = px[ci];
            cy[k] = py[ci];
            cz[k] = pz[ci];
        }
        const long long a_end = (chunk + 1) * SH_CHUNK < n ? (chunk + 1) * SH_CHUNK : n;
        for (long long a = chunk * SH_CHUNK + threadIdx.x; a < a_end; a += SH_THREADS) {
            const double x = px[a], y = py[a], z = pz[a];
            unsigned hits = 0;
#pragma unroll
            for (int k = 0; k < SH_TC; ++k)
                if (sh_rsq(cx[k], cy[k], cz[k], x, y, z, Lx, Ly, Lz) < rc2) hits |= 1u << k;
            hits &= (nc >= 32 ? ~0u : (1u << nc) - 1u);
            while (hits) {  // (rare: a few atoms per centre in a whole frame)
                const int k = __builtin_ctz(hits);
                hits &= hits - 1u;
                const int ci = centres[c0 + k];
                sh_hit(px, py, pz, mol_of, a, px[ci], py[ci], pz[ci], Lx, Ly, Lz, rc2, cap,
                       (size_t)f * (size_t)n_c + (size_t)(c0 + k), mols, count);
            }
        }
    }
}

// One wave per row; LDS: the row [cap] (int).
__global__ __launch_bounds__(64) void shell_sort_kernel(int *__restrict__ mols, const int *__restrict__ count,
                                                        long long n_rows, int cap)
{
    extern __shared__ int s_row[];
    const int lane = threadIdx.x;
    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        int *r = mols + (size_t)row * (size_t)cap;
        const int n = count[row] < cap ? count[row] : cap;
        __syncthreads();  // (the previous row's ranks have read s_row)
        for (int i = lane; i < n; i += 64) s_row[i] = r[i];
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            const int v = s_row[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += s_row[j] < v;
            r[rank] = v;
        }
        for (int i = n + lane; i < cap; i += 64) r[i] = -1;
    }
}

// out[f][k][m] = the compensated sum of attr[f][k][seg_off[m] .. seg_off[m+1]) in ascending order — pandas'
// group_sum (y = v - c; t = s + y; c = (t - s) - y; s = t; a NaN compensation is reset to 0), contraction off.
__global__ __launch_bounds__(256) void mol_kahan_kernel(const double *__restrict__ attr, long long n,
                                                        const long long *__restrict__ seg_off, long long n_mols,
                                                        long long total, double *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long m = i % n_mols, fk = i / n_mols;
        const double *p = attr + (size_t)fk * (size_t)n;
        double s = 0.0, c = 0.0;
        for (long long a = seg_off[m]; a < seg_off[m + 1]; ++a) {
            const double y = p[a] - c;
            const double t = s + y;
            c = (t - s) - y;
            if (c != c) c = 0.0;
            s = t;
        }
        out[i] = s;
    }
}

}  // namespace

extern "C" {

int mdhip_shell_members(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                        const double *box, int32_t n_centres, const int32_t *centres, const int32_t *mol_of,
                        double r_cut_sq, int32_t cap, int32_t *mols, int32_t *count)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_centres >= 0, "negative sizes");
    MD_REQUIRE(cap >= 1 && cap <= SH_MAX_CAP, "cap must be in [1, %d]", SH_MAX_CAP);
    if (n_frames == 0 || n_centres == 0) return cs.end();
    MD_REQUIRE(n_atoms > 0, "centres without atoms");
    MD_REQUIRE(xyz && box && centres && mol_of && mols && count, "NULL array");
    MD_REQUIRE(n_atoms < (1ll << 31), "at most 2^31 - 1 atoms");
    for (int32_t c = 0; c < n_centres; ++c)
        MD_REQUIRE(centres[c] >= 0 && centres[c] < n_atoms, "centre %d: atom index %d out of range", (int)c,
                   (int)centres[c]);
    const size_t n_rows = (size_t)n_frames * (size_t)n_centres;
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const double *d_xyz =
        (const double *)mdhip_stage(ctx, WS_XYZ_I, xyz, (size_t)n_frames * 3 * (size_t)n_atoms * 8, xyz_on_device, &rc);
    if (rc) return rc;
    MD_WS(d_box, double, WS_BOX, (size_t)n_frames * 3 * 8);
    if ((rc = mdhip_h2d_small(ctx, d_box, box, (size_t)n_frames * 3 * 8))) return rc;
    MD_WS(d_cen, int, WS_TYPE_I, (size_t)n_centres * 4);
    if ((rc = mdhip_h2d_small(ctx, d_cen, centres, (size_t)n_centres * 4))) return rc;
    MD_WS(d_mol, int, WS_TYPE_J, (size_t)n_atoms * 4);
    if ((rc = mdhip_h2d_small(ctx, d_mol, mol_of, (size_t)n_atoms * 4))) return rc;
    MD_WS(d_count, int, WS_AUX0, n_rows * 4);
    MD_WS(d_mols, int, WS_OUT, n_rows * (size_t)cap * 4);
    MD_HIP(hipMemsetAsync(d_count, 0, n_rows * 4, ctx->stream));

    const long long n_tiles = (n_centres + SH_TC - 1) / SH_TC, n_chunks = (n_atoms + SH_CHUNK - 1) / SH_CHUNK;
    const long long n_blocks = (long long)n_frames * n_tiles * n_chunks;
    const unsigned grid = (unsigned)std::min<long long>(n_blocks, (long long)ctx->cu_count * 64);
    KernelTimer timer(ctx, 2);
    ctx->last_kernel = "shell_hits_kernel";
    hipLaunchKernelGGL(shell_hits_kernel, dim3(grid), dim3(SH_THREADS), 0, ctx->stream, d_xyz, (long long)n_atoms,
                       d_box, d_cen, (int)n_centres, d_mol, r_cut_sq, (int)cap, n_tiles, n_chunks, n_blocks, d_mols,
                       d_count);
    MD_HIP(hipGetLastError());
    const unsigned sort_grid = (unsigned)std::min<size_t>(n_rows, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(shell_sort_kernel, dim3(sort_grid), dim3(64), (size_t)cap * 4, ctx->stream, d_mols, d_count,
                       (long long)n_rows, (int)cap);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, mols, d_mols, n_rows * (size_t)cap * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, count, d_count, n_rows * 4, 0))) return rc;
    cs.defer([timer]() {
        timer.collect();
        return MDHIP_OK;
    });
    return cs.end();
}

int mdhip_mol_kahan_sums(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, int n_attr, const double *attr,
                         int attr_on_device, int64_t n_mols, const int64_t *seg_off, double *out)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_attr >= 0 && n_mols >= 0, "negative sizes");
    const size_t total = (size_t)n_frames * (size_t)n_attr * (size_t)n_mols;
    if (total == 0) return cs.end();
    MD_REQUIRE(attr && seg_off && out, "NULL array");
    MD_REQUIRE(seg_off[0] >= 0 && seg_off[n_mols] <= n_atoms, "segments outside [0, n_atoms)");
    for (int64_t m = 0; m < n_mols; ++m) MD_REQUIRE(seg_off[m] <= seg_off[m + 1], "segment %lld is negative", (long long)m);
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const double *d_attr = (const double *)mdhip_stage(ctx, WS_XYZ_I, attr,
                                                       (size_t)n_frames * (size_t)n_attr * (size_t)n_atoms * 8,
                                                       attr_on_device, &rc);
    if (rc) return rc;
    MD_WS(d_off, long long, WS_TABLES, ((size_t)n_mols + 1) * 8);
    if ((rc = mdhip_h2d_small(ctx, d_off, seg_off, ((size_t)n_mols + 1) * 8))) return rc;
    MD_WS(d_out, double, WS_OUT, total * 8);
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)ctx->cu_count * 32);
    KernelTimer timer(ctx);
    ctx->last_kernel = "mol_kahan_kernel";
    hipLaunchKernelGGL(mol_kahan_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_attr, (long long)n_atoms, d_off,
                       (long long)n_mols, (long long)total, d_out);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, out, d_out, total * 8, 0))) return rc;
    cs.defer([timer]() {
        timer.collect();
        return MDHIP_OK;
    });
    return cs.end();
}

}  // extern "C"
