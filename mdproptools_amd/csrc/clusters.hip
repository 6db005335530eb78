// clusters.hip — solvation-shell search and per-molecule force sums for cluster extraction.
//
// Replaces the per-centre pair work of structural/cluster_analysis.py:47-235 of the reference (get_clusters): for each
// centre atom of each frame, the molecules that have an atom within r_cut (cluster_analysis.py:127-142), and the
// per-molecule force sums the cluster filter thresholds (cluster_analysis.py:146-152). Everything else a cluster needs
// (row order, the force filter, the boundary shift, the text) is per-cluster bookkeeping on the host
// (mdproptools_amd/structural/cluster_analysis.py).
//
//  1. shell_hits_kernel: the sweep of shell_search.h, every centre against every atom of its frame. A hit is counted
//     for its molecule only when it is the molecule's FIRST hit in id order: the atoms before it in the same molecule
//     (molecules are contiguous id ranges) are tested again, and any earlier hit means another lane counts the
//     molecule. So every shell molecule is appended (shell::append) exactly once: count[f][c] is the number of shell
//     molecules.
//  2. shell_sort_kernel: one wave per (frame, centre) row puts the row's molecule indices in ascending order (the row
//     pass of shell_search.h: the values are distinct) and pads the row to `cap` with -1.
//  3. mol_kahan_kernel: one lane per (frame, attribute, molecule), the compensated sum of pandas' groupby().sum() over
//     the molecule's atoms in id order.

#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_search.h"

namespace {

// Atom a of frame plane p* is within the cutoff of centre row `row` (coordinates c*): append its molecule unless an
// atom before it in the same molecule is within the cutoff too (that atom's lane appends it).
__device__ __noinline__ void sh_hit(const double *__restrict__ px, const double *__restrict__ py,
                                    const double *__restrict__ pz, const int *__restrict__ mol_of, long long a,
                                    double cx, double cy, double cz, double Lx, double Ly, double Lz, double rc2,
                                    int cap, size_t row, int *__restrict__ mols, int *__restrict__ count)
{
    const int m = mol_of[a];
    for (long long b = a - 1; b >= 0 && mol_of[b] == m; --b)
        if (shell::rsq(cx, cy, cz, px[b], py[b], pz[b], Lx, Ly, Lz) < rc2) return;
    shell::append(count, mols, row, cap, m);
}

__global__ __launch_bounds__(shell::THREADS) void shell_hits_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ box, const int *__restrict__ centres,
    int n_c, const int *__restrict__ mol_of, double rc2, int cap, shell::Grid g, int *__restrict__ mols,
    int *__restrict__ count)
{
    shell::sweep(xyz, n, centres, n_c, xyz, 3, n, box, rc2, g,
                 [=](const shell::Row &r, size_t row, long long a) {
                     sh_hit(r.px, r.py, r.pz, mol_of, a, r.cx, r.cy, r.cz, r.Lx, r.Ly, r.Lz, rc2, cap, row, mols, count);
                 });
}

// One wave per row; LDS: the row [cap] (int).
__global__ __launch_bounds__(64) void shell_sort_kernel(int *__restrict__ mols, const int *__restrict__ count,
                                                        long long n_rows, int cap)
{
    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        int *r = mols + (size_t)row * (size_t)cap;
        shell::rank_row(r, count[row], cap, [&](int rank, int v) { r[rank] = v; }, [&](int i) { r[i] = -1; });
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
    shell::RowSet rs;
    int rc;
    if ((rc = shell::take_rows(ctx, n_frames, n_centres, cap, shell::MAX_CAP, rs))) return rc;
    if (rs.n_rows == 0) return cs.end();
    MD_REQUIRE(mol_of && mols && count, "NULL array");
    shell::Inputs in;
    if ((rc = shell::stage(ctx, "centre", n_frames, n_atoms, xyz, xyz_on_device, box, n_centres, centres, in)))
        return rc;
    MD_WS(d_mol, int, WS_TYPE_J, (size_t)n_atoms * 4);
    if ((rc = mdhip_h2d_small(ctx, d_mol, mol_of, (size_t)n_atoms * 4))) return rc;

    const shell::Grid g = shell::sweep_grid(ctx, n_frames, n_centres, n_atoms);
    KernelTimer timer(ctx, 2);
    ctx->last_kernel = "shell_hits_kernel";
    hipLaunchKernelGGL(shell_hits_kernel, dim3(g.grid), dim3(shell::THREADS), 0, ctx->stream, in.xyz,
                       (long long)n_atoms, in.box, in.centres, (int)n_centres, d_mol, r_cut_sq, (int)cap, g, rs.idx, rs.count);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(shell_sort_kernel, dim3(rs.grid(ctx, 32)), dim3(64), (size_t)cap * 4, ctx->stream, rs.idx, rs.count,
                       (long long)rs.n_rows, (int)cap);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = shell::row_results(cs, rs, mols, count))) return rc;
    return shell::finish(cs, timer);
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
    return shell::finish(cs, timer);
}

}  // extern "C"
