// configurations.hip — the solvation shell of every centre as (molecule, coordination word) records in one canonical
// order: the configuration census of get_unique_configurations (structural/cluster_analysis.py:238-457 of the
// reference) taken straight from the trajectory, without a Cluster_*.xyz file in between.
//
// The reference reads every cluster file back, takes the atoms within r_cut of the file's first atom and matches the
// rest of the file against the molecules' element sequences (cluster_analysis.py:341-373). Here the molecules are
// known by layout, and two radii do what the two functions of the reference do with theirs: r_shell decides which
// molecules belong to the cluster (get_clusters), r_coord which of their atoms coordinate (get_unique_configurations).
//
//  1. coord_hits_kernel: the sweep of shell_search.h at r_shell, every centre against every atom of its frame. A hit
//     is dropped when its molecule is the centre's own or fails the pass mask (the force filter's verdict, [F][M]),
//     and, as in clusters.hip, unless it is the molecule's FIRST hit in id order. The lane walks the whole molecule
//     once for both: whether an earlier atom is within r_shell too, and, per coordination class, the atoms with
//     rsq < r_coord_sq: eight 8-bit counters in one 64-bit word (a molecule has at most 255 atoms, so no counter
//     wraps). shell::append gives the record's slot.
//  2. coord_rank_kernel: one wave per (frame, centre) row puts the row's records in (molecule type, word, molecule)
//     order (the keyed row pass of shell_search.h) and pads the row with -1 / ~0. A row then has one form whatever
//     order the atomics landed in, and two rows are the same configuration exactly when their (type, word) sequences
//     are equal.

#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_search.h"

namespace {

constexpr int MAX_CLASSES = 8;       // 8-bit counters in a 64-bit word
constexpr unsigned char NO_CLASS = 0xFF;
constexpr int MAX_MOL_ATOMS = 255;   // what an 8-bit counter holds

// What the hit path reads, in device memory: the sweep's lanes carry a pointer to it, not its fields, into the
// (rare, not inlined) call, so the sweep itself keeps the registers and the occupancy of shell_hits_kernel.
struct CoordTable {
    const double *xyz, *box;
    const int *centres, *mol_of;
    const long long *seg_off;
    const unsigned char *cls, *passes;  // passes: [F][n_mols] or NULL (every molecule passes)
    long long n, n_mols;
    double r_shell_sq, r_coord_sq;
    int n_c, cap;
    int *mols, *count;
    unsigned long long *words;
};

// Atom a of frame f is within the shell radius of centre row `row`: append its molecule's record unless the molecule
// is dropped or an atom before it in the molecule is within the radius too.
__device__ __noinline__ void co_hit(const CoordTable *__restrict__ tab, long long f, size_t row, long long a)
{
    const CoordTable &t = *tab;
    const shell::Row r = shell::row_of(t.xyz, t.n, t.box, t.centres, f, (int)(row - (size_t)f * (size_t)t.n_c));
    const int m = t.mol_of[a];
    if (m == t.mol_of[r.ci]) return;
    if (t.passes && !t.passes[(size_t)f * (size_t)t.n_mols + (size_t)m]) return;
    // one walk over the molecule, every load unconditional so that the loads of several atoms are in flight together
    // (a lane is alone here, and a chain of dependent loads per atom is what the block would wait for)
    const long long b0 = t.seg_off[m], b1 = t.seg_off[m + 1];
    const double rs2 = t.r_shell_sq, rc2 = t.r_coord_sq;
    unsigned long long word = 0ull;
    bool earlier = false;
    for (long long b = b0; b < b1; ++b) {
        const unsigned c = t.cls[b];
        const double d2 = shell::rsq(r.cx, r.cy, r.cz, r.px[b], r.py[b], r.pz[b], r.Lx, r.Ly, r.Lz);
        earlier |= b < a && d2 < rs2;
        word += (c != NO_CLASS && d2 < rc2) ? 1ull << (8u * (c & 7u)) : 0ull;
    }
    if (earlier) return;  // (that atom's lane appends the molecule)
    const int slot = shell::append(t.count, t.mols, row, t.cap, m);
    if (slot >= 0) t.words[row * (size_t)t.cap + (size_t)slot] = word;
}

__global__ __launch_bounds__(shell::THREADS) void coord_hits_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ box, const int *__restrict__ centres,
    int n_c, double rs2, shell::Grid g, const CoordTable *__restrict__ tab)
{
    shell::sweep(xyz, n, centres, n_c, xyz, 3, n, box, rs2, g,
                 [=](const shell::Row &r, size_t row, long long a) { co_hit(tab, r.f, row, a); });
}

// One wave per row; LDS: the row [cap] (16-byte records).
__global__ __launch_bounds__(64) void coord_rank_kernel(int *__restrict__ mols, unsigned long long *__restrict__ words,
                                                        const int *__restrict__ count,
                                                        const int *__restrict__ mol_type, long long n_rows, int cap)
{
    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        int *r = mols + (size_t)row * (size_t)cap;
        unsigned long long *w = words + (size_t)row * (size_t)cap;
        shell::rank_row_keyed(
            count[row], cap,
            [&](int i, int &type, int &mol, unsigned long long &word) {
                mol = r[i];
                word = w[i];
                type = mol_type[mol];
            },
            [&](int rank, int mol, unsigned long long word) {
                r[rank] = mol;
                w[rank] = word;
            },
            [&](int i) {
                r[i] = -1;
                w[i] = ~0ull;
            });
    }
}

}  // namespace

extern "C" {

int mdhip_shell_coordination(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                             const double *box, int32_t n_centres, const int32_t *centres, int64_t n_mols,
                             const int32_t *mol_of, const int64_t *seg_off, const int32_t *mol_type,
                             const uint8_t *cls, const uint8_t *passes, double r_shell_sq, double r_coord_sq,
                             int32_t cap, int32_t *mols, uint64_t *words, int32_t *count)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_centres >= 0 && n_mols >= 0, "negative sizes");
    shell::RowSet rs;
    int rc;
    if ((rc = shell::take_rows(ctx, n_frames, n_centres, cap, shell::MAX_KEYED_CAP, rs,
                               ": a row of more records does not fit in LDS")))
        return rc;
    if (rs.n_rows == 0) return cs.end();
    MD_REQUIRE(mol_of && seg_off && mol_type && cls && mols && words && count, "NULL array");
    // the kernels index seg_off, mol_type and passes by mol_of, and shift by the class: all of it checked here
    MD_REQUIRE(n_mols > 0 && n_mols < (1ll << 31), "the number of molecules must be in [1, 2^31)");
    MD_REQUIRE(seg_off[0] == 0 && seg_off[n_mols] == n_atoms, "the molecules must cover the atoms [0, n_atoms)");
    for (int64_t m = 0; m < n_mols; ++m) {
        MD_REQUIRE(seg_off[m] < seg_off[m + 1] && seg_off[m + 1] <= n_atoms, "molecule %lld is empty or out of range",
                   (long long)m);
        MD_REQUIRE(seg_off[m + 1] - seg_off[m] <= MAX_MOL_ATOMS, "molecule %lld has more than %d atoms", (long long)m,
                   MAX_MOL_ATOMS);
        MD_REQUIRE(mol_type[m] >= 0, "molecule %lld: negative type", (long long)m);
        for (int64_t a = seg_off[m]; a < seg_off[m + 1]; ++a)
            MD_REQUIRE(mol_of[a] == m, "atom %lld: mol_of disagrees with seg_off", (long long)a);
    }
    for (int64_t a = 0; a < n_atoms; ++a)
        MD_REQUIRE(cls[a] == NO_CLASS || cls[a] < MAX_CLASSES, "atom %lld: class %d (at most %d classes, or 255)",
                   (long long)a, (int)cls[a], MAX_CLASSES);
    shell::Inputs in;
    if ((rc = shell::stage(ctx, "centre", n_frames, n_atoms, xyz, xyz_on_device, box, n_centres, centres, in)))
        return rc;
    MD_WS(d_mol, int, WS_TYPE_J, (size_t)n_atoms * 4);
    if ((rc = mdhip_h2d_small(ctx, d_mol, mol_of, (size_t)n_atoms * 4))) return rc;
    MD_WS(d_off, long long, WS_TABLES, ((size_t)n_mols + 1) * 8);
    if ((rc = mdhip_h2d_small(ctx, d_off, seg_off, ((size_t)n_mols + 1) * 8))) return rc;
    MD_WS(d_type, int, WS_AUX1, (size_t)n_mols * 4);
    if ((rc = mdhip_h2d_small(ctx, d_type, mol_type, (size_t)n_mols * 4))) return rc;
    MD_WS(d_cls, unsigned char, WS_AUX2, (size_t)n_atoms);
    if ((rc = mdhip_h2d_small(ctx, d_cls, cls, (size_t)n_atoms))) return rc;
    unsigned char *d_pass = nullptr;
    if (passes) {
        MD_WS(d_p, unsigned char, WS_AUX3, (size_t)n_frames * (size_t)n_mols);
        if ((rc = mdhip_h2d_small(ctx, d_p, passes, (size_t)n_frames * (size_t)n_mols))) return rc;
        d_pass = d_p;
    }
    MD_WS(d_words, unsigned long long, WS_OUT2, rs.n_rows * (size_t)cap * 8);

    const shell::Grid g = shell::sweep_grid(ctx, n_frames, n_centres, n_atoms);
    const CoordTable table{in.xyz, in.box, in.centres, d_mol, d_off, d_cls, d_pass, (long long)n_atoms, (long long)n_mols,
                           r_shell_sq, r_coord_sq, (int)n_centres, (int)cap, rs.idx, rs.count, d_words};
    MD_WS(d_table, CoordTable, WS_MISC, sizeof(CoordTable));
    if ((rc = mdhip_h2d_small(ctx, d_table, &table, sizeof(CoordTable)))) return rc;
    KernelTimer timer(ctx, 2);
    ctx->last_kernel = "coord_hits_kernel";
    hipLaunchKernelGGL(coord_hits_kernel, dim3(g.grid), dim3(shell::THREADS), 0, ctx->stream, in.xyz,
                       (long long)n_atoms, in.box, in.centres, (int)n_centres, r_shell_sq, g, d_table);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(coord_rank_kernel, dim3(rs.grid(ctx, 32)), dim3(64), (size_t)cap * 16, ctx->stream, rs.idx,
                       d_words, rs.count, d_type, (long long)rs.n_rows, (int)cap);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, words, d_words, rs.n_rows * (size_t)cap * 8, 0))) return rc;
    if ((rc = shell::row_results(cs, rs, mols, count))) return rc;
    return shell::finish(cs, timer);
}

}  // extern "C"
