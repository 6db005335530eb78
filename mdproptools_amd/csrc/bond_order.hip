// bond_order.hip — per-centre order parameters of structural/order_parameters.py (calc_order_parameters): the Steinhardt
// bond-orientational q_l, the Lechner-Dellago averaged qbar_l and the tetrahedral pair q_tet, s_k. The reference has no
// such function; the arithmetic is specified in DESIGN.md (order parameters) and restated in tests/order_ref.py.
//
// One frame, one centre c:
//   neighbour j of c: a candidate with j != c, shell::rsq(c, j) < r_cut**2 (strict; the |d| form of the single wrap), and
//     mol_of[j] != mol_of[c] under exclusion; with n_nearest = k the k smallest by (rsq, atom index); a row with fewer
//     than k (without k: with no) neighbours is short;
//   d_j = shell::wrap_signed(x_j - x_c), n_j = sqrt((dx dx + dy dy) + dz dz), u_j = d_j / n_j; a selected neighbour whose
//     n_j is 0 or not finite makes the row degenerate;
//   q_lm = (1 / N) sum_j Y_lm(u_j) in a real basis, the sum in ascending atom index, q_l = sqrt(4 pi / (2l + 1) sum_m q_lm**2);
//   qbar_lm(c) = (q_lm(c) + sum_{j in N(c)} q_lm(j)) / (N + 1), the sum in ascending atom index, qbar_l as q_l; NaN of
//     any member (the row itself or a neighbour, short or degenerate) propagates and the row counts as short;
//   q_tet = 1 - 3/8 sum_{j<k} (cos_jk + 1/3)**2 and s_k = 1 - 1/3 sum_k (n_k - rbar)**2 / (4 rbar**2) over the 4 nearest
//     by (rsq, atom index), taken in ascending atom index.
// Contraction is off in this file.
//
//  1. shell::gather_kernel (shell_gather.h): one lane per (frame, candidate): the candidate planes [F][3][n_cand].
//  2. bo_search_kernel: the sweep of shell_search.h; a hit that is not the centre itself and not of its molecule under
//     exclusion is appended to the row (frame, centre) (shell::append).
//  3. bo_row_kernel: one wave per row. The row is staged in LDS (d, rsq, atom, candidate position), ranked by
//     (rsq, atom) when a selection is asked for, and the selected neighbours are put in ascending atom order as unit
//     vectors. Y_lm: tiles of BO_TILE neighbours, one lane per (neighbour of the tile, m): rho**m and ((x + i y) / rho)**m
//     by repeated products (rho == 0: only m = 0 is not zero), the normalised associated Legendre functions by their
//     recurrence in l, every requested degree on the way; the terms go to LDS, and one lane per component (l, m, re / im)
//     adds the tile's terms to its sum, neighbour by neighbour. The tetrahedral pair is lane 0's.
//  4. bo_average_kernel (averaged): one wave per row, one lane per component: the row's q_lm and those of its selected
//     neighbours (rows of the same frame: the candidates are the centres) from the workspace.
// Rows with count > cap give NaN and no flag: the host runs the call again.

#include <algorithm>
#include <cmath>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_gather.h"

namespace {

constexpr int BO_MAX_DEG = 4;
constexpr int BO_MAX_L = 12;
constexpr int BO_NL = BO_MAX_L + 1;
constexpr int BO_MAX_CAP = 512;
constexpr int BO_TILE = 4;                              // neighbours per tile of the Y_lm pass: 4 x 16 m-slots = one wave
constexpr int BO_MSLOTS = 16;
constexpr int BO_TERMS = BO_MAX_DEG * BO_MSLOTS * 2;    // the terms of one neighbour: [degree][m][re, im]
constexpr int BO_MAX_COMP = 128;                        // components of a row: sum of 2l + 1 (at most 25 + 23 + 21 + 19)
constexpr int BO_TABLE = BO_NL + 2 * BO_NL * BO_NL + BO_MAX_DEG;  // cmm | a | b | 4 pi / (2l + 1) per degree

constexpr int BO_AVERAGED = 1, BO_TETRAHEDRAL = 2;      // what a call computes beside q_l
constexpr int BO_Q_SHORT = 1, BO_Q_DEGENERATE = 2, BO_TET_SHORT = 4, BO_TET_DEGENERATE = 8,
              BO_QBAR_SHORT = 16;                       // the row's flags (include/mdhip.h)

// The requested degrees (by value: wave-uniform loads); component w of degree d is (m, re / im) = (0, re) for w == 0,
// ((w + 1) / 2, re) for odd w, (w / 2, im) for even w > 0, at off[d] + w of a row's n_comp components.
struct BoDegrees {
    int n, l_max, n_comp;
    int l[BO_MAX_DEG], off[BO_MAX_DEG];
};

// A candidate within the cutoff of a row's centre is appended unless it is the centre or of the centre's molecule
// (mol_of != nullptr). test_atom (wave-uniform, decided on the host): some atom is both centre and candidate, or there
// is an exclusion; most calls of distinct types test nothing more and a hit is an append.
__global__ __launch_bounds__(shell::THREADS) void bo_search_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ planes, long long n_cand,
    const double *__restrict__ box, const int *__restrict__ centres, int n_c, const int *__restrict__ cand,
    const int *__restrict__ mol_of, int test_atom, double rc2, int cap, shell::Grid g, int *__restrict__ idx,
    int *__restrict__ count)
{
    shell::sweep(xyz, n, centres, n_c, planes, 3, n_cand, box, rc2, g, [=](const shell::Row &r, size_t row, long long a) {
        if (test_atom && shell::excluded(cand[a], r.ci, mol_of)) return;
        shell::append(count, idx, row, cap, (int)a);
    });
}

// the term slot of component c of a row ([degree][m][re, im] of BO_TERMS), or -1 past n_comp
__device__ __forceinline__ int bo_term_slot(const BoDegrees &dg, int c)
{
    int slot = -1;
#pragma unroll
    for (int d = 0; d < BO_MAX_DEG; ++d) {
        const int w = c - dg.off[d];
        if (d < dg.n && w >= 0 && w <= 2 * dg.l[d])
            slot = (d * BO_MSLOTS + (w + 1) / 2) * 2 + (w > 0 && !(w & 1) ? 1 : 0);
    }
    return slot;
}

// q_l of the degrees from a row's components in LDS (lanes d < dg.n; the others return 0): the squares in component
// order
__device__ __forceinline__ double bo_invariant(const BoDegrees &dg, int lane, const double *s_qlm, const double *s_fac)
{
    double q = 0.0;
    if (lane < dg.n) {
        int off = 0, l = 0;
#pragma unroll
        for (int d = 0; d < BO_MAX_DEG; ++d)
            if (d == lane) off = dg.off[d], l = dg.l[d];
        double s = 0.0;
        for (int w = 0; w <= 2 * l; ++w) s += s_qlm[off + w] * s_qlm[off + w];
        q = __builtin_sqrt(s_fac[lane] * s);
    }
    return q;
}

// Dynamic LDS (doubles, then ints; every carve offset of the doubles is a multiple of 8 bytes): the tables [BO_TABLE,
// padded to even] | raw dx, dy, dz, rsq [cap] each | ux, uy, uz of the selected, in atom order [cap] each | the terms of
// a tile [BO_TILE][BO_TERMS] | the row's components [BO_MAX_COMP] | the four tetrahedral neighbours dx, dy, dz, n [4]
// each | atom, candidate position, rank [cap] each | the degenerate marks [2]. At cap 512: 2.8 + 16 + 12 + 4 + 1 + 0.1
// + 6 KB = 42 KB; at the first-try cap 64: 12.2 KB.
__global__ __launch_bounds__(64) void bo_row_kernel(const double *__restrict__ xyz, long long n,
                                                    const double *__restrict__ planes, long long n_cand,
                                                    const double *__restrict__ box, const int *__restrict__ centres,
                                                    int n_c, const int *__restrict__ cand, int *__restrict__ idx,
                                                    const int *__restrict__ count, long long n_rows, int cap,
                                                    BoDegrees dg, int k_nearest, int what,
                                                    const double *__restrict__ table, double *__restrict__ q_out,
                                                    double *__restrict__ tet_out, int *__restrict__ flags,
                                                    double *__restrict__ qlm, int *__restrict__ n_sel)
{
    extern __shared__ __attribute__((aligned(16))) double s_bo[];
    constexpr int TAB = (BO_TABLE + 1) & ~1;
    double *s_cmm = s_bo, *s_a = s_cmm + BO_NL, *s_b = s_a + BO_NL * BO_NL, *s_fac = s_b + BO_NL * BO_NL;
    double *p = s_bo + TAB;
    double *r_dx = p, *r_dy = p + cap, *r_dz = p + 2 * cap, *r_rsq = p + 3 * cap;
    p += 4 * (size_t)cap;
    double *s_ux = p, *s_uy = p + cap, *s_uz = p + 2 * cap;
    p += 3 * (size_t)cap;
    double *s_term = p;
    p += BO_TILE * BO_TERMS;
    double *s_qlm = p;
    p += BO_MAX_COMP;
    double *t_dx = p, *t_dy = p + 4, *t_dz = p + 8, *t_n = p + 12;
    p += 16;
    int *s_atom = (int *)p, *s_pos = s_atom + cap, *s_rank = s_pos + cap, *s_bad = s_rank + cap;
    const int lane = threadIdx.x;
    const bool averaged = what & BO_AVERAGED, tetra = what & BO_TETRAHEDRAL;
    const double qnan = __builtin_nan("");

    for (int i = lane; i < BO_TABLE; i += 64) s_bo[i] = table[i];
    const int slot0 = bo_term_slot(dg, lane), slot1 = bo_term_slot(dg, lane + 64);

    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int k = count[row];
        __syncthreads();  // (the tables are in place; the row before has been read)
        if (lane < 2) s_bad[lane] = 0;
        const bool over = k > cap;
        const int n_q = k_nearest > 0 ? k_nearest : k;  // the neighbours q_lm sums over
        const bool q_short = k == 0 || k < k_nearest, t_short = k < 4;
        if (!over && k > 0) {
            const shell::Row c = shell::row_of(xyz, n, box, centres, row / n_c, (int)(row % n_c));
            const int *r = idx + (size_t)row * (size_t)cap;
            for (int i = lane; i < k; i += 64) {
                const long long a = r[i];
                const auto [x, y, z] = shell::cand_xyz(planes, n_cand, c.f, a);
                r_dx[i] = shell::wrap_signed(x - c.cx, c.Lx);
                r_dy[i] = shell::wrap_signed(y - c.cy, c.Ly);
                r_dz[i] = shell::wrap_signed(z - c.cz, c.Lz);
                r_rsq[i] = shell::rsq(c.cx, c.cy, c.cz, x, y, z, c.Lx, c.Ly, c.Lz);
                s_atom[i] = cand[a];
                s_pos[i] = (int)a;
            }
            __syncthreads();
            const bool select = k_nearest > 0 || tetra;
            if (select) {
                for (int i = lane; i < k; i += 64) {
                    const double v = r_rsq[i];
                    const int at = s_atom[i];
                    int rank = 0;
                    for (int j = 0; j < k; ++j) rank += r_rsq[j] < v || (r_rsq[j] == v && s_atom[j] < at);
                    s_rank[i] = rank;
                }
                __syncthreads();
            }
            for (int i = lane; i < k; i += 64) {
                const int at = s_atom[i];
                const double dx = r_dx[i], dy = r_dy[i], dz = r_dz[i];
                const double nrm = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
                const bool bad = !(nrm > 0.0 && nrm < __builtin_inf());
                if (dg.n > 0 && !q_short && (k_nearest == 0 || s_rank[i] < k_nearest)) {
                    int pos = 0;
                    for (int j = 0; j < k; ++j)
                        pos += (k_nearest == 0 || s_rank[j] < k_nearest) && s_atom[j] < at;
                    s_ux[pos] = dx / nrm, s_uy[pos] = dy / nrm, s_uz[pos] = dz / nrm;
                    if (averaged) idx[(size_t)row * (size_t)cap + pos] = s_pos[i];  // (the staged row is in LDS)
                    if (bad) s_bad[0] = 1;
                }
                if (tetra && !t_short && s_rank[i] < 4) {
                    int pos = 0;
                    for (int j = 0; j < k; ++j) pos += s_rank[j] < 4 && s_atom[j] < at;
                    t_dx[pos] = dx, t_dy[pos] = dy, t_dz[pos] = dz, t_n[pos] = nrm;
                    if (bad) s_bad[1] = 1;
                }
            }
        }
        __syncthreads();
        const bool q_bad = s_bad[0] != 0, t_bad = s_bad[1] != 0;
        const bool q_ok = dg.n > 0 && !over && !q_short && !q_bad;

        double acc0 = 0.0, acc1 = 0.0;
        if (q_ok) {
            const int jj = lane >> 4, m = lane & (BO_MSLOTS - 1);
            for (int t0 = 0; t0 < n_q; t0 += BO_TILE) {
                const int j = t0 + jj;
                if (j < n_q) {
                    double re[BO_MAX_DEG], im[BO_MAX_DEG];
#pragma unroll
                    for (int d = 0; d < BO_MAX_DEG; ++d) re[d] = im[d] = 0.0;
                    if (m <= dg.l_max) {
                        const double x = s_ux[j], y = s_uy[j], z = s_uz[j];
                        const double rho = __builtin_sqrt(x * x + y * y);
                        const double ex = rho > 0.0 ? x / rho : 1.0, ey = rho > 0.0 ? y / rho : 0.0;
                        double cr = 1.0, ci = 0.0, rp = 1.0;  // ((x + i y) / rho)**m and rho**m
                        for (int t = 0; t < m; ++t) {
                            const double nr = cr * ex - ci * ey, ni = cr * ey + ci * ex;
                            cr = nr, ci = ni;
                            rp *= rho;
                        }
                        const double w = m ? 1.4142135623730951 : 1.0;
                        double p2 = 0.0, p1 = s_cmm[m] * rp;  // the normalised P_l^m: l - 2 and l - 1, then l
                        for (int l = m; l <= dg.l_max; ++l) {
                            if (l > m) {
                                const double pn = s_a[l * BO_NL + m] * (z * p1 - s_b[l * BO_NL + m] * p2);
                                p2 = p1, p1 = pn;
                            }
#pragma unroll
                            for (int d = 0; d < BO_MAX_DEG; ++d)
                                if (d < dg.n && dg.l[d] == l) re[d] = w * p1 * cr, im[d] = m ? w * p1 * ci : 0.0;
                        }
                    }
#pragma unroll
                    for (int d = 0; d < BO_MAX_DEG; ++d) {
                        s_term[jj * BO_TERMS + (d * BO_MSLOTS + m) * 2] = re[d];
                        s_term[jj * BO_TERMS + (d * BO_MSLOTS + m) * 2 + 1] = im[d];
                    }
                }
                __syncthreads();
                const int tn = n_q - t0 < BO_TILE ? n_q - t0 : BO_TILE;
                for (int b = 0; b < tn; ++b) {  // (ascending atom index: the tiles in order, their neighbours in order)
                    if (slot0 >= 0) acc0 += s_term[b * BO_TERMS + slot0];
                    if (slot1 >= 0) acc1 += s_term[b * BO_TERMS + slot1];
                }
                __syncthreads();
            }
        }
        if (dg.n > 0) {
            const double v0 = q_ok ? acc0 / (double)n_q : qnan, v1 = q_ok ? acc1 / (double)n_q : qnan;
            if (slot0 >= 0) s_qlm[lane] = v0;
            if (slot1 >= 0) s_qlm[lane + 64] = v1;
            if (averaged) {
                if (slot0 >= 0) qlm[(size_t)row * (size_t)dg.n_comp + lane] = v0;
                if (slot1 >= 0) qlm[(size_t)row * (size_t)dg.n_comp + lane + 64] = v1;
                if (lane == 0) n_sel[row] = q_ok ? n_q : 0;
            }
            __syncthreads();
            const double q = bo_invariant(dg, lane, s_qlm, s_fac);
            if (lane < dg.n) q_out[(size_t)row * (size_t)dg.n + lane] = q;
        }
        if (lane == 0) {
            int fl = 0;
            if (!over && dg.n > 0) fl |= q_short ? BO_Q_SHORT : (q_bad ? BO_Q_DEGENERATE : 0);
            if (tetra) {
                double q_tet = qnan, s_k = qnan;
                if (!over) fl |= t_short ? BO_TET_SHORT : (t_bad ? BO_TET_DEGENERATE : 0);
                if (!over && !t_short && !t_bad) {
                    double s = 0.0;
                    for (int a = 0; a < 3; ++a)
                        for (int b = a + 1; b < 4; ++b) {
                            const double dot = (t_dx[a] * t_dx[b] + t_dy[a] * t_dy[b]) + t_dz[a] * t_dz[b];
                            const double cs = dot / (t_n[a] * t_n[b]) + 1.0 / 3.0;
                            s += cs * cs;
                        }
                    q_tet = 1.0 - 0.375 * s;
                    const double rbar = (((t_n[0] + t_n[1]) + t_n[2]) + t_n[3]) / 4.0;
                    const double den = 4.0 * (rbar * rbar);
                    double v = 0.0;
                    for (int a = 0; a < 4; ++a) v += ((t_n[a] - rbar) * (t_n[a] - rbar)) / den;
                    s_k = 1.0 - v / 3.0;
                }
                tet_out[2 * (size_t)row] = q_tet;
                tet_out[2 * (size_t)row + 1] = s_k;
            }
            flags[row] = fl;
        }
    }
}

// LDS: the row's averaged components [BO_MAX_COMP] | 4 pi / (2l + 1) [BO_MAX_DEG] (static).
__global__ __launch_bounds__(64) void bo_average_kernel(const double *__restrict__ qlm, const int *__restrict__ idx,
                                                        const int *__restrict__ n_sel, const int *__restrict__ count,
                                                        long long n_rows, int n_c, int cap, BoDegrees dg,
                                                        const double *__restrict__ table, double *__restrict__ qbar_out,
                                                        int *__restrict__ flags)
{
    __shared__ double s_qlm[BO_MAX_COMP], s_fac[BO_MAX_DEG];
    const int lane = threadIdx.x;
    if (lane < BO_MAX_DEG) s_fac[lane] = table[BO_NL + 2 * BO_NL * BO_NL + lane];
    const bool has0 = lane < dg.n_comp, has1 = lane + 64 < dg.n_comp;
    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const bool over = count[row] > cap;
        const int n_nb = n_sel[row];
        const size_t frame0 = (size_t)(row / n_c) * (size_t)n_c;
        const int *r = idx + (size_t)row * (size_t)cap;
        const double qnan = __builtin_nan("");
        double acc0 = has0 ? qlm[(size_t)row * (size_t)dg.n_comp + lane] : 0.0;
        double acc1 = has1 ? qlm[(size_t)row * (size_t)dg.n_comp + lane + 64] : 0.0;
        for (int b = 0; b < n_nb; ++b) {  // (ascending atom index)
            const double *nb = qlm + (frame0 + (size_t)r[b]) * (size_t)dg.n_comp;
            if (has0) acc0 += nb[lane];
            if (has1) acc1 += nb[lane + 64];
        }
        __syncthreads();  // (the tables are in place; the row before has been read)
        if (has0) s_qlm[lane] = over ? qnan : acc0 / (double)(n_nb + 1);
        if (has1) s_qlm[lane + 64] = over ? qnan : acc1 / (double)(n_nb + 1);
        __syncthreads();
        const double q = bo_invariant(dg, lane, s_qlm, s_fac);
        if (lane < dg.n) qbar_out[(size_t)row * (size_t)dg.n + lane] = q;
        if (lane == 0 && !over && q != q)  // (a NaN of any member is one of every component: every degree is NaN)
            flags[row] |= BO_QBAR_SHORT;
    }
}

// cmm[m] = sqrt((2m + 1)!! / ((2m)!! 4 pi)): P_m^m = cmm[m] rho**m; P_l^m = a[l][m] (z P_(l-1)^m - b[l][m] P_(l-2)^m)
void bo_tables(const BoDegrees &dg, double *t)
{
    const double pi = 3.14159265358979323846;
    double *cmm = t, *a = t + BO_NL, *b = a + BO_NL * BO_NL, *fac = b + BO_NL * BO_NL;
    std::fill(t, t + BO_TABLE, 0.0);
    long double v = 1.0L / (4.0L * (long double)pi);
    cmm[0] = (double)sqrtl(v);
    for (int m = 1; m <= BO_MAX_L; ++m) {
        v *= (long double)(2 * m + 1) / (long double)(2 * m);
        cmm[m] = (double)sqrtl(v);
    }
    for (int l = 1; l <= BO_MAX_L; ++l)
        for (int m = 0; m < l; ++m) {
            a[l * BO_NL + m] = std::sqrt((4.0 * l * l - 1.0) / ((double)l * l - (double)m * m));
            b[l * BO_NL + m] = std::sqrt((((double)l - 1.0) * (l - 1.0) - (double)m * m) / (4.0 * (l - 1.0) * (l - 1.0) - 1.0));
        }
    for (int d = 0; d < dg.n; ++d) fac[d] = 4.0 * pi / (2.0 * dg.l[d] + 1.0);
}

}  // namespace

extern "C" {

int mdhip_bond_order(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                     const double *box, int32_t n_centres, const int32_t *centres, int32_t n_cand, const int32_t *cand,
                     const int32_t *mol_of, double r_cut_sq, int32_t n_degrees, const int32_t *degrees,
                     int32_t n_nearest, int32_t averaged, int32_t tetrahedral, int32_t cap, double *q, double *qbar,
                     double *tet, int32_t *flags, int32_t *count)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_centres >= 0 && n_cand >= 0, "negative sizes");
    MD_REQUIRE(n_degrees >= 0 && n_degrees <= BO_MAX_DEG, "n_degrees must be in [0, %d]", BO_MAX_DEG);
    MD_REQUIRE(n_degrees == 0 || degrees, "NULL array");
    BoDegrees dg;
    memset(&dg, 0, sizeof dg);
    dg.n = n_degrees;
    for (int d = 0; d < n_degrees; ++d) {
        MD_REQUIRE(degrees[d] >= 1 && degrees[d] <= BO_MAX_L, "degree %d: l must be in [1, %d]", d, BO_MAX_L);
        for (int e = 0; e < d; ++e) MD_REQUIRE(degrees[e] != degrees[d], "degree %d: l = %d twice", d, (int)degrees[d]);
        dg.l[d] = degrees[d];
        dg.off[d] = dg.n_comp;
        dg.n_comp += 2 * dg.l[d] + 1;
        dg.l_max = std::max(dg.l_max, dg.l[d]);
    }
    MD_REQUIRE(n_degrees > 0 || tetrahedral, "nothing to compute: no degrees and no tetrahedral order");
    MD_REQUIRE(!averaged || n_degrees > 0, "averaged needs at least one degree");
    MD_REQUIRE(n_nearest >= 0 && n_nearest <= BO_MAX_CAP, "n_nearest must be in [0, %d]", BO_MAX_CAP);
    MD_REQUIRE(r_cut_sq >= 0.0, "the squared cutoff must not be negative");
    shell::RowSet rs;
    int rc;
    if ((rc = shell::take_rows(ctx, n_frames, n_centres, cap, BO_MAX_CAP, rs))) return rc;
    if (rs.n_rows == 0) return cs.end();
    MD_REQUIRE(flags && count, "NULL array");
    MD_REQUIRE((q || n_degrees == 0) && (qbar || !averaged) && (tet || !tetrahedral), "NULL array");
    MD_REQUIRE(cand || n_cand == 0, "NULL array");
    if ((rc = shell::check_indices(ctx, "candidate", n_cand, cand, 1, n_atoms))) return rc;
    shell::Inputs in;
    if ((rc = shell::stage(ctx, "centre", n_frames, n_atoms, xyz, xyz_on_device, box, n_centres, centres, in)))
        return rc;
    if (averaged)  // (a neighbour's q_lm is a row of this call)
        MD_REQUIRE(n_cand == n_centres && std::equal(cand, cand + n_cand, centres),
                   "averaged needs the candidates to be the centres");
    if (n_cand == 0) {  // (no atom can be a neighbour: every row is short)
        const double nan = std::nan("");
        if (n_degrees) std::fill(q, q + rs.n_rows * (size_t)n_degrees, nan);
        if (averaged) std::fill(qbar, qbar + rs.n_rows * (size_t)n_degrees, nan);
        if (tetrahedral) std::fill(tet, tet + rs.n_rows * 2, nan);
        std::fill(flags, flags + rs.n_rows, (n_degrees ? BO_Q_SHORT : 0) | (tetrahedral ? BO_TET_SHORT : 0));
        if ((rc = shell::row_results(cs, rs, nullptr, count))) return rc;
        return cs.end();
    }

    // the tables: doubles cmm | a | b | 4 pi / (2l + 1); ints the candidates' atoms | mol_of [n_atoms] (under exclusion)
    double h_tab[BO_TABLE];
    bo_tables(dg, h_tab);
    MD_WS(d_tab, double, WS_TABLES, sizeof h_tab);
    if ((rc = mdhip_h2d_small(ctx, d_tab, h_tab, sizeof h_tab))) return rc;
    const int *d_cand, *d_mol;
    shell::IntTable ints;
    ints.add(cand, n_cand, &d_cand);
    ints.add_optional(mol_of, n_atoms, &d_mol);
    if ((rc = shell::upload_ints(ctx, ints, WS_TYPE_J))) return rc;
    const int test_atom = mol_of || shell::shares_an_atom(n_atoms, centres, n_centres, cand, n_cand);

    const size_t nq = rs.n_rows * (size_t)std::max(n_degrees, 1);
    double *d_planes;
    if ((rc = shell::planes_room(ctx, n_frames, n_cand, d_planes))) return rc;
    MD_WS(d_q, double, WS_HIST, nq * 8);
    MD_WS(d_qbar, double, WS_OUT2, averaged ? nq * 8 : 8);
    MD_WS(d_tet, double, WS_OUT3, rs.n_rows * 16);
    MD_WS(d_flags, int, WS_MISC, rs.n_rows * 4);
    MD_WS(d_qlm, double, WS_AUX2, averaged ? rs.n_rows * (size_t)dg.n_comp * 8 : 8);
    MD_WS(d_nsel, int, WS_AUX3, rs.n_rows * 4);

    KernelTimer timer(ctx, averaged ? 4 : 3);
    KernelTimer search(ctx, 2, true);  // the gather and the search: the call's aux time; the rest is the row passes
    ctx->last_kernel = "bo_search_kernel";
    if ((rc = shell::gather(ctx, in.xyz, n_frames, n_atoms, d_cand, n_cand, d_planes))) return rc;
    const shell::Grid g = shell::sweep_grid(ctx, n_frames, n_centres, n_cand);
    hipLaunchKernelGGL(bo_search_kernel, dim3(g.grid), dim3(shell::THREADS), 0, ctx->stream, in.xyz,
                       (long long)n_atoms, d_planes, (long long)n_cand, in.box, in.centres, (int)n_centres, d_cand, d_mol,
                       test_atom, r_cut_sq, (int)cap, g, rs.idx, rs.count);
    MD_HIP(hipGetLastError());
    search.stop();
    const int what = (averaged ? BO_AVERAGED : 0) | (tetrahedral ? BO_TETRAHEDRAL : 0);
    const size_t lds = (((size_t)BO_TABLE + 1) / 2 * 2 + 7 * (size_t)cap + BO_TILE * BO_TERMS + BO_MAX_COMP + 16) * 8 +
                       (3 * (size_t)cap + 2) * 4;
    hipLaunchKernelGGL(bo_row_kernel, dim3(rs.grid(ctx, 16)), dim3(64), lds, ctx->stream, in.xyz, (long long)n_atoms,
                       d_planes, (long long)n_cand, in.box, in.centres, (int)n_centres, d_cand, rs.idx, rs.count,
                       (long long)rs.n_rows, (int)cap, dg, (int)n_nearest, what, d_tab, d_q, d_tet, d_flags, d_qlm,
                       d_nsel);
    MD_HIP(hipGetLastError());
    if (averaged) {
        hipLaunchKernelGGL(bo_average_kernel, dim3(rs.grid(ctx, 16)), dim3(64), 0, ctx->stream, d_qlm, rs.idx, d_nsel,
                           rs.count, (long long)rs.n_rows, (int)n_centres, (int)cap, dg, d_tab, d_qbar, d_flags);
        MD_HIP(hipGetLastError());
    }
    timer.stop();
    if (n_degrees && (rc = mdhip_result(cs, q, d_q, rs.n_rows * (size_t)n_degrees * 8, 0))) return rc;
    if (averaged && (rc = mdhip_result(cs, qbar, d_qbar, rs.n_rows * (size_t)n_degrees * 8, 0))) return rc;
    if (tetrahedral && (rc = mdhip_result(cs, tet, d_tet, rs.n_rows * 16, 0))) return rc;
    if ((rc = mdhip_result(cs, flags, d_flags, rs.n_rows * 4, 0))) return rc;
    if ((rc = shell::row_results(cs, rs, nullptr, count))) return rc;
    return shell::finish(cs, timer, &search);
}

}  // extern "C"
