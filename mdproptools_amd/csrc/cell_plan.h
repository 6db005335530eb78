// cell_plan.h — the per-frame cell grid of mdhip_free_volume (free_volume.hip): how many cells an axis gets, which cell
// an atom and a grid point fall in, which grid points a cell holds and which DISTINCT cells neighbour it.
// Everything here is arithmetic on plain values (no HIP header, no context), in the form of shape_plan.h:
// tests/native/cell_plan_main.cpp includes this header with g++ and walks it under sanitizers; the kernels call the same
// functions (CP_HD), so what the test walks is what the device does. An unnamed namespace, as the kernels that take
// CpFrame: their symbols keep their names.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define CP_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define CP_HD inline
#endif

namespace {

constexpr int CP_MAX_NC = 64;  // cells per axis at most: 2^18 cells, 1 MiB of cell starts per frame in flight
constexpr int CP_BRICK = 1024;  // grid points of one cell that one workgroup takes at a time (256 lanes x 4)

// The relative margin of a cell edge over r_search: nc_a is the largest count with L_a / nc_a >= r_search * (1 + CP_MARGIN).
// Why every candidate of a point lies in the up to 27 cells around the point's cell, whatever the roundings:
//   positions in CELL UNITS. An atom's cell is min((int)(f * nc), nc - 1) of its wrapped fraction f in [0, 1), and its
//   coordinate is xw = fl(f * L); a point's cell is the same function of u = fl((i + 0.5) / g), its coordinate p = fl(u * L).
//   xw / (L / nc) and fl(f * nc) differ by two roundings of a number below nc <= 64, so a position lies within
//   delta = 64 * 2^-51 = 2^-45 of the interval [c, c + 1] of its cell c (the clamp to nc - 1 and an xw that rounds to L
//   itself included).
//   A candidate has the COMPUTED rsq < r_search_sq = fl(r_search^2); the squares, their two sums and the three
//   differences |p - xw|, ||p - xw| - L| carry one rounding each, so per axis the real minimum-image distance of the two
//   coordinates is below r_search * (1 + 2^-50), which in cell units is below (1 + 2^-50) / (1 + 2^-20) < 1 - 2^-21.
//   Two positions less than 1 - 2^-21 apart (under some image), each within 2^-45 of its cell's interval, have cell
//   indices that differ by less than 2 - 2^-21 + 2^-44 < 2, that is by at most 1, cyclically. The roundings
//   (2^-44 all told) stand against a margin of 2^-21: rounding does not decide whether an atom is found, and since the
//   cell edge EXCEEDS r_search while a candidate is strictly inside it, an exact tie does not either. The host's own
//   roundings in choosing nc (one product, one quotient: 2^-52 each) vanish against the margin in the same way.
constexpr double CP_MARGIN = 0x1p-20;

// the cells of an axis of edge L: at least 1 (then every atom is staged for every point; L < r_search is the caller's affair)
inline int cp_cells(double L, double r_search)
{
    const double need = r_search * (1.0 + CP_MARGIN);
    const double q = L / need;
    int nc = q >= (double)CP_MAX_NC ? CP_MAX_NC : (q >= 1.0 ? (int)q : 1);
    while (nc > 1 && !(L / (double)nc >= need)) --nc;
    while (nc < CP_MAX_NC && L / (double)(nc + 1) >= need) ++nc;
    return nc;
}

// the cell of a fraction in [0, 1]
CP_HD int cp_cell_of(double frac, int nc)
{
    const int c = (int)(frac * (double)nc);
    return c < nc - 1 ? c : nc - 1;
}

// the fraction and the cell of grid point i of g along an axis
CP_HD double cp_point_frac(int i, int g) { return ((double)i + 0.5) / (double)g; }
CP_HD int cp_point_cell(int i, int g, int nc) { return cp_cell_of(cp_point_frac(i, g), nc); }

// The first grid point whose cell is c or beyond (c in [0, nc]; g for c = nc): the points of cell c are
// [cp_point_lo(c), cp_point_lo(c + 1)). cp_point_cell does not decrease with i, so an estimate is walked to the place.
CP_HD int cp_point_lo(int c, int g, int nc)
{
    if (c <= 0) return 0;
    if (c >= nc) return g;
    int i = (int)(((double)c * (double)g) / (double)nc);
    if (i > g) i = g;
    while (i > 0 && cp_point_cell(i - 1, g, nc) >= c) --i;
    while (i < g && cp_point_cell(i, g, nc) < c) ++i;
    return i;
}

// The distinct cells among c - 1, c, c + 1 (cyclic) of an axis of nc cells, c first: 1 for nc = 1, 2 for nc = 2, else 3
CP_HD int cp_neighbours(int c, int nc, int out[3])
{
    out[0] = c;
    if (nc == 1) return 1;
    out[1] = c + 1 < nc ? c + 1 : 0;
    if (nc == 2) return 2;
    out[2] = c > 0 ? c - 1 : nc - 1;
    return 3;
}

// One frame's grid: cells per axis, and how many bricks of CP_BRICK points its fullest cell may need. A cell holds at
// most g / nc + 2 points along an axis (the real count is within one of g / nc) and never more than g.
struct CpFrame {
    int nc[3];
    int nsub;
    CP_HD long long cells() const { return (long long)nc[0] * nc[1] * nc[2]; }
    CP_HD long long units() const { return cells() * nsub; }  // (cell, brick) pairs: what a workgroup takes at a time
};

inline CpFrame cp_frame(const double *L, const int32_t *g, double r_search)
{
    CpFrame fr;
    long long pts = 1;
    for (int a = 0; a < 3; ++a) {
        fr.nc[a] = cp_cells(L[a], r_search);
        const long long per = (long long)g[a] / fr.nc[a] + 2;
        pts *= per < g[a] ? per : g[a];
    }
    fr.nsub = (int)((pts + CP_BRICK - 1) / CP_BRICK);
    return fr;
}

}  // namespace
