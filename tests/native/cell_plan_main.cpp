// cell_plan_main.cpp — walks the cell grid of csrc/cell_plan.h (the cells of mdhip_free_volume) over fixed cases and seeded
// random ones; tests/test_cell_plan_native_cpu.py builds it with g++ under -fsanitize=address,undefined. The header is
// host arithmetic only (its CP_HD functions are the ones the kernels call).
// Checked:
//   cp_cells      at an edge of exactly k * r_search, one step of the double below and above it, and at
//                 k * r_search * (1 + 2^-19): the margin, not a rounding, decides — k - 1 cells for the first three, k for
//                 the last; the cap of 64; never fewer than 1; for random edges nc is the LARGEST count whose cell edge
//                 holds the margin (checked in long double);
//   cp_neighbours at nc = 1, 2, 3 and more: no cell twice, and as a set the cells c - 1, c, c + 1 (cyclic);
//   cp_point_lo   the cells' point ranges tile [0, g) in order, a point lies in the range of cp_point_cell of it, a range
//                 holds at most min(g, g / nc + 2) points; cp_frame's nsub bricks hold the fullest cell, on a frame whose
//                 three axes differ and on random ones;
//   the margin    for random atoms (fractions drawn at and next to cell faces as well) and grid points: whenever the
//                 minimum-image distance along an axis, formed in long double from the coordinates the kernel forms, is
//                 below r_search * (1 + 2^-40), the two cells differ by at most one, cyclically.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>

#include "../../mdproptools_amd/csrc/cell_plan.h"

static long failures = 0, n_cells = 0, n_sets = 0, n_points = 0, n_pairs = 0;
static std::string what;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                \
    } while (0)

static void check_cells(double L, double r)
{
    const int nc = cp_cells(L, r);
    ++n_cells;
    const long double need = (long double)r * (1.0L + (long double)CP_MARGIN);
    CHECK(nc >= 1 && nc <= CP_MAX_NC);
    // the count holds the margin (unless it is the 1 that every axis gets), and the next one does not, up to the host's roundings
    CHECK(nc == 1 || (long double)L / nc >= need * (1.0L - 0x1p-50L));
    CHECK(nc == CP_MAX_NC || (long double)L / (nc + 1) < need * (1.0L + 0x1p-50L));
}

static void at_the_edges()
{
    what = "cp_cells at k * r_search";
    const double rs[] = {2.5, 3.0, 0.7, 4.0 / 3.0, 1e-3, 977.0};
    for (double r : rs)
        for (int k = 1; k <= 70; ++k) {
            const double L = (double)k * r;
            const int below = k == 1 ? 1 : (k - 1 > CP_MAX_NC ? CP_MAX_NC : k - 1);
            CHECK(cp_cells(L, r) == below);
            CHECK(cp_cells(std::nextafter(L, 0.0), r) == below);
            CHECK(cp_cells(std::nextafter(L, 2.0 * L), r) == below);
            CHECK(cp_cells(L * (1.0 + 0x1p-19), r) == (k > CP_MAX_NC ? CP_MAX_NC : k));
            check_cells(L, r), check_cells(std::nextafter(L, 0.0), r), check_cells(L * (1.0 + 0x1p-19), r);
        }
    CHECK(cp_cells(1.0, 5.0) == 1 && cp_cells(1e9, 1.0) == CP_MAX_NC && cp_cells(std::nan(""), 1.0) == 1);
}

static void neighbour_sets()
{
    what = "cp_neighbours";
    for (int nc = 1; nc <= CP_MAX_NC; ++nc)
        for (int c = 0; c < nc; ++c) {
            int out[3] = {-1, -1, -1};
            const int k = cp_neighbours(c, nc, out);
            ++n_sets;
            std::set<int> got(out, out + k), want = {(c + nc - 1) % nc, c, (c + 1) % nc};
            CHECK(k == (nc >= 3 ? 3 : nc));
            CHECK((int)got.size() == k);  // no cell twice
            CHECK(got == want);
            CHECK(out[0] == c);
        }
}

static void point_ranges(int g, int nc)
{
    char buf[96];
    snprintf(buf, sizeof buf, "cp_point_lo g = %d, nc = %d", g, nc);
    what = buf;
    CHECK(cp_point_lo(0, g, nc) == 0 && cp_point_lo(nc, g, nc) == g);
    const int most = g / nc + 2 < g ? g / nc + 2 : g;
    for (int c = 0; c < nc; ++c) {
        const int lo = cp_point_lo(c, g, nc), hi = cp_point_lo(c + 1, g, nc);
        CHECK(lo <= hi && hi - lo <= most);
        for (int i = lo; i < hi; ++i, ++n_points) CHECK(cp_point_cell(i, g, nc) == c);
    }
}

static void frame(const double *L, const int32_t *g, double r)
{
    what = "cp_frame";
    const CpFrame fr = cp_frame(L, g, r);
    long long fullest = 1;
    for (int a = 0; a < 3; ++a) {
        CHECK(fr.nc[a] == cp_cells(L[a], r));
        point_ranges(g[a], fr.nc[a]);
        int most = 0;
        for (int c = 0; c < fr.nc[a]; ++c) most = std::max(most, cp_point_lo(c + 1, g[a], fr.nc[a]) - cp_point_lo(c, g[a], fr.nc[a]));
        fullest *= most;
    }
    what = "cp_frame";
    CHECK(fr.nsub >= 1 && (long long)fr.nsub * CP_BRICK >= fullest);
    CHECK(fr.cells() == (long long)fr.nc[0] * fr.nc[1] * fr.nc[2] && fr.units() == fr.cells() * fr.nsub);
}

// the kernel's coordinates of an atom (from its wrapped fraction f) and of a point, and their cells
static void margin_pair(double L, double r, int g, int i, double f)
{
    const int nc = cp_cells(L, r);
    const double xw = f * L, p = cp_point_frac(i, g) * L;
    const int ca = cp_cell_of(f, nc), cp = cp_point_cell(i, g, nc);
    long double d = fabsl((long double)p - (long double)xw);
    d = std::min(d, fabsl(d - (long double)L));
    ++n_pairs;
    if (d < (long double)r * (1.0L + 0x1p-40L)) {
        const int diff = ((ca - cp) % nc + nc) % nc;
        CHECK(diff == 0 || diff == 1 || diff == nc - 1);
    }
}

int main(int argc, char **argv)
{
    const long n_random = argc > 1 ? atol(argv[1]) : 2000;
    at_the_edges();
    neighbour_sets();
    const int gs[] = {1, 2, 3, 7, 8, 17, 64, 65, 1000, 65537};
    for (int g : gs)
        for (int nc = 1; nc <= CP_MAX_NC; ++nc) point_ranges(g, nc);
    {   // a frame whose three axes differ: 2, 3 and 1 cells, an odd grid
        const double L[3] = {11.3, 13.1, 6.0};
        const int32_t g[3] = {17, 19, 13};
        frame(L, g, 4.0);
        const CpFrame fr = cp_frame(L, g, 4.0);
        what = "three different axes";
        CHECK(fr.nc[0] == 2 && fr.nc[1] == 3 && fr.nc[2] == 1 && fr.nsub == 2 && fr.units() == 12);
    }
    std::mt19937_64 rng(20261021);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (long n = 0; n < n_random; ++n) {
        const double r = 0.5 + 5.0 * u(rng);
        double L[3];
        int32_t g[3];
        for (int a = 0; a < 3; ++a) {
            L[a] = r * (0.6 + 12.0 * u(rng));
            if (n % 7 == 0) L[a] = r * std::floor(1.0 + 9.0 * u(rng));  // exactly a multiple
            g[a] = 1 + (int32_t)(rng() % (a == 0 && n % 11 == 0 ? 5000 : 90));
            check_cells(L[a], r);
        }
        frame(L, g, r);
        what = "the margin";
        for (int a = 0; a < 3; ++a) {
            const int nc = cp_cells(L[a], r);
            for (int t = 0; t < 40; ++t) {
                double f = u(rng);
                if (t % 4 == 1) f = (double)(rng() % (nc + 1)) / nc;                       // on a face
                if (t % 4 == 2) f = std::nextafter((double)(rng() % (nc + 1)) / nc, 0.0);  // just inside it
                if (t % 4 == 3) f = std::nextafter((double)(rng() % nc) / nc, 1.0);
                if (!(f < 1.0)) f = 0.0;  // (the kernel's own fold)
                margin_pair(L[a], r, g[a], (int)(rng() % g[a]), f);
            }
        }
    }
    printf("cells %ld sets %ld points %ld pairs %ld failures %ld\n", n_cells, n_sets, n_points, n_pairs, failures);
    return failures ? 1 : 0;
}
