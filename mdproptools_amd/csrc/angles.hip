// angles.hip — bond-angle histograms of structural/angular_distribution.py (calc_angular_distribution): the
// distribution of the angle A-C-B at a centre atom C between two of its shell neighbours. The reference has no such
// function; the arithmetic is specified in DESIGN.md (angular distribution) and restated in tests/angular_ref.py.
//
// One frame, one centre c, one triplet t = (type_a, type_c, type_b, r_ca, r_cb):
//   neighbour j of c in role A: j != c, type[j] == type_a, shell::rsq(c, j) < r_ca**2 (strict; the |d| form of the
//     single wrap), and mol_of[j] != mol_of[c] under exclusion; role B the same with type_b and r_cb;
//   d_j = shell::wrap_signed(x_j - x_c), n_j = sqrt((dx dx + dy dy) + dz dz),
//   cos = ((dxj dxk + dyj dyk) + dzj dzk) / (n_j * n_k), unfused, correctly rounded sqrt and division;
//   bin = the number of m in [1, n_bins) with cos <= E[m], E[m] = cos(m * bin_size) from the host, strictly
//     decreasing (theta in [m D, (m + 1) D), the last bin closed, no clamp, no acos); a NaN cosine is in no bin and
//     counts in n_degenerate[t];
//   a symmetric triplet (type_a == type_b and r_ca == r_cb) counts every unordered pair {j, k} of role-A neighbours
//     once, an asymmetric one every ordered (j, k), j != k, j in role A and k in role B.
// Contraction is off in this file.
//
//  1. shell::gather_kernel (shell_gather.h): one lane per (frame, candidate): the candidate planes [F][3][n_cand], so
//     that the sweep reads coalesced planes of only the atoms that can be a neighbour.
//  2. ang_search_kernel: the sweep of shell_search.h with the largest cutoff of all. A hit (rare) that is not the
//     centre itself, not of its molecule under exclusion, and within the largest cutoff of the centre's class is
//     appended to the row (frame, centre) (shell::append). Which of those tests a call needs at all is decided on
//     the host.
//  3. ang_pair_kernel: one wave per row. The row is staged in LDS in tiles of ANG_TILE neighbours (d, the norm and a
//     mask of the (triplet, role) pairs the neighbour serves); the lanes walk the pairs j < k of a tile pair, test the
//     two masks against each other, and only a pair that counts somewhere computes its cosine, finds the bin by binary
//     search in the LDS copy of E and adds into the block's LDS histogram, which goes to the global uint64 bins once
//     per block. Rows with count > cap add nothing.

#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_gather.h"

namespace {

constexpr int ANG_MAX_TRIPLETS = 8;
constexpr int ANG_MAX_CELLS = 4096;  // n_triplets * n_bins: the block's histogram (16 KB) and E (up to 32 KB) in LDS
constexpr int ANG_MAX_CAP = 512;
constexpr int ANG_TILE = 64;         // neighbours per staged tile (two tiles: 4.5 KB)

// The triplet table (by value: wave-uniform loads). Classes are the caller's atom types.
struct AngTriplets {
    int n;
    unsigned sym;  // bit t: triplet t is symmetric
    int ta[ANG_MAX_TRIPLETS], tc[ANG_MAX_TRIPLETS], tb[ANG_MAX_TRIPLETS];
    double ra2[ANG_MAX_TRIPLETS], rb2[ANG_MAX_TRIPLETS];
};

// What the search tests at a hit beyond the sweep's own cutoff, decided per call on the host (wave-uniform): most calls
// (one centre type, no atom both centre and candidate, no exclusion) test nothing more and a hit is an append.
constexpr int ANG_TEST_ATOM = 1;    // the candidate's atom is looked up: it may be the centre, or of its molecule
constexpr int ANG_TEST_RADIUS = 2;  // the centres' largest cutoffs differ: rsq again, against the centre's own

// A candidate within the sweep's cutoff of a row's centre is appended unless it is the centre, of the centre's molecule
// (mol_of != nullptr), or beyond the largest cutoff of the centre's class.
__global__ __launch_bounds__(shell::THREADS) void ang_search_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ planes, long long n_cand,
    const double *__restrict__ box, const int *__restrict__ centres, int n_c, const int *__restrict__ cand,
    const int *__restrict__ mol_of, const double *__restrict__ cen_rmax2, int tests, double rc2, int cap,
    shell::Grid g, int *__restrict__ idx, int *__restrict__ count)
{
    shell::sweep(xyz, n, centres, n_c, planes, 3, n_cand, box, rc2, g, [=](const shell::Row &r, size_t row, long long a) {
        if ((tests & ANG_TEST_ATOM) && shell::excluded(cand[a], r.ci, mol_of)) return;
        if (tests & ANG_TEST_RADIUS) {
            const shell::Xyz p = shell::cand_xyz(planes, n_cand, r.f, a);
            if (!(shell::rsq(r.cx, r.cy, r.cz, p.x, p.y, p.z, r.Lx, r.Ly, r.Lz) < cen_rmax2[r.c])) return;
        }
        shell::append(count, idx, row, cap, (int)a);
    });
}

// One staged tile of a row: d, the norm, and the mask (bit t: role A of triplet t, bit 8 + t: role B of an asymmetric
// triplet t; only triplets of the centre's class).
struct AngTile {
    double *dx, *dy, *dz, *nrm;
    unsigned *mask;
};

__device__ __forceinline__ void ang_stage(const AngTile &s, int lane, int m, const int *__restrict__ r,
                                          const double *__restrict__ q, long long n_cand,
                                          const int *__restrict__ cand_class, int cc, const AngTriplets &tr,
                                          const shell::Row &c)
{
    if (lane < m) {
        const long long a = r[lane];
        const double x = q[a], y = q[n_cand + a], z = q[2 * n_cand + a];  // (q: the frame's planes, found once per row)
        const double dx = shell::wrap_signed(x - c.cx, c.Lx), dy = shell::wrap_signed(y - c.cy, c.Ly),
                     dz = shell::wrap_signed(z - c.cz, c.Lz);
        const double rsq = shell::rsq(c.cx, c.cy, c.cz, x, y, z, c.Lx, c.Ly, c.Lz);
        const int cls = cand_class[a];
        unsigned mask = 0;
#pragma unroll
        for (int t = 0; t < ANG_MAX_TRIPLETS; ++t) {
            if (t < tr.n && tr.tc[t] == cc) {
                if (cls == tr.ta[t] && rsq < tr.ra2[t]) mask |= 1u << t;
                if (!((tr.sym >> t) & 1u) && cls == tr.tb[t] && rsq < tr.rb2[t]) mask |= 0x100u << t;
            }
        }
        s.dx[lane] = dx;
        s.dy[lane] = dy;
        s.dz[lane] = dz;
        s.nrm[lane] = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
        s.mask[lane] = mask;
    }
}

// Dynamic LDS: E [n_bins] (double) | tiles J and K: 4 x [ANG_TILE] double each | hist [n_trip * n_bins + n_trip]
// (unsigned: the bins, then the degenerate counts) | masks J, K [ANG_TILE] (unsigned). At the limits 32 KB + 4 KB +
// 16 KB + 32 B + 512 B < 64 KB. Every carve offset of the doubles is a multiple of 8.
__global__ __launch_bounds__(64) void ang_pair_kernel(const double *__restrict__ xyz, long long n,
                                                      const double *__restrict__ planes, long long n_cand,
                                                      const double *__restrict__ box, const int *__restrict__ centres,
                                                      const int *__restrict__ cen_class, int n_c,
                                                      const int *__restrict__ cand_class, const int *__restrict__ idx,
                                                      const int *__restrict__ count, long long n_rows, int cap,
                                                      AngTriplets tr, const double *__restrict__ edges, int n_bins,
                                                      unsigned long long *__restrict__ hist)
{
    extern __shared__ __attribute__((aligned(16))) double s_ang[];
    double *s_e = s_ang;
    AngTile tj, tk;
    double *p = s_e + n_bins;
    tj.dx = p, tj.dy = p + ANG_TILE, tj.dz = p + 2 * ANG_TILE, tj.nrm = p + 3 * ANG_TILE;
    p += 4 * ANG_TILE;
    tk.dx = p, tk.dy = p + ANG_TILE, tk.dz = p + 2 * ANG_TILE, tk.nrm = p + 3 * ANG_TILE;
    p += 4 * ANG_TILE;
    const int n_cells = tr.n * n_bins + tr.n;  // bins of every triplet, then n_degenerate
    unsigned *s_hist = (unsigned *)p;
    tj.mask = s_hist + n_cells;
    tk.mask = tj.mask + ANG_TILE;
    const int lane = threadIdx.x;

    for (int b = lane; b < n_bins; b += 64) s_e[b] = edges[b];
    for (int b = lane; b < n_cells; b += 64) s_hist[b] = 0u;
    __syncthreads();

    // No LDS counter wraps: a pair adds at most 2 to a cell (both role assignments of an asymmetric triplet), so a row
    // of k neighbours adds at most k (k - 1) to any cell. `pending` is that bound summed over the rows since the last
    // flush; the cells are flushed before it could pass 2^32 - 1.
    unsigned long long pending = 0;
    auto flush = [&]() {
        __syncthreads();
        for (int b = lane; b < n_cells; b += 64) {
            if (s_hist[b]) atomicAdd(&hist[b], (unsigned long long)s_hist[b]);
            s_hist[b] = 0u;
        }
        __syncthreads();
    };

    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int k = count[row];
        if (k < 2 || k > cap) continue;  // (no pair; an overflowed row adds nothing: the host runs the call again)
        const unsigned long long inc = (unsigned long long)k * (unsigned long long)(k - 1);
        if (pending + inc > 0xFFFFFFFFull) {
            flush();
            pending = 0;
        }
        pending += inc;
        const shell::Row c = shell::row_of(xyz, n, box, centres, row / n_c, (int)(row % n_c));
        const int cc = cen_class[c.c];
        const double *q = planes + (size_t)c.f * 3 * (size_t)n_cand;
        const int *r = idx + (size_t)row * (size_t)cap;
        const int n_tiles = (k + ANG_TILE - 1) / ANG_TILE;
        for (int ta = 0; ta < n_tiles; ++ta) {
            const int ma = k - ta * ANG_TILE < ANG_TILE ? k - ta * ANG_TILE : ANG_TILE;
            __syncthreads();  // (the pairs of the tiles before have been read)
            ang_stage(tj, lane, ma, r + ta * ANG_TILE, q, n_cand, cand_class, cc, tr, c);
            for (int tb = ta; tb < n_tiles; ++tb) {
                const int mb = k - tb * ANG_TILE < ANG_TILE ? k - tb * ANG_TILE : ANG_TILE;
                const bool same = tb == ta;
                if (!same) {
                    __syncthreads();
                    ang_stage(tk, lane, mb, r + tb * ANG_TILE, q, n_cand, cand_class, cc, tr, c);
                }
                __syncthreads();
                AngTile sk;  // (the K tile is the J tile on the diagonal)
                sk.dx = same ? tj.dx : tk.dx, sk.dy = same ? tj.dy : tk.dy, sk.dz = same ? tj.dz : tk.dz;
                sk.nrm = same ? tj.nrm : tk.nrm, sk.mask = same ? tj.mask : tk.mask;
                for (int pi = lane; pi < ma * mb; pi += 64) {
                    const int j = pi / mb, kk = pi - j * mb;
                    if (same && j >= kk) continue;
                    const unsigned mj = tj.mask[j], mk = sk.mask[kk];
                    const unsigned once = mj & mk & tr.sym;                       // symmetric: the unordered pair
                    const unsigned jk = mj & (mk >> 8) & 0xFFu;                   // j in role A, k in role B
                    const unsigned kj = mk & (mj >> 8) & 0xFFu;                   // k in role A, j in role B
                    if (!(once | jk | kj)) continue;
                    const double dot = (tj.dx[j] * sk.dx[kk] + tj.dy[j] * sk.dy[kk]) + tj.dz[j] * sk.dz[kk];
                    const double cs = dot / (tj.nrm[j] * sk.nrm[kk]);
                    int bin = -1;  // NaN: the degenerate count
                    if (cs == cs) {
                        int lo = 0, hi = n_bins;  // cs <= E[m] for every m in [1, lo], not for m = hi (n_bins: none)
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (cs <= s_e[mid]) lo = mid; else hi = mid;
                        }
                        bin = lo;
                    }
#pragma unroll
                    for (int t = 0; t < ANG_MAX_TRIPLETS; ++t) {
                        const unsigned add = ((once >> t) & 1u) + ((jk >> t) & 1u) + ((kj >> t) & 1u);
                        if (add) atomicAdd(&s_hist[bin < 0 ? tr.n * n_bins + t : t * n_bins + bin], add);
                    }
                }
            }
        }
    }
    flush();
}

}  // namespace

extern "C" {

int mdhip_angle_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                     const double *box, int32_t n_centres, const int32_t *centres, const int32_t *centre_class,
                     int32_t n_cand, const int32_t *cand, const int32_t *cand_class, const int32_t *mol_of,
                     int32_t n_triplets, const int32_t *triplet_class, const double *triplet_rsq, int32_t n_bins,
                     const double *cos_edges, int32_t cap, uint64_t *hist, uint64_t *n_degenerate, int32_t *count)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_centres >= 0 && n_cand >= 0, "negative sizes");
    MD_REQUIRE(n_triplets >= 1 && n_triplets <= ANG_MAX_TRIPLETS, "n_triplets must be in [1, %d]", ANG_MAX_TRIPLETS);
    MD_REQUIRE(n_bins >= 1 && (int64_t)n_triplets * n_bins <= ANG_MAX_CELLS,
               "n_triplets * n_bins must be in [1, %d]", ANG_MAX_CELLS);
    shell::RowSet rs;
    int rc;
    if ((rc = shell::take_rows(ctx, n_frames, n_centres, cap, ANG_MAX_CAP, rs))) return rc;
    MD_REQUIRE(triplet_class && triplet_rsq && cos_edges && hist && n_degenerate, "NULL array");
    for (int32_t m = 1; m < n_bins; ++m)
        MD_REQUIRE(cos_edges[m] < cos_edges[m - 1], "cos_edges must be strictly decreasing (edge %d)", (int)m);
    memset(hist, 0, (size_t)n_triplets * (size_t)n_bins * 8);
    memset(n_degenerate, 0, (size_t)n_triplets * 8);
    if (rs.n_rows == 0) return cs.end();
    MD_REQUIRE(centre_class && count, "NULL array");
    MD_REQUIRE(cand || n_cand == 0, "NULL array");
    MD_REQUIRE(cand_class || n_cand == 0, "NULL array");
    if ((rc = shell::check_indices(ctx, "candidate", n_cand, cand, 1, n_atoms))) return rc;

    AngTriplets tr;
    memset(&tr, 0, sizeof tr);
    tr.n = n_triplets;
    double rc2 = 0.0;
    for (int t = 0; t < n_triplets; ++t) {
        tr.ta[t] = triplet_class[3 * t], tr.tc[t] = triplet_class[3 * t + 1], tr.tb[t] = triplet_class[3 * t + 2];
        tr.ra2[t] = triplet_rsq[2 * t], tr.rb2[t] = triplet_rsq[2 * t + 1];
        MD_REQUIRE(tr.ra2[t] >= 0.0 && tr.rb2[t] >= 0.0, "triplet %d: squared cutoffs must not be negative", t);
        if (tr.ta[t] == tr.tb[t] && tr.ra2[t] == tr.rb2[t]) tr.sym |= 1u << t;
        rc2 = std::max(rc2, std::max(tr.ra2[t], tr.rb2[t]));
    }
    shell::Inputs in;
    if ((rc = shell::stage(ctx, "centre", n_frames, n_atoms, xyz, xyz_on_device, box, n_centres, centres, in)))
        return rc;
    if (n_cand == 0) {  // (no atom can be a neighbour: every count is 0)
        if ((rc = shell::row_results(cs, rs, nullptr, count))) return rc;
        return cs.end();
    }

    // the tables: doubles E [n_bins] | largest squared cutoff of every centre's class [n_centres]; ints the centres'
    // classes | the candidates' atoms | their classes | mol_of [n_atoms] (under exclusion)
    const size_t n_dbl = (size_t)n_bins + (size_t)n_centres;
    std::vector<double> h_dbl(n_dbl);
    std::copy(cos_edges, cos_edges + n_bins, h_dbl.begin());
    for (int32_t c = 0; c < n_centres; ++c) {
        double r2 = 0.0;  // (a centre of no triplet's class has no neighbours)
        for (int t = 0; t < n_triplets; ++t)
            if (tr.tc[t] == centre_class[c]) r2 = std::max(r2, std::max(tr.ra2[t], tr.rb2[t]));
        h_dbl[(size_t)n_bins + c] = r2;
    }
    int tests = mol_of ? ANG_TEST_ATOM : 0;
    for (int32_t c = 0; c < n_centres; ++c)
        if (h_dbl[(size_t)n_bins + c] != rc2) tests |= ANG_TEST_RADIUS;
    if (!mol_of && shell::shares_an_atom(n_atoms, centres, n_centres, cand, n_cand)) tests |= ANG_TEST_ATOM;
    MD_WS(d_dbl, double, WS_TABLES, n_dbl * 8);
    if ((rc = mdhip_h2d_small(ctx, d_dbl, h_dbl.data(), n_dbl * 8))) return rc;
    const int *d_cen_class, *d_cand, *d_cand_class, *d_mol;
    shell::IntTable ints;
    ints.add(centre_class, n_centres, &d_cen_class);
    ints.add(cand, n_cand, &d_cand);
    ints.add(cand_class, n_cand, &d_cand_class);
    ints.add_optional(mol_of, n_atoms, &d_mol);
    if ((rc = shell::upload_ints(ctx, ints, WS_TYPE_J))) return rc;
    const double *d_edges = d_dbl, *d_rmax2 = d_dbl + n_bins;

    const size_t n_cells = (size_t)n_triplets * (size_t)n_bins + (size_t)n_triplets;
    double *d_planes;
    if ((rc = shell::planes_room(ctx, n_frames, n_cand, d_planes))) return rc;
    MD_WS(d_hist, unsigned long long, WS_HIST, n_cells * 8);
    MD_HIP(hipMemsetAsync(d_hist, 0, n_cells * 8, ctx->stream));

    KernelTimer timer(ctx, 3);
    KernelTimer search(ctx, 2, true);  // the gather and the search: the call's aux time; the rest is the angle pass
    ctx->last_kernel = "ang_search_kernel";
    if ((rc = shell::gather(ctx, in.xyz, n_frames, n_atoms, d_cand, n_cand, d_planes))) return rc;
    const shell::Grid g = shell::sweep_grid(ctx, n_frames, n_centres, n_cand);
    hipLaunchKernelGGL(ang_search_kernel, dim3(g.grid), dim3(shell::THREADS), 0, ctx->stream, in.xyz,
                       (long long)n_atoms, d_planes, (long long)n_cand, in.box, in.centres, (int)n_centres, d_cand, d_mol,
                       d_rmax2, tests, rc2, (int)cap, g, rs.idx, rs.count);
    MD_HIP(hipGetLastError());
    search.stop();
    const size_t lds = ((size_t)n_bins + 8 * ANG_TILE) * 8 + (n_cells + 2 * ANG_TILE) * 4;
    hipLaunchKernelGGL(ang_pair_kernel, dim3(rs.grid(ctx, 16)), dim3(64), lds, ctx->stream, in.xyz, (long long)n_atoms,
                       d_planes, (long long)n_cand, in.box, in.centres, d_cen_class, (int)n_centres, d_cand_class, rs.idx,
                       rs.count, (long long)rs.n_rows, (int)cap, tr, d_edges, (int)n_bins, d_hist);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, hist, d_hist, (size_t)n_triplets * (size_t)n_bins * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, n_degenerate, d_hist + (size_t)n_triplets * (size_t)n_bins, (size_t)n_triplets * 8, 0)))
        return rc;
    if ((rc = shell::row_results(cs, rs, nullptr, count))) return rc;
    return shell::finish(cs, timer, &search);
}

}  // extern "C"
