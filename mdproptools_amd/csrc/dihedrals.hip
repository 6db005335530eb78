// dihedrals.hip — intramolecular dihedral angles: their distributions and the series behind the torsional
// autocorrelation (structural/dihedral_distribution.py; the reference has no such module).
//
// mdhip_dihedral_angles: per (job, molecule, frame) the torsion i-j-k-l of four named atoms of the molecule, as its
//   cosine c and sine sn (include/mdhip.h states every operation; no acos, no atan2). Counted into hist[row][bin] —
//   bins of 360 / n_bins degrees over [-180, 180), decided on c against the host's cos(m * D) and on the sign of s — and
//   / or written as U[s][.][t] = (c, sn, 0), time-major, so that mdhip_orient_corr sums u(t) . u(t + k) =
//   cos(phi(t + k) - phi(t)) at every lag.
//   The tile is that of axis_vectors_kernel (reorient.hip): a workgroup owns DH_TM = 64 molecules x DH_TF = 64 frames.
//   Lane = molecule while reading (consecutive lanes read atoms one molecule apart, every fetched line is used by the
//   neighbouring lanes), the two finished components go through an LDS tile ([2][64][64 + 1], conflict-free both
//   ways), lane = frame while writing (512 contiguous bytes per wave and row; the third row of a series is zeros).
//   Counts go to a workgroup's LDS histogram (n_rows * n_bins 32-bit cells, 32-bit integer LDS atomics) that is added
//   ONCE to the 64-bit device bins with integer atomics: exact whatever the order, no floating-point atomics.
//   Jobs over the same molecules (same first atom, count and length: the five O-C-C-O torsions of a tetraglyme) form
//   a CLASS: its tiles are worked by one workgroup, job after job, so the lines of a tile come from HBM once and from
//   the caches for the other jobs. One read of the lines that hold named atoms, one write of U when asked: one job
//   per molecule type runs at the HBM rate; every further job of a class costs about 0.7 of that again, paced by
//   the lane-strided loads through the caches.
#include <algorithm>
#include <cmath>
#include <map>
#include <tuple>
#include <vector>

#include "ctx.h"

#pragma clang fp contract(off)

namespace {

constexpr int DH_TM = 64;           // molecules per tile
constexpr int DH_TF = 64;           // frames per tile
constexpr int DH_WAVES = 16;
constexpr int DH_THREADS = 64 * DH_WAVES;
constexpr int DH_ROW = DH_TF + 1;   // doubles per (component, molecule) row of the LDS tile
constexpr size_t DH_TILE_LDS = (size_t)2 * DH_TM * DH_ROW * 8;
constexpr int DH_MAX_ROWS = 16;
constexpr int DH_MAX_BINS = 1440;
constexpr int DH_CLASS_JOBS = 1 << 16;  // jobs per class: 2^16 * 64 * 64 counts fit a 32-bit cell
constexpr long long DH_MAX_GRID = 65535;
static_assert(DH_TILE_LDS + (size_t)DH_MAX_ROWS * DH_MAX_BINS * 4 <= 160 * 1024, "tile and histogram must fit LDS");
static_assert(DH_TILE_LDS % 16 == 0, "the histogram behind the tile stays aligned");

struct DhJob {
    long long series0;  // first series of the job
    int q[4];           // the atoms i j k l inside the molecule
    int row, index;     // histogram row; the job's number in the call (degenerate[index])
};

struct DhClass {
    long long atom0, mols, tile0;  // first atom, molecules, first molecule tile of the class
    int len, job0, n_jobs, pad;    // atoms per molecule; its jobs are d_jobs[job0 .. job0 + n_jobs)
};

__device__ __forceinline__ double dh_dot(const double *a, const double *b)
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ void dh_cross(const double *a, const double *b, double *n)
{
    n[0] = a[1] * b[2] - a[2] * b[1];
    n[1] = a[2] * b[0] - a[0] * b[2];
    n[2] = a[0] * b[1] - a[1] * b[0];
}

// Block (x, y): molecule tile tile_base + x (over all classes), frame tile ftile_base + y.
// Dynamic LDS: [the tile, when U] [n_cells 32-bit counters, when hist].
__global__ __launch_bounds__(DH_THREADS) void dihedral_kernel(const double *__restrict__ x, const double *__restrict__ box,
                                                              long long F, long long A,
                                                              const DhClass *__restrict__ classes, int n_classes,
                                                              const DhJob *__restrict__ jobs,
                                                              const double *__restrict__ cos_edges, int n_bins,
                                                              int n_cells, long long tile_base, long long ftile_base,
                                                              unsigned long long *__restrict__ hist,
                                                              double *__restrict__ U,
                                                              unsigned long long *__restrict__ degenerate)
{
    extern __shared__ double s_dyn[];
    double *const s_u = s_dyn;  // [2][DH_TM][DH_ROW]
    unsigned int *const s_h = reinterpret_cast<unsigned int *>(s_dyn + (U ? 2 * DH_TM * DH_ROW : 0));
    const long long tile = tile_base + blockIdx.x;
    int lo = 0, hi = n_classes - 1;  // the last class whose first tile is not beyond this one (empty classes have none)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (classes[mid].tile0 <= tile) lo = mid;
        else hi = mid - 1;
    }
    const DhClass cls = classes[lo];
    const long long m0 = (tile - cls.tile0) * DH_TM;
    const int nm = (int)(cls.mols - m0 < DH_TM ? cls.mols - m0 : DH_TM);
    const long long f0 = (ftile_base + blockIdx.y) * DH_TF;
    const int nf = (int)(F - f0 < DH_TF ? F - f0 : DH_TF);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb2 = n_bins >> 1;
    // where the walk along the edges starts: a float estimate of |phi| / D. Any start gives the same bin.
    const float guess_scale = (float)nb2 * 0.31830988618f;
    if (hist) {
        for (int i = threadIdx.x; i < n_cells; i += DH_THREADS) s_h[i] = 0u;
        __syncthreads();
    }
    for (int jj = 0; jj < cls.n_jobs; ++jj) {
        const DhJob job = jobs[cls.job0 + jj];
        if (lane < nm) {
            const long long a = cls.atom0 + (m0 + lane) * cls.len;
            unsigned long long zeros = 0;
            for (int ff = wave; ff < nf; ff += DH_WAVES) {
                const long long f = f0 + ff;
                double b1[3], b2[3], b3[3];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double *__restrict__ plane = x + ((size_t)f * 3 + ax) * (size_t)A + a;
                    const double xi = plane[job.q[0]], xj = plane[job.q[1]], xk = plane[job.q[2]], xl = plane[job.q[3]];
                    double d1 = xj - xi, d2 = xk - xj, d3 = xl - xk;
                    if (box) {  // the single strict wrap of the siblings; a NaN shifts nothing
                        const double L = box[f * 3 + ax], half = L / 2;
                        if (d1 > half) d1 -= L;
                        else if (d1 < -half) d1 += L;
                        if (d2 > half) d2 -= L;
                        else if (d2 < -half) d2 += L;
                        if (d3 > half) d3 -= L;
                        else if (d3 < -half) d3 += L;
                    }
                    b1[ax] = d1, b2[ax] = d2, b3[ax] = d3;
                }
                double n1[3], n2[3];
                dh_cross(b1, b2, n1);
                dh_cross(b2, b3, n2);
                const double l1 = __builtin_sqrt(dh_dot(n1, n1)), l2 = __builtin_sqrt(dh_dot(n2, n2));
                const double lb = __builtin_sqrt(dh_dot(b2, b2));
                const double den = l1 * l2;
                const double c = dh_dot(n1, n2) / den;
                const double s = dh_dot(b1, n2);
                const double sn = (s * lb) / den;
                double u0, u1;
                if (den == 0.0) {
                    u0 = u1 = 0.0;
                    ++zeros;
                } else if (c != c || s != s) {
                    u0 = u1 = __builtin_nan("");
                } else {
                    u0 = c, u1 = sn;
                    if (hist) {
                        // m = the number of q in [1, nb2) with c <= cos_edges[q] (strictly decreasing): walk from the guess
                        const float cf = __builtin_fminf(1.0f, __builtin_fmaxf(-1.0f, (float)c));
                        int m = (int)(acosf(cf) * guess_scale);
                        m = m < 0 ? 0 : (m > nb2 - 1 ? nb2 - 1 : m);
                        while (m + 1 < nb2 && c <= cos_edges[m + 1]) ++m;
                        while (m > 0 && !(c <= cos_edges[m])) --m;
                        const int bin = s >= 0.0 ? nb2 + m : nb2 - 1 - m;
                        atomicAdd(s_h + job.row * n_bins + bin, 1u);
                    }
                }
                if (U) {
                    s_u[(0 * DH_TM + lane) * DH_ROW + ff] = u0;
                    s_u[(1 * DH_TM + lane) * DH_ROW + ff] = u1;
                }
            }
            if (zeros) atomicAdd(degenerate + job.index, zeros);
        }
        if (U) {
            __syncthreads();
            for (int row = wave; row < 3 * nm; row += DH_WAVES) {
                const int mol = row / 3, comp = row - 3 * mol;
                if (lane < nf)
                    U[((size_t)(job.series0 + m0 + mol) * 3 + comp) * (size_t)F + (size_t)(f0 + lane)] =
                        comp < 2 ? s_u[(comp * DH_TM + mol) * DH_ROW + lane] : 0.0;
            }
            __syncthreads();  // the next job fills the tile again
        }
    }
    if (hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_cells; i += DH_THREADS) {
            const unsigned int n = s_h[i];
            if (n) atomicAdd(hist + i, (unsigned long long)n);
        }
    }
}

}  // namespace

extern "C" {

int mdhip_dihedral_angles(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                          const double *box, int n_jobs, const int64_t *job_atom0, const int64_t *job_mols,
                          const int32_t *job_len, const int32_t *job_quad, const int32_t *job_row, int n_rows, int n_bins,
                          const double *cos_edges, uint64_t *hist, double *U, int U_on_device, uint64_t *degenerate)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_jobs >= 1 && n_jobs <= (1 << 20), "n_jobs must be in [1, 2^20]");
    MD_REQUIRE(n_rows >= 1 && n_rows <= DH_MAX_ROWS, "n_rows must be in [1, %d]", DH_MAX_ROWS);
    MD_REQUIRE(n_bins >= 2 && n_bins <= DH_MAX_BINS && n_bins % 2 == 0, "n_bins must be even and in [2, %d]", DH_MAX_BINS);
    MD_REQUIRE(n_frames >= 1 && n_atoms >= 1, "n_frames and n_atoms must be positive");
    MD_REQUIRE(n_atoms < (1ll << 40) && n_frames < (1ll << 31) && n_frames < (1ll << 40) / n_atoms, "trajectory too large");
    MD_REQUIRE(x && job_atom0 && job_mols && job_len && job_quad && job_row && degenerate, "NULL array");
    MD_REQUIRE(hist || U, "hist and U are both NULL: nothing to compute");
    MD_REQUIRE(!hist || cos_edges, "cos_edges is NULL while hist is not");
    const int nb2 = n_bins / 2;
    if (hist)
        for (int q = 1; q < nb2; ++q)
            MD_REQUIRE(cos_edges[q] < cos_edges[q - 1], "cos_edges must descend strictly (entry %d)", q);
    // classes: the jobs over the same molecules, in the order in which their first job comes
    std::vector<DhJob> jobs((size_t)n_jobs);
    std::vector<int> class_of((size_t)n_jobs);
    std::vector<DhClass> classes;
    std::map<std::tuple<long long, long long, long long>, int> open;  // (atom0, mols, len) -> the class still taking jobs
    long long series = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const long long len = job_len[j], mols = job_mols[j], a0 = job_atom0[j];
        MD_REQUIRE(len >= 1 && mols >= 0 && a0 >= 0 && a0 <= n_atoms && mols <= (n_atoms - a0) / len,
                   "job %d runs past the %lld atoms of a frame", j, (long long)n_atoms);
        MD_REQUIRE(job_row[j] >= 0 && job_row[j] < n_rows, "job %d: job_row must be in [0, n_rows)", j);
        const int32_t *q = job_quad + (size_t)j * 4;
        for (int p = 0; p < 4; ++p) {
            MD_REQUIRE(q[p] >= 0 && q[p] < len, "job %d: the quadruple's atoms must be in [0, job_len)", j);
            for (int r = 0; r < p; ++r) MD_REQUIRE(q[r] != q[p], "job %d: the quadruple names an atom twice", j);
        }
        const auto key = std::make_tuple(a0, mols, len);
        auto it = open.find(key);
        if (it == open.end() || classes[(size_t)it->second].n_jobs == DH_CLASS_JOBS) {
            classes.push_back({a0, mols, 0, (int)len, 0, 0, 0});
            it = open.insert_or_assign(key, (int)classes.size() - 1).first;
        }
        class_of[(size_t)j] = it->second;
        ++classes[(size_t)it->second].n_jobs;
        jobs[(size_t)j] = {series, {q[0], q[1], q[2], q[3]}, job_row[j], j};
        series += mols;
    }
    MD_REQUIRE(series < (1ll << 40) / n_frames, "result too large");
    long long tiles = 0;
    int first = 0;
    for (DhClass &c : classes) {
        c.tile0 = tiles;
        c.job0 = first;
        tiles += (c.mols + DH_TM - 1) / DH_TM;
        first += c.n_jobs;
        c.n_jobs = 0;  // (counted again while the jobs are put in place)
    }
    std::vector<DhJob> sorted((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        DhClass &c = classes[(size_t)class_of[(size_t)j]];
        sorted[(size_t)(c.job0 + c.n_jobs++)] = jobs[(size_t)j];
    }
    const int n_classes = (int)classes.size();
    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const size_t x_bytes = (size_t)n_frames * 3 * (size_t)n_atoms * 8;
    const double *d_x = (const double *)mdhip_stage(ctx, WS_XYZ_I, x, x_bytes, x_on_device, &rc);
    if (rc) return rc;
    const double *d_box = nullptr;
    if (box) {
        MD_WS(d_b, double, WS_BOX, (size_t)n_frames * 3 * 8);
        if ((rc = mdhip_h2d_small(ctx, d_b, box, (size_t)n_frames * 3 * 8))) return rc;
        d_box = d_b;
    }
    // tables: classes | jobs | edges | degenerate counters
    const size_t cls_b = (size_t)n_classes * sizeof(DhClass), jobs_b = (size_t)n_jobs * sizeof(DhJob);
    const size_t edge_b = hist ? (size_t)nb2 * 8 : 0, deg_b = (size_t)n_jobs * 8;
    MD_WS(d_tab, char, WS_TABLES, cls_b + jobs_b + edge_b + deg_b);
    if ((rc = mdhip_h2d_small(ctx, d_tab, classes.data(), cls_b))) return rc;
    if ((rc = mdhip_h2d_small(ctx, d_tab + cls_b, sorted.data(), jobs_b))) return rc;
    if (hist && (rc = mdhip_h2d_small(ctx, d_tab + cls_b + jobs_b, cos_edges, edge_b))) return rc;
    unsigned long long *d_deg = (unsigned long long *)(d_tab + cls_b + jobs_b + edge_b);
    MD_HIP(hipMemsetAsync(d_deg, 0, deg_b, ctx->stream));
    const int n_cells = hist ? n_rows * n_bins : 0;
    const size_t hist_b = (size_t)n_cells * 8;
    unsigned long long *d_hist = nullptr;
    if (hist) {
        d_hist = (unsigned long long *)mdhip_ws(ctx, WS_HIST, hist_b);
        if (!d_hist) return MDHIP_ENOMEM;
        MD_HIP(hipMemsetAsync(d_hist, 0, hist_b, ctx->stream));
    }
    const size_t u_bytes = U ? (size_t)series * 3 * (size_t)n_frames * 8 : 0;
    double *d_U = U;
    if (U && !U_on_device) {
        d_U = (double *)mdhip_ws(ctx, WS_OUT, std::max<size_t>(u_bytes, 8));
        if (!d_U) return MDHIP_ENOMEM;
    }
    const size_t lds = (U ? DH_TILE_LDS : 0) + (size_t)n_cells * 4;
    MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dihedral_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(DH_TILE_LDS + (size_t)DH_MAX_ROWS * DH_MAX_BINS * 4)));
    KernelTimer timer(ctx, 0);
    int launches = 0;
    const long long f_tiles = (n_frames + DH_TF - 1) / DH_TF;
    // (launch dimensions stay within 65 535: more tiles go in several launches)
    for (long long t0 = 0; t0 < tiles; t0 += DH_MAX_GRID)
        for (long long ft0 = 0; ft0 < f_tiles; ft0 += DH_MAX_GRID, ++launches) {
            const dim3 grid((unsigned)std::min(DH_MAX_GRID, tiles - t0), (unsigned)std::min(DH_MAX_GRID, f_tiles - ft0));
            hipLaunchKernelGGL(dihedral_kernel, grid, dim3(DH_THREADS), lds, ctx->stream, d_x, d_box, (long long)n_frames,
                               (long long)n_atoms, (const DhClass *)d_tab, n_classes, (const DhJob *)(d_tab + cls_b),
                               (const double *)(d_tab + cls_b + jobs_b), n_bins, n_cells, t0, ft0, d_hist, d_U, d_deg);
            MD_HIP(hipGetLastError());
        }
    ctx->last_kernel = "dihedral_kernel";
    ctx->last_launches = launches;
    timer.stop();
    if (U && !U_on_device && (rc = mdhip_result(cs, U, d_U, u_bytes, 0))) return rc;
    if (hist && (rc = mdhip_result(cs, hist, d_hist, hist_b, 0))) return rc;
    if ((rc = mdhip_result(cs, degenerate, d_deg, deg_b, 0))) return rc;
    cs.defer([timer]() {
        timer.collect();
        return MDHIP_OK;
    });
    return cs.end();
}

}  // extern "C"
