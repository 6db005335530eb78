// dihedrals.hip — intramolecular dihedral angles: their distributions and the series behind the torsional
// autocorrelation (structural/dihedral_distribution.py; the reference has no such module).
//
// mdhip_dihedral_angles: per (job, molecule, frame) the torsion i-j-k-l of four named atoms of the molecule, as its
//   cosine c and sine sn (include/mdhip.h states every operation; no acos, no atan2). Counted into hist[row][bin] —
//   bins of 360 / n_bins degrees over [-180, 180), decided on c against the host's cos(m * D) and on the sign of s — and
//   / or written as U[s][.][t] = (c, sn, 0), time-major, so that mdhip_orient_corr sums u(t) . u(t + k) =
//   cos(phi(t + k) - phi(t)) at every lag.
//   Tile, job plan and launch are those of mol_tile.h, with two components in the LDS tile (the third row of a series
//   is zeros) and the jobs over the same molecules pooled into classes (the five O-C-C-O torsions of a tetraglyme);
//   here: what a lane computes per (molecule, frame), and the histogram.
//   Counts go to a workgroup's LDS histogram (n_rows * n_bins 32-bit cells, 32-bit integer LDS atomics) that is added
//   ONCE to the 64-bit device bins with integer atomics: exact whatever the order, no floating-point atomics.
//   One job per molecule type runs at the HBM rate; every further job of a class costs about 0.7 of that again, paced
//   by the lane-strided loads through the caches.
#include <algorithm>
#include <cmath>
#include <vector>

#include "call_tables.h"
#include "ctx.h"
#include "mol_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr size_t DH_TILE_LDS = mt_tile_lds(2);
constexpr int DH_MAX_ROWS = 16;
constexpr int DH_MAX_BINS = 1440;
constexpr int DH_CLASS_JOBS = 1 << 16;  // jobs per class: 2^16 * 64 * 64 counts fit a 32-bit cell
static_assert(DH_TILE_LDS + (size_t)DH_MAX_ROWS * DH_MAX_BINS * 4 <= 160 * 1024, "tile and histogram must fit LDS");
static_assert(DH_TILE_LDS % 16 == 0, "the histogram behind the tile stays aligned");

struct DhJob {  // by position in the plan
    long long series0;  // first series of the job
    int q[4];           // the atoms i j k l inside the molecule
    int row, index;     // histogram row; the job's number in the call (degenerate[index])
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

// Dynamic LDS: [the tile, when U] [n_cells 32-bit counters, when hist].
__global__ __launch_bounds__(MT_THREADS) void dihedral_kernel(
    const double *__restrict__ x, const double *__restrict__ box, long long F, long long A,
    const MolClass *__restrict__ classes, int n_classes, const DhJob *__restrict__ jobs,
    const double *__restrict__ cos_edges, int n_bins, int n_cells, long long tile_base, long long ftile_base,
    unsigned long long *__restrict__ hist, double *__restrict__ U, unsigned long long *__restrict__ degenerate)
{
    extern __shared__ double s_dyn[];
    double *const s_u = s_dyn;  // [2][MT_TM][MT_ROW]
    unsigned int *const s_h = reinterpret_cast<unsigned int *>(s_dyn + (U ? 2 * MT_TM * MT_ROW : 0));
    const MolTile t = mt_locate(classes, n_classes, tile_base, ftile_base, F);
    const int nb2 = n_bins >> 1;
    // where the walk along the edges starts: a float estimate of |phi| / D. Any start gives the same bin.
    const float guess_scale = (float)nb2 * 0.31830988618f;
    if (hist) {
        for (int i = threadIdx.x; i < n_cells; i += MT_THREADS) s_h[i] = 0u;
        __syncthreads();
    }
    for (int jj = 0; jj < t.cls.n_jobs; ++jj) {
        const DhJob job = jobs[t.cls.job0 + jj];
        mt_walk(t, degenerate + job.index, [&](long long a, long long f, int ff, unsigned long long &zeros) {
            double b1[3], b2[3], b3[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double *__restrict__ plane = x + ((size_t)f * 3 + ax) * (size_t)A + a;
                const double xi = plane[job.q[0]], xj = plane[job.q[1]], xk = plane[job.q[2]], xl = plane[job.q[3]];
                double d1 = xj - xi, d2 = xk - xj, d3 = xl - xk;
                if (box) {
                    const double L = box[f * 3 + ax], half = L / 2;
                    d1 = mt_wrap(d1, L, half), d2 = mt_wrap(d2, L, half), d3 = mt_wrap(d3, L, half);
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
                s_u[mt_at(0, t.lane, ff)] = u0;
                s_u[mt_at(1, t.lane, ff)] = u1;
            }
        });
        if (U) {
            __syncthreads();
            mt_store<2>(t, s_u, job.series0, F, U);
            __syncthreads();  // the next job fills the tile again
        }
    }
    if (hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_cells; i += MT_THREADS) {
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
    const MolPlan plan = mol_plan(n_jobs, job_atom0, job_mols, job_len, n_atoms, n_frames, true, DH_CLASS_JOBS);
    std::vector<DhJob> jobs((size_t)n_jobs);  // in call order, then by position
    for (int j = 0; j < plan.checked_jobs(); ++j) {
        MD_REQUIRE(job_row[j] >= 0 && job_row[j] < n_rows, "job %d: job_row must be in [0, n_rows)", j);
        const int32_t *q = job_quad + (size_t)j * 4;
        for (int p = 0; p < 4; ++p) {
            MD_REQUIRE(q[p] >= 0 && q[p] < job_len[j], "job %d: the quadruple's atoms must be in [0, job_len)", j);
            for (int r = 0; r < p; ++r) MD_REQUIRE(q[r] != q[p], "job %d: the quadruple names an atom twice", j);
        }
        jobs[(size_t)j] = {plan.series0[(size_t)j], {q[0], q[1], q[2], q[3]}, job_row[j], j};
    }
    int rc;
    if ((rc = mt_plan_error(ctx, plan, n_atoms))) return rc;
    std::vector<DhJob> sorted((size_t)n_jobs);
    for (int p = 0; p < n_jobs; ++p) sorted[(size_t)p] = jobs[(size_t)plan.order[(size_t)p]];
    const int n_classes = (int)plan.classes.size();
    MolIo io;
    if ((rc = io.open(ctx, n_frames, n_atoms, x, x_on_device, box, U, U_on_device, plan.series))) return rc;
    const MolClass *d_cls;
    const DhJob *d_jobs;
    const double *d_edges;
    unsigned long long *d_deg;
    CallTables tab;
    tab.add(plan.classes.data(), (size_t)n_classes, &d_cls);
    tab.add(sorted.data(), (size_t)n_jobs, &d_jobs);
    tab.add_optional(hist ? cos_edges : nullptr, (size_t)nb2, &d_edges);
    tab.add_zeroed((size_t)n_jobs, &d_deg);
    if ((rc = upload_tables(ctx, tab, WS_TABLES))) return rc;
    const int n_cells = hist ? n_rows * n_bins : 0;
    const size_t hist_b = (size_t)n_cells * 8;
    unsigned long long *d_hist = nullptr;
    if (hist) {
        d_hist = (unsigned long long *)mdhip_ws(ctx, WS_HIST, hist_b);
        if (!d_hist) return MDHIP_ENOMEM;
        MD_HIP(hipMemsetAsync(d_hist, 0, hist_b, ctx->stream));
    }
    const size_t lds = (U ? DH_TILE_LDS : 0) + (size_t)n_cells * 4;
    MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dihedral_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(DH_TILE_LDS + (size_t)DH_MAX_ROWS * DH_MAX_BINS * 4)));
    KernelTimer timer(ctx, 0);
    rc = mt_launch(ctx, "dihedral_kernel", timer, plan.tiles, n_frames, [&](dim3 grid, long long t0, long long ft0) {
        hipLaunchKernelGGL(dihedral_kernel, grid, dim3(MT_THREADS), lds, ctx->stream, io.x, io.box, (long long)n_frames,
                           (long long)n_atoms, d_cls, n_classes, d_jobs, d_edges, n_bins, n_cells, t0, ft0, d_hist, io.U.dev,
                           d_deg);
    });
    if (rc) return rc;
    if ((rc = io.U.deliver(cs))) return rc;
    if (hist && (rc = mdhip_result(cs, hist, d_hist, hist_b, 0))) return rc;
    if ((rc = mdhip_result(cs, degenerate, d_deg, (size_t)n_jobs * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
