// moments.hip — per-molecule sites and vectors, frame-major, and the per-frame totals of the vectors
// (structural/orientational_correlation.py, structural/dielectric.py). include/mdhip.h states every operation.
//
// mdhip_mol_moments: site[f][x][s] = x[a] + sum_k w_k * w(x[a+k] - x[a]) over the job's site terms, vec[f][x][s] the same
//   sum over its vector terms (normalised when job_unit says so): the per-molecule pass in front of
//   mdhip_vector_pair_hist. Job plan, tile walk, wrap and launch are those of mol_tile.h, every job a class of its own:
//   lane = molecule, wave = frame. Unlike the series kernels the outputs are FRAME-major, so a wave writes the 64
//   consecutive molecules it read: no LDS tile stands between reading and writing. One read of the lines that hold
//   named atoms, one write of the two outputs: HBM-bound.
// moments_total_kernel: total[j][x][f] and sq_total[j][f] from the vectors as written. One workgroup per (frame, job):
//   lane i adds the molecules i, i + 256, ... of the job in order, then a fixed tree over the 256 partial sums — the
//   scheme of collective_kernel (collective.hip): the order depends on the job's size alone, every call gives the same bits.
#include <algorithm>
#include <vector>

#include "call_tables.h"
#include "ctx.h"
#include "mol_tile.h"

#pragma clang fp contract(off)

namespace {

struct MmJob {  // by position in the plan (= the job's number: nothing is pooled)
    long long series0;  // first series of the job
    int site0, n_site;  // its site terms and its vector terms in the term table
    int vec0, n_vec;
    int unit, pad;
};

// sum_k w_k * w(plane[k] - xa) in ascending k, starting from w_1 * d_1; 0 without terms
__device__ __forceinline__ double mm_sum(const double *__restrict__ plane, double xa, bool wrap, double L, double half,
                                         const int *__restrict__ term_atom, const double *__restrict__ term_w, int t0, int n)
{
    double acc = 0.0;
    for (int k = 0; k < n; ++k) {
        double d = plane[term_atom[t0 + k]] - xa;
        if (wrap) d = mt_wrap(d, L, half);
        const double p = term_w[t0 + k] * d;
        acc = k == 0 ? p : acc + p;
    }
    return acc;
}

__global__ __launch_bounds__(MT_THREADS) void mol_moments_kernel(
    const double *__restrict__ x, const double *__restrict__ box, long long F, long long A, long long S,
    const MolClass *__restrict__ classes, int n_classes, const MmJob *__restrict__ jobs, const int *__restrict__ term_atom,
    const double *__restrict__ term_w, long long tile_base, long long ftile_base, double *__restrict__ site,
    double *__restrict__ vec, unsigned long long *__restrict__ degenerate)
{
    const MolTile t = mt_locate(classes, n_classes, tile_base, ftile_base, F);
    const MmJob job = jobs[t.cls.job0];
    const long long s = job.series0 + t.m0 + t.lane;
    mt_walk(t, degenerate + t.cls.job0, [&](long long a, long long f, int, unsigned long long &zeros) {
        double o[3], v[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double *__restrict__ plane = x + ((size_t)f * 3 + ax) * (size_t)A + a;
            const double xa = plane[0];
            const double L = box ? box[f * 3 + ax] : 0.0, half = L / 2;
            const double off = mm_sum(plane, xa, box != nullptr, L, half, term_atom, term_w, job.site0, job.n_site);
            o[ax] = job.n_site ? xa + off : xa;
            v[ax] = mm_sum(plane, xa, box != nullptr, L, half, term_atom, term_w, job.vec0, job.n_vec);
        }
        if (job.unit && job.n_vec) {
            const double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
            if (n2 == 0.0) {
                v[0] = v[1] = v[2] = 0.0;
                ++zeros;
            } else if (!(__builtin_fabs(n2) < __builtin_inf())) {
                v[0] = v[1] = v[2] = __builtin_nan("");
            } else {
                const double r = __builtin_sqrt(n2);
                v[0] = v[0] / r, v[1] = v[1] / r, v[2] = v[2] / r;
            }
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const size_t at = ((size_t)f * 3 + ax) * (size_t)S + (size_t)s;
            if (site) site[at] = o[ax];
            if (vec) vec[at] = v[ax];
        }
    });
}

constexpr int MM_THREADS = 256;

// Block (x, y): frame f0 + x, job job0 + y. The three axis sums and the sum of squares of the job's vectors at that frame.
__global__ __launch_bounds__(MM_THREADS) void moments_total_kernel(const double *__restrict__ vec, long long F, long long S,
                                                                   const MmJob *__restrict__ jobs,
                                                                   const MolClass *__restrict__ classes, long long f0,
                                                                   int job0, double *__restrict__ total,
                                                                   double *__restrict__ sq_total)
{
    __shared__ double s_red[4][MM_THREADS];
    const long long f = f0 + blockIdx.x;
    const int job = job0 + (int)blockIdx.y;
    const long long s0 = jobs[job].series0, n = classes[job].mols;
    const double *__restrict__ vx = vec + (size_t)f * 3 * (size_t)S + (size_t)s0;
    const double *__restrict__ vy = vx + S, *__restrict__ vz = vy + S;
    double sx = 0.0, sy = 0.0, sz = 0.0, sq = 0.0;
    for (long long m = threadIdx.x; m < n; m += MM_THREADS) {
        const double a = vx[m], b = vy[m], c = vz[m];
        sx += a, sy += b, sz += c;
        sq += (a * a + b * b) + c * c;
    }
    s_red[0][threadIdx.x] = sx, s_red[1][threadIdx.x] = sy, s_red[2][threadIdx.x] = sz, s_red[3][threadIdx.x] = sq;
    __syncthreads();
    for (int half = MM_THREADS / 2; half; half >>= 1) {
        if ((int)threadIdx.x < half) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s_red[q][threadIdx.x] += s_red[q][threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3 && total) total[((size_t)job * 3 + threadIdx.x) * (size_t)F + (size_t)f] = s_red[threadIdx.x][0];
    if (threadIdx.x == 3 && sq_total) sq_total[(size_t)job * (size_t)F + (size_t)f] = s_red[3][0];
}

}  // namespace

extern "C" {

int mdhip_mol_moments(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device,
                      const double *box, int n_jobs, const int64_t *job_atom0, const int64_t *job_mols,
                      const int32_t *job_len, const int64_t *site_off, const int32_t *site_atom, const double *site_w,
                      const int64_t *vec_off, const int32_t *vec_atom, const double *vec_w, const int32_t *job_unit,
                      double *site, double *vec, int out_on_device, double *total, double *sq_total,
                      uint64_t *degenerate)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_jobs >= 1 && n_jobs <= (1 << 20), "n_jobs must be in [1, 2^20]");
    MD_REQUIRE(n_frames >= 1 && n_atoms >= 1, "n_frames and n_atoms must be positive");
    MD_REQUIRE(n_atoms < (1ll << 40) && n_frames < (1ll << 31) && n_frames < (1ll << 40) / n_atoms, "trajectory too large");
    MD_REQUIRE(x && job_atom0 && job_mols && job_len && site_off && vec_off && job_unit && degenerate, "NULL array");
    MD_REQUIRE(site_off[0] == 0 && vec_off[0] == 0, "site_off and vec_off must start at 0");
    const MolPlan plan = mol_plan(n_jobs, job_atom0, job_mols, job_len, n_atoms, n_frames, false, 1);
    std::vector<MmJob> jobs((size_t)n_jobs);
    std::vector<int> t_atom;
    std::vector<double> t_w;
    for (int j = 0; j < plan.checked_jobs(); ++j) {
        const long long len = job_len[j];
        MD_REQUIRE(job_unit[j] == 0 || job_unit[j] == 1, "job %d: job_unit must be 0 or 1", j);
        MmJob &J = jobs[(size_t)j];
        J = {plan.series0[(size_t)j], 0, 0, 0, 0, job_unit[j], 0};
        for (int list = 0; list < 2; ++list) {
            const int64_t *off = list ? vec_off : site_off;
            const int32_t *atom = list ? vec_atom : site_atom;
            const double *w = list ? vec_w : site_w;
            const long long t0 = off[j], t1 = off[j + 1];
            MD_REQUIRE(t1 >= t0 && t1 - t0 < len && t1 <= (1ll << 29), "job %d takes at most job_len - 1 %s terms", j,
                       list ? "vector" : "site");
            MD_REQUIRE(t1 == t0 || (atom && w), "NULL term array");
            if (int rc = mt_terms_ascend(ctx, j, atom, t0, t1, len)) return rc;
            (list ? J.vec0 : J.site0) = (int)t_atom.size();
            (list ? J.n_vec : J.n_site) = (int)(t1 - t0);
            if (t1 > t0) {  // (a NULL array may stand for empty lists)
                t_atom.insert(t_atom.end(), atom + t0, atom + t1);
                t_w.insert(t_w.end(), w + t0, w + t1);
            }
        }
    }
    int rc;
    if ((rc = mt_plan_error(ctx, plan, n_atoms))) return rc;
    const long long S = plan.series;
    MolIo io;
    if ((rc = io.open(ctx, n_frames, n_atoms, x, x_on_device, box, nullptr, 0, S))) return rc;
    // the totals read the vectors back, so they are written somewhere whenever a total is asked for
    const bool totals = total || sq_total;
    const size_t out_b = (size_t)n_frames * 3 * (size_t)S * 8;
    MolOut o_site, o_vec;
    if ((rc = o_site.open(ctx, WS_OUT, site, out_on_device, out_b))) return rc;
    if ((rc = o_vec.open(ctx, WS_OUT2, vec, out_on_device, out_b, totals))) return rc;
    const MolClass *d_cls;
    const MmJob *d_jobs;
    const double *d_w;
    const int *d_atom;
    unsigned long long *d_deg;
    CallTables tab;
    tab.add(plan.classes.data(), (size_t)n_jobs, &d_cls);
    tab.add(jobs.data(), (size_t)n_jobs, &d_jobs);
    tab.add(t_w.data(), t_w.size(), &d_w);
    tab.add(t_atom.data(), t_atom.size(), &d_atom);
    tab.add_zeroed((size_t)n_jobs, &d_deg);
    if ((rc = upload_tables(ctx, tab, WS_TABLES))) return rc;
    const size_t tot_b = (size_t)n_jobs * 3 * (size_t)n_frames * 8, sq_b = (size_t)n_jobs * (size_t)n_frames * 8;
    double *d_total = nullptr, *d_sq = nullptr;
    if (totals) {
        d_total = (double *)mdhip_ws(ctx, WS_PART, tot_b + sq_b);
        if (!d_total) return MDHIP_ENOMEM;
        d_sq = d_total + tot_b / 8;
    }
    KernelTimer timer(ctx, 0);
    rc = mt_launch(ctx, "mol_moments_kernel", timer, plan.tiles, n_frames, [&](dim3 grid, long long t0, long long ft0) {
        hipLaunchKernelGGL(mol_moments_kernel, grid, dim3(MT_THREADS), 0, ctx->stream, io.x, io.box, (long long)n_frames,
                           (long long)n_atoms, S, d_cls, n_jobs, d_jobs, d_atom, d_w, t0, ft0, o_site.dev, o_vec.dev, d_deg);
    });
    if (rc) return rc;
    if (totals) {
        // (they are not counted in last_launches)
        rc = mt_launch_totals(ctx, n_frames, n_jobs, [&](dim3 grid, long long f0, int j0) {
            hipLaunchKernelGGL(moments_total_kernel, grid, dim3(MM_THREADS), 0, ctx->stream, (const double *)o_vec.dev,
                               (long long)n_frames, S, d_jobs, d_cls, f0, j0, d_total, d_sq);
        });
        if (rc < 0) return rc;
        if (total && (rc = mdhip_result(cs, total, d_total, tot_b, 0))) return rc;
        if (sq_total && (rc = mdhip_result(cs, sq_total, d_sq, sq_b, 0))) return rc;
    }
    if ((rc = o_site.deliver(cs))) return rc;
    if ((rc = o_vec.deliver(cs))) return rc;
    if ((rc = mdhip_result(cs, degenerate, d_deg, (size_t)n_jobs * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
