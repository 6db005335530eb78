// mol_shape.hip — the shape of flexible molecules (structural/molecular_shape.py; the reference has no such module):
// per (job, molecule, frame) the mass-weighted gyration tensor about the centre of mass, Rg^2, the end-to-end distance
// squared, the invariant I2 and the relative shape anisotropy kappa^2, and the principal moments by cyclic Jacobi.
// include/mdhip.h (mdhip_mol_shape) states every operation; tests/shape_ref.py restates them in numpy.
//
// mol_shape_kernel<true> (staged; segment_staged_kernel of segment_com.hip is the model): a workgroup owns a RUN of whole
//   molecules of one job that fits an LDS stage (shape_plan.h: at most 256 molecules and 1024 atoms) and strides over
//   the frames along gridDim.y. Per frame the run's three planes come in with coalesced full-width loads — the next
//   frame's while this one is worked — into padded LDS; then one lane per molecule walks its atoms in index order in
//   LDS, twice (centre, then tensor), and does the invariants, the sweeps, its three LDS histogram adds and its stores,
//   consecutive lanes writing consecutive series. Every atom of a molecule is read here, so lanes striding through
//   global memory a molecule apart would fetch every line many times; through the stage every HBM byte is
//   fetched once.
// mol_shape_kernel<false> (walk): molecules longer than the stage, one lane per (molecule, frame) in global memory. The
//   same function sh_molecule with another reader: the same operations in the same order, the same bits.
// Counts go to the workgroup's LDS row (32-bit cells, integer LDS atomics; a run belongs to one job) and from there once
// into 64-bit device cells with integer atomics: exact whatever the order. shape_total_kernel then adds the values as
// written per (frame, job) in the fixed order of moments_total_kernel (moments.hip). No floating-point atomics.
#include <algorithm>
#include <cstring>
#include <vector>

#include "call_tables.h"
#include "group_pairs.h"  // (gp_check_edges, gp_edges: the edge table of the siblings)
#include "mol_tile.h"     // (mt_wrap, MolIo, MolOut, mt_plan_error, mt_launch_totals)
#include "shape_plan.h"

#pragma clang fp contract(off)

namespace {

constexpr int SH_SWEEPS = 5;                                 // cyclic Jacobi sweeps (measured, plus one)
constexpr int SH_PER = SH_CAP / SH_MOLS;                    // atoms per lane and plane of a stage
constexpr int SH_STRIDE = SH_CAP + SH_CAP / 32 + 2;          // doubles per plane of the padded stage
constexpr int SH_MAX_BINS = 4096, SH_MAX_KBINS = 1024;
constexpr int SH_VALS = 6, SH_TOTALS = 9;
constexpr int SH_STAGE_DOUBLES = 3 * SH_STRIDE + SH_CAP;    // the stage and the job's weight row
constexpr size_t SH_MAX_LDS = (size_t)SH_STAGE_DOUBLES * 8 + (size_t)(2 * SH_MAX_BINS + SH_MAX_KBINS + 3) * 4;
static_assert(SH_MAX_LDS <= 160 * 1024 && (SH_STAGE_DOUBLES * 8) % 16 == 0, "stage, weights and row must fit LDS");

struct ShJob {  // by the job's number in the call
    long long atom0, mols, series0;
    double msum;          // the mass of one molecule: the host's sum in index order
    int len, e0, e1, w0;  // atoms per molecule, the two end atoms, where its weight row starts in the table
};

// LDS index with one pad double per 32 (segment_com.hip: sc_pad): lanes whose molecules start 4, 8, 16, ... atoms apart
// would otherwise all hit the same banks
__device__ __forceinline__ int sh_pad(int i) { return i + (i >> 5); }

struct ShValues {
    double rg2, ree2, k2, lam[3], i2;
};

// One Jacobi rotation of the pair (p, q), r the third axis: the operations of include/mdhip.h in their order
__device__ __forceinline__ void sh_rotate(double &gpp, double &gqq, double &gpq, double &grp, double &grq)
{
    if (gpq == 0.0) return;
    const double theta = (gqq - gpp) / (2.0 * gpq);
    const double root = __builtin_sqrt(theta * theta + 1.0);
    const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (-theta + root);
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    const double tp = t * gpq;
    gpp = gpp - tp;
    gqq = gqq + tp;
    gpq = 0.0;
    const double a = grp, b = grq;
    grp = c * a - s * b;
    grq = s * a + c * b;
}

// The molecule whose atom k has the coordinate at(axis, k) and the weight w(k): everything mdhip_mol_shape defines per
// (molecule, frame). `eigen`: the principal moments are wanted (they are not binned: a call for histograms alone skips the sweeps).
template <class At, class Wt>
__device__ __forceinline__ ShValues sh_molecule(At at, Wt w, int len, double M, int e0, int e1,
                                                bool chain, bool wrap, const double *L, const double *half, bool eigen)
{
    // positions about the first atom, and the centre. Atom 0 (p_0 = 0.0) stands in front of the loops, which are unrolled
    // by four so that the reads of four atoms and their weights are in flight together: the operations and their order
    // are those of one atom after the other.
    double first[3], prev[3], p[3], sum[3], pe0[3] = {0.0, 0.0, 0.0}, pe1[3] = {0.0, 0.0, 0.0};
    auto step = [&](int ax, double xk) {  // p_k from p_(k-1), k >= 1
        double d = xk - (chain ? prev[ax] : first[ax]);
        if (wrap) d = mt_wrap(d, L[ax], half[ax]);
        p[ax] = chain ? p[ax] + d : d;
        prev[ax] = xk;
    };
    const double w0 = w(0);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        first[ax] = prev[ax] = at(ax, 0);
        p[ax] = 0.0;
        sum[ax] = 0.0 + w0 * p[ax];
    }
#pragma unroll 4
    for (int k = 1; k < len; ++k) {
        const double wk = w(k);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            step(ax, at(ax, k));
            sum[ax] = sum[ax] + wk * p[ax];
            if (k == e0) pe0[ax] = p[ax];
            if (k == e1) pe1[ax] = p[ax];
        }
    }
    const double c[3] = {sum[0] / M, sum[1] / M, sum[2] / M};
    // the tensor about the centre: the positions again, by the same operations
    double gxx = 0.0, gyy = 0.0, gzz = 0.0, gxy = 0.0, gyz = 0.0, gzx = 0.0;
    auto add = [&](double wk) {
        const double q[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
        const double wx = wk * q[0], wy = wk * q[1], wz = wk * q[2];
        gxx = gxx + wx * q[0];
        gyy = gyy + wy * q[1];
        gzz = gzz + wz * q[2];
        gxy = gxy + wx * q[1];
        gyz = gyz + wy * q[2];
        gzx = gzx + wz * q[0];
    };
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) prev[ax] = first[ax], p[ax] = 0.0;
    add(w0);
#pragma unroll 4
    for (int k = 1; k < len; ++k) {
        const double wk = w(k);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) step(ax, at(ax, k));
        add(wk);
    }
    gxx = gxx / M, gyy = gyy / M, gzz = gzz / M, gxy = gxy / M, gyz = gyz / M, gzx = gzx / M;
    ShValues o;
    o.rg2 = (gxx + gyy) + gzz;
    o.i2 = ((gxx * gyy + gyy * gzz) + gzz * gxx) - ((gxy * gxy + gyz * gyz) + gzx * gzx);
    o.k2 = o.rg2 == 0.0 ? 0.0 : 1.0 - (3.0 * o.i2) / (o.rg2 * o.rg2);
    const double rx = pe1[0] - pe0[0], ry = pe1[1] - pe0[1], rz = pe1[2] - pe0[2];
    o.ree2 = (rx * rx + ry * ry) + rz * rz;
    o.lam[0] = o.lam[1] = o.lam[2] = 0.0;
    if (eigen) {
        for (int sweep = 0; sweep < SH_SWEEPS; ++sweep) {
            sh_rotate(gxx, gyy, gxy, gzx, gyz);  // (x, y), r = z
            sh_rotate(gxx, gzz, gzx, gxy, gyz);  // (x, z), r = y
            sh_rotate(gyy, gzz, gyz, gxy, gzx);  // (y, z), r = x
        }
        double a = gxx, b = gyy, d = gzz, t;
        if (a < b) t = a, a = b, b = t;
        if (b < d) t = b, b = d, d = t;
        if (a < b) t = a, a = b, b = t;
        o.lam[0] = a, o.lam[1] = b, o.lam[2] = d;
    }
    return o;
}

// v = Rg^2 or Ree^2 into its row: the bin of sqrt(v) / bin_size by comparison with the exact edge table (the float
// estimate only says where the walk along the edges starts), everything else — a NaN included — in *beyond
__device__ __forceinline__ void sh_count(double v, double top, const double *__restrict__ edges, float gscale, int nbins,
                                         unsigned *row, unsigned *beyond)
{
    if (v >= 0.0 && v < top) {
        const float g = __builtin_amdgcn_sqrtf((float)v) * gscale;
        int k = g < (float)(nbins - 1) ? (int)g : nbins - 1;
        while (v < edges[k]) --k;       // edges[0] == 0 stops it
        while (v >= edges[k + 1]) ++k;  // v < edges[nbins] stops it
        atomicAdd(row + k, 1u);
    } else {
        atomicAdd(beyond, 1u);
    }
}

// Block (x, y): run run0 + x, the frames y, y + gridDim.y, ... Dynamic LDS: the job's row of n_cells 32-bit cells
// [Rg: nbins][Ree: nbins][kappa^2: n_kbins][beyond Rg, beyond Ree, degenerate]; cnt [n_jobs][n_cells] the same in 64 bits.
// pm [F][6][S] and i2 [F][S] may be NULL: no values.
template <bool STAGED>
__global__ __launch_bounds__(SH_MOLS) void mol_shape_kernel(
    const double *__restrict__ x, const double *__restrict__ box, long long F, long long A, long long S,
    const ShJob *__restrict__ jobs, const ShRun *__restrict__ runs, const double *__restrict__ w_tab,
    const double *__restrict__ edges, float gscale, int nbins, int n_kbins, int n_cells, int chain,
    unsigned long long *__restrict__ cnt, double *__restrict__ pm, double *__restrict__ i2)
{
    // dynamic LDS: staged [the stage: 3 planes of SH_STRIDE][the job's weight row: SH_CAP] [the row of n_cells counters]
    extern __shared__ double s_dyn[];
    double *const s_x = s_dyn, *const s_w = s_dyn + 3 * SH_STRIDE;
    unsigned int *const s_h = reinterpret_cast<unsigned int *>(s_dyn + (STAGED ? SH_STAGE_DOUBLES : 0));
    const int tid = threadIdx.x;
    const ShRun run = runs[blockIdx.x];
    const ShJob job = jobs[run.job];
    for (int i = tid; i < n_cells; i += SH_MOLS) s_h[i] = 0u;
    const double *__restrict__ w = w_tab + job.w0;
    if (STAGED)  // (the walk then reads LDS only; DESIGN 4.13e: measured, no difference to uniform loads from global memory)
        for (int i = tid; i < job.len; i += SH_MOLS) s_w[i] = w[i];
    __syncthreads();
    const long long a_run = job.atom0 + run.m0 * job.len;  // the run's first atom
    const int na = STAGED ? run.nm * job.len : 0;          // staged: its atoms, at most SH_CAP
    const bool mine = tid < run.nm;
    const long long s = job.series0 + run.m0 + tid;
    const double top = edges[nbins];
    const bool eigen = pm != nullptr;
    double v[3][SH_PER];
    auto fetch = [&](long long f) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double *__restrict__ plane = x + ((size_t)f * 3 + ax) * (size_t)A + a_run;
#pragma unroll
            for (int r = 0; r < SH_PER; ++r) {
                const int i = tid + r * SH_MOLS;
                v[ax][r] = i < na ? plane[i] : 0.0;
            }
        }
    };
    if (STAGED && (long long)blockIdx.y < F) fetch(blockIdx.y);
    for (long long f = blockIdx.y; f < F; f += gridDim.y) {
        if (STAGED) {
            __syncthreads();  // the previous frame's walks are done with the stage
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int r = 0; r < SH_PER; ++r) {
                    const int i = tid + r * SH_MOLS;
                    if (i < na) s_x[ax * SH_STRIDE + sh_pad(i)] = v[ax][r];
                }
            __syncthreads();
            if (f + gridDim.y < F) fetch(f + gridDim.y);  // lands while this frame's walks run
        }
        if (!mine) continue;
        double L[3] = {0.0, 0.0, 0.0}, half[3] = {0.0, 0.0, 0.0};
        if (box) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) L[ax] = box[f * 3 + ax], half[ax] = L[ax] / 2;
        }
        ShValues o;
        if (STAGED) {
            const int base = tid * job.len;
            o = sh_molecule([&](int ax, int k) { return s_x[ax * SH_STRIDE + sh_pad(base + k)]; }, [&](int k) { return s_w[k]; },
                            job.len, job.msum, job.e0, job.e1, chain != 0, box != nullptr, L, half, eigen);
        } else {
            const double *__restrict__ mol = x + (size_t)f * 3 * (size_t)A + (size_t)(a_run + (long long)tid * job.len);
            o = sh_molecule([&](int ax, int k) { return mol[(size_t)ax * (size_t)A + k]; }, [&](int k) { return w[k]; },
                            job.len, job.msum, job.e0, job.e1, chain != 0, box != nullptr, L, half, eigen);
        }
        sh_count(o.rg2, top, edges, gscale, nbins, s_h, s_h + 2 * nbins + n_kbins);
        sh_count(o.ree2, top, edges, gscale, nbins, s_h + nbins, s_h + 2 * nbins + n_kbins + 1);
        if (o.rg2 == 0.0) {
            atomicAdd(s_h + 2 * nbins + n_kbins + 2, 1u);
        } else if (__builtin_fabs(o.k2) < __builtin_inf()) {
            const double kb = o.k2 * (double)n_kbins;
            const int bin = kb >= (double)n_kbins ? n_kbins - 1 : (kb < 0.0 ? 0 : (int)kb);
            atomicAdd(s_h + 2 * nbins + bin, 1u);
        }
        if (pm) {
            double *__restrict__ dst = pm + (size_t)f * SH_VALS * (size_t)S + (size_t)s;
            dst[0] = o.rg2;
            dst[(size_t)S] = o.ree2;
            dst[2 * (size_t)S] = o.k2;
            dst[3 * (size_t)S] = o.lam[0];
            dst[4 * (size_t)S] = o.lam[1];
            dst[5 * (size_t)S] = o.lam[2];
        }
        if (i2) i2[(size_t)f * (size_t)S + (size_t)s] = o.i2;
    }
    __syncthreads();
    unsigned long long *__restrict__ g_row = cnt + (size_t)run.job * (size_t)n_cells;
    for (int i = tid; i < n_cells; i += SH_MOLS) {
        const unsigned n = s_h[i];
        if (n) atomicAdd(g_row + i, (unsigned long long)n);
    }
}

constexpr int SHT_THREADS = 256;

// Block (x, y): frame f0 + x, job job0 + y. totals[job][.][f] = the sums over the job's molecules of Rg^2, sqrt(Rg^2),
// Ree^2, lambda1, lambda2, lambda3, kappa^2, I2, Rg^2 * Rg^2 of the values as written: lane i adds the molecules i,
// i + 256, ... in order, then a fixed tree over the 256 partial sums (moments_total_kernel of moments.hip).
__global__ __launch_bounds__(SHT_THREADS) void shape_total_kernel(const double *__restrict__ pm, const double *__restrict__ i2,
                                                                  long long F, long long S, const ShJob *__restrict__ jobs,
                                                                  long long f0, int job0, double *__restrict__ totals)
{
    __shared__ double s_red[SH_TOTALS][SHT_THREADS];
    const long long f = f0 + blockIdx.x;
    const int job = job0 + (int)blockIdx.y;
    const long long s0 = jobs[job].series0, n = jobs[job].mols;
    const double *__restrict__ row = pm + (size_t)f * SH_VALS * (size_t)S + (size_t)s0;
    const double *__restrict__ ri = i2 + (size_t)f * (size_t)S + (size_t)s0;
    double acc[SH_TOTALS];
#pragma unroll
    for (int q = 0; q < SH_TOTALS; ++q) acc[q] = 0.0;
    for (long long m = threadIdx.x; m < n; m += SHT_THREADS) {
        const double rg2 = row[m], ree2 = row[(size_t)S + m], k2 = row[2 * (size_t)S + m];
        acc[0] += rg2;
        acc[1] += __builtin_sqrt(rg2);
        acc[2] += ree2;
        acc[3] += row[3 * (size_t)S + m];
        acc[4] += row[4 * (size_t)S + m];
        acc[5] += row[5 * (size_t)S + m];
        acc[6] += k2;
        acc[7] += ri[m];
        acc[8] += rg2 * rg2;
    }
#pragma unroll
    for (int q = 0; q < SH_TOTALS; ++q) s_red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int half = SHT_THREADS / 2; half; half >>= 1) {
        if ((int)threadIdx.x < half) {
#pragma unroll
            for (int q = 0; q < SH_TOTALS; ++q) s_red[q][threadIdx.x] += s_red[q][threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x < SH_TOTALS) totals[((size_t)job * SH_TOTALS + threadIdx.x) * (size_t)F + (size_t)f] = s_red[threadIdx.x][0];
}

}  // namespace

extern "C" {

int mdhip_mol_shape(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *x, int x_on_device, const double *box,
                    int n_jobs, const int64_t *job_atom0, const int64_t *job_mols, const int32_t *job_len,
                    const int64_t *w_off, const double *w, const int32_t *job_ends, int unwrap, double bin_size,
                    int32_t nbins, const double *edges, int32_t n_kbins, uint64_t *hist_rg, uint64_t *hist_ee,
                    uint64_t *hist_k, uint64_t *beyond, uint64_t *degenerate, double *totals, double *per_mol,
                    int per_mol_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_jobs >= 1 && n_jobs <= (1 << 20), "n_jobs must be in [1, 2^20]");
    MD_REQUIRE(n_frames >= 1 && n_atoms >= 1, "n_frames and n_atoms must be positive");
    MD_REQUIRE(n_atoms < (1ll << 40) && n_frames < (1ll << 31) && n_frames < (1ll << 40) / n_atoms, "trajectory too large");
    MD_REQUIRE(nbins >= 1 && nbins <= SH_MAX_BINS, "nbins must be in [1, %d]", SH_MAX_BINS);
    MD_REQUIRE(n_kbins >= 1 && n_kbins <= SH_MAX_KBINS, "n_kbins must be in [1, %d]", SH_MAX_KBINS);
    MD_REQUIRE(unwrap == 0 || unwrap == 1, "unwrap must be 0 (about the first atom) or 1 (along the chain)");
    MD_REQUIRE(bin_size > 0.0 && bin_size < __builtin_inf(), "bin_size must be positive and finite");
    MD_REQUIRE(x && job_atom0 && job_mols && job_len && w_off && w && job_ends, "NULL array");
    MD_REQUIRE(hist_rg || hist_ee || hist_k || beyond || degenerate || totals || per_mol,
               "every output is NULL: nothing to compute");
    MD_REQUIRE(w_off[0] == 0, "w_off must start at 0");
    const ShPlan plan = shape_plan(n_jobs, job_atom0, job_mols, job_len, n_atoms, n_frames);
    for (int j = 0; j < plan.checked_jobs(); ++j) {
        MD_REQUIRE(w_off[j + 1] - w_off[j] == job_len[j], "job %d: its weight row must hold job_len weights", j);
        const int e0 = job_ends[2 * (size_t)j], e1 = job_ends[2 * (size_t)j + 1];
        MD_REQUIRE(e0 >= 0 && e0 < job_len[j] && e1 >= 0 && e1 < job_len[j], "job %d: the end atoms must be in [0, job_len)", j);
    }
    int rc;
    if ((rc = mt_plan_error(ctx, plan, n_atoms))) return rc;
    MD_REQUIRE(w_off[n_jobs] < (1ll << 31), "weight table too large");
    const std::vector<double> msum = shape_mass_sums(n_jobs, job_len, w_off, w);
    for (int j = 0; j < n_jobs; ++j)
        MD_REQUIRE(msum[(size_t)j] > 0.0 && msum[(size_t)j] < __builtin_inf(), "job %d: the weights must add up to a positive, finite mass", j);
    const int n_cells = 2 * nbins + n_kbins + 3;
    MD_REQUIRE((size_t)n_jobs * (size_t)n_cells < ((size_t)1 << 24), "result too large");
    if ((rc = gp_check_edges(ctx, edges, nbins, n_jobs))) return rc;
    std::vector<double> own;
    if ((rc = gp_edges(ctx, edges, own, bin_size, nbins))) return rc;

    std::vector<ShJob> jobs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j)
        jobs[(size_t)j] = {job_atom0[j], job_mols[j], plan.series0[(size_t)j], msum[(size_t)j], job_len[j],
                           job_ends[2 * (size_t)j], job_ends[2 * (size_t)j + 1], (int)w_off[j]};
    const long long S = plan.series;
    MolIo io;
    if ((rc = io.open(ctx, n_frames, n_atoms, x, x_on_device, box, nullptr, 0, S))) return rc;
    // the totals read the values (and I2, which no caller gets) back, so they are written somewhere whenever totals are
    // asked for
    const size_t pm_b = (size_t)n_frames * SH_VALS * (size_t)S * 8, i2_b = (size_t)n_frames * (size_t)S * 8;
    MolOut o_pm, o_i2;
    if ((rc = o_pm.open(ctx, WS_OUT, per_mol, per_mol_on_device, pm_b, totals != nullptr))) return rc;
    if ((rc = o_i2.open(ctx, WS_OUT2, nullptr, 0, i2_b, totals != nullptr))) return rc;
    double *const d_pm = o_pm.dev, *const d_i2 = o_i2.dev;
    const size_t n_st = plan.staged.size(), n_wk = plan.walk.size();
    const ShJob *d_jobs;
    const ShRun *d_staged, *d_walk;
    const double *d_w, *d_edges;
    CallTables tab;
    tab.add(jobs.data(), (size_t)n_jobs, &d_jobs);
    tab.add(plan.staged.data(), n_st, &d_staged);
    tab.add(plan.walk.data(), n_wk, &d_walk);
    tab.add(w, (size_t)w_off[n_jobs], &d_w);
    tab.add(edges, (size_t)nbins + 1, &d_edges);
    if ((rc = upload_tables(ctx, tab, WS_TABLES))) return rc;
    const size_t cnt_b = (size_t)n_jobs * (size_t)n_cells * 8;
    MD_WS(d_cnt, unsigned long long, WS_HIST, cnt_b);
    MD_HIP(hipMemsetAsync(d_cnt, 0, cnt_b, ctx->stream));
    double *d_tot = nullptr;
    const size_t tot_b = (size_t)n_jobs * SH_TOTALS * (size_t)n_frames * 8;
    if (totals) {
        d_tot = (double *)mdhip_ws(ctx, WS_PART, tot_b);
        if (!d_tot) return MDHIP_ENOMEM;
    }
    const float gscale = (float)(1.0 / bin_size);
    const size_t lds = (size_t)n_cells * 4, lds_staged = (size_t)SH_STAGE_DOUBLES * 8 + lds;
    KernelTimer timer(ctx, 0);
    int launches = 0;
    if (n_st) {
        const unsigned gy = shape_frame_slices((long long)n_st, n_frames, ctx->cu_count);
        MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(mol_shape_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)SH_MAX_LDS));
        hipLaunchKernelGGL(mol_shape_kernel<true>, dim3((unsigned)n_st, gy), dim3(SH_MOLS), lds_staged, ctx->stream, io.x, io.box,
                           (long long)n_frames, (long long)n_atoms, S, d_jobs, d_staged, d_w, d_edges,
                           gscale, (int)nbins, (int)n_kbins, n_cells, unwrap, d_cnt, d_pm, d_i2);
        MD_HIP(hipGetLastError());
        ++launches;
    }
    if (n_wk) {
        const unsigned gy = shape_frame_slices((long long)n_wk, n_frames, ctx->cu_count);
        hipLaunchKernelGGL(mol_shape_kernel<false>, dim3((unsigned)n_wk, gy), dim3(SH_MOLS), lds, ctx->stream, io.x, io.box,
                           (long long)n_frames, (long long)n_atoms, S, d_jobs, d_walk, d_w, d_edges, gscale, (int)nbins,
                           (int)n_kbins, n_cells, unwrap, d_cnt, d_pm, d_i2);
        MD_HIP(hipGetLastError());
        ++launches;
    }
    if (totals) {
        rc = mt_launch_totals(ctx, n_frames, n_jobs, [&](dim3 grid, long long f0, int j0) {
            hipLaunchKernelGGL(shape_total_kernel, grid, dim3(SHT_THREADS), 0, ctx->stream, (const double *)d_pm,
                               (const double *)d_i2, (long long)n_frames, S, d_jobs, f0, j0, d_tot);
        });
        if (rc < 0) return rc;
        launches += rc;
    }
    ctx->last_kernel = n_st ? "mol_shape_kernel<true>" : "mol_shape_kernel<false>";
    ctx->last_launches = launches;
    timer.stop();
    if (totals && (rc = mdhip_result(cs, totals, d_tot, tot_b, 0))) return rc;
    if ((rc = o_pm.deliver(cs))) return rc;
    if (hist_rg || hist_ee || hist_k || beyond || degenerate) {
        // the rows come back whole and are dealt to the caller's arrays once the copy has landed
        unsigned long long *h_cnt = (unsigned long long *)mdhip_pin(ctx, cnt_b);
        if (!h_cnt) return MDHIP_ENOMEM;
        if ((rc = mdhip_copy_small(ctx, h_cnt, d_cnt, cnt_b, hipMemcpyDeviceToHost))) return rc;
        const int nb = nbins, nk = n_kbins, nj = n_jobs;
        cs.defer([=]() {
            for (int j = 0; j < nj; ++j) {
                const unsigned long long *row = h_cnt + (size_t)j * (size_t)n_cells;
                if (hist_rg) memcpy(hist_rg + (size_t)j * nb, row, (size_t)nb * 8);
                if (hist_ee) memcpy(hist_ee + (size_t)j * nb, row + nb, (size_t)nb * 8);
                if (hist_k) memcpy(hist_k + (size_t)j * nk, row + 2 * nb, (size_t)nk * 8);
                if (beyond) beyond[2 * (size_t)j] = row[2 * nb + nk], beyond[2 * (size_t)j + 1] = row[2 * nb + nk + 1];
                if (degenerate) degenerate[j] = row[2 * nb + nk + 2];
            }
            return MDHIP_OK;
        });
    }
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
