// segment_com.hip — per-molecule centre of mass and per-frame charge flux (R6, M3, G1).
//
// Replaces structural/rdf_cn.py:218-241 (_define_mol_cols), common/com_mols.py:58-60 (calc_com),
// dynamical/diffusion.py:83-89 and dynamical/_conductivity.py:11-35 of the reference.
// HBM-bound: 8*(1+n_attr) bytes read per atom, 8*n_attr written per molecule.
//
// Rounding: every product m*a and every addition is its own IEEE operation (contraction off), atoms
// are added in index order, then one correctly rounded division by the mass sum. The reference's
// pandas/BLAS sums use another order, so agreement is ~1e-15 relative, not bitwise.
#include <algorithm>
#include <vector>

#include <cmath>

#include "ctx.h"
#include "seg_plan.h"

#pragma clang fp contract(off)

namespace {

// Staged kernel (default). A block owns a run of whole segments with at most SC_CAP atoms in total and
// loops over frames and attribute planes: the run's atoms are read with coalesced 8-byte loads,
// multiplied by their mass and parked in LDS; then one lane per segment adds its atoms up in index
// order from LDS and divides by the mass sum. Same operations in the same order as one lane walking
// its segment in global memory (the fallback below, kept for segments longer than SC_CAP), but every
// HBM byte is fetched once by a full-width load. The runs (SegBlock) and the stage sizes come from seg_plan.h.

// LDS index with one pad double per 32: lanes whose segments start 4, 8, 16, ... atoms apart would otherwise
// all hit the same banks
__device__ __forceinline__ int sc_pad(int i) { return i + (i >> 5); }
constexpr int sc_stride(int cap) { return cap + cap / 32 + 2; }

// FLUX = false: out[f][k][s] = sum(m a) / sum(m)                                   (com_mols.py:58-60)
// FLUX = true : out[f][k][s] = (sum(m v) / sum(m) * vel_conv) * (sum(q) * charge_conv)   (_conductivity.py:21-25)
// NT = threads per block: 256 (four waves share a stage of SC_CAP atoms, two block barriers per step) or 64 — ONE wave
// per block with a stage of 256 atoms: the barriers then cost nothing and every wave runs its own pipeline, decoupled
// from its neighbours (the wave-private form; default whenever no segment is longer than 256 atoms).
template <bool FLUX, int SC_CAP, int NT>
__global__ __launch_bounds__(NT) void segment_staged_kernel(
    const double *__restrict__ attr, const double *__restrict__ mass, const double *__restrict__ q,
    const long long *__restrict__ seg_off, const SegBlock *__restrict__ blocks, double *__restrict__ out,
    int n_attr, long long n_atoms, long long n_seg, long long n_frames, double vel_conv, double charge_conv, int use_vec)
{
    constexpr int SC_STRIDE = sc_stride(SC_CAP);
    __shared__ double s_v[SC_PLANES * SC_STRIDE];
    __shared__ double s_m[SC_CAP];
    const int tid = threadIdx.x;
    const SegBlock b = blocks[blockIdx.x];
    const long long a0 = seg_off[b.s0];
    const int na = (int)(seg_off[b.s1] - a0);
    for (int i = tid; i < na; i += NT) s_m[i] = mass[a0 + i];
    // Sum tasks: (segment, plane) pairs of the block, dealt plane-major over the 256 lanes — consecutive lanes take
    // consecutive segments of one plane (coalesced stores, spread LDS banks), and a block of 64 sixteen-atom molecules
    // keeps 192 lanes busy in the sum phase instead of 64 (SC_TPL tasks per lane cover 256 segments x 3 planes).
    constexpr int SC_TPL = SC_PLANES;
    const int nseg = (int)(b.s1 - b.s0);
    int t_lo[SC_TPL], t_hi[SC_TPL], t_kk[SC_TPL], t_seg[SC_TPL];
    double t_msum[SC_TPL], t_qsi[SC_TPL];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SC_TPL; ++j) {
        const int t = tid + j * NT;
        const int kk = t / nseg, sg = t - kk * nseg;
        t_kk[j] = kk < SC_PLANES ? kk : -1;
        t_seg[j] = sg;
        t_lo[j] = t_hi[j] = 0;
        t_msum[j] = 1.0;
        t_qsi[j] = 0.0;
        if (t_kk[j] >= 0) {
            t_lo[j] = (int)(seg_off[b.s0 + sg] - a0);
            t_hi[j] = (int)(seg_off[b.s0 + sg + 1] - a0);
            double msum = 0.0;
            for (int a = t_lo[j]; a < t_hi[j]; ++a) msum += s_m[a];
            t_msum[j] = msum;
            if (FLUX) {
                double qsum = 0.0;
                for (int a = t_lo[j]; a < t_hi[j]; ++a) qsum += q[a0 + a];
                t_qsi[j] = qsum * charge_conv;  // _conductivity.py:25
            }
        }
    }
    // Software pipeline over (frame, plane group) steps: the values of step n+1 are loaded into registers while
    // the segment sums of step n run out of LDS, so that HBM requests are in flight all the time.
    constexpr int PER = SC_CAP / NT;  // atoms per lane per plane
    const int groups = (n_attr + SC_PLANES - 1) / SC_PLANES;
    const long long n_my = blockIdx.y < n_frames ? (n_frames - blockIdx.y + gridDim.y - 1) / gridDim.y : 0;
    const long long steps = n_my * groups;
    // The loads of step n+1 are issued right after the barrier that ends the LDS writes of step n and land while
    // its sums run. (A second register set, fetching at the very top of the step, measured slower: 102 VGPRs.)
    // A lane owns the atoms (2 tid, 2 tid + 1) + 512 r: 16-byte loads when the planes allow it (even atom count and
    // block start, 16-byte aligned base) — half the load instructions of 8-byte loads.
    double v[SC_PLANES][PER];
    const bool vec2 = use_vec && ((n_atoms | a0) & 1LL) == 0 && ((reinterpret_cast<unsigned long long>(attr) & 15ULL) == 0);
    auto fetch = [&](long long step) {
        const long long f = blockIdx.y + (step / groups) * gridDim.y;
        const int k0 = (int)(step % groups) * SC_PLANES;
        const double *p = attr + ((size_t)f * n_attr + k0) * n_atoms + a0;
#pragma unroll
        for (int kk = 0; kk < SC_PLANES; ++kk)
#pragma unroll
            for (int r = 0; r < PER / 2; ++r) {
                const int i = 2 * tid + r * (2 * NT);
                const bool ok = k0 + kk < n_attr;
                if (!use_vec) {  // A/B: the 8-byte layout (lane owns tid + 256 r)
                    const int i0 = tid + (2 * r) * NT, i1 = tid + (2 * r + 1) * NT;
                    v[kk][2 * r] = (ok && i0 < na) ? p[(size_t)kk * n_atoms + i0] : 0.0;
                    v[kk][2 * r + 1] = (ok && i1 < na) ? p[(size_t)kk * n_atoms + i1] : 0.0;
                    continue;
                }
                if (vec2 && ok && i + 1 < na) {
                    typedef double d2_t __attribute__((ext_vector_type(2)));
                    const d2_t t2 = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(p + (size_t)kk * n_atoms + i));
                    v[kk][2 * r] = t2[0];
                    v[kk][2 * r + 1] = t2[1];
                } else {
                    v[kk][2 * r] = (ok && i < na) ? p[(size_t)kk * n_atoms + i] : 0.0;
                    v[kk][2 * r + 1] = (ok && i + 1 < na) ? p[(size_t)kk * n_atoms + i + 1] : 0.0;
                }
            }
    };
    auto process = [&](long long step) {
        const long long f = blockIdx.y + (step / groups) * gridDim.y;
        const int k0 = (int)(step % groups) * SC_PLANES;
        const int nk = n_attr - k0 < SC_PLANES ? n_attr - k0 : SC_PLANES;
        __syncthreads();  // the previous step's sums have been taken
#pragma unroll
        for (int kk = 0; kk < SC_PLANES; ++kk)
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int i = use_vec ? 2 * tid + (r >> 1) * (2 * NT) + (r & 1) : tid + r * NT;
                if (i < na) s_v[kk * SC_STRIDE + sc_pad(i)] = v[kk][r] * s_m[i];
            }
        __syncthreads();
        if (step + 1 < steps) fetch(step + 1);
#pragma unroll
        for (int j = 0; j < SC_TPL; ++j) {
            const int kk = t_kk[j];
            if (kk >= 0 && kk < nk) {
                // atoms added in index order (one rounding per addition, as a lane walking the segment would);
                // four LDS reads are issued before their additions so that the reads overlap
                const double *row = s_v + kk * SC_STRIDE;
                double acc = 0.0;
                int a = t_lo[j];
                for (; a + 4 <= t_hi[j]; a += 4) {
                    const double x0 = row[sc_pad(a)], x1 = row[sc_pad(a + 1)], x2 = row[sc_pad(a + 2)],
                                 x3 = row[sc_pad(a + 3)];
                    acc += x0;
                    acc += x1;
                    acc += x2;
                    acc += x3;
                }
                for (; a < t_hi[j]; ++a) acc += row[sc_pad(a)];
                double r = acc / t_msum[j];
                if (FLUX) r = (r * vel_conv) * t_qsi[j];  // com_mols.py:60 then _conductivity.py:21-23
                out[((size_t)f * n_attr + k0 + kk) * n_seg + b.s0 + t_seg[j]] = r;
            }
        }
    };
    if (steps > 0) fetch(0);
    for (long long step = 0; step < steps; ++step) process(step);
}

// One (run of segments, frame, plane group) per block and nothing carried between frames (round 3; option seg_frame):
// the run's table entry (SegRun) holds its atom range, the per-segment mass sums come from the host's index-order sums
// (seg_sums; mdhip_segment_com computes them anyway), the masses are re-read per block (L2 hits: 8 B per atom against 24 B of
// coordinates from HBM). No software pipeline, no register double buffer: the loads of many small blocks overlap
// instead, as in msd_pairs_kernel. Same products, same additions in the same order, one division.
// (88 / 100 VGPRs: 5 / 4 blocks per CU where LDS would hold 6; forcing 80 registers spills 3 / 11 of them and measured
// 5 % / 20 % slower.)
template <bool FLUX, int SC_CAP>
__global__ __launch_bounds__(256) void segment_frame_kernel(
    const double *__restrict__ attr, const double *__restrict__ mass, const double *__restrict__ seg_msum,
    const double *__restrict__ seg_qsi, const long long *__restrict__ seg_off, const SegRun *__restrict__ runs,
    double *__restrict__ out, int n_attr, long long n_atoms, long long n_seg, long long n_steps, double vel_conv)
{
    constexpr int NT = 256, SC_STRIDE = sc_stride(SC_CAP), PER = SC_CAP / NT;
    __shared__ double s_v[SC_PLANES * SC_STRIDE];
    const int tid = threadIdx.x;
    const SegRun b = runs[blockIdx.x];
    const int na = b.na, nseg = (int)(b.s1 - b.s0);
    const int groups = (n_attr + SC_PLANES - 1) / SC_PLANES;
    typedef double d2_t __attribute__((ext_vector_type(2)));
    const bool vec2 = ((n_atoms | b.a0) & 1LL) == 0 &&
                      ((reinterpret_cast<unsigned long long>(attr) | reinterpret_cast<unsigned long long>(mass)) & 15ULL) == 0;
    for (long long step = blockIdx.y; step < n_steps; step += gridDim.y) {
        const long long f = step / groups;
        const int k0 = (int)(step % groups) * SC_PLANES;
        const int nk = n_attr - k0 < SC_PLANES ? n_attr - k0 : SC_PLANES;
        const double *p = attr + ((size_t)f * n_attr + k0) * n_atoms + b.a0;
        double v[SC_PLANES][PER], mm[PER];
#pragma unroll
        for (int r = 0; r < PER / 2; ++r) {
            const int i = 2 * tid + r * (2 * NT);
#pragma unroll
            for (int kk = 0; kk < SC_PLANES; ++kk) {
                v[kk][2 * r] = v[kk][2 * r + 1] = 0.0;
                if (kk < nk) {
                    if (vec2 && i + 1 < na) {
                        const d2_t t2 = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(p + (size_t)kk * n_atoms + i));
                        v[kk][2 * r] = t2[0];
                        v[kk][2 * r + 1] = t2[1];
                    } else {
                        if (i < na) v[kk][2 * r] = p[(size_t)kk * n_atoms + i];
                        if (i + 1 < na) v[kk][2 * r + 1] = p[(size_t)kk * n_atoms + i + 1];
                    }
                }
            }
            mm[2 * r] = mm[2 * r + 1] = 0.0;
            if (vec2 && i + 1 < na) {
                const d2_t t2 = *reinterpret_cast<const d2_t *>(mass + b.a0 + i);
                mm[2 * r] = t2[0];
                mm[2 * r + 1] = t2[1];
            } else {
                if (i < na) mm[2 * r] = mass[b.a0 + i];
                if (i + 1 < na) mm[2 * r + 1] = mass[b.a0 + i + 1];
            }
        }
        // the (segment, plane) sum tasks of this lane, plane-major over the lanes as in segment_staged_kernel
        int t_lo[SC_PLANES], t_hi[SC_PLANES], t_kk[SC_PLANES], t_seg[SC_PLANES];
        double t_msum[SC_PLANES], t_qsi[SC_PLANES];
#pragma unroll
        for (int j = 0; j < SC_PLANES; ++j) {
            const int t = tid + j * NT;
            const int kk = t / nseg, sg = t - kk * nseg;
            t_kk[j] = kk < nk ? kk : -1;
            t_seg[j] = sg;
            t_lo[j] = t_hi[j] = 0;
            t_msum[j] = 1.0;
            t_qsi[j] = 0.0;
            if (t_kk[j] >= 0) {
                t_lo[j] = (int)(seg_off[b.s0 + sg] - b.a0);
                t_hi[j] = (int)(seg_off[b.s0 + sg + 1] - b.a0);
                t_msum[j] = seg_msum[b.s0 + sg];
                if (FLUX) t_qsi[j] = seg_qsi[b.s0 + sg];
            }
        }
#pragma unroll
        for (int kk = 0; kk < SC_PLANES; ++kk)
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int i = 2 * tid + (r >> 1) * (2 * NT) + (r & 1);
                if (i < na) s_v[kk * SC_STRIDE + sc_pad(i)] = v[kk][r] * mm[r];
            }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SC_PLANES; ++j) {
            const int kk = t_kk[j];
            if (kk >= 0) {
                const double *row = s_v + kk * SC_STRIDE;
                double acc = 0.0;
                int a = t_lo[j];
                for (; a + 4 <= t_hi[j]; a += 4) {
                    const double x0 = row[sc_pad(a)], x1 = row[sc_pad(a + 1)], x2 = row[sc_pad(a + 2)],
                                 x3 = row[sc_pad(a + 3)];
                    acc += x0;
                    acc += x1;
                    acc += x2;
                    acc += x3;
                }
                for (; a < t_hi[j]; ++a) acc += row[sc_pad(a)];
                double r = acc / t_msum[j];
                if (FLUX) r = (r * vel_conv) * t_qsi[j];
                // (non-temporal: a write stream of a tenth of the bytes read costs a plain read stream a quarter of its
                // rate with ordinary stores and a sixth with these — tools/ubench_hbm.hip, 0.65 against 0.75 of 8 TB/s)
                __builtin_nontemporal_store(r, out + ((size_t)f * n_attr + k0 + kk) * n_seg + b.s0 + t_seg[j]);
            }
        }
        if (step + gridDim.y < n_steps) __syncthreads();  // (only when the grid could not hold every step)
    }
}

// Fallback: one lane per (segment, frame) walking global memory
__global__ __launch_bounds__(256) void segment_com_kernel(
    const double *__restrict__ attr, const double *__restrict__ mass,
    const long long *__restrict__ seg_off, double *__restrict__ out, int n_attr, long long n_atoms,
    long long n_seg, long long n_frames)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const long long lo = seg_off[s], hi = seg_off[s + 1];
    double msum = 0.0;
    for (long long a = lo; a < hi; ++a) msum += mass[a];
    for (long long f = blockIdx.y; f < n_frames; f += gridDim.y) {
        for (int k = 0; k < n_attr; ++k) {
            const double *p = attr + ((size_t)f * n_attr + k) * n_atoms;
            double acc = 0.0;
            for (long long a = lo; a < hi; ++a) acc += p[a] * mass[a];
            out[((size_t)f * n_attr + k) * n_seg + s] = acc / msum;
        }
    }
}

// q_mol * v_com,k in SI for every molecule: tmp [F][3][M] (fallback, as above)
__global__ __launch_bounds__(256) void mol_flux_kernel(
    const double *__restrict__ vel, const double *__restrict__ mass, const double *__restrict__ q,
    const long long *__restrict__ seg_off, double *__restrict__ tmp, long long n_atoms,
    long long n_seg, long long n_frames, double vel_conv, double charge_conv)
{
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const long long lo = seg_off[s], hi = seg_off[s + 1];
    double msum = 0.0, qsum = 0.0;
    for (long long a = lo; a < hi; ++a) {
        msum += mass[a];
        qsum += q[a];
    }
    const double q_si = qsum * charge_conv;  // _conductivity.py:25
    for (long long f = blockIdx.y; f < n_frames; f += gridDim.y) {
        for (int k = 0; k < 3; ++k) {
            const double *p = vel + ((size_t)f * 3 + k) * n_atoms;
            double acc = 0.0;
            for (long long a = lo; a < hi; ++a) acc += p[a] * mass[a];
            const double v_si = (acc / msum) * vel_conv;  // com_mols.py:60 then _conductivity.py:21-23
            tmp[((size_t)f * 3 + k) * n_seg + s] = v_si * q_si;
        }
    }
}

// J[k][type][f] = sum over the molecules of that type (a contiguous run) — fixed-order tree sum.
__global__ __launch_bounds__(256) void type_sum_kernel(const double *__restrict__ tmp,
                                                       const long long *__restrict__ type_off,
                                                       double *__restrict__ flux, long long n_seg,
                                                       long long n_frames, int n_types)
{
    __shared__ double red[256];
    const int t = blockIdx.x, k = blockIdx.y;
    const long long f = blockIdx.z;
    const long long lo = type_off[t], hi = type_off[t + 1];
    const double *p = tmp + ((size_t)f * 3 + k) * n_seg;
    double acc = 0.0;
    for (long long s = lo + threadIdx.x; s < hi; s += 256) acc += p[s];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) flux[((size_t)k * n_types + t) * n_frames + f] = red[0];
}

int check_segments(mdhip_ctx *ctx, int64_t n_atoms, int64_t n_seg, const int64_t *seg_off)
{
    MD_REQUIRE(n_seg >= 0 && (n_seg == 0 || seg_off), "bad segment table");
    for (int64_t s = 0; s < n_seg; ++s)
        MD_REQUIRE(seg_off[s] >= 0 && seg_off[s] < seg_off[s + 1] && seg_off[s + 1] <= n_atoms,
                   "seg_off must be increasing and within [0, n_atoms] (segment %lld)", (long long)s);
    return MDHIP_OK;
}

// What a segment kernel is given, whichever of them runs
struct SegArgs {
    const double *attr, *mass, *q;  // q: the flux's charges (staged and walk forms)
    const long long *seg_off;
    double *out;
    int n_attr;
    long long n_atoms, n_seg, n_frames;
    double vel_conv, charge_conv;  // the COM: 1.0
    // seg_stage_tables: the SegBlock | SegRun table and, by frame, the per-segment sums behind it
    const void *table = nullptr;
    const double *seg_msum = nullptr, *seg_qsi = nullptr;
};

SegOptions seg_options(const mdhip_ctx *ctx) { return {ctx->opt_seg_cap, ctx->opt_seg_frame, ctx->opt_seg_gy, ctx->opt_seg_vec}; }

// Only the table the chosen kernel reads goes to the device, into workspace slot `slot` (the callers' slots differ:
// the flux's result of this kernel lives in WS_AUX3). Staged: the SegBlock runs. By frame: the SegRun runs, then the
// n_sums per-segment sums (n_seg mass sums | + n_seg charge sums x charge_conv). The tables are the caller's locals:
// through pinned staging of the call.
int seg_stage_tables(mdhip_ctx *ctx, int slot, const SegPlan &pl, const double *sums, size_t n_sums, SegArgs &a)
{
    if (pl.form == SEG_WALK) return MDHIP_OK;
    const bool by_frame = pl.form == SEG_FRAME;
    const size_t tb = by_frame ? pl.runs.size() * sizeof(SegRun) : pl.blocks.size() * sizeof(SegBlock);
    const size_t sb = by_frame ? n_sums * 8 : 0;
    MD_WS(d_tab, unsigned char, slot, tb + sb);
    a.table = d_tab;
    int rc = mdhip_h2d_small(ctx, d_tab, by_frame ? (const void *)pl.runs.data() : (const void *)pl.blocks.data(), tb);
    if (rc || !by_frame) return rc;
    a.seg_msum = reinterpret_cast<const double *>(d_tab + tb);
    a.seg_qsi = n_sums > (size_t)a.n_seg ? a.seg_msum + a.n_seg : nullptr;
    return mdhip_h2d_small(ctx, d_tab + tb, sums, sb);
}

constexpr int seg_case(int form, int cap) { return form == SEG_WALK ? 0 : form * 2048 + cap; }

// The one place that launches a segment kernel: the plan's (form, stage size) names the instance
template <bool FLUX>
int seg_launch(mdhip_ctx *ctx, const SegPlan &pl, const SegArgs &a)
{
    const dim3 grid(pl.gx, pl.gy), block((unsigned)pl.threads);
    ctx->last_kernel = pl.name;
#define SEG_STAGED(CAP, NT)                                                                                              \
    hipLaunchKernelGGL((segment_staged_kernel<FLUX, CAP, NT>), grid, block, 0, ctx->stream, a.attr, a.mass, a.q, a.seg_off, \
                       (const SegBlock *)a.table, a.out, a.n_attr, a.n_atoms, a.n_seg, a.n_frames, a.vel_conv,           \
                       a.charge_conv, pl.vec)
#define SEG_FRAME(CAP)                                                                                                   \
    hipLaunchKernelGGL((segment_frame_kernel<FLUX, CAP>), grid, block, 0, ctx->stream, a.attr, a.mass, a.seg_msum,        \
                       a.seg_qsi, a.seg_off, (const SegRun *)a.table, a.out, a.n_attr, a.n_atoms, a.n_seg, pl.n_steps,    \
                       a.vel_conv)
    switch (seg_case(pl.form, pl.cap)) {
    case seg_case(SEG_FRAME, 512): SEG_FRAME(512); break;
    case seg_case(SEG_FRAME, 1024): SEG_FRAME(1024); break;
    case seg_case(SEG_STAGED, 256): SEG_STAGED(256, 64); break;
    case seg_case(SEG_STAGED, 512): SEG_STAGED(512, 256); break;
    case seg_case(SEG_STAGED, 1024): SEG_STAGED(1024, 256); break;
    case seg_case(SEG_WALK, 0):
        if constexpr (FLUX)
            hipLaunchKernelGGL(mol_flux_kernel, grid, block, 0, ctx->stream, a.attr, a.mass, a.q, a.seg_off, a.out, a.n_atoms,
                               a.n_seg, a.n_frames, a.vel_conv, a.charge_conv);
        else
            hipLaunchKernelGGL(segment_com_kernel, grid, block, 0, ctx->stream, a.attr, a.mass, a.seg_off, a.out, a.n_attr,
                               a.n_atoms, a.n_seg, a.n_frames);
        break;
    default: MD_REQUIRE(false, "no segment kernel of form %d with a stage of %d atoms", pl.form, pl.cap);
    }
#undef SEG_STAGED
#undef SEG_FRAME
    return MDHIP_OK;
}

}  // namespace

extern "C" {

int mdhip_segment_com(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, int n_attr,
                      const double *attr, int attr_on_device, const double *atom_mass,
                      const double *atom_q, int64_t n_seg, const int64_t *seg_off, double *out,
                      int out_on_device, double *seg_mass, double *seg_q)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_attr >= 0, "negative sizes");
    MD_REQUIRE(atom_mass || n_atoms == 0, "atom_mass is NULL");
    int rc = check_segments(ctx, n_atoms, n_seg, seg_off);
    if (rc) return rc;
    // sums that do not depend on the frame are done on the host, in index order
    const std::vector<double> sums = seg_sums(n_seg, seg_off, atom_mass, atom_q);
    if (seg_mass) std::copy_n(sums.begin(), n_seg, seg_mass);
    if (seg_q && atom_q) std::copy_n(sums.begin() + n_seg, n_seg, seg_q);
    if (n_frames == 0 || n_seg == 0 || n_attr == 0) return cs.end();
    MD_REQUIRE(attr && out, "NULL attr/out");
    MD_HIP(hipSetDevice(ctx->device));
    const double *d_attr = (const double *)mdhip_stage(ctx, WS_AUX0, attr,
                                                       (size_t)n_frames * n_attr * n_atoms * 8,
                                                       attr_on_device, &rc);
    if (rc) return rc;
    MD_WS(d_mass, double, WS_AUX1, (size_t)n_atoms * 8);
    rc = mdhip_h2d_small(ctx, d_mass, atom_mass, (size_t)n_atoms * 8);
    if (rc) return rc;
    MD_WS(d_off, long long, WS_AUX2, (size_t)(n_seg + 1) * 8);
    rc = mdhip_h2d_small(ctx, d_off, seg_off, (size_t)(n_seg + 1) * 8);
    if (rc) return rc;
    const size_t out_b = (size_t)n_frames * n_attr * n_seg * 8;
    double *d_out = out;
    if (!out_on_device) {
        d_out = (double *)mdhip_ws(ctx, WS_OUT, out_b);
        if (!d_out) return MDHIP_ENOMEM;
    }
    const SegPlan pl = seg_plan(seg_options(ctx), ctx->cu_count, n_seg, seg_off, n_attr, n_frames, false);
    SegArgs a = {d_attr, d_mass, nullptr, d_off, d_out, n_attr, n_atoms, n_seg, n_frames, 1.0, 1.0};
    rc = seg_stage_tables(ctx, WS_AUX3, pl, sums.data(), (size_t)n_seg, a);
    if (rc) return rc;
    KernelTimer timer(ctx);
    rc = seg_launch<false>(ctx, pl, a);
    timer.stop();
    if (rc) return rc;
    MD_HIP(hipGetLastError());
    if (!out_on_device) {
        rc = mdhip_result(cs, out, d_out, out_b, 0);
        if (rc) return rc;
    }
    return mdhip_end_timed(cs, timer);
}

static int charge_flux_impl(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *vel,
                            int on_device, const double *atom_mass, const double *atom_q, int64_t n_seg,
                            const int64_t *seg_off, const int32_t *seg_type, int n_types,
                            double vel_conv, double charge_conv, double *flux, int flux_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_types >= 0, "negative sizes");
    MD_REQUIRE(n_frames < 65536LL * 65536LL, "too many frames");
    int rc = check_segments(ctx, n_atoms, n_seg, seg_off);
    if (rc) return rc;
    MD_REQUIRE(flux || n_frames == 0 || n_types == 0, "flux is NULL");
    if (n_frames == 0 || n_types == 0) return cs.end();
    MD_REQUIRE(vel && atom_mass && atom_q && seg_type, "NULL input");
    // molecules of one type must be contiguous (they are: ids are type-major, com_mols.py:31-42)
    std::vector<long long> type_off(n_types + 1, 0);
    {
        int64_t s = 0;
        for (int t = 0; t < n_types; ++t) {
            type_off[t] = s;
            while (s < n_seg && seg_type[s] == t) ++s;
        }
        type_off[n_types] = s;
        MD_REQUIRE(s == n_seg, "seg_type must be non-decreasing in 0..n_types-1");
    }
    MD_HIP(hipSetDevice(ctx->device));
    const double *d_vel = (const double *)mdhip_stage(ctx, WS_AUX0, vel, (size_t)n_frames * 3 * n_atoms * 8,
                                                      on_device, &rc);
    if (rc) return rc;
    MD_WS(d_mq, double, WS_AUX1, (size_t)n_atoms * 16);
    {
        // masses | charges and segment offsets | type offsets: pinned staging of the call, one copy each
        MD_PIN(h_mq, double, (size_t)n_atoms * 16);
        memcpy(h_mq, atom_mass, (size_t)n_atoms * 8);
        memcpy(h_mq + n_atoms, atom_q, (size_t)n_atoms * 8);
        MD_HIP(hipMemcpyAsync(d_mq, h_mq, (size_t)n_atoms * 16, hipMemcpyHostToDevice, ctx->stream));
    }
    MD_WS(d_off, long long, WS_AUX2, (size_t)(n_seg + 1 + n_types + 1) * 8);
    {
        MD_PIN(h_off, long long, (size_t)(n_seg + 1 + n_types + 1) * 8);
        memcpy(h_off, seg_off, (size_t)(n_seg + 1) * 8);
        memcpy(h_off + n_seg + 1, type_off.data(), (size_t)(n_types + 1) * 8);
        MD_HIP(hipMemcpyAsync(d_off, h_off, (size_t)(n_seg + 1 + n_types + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    MD_WS(d_tmp, double, WS_AUX3, (size_t)n_frames * 3 * n_seg * 8);
    const size_t flux_b = (size_t)3 * n_types * n_frames * 8;
    double *d_flux = flux;
    if (!flux_on_device) {
        d_flux = (double *)mdhip_ws(ctx, WS_OUT, flux_b);
        if (!d_flux) return MDHIP_ENOMEM;
    }
    const SegPlan pl = seg_plan(seg_options(ctx), ctx->cu_count, n_seg, seg_off, 3, n_frames, true);
    std::vector<double> sums;  // by frame: per segment the mass sum, then (charge sum) x charge_conv
    if (pl.form == SEG_FRAME) {
        sums = seg_sums(n_seg, seg_off, atom_mass, atom_q);
        for (int64_t sg = 0; sg < n_seg; ++sg) sums[(size_t)(n_seg + sg)] *= charge_conv;  // _conductivity.py:25
    }
    SegArgs a = {d_vel, d_mq, d_mq + n_atoms, d_off, d_tmp, 3, n_atoms, n_seg, n_frames, vel_conv, charge_conv};
    rc = seg_stage_tables(ctx, WS_PART, pl, sums.data(), sums.size(), a);
    if (rc) return rc;
    KernelTimer timer(ctx);
    rc = seg_launch<true>(ctx, pl, a);
    timer.stop();
    if (rc) return rc;
    MD_HIP(hipGetLastError());
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {
        const unsigned nf = (unsigned)std::min<int64_t>(65535, n_frames - f0);
        // frames beyond 65535 are handled by offsetting the pointers
        hipLaunchKernelGGL(type_sum_kernel, dim3((unsigned)n_types, 3, nf), dim3(256), 0, ctx->stream,
                           d_tmp + (size_t)f0 * 3 * n_seg, d_off + n_seg + 1, d_flux + f0,
                           (long long)n_seg, (long long)n_frames, n_types);
        MD_HIP(hipGetLastError());
    }
    if (!flux_on_device) {
        rc = mdhip_result(cs, flux, d_flux, flux_b, 0);
        if (rc) return rc;
    }
    return mdhip_end_timed(cs, timer);
}

int mdhip_charge_flux(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *vel,
                      int on_device, const double *atom_mass, const double *atom_q, int64_t n_seg,
                      const int64_t *seg_off, const int32_t *seg_type, int n_types,
                      double vel_conv, double charge_conv, double *flux)
{
    return charge_flux_impl(ctx, n_frames, n_atoms, vel, on_device, atom_mass, atom_q, n_seg, seg_off, seg_type,
                            n_types, vel_conv, charge_conv, flux, 0);
}

int mdhip_charge_flux_dev(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *vel,
                          int on_device, const double *atom_mass, const double *atom_q, int64_t n_seg,
                          const int64_t *seg_off, const int32_t *seg_type, int n_types,
                          double vel_conv, double charge_conv, double *flux_dev)
{
    return charge_flux_impl(ctx, n_frames, n_atoms, vel, on_device, atom_mass, atom_q, n_seg, seg_off, seg_type,
                            n_types, vel_conv, charge_conv, flux_dev, 1);
}

int mdhip_charge_flux_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *vel, int on_device,
                            const double *atom_mass, const double *atom_q, int64_t n_seg, const int64_t *seg_off,
                            const int32_t *seg_type, int n_types, double vel_conv, double charge_conv, double *flux,
                            int flux_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    AsyncCall mark(ctx);
    return charge_flux_impl(ctx, n_frames, n_atoms, vel, on_device, atom_mass, atom_q, n_seg, seg_off, seg_type, n_types,
                            vel_conv, charge_conv, flux, flux_on_device ? 1 : 0);
}

int mdhip_segment_com_async(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, int n_attr, const double *attr,
                            int attr_on_device, const double *atom_mass, const double *atom_q, int64_t n_seg,
                            const int64_t *seg_off, double *out, int out_on_device, double *seg_mass, double *seg_q)
{
    if (!ctx) return MDHIP_EINVAL;
    AsyncCall mark(ctx);
    return mdhip_segment_com(ctx, n_frames, n_atoms, n_attr, attr, attr_on_device, atom_mass, atom_q, n_seg, seg_off, out,
                             out_on_device, seg_mass, seg_q);
}

}  // extern "C"
