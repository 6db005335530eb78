// sdf.hip — spatial distribution functions of structural/spatial_distribution.py (calc_spatial_distribution): the
// three-dimensional histogram of observed atoms in the body-fixed frame of a reference molecule. The reference has no
// such function; the arithmetic is specified in include/mdhip.h (mdhip_sdf_hist) and DESIGN.md (spatial distribution)
// and restated in tests/sdf_ref.py.
//
// One frame, one reference molecule with origin atom o, x-axis atom p and xy-plane atom q:
//   a = wrap(x_p - x_o), b = wrap(x_q - x_o) (shell::wrap_signed per axis);
//   na2 = (ax ax + ay ay) + az az, e1 = a / sqrt(na2); s = (bx e1x + by e1y) + bz e1z, c = b - s e1;
//   nc2 = (cx cx + cy cy) + cz cz, e2 = c / sqrt(nc2); e3 = e1 x e2; the row is degenerate when na2 or nc2 is zero or
//   not finite;
//   candidate j (class s) is a hit when j != o, mol_of[j] != mol_of[o] under exclusion, and shell::rsq(o, j) < r_cut**2;
//   d = wrap(x_j - x_o), p_k = (dx ekx + dy eky) + dz ekz, i_k = floor((p_k + r_cut) / bin_size) clamped to [0, G - 1]
//   (as doubles: NaN -> 0), hist[s][i1][i2][i3] += 1; a hit of a degenerate row counts in n_degenerate[s] instead.
// Contraction is off in this file.
//
//  1. shell::gather_kernel (shell_gather.h): one lane per (frame, candidate): the candidate planes [F][3][n_cand].
//  2. sdf_frames_kernel: one lane per (frame, molecule): rows of SDF_FRAME doubles, e1 e2 e3 and a valid flag, so that a
//     tile of 16 molecules is one contiguous run of 160 doubles; counts the degenerate rows.
//  3. sdf_sweep_kernel: the tile and chunk decomposition of shell::sweep (16 centres per block step with wave-uniform
//     loads, lanes on coalesced candidate planes), with three differences. The tile's frames, centre coordinates,
//     atoms and molecules are staged in LDS once per block step. The tile is swept SDF_PASS = 8 centres at a time, so
//     that their coordinates stay in SGPRs beside everything else the loop needs (a centre past a short tile's end and
//     a lane past the chunk's end carry NaN: no hit, no mask). And a hit is not handled where it is found: the
//     comparison of centre k is a wave-wide mask already, so its lanes rank themselves in it (mbcnt) and append 16-bit
//     records (centre-in-tile << 12 | candidate-in-chunk) to the wave's LDS queue. Whenever the queue holds a full
//     wave of records, 64 of them are taken off its end, one per lane: class, atom tests, projection, three cell
//     indices and one 64-bit atomic into the grid in HBM. What is left at the end of the step (< 64) is drained by a
//     partial wave. The queue's depth, SDF_QUEUE = 64 * (SDF_PASS + 1), is what can be left below a full wave plus the
//     largest burst of one sweep iteration (64 lanes x SDF_PASS centres): it cannot fill, so nothing is dropped and
//     nothing re-run. n_hits and n_degenerate are LDS counters, flushed per block step and per block.
//     The same hit as a functor on shell::sweep (handled where it is found, lane by lane) measured 1.40 times this
//     sweep's time at a hit share of 2.4 % (spatial distribution); it is not kept.

#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_gather.h"

namespace {

constexpr int SDF_MAX_SPECIES = 8;
constexpr int SDF_MAX_GRID = 256;
constexpr long long SDF_MAX_CELLS = 1ll << 25;  // n_species * G**3: 256 MB of uint64 cells
constexpr int SDF_FRAME = 10;                   // doubles per (frame, molecule): e1, e2, e3, valid (1.0 / 0.0)
constexpr int SDF_WAVES = shell::THREADS / 64;
constexpr int SDF_PASS = 8;                     // centres of the tile swept at a time
constexpr int SDF_QUEUE = 64 * (SDF_PASS + 1);  // records per wave (see above); 2 bytes each: 4.5 KB per block
constexpr int SDF_TEST_ATOM = 1;  // the candidate's atom is looked up: it may be the origin atom, or of its molecule

static_assert(shell::CHUNK <= 4096 && shell::TC <= 16 && shell::TC % SDF_PASS == 0, "a queue record is 4 + 12 bits");

__global__ __launch_bounds__(256) void sdf_frames_kernel(const double *__restrict__ xyz, long long n,
                                                         const double *__restrict__ box,
                                                         const int *__restrict__ origin, const int *__restrict__ x_atom,
                                                         const int *__restrict__ xy_atom, long long n_m, long long total,
                                                         double *__restrict__ frames,
                                                         unsigned long long *__restrict__ n_bad)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long m = i % n_m, f = i / n_m;
        const double *px = xyz + (size_t)f * 3 * (size_t)n, *py = px + n, *pz = py + n;
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const int o = origin[m], p = x_atom[m], q = xy_atom[m];
        const double ox = px[o], oy = py[o], oz = pz[o];
        const double ax = shell::wrap_signed(px[p] - ox, Lx), ay = shell::wrap_signed(py[p] - oy, Ly),
                     az = shell::wrap_signed(pz[p] - oz, Lz);
        const double bx = shell::wrap_signed(px[q] - ox, Lx), by = shell::wrap_signed(py[q] - oy, Ly),
                     bz = shell::wrap_signed(pz[q] - oz, Lz);
        const double na2 = (ax * ax + ay * ay) + az * az, na = __builtin_sqrt(na2);
        const double e1x = ax / na, e1y = ay / na, e1z = az / na;
        const double s = (bx * e1x + by * e1y) + bz * e1z;
        const double cx = bx - s * e1x, cy = by - s * e1y, cz = bz - s * e1z;
        const double nc2 = (cx * cx + cy * cy) + cz * cz, nc = __builtin_sqrt(nc2);
        const double e2x = cx / nc, e2y = cy / nc, e2z = cz / nc;
        const double inf = __builtin_inf();
        const bool valid = na2 > 0.0 && na2 < inf && nc2 > 0.0 && nc2 < inf;
        double *o_ = frames + (size_t)i * SDF_FRAME;
        o_[0] = e1x, o_[1] = e1y, o_[2] = e1z;
        o_[3] = e2x, o_[4] = e2y, o_[5] = e2z;
        o_[6] = e1y * e2z - e1z * e2y, o_[7] = e1z * e2x - e1x * e2z, o_[8] = e1x * e2y - e1y * e2x;
        o_[9] = valid ? 1.0 : 0.0;
        if (!valid) atomicAdd(n_bad, 1ull);
    }
}

// the grid of a call (by value: wave-uniform loads)
struct SdfBins {
    double r_cut, bin_size;
    int G;
};

// floor((p + r_cut) / bin_size) clamped to [0, G - 1]; the clamp is made on the double (NaN -> 0, +-Inf to the ends)
__device__ __forceinline__ int sdf_index(double p, const SdfBins &b)
{
    const double t = __builtin_floor((p + b.r_cut) / b.bin_size);
    return t >= (double)(b.G - 1) ? b.G - 1 : (t > 0.0 ? (int)t : 0);
}

// the cell of class `cls` that the wrapped d falls in under the frame fr = (e1, e2, e3)
__device__ __forceinline__ size_t sdf_cell(int cls, double dx, double dy, double dz, const double *fr, const SdfBins &b)
{
    const int i1 = sdf_index((dx * fr[0] + dy * fr[1]) + dz * fr[2], b);
    const int i2 = sdf_index((dx * fr[3] + dy * fr[4]) + dz * fr[5], b);
    const int i3 = sdf_index((dx * fr[6] + dy * fr[7]) + dz * fr[8], b);
    return (((size_t)cls * b.G + i1) * b.G + i2) * b.G + i3;
}

__device__ __forceinline__ void sdf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(shell::THREADS) void sdf_sweep_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ planes, long long n_cand,
    const double *__restrict__ box, const int *__restrict__ centres, int n_c, const int *__restrict__ cand,
    const int *__restrict__ cand_class, const int *__restrict__ mol_of, const double *__restrict__ frames, int tests,
    double rc2, SdfBins bins, shell::Grid g, unsigned long long *__restrict__ hist,
    unsigned long long *__restrict__ n_degenerate, int *__restrict__ n_hits)
{
    constexpr int TC = shell::TC, THREADS = shell::THREADS, CHUNK = shell::CHUNK;
    __shared__ double s_fr[TC * SDF_FRAME];
    __shared__ double s_cen[3 * TC];
    __shared__ unsigned long long s_deg[SDF_MAX_SPECIES];
    __shared__ int s_ci[TC], s_mol[TC], s_nh[TC];
    __shared__ unsigned short s_queue[SDF_WAVES][SDF_QUEUE];
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned short *queue = s_queue[tid >> 6];
    if (tid < TC) s_nh[tid] = 0;
    if (tid < SDF_MAX_SPECIES) s_deg[tid] = 0ull;

    for (long long blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const long long chunk = blk % g.n_chunks, rest = blk / g.n_chunks;
        const long long tile = rest % g.n_tiles, f = rest / g.n_tiles;
        const int c0 = (int)tile * TC;
        const int nc = n_c - c0 < TC ? n_c - c0 : TC;
        const double *px = xyz + (size_t)f * 3 * (size_t)n, *py = px + n, *pz = py + n;
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const double *qx = planes + (size_t)f * 3 * (size_t)n_cand, *qy = qx + n_cand, *qz = qy + n_cand;

        // the tile in LDS (every wave has drained the step before: the barrier that ends a step)
        if (tid < nc * SDF_FRAME) {
            s_fr[tid] = frames[((size_t)f * (size_t)n_c + (size_t)c0) * SDF_FRAME + tid];
        } else if (tid >= TC * SDF_FRAME && tid < TC * SDF_FRAME + 3 * TC) {
            const int j = tid - TC * SDF_FRAME, k = j % TC, axis = j / TC;
            const int ci = centres[k < nc ? c0 + k : c0];
            s_cen[j] = (axis == 0 ? px : (axis == 1 ? py : pz))[ci];
        } else if (tid >= TC * SDF_FRAME + 3 * TC && tid < TC * SDF_FRAME + 4 * TC) {
            const int k = tid - (TC * SDF_FRAME + 3 * TC);
            const int ci = centres[k < nc ? c0 + k : c0];
            s_ci[k] = ci;
            s_mol[k] = mol_of ? mol_of[ci] : 0;
        }
        __syncthreads();

        // one queued hit per lane
        auto drain = [&](unsigned rec) {
            const int k = (int)(rec >> 12);
            const long long a = chunk * CHUNK + (long long)(rec & 4095u);
            const int cls = cand_class[a];
            if (tests & SDF_TEST_ATOM) {
                const int aj = cand[a];
                if (aj == s_ci[k]) return;
                if (mol_of && mol_of[aj] == s_mol[k]) return;
            }
            atomicAdd(&s_nh[k], 1);
            const double *fr = s_fr + k * SDF_FRAME;
            if (fr[9] == 0.0) {
                atomicAdd(&s_deg[cls], 1ull);
                return;
            }
            const double dx = shell::wrap_signed(qx[a] - s_cen[k], Lx);
            const double dy = shell::wrap_signed(qy[a] - s_cen[TC + k], Ly);
            const double dz = shell::wrap_signed(qz[a] - s_cen[2 * TC + k], Lz);
            atomicAdd(&hist[sdf_cell(cls, dx, dy, dz, fr, bins)], 1ull);
        };

        const long long a0 = chunk * CHUNK;
        const long long a_end = a0 + CHUNK < n_cand ? a0 + CHUNK : n_cand;
        const int n_it = (int)((a_end - a0 + THREADS - 1) / THREADS);
        int qn = 0;  // records in this wave's queue (wave-uniform)
        for (int k0 = 0; k0 < nc; k0 += SDF_PASS) {  // (SDF_PASS centres at a time: their coordinates stay in SGPRs)
            double cx[SDF_PASS], cy[SDF_PASS], cz[SDF_PASS];
#pragma unroll
            for (int k = 0; k < SDF_PASS; ++k) {
                const int ci = centres[k0 + k < nc ? c0 + k0 + k : c0];
                cx[k] = k0 + k < nc ? px[ci] : __builtin_nan("");  // (past a short tile's end: NaN, no hits)
                cy[k] = py[ci];
                cz[k] = pz[ci];
            }
            for (int it = 0; it < n_it; ++it) {
                const int rel = it * THREADS + tid;
                const bool in = a0 + rel < a_end;
                const long long a = in ? a0 + rel : a_end - 1;
                const double x = in ? qx[a] : __builtin_nan(""), y = qy[a], z = qz[a];  // (past the chunk's end: no hits)
#pragma unroll
                for (int k = 0; k < SDF_PASS; ++k) {
                    const bool h = shell::rsq(cx[k], cy[k], cz[k], x, y, z, Lx, Ly, Lz) < rc2;
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(h);
                    if (h)
                        queue[qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                            (unsigned short)(((k0 + k) << 12) | rel);
                    qn += __builtin_popcountll(m);
                }
                while (qn >= 64) {  // full waves
                    qn -= 64;
                    sdf_wave_sync();
                    drain(queue[qn + lane]);
                    sdf_wave_sync();
                }
            }
        }
        sdf_wave_sync();
        if (lane < qn) drain(queue[lane]);
        __syncthreads();  // every wave's hits of this step are counted; s_fr and the queues are free
        if (tid < nc && s_nh[tid]) {
            atomicAdd(&n_hits[(size_t)f * (size_t)n_c + (size_t)(c0 + tid)], s_nh[tid]);
            s_nh[tid] = 0;
        }
    }
    __syncthreads();
    if (tid < SDF_MAX_SPECIES && s_deg[tid]) atomicAdd(&n_degenerate[tid], s_deg[tid]);
}

}  // namespace

extern "C" {

int mdhip_body_frames(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                      const double *box, int32_t n_mols, const int32_t *origin, const int32_t *x_atom,
                      const int32_t *xy_atom, double *frames, uint64_t *n_degenerate_rows)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_mols >= 0, "negative sizes");
    MD_REQUIRE(n_degenerate_rows, "NULL array");
    *n_degenerate_rows = 0;
    const size_t n_rows = (size_t)n_frames * (size_t)n_mols;
    if (n_rows == 0) return cs.end();
    MD_REQUIRE(frames && x_atom && xy_atom, "NULL array");
    shell::Inputs in;
    int rc;
    if ((rc = shell::stage(ctx, "origin", n_frames, n_atoms, xyz, xyz_on_device, box, n_mols, origin, in))) return rc;
    if ((rc = shell::check_indices(ctx, "x-axis atom", n_mols, x_atom, 1, n_atoms))) return rc;
    if ((rc = shell::check_indices(ctx, "xy-plane atom", n_mols, xy_atom, 1, n_atoms))) return rc;
    const int *d_xa, *d_xya;
    shell::IntTable ints;
    ints.add(x_atom, n_mols, &d_xa);
    ints.add(xy_atom, n_mols, &d_xya);
    if ((rc = shell::upload_ints(ctx, ints, WS_TYPE_J))) return rc;
    MD_WS(d_frames, double, WS_AUX2, n_rows * SDF_FRAME * 8);
    MD_WS(d_cnt, unsigned long long, WS_MISC, 8);
    MD_HIP(hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
    KernelTimer timer(ctx, 1);
    ctx->last_kernel = "sdf_frames_kernel";
    const unsigned fgrid = (unsigned)std::min<size_t>((n_rows + 255) / 256, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(sdf_frames_kernel, dim3(fgrid), dim3(256), 0, ctx->stream, in.xyz, (long long)n_atoms, in.box,
                       in.centres, d_xa, d_xya, (long long)n_mols, (long long)n_rows, d_frames, d_cnt);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, frames, d_frames, n_rows * SDF_FRAME * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, n_degenerate_rows, d_cnt, 8, 0))) return rc;
    return shell::finish(cs, timer);
}

int mdhip_sdf_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                   const double *box, int32_t n_centres, const int32_t *origin, const int32_t *x_atom,
                   const int32_t *xy_atom, int32_t n_cand, const int32_t *cand, const int32_t *cand_class,
                   int32_t n_species, const int32_t *mol_of, double r_cut, double r_cut_sq, double bin_size,
                   int32_t n_grid, uint64_t *hist, uint64_t *n_degenerate, int32_t *n_hits,
                   uint64_t *n_degenerate_rows)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_centres >= 0 && n_cand >= 0, "negative sizes");
    MD_REQUIRE(n_species >= 1 && n_species <= SDF_MAX_SPECIES, "n_species must be in [1, %d]", SDF_MAX_SPECIES);
    MD_REQUIRE(n_grid >= 1 && n_grid <= SDF_MAX_GRID, "n_grid must be in [1, %d]", SDF_MAX_GRID);
    const size_t n_cells = (size_t)n_species * (size_t)n_grid * (size_t)n_grid * (size_t)n_grid;
    MD_REQUIRE((long long)n_cells <= SDF_MAX_CELLS, "n_species * n_grid**3 must be at most %lld", SDF_MAX_CELLS);
    MD_REQUIRE(r_cut > 0.0 && r_cut < __builtin_inf() && bin_size > 0.0 && bin_size < __builtin_inf(),
               "r_cut and bin_size must be positive and finite");
    MD_REQUIRE(r_cut_sq >= 0.0, "r_cut_sq must not be negative");
    MD_REQUIRE(hist && n_degenerate && n_degenerate_rows, "NULL array");
    memset(n_degenerate, 0, (size_t)n_species * 8);
    *n_degenerate_rows = 0;
    const size_t n_rows = (size_t)n_frames * (size_t)n_centres;
    if (n_rows == 0) {
        memset(hist, 0, n_cells * 8);
        return cs.end();
    }
    MD_REQUIRE(n_hits && x_atom && xy_atom, "NULL array");
    MD_REQUIRE((cand && cand_class) || n_cand == 0, "NULL array");
    shell::Inputs in;
    int rc;
    if ((rc = shell::stage(ctx, "origin", n_frames, n_atoms, xyz, xyz_on_device, box, n_centres, origin, in)))
        return rc;
    if ((rc = shell::check_indices(ctx, "x-axis atom", n_centres, x_atom, 1, n_atoms))) return rc;
    if ((rc = shell::check_indices(ctx, "xy-plane atom", n_centres, xy_atom, 1, n_atoms))) return rc;
    if ((rc = shell::check_indices(ctx, "candidate", n_cand, cand, 1, n_atoms))) return rc;
    for (int32_t w = 0; w < n_cand; ++w)
        MD_REQUIRE(cand_class[w] >= 0 && cand_class[w] < n_species, "candidate %d: class %d out of range", (int)w,
                   (int)cand_class[w]);

    // is an origin atom a candidate?
    const int tests = (mol_of || shell::shares_an_atom(n_atoms, origin, n_centres, cand, n_cand)) ? SDF_TEST_ATOM : 0;
    // the tables: ints the x-axis atoms | the xy-plane atoms | the candidates' atoms | their classes | mol_of [n_atoms]
    // (under exclusion)
    const int *d_xa, *d_xya, *d_cand, *d_cls, *d_mol;
    shell::IntTable ints;
    ints.add(x_atom, n_centres, &d_xa);
    ints.add(xy_atom, n_centres, &d_xya);
    ints.add(cand, n_cand, &d_cand);
    ints.add(cand_class, n_cand, &d_cls);
    ints.add_optional(mol_of, n_atoms, &d_mol);
    if ((rc = shell::upload_ints(ctx, ints, WS_TYPE_J))) return rc;

    MD_WS(d_frames, double, WS_AUX2, n_rows * SDF_FRAME * 8);
    MD_WS(d_hits, int, WS_AUX0, n_rows * 4);
    MD_WS(d_hist, unsigned long long, WS_HIST, n_cells * 8);
    MD_WS(d_cnt, unsigned long long, WS_MISC, (SDF_MAX_SPECIES + 1) * 8);  // n_degenerate | the degenerate rows
    MD_HIP(hipMemsetAsync(d_hits, 0, n_rows * 4, ctx->stream));
    MD_HIP(hipMemsetAsync(d_hist, 0, n_cells * 8, ctx->stream));
    MD_HIP(hipMemsetAsync(d_cnt, 0, (SDF_MAX_SPECIES + 1) * 8, ctx->stream));

    KernelTimer timer(ctx, n_cand ? 3 : 1);
    KernelTimer pre(ctx, n_cand ? 2 : 1, true);  // the gather and the frames: the call's aux time; the rest is the sweep
    ctx->last_kernel = "sdf_sweep_kernel";
    const unsigned fgrid = (unsigned)std::min<size_t>((n_rows + 255) / 256, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(sdf_frames_kernel, dim3(fgrid), dim3(256), 0, ctx->stream, in.xyz, (long long)n_atoms, in.box,
                       in.centres, d_xa, d_xya, (long long)n_centres, (long long)n_rows, d_frames,
                       d_cnt + SDF_MAX_SPECIES);
    MD_HIP(hipGetLastError());
    if (n_cand) {
        double *d_planes;
        if ((rc = shell::planes_room(ctx, n_frames, n_cand, d_planes))) return rc;
        if ((rc = shell::gather(ctx, in.xyz, n_frames, n_atoms, d_cand, n_cand, d_planes))) return rc;
        pre.stop();
        const shell::Grid g = shell::sweep_grid(ctx, n_frames, n_centres, n_cand);
        hipLaunchKernelGGL(sdf_sweep_kernel, dim3(g.grid), dim3(shell::THREADS), 0, ctx->stream, in.xyz,
                           (long long)n_atoms, d_planes, (long long)n_cand, in.box, in.centres, (int)n_centres, d_cand,
                           d_cls, d_mol, d_frames, tests, r_cut_sq, SdfBins{r_cut, bin_size, (int)n_grid}, g, d_hist,
                           d_cnt, d_hits);
        MD_HIP(hipGetLastError());
    } else {
        pre.stop();
    }
    timer.stop();
    if ((rc = mdhip_result(cs, hist, d_hist, n_cells * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, n_degenerate, d_cnt, (size_t)n_species * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, n_degenerate_rows, d_cnt + SDF_MAX_SPECIES, 8, 0))) return rc;
    if ((rc = mdhip_result(cs, n_hits, d_hits, n_rows * 4, 0))) return rc;
    return shell::finish(cs, timer, &pre);
}

}  // extern "C"
