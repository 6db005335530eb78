// hbonds.hip — hydrogen bonds of structural/hydrogen_bonds.py (calc_hydrogen_bonds, calc_hbond_lifetime): which
// D-H...A bonds exist in every frame, how many each donor gives and each acceptor takes, the distribution of the angle,
// and how long a bond lives. The reference has no such function; the definition is in DESIGN.md (hydrogen bonds) and
// restated in tests/hbonds_ref.py.
//
// One frame, donor d (a heavy atom) with its hydrogens h (CSR rows h_off / h_atoms), acceptor a:
//   the atom of a is not the atom of d, and mol_of[a] != mol_of[d] under exclusion;
//   shell::rsq(d, a) < r_da_sq (strict; the |d| form of the single wrap);
//   shell::rsq(h, a) < r_ha_sq, when r_ha_sq > 0;
//   u = shell::wrap_signed(x_d - x_h), v = shell::wrap_signed(x_a - x_h),
//   cos = ((ux vx + uy vy) + uz vz) / (sqrt((ux ux + uy uy) + uz uz) * sqrt((vx vx + vy vy) + vz vz)), unfused,
//     correctly rounded sqrt and division; a NaN cosine is no bond and counts in n_degenerate;
//   bonded when cos <= cos_cut (the angle D-H...A is at least angle_cut).
// Contraction is off in this file.
//
//  1. shell::gather_kernel (shell_gather.h): one lane per (frame, acceptor): the acceptor planes [F][3][n_acc], so that
//     the sweep reads coalesced planes of only the atoms that can accept.
//  2. hb_search_kernel<LIFE>: the sweep of shell_search.h, the donors as centres against the acceptor planes with
//     r_da_sq. A hit (rare) walks the donor's hydrogens through the tests above (hb_walk).
//       counts (LIFE = false): every (h, a) that reaches the angle test is binned by its cosine into the block's LDS
//         histogram of its class pair (the rule of angles.hip against the block's LDS copy of cos_edges: the binary
//         search in device memory took 2.3 of the call's 16.0 ms), which goes to the global uint64 bins once per block; a bond adds to n_bonds[f][dc][ac], n_donated[d] and n_accepted[a] (global atomics: a few per
//         donor and frame).
//       lifetime (LIFE = true): a bond sets bit f of the presence mask of the pair hpos * n_acc + apos
//         (presence_table.h).
//  3. lifetime only: presence::lag_kernel (the intermittent sums c_int) and hb_runs_kernel (the continuous ones): a
//     wave per occupied slot stages the mask in LDS; a lane takes the words w = lane, lane + 64, ..., finds the bits
//     that END a run of ones (bit t set, bit t + 1 clear) and walks back to the run's start, through whole words of
//     ones where it must. The run lengths L are counted in runs[L]: L < HB_RUNS_LDS in the block's LDS histogram
//     (merged with 64-bit atomics once per block), longer ones — few: such a run is HB_RUNS_LDS frames of one pair —
//     straight in device memory. The host finishes with two exact integer suffix sums: a run of L ones holds
//     max(0, L - k) windows of k + 1 consecutive ones, so with A[j] = sum_{L > j} runs[L],
//     c_cont[k] = sum_{j >= k} A[j].

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_gather.h"

#include "presence_table.h"

namespace {

constexpr int HB_MAX_CELLS = 4096;  // n_dc * n_ac * n_bins: the counts sweep keeps its histogram (32 KB) and the edges
                                    // (n_bins <= n_cells: 32 KB) in LDS
constexpr int HB_MAX_CLASSES = 64;  // n_dc * n_ac
constexpr int HB_RUNS_LDS = 4096;   // run lengths below this are counted in LDS (32 KB)

// what both searches read (device pointers; by value: wave-uniform loads)
struct HbGeom {
    const double *planes;  // [F][3][n_acc]
    long long n_acc;
    const int *don_class, *h_off, *h_atoms, *acc, *acc_class, *mol_of;
    double r_ha_sq, cos_cut;
};

// The hydrogens of the donor of row r against acceptor position a, which the sweep found at rsq(d, a) < r_da_sq:
// degenerate() for a NaN cosine, else angle(cos) for every (h, a) that reaches the angle test and bond(hpos) for
// those that pass it.
template <class Degenerate, class Angle, class Bond>
__device__ __forceinline__ void hb_walk(const HbGeom &g, const shell::Row &r, long long a, Degenerate degenerate,
                                        Angle angle, Bond bond)
{
    if (shell::excluded(g.acc[a], r.ci, g.mol_of)) return;
    const auto [ax, ay, az] = shell::cand_xyz(g.planes, g.n_acc, r.f, a);
    for (int k = g.h_off[r.c]; k < g.h_off[r.c + 1]; ++k) {
        const int hi = g.h_atoms[k];
        const double hx = r.px[hi], hy = r.py[hi], hz = r.pz[hi];
        if (g.r_ha_sq > 0.0 && !(shell::rsq(hx, hy, hz, ax, ay, az, r.Lx, r.Ly, r.Lz) < g.r_ha_sq)) continue;
        const double ux = shell::wrap_signed(r.cx - hx, r.Lx), uy = shell::wrap_signed(r.cy - hy, r.Ly),
                     uz = shell::wrap_signed(r.cz - hz, r.Lz);
        const double vx = shell::wrap_signed(ax - hx, r.Lx), vy = shell::wrap_signed(ay - hy, r.Ly),
                     vz = shell::wrap_signed(az - hz, r.Lz);
        const double dot = (ux * vx + uy * vy) + uz * vz;
        const double nu = __builtin_sqrt((ux * ux + uy * uy) + uz * uz);
        const double nv = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
        const double cs = dot / (nu * nv);
        if (cs != cs) {
            degenerate();
            continue;
        }
        angle(cs);
        if (cs <= g.cos_cut) bond(k);
    }
}

// what a mode of the search writes
struct HbCounts {
    int n_dc, n_ac, n_bins;
    const double *edges;                      // [n_bins]
    int *n_bonds;                             // [F][n_dc][n_ac]
    unsigned long long *n_donated, *n_accepted;
    unsigned long long *hist;                 // [n_dc][n_ac][n_bins], then n_degenerate
};
struct HbLife {
    presence::Table tb;
    unsigned max_probe;
    unsigned long long *stat;  // [0] += bonds, [1] = 1 when a bond found no slot
};

template <bool LIFE>
__global__ __launch_bounds__(shell::THREADS) void hb_search_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ box, const int *__restrict__ donors,
    int n_don, double r_da_sq, shell::Grid grid, HbGeom g, std::conditional_t<LIFE, HbLife, HbCounts> o)
{
    extern __shared__ unsigned long long s_hb_hist[];  // counts: the histogram [n_cells] | the edges [n_bins] (double)
    double *s_edges = nullptr;
    if constexpr (!LIFE) {
        s_edges = reinterpret_cast<double *>(s_hb_hist + o.n_dc * o.n_ac * o.n_bins);
        const int n_cells = o.n_dc * o.n_ac * o.n_bins;
        for (int b = threadIdx.x; b < n_cells; b += shell::THREADS) s_hb_hist[b] = 0ull;
        for (int b = threadIdx.x; b < o.n_bins; b += shell::THREADS) s_edges[b] = o.edges[b];
        __syncthreads();
    }
    unsigned long long mine = 0;  // (lifetime: this lane's bonds, and whether one of them found no slot)
    bool lost = false;
    shell::sweep(xyz, n, donors, n_don, g.planes, 3, g.n_acc, box, r_da_sq, grid,
                 [&](const shell::Row &r, size_t, long long a) {
                     if constexpr (LIFE) {
                         hb_walk(
                             g, r, a, []() {}, [](double) {},
                             [&](int hpos) {
                                 ++mine;
                                 const unsigned long long key = (unsigned long long)hpos * (unsigned long long)g.n_acc +
                                                                (unsigned long long)a;
                                 if (!presence::mark(o.tb, o.max_probe, key, r.f)) lost = true;
                             });
                     } else {
                         const int cell = g.don_class[r.c] * o.n_ac + g.acc_class[a];
                         hb_walk(
                             g, r, a,
                             [&]() { atomicAdd(&o.hist[(size_t)o.n_dc * o.n_ac * o.n_bins], 1ull); },
                             [&](double cs) {
                                 if (o.n_bins == 0) return;
                                 int lo = 0, hi = o.n_bins;  // cs <= E[m] for every m in [1, lo], not for m = hi
                                 while (hi - lo > 1) {
                                     const int mid = (lo + hi) >> 1;
                                     if (cs <= s_edges[mid]) lo = mid; else hi = mid;
                                 }
                                 atomicAdd(&s_hb_hist[cell * o.n_bins + lo], 1ull);
                             },
                             [&](int) {
                                 atomicAdd(&o.n_bonds[(size_t)r.f * (size_t)(o.n_dc * o.n_ac) + cell], 1);
                                 atomicAdd(&o.n_donated[r.c], 1ull);
                                 atomicAdd(&o.n_accepted[a], 1ull);
                             });
                     }
                 });
    if constexpr (!LIFE) {
        const int n_cells = o.n_dc * o.n_ac * o.n_bins;
        __syncthreads();
        for (int b = threadIdx.x; b < n_cells; b += shell::THREADS)
            if (s_hb_hist[b]) atomicAdd(&o.hist[b], s_hb_hist[b]);
    } else {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(o.stat, mine);
        if (lost) atomicOr(o.stat + 1, 1ull);
    }
}

// One wave per occupied slot (grid-stride over the table). runs [n_frames + 1]: runs[L] += the runs of exactly L ones;
// stat[2] += occupied slots. LDS: the mask [words] + the histogram [HB_RUNS_LDS] (u64).
__global__ __launch_bounds__(64) void hb_runs_kernel(presence::Table tb, unsigned long long *__restrict__ runs,
                                                     unsigned long long *__restrict__ stat)
{
    extern __shared__ unsigned long long s_runs[];
    const int words = tb.words, lane = threadIdx.x;
    unsigned long long *hist = s_runs;               // [HB_RUNS_LDS]
    unsigned long long *mask = s_runs + HB_RUNS_LDS;  // [words]
    for (int b = lane; b < HB_RUNS_LDS; b += 64) hist[b] = 0ull;
    unsigned long long n_pairs = 0;
    for (unsigned long long r = blockIdx.x; r < tb.slots; r += gridDim.x) {
        if (tb.keys[r] == presence::EMPTY) continue;  // (wave-uniform)
        ++n_pairs;
        __syncthreads();  // (the previous pair's runs have read the mask)
        for (int w = lane; w < words; w += 64) mask[w] = tb.masks[(size_t)r * (size_t)words + w];
        __syncthreads();
        for (int w = lane; w < words; w += 64) {
            const unsigned long long m = mask[w], next = w + 1 < words ? mask[w + 1] : 0ull;
            unsigned long long ends = m & ~((m >> 1) | (next << 63));  // bit t set, bit t + 1 clear
            while (ends) {
                const int e = __builtin_ctzll(ends);
                ends &= ends - 1ull;
                const unsigned long long zeros_below = ~m & ((1ull << e) - 1ull);
                long long L;
                if (zeros_below) {
                    L = e - (63 - __builtin_clzll(zeros_below));  // (the start is the bit above the highest zero)
                } else {  // the run reaches the bottom of the word: back through whole words of ones
                    L = e + 1;
                    int ww = w - 1;
                    while (ww >= 0 && mask[ww] == ~0ull) {
                        L += 64;
                        --ww;
                    }
                    if (ww >= 0) L += __builtin_clzll(~mask[ww]);  // (its leading ones; ~mask[ww] != 0)
                }
                if (L < HB_RUNS_LDS) atomicAdd(&hist[L], 1ull);
                else atomicAdd(&runs[L], 1ull);
            }
        }
    }
    __syncthreads();
    for (int b = lane; b < HB_RUNS_LDS; b += 64)
        if (hist[b]) atomicAdd(&runs[b], hist[b]);
    if (lane == 0 && n_pairs) atomicAdd(stat + 2, n_pairs);
}

struct HbInputs : shell::Inputs {
    HbGeom g;
    double *planes = nullptr;  // (g.planes, to write)
    shell::Grid grid;
    int n_h = 0;
};

// What both entry points check and stage (no launch): the shell search's inputs with the donors as centres, the
// integer tables and the room for the acceptor planes.
int hb_stage(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
             const double *box, int32_t n_don, const int32_t *donors, const int32_t *don_class, const int32_t *h_off,
             int32_t n_h, const int32_t *h_atoms, int32_t n_acc, const int32_t *acceptors, const int32_t *acc_class,
             int32_t n_dc, int32_t n_ac, const int32_t *mol_of, double r_ha_sq, double cos_cut, HbInputs &in)
{
    MD_REQUIRE(donors && don_class && h_off && acceptors && acc_class, "NULL array");
    MD_REQUIRE(h_atoms || n_h == 0, "NULL array");
    MD_REQUIRE(h_off[0] == 0 && h_off[n_don] == n_h, "h_off must run from 0 to n_h = %d", (int)n_h);
    for (int32_t d = 0; d < n_don; ++d) {
        MD_REQUIRE(h_off[d + 1] >= h_off[d], "h_off must not decrease (donor %d)", (int)d);
        MD_REQUIRE(don_class[d] >= 0 && don_class[d] < n_dc, "donor %d: class %d outside [0, %d)", (int)d,
                   (int)don_class[d], (int)n_dc);
    }
    for (int32_t a = 0; a < n_acc; ++a)
        MD_REQUIRE(acc_class[a] >= 0 && acc_class[a] < n_ac, "acceptor %d: class %d outside [0, %d)", (int)a,
                   (int)acc_class[a], (int)n_ac);
    int rc;
    if ((rc = shell::stage(ctx, "donor", n_frames, n_atoms, xyz, xyz_on_device, box, n_don, donors, in))) return rc;
    if ((rc = shell::check_indices(ctx, "hydrogen", n_h, h_atoms, 1, n_atoms))) return rc;
    if ((rc = shell::check_indices(ctx, "acceptor", n_acc, acceptors, 1, n_atoms))) return rc;

    // ints: the donors' classes | h_off | h_atoms | the acceptors' atoms | their classes | mol_of (under exclusion)
    shell::IntTable ints;
    ints.add(don_class, n_don, &in.g.don_class);
    ints.add(h_off, (size_t)n_don + 1, &in.g.h_off);
    ints.add(h_atoms, n_h, &in.g.h_atoms);
    ints.add(acceptors, n_acc, &in.g.acc);
    ints.add(acc_class, n_acc, &in.g.acc_class);
    ints.add_optional(mol_of, n_atoms, &in.g.mol_of);
    if ((rc = shell::upload_ints(ctx, ints, WS_TYPE_J))) return rc;
    if ((rc = shell::planes_room(ctx, n_frames, n_acc, in.planes))) return rc;
    in.g.planes = in.planes;
    in.g.n_acc = n_acc;
    in.g.r_ha_sq = r_ha_sq;
    in.g.cos_cut = cos_cut;
    in.grid = shell::sweep_grid(ctx, n_frames, n_don, n_acc);
    in.n_h = n_h;
    return MDHIP_OK;
}

}  // namespace

extern "C" {

int mdhip_hbond_counts(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                       const double *box, int32_t n_don, const int32_t *donors, const int32_t *don_class,
                       const int32_t *h_off, int32_t n_h, const int32_t *h_atoms, int32_t n_acc,
                       const int32_t *acceptors, const int32_t *acc_class, int32_t n_dc, int32_t n_ac,
                       const int32_t *mol_of, double r_da_sq, double r_ha_sq, double cos_cut, int32_t n_bins,
                       const double *cos_edges, int32_t *n_bonds, uint64_t *n_donated, uint64_t *n_accepted,
                       uint64_t *angle_hist, uint64_t *n_degenerate)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_don >= 0 && n_h >= 0 && n_acc >= 0 && n_bins >= 0, "negative sizes");
    MD_REQUIRE(n_dc >= 1 && n_ac >= 1 && (int64_t)n_dc * n_ac <= HB_MAX_CLASSES, "n_dc * n_ac must be in [1, %d]",
               HB_MAX_CLASSES);
    MD_REQUIRE((int64_t)n_dc * n_ac * n_bins <= HB_MAX_CELLS, "n_dc * n_ac * n_bins must be at most %d", HB_MAX_CELLS);
    MD_REQUIRE(r_da_sq >= 0.0, "r_da_sq must not be negative");
    MD_REQUIRE(n_degenerate && (n_frames == 0 || n_bonds) && (n_don == 0 || n_donated) && (n_acc == 0 || n_accepted),
               "NULL array");
    MD_REQUIRE(n_bins == 0 || (cos_edges && angle_hist), "NULL array");
    for (int32_t m = 1; m < n_bins; ++m)
        MD_REQUIRE(cos_edges[m] < cos_edges[m - 1], "cos_edges must be strictly decreasing (edge %d)", (int)m);
    const size_t n_cls = (size_t)n_dc * (size_t)n_ac, n_cells = n_cls * (size_t)n_bins;
    if (n_bonds) memset(n_bonds, 0, (size_t)n_frames * n_cls * 4);
    if (n_donated) memset(n_donated, 0, (size_t)n_don * 8);
    if (n_accepted) memset(n_accepted, 0, (size_t)n_acc * 8);
    if (angle_hist) memset(angle_hist, 0, n_cells * 8);
    *n_degenerate = 0;
    if (n_frames == 0 || n_don == 0 || n_acc == 0) return cs.end();
    HbInputs in;
    int rc;
    if ((rc = hb_stage(ctx, n_frames, n_atoms, xyz, xyz_on_device, box, n_don, donors, don_class, h_off, n_h, h_atoms,
                       n_acc, acceptors, acc_class, n_dc, n_ac, mol_of, r_ha_sq, cos_cut, in)))
        return rc;
    MD_WS(d_edges, double, WS_TABLES, (size_t)n_bins * 8);
    if ((rc = mdhip_h2d_small(ctx, d_edges, cos_edges, (size_t)n_bins * 8))) return rc;
    MD_WS(d_bonds, int, WS_OUT, (size_t)n_frames * n_cls * 4);
    MD_WS(d_atoms, unsigned long long, WS_OUT2, ((size_t)n_don + (size_t)n_acc) * 8);
    MD_WS(d_hist, unsigned long long, WS_HIST, (n_cells + 1) * 8);
    MD_HIP(hipMemsetAsync(d_bonds, 0, (size_t)n_frames * n_cls * 4, ctx->stream));
    MD_HIP(hipMemsetAsync(d_atoms, 0, ((size_t)n_don + (size_t)n_acc) * 8, ctx->stream));
    MD_HIP(hipMemsetAsync(d_hist, 0, (n_cells + 1) * 8, ctx->stream));

    KernelTimer timer(ctx, 2);
    ctx->last_kernel = "hb_search_kernel<false>";
    if ((rc = shell::gather(ctx, in.xyz, n_frames, n_atoms, in.g.acc, n_acc, in.planes))) return rc;
    hipLaunchKernelGGL(hb_search_kernel<false>, dim3(in.grid.grid), dim3(shell::THREADS),
                       (n_cells + (size_t)n_bins) * 8, ctx->stream, in.xyz, (long long)n_atoms, in.box, in.centres, (int)n_don, r_da_sq, in.grid, in.g,
                       HbCounts{(int)n_dc, (int)n_ac, (int)n_bins, d_edges, d_bonds, d_atoms, d_atoms + n_don, d_hist});
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, n_bonds, d_bonds, (size_t)n_frames * n_cls * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, n_donated, d_atoms, (size_t)n_don * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, n_accepted, d_atoms + n_don, (size_t)n_acc * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, angle_hist, d_hist, n_cells * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, n_degenerate, d_hist + n_cells, 8, 0))) return rc;
    return shell::finish(cs, timer);
}

int mdhip_hbond_lifetime(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                         const double *box, int32_t n_don, const int32_t *donors, const int32_t *h_off, int32_t n_h,
                         const int32_t *h_atoms, int32_t n_acc, const int32_t *acceptors, const int32_t *mol_of,
                         double r_da_sq, double r_ha_sq, double cos_cut, int32_t max_lag, int64_t table_slots,
                         uint64_t *c_int, uint64_t *c_cont, uint64_t *n_pairs, uint64_t *n_records)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);  // (synchronous throughout: the first sweep's counters steer the launches that follow)
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_don >= 0 && n_h >= 0 && n_acc >= 0 && table_slots >= 0,
               "negative sizes");
    MD_REQUIRE(n_frames <= presence::MAX_FRAMES, "at most %d frames per call (%lld given)", presence::MAX_FRAMES,
               (long long)n_frames);
    MD_REQUIRE(max_lag >= 0 && (max_lag < n_frames || max_lag == 0), "max_lag must be in [0, n_frames - 1]");
    MD_REQUIRE(r_da_sq >= 0.0, "r_da_sq must not be negative");
    MD_REQUIRE(c_int && c_cont && n_pairs && n_records, "NULL array");
    const int n_lags = (int)max_lag + 1;
    std::fill(c_int, c_int + n_lags, (uint64_t)0);
    std::fill(c_cont, c_cont + n_lags, (uint64_t)0);
    *n_pairs = *n_records = 0;
    if (n_frames == 0 || n_don == 0 || n_acc == 0 || n_h == 0) return cs.end();
    HbInputs in;
    int rc;
    std::vector<int32_t> one_class((size_t)std::max(n_don, n_acc), 0);  // (the lifetime has no classes)
    if ((rc = hb_stage(ctx, n_frames, n_atoms, xyz, xyz_on_device, box, n_don, donors, one_class.data(), h_off, n_h,
                       h_atoms, n_acc, acceptors, one_class.data(), 1, 1, mol_of, r_ha_sq, cos_cut, in)))
        return rc;
    const int words = presence::words_of(n_frames);
    const size_t slot_b = presence::slot_bytes(words);
    const double max_pairs = (double)n_h * (double)n_acc;
    size_t mem_cap = 0;
    if ((rc = presence::budget(ctx, WS_AUX0, mem_cap))) return rc;

    MD_WS(d_stat, unsigned long long, WS_MISC, 64);
    // c_int [n_lags] | runs [n_frames + 1]
    const size_t n_out = (size_t)n_lags + (size_t)n_frames + 1;
    MD_WS(d_out, unsigned long long, WS_OUT, n_out * 8);
    MD_HIP(hipMemsetAsync(d_out, 0, n_out * 8, ctx->stream));
    MD_PIN(h_stat, unsigned long long, 64);
    MD_PIN(h_runs, unsigned long long, ((size_t)n_frames + 1) * 8);

    KernelTimer timer(ctx);
    ctx->last_kernel = "hb_search_kernel<true>";
    if ((rc = shell::gather(ctx, in.xyz, n_frames, n_atoms, in.g.acc, n_acc, in.planes))) return rc;
    // The table: one slot per (hydrogen, acceptor) pair that is ever bonded, at most half full. The first sweep's
    // comes from the acceptors expected within r_da of a donor in ONE frame, times its hydrogens, times 8: far more
    // than pass the angle test, and a pair that is bonded in one frame is mostly the same pair in the next. A call
    // whose table fills up all the same (uncorrelated frames) sweeps again, with slots from min(bonds, n_h * n_acc).
    unsigned long long slots;
    if (table_slots > 0) {
        slots = presence::pow2_at_least((double)table_slots, 4);
    } else {
        const double pi43 = 4.18879020478639;
        const double vol = box[0] * box[1] * box[2], r_da = std::sqrt(r_da_sq);
        const double share = vol > 0.0 ? std::min(1.0, pi43 * r_da * r_da * r_da / vol) : 1.0;
        slots = presence::pow2_at_least(2.0 * std::min(max_pairs * share * 8.0 + 65536.0, max_pairs));
        while (slots > 1024 && slots * slot_b > mem_cap) slots >>= 1;
    }
    MD_REQUIRE(slots * slot_b <= mem_cap || table_slots == 0, "table_slots = %lld: a pair table of %.1f GB does not fit",
               (long long)table_slots, (double)(slots * slot_b) / 1073741824.0);
    presence::Table tb;
    unsigned long long n_hit = 0;
    int launches = 1;
    for (int sweep = 0; sweep < 2; ++sweep) {
        if ((rc = presence::take(ctx, WS_AUX0, slots, words, tb))) return rc;
        MD_HIP(hipMemsetAsync(d_stat, 0, 64, ctx->stream));
        hipLaunchKernelGGL(hb_search_kernel<true>, dim3(in.grid.grid), dim3(shell::THREADS), 0, ctx->stream, in.xyz,
                           (long long)n_atoms, in.box, in.centres, (int)n_don, r_da_sq, in.grid, in.g,
                           HbLife{tb, presence::probes(sweep, slots), d_stat});
        MD_HIP(hipGetLastError());
        ++launches;
        MD_HIP(hipMemcpyAsync(h_stat, d_stat, 16, hipMemcpyDeviceToHost, ctx->stream));
        MD_HIP(mdhip_stream_wait(ctx));
        n_hit = h_stat[0];
        if (h_stat[1] == 0) break;
        MD_REQUIRE(sweep == 0, "hbond lifetime: the pair table filled up although it was sized from the bond count");
        const double pairs = std::min((double)n_hit, max_pairs);  // distinct pairs: at most one per bond
        slots = presence::pow2_at_least(2.0 * pairs, 4);
        if (slots * slot_b > mem_cap)
            return mdhip_fail(ctx, MDHIP_ELIMIT,
                              "hbond lifetime: %.0f bonded pairs over %lld frames need a pair table of %.1f GB; %.1f GB "
                              "of device memory can be had",
                              pairs, (long long)n_frames, (double)(slots * slot_b) / 1073741824.0,
                              (double)mem_cap / 1073741824.0);
    }
    KernelTimer lags(ctx, 2, true);  // the two lag kernels: the call's aux time
    if (n_hit > 0) {
        if ((rc = presence::lag_launch(ctx, tb, n_frames, n_lags, d_out))) return rc;
        const unsigned grid = (unsigned)std::min<unsigned long long>(slots, (unsigned long long)ctx->cu_count * 16);
        hipLaunchKernelGGL(hb_runs_kernel, dim3(grid), dim3(64), ((size_t)HB_RUNS_LDS + (size_t)words) * 8, ctx->stream,
                           tb, d_out + n_lags, d_stat);
        MD_HIP(hipGetLastError());
        launches += 2;
    }
    lags.stop();
    timer.stop();
    ctx->last_launches = launches;
    if ((rc = mdhip_result(cs, c_int, d_out, (size_t)n_lags * 8, 0))) return rc;
    MD_HIP(hipMemcpyAsync(h_runs, d_out + n_lags, ((size_t)n_frames + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    MD_HIP(hipMemcpyAsync(h_stat, d_stat, 24, hipMemcpyDeviceToHost, ctx->stream));
    const int64_t F = n_frames;
    cs.defer([=]() {
        // A[j] = runs longer than j; c_cont[k] = sum_{j >= k} A[j] (every lag up to F - 1 enters the sums)
        unsigned long long longer = 0, windows = 0;
        for (int64_t j = F - 1; j >= 0; --j) {
            longer += h_runs[j + 1];
            windows += longer;
            if (j < n_lags) c_cont[j] = windows;
        }
        *n_records = windows;  // (c_cont[0]: a run of L ones holds L set bits)
        *n_pairs = h_stat[2];
        return MDHIP_OK;
    });
    return shell::finish(cs, timer, &lags);
}

}  // extern "C"
