// free_volume.hip — free volume and cavity sizes (structural/free_volume.py; the reference has no such module): for every
// point of a regular grid over the periodic cell of every frame the distance to the nearest atom surface and the atom that
// attains it, and integer counts of these. include/mdhip.h (mdhip_free_volume) states every operation;
// tests/free_volume_ref.py restates them in numpy, brute force.
//
// The centres are grid points, 10^6 a frame, so the tile-against-chunk sweep of shell_search.h (every centre against every
// candidate) is the wrong organisation; here the atoms of every frame are put into a cell grid (cell_plan.h):
//   fv_bin_kernel      per (frame, atom): the wrapped fractions, the cell, a count per cell (integer atomics in device
//                      memory: no limit on the atoms of a frame); atoms that are ignored or not finite get no cell
//   fv_scan_kernel     per frame: the exclusive scan of the cell counts (one workgroup a frame, frames stride)
//   fv_scatter_kernel  per (frame, atom): its slot in its cell (an atomic cursor: the order inside a cell is that of
//                      arrival, and only minima over (s, index) and integer sums are formed from it) and its record in the
//                      cell-ordered planes x, y, z (wrapped), radius and the original index
//   fv_sweep_kernel    a workgroup takes a UNIT = (frame, cell, brick): up to CP_BRICK of the grid points that lie in the
//                      cell, four per lane. All of them share the neighbourhood: the distinct cells among the 27 around
//                      theirs. The neighbourhood's atoms are staged in LDS as ONE run, in chunks of FV_CHUNK, and every lane
//                      reads them there at the same address (a broadcast); rsq is shell_search.h's. The units of a batch
//                      are strided over by a grid that does not grow with frames or points.
// Counts go to the workgroup's 32-bit LDS bins and from there once into 64-bit device cells (rows beyond the LDS budget
// go straight there), n_free through eight LDS words per unit: integer atomics only, exact whatever the order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "call_tables.h"
#include "cell_plan.h"
#include "shell_search.h"  // (rsq: the single wrap of the shell searches)

namespace {

constexpr int FV_THREADS = 256;
constexpr int FV_PPL = CP_BRICK / FV_THREADS;  // grid points per lane
constexpr int FV_CHUNK = 1024;                 // atoms per LDS stage: 4 planes of doubles and the indices, 36 KiB
constexpr int FV_MAX_CLASSES = 16, FV_MAX_BINS = 4096, FV_MAX_PROBES = 8;
// LDS of the sweep: the stage, the bins and a few words stay under 64 KiB, so two to four workgroups share a CU's 160 KiB
// (MI355X_MICROARCH.md) and one hides the other's staging; the bins of a usual call (3 classes x 200) are 2.4 KiB
constexpr int FV_LDS_CELLS = 6144;
constexpr size_t FV_STAGE_BYTES = (size_t)FV_CHUNK * (4 * 8 + 4);
static_assert(FV_STAGE_BYTES + FV_LDS_CELLS * 4 + 1024 <= 64 * 1024, "the sweep's LDS must stay under 64 KiB");
static_assert(FV_PPL * FV_THREADS == CP_BRICK && FV_CHUNK % FV_THREADS == 0, "brick and chunk are whole rounds of the lanes");
constexpr size_t FV_BATCH_BYTES = (size_t)1 << 30;  // workspace of the frames in flight
constexpr long long FV_MAX_BATCH_UNITS = 1ll << 24;  // units of a batch of several frames (fv_batch_frames)
constexpr int FV_NO_ATOM = 0x7fffffff;

struct FvBatch {  // one batch of frames, everything on the device
    const double *xyz, *box;        // [Fb][3][n], [Fb][3]
    const CpFrame *fr;              // [Fb]
    const int *atom_class;          // [n]
    const double *radius, *edges, *probe;
    int *cellid;                    // [Fb][n]
    int *start, *cursor;            // [Fb][stride]
    double *planes;                 // [Fb][4][n]: wrapped x, y, z and the radius, cell-ordered
    int *index;                     // [Fb][n]: the atom of every slot
    long long Fb, n, units_per_frame;
    int stride, g[3], G;
    double rs2;
    int nbins, n_probes, n_classes, lds_bins, n_cells;
    unsigned long long *cnt;        // [n_cells]: hist | occupied | beyond
    unsigned long long *n_free;     // [Fb][n_probes], this batch's rows
    unsigned *free_map;             // [G] or NULL
    double *s_out;                  // [Fb][G] or NULL, this batch's rows
    int *nearest_out;
};

// pair_cull.hip's wrapped_frac
__device__ __forceinline__ double fv_frac(double x, double L)
{
    const double s = x / L;
    const double f = s - __builtin_floor(s);
    return f < 1.0 ? f : 0.0;
}

__global__ __launch_bounds__(FV_THREADS) void fv_bin_kernel(FvBatch b)
{
    const long long total = b.Fb * b.n;
    for (long long t = (long long)blockIdx.x * FV_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * FV_THREADS) {
        const long long f = t / b.n, i = t - f * b.n;
        const double *p = b.xyz + (size_t)f * 3 * (size_t)b.n + (size_t)i;
        const double x = p[0], y = p[(size_t)b.n], z = p[2 * (size_t)b.n];
        const double inf = __builtin_inf();
        int cell = -1;
        if (b.atom_class[i] >= 0 && __builtin_fabs(x) < inf && __builtin_fabs(y) < inf && __builtin_fabs(z) < inf) {
            const CpFrame fr = b.fr[f];
            const int cx = cp_cell_of(fv_frac(x, b.box[3 * f]), fr.nc[0]);
            const int cy = cp_cell_of(fv_frac(y, b.box[3 * f + 1]), fr.nc[1]);
            const int cz = cp_cell_of(fv_frac(z, b.box[3 * f + 2]), fr.nc[2]);
            cell = (cz * fr.nc[1] + cy) * fr.nc[0] + cx;
            atomicAdd(b.cursor + (size_t)f * b.stride + cell, 1);
        }
        b.cellid[t] = cell;
    }
}

// start[f][c] = the atoms in the cells before c, c = 0 .. cells (the last one: the atoms that have a cell); the cursor
// takes the same values. Lane i adds a run of consecutive cells, the 256 runs are scanned in LDS.
__global__ __launch_bounds__(FV_THREADS) void fv_scan_kernel(FvBatch b)
{
    __shared__ int s_part[FV_THREADS];
    const int tid = threadIdx.x;
    for (long long f = blockIdx.x; f < b.Fb; f += gridDim.x) {
        const int cells = (int)b.fr[f].cells();
        int *cur = b.cursor + (size_t)f * b.stride, *st = b.start + (size_t)f * b.stride;
        const int per = (cells + FV_THREADS - 1) / FV_THREADS;
        const int c0 = tid * per < cells ? tid * per : cells, c1 = c0 + per < cells ? c0 + per : cells;
        int sum = 0;
        for (int c = c0; c < c1; ++c) sum += cur[c];
        __syncthreads();  // (the previous frame's partial sums have been read)
        s_part[tid] = sum;
        __syncthreads();
        for (int w = 1; w < FV_THREADS; w <<= 1) {
            const int v = tid >= w ? s_part[tid - w] : 0;
            __syncthreads();
            s_part[tid] += v;
            __syncthreads();
        }
        int run = s_part[tid] - sum;
        for (int c = c0; c < c1; ++c) {
            const int k = cur[c];
            st[c] = run, cur[c] = run;
            run += k;
        }
        if (tid == FV_THREADS - 1) st[cells] = s_part[tid];
    }
}

__global__ __launch_bounds__(FV_THREADS) void fv_scatter_kernel(FvBatch b)
{
    const long long total = b.Fb * b.n;
    for (long long t = (long long)blockIdx.x * FV_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * FV_THREADS) {
        const int cell = b.cellid[t];
        if (cell < 0) continue;
        const long long f = t / b.n, i = t - f * b.n;
        const int slot = atomicAdd(b.cursor + (size_t)f * b.stride + cell, 1);
        const double *p = b.xyz + (size_t)f * 3 * (size_t)b.n + (size_t)i;
        double *q = b.planes + (size_t)f * 4 * (size_t)b.n + (size_t)slot;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double L = b.box[3 * f + ax];
            q[(size_t)ax * (size_t)b.n] = fv_frac(p[(size_t)ax * (size_t)b.n], L) * L;
        }
        q[3 * (size_t)b.n] = b.radius[b.atom_class[i]];
        b.index[(size_t)f * (size_t)b.n + (size_t)slot] = (int)i;
    }
}

// One count: into the workgroup's LDS bins, or straight into the device cells when the rows are beyond the LDS budget
__device__ __forceinline__ void fv_count(const FvBatch &b, unsigned *s_h, int cell)
{
    if (b.lds_bins) atomicAdd(s_h + cell, 1u);
    else atomicAdd(b.cnt + cell, 1ull);
}

// Dynamic LDS: [x, y, z, radius: FV_CHUNK doubles each][index: FV_CHUNK ints][bins: n_cells words when lds_bins]
__global__ __launch_bounds__(FV_THREADS) void fv_sweep_kernel(FvBatch b)
{
    extern __shared__ double s_dyn[];
    double *const s_x = s_dyn, *const s_y = s_x + FV_CHUNK, *const s_z = s_y + FV_CHUNK, *const s_r = s_z + FV_CHUNK;
    int *const s_i = reinterpret_cast<int *>(s_r + FV_CHUNK);
    unsigned *const s_h = reinterpret_cast<unsigned *>(s_i + FV_CHUNK);
    __shared__ int s_from[27], s_pre[28];
    __shared__ unsigned s_free[FV_MAX_PROBES];
    const int tid = threadIdx.x;
    if (b.lds_bins)
        for (int i = tid; i < b.n_cells; i += FV_THREADS) s_h[i] = 0u;
    const double top = b.edges[b.nbins];
    const long long units = b.Fb * b.units_per_frame;
    for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const long long f = unit / b.units_per_frame, rest = unit - f * b.units_per_frame;
        const CpFrame fr = b.fr[f];
        if (rest >= fr.units()) continue;  // (the batch's stride is that of its largest frame; uniform over the workgroup)
        const int cell = (int)(rest / fr.nsub), sub = (int)(rest - (long long)cell * fr.nsub);
        const int c[3] = {cell % fr.nc[0], (cell / fr.nc[0]) % fr.nc[1], cell / (fr.nc[0] * fr.nc[1])};
        int lo[3], np[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = cp_point_lo(c[a], b.g[a], fr.nc[a]);
            np[a] = cp_point_lo(c[a] + 1, b.g[a], fr.nc[a]) - lo[a];
        }
        const int npts = np[0] * np[1] * np[2], q0 = sub * CP_BRICK;  // (npts <= G <= 2^27)
        if (q0 >= npts) continue;
        const double L[3] = {b.box[3 * f], b.box[3 * f + 1], b.box[3 * f + 2]};
        // the neighbourhood: the runs of its distinct cells, and where each begins in the one run that is staged
        if (tid < FV_MAX_PROBES) s_free[tid] = 0u;
        if (tid < 27) {
            int nb[3][3], k[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) k[a] = cp_neighbours(c[a], fr.nc[a], nb[a]);
            const int dx = tid % 3, dy = (tid / 3) % 3, dz = tid / 9;
            int from = 0, count = 0;
            if (dx < k[0] && dy < k[1] && dz < k[2]) {
                const int *st = b.start + (size_t)f * b.stride + ((nb[2][dz] * fr.nc[1] + nb[1][dy]) * fr.nc[0] + nb[0][dx]);
                from = st[0], count = st[1] - st[0];
            }
            s_from[tid] = from, s_pre[tid + 1] = count;
        }
        __syncthreads();
        if (tid == 0) {
            s_pre[0] = 0;
            for (int r = 0; r < 27; ++r) s_pre[r + 1] += s_pre[r];
        }
        __syncthreads();
        const int T = s_pre[27];
        // the lane's points
        double px[FV_PPL], py[FV_PPL], pz[FV_PPL], best[FV_PPL];
        int who[FV_PPL], at[FV_PPL];
#pragma unroll
        for (int p = 0; p < FV_PPL; ++p) {
            const int q = q0 + tid + p * FV_THREADS;
            const int qq = q < npts ? q : q0;  // (a short last brick repeats its first point; masked below)
            const int kk = qq % np[2], jj = (qq / np[2]) % np[1], ii = qq / (np[2] * np[1]);
            const int i = lo[0] + ii, j = lo[1] + jj, k = lo[2] + kk;
            px[p] = cp_point_frac(i, b.g[0]) * L[0];
            py[p] = cp_point_frac(j, b.g[1]) * L[1];
            pz[p] = cp_point_frac(k, b.g[2]) * L[2];
            at[p] = q < npts ? (i * b.g[1] + j) * b.g[2] + k : -1;
            best[p] = __builtin_inf();
            who[p] = FV_NO_ATOM;
        }
        const double *plane = b.planes + (size_t)f * 4 * (size_t)b.n;
        const int *index = b.index + (size_t)f * (size_t)b.n;
        for (int base = 0; base < T; base += FV_CHUNK) {
            const int m = T - base < FV_CHUNK ? T - base : FV_CHUNK;
            __syncthreads();  // (the previous chunk has been read)
            for (int v = tid; v < m; v += FV_THREADS) {
                const int gpos = base + v;
                int r = 0;
                while (gpos >= s_pre[r + 1]) ++r;  // (gpos < T = s_pre[27] ends it)
                const int src = s_from[r] + (gpos - s_pre[r]);
                s_x[v] = plane[src];
                s_y[v] = plane[(size_t)b.n + src];
                s_z[v] = plane[2 * (size_t)b.n + src];
                s_r[v] = plane[3 * (size_t)b.n + src];
                s_i[v] = index[src];
            }
            __syncthreads();
            for (int v = 0; v < m; ++v) {
                const double ax = s_x[v], ay = s_y[v], az = s_z[v];
#pragma unroll
                for (int p = 0; p < FV_PPL; ++p) {
                    const double d2 = shell::rsq(px[p], py[p], pz[p], ax, ay, az, L[0], L[1], L[2]);
                    if (d2 < b.rs2) {
                        const double s = __builtin_sqrt(d2) - s_r[v];
                        const int j = s_i[v];
                        if (s < best[p] || (s == best[p] && j < who[p])) best[p] = s, who[p] = j;
                    }
                }
            }
        }
        // the values, the counts
        unsigned free_n[FV_MAX_PROBES];
#pragma unroll
        for (int k = 0; k < FV_MAX_PROBES; ++k) free_n[k] = 0u;
#pragma unroll
        for (int p = 0; p < FV_PPL; ++p) {
            if (at[p] < 0) continue;
            const bool none = who[p] == FV_NO_ATOM;
            const double s = best[p];
            const int nearest = none ? -1 : who[p];
            const size_t out = (size_t)f * (size_t)b.G + (size_t)at[p];
            if (b.s_out) b.s_out[out] = s;
            if (b.nearest_out) b.nearest_out[out] = nearest;
            if (none || s >= top) {
                fv_count(b, s_h, b.n_classes * b.nbins + b.n_classes);
            } else {
                const int lining = b.atom_class[nearest];
                if (s < 0.0) {
                    fv_count(b, s_h, b.n_classes * b.nbins + lining);
                } else {  // edges[lo_] <= s < edges[hi_] throughout: edges[0] == 0 <= s < edges[nbins]
                    int lo_ = 0, hi_ = b.nbins;
                    while (hi_ - lo_ > 1) {
                        const int mid = (lo_ + hi_) >> 1;
                        if (s < b.edges[mid]) hi_ = mid;
                        else lo_ = mid;
                    }
                    fv_count(b, s_h, lining * b.nbins + lo_);
                }
            }
#pragma unroll
            for (int k = 0; k < FV_MAX_PROBES; ++k)
                if (k < b.n_probes && (none || s >= b.probe[k])) ++free_n[k];
            if (b.free_map && (none || s >= b.probe[0])) atomicAdd(b.free_map + at[p], 1u);
        }
#pragma unroll
        for (int k = 0; k < FV_MAX_PROBES; ++k)
            if (free_n[k]) atomicAdd(s_free + k, free_n[k]);
        __syncthreads();
        if (tid < b.n_probes && s_free[tid])
            atomicAdd(b.n_free + (size_t)f * b.n_probes + tid, (unsigned long long)s_free[tid]);
    }
    __syncthreads();
    if (b.lds_bins)
        for (int i = tid; i < b.n_cells; i += FV_THREADS) {
            const unsigned n = s_h[i];
            if (n) atomicAdd(b.cnt + i, (unsigned long long)n);
        }
}

// How many frames one batch takes: what the workspace budget holds, and few enough units that no workgroup's 32-bit LDS
// bin can wrap: the grid is min(units, 8 per CU), so a workgroup takes at most units / 8 + 1 units of at most 2^10
// points: below 2^32 with units <= 2^24. A batch of ONE frame is always allowed: its points are at most 2^27 in all.
inline long long fv_batch_frames(long long n_frames, size_t bytes_per_frame, long long units_per_frame)
{
    long long fb = (long long)(FV_BATCH_BYTES / std::max<size_t>(bytes_per_frame, 1));
    fb = std::min(fb, FV_MAX_BATCH_UNITS / std::max<long long>(units_per_frame, 1));
    return std::max<long long>(1, std::min(fb, n_frames));
}

}  // namespace

extern "C" {

int mdhip_free_volume(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                      const double *box, const int32_t *atom_class, int32_t n_classes, const double *radius,
                      const int32_t *grid, double r_search, double r_search_sq, int32_t nbins, const double *edges,
                      int32_t n_probes, const double *probe, uint64_t *hist, uint64_t *occupied, uint64_t *beyond,
                      int64_t *n_free, uint32_t *free_map, double *s_out, int32_t *nearest_out, int field_on_device)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    const double inf = __builtin_inf();
    MD_REQUIRE(n_frames >= 1, "n_frames must be positive");
    MD_REQUIRE(n_atoms >= 1 && n_atoms < (1ll << 31), "n_atoms must be in [1, 2^31)");
    MD_REQUIRE(n_classes >= 1 && n_classes <= FV_MAX_CLASSES, "n_classes must be in [1, %d]", FV_MAX_CLASSES);
    MD_REQUIRE(nbins >= 1 && nbins <= FV_MAX_BINS, "nbins must be in [1, %d]", FV_MAX_BINS);
    MD_REQUIRE(n_probes >= 1 && n_probes <= FV_MAX_PROBES, "n_probes must be in [1, %d]", FV_MAX_PROBES);
    MD_REQUIRE(xyz && box && atom_class && radius && grid && edges && probe, "NULL array");
    MD_REQUIRE(hist || occupied || beyond || n_free || free_map || s_out || nearest_out,
               "every output is NULL: nothing to compute");
    MD_REQUIRE(grid[0] >= 1 && grid[1] >= 1 && grid[2] >= 1, "every grid dimension must be at least 1");
    const long long G = (long long)grid[0] * grid[1] <= (1ll << 27) ? (long long)grid[0] * grid[1] * grid[2] : (1ll << 28);
    MD_REQUIRE(G <= (1ll << 27), "the grid must hold at most 2^27 points");
    MD_REQUIRE(r_search > 0.0 && r_search < inf, "r_search must be positive and finite");
    MD_REQUIRE(r_search_sq == r_search * r_search && r_search_sq < inf, "r_search_sq must be the square of r_search as a double");
    MD_REQUIRE(edges[0] == 0.0, "edges must start at 0");
    for (int k = 0; k < nbins; ++k)
        MD_REQUIRE(edges[k + 1] > edges[k] && edges[k + 1] < inf, "edges must ascend and be finite (edge %d)", k + 1);
    for (int k = 0; k < n_probes; ++k)
        MD_REQUIRE(probe[k] >= 0.0 && probe[k] <= edges[nbins], "probe %d must be finite and in [0, edges[nbins]]", k);
    for (int k = 0; k < n_classes; ++k)
        MD_REQUIRE(radius[k] >= 0.0 && radius[k] < inf, "radius %d must be finite and not negative", k);
    for (int64_t i = 0; i < n_atoms; ++i)
        MD_REQUIRE(atom_class[i] >= -1 && atom_class[i] < n_classes, "atom %lld: class %d outside [-1, %d)", (long long)i,
                   (int)atom_class[i], (int)n_classes);
    for (int64_t k = 0; k < 3 * n_frames; ++k)
        MD_REQUIRE(box[k] > 0.0 && box[k] < inf, "frame %lld: box edges must be positive and finite", (long long)(k / 3));

    // the plan of every frame, and the largest of them: the stride of the cell tables and of the units of a batch
    std::vector<CpFrame> frames((size_t)n_frames);
    long long max_cells = 1, max_units = 1;
    for (int64_t f = 0; f < n_frames; ++f) {
        frames[(size_t)f] = cp_frame(box + 3 * f, grid, r_search);
        max_cells = std::max(max_cells, frames[(size_t)f].cells());
        max_units = std::max(max_units, frames[(size_t)f].units());
    }
    const int stride = (int)max_cells + 1;
    const bool field_ws = (s_out || nearest_out) && !field_on_device;
    const size_t n = (size_t)n_atoms;
    const size_t frame_bytes = n * 4 + 2 * (size_t)stride * 4 + 4 * n * 8 + n * 4 + (xyz_on_device ? 0 : 3 * n * 8) +
                               (field_ws ? (size_t)G * 12 : 0) + 3 * 8 + sizeof(CpFrame) + FV_MAX_PROBES * 8;
    const long long Fb = ctx->opt_fv_batch > 0 ? std::min<long long>(ctx->opt_fv_batch, fv_batch_frames(n_frames, 1, max_units))
                                               : fv_batch_frames(n_frames, frame_bytes, max_units);

    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const int n_cells = n_classes * nbins + n_classes + 1;
    FvBatch b;
    CallTables tab;
    tab.add(atom_class, n, &b.atom_class);
    tab.add(radius, (size_t)n_classes, &b.radius);
    tab.add(edges, (size_t)nbins + 1, &b.edges);
    tab.add(probe, (size_t)n_probes, &b.probe);
    if ((rc = upload_tables(ctx, tab, WS_TABLES))) return rc;
    MD_WS(d_cnt, unsigned long long, WS_HIST, (size_t)n_cells * 8);
    MD_HIP(hipMemsetAsync(d_cnt, 0, (size_t)n_cells * 8, ctx->stream));
    const size_t free_b = (size_t)n_frames * (size_t)n_probes * 8;
    MD_WS(d_free, unsigned long long, WS_MISC, free_b);
    MD_HIP(hipMemsetAsync(d_free, 0, free_b, ctx->stream));
    unsigned *d_map = nullptr;
    if (free_map) {
        d_map = (unsigned *)mdhip_ws(ctx, WS_OUT3, (size_t)G * 4);
        if (!d_map) return MDHIP_ENOMEM;
        MD_HIP(hipMemsetAsync(d_map, 0, (size_t)G * 4, ctx->stream));
    }
    MD_WS(d_box, double, WS_BOX, (size_t)Fb * 3 * 8);
    MD_WS(d_fr, CpFrame, WS_AUX0, (size_t)Fb * sizeof(CpFrame));
    MD_WS(d_cellid, int, WS_AUX1, (size_t)Fb * n * 4);
    MD_WS(d_start, int, WS_CELLS, (size_t)Fb * (size_t)stride * 4);
    MD_WS(d_cursor, int, WS_AUX2, (size_t)Fb * (size_t)stride * 4);
    MD_WS(d_planes, double, WS_SORT_XYZ, (size_t)Fb * 4 * n * 8);
    MD_WS(d_index, int, WS_SORT_TYPE, (size_t)Fb * n * 4);
    double *d_s = nullptr;
    int *d_near = nullptr;
    if (s_out && !field_on_device && !(d_s = (double *)mdhip_ws(ctx, WS_OUT, (size_t)Fb * (size_t)G * 8))) return MDHIP_ENOMEM;
    if (nearest_out && !field_on_device && !(d_near = (int *)mdhip_ws(ctx, WS_OUT2, (size_t)Fb * (size_t)G * 4))) return MDHIP_ENOMEM;

    b.box = d_box, b.fr = d_fr, b.cellid = d_cellid, b.start = d_start, b.cursor = d_cursor, b.planes = d_planes, b.index = d_index;
    b.n = n_atoms, b.units_per_frame = max_units, b.stride = stride;
    b.g[0] = grid[0], b.g[1] = grid[1], b.g[2] = grid[2], b.G = (int)G;
    b.rs2 = r_search_sq;
    b.nbins = nbins, b.n_probes = n_probes, b.n_classes = n_classes, b.n_cells = n_cells;
    b.lds_bins = n_cells <= FV_LDS_CELLS;
    b.cnt = d_cnt, b.free_map = d_map;
    const size_t lds = FV_STAGE_BYTES + (b.lds_bins ? (size_t)n_cells * 4 : 0);
    const long long max_grid = (long long)ctx->cu_count * 8;

    // the call's aux time: the pre-pass (bin, scan, scatter) of the FIRST batch
    KernelTimer timer(ctx, 0), pre(ctx, 0, true);
    int launches = 0;
    for (int64_t f0 = 0; f0 < n_frames; f0 += Fb) {
        const long long fb = std::min<long long>(Fb, n_frames - f0);
        const size_t xyz_b = (size_t)fb * 3 * n * 8;
        b.xyz = (const double *)mdhip_stage(ctx, WS_XYZ_I, xyz + (size_t)f0 * 3 * n, xyz_b, xyz_on_device, &rc);
        if (rc) return rc;
        if ((rc = mdhip_h2d_small(ctx, d_box, box + 3 * f0, (size_t)fb * 3 * 8))) return rc;
        if ((rc = mdhip_h2d_small(ctx, d_fr, frames.data() + f0, (size_t)fb * sizeof(CpFrame)))) return rc;
        b.Fb = fb;
        b.n_free = d_free + (size_t)f0 * (size_t)n_probes;
        b.s_out = s_out ? (field_on_device ? s_out + (size_t)f0 * (size_t)G : d_s) : nullptr;
        b.nearest_out = nearest_out ? (field_on_device ? nearest_out + (size_t)f0 * (size_t)G : d_near) : nullptr;
        MD_HIP(hipMemsetAsync(d_cursor, 0, (size_t)fb * (size_t)stride * 4, ctx->stream));
        const long long atoms = fb * (long long)n_atoms;
        const unsigned grid_a = (unsigned)std::min<long long>((atoms + FV_THREADS - 1) / FV_THREADS, max_grid);
        hipLaunchKernelGGL(fv_bin_kernel, dim3(grid_a), dim3(FV_THREADS), 0, ctx->stream, b);
        MD_HIP(hipGetLastError());
        hipLaunchKernelGGL(fv_scan_kernel, dim3((unsigned)std::min<long long>(fb, max_grid)), dim3(FV_THREADS), 0, ctx->stream, b);
        MD_HIP(hipGetLastError());
        hipLaunchKernelGGL(fv_scatter_kernel, dim3(grid_a), dim3(FV_THREADS), 0, ctx->stream, b);
        MD_HIP(hipGetLastError());
        if (f0 == 0) pre.stop();
        const long long units = fb * max_units;
        hipLaunchKernelGGL(fv_sweep_kernel, dim3((unsigned)std::min(units, max_grid)), dim3(FV_THREADS), lds, ctx->stream, b);
        MD_HIP(hipGetLastError());
        launches += 4;
        if (s_out && !field_on_device && (rc = mdhip_result(cs, s_out + (size_t)f0 * (size_t)G, d_s, (size_t)fb * (size_t)G * 8, 0))) return rc;
        if (nearest_out && !field_on_device &&
            (rc = mdhip_result(cs, nearest_out + (size_t)f0 * (size_t)G, d_near, (size_t)fb * (size_t)G * 4, 0)))
            return rc;
    }
    ctx->last_kernel = "fv_sweep_kernel";
    ctx->last_launches = launches;
    timer.stop();
    if (n_free && (rc = mdhip_result(cs, n_free, d_free, free_b, 0))) return rc;
    if (free_map && (rc = mdhip_result(cs, free_map, d_map, (size_t)G * 4, 0))) return rc;
    if (hist || occupied || beyond) {
        unsigned long long *h_cnt = (unsigned long long *)mdhip_pin(ctx, (size_t)n_cells * 8);
        if (!h_cnt) return MDHIP_ENOMEM;
        if ((rc = mdhip_copy_small(ctx, h_cnt, d_cnt, (size_t)n_cells * 8, hipMemcpyDeviceToHost))) return rc;
        const int nb = nbins, ncl = n_classes;
        cs.defer([=]() {
            if (hist) memcpy(hist, h_cnt, (size_t)ncl * nb * 8);
            if (occupied) memcpy(occupied, h_cnt + (size_t)ncl * nb, (size_t)ncl * 8);
            if (beyond) beyond[0] = h_cnt[(size_t)ncl * nb + ncl];
            return MDHIP_OK;
        });
    }
    return shell::finish(cs, timer, &pre);
}

}  // extern "C"
