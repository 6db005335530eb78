// velocity_spectrum.hip — from a frame-major velocity trajectory to per-group power spectra and lag sums
// (dynamical/velocity_correlation.py, class VelocityCorrelation; the reference has no such module).
//
// mdhip_velocity_spectrum: the series s_e,a(t) = coef[e] * v[t][a][e] of every grouped entity, the column sums of
//   |X(j)|^2 over the entities of a group per axis, and the lag sums those spectra are the transform of
//   (autocorrelation theorem, zero padding to L >= n_frames + max_lag: the circular correlation is the linear one).
//   vs_gather_kernel       reads the trajectory through 64 x 64 tiles, entities along the lanes, multiplies by coef and
//                          writes time-major rows [row][n_frames]; the row of an entity comes from the row table of
//                          spectrum_plan.h (rows ordered (axis, group, entity): every (axis, group) a contiguous range;
//                          a batch = one axis of a range of entities with all their groups, so that every line of
//                          the trajectory is read once). The same pass leaves the sum of the squares per (frame tile, row).
//   vs_row_sum_kernel, vs_a0_kernel   add those in a fixed order: a0[g][a] = sum_e sum_t s^2, without a transform.
//   transforms             the shared ones of fft_pow2.hip per batch of rows: first pass + the pass fused with the column
//                          sums where the length has a two-pass plan, else the packed transform + column sums.
//   vs_fold_kernel         adds the partial spectra of a batch's splits to the (group, axis) row of [3 G][L/2 + 1].
//   vs_spectrum_finish_kernel   the summed spectra as complex input of the inverse; `power` with its totals.
//   one inverse transform over the 3 G rows, and
//   vs_lag_finish_kernel   sums[k][g][.] = corr[.][k] / L, column 3 = (x + y) + z.
// No floating-point atomics anywhere; every order is fixed by the shape, the batch bound and the split counts.
#include <algorithm>
#include <vector>

#include "ctx.h"
#include "spectrum_plan.h"

namespace {

constexpr int VS_SPLITS_PASS = 128;  // row splits of the fused pass (its tiles are few: as msd_fft.hip's batched path)
constexpr int VS_SPLITS_ROWS = 32;   // row splits of the column sums over the packed transform
constexpr long long VS_MAX_GRID_Y = 65535;

// One axis of one cut (spectrum_plan.h): ser[ent_row[e] + shift.add[g]][t] = coef[e] * v[t][axis][e] for the grouped entities
// e of [e_lo, e_hi), g their group, and rowsq[frame tile][axis * N + ent_row[e]] = the sum of the squares of the tile's 64
// values of that series: lane (tx, ty) adds the frames ty, ty + 4, ... of entity tx in order, then (p0 + p1) + (p2 + p3).
// An entity of no group is not loaded. grid (frame tiles, tiles of 64 entities from e_lo + 64 ytile0); 256 lanes = 64 x 4.
__global__ __launch_bounds__(256) void vs_gather_kernel(const double *__restrict__ v, const double *__restrict__ coef,
                                                        const long long *__restrict__ ent_row, const int *__restrict__ ent_group,
                                                        long long F, long long E, long long N, long long e_lo, long long e_hi,
                                                        long long ytile0, int axis, SpShift shift, double *__restrict__ ser,
                                                        double *__restrict__ rowsq)
{
    __shared__ double tile[64][65];
    __shared__ double red[4][64];
    __shared__ long long srow[64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long t0 = (long long)blockIdx.x * 64, e = e_lo + (ytile0 + (long long)blockIdx.y) * 64 + tx;
    long long row = -1, buf_row = -1;  // of the 3 N rows, and of the batch buffer
    if (e < e_hi) {
        const long long j = ent_row[e];
        if (j >= 0) {
            row = (long long)axis * N + j;
            buf_row = j + shift.add[ent_group[e]];
        }
    }
    if (__syncthreads_or(row >= 0) == 0) return;  // (no grouped entity in this tile)
    if (ty == 0) srow[tx] = buf_row;
    const double c = row >= 0 && coef ? coef[e] : 1.0;
    const double *__restrict__ plane = v + (size_t)axis * (size_t)E + (size_t)(row >= 0 ? e : 0);
    double sq = 0.0;
#pragma unroll 4
    for (int k = ty; k < 64; k += 4) {
        const long long tt = t0 + k;
        double s = 0.0;
        if (row >= 0 && tt < F) s = __builtin_nontemporal_load(plane + (size_t)tt * 3 * (size_t)E) * c;
        tile[k][tx] = s;
        sq += s * s;
    }
    red[ty][tx] = sq;
    __syncthreads();
    if (ty == 0 && row >= 0) rowsq[(size_t)blockIdx.x * (size_t)(3 * N) + (size_t)row] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
#pragma unroll 4
    for (int k = ty; k < 64; k += 4) {
        const long long rk = srow[k], tt = t0 + tx;
        if (rk >= 0 && tt < F) __builtin_nontemporal_store(tile[tx][k], ser + (size_t)rk * (size_t)F + (size_t)tt);
    }
}

// rowsum[row] = the frame tiles' sums of the row, in tile order
__global__ void vs_row_sum_kernel(const double *__restrict__ rowsq, long long n_ftiles, long long R, double *__restrict__ rowsum)
{
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= R) return;
    double s = 0.0;
    for (long long f = 0; f < n_ftiles; ++f) s += rowsq[(size_t)f * (size_t)R + (size_t)row];
    rowsum[row] = s;
}

// a0[g][a] = the sum of the row sums of (axis a, group g): 256 partial sums, partial i adding the rows i, i + 256, ... of the
// range in order, and a fixed tree over them; a0[g][3] = (x + y) + z. One workgroup per group.
__global__ __launch_bounds__(256) void vs_a0_kernel(const double *__restrict__ rowsum, SpGroups groups, long long N,
                                                    double *__restrict__ a0)
{
    __shared__ double red[256];
    __shared__ double fin[3];
    const int g = blockIdx.x, tid = threadIdx.x;
    for (int a = 0; a < 3; ++a) {
        const long long lo = (long long)a * N + groups.row0[g], hi = (long long)a * N + groups.row0[g + 1];
        double s = 0.0;
        for (long long r = lo + tid; r < hi; r += 256) s += rowsum[r];
        red[tid] = s;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) fin[a] = red[0];
        __syncthreads();
    }
    if (tid == 0) {
        double *o = a0 + (size_t)g * 4;
        o[0] = fin[0], o[1] = fin[1], o[2] = fin[2];
        o[3] = (fin[0] + fin[1]) + fin[2];
    }
}

// P[k] += the splits' partial sums at k, in split order (P: the spectrum row of one (group, axis))
__global__ void vs_fold_kernel(const double *__restrict__ partial, int splits, long long K, double *__restrict__ P)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int q = 0; q < splits; ++q) s += partial[(size_t)q * (size_t)K + (size_t)k];
    P[k] += s;
}

// Z[g * 3 + a][k] = (P[g * 3 + a][k], 0): the inverse transform's input; power[g][a][k] = P, power[g][3][k] = (x + y) + z
// (power may be nullptr). grid (ceil(K / 256), G).
__global__ void vs_spectrum_finish_kernel(const double *__restrict__ P, long long K, double2 *__restrict__ Z,
                                          double *__restrict__ power)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const size_t g = blockIdx.y;
    const double x = P[(g * 3 + 0) * (size_t)K + k], y = P[(g * 3 + 1) * (size_t)K + k], z = P[(g * 3 + 2) * (size_t)K + k];
    Z[(g * 3 + 0) * (size_t)K + k] = make_double2(x, 0.0);
    Z[(g * 3 + 1) * (size_t)K + k] = make_double2(y, 0.0);
    Z[(g * 3 + 2) * (size_t)K + k] = make_double2(z, 0.0);
    if (power) {
        double *o = power + g * 4 * (size_t)K + k;
        o[0] = x, o[(size_t)K] = y, o[2 * (size_t)K] = z;
        o[3 * (size_t)K] = (x + y) + z;
    }
}

// sums[k][g][a] = corr[g * 3 + a][k] * inv_L, sums[k][g][3] = (x + y) + z of those. One lane per (k, g).
__global__ void vs_lag_finish_kernel(const double *__restrict__ corr, long long L, double inv_L, int G, long long n_lags,
                                     double *__restrict__ sums)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_lags * G) return;
    const long long k = idx / G;
    const size_t g = (size_t)(idx - k * G);
    const double x = corr[(g * 3 + 0) * (size_t)L + k] * inv_L, y = corr[(g * 3 + 1) * (size_t)L + k] * inv_L,
                 z = corr[(g * 3 + 2) * (size_t)L + k] * inv_L;
    double *o = sums + (size_t)idx * 4;
    o[0] = x, o[1] = y, o[2] = z;
    o[3] = (x + y) + z;
}

inline size_t vs_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int mdhip_velocity_spectrum(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *v, int v_on_device,
                            const double *coef, int n_groups, const int32_t *ent_group, int64_t L, int64_t max_lag,
                            double *sums, double *power, int out_on_device, double *a0)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(ent_group && sums && a0 && (n_ent <= 0 || v), "NULL array");
    MD_HIP(hipSetDevice(ctx->device));
    // the rules of the groups, the lengths and the group table are the plan's (spectrum_plan.h): one place
    const bool two_pass = mdhip_fft_power2_plan(ctx, L);
    const SpPlan pl = spectrum_plan(n_frames, n_ent, n_groups, ent_group, L, max_lag, two_pass ? 1 : 2,
                                    (long long)ctx->opt_lag_batch_mb << 20);
    MD_REQUIRE(pl.error != SP_PLAN_GROUPS, "n_groups must be in [1, %d]", SP_MAX_GROUPS);
    MD_REQUIRE(pl.error != SP_PLAN_LENGTH,
               "n_frames >= 1, n_ent >= 0, 0 <= max_lag <= n_frames - 1 and L a power of two in [4, 2^30) that is at least "
               "n_frames + max_lag are required");
    MD_REQUIRE(pl.error != SP_PLAN_ENTITY, "ent_group[%lld] is outside [-1, n_groups)", pl.bad_entity);
    MD_REQUIRE(n_ent == 0 || n_frames < (1ll << 40) / n_ent, "trajectory too large (n_frames * n_ent reaches 2^40)");
    const long long F = n_frames, E = n_ent, G = n_groups, N = pl.n_rows, R = pl.rows_total(), K = L / 2 + 1;
    const long long n_lags = max_lag + 1;
    const size_t sums_b = (size_t)n_lags * G * 4 * 8, power_b = power ? (size_t)G * 4 * K * 8 : 0, a0_b = (size_t)G * 4 * 8;
    int rc;
    if (R == 0) {  // no grouped entity: zeros
        if ((rc = mdhip_zero_result(ctx, sums, sums_b, out_on_device))) return rc;
        if ((rc = mdhip_zero_result(ctx, power, power_b, out_on_device))) return rc;
        memset(a0, 0, a0_b);
        ctx->last_kernel = "";
        ctx->last_launches = 0;
        return cs.end();
    }
    const double *d_v = (const double *)mdhip_stage(ctx, WS_XYZ_I, v, (size_t)F * 3 * (size_t)E * 8, v_on_device, &rc);
    if (rc) return rc;
    // tables: row of every entity | group of every entity | coef
    const size_t row_b = vs_align((size_t)E * 8), grp_b = vs_align((size_t)E * 4);
    MD_WS(d_tab, char, WS_TABLES, row_b + grp_b + (coef ? (size_t)E * 8 : 0));
    // (small tables through pinned staging; large ones straight from where they are: the call completes before it returns)
    auto table = [&](void *dst, const void *src, size_t bytes) -> int {
        if (bytes <= MD_STAGE_MAX) return mdhip_h2d_small(ctx, dst, src, bytes);
        MD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return MDHIP_OK;
    };
    if ((rc = table(d_tab, pl.ent_row.data(), (size_t)E * 8))) return rc;
    if ((rc = table(d_tab + row_b, ent_group, (size_t)E * 4))) return rc;
    const double *d_coef = nullptr;
    if (coef) {
        if ((rc = table(d_tab + row_b + grp_b, coef, (size_t)E * 8))) return rc;
        d_coef = (const double *)(d_tab + row_b + grp_b);
    }
    const long long *d_row = (const long long *)d_tab;
    const int *d_grp = (const int *)(d_tab + row_b);
    const long long nb0 = pl.max_rows;
    const long long n_ftiles = (F + 63) / 64;
    MD_WS(d_ser, double, WS_AUX1, (size_t)nb0 * F * 8);
    MD_WS(d_buf, double2, WS_AUX2, (size_t)nb0 * L * 8);                                              // nb0 * H complex points
    MD_WS(d_tmp, double2, WS_FFT_TMP, (size_t)std::max(two_pass ? 0 : nb0, 3 * G) * L * 8 + 64);        // packed: the second buffer
    MD_WS(d_rowsq, double, WS_AUX0, (size_t)(n_ftiles + 1) * R * 8);                                  // [frame tile][row] | row sums
    double *d_rowsum = d_rowsq + (size_t)n_ftiles * R;
    // WS_AUX3: P [3 G][K] | complex P [3 G][K] | correlations [3 G][L]
    const size_t p_b = vs_align((size_t)3 * G * K * 8), z_b = vs_align((size_t)3 * G * K * 16);
    MD_WS(d_small, char, WS_AUX3, p_b + z_b + (size_t)3 * G * L * 8);
    double *d_P = (double *)d_small;
    double2 *d_Z = (double2 *)(d_small + p_b);
    double *d_corr = (double *)(d_small + p_b + z_b);
    const int max_splits = two_pass ? VS_SPLITS_PASS : VS_SPLITS_ROWS;
    MD_WS(d_part, double, WS_PART, (size_t)max_splits * K * 8);
    // results: sums | power | a0 (the first two in the caller's device buffers when it gave some)
    const size_t s_off = vs_align(a0_b), p_off = s_off + vs_align(sums_b);
    MD_WS(d_out, char, WS_OUT, p_off + power_b);
    double *d_a0 = (double *)d_out;
    double *d_sums = out_on_device ? sums : (double *)(d_out + s_off);
    double *d_power = !power ? nullptr : out_on_device ? power : (double *)(d_out + p_off);

    MD_HIP(hipMemsetAsync(d_P, 0, (size_t)3 * G * K * 8, ctx->stream));
    KernelTimer timer(ctx, 0);
    for (int axis = 0; axis < 3; ++axis)
        for (const SpCut &cut : pl.cuts) {
            const long long n_etiles = (cut.e_hi - cut.e_lo + 63) / 64;
            for (long long y0 = 0; y0 < n_etiles; y0 += VS_MAX_GRID_Y) {
                const dim3 grid((unsigned)n_ftiles, (unsigned)std::min(VS_MAX_GRID_Y, n_etiles - y0));
                hipLaunchKernelGGL(vs_gather_kernel, grid, dim3(256), 0, ctx->stream, d_v, d_coef, d_row, d_grp, F, E, N, cut.e_lo,
                                   cut.e_hi, y0, axis, cut.shift, d_ser, d_rowsq);
            }
            MD_HIP(hipGetLastError());
            const double2 *d_Zp = nullptr;
            rc = two_pass ? mdhip_fft_first_perm(ctx, d_ser, F, d_buf, L, (int)cut.rows)
                          : mdhip_fft_r2c_packed(ctx, d_ser, F, d_buf, d_tmp, L, (int)cut.rows, &d_Zp);
            if (rc) return rc;
            for (int g = 0; g < G; ++g) {
                const long long lo = cut.seg[g], hi = cut.seg[g + 1];
                if (lo >= hi) continue;
                const int splits = (int)std::min<long long>(max_splits, hi - lo);
                rc = two_pass ? mdhip_fft_power_pass(ctx, d_buf, L, lo, hi, splits, d_part)
                              : mdhip_fft_power_rows(ctx, d_Zp, L, lo, hi, splits, d_part);
                if (rc) return rc;
                hipLaunchKernelGGL(vs_fold_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, ctx->stream, d_part, splits, K,
                                   d_P + (size_t)(g * 3 + axis) * K);
            }
            MD_HIP(hipGetLastError());
        }
    hipLaunchKernelGGL(vs_row_sum_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, ctx->stream, d_rowsq, n_ftiles, R,
                       d_rowsum);
    hipLaunchKernelGGL(vs_a0_kernel, dim3((unsigned)G), dim3(256), 0, ctx->stream, d_rowsum, pl.groups, N, d_a0);
    hipLaunchKernelGGL(vs_spectrum_finish_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)G), dim3(256), 0, ctx->stream, d_P, K,
                       d_Z, d_power);
    MD_HIP(hipGetLastError());
    if ((rc = mdhip_fft_c2r(ctx, d_Z, d_tmp, d_corr, L, (int)(3 * G)))) return rc;
    hipLaunchKernelGGL(vs_lag_finish_kernel, dim3((unsigned)((n_lags * G + 255) / 256)), dim3(256), 0, ctx->stream, d_corr, L,
                       1.0 / (double)L, (int)G, n_lags, d_sums);
    MD_HIP(hipGetLastError());
    timer.stop();
    ctx->last_kernel = two_pass ? "vs_gather_kernel+fft_power_pass_kernel" : "vs_gather_kernel+r2c_power_rows_kernel";
    ctx->last_launches = (int)std::min<long long>(pl.n_batches(), 1ll << 30);  // the batches: each one gather, one forward transform, its column sums
    if (!out_on_device) {
        if ((rc = mdhip_result(cs, sums, d_sums, sums_b, 0))) return rc;
        if (power && (rc = mdhip_result(cs, power, d_power, power_b, 0))) return rc;
    }
    if ((rc = mdhip_result(cs, a0, d_a0, a0_b, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
