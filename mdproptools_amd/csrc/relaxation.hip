// relaxation.hip — self-intermediate scattering function and overlap counts at EVERY lag, per time origin: the hot loop
// of StructuralRelaxation.calc_relaxation (F_s(q, t), Q(t), chi4(t)). include/mdhip.h states every operation under
// mdhip_self_relaxation. For coordinates r [F][3][E], groups g, lags k = 0 .. max_lag and origins t0 = 0, s, 2s, ...:
//   per entity e of g: d = xu(t0 + k) - xu(t0), rsq = (dx dx + dy dy) + dz dz unfused;
//   a non-finite rsq counts in nonfinite[k][g] and nowhere else; else
//   n(t0, k) += rsq < a_sq[g], and per wave number q_j: fs[k][g][j] += (int64) rint(sinc(q_j * sqrt(rsq)) * 2^32);
//   count1[k][g] = sum over t0 of n, count2[k][g] = sum over t0 of n * n.
// n(t0, k) has to be COMPLETE before it is squared, so the organisation of lag_tiles.h (a lane owns lags and sums over
// origins as it goes) does not fit. Here a workgroup owns a tile of 32 origins x 64 lags of one group
// (relaxation_plan.h): a lane keeps one origin and 8 consecutive lags, i.e. 8 cells, each a uint32 count and n_q int64
// sums in registers, and the workgroup walks the group's entities in stages of 16. A stage puts the 32 origin frames
// and the 95 partner frames the tile needs, unwrapped, into LDS (48 KiB) straight from the frame-major rows — 16
// entities are 128 contiguous bytes of a row — transposed to [axis][entity][frame], so that the lanes of a wave, which
// differ in the origin, read consecutive doubles. When the last entity is through, a cell's n is final: n, n * n and
// the sinc sums are added over the 32 origins of half a wave by shuffles and go to the per-lag outputs with 64-bit
// integer atomics. Nothing of size F x max_lag ever goes to device memory. origin_stride > 1 spreads the partner
// frames of a tile over (32 - 1) * s + 64 frames: those calls read both ends through L2 instead (WINDOW = false), same
// cells, same integers. Integers only: no float atomics, no float accumulators; the results do not depend on the launch
// geometry nor on the order of the entities. Measured: DESIGN.md 4.13h.

#include "fixed_point.h"
#include "group_pairs.h"  // (gp_check_groups)
#include "image_counts.h"
#include "relaxation_plan.h"

#pragma clang fp contract(off)

namespace {

struct RxArgs {
    const double *r;    // [F][3][E]
    const int *img;     // [F][3E] image counts, or nullptr: r is unwrapped
    const double *box;  // [F][3] (device) when img
    long long F, E, stride, max_lag;
    long long ot0, kt0;  // first origin tile and lag tile of the launch
    int G, n_q;
    unsigned long long *count1, *count2, *fs, *nonfinite;  // [max_lag+1][G], fs [max_lag+1][G][n_q]
    long long group_off[rx::MAX_GROUPS + 1];
    double a_sq[rx::MAX_GROUPS];               // -1 without the overlap part: nothing passes
    double q[rx::MAX_GROUPS][rx::MAX_Q];
};

// xu of (frame f, axis a, entity e)
__device__ __forceinline__ double rx_xu(const RxArgs &A, long long f, int a, long long e)
{
    const size_t at = (size_t)f * 3 * (size_t)A.E + (size_t)a * (size_t)A.E + (size_t)e;
    const double x = A.r[at];
    if (!A.img) return x;
    const double nl = (double)A.img[at] * A.box[3 * f + a];
    return x + nl;
}

// Block (x, y, z): origin tile ot0 + x, lag tile kt0 + y, group z.
template <int NQ, bool WINDOW>
__global__ __launch_bounds__(rx::THREADS) void rx_tile_kernel(const RxArgs A)
{
    using namespace rx;
    __shared__ double s_win[WINDOW ? LDS_DOUBLES : 1];
    double *const s_org = s_win;                      // [3][EB][ORG_W]
    double *const s_par = s_win + 3 * EB * ORG_W;     // [3][EB][WIN]
    const int g = blockIdx.z;
    const long long e0 = A.group_off[g], ng = A.group_off[g + 1] - e0;
    const long long ot = A.ot0 + blockIdx.x, kt = A.kt0 + blockIdx.y;
    if (ng == 0 || tile_empty(A.F, A.max_lag, A.stride, ot, kt)) return;  // (the whole workgroup)
    const int lane = threadIdx.x, o = lane_origin(lane), kl = lane_lag(lane, 0);
    const long long t0 = (ot * TO + o) * A.stride, k0 = kt * TK + kl;
    const int nv = n_cells(A.F, A.max_lag, t0, k0);
    const long long f_org = ot * TO * A.stride, f_par = f_org + kt * TK;  // first frames of the two LDS windows
    const double a_sq = A.a_sq[g];
    double qv[NQ ? NQ : 1];
#pragma unroll
    for (int j = 0; j < NQ; ++j) qv[j] = A.q[g][j];
    unsigned cnt[CELLS];
    unsigned long long sum[CELLS][NQ ? NQ : 1];
#pragma unroll
    for (int c = 0; c < CELLS; ++c) {
        cnt[c] = 0u;
#pragma unroll
        for (int j = 0; j < (NQ ? NQ : 1); ++j) sum[c][j] = 0ull;
    }

    // one cell and one entity: the origin's position against the partner's
    auto cell = [&](int c, double ox, double oy, double oz, double px, double py, double pz) {
        const double dx = px - ox, dy = py - oy, dz = pz - oz;
        const double rsq = (dx * dx + dy * dy) + dz * dz;
        if (rsq < __builtin_inf()) {  // (false for a NaN)
            cnt[c] += rsq < a_sq ? 1u : 0u;
            if (NQ) {
                const double d = __builtin_sqrt(rsq);
#pragma unroll
                for (int j = 0; j < NQ; ++j) sum[c][j] += vp_fixed(sinc(qv[j] * d));
            }
        } else {
            atomicAdd(&A.nonfinite[(size_t)(k0 + c) * A.G + g], 1ull);
        }
    };

    for (long long eb = 0; eb < ng; eb += EB) {
        const int ne = (int)(ng - eb < EB ? ng - eb : EB);
        if (WINDOW) {
            __syncthreads();  // (the stage before has been read)
            // the origin frames f_org + w, w < TO, and the partner frames f_par + w, w < WIN: e fastest, so that 16 lanes
            // read 128 contiguous bytes; frames beyond the trajectory hold zeros that no cell reads
            for (int i = lane; i < 3 * (TO + WIN) * EB; i += THREADS) {
                const int e = i % EB, row = i / EB;
                const int a = row / (TO + WIN), w = row % (TO + WIN);
                const bool org = w < TO;
                const long long f = org ? f_org + w : f_par + (w - TO);
                const double v = (e < ne && f < A.F) ? rx_xu(A, f, a, e0 + eb + e) : 0.0;
                if (org)
                    s_org[(a * EB + e) * ORG_W + w] = v;
                else
                    s_par[(a * EB + e) * WIN + (w - TO)] = v;
            }
            __syncthreads();
        }
        if (nv == 0) continue;
        for (int e = 0; e < ne; ++e) {
            double ox, oy, oz;
            if (WINDOW) {
                ox = s_org[e * ORG_W + o];
                oy = s_org[(EB + e) * ORG_W + o];
                oz = s_org[(2 * EB + e) * ORG_W + o];
            } else {
                ox = rx_xu(A, t0, 0, e0 + eb + e);
                oy = rx_xu(A, t0, 1, e0 + eb + e);
                oz = rx_xu(A, t0, 2, e0 + eb + e);
            }
#pragma unroll
            for (int c = 0; c < CELLS; ++c) {
                if (c < nv) {
                    if (WINDOW) {
                        const int w = o + kl + c;
                        cell(c, ox, oy, oz, s_par[e * WIN + w], s_par[(EB + e) * WIN + w], s_par[(2 * EB + e) * WIN + w]);
                    } else {
                        const long long f = t0 + k0 + c;
                        cell(c, ox, oy, oz, rx_xu(A, f, 0, e0 + eb + e), rx_xu(A, f, 1, e0 + eb + e),
                             rx_xu(A, f, 2, e0 + eb + e));
                    }
                }
            }
        }
    }

    // every n(t0, k) of the tile is final: the sums over the 32 origins of half a wave, then the per-lag words. Cells
    // that do not exist hold zeros; a lag beyond max_lag has no word.
#pragma unroll
    for (int c = 0; c < CELLS; ++c) {
        unsigned long long n1 = cnt[c], n2 = (unsigned long long)cnt[c] * cnt[c];
#pragma unroll
        for (int sh = TO / 2; sh; sh >>= 1) {
            n1 += __shfl_xor(n1, sh);
            n2 += __shfl_xor(n2, sh);
#pragma unroll
            for (int j = 0; j < NQ; ++j) sum[c][j] += __shfl_xor(sum[c][j], sh);
        }
        if (o == 0 && k0 + c <= A.max_lag) {
            const size_t at = (size_t)(k0 + c) * A.G + g;
            if (n1) {
                atomicAdd(&A.count1[at], n1);
                atomicAdd(&A.count2[at], n2);
            }
#pragma unroll
            for (int j = 0; j < NQ; ++j)
                if (sum[c][j]) atomicAdd(&A.fs[at * NQ + j], sum[c][j]);
        }
    }
}

template <int NQ>
void rx_launch(bool window, dim3 grid, hipStream_t stream, const RxArgs &A)
{
    if (window)
        hipLaunchKernelGGL((rx_tile_kernel<NQ, true>), grid, dim3(rx::THREADS), 0, stream, A);
    else
        hipLaunchKernelGGL((rx_tile_kernel<NQ, false>), grid, dim3(rx::THREADS), 0, stream, A);
}

}  // namespace

extern "C" {

int mdhip_self_relaxation(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *r, int r_on_device,
                          const double *box, int n_groups, const int64_t *group_off, int64_t max_lag,
                          int64_t origin_stride, const double *a_sq, int n_q, const double *q, uint64_t *origins,
                          uint64_t *count1, uint64_t *count2, int64_t *fs, uint64_t *nonfinite)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    int rc;
    MD_REQUIRE(n_groups >= 1 && n_groups <= rx::MAX_GROUPS, "n_groups must be in [1, %d]", rx::MAX_GROUPS);
    MD_REQUIRE(n_q >= 0 && n_q <= rx::MAX_Q, "n_q must be in [0, %d]", rx::MAX_Q);
    MD_REQUIRE(n_frames >= 1 && n_frames <= rx::MAX_FRAMES, "n_frames must be in [1, 2^29 - 1]");
    MD_REQUIRE(n_ent >= 0 && n_ent < (1ll << 40) && (n_ent == 0 || n_frames < (1ll << 40) / n_ent),
               "trajectory too large");
    MD_REQUIRE(max_lag >= 0 && max_lag <= n_frames - 1, "max_lag must be in [0, n_frames - 1]");
    MD_REQUIRE(origin_stride >= 1, "origin_stride must be at least 1");
    // every stride beyond n_frames - 1 means the one origin t0 = 0: from here on the stride is at most n_frames, so that
    // no (origin index) * stride of the plan or the kernel can overflow
    const long long stride = rx::clamp_stride(n_frames, origin_stride);
    MD_REQUIRE(a_sq || n_q > 0, "nothing to compute: a_sq is NULL and n_q is 0");
    if ((rc = gp_check_groups(ctx, n_groups, group_off, n_ent))) return rc;
    MD_REQUIRE(origins && nonfinite && (!a_sq || (count1 && count2)) && (n_q == 0 || (q && fs)), "NULL array");
    for (int g = 0; g < n_groups; ++g) {
        MD_REQUIRE(!a_sq || a_sq[g] >= 0.0, "a_sq[%d] must not be negative or NaN", g);
        for (int j = 0; j < n_q; ++j)
            MD_REQUIRE(q[g * n_q + j] >= 0.0 && q[g * n_q + j] < __builtin_inf(),
                       "q[%d][%d] must be finite and not negative", g, j);
        MD_REQUIRE(rx::guard_ok(n_frames, stride, group_off[g + 1] - group_off[g]),
                   "group %d: origins * group size = %lld * %lld reaches 2^30, beyond which the integer sums could "
                   "overflow: raise origin_stride", g, rx::origins(n_frames, 0, stride),
                   (long long)(group_off[g + 1] - group_off[g]));
    }
    MD_REQUIRE(n_ent == 0 || r, "NULL coordinates");

    const size_t L = (size_t)max_lag + 1, G = (size_t)n_groups;
    for (size_t k = 0; k < L; ++k) origins[k] = (uint64_t)rx::origins(n_frames, (long long)k, stride);
    RxArgs A;
    memset(&A, 0, sizeof A);
    for (int g = 0; g <= n_groups; ++g) A.group_off[g] = group_off[g];
    for (int g = 0; g < n_groups; ++g) {
        A.a_sq[g] = a_sq ? a_sq[g] : -1.0;
        for (int j = 0; j < n_q; ++j) A.q[g][j] = q[g * n_q + j];
    }
    A.F = n_frames, A.E = n_ent, A.stride = stride, A.max_lag = max_lag, A.G = n_groups, A.n_q = n_q;

    MD_HIP(hipSetDevice(ctx->device));
    const size_t r_bytes = (size_t)n_frames * 3 * (size_t)n_ent * 8;
    const double *d_r = (const double *)mdhip_stage(ctx, WS_XYZ_I, r, r_bytes, r_on_device || r_bytes == 0, &rc);
    if (rc) return rc;
    // count1 | count2 | nonfinite | fs, one zeroed run; and a word for the image passes' crossings
    const size_t words = L * G * (3 + (size_t)n_q);
    MD_WS(d_out, unsigned long long, WS_HIST, words * 8);
    MD_WS(d_cross, unsigned long long, WS_MISC, 8);
    A.r = d_r;
    A.count1 = d_out, A.count2 = d_out + L * G, A.nonfinite = d_out + 2 * L * G, A.fs = d_out + 3 * L * G;
    KernelTimer timer(ctx, 0);
    int launches = 0;
    MD_HIP(hipMemsetAsync(d_out, 0, words * 8, ctx->stream));
    if (box != nullptr && n_ent > 0 && n_frames >= 2) {
        MD_HIP(hipMemsetAsync(d_cross, 0, 8, ctx->stream));
        if ((rc = dp_image_counts(ctx, d_r, box, n_frames, n_ent, d_cross, A.box, A.img, launches))) return rc;
    }
    if (n_ent > 0) {
        const bool window = stride == 1;
        for (const rx::Launch &Ln : rx::launches(n_frames, max_lag, stride)) {
            A.ot0 = Ln.ot0, A.kt0 = Ln.kt0;
            const dim3 grid(Ln.gx, Ln.gy, (unsigned)n_groups);
            switch (n_q) {
            case 0: rx_launch<0>(window, grid, ctx->stream, A); break;
            case 1: rx_launch<1>(window, grid, ctx->stream, A); break;
            case 2: rx_launch<2>(window, grid, ctx->stream, A); break;
            case 3: rx_launch<3>(window, grid, ctx->stream, A); break;
            default: rx_launch<4>(window, grid, ctx->stream, A); break;
            }
            MD_HIP(hipGetLastError());
            ++launches;
        }
        ctx->last_kernel = "rx_tile_kernel";
    }
    ctx->last_launches = launches;
    timer.stop();
    if (a_sq) {
        if ((rc = mdhip_result(cs, count1, A.count1, L * G * 8, 0))) return rc;
        if ((rc = mdhip_result(cs, count2, A.count2, L * G * 8, 0))) return rc;
    }
    if ((rc = mdhip_result(cs, nonfinite, A.nonfinite, L * G * 8, 0))) return rc;
    if (n_q && (rc = mdhip_result(cs, fs, A.fs, L * G * (size_t)n_q * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
