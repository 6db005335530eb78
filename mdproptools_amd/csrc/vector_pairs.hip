// vector_pairs.hip — distance-resolved orientational pair sums (structural/orientational_correlation.py): per frame, for
// every i in group a and j in group b (j != i), the bin of the site-site distance and, per bin, the number of pairs and
// the exact sums of c = v_i . v_j, c * c and e = v_j . (r_j - r_i) / |r_j - r_i|. include/mdhip.h states every operation.
//
// The sweep over the two groups — job plan (lag 0, stride 1: an origin is a frame), units, bin lookup, the beyond and
// unsummed counts, launch — is group_pairs.h, shared with vanhove.hip; this file owns what a unit does. The lane
// entity's site and vector stay in six registers; the uniform entities come VP_U (six doubles each) at a time. The kernel
// forms d = site(uniform) - site(lane); when the lanes hold group b (lanes_b) that is i - j, the exact negative of the
// j - i the header defines — subtraction, rint (half to even) and the wrap are odd functions, bit for bit — so rsq is
// the same number and only e changes sign, exactly: it is negated once, behind the division. c is a sum of commutative
// products: it does not know which end is which. The vector that e uses is j's: the uniform one, or the lane's own.
// The cutoff compare comes first; the payload, the f64 sqrt and the division run only for pairs inside.
// A workgroup holds the job's row in LDS: three int64 sums and a uint32 count per bin (28 bytes: 112 KiB at the 4096
// bins allowed), added with LDS integer atomics, flushed into the 128-bit device words with 64-bit integer atomics —
// add the low word, carry into the high word when that add wrapped, add the sign extension. Counting carries is exact
// in any order: the low words wrap as often as their exact sum passes 2^64. Integers only: no float atomics, the
// results do not depend on the launch geometry. Measured: DESIGN.md 4.13d.

#include "fixed_point.h"
#include "group_pairs.h"

#pragma clang fp contract(off)

namespace {

constexpr int VP_THREADS = 256;
constexpr int VP_WAVES = VP_THREADS / 64;
constexpr int VP_U = 4;                       // uniform entities per batch of scalar loads (six doubles each)
constexpr int VP_MAX_BINS = 4096;             // 28 bytes per bin: 112 KiB of the 160 KiB of LDS
constexpr long long VP_JCHUNK = 1ll << 20;    // uniform entities per unit: 64 * 2^20 = 2^26 pairs at most
constexpr long long VP_BLOCKS = 4096;         // about this many workgroups per job at most
// Pairs a workgroup bins between zeroing and flushing its row. An addend is rint(v * 2^32) with |v| < 2, so |addend| <
// 2^33 and an int64 word of the row holds |sum| <= 2^29 * 2^33 = 2^62 < 2^63; the uint32 count holds 2^29 as well.
constexpr long long VP_MAX_PAIRS = 1ll << 29;  // (the addend itself: vp_fixed, fixed_point.h)

// Dynamic LDS: int64 [3][nbins] | uint32 [nbins].
__global__ __launch_bounds__(VP_THREADS) void vp_pair_kernel(
    const double *__restrict__ site, const double *__restrict__ vec, const double *__restrict__ box, long long E,
    const GpJob *__restrict__ jobs, int job0, const double *__restrict__ edges, float gscale, float near, int nbins,
    unsigned long long *__restrict__ hist, unsigned long long *__restrict__ sums, unsigned long long *__restrict__ beyond,
    unsigned long long *__restrict__ unsummed)
{
    extern __shared__ unsigned long long s_sum[];  // [3][nbins], two's complement
    unsigned *const s_cnt = reinterpret_cast<unsigned *>(s_sum + 3 * (size_t)nbins);
    __shared__ unsigned s_tot[2];  // beyond, unsummed
    const int job = job0 + (int)blockIdx.y;
    GpJob J;
    if (!gp_job(jobs, job, J)) return;
    for (int w = threadIdx.x; w < nbins; w += VP_THREADS) {
        s_sum[w] = s_sum[nbins + w] = s_sum[2 * nbins + w] = 0ull;
        s_cnt[w] = 0u;
    }
    if (threadIdx.x == 0) s_tot[0] = s_tot[1] = 0u;
    __syncthreads();
    const double top = edges[nbins];
    const float near2 = near + near;
    const bool lane_is_j = J.lanes_b != 0;
    unsigned n_in = 0, n_uns = 0;  // the pairs this lane binned, and those of them it could not sum

    const unsigned n_pairs = gp_walk<VP_WAVES, VP_JCHUNK>(J, [&](long long f, long long il, long long j0, int jlen, int self) {
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const double ix = 1.0 / Lx, iy = 1.0 / Ly, iz = 1.0 / Lz;
        const size_t al = (size_t)f * 3 * (size_t)E + (size_t)(J.l0 + il);
        const double sx = site[al], sy = site[al + E], sz = site[al + 2 * E];
        const double wx = vec[al], wy = vec[al + E], wz = vec[al + 2 * E];
        const size_t au = (size_t)f * 3 * (size_t)E + (size_t)(J.u0 + j0);
        const double *__restrict__ px = site + au, *__restrict__ py = px + E, *__restrict__ pz = py + E;
        const double *__restrict__ qx = vec + au, *__restrict__ qy = qx + E, *__restrict__ qz = qy + E;

        // one pair: the uniform entity's site (xu ..) and vector (ux ..) against the lane's
        auto pair = [&](double xu, double yu, double zu, double ux, double uy, double uz, bool valid) {
            double dx = xu - sx, dy = yu - sy, dz = zu - sz;
            dx = dx - Lx * __builtin_rint(dx * ix);
            dy = dy - Ly * __builtin_rint(dy * iy);
            dz = dz - Lz * __builtin_rint(dz * iz);
            const double rsq = (dx * dx + dy * dy) + dz * dz;
            if (rsq < top && valid) {
                const int k = gp_bin(rsq, edges, gscale, near, near2, nbins);
                ++n_in;
                atomicAdd(&s_cnt[k], 1u);
                const double c = (wx * ux + wy * uy) + wz * uz;
                const double c2 = c * c;
                // v_j against i -> j: d here is uniform - lane, which is j - i unless the lanes hold j
                const double dot = lane_is_j ? (dx * wx + dy * wy) + dz * wz : (dx * ux + dy * uy) + dz * uz;
                const double q = dot / __builtin_sqrt(rsq);
                const double e = lane_is_j ? -q : q;
                if (__builtin_fabs(c) < 2.0 && __builtin_fabs(c2) < 2.0 && __builtin_fabs(e) < 2.0) {  // (false for a NaN)
                    atomicAdd(&s_sum[k], vp_fixed(c));
                    atomicAdd(&s_sum[nbins + k], vp_fixed(c2));
                    atomicAdd(&s_sum[2 * nbins + k], vp_fixed(e));
                } else {
                    ++n_uns;
                }
            }
        };

        int jj = 0;
        for (; jj + VP_U <= jlen; jj += VP_U) {
            double xu[VP_U], yu[VP_U], zu[VP_U], ux[VP_U], uy[VP_U], uz[VP_U];
#pragma unroll
            for (int q = 0; q < VP_U; ++q) {
                xu[q] = px[jj + q], yu[q] = py[jj + q], zu[q] = pz[jj + q];
                ux[q] = qx[jj + q], uy[q] = qy[jj + q], uz[q] = qz[jj + q];
            }
#pragma unroll
            for (int q = 0; q < VP_U; ++q) pair(xu[q], yu[q], zu[q], ux[q], uy[q], uz[q], jj + q != self);
        }
        for (; jj < jlen; ++jj) pair(px[jj], py[jj], pz[jj], qx[jj], qy[jj], qz[jj], jj != self);
    });
    unsigned n_tot[2] = {n_pairs - n_in, n_uns};
    unsigned long long *const g_tot[2] = {beyond + job, unsummed + job};
    gp_tail(n_tot, s_tot, g_tot);
    unsigned long long *g_row = hist + (size_t)job * (size_t)nbins;
    unsigned long long *g_sum = sums + (size_t)job * 3 * (size_t)nbins * 2;
    for (int k = threadIdx.x; k < nbins; k += VP_THREADS) {
        const unsigned v = s_cnt[k];
        if (!v) continue;  // (no pair, no addend)
        atomicAdd(&g_row[k], (unsigned long long)v);
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const unsigned long long add = s_sum[s * nbins + k];
            if (!add) continue;
            unsigned long long *word = g_sum + ((size_t)s * (size_t)nbins + (size_t)k) * 2;
            const unsigned long long old = atomicAdd(&word[0], add);
            // the high word: +1 when the low word wrapped, and the sign extension of the addend (all ones when negative)
            const unsigned long long high = (old + add < old ? 1ull : 0ull) + ((long long)add < 0 ? ~0ull : 0ull);
            if (high) atomicAdd(&word[1], high);
        }
    }
}

}  // namespace

extern "C" {

int mdhip_vector_pair_hist(mdhip_ctx *ctx, int64_t n_frames, int64_t n_ent, const double *site, const double *vec,
                           int in_on_device, const double *box, int n_groups, const int64_t *group_off, int n_jobs,
                           const int32_t *jobs, double bin_size, int32_t nbins, const double *edges, uint64_t *hist,
                           uint64_t *sums, uint64_t *beyond, uint64_t *unsummed, uint64_t *pairs)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    int rc;
    MD_REQUIRE(n_frames >= 0 && n_ent >= 0 && n_groups >= 0 && n_jobs >= 0, "negative sizes");
    MD_REQUIRE(n_ent < (1ll << 40) && n_frames < (1ll << 40) && (n_ent == 0 || n_frames < (1ll << 40) / n_ent),
               "trajectory too large");
    MD_REQUIRE(box, "NULL box: the pair sums take the nearest image, which needs the box");
    MD_REQUIRE(nbins >= 1 && nbins <= VP_MAX_BINS, "nbins must be in [1, %d]", VP_MAX_BINS);
    MD_REQUIRE(bin_size > 0.0 && bin_size < __builtin_inf(), "bin_size must be positive and finite");
    if ((rc = gp_check_groups(ctx, n_groups, group_off, n_ent))) return rc;
    MD_REQUIRE(n_jobs == 0 || (jobs && hist && sums && beyond && unsummed && pairs), "NULL array");
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 2 * (size_t)j;
        MD_REQUIRE(q[0] >= 0 && q[0] < n_groups && q[1] >= 0 && q[1] < n_groups, "job %d: group (%d, %d) out of range",
                   j, q[0], q[1]);
    }
    MD_REQUIRE((size_t)n_jobs * (size_t)nbins < ((size_t)1 << 30), "result too large");
    if ((rc = gp_check_edges(ctx, edges, nbins, n_jobs))) return rc;
    if (n_jobs == 0) return cs.end();
    MD_REQUIRE(n_ent == 0 || n_frames == 0 || (site && vec), "NULL sites or vectors");

    const GpRule rule = {VP_WAVES, VP_JCHUNK, VP_BLOCKS, VP_MAX_PAIRS, 32ll * nbins};
    std::vector<GpJob> tab((size_t)n_jobs);
    std::vector<uint64_t> n_pairs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 2 * (size_t)j;
        const long long a0 = group_off[q[0]], b0 = group_off[q[1]];
        n_pairs[(size_t)j] = gp_plan(tab[(size_t)j], n_frames, a0, group_off[q[0] + 1] - a0, b0, group_off[q[1] + 1] - b0,
                                     q[0] == q[1], rule);
    }
    for (int j = 0; j < n_jobs; ++j) MD_REQUIRE(tab[(size_t)j].nblk < (1ll << 31), "job %d: too many workgroups", j);
    std::vector<double> own;
    if ((rc = gp_edges(ctx, edges, own, bin_size, nbins))) return rc;
    std::copy(n_pairs.begin(), n_pairs.end(), pairs);
    const GpBand band = gp_band(nbins, bin_size);

    MD_HIP(hipSetDevice(ctx->device));
    const size_t in_bytes = (size_t)n_frames * 3 * (size_t)n_ent * 8;
    const double *d_site = (const double *)mdhip_stage(ctx, WS_XYZ_I, site, in_bytes, in_on_device || in_bytes == 0, &rc);
    if (rc) return rc;
    const double *d_vec = (const double *)mdhip_stage(ctx, WS_XYZ_J, vec, in_bytes, in_on_device || in_bytes == 0, &rc);
    if (rc) return rc;
    MD_WS(d_cnt, unsigned long long, WS_MISC, (size_t)n_jobs * 16);  // beyond | unsummed
    GpTables d;
    if ((rc = gp_stage(ctx, box, n_frames, tab, edges, nbins, d))) return rc;
    const size_t hist_bytes = (size_t)n_jobs * (size_t)nbins * 8, sums_bytes = hist_bytes * 6;
    MD_WS(d_hist, unsigned long long, WS_HIST, hist_bytes + sums_bytes);  // hist | sums
    unsigned long long *d_sums = d_hist + hist_bytes / 8;
    const size_t lds_b = (size_t)nbins * 28;
    if (lds_b > 65536 - 64)
        MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vp_pair_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    KernelTimer timer(ctx, 0);
    MD_HIP(hipMemsetAsync(d_cnt, 0, (size_t)n_jobs * 16, ctx->stream));
    MD_HIP(hipMemsetAsync(d_hist, 0, hist_bytes + sums_bytes, ctx->stream));
    if ((rc = gp_launch(ctx, "vp_pair_kernel", timer, tab, [&](dim3 grid, int j0) {
        hipLaunchKernelGGL(vp_pair_kernel, grid, dim3(VP_THREADS), lds_b, ctx->stream, d_site, d_vec, d.box,
                           (long long)n_ent, d.jobs, j0, d.edges, band.gscale, band.near, (int)nbins, d_hist, d_sums, d_cnt,
                           d_cnt + n_jobs);
    }))) return rc;
    if ((rc = mdhip_result(cs, hist, d_hist, hist_bytes, 0))) return rc;
    if ((rc = mdhip_result(cs, sums, d_sums, sums_bytes, 0))) return rc;
    if ((rc = mdhip_result(cs, beyond, d_cnt, (size_t)n_jobs * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, unsummed, d_cnt + n_jobs, (size_t)n_jobs * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
