// vector_pairs.hip — distance-resolved orientational pair sums (structural/orientational_correlation.py): per frame, for
// every i in group a and j in group b (j != i), the bin of the site-site distance and, per bin, the number of pairs and
// the exact sums of c = v_i . v_j, c * c and e = v_j . (r_j - r_i) / |r_j - r_i|. include/mdhip.h states every operation.
//
// Organised as vh_pair_kernel (vanhove.hip): one launch for all jobs (blockIdx.y = job; more than 65 535 jobs go in
// slices). Of a job's two groups the one that fills its tiles of 64 better lies along the lanes, its site and vector in
// six registers; the other is swept as wave-uniform operands through uniform addresses on const __restrict__ pointers,
// VP_U entities (six doubles each) at a time, which the compiler turns into scalar loads. A wave takes one unit at a
// time: (frame, tile of 64 lane entities, chunk of up to VP_JCHUNK uniform entities). The kernel always forms
// d = site(uniform) - site(lane); when the lanes hold group b (lane_is_j) that is i - j, the exact negative of the
// j - i the header defines — subtraction, rint (half to even) and the wrap are odd functions, bit for bit — so rsq is
// the same number and only e changes sign, exactly: it is negated once, behind the division. c is a sum of commutative
// products: it does not know which end is which. The vector that e uses is j's: the uniform one, or the lane's own.
// The cutoff compare comes first; the bin is the float guess with guard band of the siblings (only a guess within the
// band of an integer walks the edge table); the payload, the f64 sqrt and the division run only for pairs inside.
// A workgroup owns a run of `upb` consecutive units of one job and the job's row in LDS: three int64 sums and a uint32
// count per bin (28 bytes: 112 KiB at the 4096 bins allowed), added with LDS integer atomics, flushed into the 128-bit
// device words with 64-bit integer atomics — add the low word, carry into the high word when that add wrapped, add the
// sign extension. Counting carries is exact in any order: the low words wrap as often as their exact sum passes 2^64.
// beyond and unsummed: a lane counts its pairs (from the unit's sizes), those it binned and those it could not sum;
// a butterfly, one LDS atomic per wave, one 64-bit atomic per workgroup. Integers only: no float atomics, the results do
// not depend on the launch geometry. Measured: DESIGN.md 4.13d.

#include <algorithm>
#include <cmath>
#include <vector>

#include "ctx.h"

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
constexpr long long VP_MAX_PAIRS = 1ll << 29;
constexpr int VP_MAX_Y = 65535;
constexpr double VP_ONE = 4294967296.0;       // 2^32: the fixed-point unit

struct VpJob {
    long long l0, nl;          // the entities along the lanes [l0, l0 + nl) ...
    long long u0, nu;          // ... and the wave-uniform ones [u0, u0 + nu)
    long long n_tiles, n_jc;   // tiles of 64 lane entities, chunks of VP_JCHUNK uniform entities
    long long n_units, upb, nblk;
    int lane_is_j;             // 1: the lanes hold group b (the j of a pair), the uniform set group a
    int pad;
};

// (int64) rint(v * 2^32) of |v| < 2 as a two's-complement word. The product is exact (a power of two) and below 2^33 in
// magnitude; adding 1.5 * 2^52 moves it to where a double's ulp is 1, which rounds it to an integer, half to even, as
// rint does, and leaves that integer in the low bits of the sum: the difference of the two bit patterns is the value.
// One addition and one 64-bit subtraction instead of a rounding and a double-to-int64 conversion sequence.
__device__ __forceinline__ unsigned long long vp_fixed(double v)
{
    constexpr double magic = 6755399441055744.0;  // 1.5 * 2^52
    return (unsigned long long)(__double_as_longlong(v * VP_ONE + magic) - __double_as_longlong(magic));
}

// Block (x, y): units [x * upb, (x + 1) * upb) of job job0 + y. Dynamic LDS: int64 [3][nbins] | uint32 [nbins].
__global__ __launch_bounds__(VP_THREADS) void vp_pair_kernel(const double *__restrict__ site,
                                                             const double *__restrict__ vec,
                                                             const double *__restrict__ box, long long E,
                                                             const VpJob *__restrict__ jobs, int job0,
                                                             const double *__restrict__ edges, float gscale,
                                                             float near, int nbins,
                                                             unsigned long long *__restrict__ hist,
                                                             unsigned long long *__restrict__ sums,
                                                             unsigned long long *__restrict__ beyond,
                                                             unsigned long long *__restrict__ unsummed)
{
    extern __shared__ unsigned long long s_sum[];  // [3][nbins], two's complement
    unsigned *const s_cnt = reinterpret_cast<unsigned *>(s_sum + 3 * (size_t)nbins);
    __shared__ unsigned s_bey, s_uns;
    const int job = job0 + (int)blockIdx.y;
    const VpJob J = jobs[job];
    if ((long long)blockIdx.x >= J.nblk) return;  // (the whole workgroup: jobs of one launch differ in size)
    for (int w = threadIdx.x; w < nbins; w += VP_THREADS) {
        s_sum[w] = s_sum[nbins + w] = s_sum[2 * nbins + w] = 0ull;
        s_cnt[w] = 0u;
    }
    if (threadIdx.x == 0) s_bey = s_uns = 0u;
    __syncthreads();
    const double top = edges[nbins];
    const float near2 = near + near;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool lane_is_j = J.lane_is_j != 0;
    const long long ua = (long long)blockIdx.x * J.upb;
    const long long ub = ua + J.upb < J.n_units ? ua + J.upb : J.n_units;
    unsigned n_pairs = 0, n_in = 0, n_uns = 0;  // this lane's pairs, those it binned, and those of them it could not sum

    for (long long u = ua + wave; u < ub; u += VP_WAVES) {
        const long long ch = u % J.n_jc, ft = u / J.n_jc;
        const long long f = ft / J.n_tiles, tile = ft - f * J.n_tiles;
        const double Lx = box[3 * f], Ly = box[3 * f + 1], Lz = box[3 * f + 2];
        const double ix = 1.0 / Lx, iy = 1.0 / Ly, iz = 1.0 / Lz;
        const long long il = tile * 64 + lane;
        const long long j0 = ch * VP_JCHUNK;
        const int jlen = (int)(J.nu - j0 < VP_JCHUNK ? J.nu - j0 : VP_JCHUNK);
        if (il >= J.nl) continue;
        const size_t al = (size_t)f * 3 * (size_t)E + (size_t)(J.l0 + il);
        const double sx = site[al], sy = site[al + E], sz = site[al + 2 * E];
        const double wx = vec[al], wy = vec[al + E], wz = vec[al + 2 * E];
        // the uniform index that is this lane's own entity (none: outside [0, jlen))
        const long long self_ll = J.l0 + il - J.u0 - j0;
        const int self = self_ll >= 0 && self_ll < jlen ? (int)self_ll : -1;
        n_pairs += (unsigned)jlen - (self >= 0);
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
                const float g = __builtin_fmaf(__builtin_amdgcn_sqrtf((float)rsq), gscale, near);
                int k = (int)g;  // the bin, unless g is within the band above an integer: then the edges decide
                if (__builtin_amdgcn_fractf(g) < near2) {
                    k = k < nbins - 1 ? k : nbins - 1;
                    while (rsq < edges[k]) --k;       // edges[0] == 0 stops it
                    while (rsq >= edges[k + 1]) ++k;  // rsq < edges[nbins] stops it
                }
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
    }
    unsigned n_bey = n_pairs - n_in;
    for (int sh = 32; sh; sh >>= 1) {
        n_bey += __shfl_xor(n_bey, sh);
        n_uns += __shfl_xor(n_uns, sh);
    }
    if (lane == 0 && n_bey) atomicAdd(&s_bey, n_bey);
    if (lane == 0 && n_uns) atomicAdd(&s_uns, n_uns);
    __syncthreads();
    if (threadIdx.x == 0 && s_bey) atomicAdd(&beyond[job], (unsigned long long)s_bey);
    if (threadIdx.x == 0 && s_uns) atomicAdd(&unsummed[job], (unsigned long long)s_uns);
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
    MD_REQUIRE(n_frames >= 0 && n_ent >= 0 && n_groups >= 0 && n_jobs >= 0, "negative sizes");
    MD_REQUIRE(n_ent < (1ll << 40) && n_frames < (1ll << 40) && (n_ent == 0 || n_frames < (1ll << 40) / n_ent),
               "trajectory too large");
    MD_REQUIRE(box, "NULL box: the pair sums take the nearest image, which needs the box");
    MD_REQUIRE(nbins >= 1 && nbins <= VP_MAX_BINS, "nbins must be in [1, %d]", VP_MAX_BINS);
    MD_REQUIRE(bin_size > 0.0 && bin_size < __builtin_inf(), "bin_size must be positive and finite");
    MD_REQUIRE(n_groups == 0 || group_off, "NULL group_off");
    for (int g = 0; g < n_groups; ++g)
        MD_REQUIRE(group_off[g] >= 0 && group_off[g] <= group_off[g + 1] && group_off[g + 1] <= n_ent,
                   "group_off must ascend within [0, n_ent] (group %d)", g);
    MD_REQUIRE(n_jobs == 0 || (jobs && hist && sums && beyond && unsummed && pairs), "NULL array");
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 2 * (size_t)j;
        MD_REQUIRE(q[0] >= 0 && q[0] < n_groups && q[1] >= 0 && q[1] < n_groups, "job %d: group (%d, %d) out of range",
                   j, q[0], q[1]);
    }
    MD_REQUIRE((size_t)n_jobs * (size_t)nbins < ((size_t)1 << 30), "result too large");
    if (edges && n_jobs) {  // (the kernel walks the table: it has to start at 0 and ascend)
        MD_REQUIRE(edges[0] == 0.0, "edges[0] must be 0");
        for (int k = 0; k < nbins; ++k) MD_REQUIRE(edges[k] <= edges[k + 1], "edges must ascend (bin %d)", k);
    }
    if (n_jobs == 0) return cs.end();
    MD_REQUIRE(n_ent == 0 || n_frames == 0 || (site && vec), "NULL sites or vectors");

    // the jobs: which group lies along the lanes, units, workgroups
    std::vector<VpJob> tab((size_t)n_jobs);
    std::vector<uint64_t> n_pairs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs + 2 * (size_t)j;
        VpJob &J = tab[(size_t)j];
        const long long a0 = group_off[q[0]], na = group_off[q[0] + 1] - a0;
        const long long b0 = group_off[q[1]], nb = group_off[q[1] + 1] - b0;
        n_pairs[(size_t)j] = (uint64_t)n_frames * ((uint64_t)na * (uint64_t)nb - (q[0] == q[1] ? (uint64_t)na : 0));
        // lanes: the group that wastes fewer lanes of its last tile (na / tiles(na) against nb / tiles(nb))
        const long long ta = (na + 63) / 64, tb = (nb + 63) / 64;
        J.lane_is_j = na * tb < nb * ta;
        J.pad = 0;
        J.l0 = J.lane_is_j ? b0 : a0;
        J.nl = J.lane_is_j ? nb : na;
        J.u0 = J.lane_is_j ? a0 : b0;
        J.nu = J.lane_is_j ? na : nb;
        J.n_tiles = (J.nl + 63) / 64;
        J.n_jc = (J.nu + VP_JCHUNK - 1) / VP_JCHUNK;
        J.n_units = (long long)n_frames * J.n_tiles * J.n_jc;
        J.upb = 1;
        J.nblk = 0;
        if (J.n_units > 0) {
            const long long per_unit = 64 * std::min(J.nu, VP_JCHUNK);  // pairs of one unit at most
            const long long even = (J.n_units + VP_BLOCKS - 1) / VP_BLOCKS;
            const long long amortise = (32ll * nbins + per_unit - 1) / per_unit;  // zeroing and flushing a row
            J.upb = std::min(std::max({(long long)VP_WAVES, even, amortise}), VP_MAX_PAIRS / per_unit);
            J.nblk = (J.n_units + J.upb - 1) / J.upb;
        }
    }
    for (int j = 0; j < n_jobs; ++j)
        MD_REQUIRE(tab[(size_t)j].nblk < (1ll << 31), "job %d: too many workgroups", j);
    std::vector<double> own;
    if (!edges) {
        own.resize((size_t)nbins + 1);
        if (mdhip_bin_edges(bin_size, nbins, own.data()) != MDHIP_OK)
            return mdhip_fail(ctx, MDHIP_EINVAL, "no bin edges for bin_size %g", bin_size);
        edges = own.data();
    }
    std::copy(n_pairs.begin(), n_pairs.end(), pairs);
    // |error| of the f32 guess fma(sqrt((float)rsq), 1/bin_size, near), as vanhove.hip: relative 2.1e-7 of the bin number
    // plus half an ulp of the largest value each for the addend and the fma; near = 2 x that.
    const double ulp = std::ldexp(1.0, (int)std::floor(std::log2((double)nbins + 1.0)) - 23);
    const float near = (float)(2.0 * ((double)nbins * 2.1e-7 + ulp) + 1.0e-5);
    const float gscale = (float)(1.0 / bin_size);

    MD_HIP(hipSetDevice(ctx->device));
    int rc;
    const size_t in_bytes = (size_t)n_frames * 3 * (size_t)n_ent * 8;
    const double *d_site = (const double *)mdhip_stage(ctx, WS_XYZ_I, site, in_bytes, in_on_device || in_bytes == 0, &rc);
    if (rc) return rc;
    const double *d_vec = (const double *)mdhip_stage(ctx, WS_XYZ_J, vec, in_bytes, in_on_device || in_bytes == 0, &rc);
    if (rc) return rc;
    MD_WS(d_cnt, unsigned long long, WS_MISC, (size_t)n_jobs * 16);  // beyond | unsummed
    MD_WS(d_box, double, WS_BOX, std::max<size_t>((size_t)n_frames * 24, 8));
    if ((rc = mdhip_h2d_small(ctx, d_box, box, (size_t)n_frames * 24))) return rc;
    MD_WS(d_jobs, VpJob, WS_AUX2, tab.size() * sizeof(VpJob));
    if ((rc = mdhip_h2d_small(ctx, d_jobs, tab.data(), tab.size() * sizeof(VpJob)))) return rc;
    MD_WS(d_edges, double, WS_TABLES, ((size_t)nbins + 1) * 8);
    if ((rc = mdhip_h2d_small(ctx, d_edges, edges, ((size_t)nbins + 1) * 8))) return rc;
    const size_t hist_bytes = (size_t)n_jobs * (size_t)nbins * 8, sums_bytes = hist_bytes * 6;
    MD_WS(d_hist, unsigned long long, WS_HIST, hist_bytes + sums_bytes);  // hist | sums
    unsigned long long *d_sums = d_hist + hist_bytes / 8;
    const size_t lds_b = (size_t)nbins * 28;
    if (lds_b > 65536 - 64)
        MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vp_pair_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    KernelTimer timer(ctx, 0);
    int launches = 0;
    MD_HIP(hipMemsetAsync(d_cnt, 0, (size_t)n_jobs * 16, ctx->stream));
    MD_HIP(hipMemsetAsync(d_hist, 0, hist_bytes + sums_bytes, ctx->stream));
    // grid.y holds at most 65535 jobs: longer job lists go in slices (a job's workgroups are the same in any slice)
    for (int j0 = 0; j0 < n_jobs; j0 += VP_MAX_Y) {
        const int nj = std::min(VP_MAX_Y, n_jobs - j0);
        long long gx = 0;
        for (int j = j0; j < j0 + nj; ++j) gx = std::max(gx, tab[(size_t)j].nblk);
        if (gx == 0) continue;
        hipLaunchKernelGGL(vp_pair_kernel, dim3((unsigned)gx, (unsigned)nj), dim3(VP_THREADS), lds_b, ctx->stream, d_site,
                           d_vec, d_box, (long long)n_ent, d_jobs, j0, d_edges, gscale, near, (int)nbins, d_hist, d_sums,
                           d_cnt, d_cnt + n_jobs);
        MD_HIP(hipGetLastError());
        ++launches;
    }
    ctx->last_kernel = "vp_pair_kernel";
    ctx->last_launches = launches;
    timer.stop();
    if ((rc = mdhip_result(cs, hist, d_hist, hist_bytes, 0))) return rc;
    if ((rc = mdhip_result(cs, sums, d_sums, sums_bytes, 0))) return rc;
    if ((rc = mdhip_result(cs, beyond, d_cnt, (size_t)n_jobs * 8, 0))) return rc;
    if ((rc = mdhip_result(cs, unsummed, d_cnt + n_jobs, (size_t)n_jobs * 8, 0))) return rc;
    return mdhip_end_timed(cs, timer);
}

}  // extern "C"
