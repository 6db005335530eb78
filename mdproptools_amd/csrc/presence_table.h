// presence_table.h — presence masks of pairs over a trajectory and their intermittent lag sums. A pair (any 63-bit
// key) that is "present" in frame t has bit t of its mask set; the masks (ceil(F / 64) words each) live in an
// open-addressing hash table, and
//
//     c_int[k] = sum_pairs sum_t h(t) h(t + k) = sum_pairs popcount(mask & (mask >> k))
//
// is exact integer work over the occupied slots. The table (slot claim, probe limit, sizing) and the lag kernel are the
// ones of residence.hip (shell_pairs_kernel's rt_slot, residence_lag_kernel), with the lag range a parameter instead of
// always all F lags. residence.hip keeps its own copies: the committed counter runs of that file are tied to it byte
// for byte (hydrogen bonds). hbonds.hip is the one user of this header so far; nothing here knows what a
// key means, so that residence can adopt it.
#pragma once

#include <algorithm>

#include "ctx.h"

namespace presence {

constexpr unsigned long long EMPTY = ~0ull;  // (a pair key is < 2^63)
constexpr unsigned NONE = ~0u;
constexpr int MAX_FRAMES = 65535;            // the mask (<= 1024 words) is staged whole in LDS
constexpr unsigned FIRST_PROBES = 512;       // probe limit of a first sweep (a re-sweep's table holds every pair)

// the table on the device: keys [slots] | masks [slots][words]
struct Table {
    unsigned long long *keys = nullptr, *masks = nullptr;
    unsigned long long slots = 0;  // a power of two
    int words = 0;
};

__device__ __forceinline__ unsigned long long mix(unsigned long long x)
{
    // splitmix64's finaliser: consecutive keys land far apart
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// the slot of `key` (claimed with one compare-and-swap if new); NONE when `max_probe` slots in a row were other
// pairs': the table is too small, and the host sweeps again with one sized from the hit count
__device__ __forceinline__ unsigned claim(unsigned long long *__restrict__ keys, unsigned slot_mask, unsigned max_probe,
                                          unsigned long long key)
{
    unsigned h = (unsigned)mix(key) & slot_mask;
    for (unsigned probe = 0; probe < max_probe; ++probe) {
        const unsigned long long seen = atomicCAS(&keys[h], EMPTY, key);
        if (seen == EMPTY || seen == key) return h;
        h = (h + 1u) & slot_mask;
    }
    return NONE;
}

// sets bit t of the mask of `key`; false when the key found no slot
__device__ __forceinline__ bool mark(const Table &tb, unsigned max_probe, unsigned long long key, long long t)
{
    const unsigned slot = claim(tb.keys, (unsigned)(tb.slots - 1), max_probe, key);
    if (slot == NONE) return false;
    atomicOr(&tb.masks[(size_t)slot * (size_t)tb.words + (size_t)(t >> 6)], 1ull << (t & 63));
    return true;
}

// One wave per occupied slot (grid-stride over the table), grid.y the lag windows [k0, k0 + win) of the lags
// [0, n_lags). LDS: presence mask [words + 1] + lag table [win] (u64).
static __global__ __launch_bounds__(64) void lag_kernel(Table tb, int n_frames, int n_lags, int win,
                                                        unsigned long long *__restrict__ counts)
{
    extern __shared__ unsigned long long s_presence[];
    const int words = tb.words;
    unsigned long long *mask = s_presence;               // [words + 1] (one zero word behind the end)
    unsigned long long *table = s_presence + words + 1;  // [win]: lag k0 + k at table[k]
    const int lane = threadIdx.x;
    const int k0 = (int)blockIdx.y * win, K = n_lags - k0 < win ? n_lags - k0 : win;
    for (int k = lane; k < K; k += 64) table[k] = 0ull;
    if (lane == 0) mask[words] = 0ull;
    for (unsigned long long r = blockIdx.x; r < tb.slots; r += gridDim.x) {
        if (tb.keys[r] == EMPTY) continue;  // (wave-uniform)
        __syncthreads();                    // (the previous pair's lags have read the mask)
        int t_first = n_frames, t_last = -1;
        for (int w = lane; w < words; w += 64) {
            const unsigned long long m = tb.masks[(size_t)r * (size_t)words + w];
            mask[w] = m;
            if (m) {
                const int lo = 64 * w + __builtin_ctzll(m), hi = 64 * w + 63 - __builtin_clzll(m);
                t_first = lo < t_first ? lo : t_first;
                t_last = hi > t_last ? hi : t_last;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int a = __shfl_xor(t_first, off, 64), b = __shfl_xor(t_last, off, 64);
            t_first = a < t_first ? a : t_first;
            t_last = b > t_last ? b : t_last;
        }
        __syncthreads();
        const int span = t_last - t_first;  // lags beyond the span see no overlap
        const int w0 = t_first >> 6, w1 = t_last >> 6;
        const int lag_end = span < k0 + K - 1 ? span : k0 + K - 1;
        for (int lag = k0 + lane; lag <= lag_end; lag += 64) {
            const int q = lag >> 6, sh = lag & 63;
            unsigned long long c = 0;
            for (int w = w0; w + q <= w1; ++w) {
                const unsigned long long lo = mask[w + q], hi = mask[w + q + 1];
                const unsigned long long shifted = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
                c += (unsigned long long)__builtin_popcountll(mask[w] & shifted);
            }
            table[lag - k0] += c;  // a lag belongs to one lane: no conflict
        }
    }
    __syncthreads();
    for (int k = lane; k < K; k += 64)
        if (table[k]) atomicAdd(&counts[k0 + k], table[k]);
}

// ---- host ----

inline int words_of(int64_t n_frames) { return (int)((n_frames + 63) / 64); }
inline size_t slot_bytes(int words) { return 8 + (size_t)words * 8; }

inline unsigned long long pow2_at_least(double v, unsigned long long lo = 1024)
{
    unsigned long long p = lo;
    while ((double)p < v && p < (1ull << 31)) p <<= 1;
    return p;
}

// What a table in workspace `slot` may take: three quarters of the device memory that is free now plus what the
// slot already holds (the workspace frees before it grows, and grows by an eighth more than it is asked for).
inline int budget(mdhip_ctx *ctx, int slot, size_t &bytes)
{
    size_t free_b = 0, total_b = 0;
    MD_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t have = free_b + mdhip_ws_cap(ctx, slot);
    bytes = have - have / 4;
    return MDHIP_OK;
}

// Takes the table of `slots` slots from workspace `slot` and clears it (on the stream).
inline int take(mdhip_ctx *ctx, int slot, unsigned long long slots, int words, Table &tb)
{
    unsigned char *d = (unsigned char *)mdhip_ws(ctx, slot, (size_t)slots * slot_bytes(words));
    if (!d) return MDHIP_ENOMEM;
    tb.keys = reinterpret_cast<unsigned long long *>(d);
    tb.masks = tb.keys + slots;
    tb.slots = slots;
    tb.words = words;
    MD_HIP(hipMemsetAsync(tb.keys, 0xFF, (size_t)slots * 8, ctx->stream));
    MD_HIP(hipMemsetAsync(tb.masks, 0, (size_t)slots * (size_t)words * 8, ctx->stream));
    return MDHIP_OK;
}

// the probe limit of sweep number `sweep` (a second sweep's table holds every pair at half load at the most: its
// probes may walk as far as they must)
inline unsigned probes(int sweep, unsigned long long slots)
{
    return sweep == 0 ? std::min<unsigned long long>(FIRST_PROBES, slots)
                      : (unsigned)std::min<unsigned long long>(slots, 0xFFFFFFFFull);
}

// Launches lag_kernel for the lags [0, n_lags) into counts [n_lags] (zeroed by the caller): ONE window while mask and
// lags fit LDS, else as many windows (grid.y) as LDS requires, each reading the masks again.
inline int lag_launch(mdhip_ctx *ctx, const Table &tb, int64_t n_frames, int n_lags, unsigned long long *counts)
{
    const int words = tb.words;
    MD_REQUIRE(((size_t)words + 1 + 64) * 8 <= ctx->lds_max - 512, "%lld frames: the presence mask exceeds LDS",
               (long long)n_frames);
    const size_t lds_lags = (ctx->lds_max - 512) / 8 - ((size_t)words + 1);  // (lag slots beside the mask)
    int win = n_lags, n_win = 1;
    if ((size_t)n_lags > lds_lags) {
        n_win = (int)(((size_t)n_lags + lds_lags - 1) / lds_lags);
        win = (int)std::min<size_t>(lds_lags / 64 * 64, ((size_t)(n_lags + n_win - 1) / n_win + 63) / 64 * 64);
        n_win = (n_lags + win - 1) / win;
    }
    const size_t lds_b = ((size_t)words + 1 + (size_t)win) * 8;
    if (lds_b > 65536)
        MD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(lag_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    const unsigned grid = (unsigned)std::min<unsigned long long>(tb.slots, (unsigned long long)ctx->cu_count * 16);
    hipLaunchKernelGGL(lag_kernel, dim3(grid, (unsigned)n_win), dim3(64), lds_b, ctx->stream, tb, (int)n_frames, n_lags,
                       win, counts);
    MD_HIP(hipGetLastError());
    return MDHIP_OK;
}

}  // namespace presence
