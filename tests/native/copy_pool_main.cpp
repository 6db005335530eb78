// copy_pool_main.cpp — csrc/copy_pool.h on its own (tests/test_copy_pool_native_cpu.py builds this file twice: with the
// thread sanitizer, and with the address and undefined-behaviour sanitizers). CopyPool is the set of helper threads that
// fills the page-locked ring of mdhip_h2d_any; here it copies between ordinary heap buffers:
//   - every size of SIZES x source offset x destination offset of OFFS: contents by memcmp, guard bytes on both sides of
//     the destination untouched (8 MiB is one ring chunk, 8 MiB + 40 the size at which three helpers get nothing);
//   - a few thousand back-to-back copies of seeded random sizes through one pool;
//   - 200 pools constructed and destroyed, most without a single copy (the constructor/destructor hand-off);
//   - two pools driven from two caller threads at once.
// Prints "copies <n> failures <m>" and exits non-zero when m > 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../mdproptools_amd/csrc/copy_pool.h"

namespace {

constexpr size_t GUARD = 128;
constexpr unsigned char GUARD_BYTE = 0xA5, STALE_BYTE = 0x5A;

struct Rng {
    uint64_t s;
    uint64_t next()
    {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
};

long long g_copies = 0;

// src: a buffer whose byte i is a function of (i, salt); room for the largest size + the largest offset
void fill_source(std::vector<unsigned char> &src, uint64_t salt)
{
    Rng r{0x9E3779B97F4A7C15ull ^ (salt * 0xD1342543DE82EF95ull + 1)};
    size_t i = 0;
    for (; i + 8 <= src.size(); i += 8) {
        const uint64_t v = r.next();
        memcpy(&src[i], &v, 8);
    }
    for (; i < src.size(); ++i) src[i] = (unsigned char)r.next();
}

// One copy of n bytes from src + so to a destination that starts `dofs` bytes past the guard; returns the failures.
int one_copy(CopyPool &pool, const std::vector<unsigned char> &src, size_t so, std::vector<unsigned char> &dst, size_t dofs,
             size_t n, const char *what)
{
    const size_t need = GUARD + dofs + n + GUARD;
    if (dst.size() < need || so + n > src.size()) {
        printf("FAIL %s: buffers too small for n=%zu\n", what, n);
        return 1;
    }
    // the guards, and stale bytes where the copy goes
    memset(dst.data(), GUARD_BYTE, GUARD + dofs);
    memset(dst.data() + GUARD + dofs, STALE_BYTE, n);
    memset(dst.data() + GUARD + dofs + n, GUARD_BYTE, GUARD);
    pool.copy(dst.data() + GUARD + dofs, src.data() + so, n);
    int bad = 0;
    if (n && memcmp(dst.data() + GUARD + dofs, src.data() + so, n) != 0) {
        size_t at = 0;
        while (dst[GUARD + dofs + at] == src[so + at]) ++at;
        printf("FAIL %s: n=%zu src+%zu dst+%zu: first wrong byte at %zu\n", what, n, so, dofs, at);
        ++bad;
    }
    for (size_t k = 0; k < GUARD + dofs; ++k)
        if (dst[k] != GUARD_BYTE) {
            printf("FAIL %s: n=%zu src+%zu dst+%zu: byte %zu BEFORE the destination written\n", what, n, so, dofs, GUARD + dofs - k);
            ++bad;
            break;
        }
    for (size_t k = 0; k < GUARD; ++k)
        if (dst[GUARD + dofs + n + k] != GUARD_BYTE) {
            printf("FAIL %s: n=%zu src+%zu dst+%zu: byte %zu AFTER the destination written\n", what, n, so, dofs, k);
            ++bad;
            break;
        }
    return bad;
}

const size_t SIZES[] = {0, 1, 7, 8, 40, 63, 64, 65, 255, 256, 257, (size_t)1 << 20, (size_t)8 << 20, ((size_t)8 << 20) + 40};
const size_t OFFS[] = {0, 1, 8, 63};
constexpr size_t MAX_N = ((size_t)8 << 20) + 40;

int fixed_sizes()
{
    int bad = 0;
    std::vector<unsigned char> src(MAX_N + 64), dst(GUARD + 64 + MAX_N + GUARD);
    fill_source(src, 1);
    CopyPool pool;
    for (size_t n : SIZES)
        for (size_t so : OFFS)
            for (size_t dofs : OFFS) {
                bad += one_copy(pool, src, so, dst, dofs, n, "fixed");
                ++g_copies;
            }
    return bad;
}

// back-to-back copies of random sizes through ONE pool: small ones mostly, a few up to 300 KB; offsets 0..63
int random_sizes(CopyPool &pool, uint64_t seed, int count, long long *copies)
{
    int bad = 0;
    const size_t cap = 300 * 1024;
    std::vector<unsigned char> src(cap + 64), dst(GUARD + 64 + cap + GUARD);
    fill_source(src, seed);
    Rng r{seed * 0x2545F4914F6CDD1Dull + 77};
    for (int it = 0; it < count; ++it) {
        const uint64_t v = r.next();
        const size_t lim = (v & 15) == 0 ? cap : (v & 3) == 0 ? 4096 : 300;
        const size_t n = (size_t)((v >> 8) % (lim + 1));
        bad += one_copy(pool, src, (size_t)((v >> 40) & 63), dst, (size_t)((v >> 48) & 63), n, "random");
        ++*copies;
    }
    return bad;
}

int many_pools()
{
    int bad = 0;
    std::vector<unsigned char> src(4096 + 64), dst(GUARD + 64 + 4096 + GUARD);
    fill_source(src, 3);
    for (int k = 0; k < 200; ++k) {
        CopyPool pool;  // (k % 4 != 0: destroyed before its helpers have been given anything)
        if (k % 4 == 0) {
            bad += one_copy(pool, src, (size_t)(k % 64), dst, (size_t)(k % 7), (size_t)(k * 19 % 4097), "pools");
            ++g_copies;
        }
    }
    // on the heap, as the library holds it
    for (int k = 0; k < 8; ++k) {
        std::unique_ptr<CopyPool> pool(new CopyPool());
        if (k & 1) {
            bad += one_copy(*pool, src, 0, dst, 0, 4096, "pools");
            ++g_copies;
        }
    }
    return bad;
}

int two_callers()
{
    int bad[2] = {0, 0};
    long long copies[2] = {0, 0};
    CopyPool pools[2];
    std::thread callers[2];
    for (int t = 0; t < 2; ++t)
        callers[t] = std::thread([&, t]() { bad[t] = random_sizes(pools[t], 100 + (uint64_t)t, 1500, &copies[t]); });
    for (auto &c : callers) c.join();
    g_copies += copies[0] + copies[1];
    return bad[0] + bad[1];
}

}  // namespace

int main()
{
    int bad = 0;
    bad += fixed_sizes();
    {
        CopyPool pool;
        long long copies = 0;
        bad += random_sizes(pool, 42, 4000, &copies);
        g_copies += copies;
    }
    bad += many_pools();
    bad += two_callers();
    printf("copies %lld failures %d\n", g_copies, bad);
    return bad ? 1 : 0;
}
