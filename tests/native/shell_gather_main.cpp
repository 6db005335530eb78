// The host part of csrc/shell_gather.h on the CPU (tests/test_shell_gather_native_cpu.py builds this with g++ under
// AddressSanitizer + UBSan; g++ sees nothing of the header's HIP part): the integer table packer and shares_an_atom on
// fixed and seeded random cases. Prints "<class> <count>" pairs and "failures <n>".
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../mdproptools_amd/csrc/shell_gather.h"

namespace {

long failures = 0, n_tables = 0, n_len0 = 0, n_len1 = 0, n_len4097 = 0, n_null0 = 0, n_absent = 0, n_generated = 0,
     n_six = 0, n_share = 0, n_disjoint = 0, n_identical = 0, n_first_end = 0, n_last_end = 0, n_empty_list = 0;

void fail(const char *what, long a, long b)
{
    if (++failures <= 20) std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
}

enum Kind { PLAIN, NULL0, OPTIONAL_ABSENT, OPTIONAL_GIVEN, GENERATED };
struct Seg {
    Kind kind;
    std::vector<int32_t> v;  // PLAIN / OPTIONAL_GIVEN: the source; GENERATED: what value(k) returns
};

// Packs the segments, lays the table at a base (a copy of its host vector: what the device holds after the upload)
// and checks every offset, every value seen through the resolved pointers, the total, and the pointers themselves.
void check_table(const std::vector<Seg> &segs)
{
    ++n_tables;
    shell::IntTable tab;
    std::vector<const int *> d(segs.size(), reinterpret_cast<const int *>(&failures));  // (neither null nor in the table)
    for (size_t s = 0; s < segs.size(); ++s) {
        const Seg &g = segs[s];
        const int32_t *p = g.v.empty() ? nullptr : g.v.data();
        // (an empty PLAIN segment is handed over with a real pointer: length 0 of an array that exists)
        static const int32_t nothing[1] = {0};
        switch (g.kind) {
        case PLAIN: tab.add(p ? p : nothing, g.v.size(), &d[s]); break;
        case NULL0: tab.add(nullptr, 0, &d[s]), ++n_null0; break;
        case OPTIONAL_ABSENT: tab.add_optional(nullptr, 12345, &d[s]), ++n_absent; break;
        case OPTIONAL_GIVEN: tab.add_optional(p ? p : nothing, g.v.size(), &d[s]); break;
        case GENERATED: tab.add_generated(g.v.size(), [&](size_t k) { return g.v[k]; }, &d[s]), ++n_generated; break;
        }
        if (g.kind != NULL0 && g.kind != OPTIONAL_ABSENT) {
            n_len0 += g.v.size() == 0, n_len1 += g.v.size() == 1, n_len4097 += g.v.size() == 4097;
        }
    }
    n_six += segs.size() >= 6;
    if (tab.off.size() != segs.size() || tab.dev.size() != segs.size()) fail("segment count", (long)tab.off.size(), 0);

    size_t expect = 0;  // the running total: where the next present segment begins
    for (size_t s = 0; s < segs.size(); ++s) {
        if (segs[s].kind == OPTIONAL_ABSENT) {
            if (tab.off[s] != shell::IntTable::ABSENT) fail("absent offset", (long)s, (long)tab.off[s]);
            continue;
        }
        if (tab.off[s] != expect) fail("offset", (long)s, (long)tab.off[s]);
        expect += segs[s].kind == NULL0 ? 0 : segs[s].v.size();
    }
    if (tab.host.size() != expect) fail("total", (long)tab.host.size(), (long)expect);

    const std::vector<int32_t> device(tab.host);  // (exactly tab.host.size() ints: a read past a segment's end that leaves
    tab.resolve(device.data());                   // the table is the sanitizer's to find)
    size_t at = 0;
    for (size_t s = 0; s < segs.size(); ++s) {
        if (segs[s].kind == OPTIONAL_ABSENT) {
            if (d[s] != nullptr) fail("absent segment not null", (long)s, 0);
            continue;
        }
        if (d[s] != device.data() + at) fail("pointer", (long)s, (long)at);  // (an empty one: where the next begins, or
        const size_t n = segs[s].kind == NULL0 ? 0 : segs[s].v.size();       // the end; never null, never before the last)
        for (size_t k = 0; k < n; ++k)
            if (d[s][k] != segs[s].v[k]) {
                fail("value", (long)s, (long)k);
                break;
            }
        at += n;
    }
}

std::vector<int32_t> values(std::mt19937_64 &rng, size_t n)
{
    std::vector<int32_t> v(n);
    for (auto &x : v) x = (int32_t)(rng() & 0x7FFFFFFF) - (int32_t)(rng() & 0xFFFF);
    return v;
}

void check_shares(int64_t n_atoms, const std::vector<int32_t> &a, const std::vector<int32_t> &b)
{
    bool brute = false;
    for (int32_t x : a)
        for (int32_t y : b) brute = brute || x == y;
    const bool got = shell::shares_an_atom(n_atoms, a.empty() ? nullptr : a.data(), (int64_t)a.size(),
                                           b.empty() ? nullptr : b.data(), (int64_t)b.size());
    if (got != brute) fail("shares_an_atom", (long)a.size(), (long)b.size());
    ++n_share;
}

}  // namespace

int main(int argc, char **argv)
{
    const long n_random = argc > 1 ? std::atol(argv[1]) : 2000;
    std::mt19937_64 rng(20240611);

    // ---- the packer: fixed tables ----
    const size_t lens[] = {0, 1, 2, 63, 4096, 4097};
    for (size_t la : lens)
        for (size_t lb : lens) {
            // the shapes of the five entry points: two to six segments, the optional one last
            check_table({{PLAIN, values(rng, la)}, {OPTIONAL_ABSENT, {}}});
            check_table({{PLAIN, values(rng, la)}, {OPTIONAL_GIVEN, values(rng, lb)}});
            check_table({{PLAIN, values(rng, la)}, {PLAIN, values(rng, lb)}, {PLAIN, values(rng, lb)},
                         {OPTIONAL_ABSENT, {}}});
            check_table({{PLAIN, values(rng, la)}, {GENERATED, values(rng, la)}, {PLAIN, values(rng, lb)},
                         {PLAIN, values(rng, lb)}, {GENERATED, values(rng, lb)}});
            check_table({{PLAIN, values(rng, la)}, {PLAIN, values(rng, la + 1)}, {NULL0, {}}, {PLAIN, values(rng, lb)},
                         {PLAIN, values(rng, lb)}, {OPTIONAL_GIVEN, values(rng, 4097)}});
            check_table({{NULL0, {}}, {PLAIN, values(rng, la)}, {NULL0, {}}, {NULL0, {}}, {PLAIN, values(rng, lb)},
                         {OPTIONAL_ABSENT, {}}});
        }
    check_table({});
    check_table({{NULL0, {}}});
    check_table({{OPTIONAL_ABSENT, {}}});
    check_table({{OPTIONAL_ABSENT, {}}, {PLAIN, values(rng, 1)}});  // (absent in the middle: the next begins at 0)

    // ---- the packer: seeded random tables ----
    for (long t = 0; t < n_random; ++t) {
        std::vector<Seg> segs(1 + rng() % 8);
        for (Seg &g : segs) {
            g.kind = (Kind)(rng() % 5);
            const unsigned pick = (unsigned)(rng() % 8);
            const size_t n = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? 4097 : (size_t)(rng() % 300);
            if (g.kind != NULL0 && g.kind != OPTIONAL_ABSENT) g.v = values(rng, n);
        }
        check_table(segs);
    }

    // ---- shares_an_atom ----
    const int64_t N = 5000;
    std::vector<int32_t> even, odd;
    for (int32_t k = 0; k < N; k += 2) even.push_back(k), odd.push_back(k + 1);
    check_shares(N, even, odd), ++n_disjoint;
    check_shares(N, odd, even), ++n_disjoint;
    check_shares(N, even, even), ++n_identical;
    check_shares(N, {7}, {7}), ++n_identical;
    for (const auto *list : {&even, &odd}) {
        std::vector<int32_t> b(list == &even ? odd : even);
        b.front() = list->front();  // one shared atom, at the first place of both
        check_shares(N, *list, b), ++n_first_end;
        b = list == &even ? odd : even;
        b.back() = list->back();  // ... at the last place of both
        check_shares(N, *list, b), ++n_last_end;
        b = list == &even ? odd : even;
        b.front() = list->back();  // ... first of one, last of the other
        check_shares(N, *list, b), ++n_first_end, ++n_last_end;
    }
    check_shares(N, {}, even), ++n_empty_list;
    check_shares(N, even, {}), ++n_empty_list;
    check_shares(N, {}, {}), ++n_empty_list;
    check_shares(0, {}, {}), ++n_empty_list;
    check_shares(1, {0}, {0}), ++n_identical;
    check_shares(N, {0, (int32_t)N - 1}, {(int32_t)N - 1}), ++n_last_end;  // (the ends of the index range)
    check_shares(N, {0, (int32_t)N - 1}, {1, 0}), ++n_first_end;
    for (long t = 0; t < n_random; ++t) {
        const int64_t n = 1 + (int64_t)(rng() % 200);
        std::vector<int32_t> a(rng() % 12), b(rng() % 12);
        for (auto &x : a) x = (int32_t)(rng() % (uint64_t)n);
        for (auto &x : b) x = (int32_t)(rng() % (uint64_t)n);
        check_shares(n, a, b);
    }

    std::printf("tables %ld len0 %ld len1 %ld len4097 %ld null0 %ld absent %ld generated %ld six %ld shares %ld "
                "disjoint %ld identical %ld first_end %ld last_end %ld empty_list %ld failures %ld\n",
                n_tables, n_len0, n_len1, n_len4097, n_null0, n_absent, n_generated, n_six, n_share, n_disjoint,
                n_identical, n_first_end, n_last_end, n_empty_list, failures);
    return failures ? 1 : 0;
}
