// call_tables_main.cpp — walks the table packer of csrc/call_tables.h (the host-only part: where every segment of a
// call's device tables lies in its workspace slot) over fixed layouts and seeded random ones;
// tests/test_call_tables_native_cpu.py builds it with g++ under -fsanitize=address,undefined. g++ sees nothing of the
// header's upload.
// Fixed layouts: elements of 1, 2, 4, 8, 40 and 48 bytes with counts 0, 1 and odd; optional segments, absent and
// present, at the front, in the middle and at the end; zeroed segments. Checked for every layout, on a real buffer of
// `total` bytes: every offset is a multiple of 8; a segment begins at the first such offset behind the one before;
// no two segments overlap (every segment's bytes are written, then all are read back); the total is the end of the last
// segment that takes room; an absent segment has a null pointer; an empty one takes no room and points at what follows.
// And the layouts of the five entry points, for one small call each, against the sums their hand-written versions
// gave, typed in as numbers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "../../mdproptools_amd/csrc/call_tables.h"

static long failures = 0, n_layouts = 0, n_segments = 0, n_absent = 0, n_empty = 0;
static std::string what;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (failures++ < 20) fprintf(stderr, "%s: %s (line %d)\n", what.c_str(), #cond, __LINE__); \
        }                                                                                \
    } while (0)

template <int N>
struct El {
    unsigned char b[N];
};

enum Kind { ADD, OPTIONAL, ABSENT, ZEROED };
struct Spec {
    int size;  // bytes per element: 1, 2, 4, 8, 16, 32, 40 or 48
    size_t count;
    Kind kind;
};

// the typed device pointer of one segment, whatever its element; it starts out pointing at `stale`, so that a null
// pointer is one that resolve() has set
static unsigned char stale[64];
template <class T>
static T *stale_as() { return reinterpret_cast<T *>(stale); }
struct Slot {
    const El<1> *p1 = stale_as<El<1>>();
    const El<2> *p2 = stale_as<El<2>>();
    const El<4> *p4 = stale_as<El<4>>();
    const El<8> *p8 = stale_as<El<8>>();
    const El<16> *p16 = stale_as<El<16>>();
    const El<32> *p32 = stale_as<El<32>>();
    const El<40> *p40 = stale_as<El<40>>();
    const El<48> *p48 = stale_as<El<48>>();
    El<4> *z4 = stale_as<El<4>>();
    El<8> *z8 = stale_as<El<8>>();
    const void *get(const Spec &s) const
    {
        if (s.kind == ZEROED) return s.size == 4 ? (const void *)z4 : (const void *)z8;
        switch (s.size) {
        case 1: return p1;
        case 2: return p2;
        case 4: return p4;
        case 8: return p8;
        case 16: return p16;
        case 32: return p32;
        case 40: return p40;
        default: return p48;
        }
    }
};

template <int N>
static void name(CallTables &tab, const Spec &s, const unsigned char *host, const El<N> **d)
{
    const El<N> *p = reinterpret_cast<const El<N> *>(host);
    if (s.kind == ADD) tab.add(p, s.count, d);
    else tab.add_optional(s.kind == ABSENT ? nullptr : p, s.count, d);
}

// Builds the layout, resolves it on a buffer and checks it; offsets[k] = where segment k came to lie (ABSENT: absent).
static std::vector<size_t> check(const std::vector<Spec> &specs, const char *label, size_t *total_out = nullptr)
{
    what = label;
    ++n_layouts;
    const size_t S = specs.size();
    std::vector<std::vector<unsigned char>> host(S);
    std::vector<Slot> slots(S);
    CallTables tab;
    for (size_t k = 0; k < S; ++k) {
        const Spec &s = specs[k];
        // (an empty std::vector may hand out a null pointer, as the entry points' vectors do; OPTIONAL needs a real one)
        host[k].assign(s.count * (size_t)s.size + (s.kind == OPTIONAL), (unsigned char)(k + 1));
        const unsigned char *h = host[k].data();
        Slot &d = slots[k];
        if (s.kind == ZEROED) {
            if (s.size == 4) tab.add_zeroed(s.count, &d.z4);
            else tab.add_zeroed(s.count, &d.z8);
            continue;
        }
        switch (s.size) {
        case 1: name<1>(tab, s, h, &d.p1); break;
        case 2: name<2>(tab, s, h, &d.p2); break;
        case 4: name<4>(tab, s, h, &d.p4); break;
        case 8: name<8>(tab, s, h, &d.p8); break;
        case 16: name<16>(tab, s, h, &d.p16); break;
        case 32: name<32>(tab, s, h, &d.p32); break;
        case 40: name<40>(tab, s, h, &d.p40); break;
        default: name<48>(tab, s, h, &d.p48); break;
        }
    }
    CHECK(tab.segments.size() == S);
    std::vector<uint64_t> room(tab.total / 8 + 2, 0);  // (8-aligned, and a past-the-end pointer stays inside)
    char *const base = reinterpret_cast<char *>(room.data());
    tab.resolve(base);
    std::vector<size_t> offsets(S, CallTables::ABSENT);
    size_t end = 0;  // of the last segment that takes room
    for (size_t k = 0; k < S; ++k, ++n_segments) {
        const Spec &s = specs[k];
        const char *at = static_cast<const char *>(slots[k].get(s));
        const size_t bytes = s.count * (size_t)s.size;
        if (s.kind == ABSENT) {
            ++n_absent;
            CHECK(at == nullptr);
            continue;
        }
        CHECK(at != nullptr && at >= base);
        if (!at || at < base) return offsets;
        const size_t off = (size_t)(at - base);
        offsets[k] = off;
        CHECK(off % 8 == 0);
        CHECK(off >= end && off - end < 8);  // the first aligned offset behind the segment before: no overlap, no gap
        CHECK(off + bytes <= tab.total || bytes == 0);
        if (off + bytes > room.size() * 8) return offsets;
        if (bytes) {
            end = off + bytes;
            memset(base + off, (int)(k + 1), bytes);  // what the upload writes there (zeroed segments: their own mark)
        } else {
            ++n_empty;
        }
    }
    CHECK(tab.total == end);
    // every segment still holds its own bytes: no two overlap
    for (size_t k = 0; k < S; ++k) {
        if (offsets[k] == CallTables::ABSENT) continue;
        const size_t bytes = specs[k].count * (size_t)specs[k].size;
        for (size_t i = 0; i < bytes; ++i)
            if ((unsigned char)base[offsets[k] + i] != (unsigned char)(k + 1)) {
                CHECK(!"a segment was overwritten by another");
                break;
            }
    }
    // an empty segment points at what follows
    for (size_t k = 0; k + 1 < S; ++k) {
        if (offsets[k] == CallTables::ABSENT || specs[k].count) continue;
        size_t next = k + 1;
        while (next < S && offsets[next] == CallTables::ABSENT) ++next;
        if (next < S) CHECK(offsets[k] == offsets[next]);
    }
    // what the packer recorded for the upload
    for (size_t k = 0; k < S && k < tab.segments.size(); ++k) {
        const CallTables::Segment &g = tab.segments[k];
        CHECK(g.off == offsets[k]);
        if (specs[k].kind == ABSENT) continue;
        CHECK(g.bytes == specs[k].count * (size_t)specs[k].size);
        CHECK(specs[k].kind == ZEROED ? g.host == nullptr : (g.bytes == 0 || g.host == host[k].data()));
    }
    if (total_out) *total_out = tab.total;
    return offsets;
}

static void expect(const std::vector<Spec> &specs, const char *label, const std::vector<size_t> &want, size_t want_total)
{
    size_t total = 0;
    const std::vector<size_t> got = check(specs, label, &total);
    CHECK(got == want);
    CHECK(total == want_total);
}

int main(int argc, char **argv)
{
    const size_t NONE = CallTables::ABSENT;
    const int sizes[] = {1, 2, 4, 8, 40, 48};
    // one segment of every element size and count between two others
    for (int size : sizes)
        for (size_t count : {(size_t)0, (size_t)1, (size_t)3, (size_t)7, (size_t)101})
            for (Kind kind : {ADD, OPTIONAL}) {
                check({{size, count, kind}}, "alone");
                check({{size, count, kind}, {8, 2, ADD}}, "front");
                check({{4, 3, ADD}, {size, count, kind}, {8, 2, ZEROED}}, "middle");
                check({{40, 2, ADD}, {1, 5, ADD}, {size, count, kind}}, "end");
            }
    // absent segments at the front, in the middle, at the end, side by side, and nothing else
    check({{8, 4, ABSENT}, {4, 3, ADD}, {8, 2, ZEROED}}, "absent front");
    check({{4, 3, ADD}, {8, 4, ABSENT}, {8, 2, ZEROED}}, "absent middle");
    check({{4, 3, ADD}, {8, 2, ZEROED}, {8, 4, ABSENT}}, "absent end");
    check({{4, 3, ADD}, {8, 4, ABSENT}, {2, 4, ABSENT}, {4, 0, ADD}, {8, 2, ZEROED}}, "absent, absent, empty");
    check({{8, 4, ABSENT}}, "only absent");
    check({}, "nothing");
    // zeroed segments: 4- and 8-byte counters, empty, behind an odd int segment
    check({{8, 3, ZEROED}}, "zeroed alone");
    check({{4, 5, ADD}, {8, 3, ZEROED}}, "zeroed behind odd ints");
    check({{4, 5, ZEROED}, {8, 0, ZEROED}, {4, 1, ZEROED}}, "zeroed, empty zeroed, zeroed");

    // The entry points, one small call each. Elements: MolClass 40, AxJob 16, MmJob 32, DhJob 32, ShJob 48, ShRun 16 bytes.
    // mdhip_axis_vectors, 3 jobs with 1 + 3 + 1 terms: classes | jobs | term weights | term atoms | degenerate counters
    expect({{40, 3, ADD}, {16, 3, ADD}, {8, 5, ADD}, {4, 5, ADD}, {8, 3, ZEROED}}, "axis vectors", {0, 120, 168, 208, 232}, 256);
    // mdhip_mol_moments, 3 jobs with 2 site and 5 vector terms in all: the same segments, MmJob
    expect({{40, 3, ADD}, {32, 3, ADD}, {8, 7, ADD}, {4, 7, ADD}, {8, 3, ZEROED}}, "moments", {0, 120, 216, 272, 304}, 328);
    // ... and without any term: both term segments empty, the counters right behind the jobs
    expect({{40, 3, ADD}, {32, 3, ADD}, {8, 0, ADD}, {4, 0, ADD}, {8, 3, ZEROED}}, "moments, no terms", {0, 120, 216, 216, 216}, 240);
    // mdhip_dihedral_angles, 3 jobs in 2 classes, n_bins = 10: classes | jobs | edges (5, with hist) | degenerate counters
    expect({{40, 2, ADD}, {32, 3, ADD}, {8, 5, OPTIONAL}, {8, 3, ZEROED}}, "dihedrals, hist", {0, 80, 176, 216}, 240);
    expect({{40, 2, ADD}, {32, 3, ADD}, {8, 5, ABSENT}, {8, 3, ZEROED}}, "dihedrals, series only", {0, 80, NONE, 176}, 200);
    // mdhip_mol_shape, 2 jobs of 4 and 1025 atoms, nbins = 4: jobs | staged runs (3) | walk runs (1) | weights | edges
    expect({{48, 2, ADD}, {16, 3, ADD}, {16, 1, ADD}, {8, 1029, ADD}, {8, 5, ADD}}, "shape", {0, 96, 144, 160, 8392}, 8432);
    expect({{48, 1, ADD}, {16, 3, ADD}, {16, 0, ADD}, {8, 4, ADD}, {8, 5, ADD}}, "shape, staged only", {0, 48, 96, 96, 128}, 168);
    // mdhip_free_volume, 7 atoms, 3 classes, nbins = 6, 2 probes: classes | radius | edges | probe
    expect({{4, 7, ADD}, {8, 3, ADD}, {8, 7, ADD}, {8, 2, ADD}}, "free volume", {0, 32, 56, 112}, 128);

    const int n_random = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20261021);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    const int all_sizes[] = {1, 2, 4, 8, 16, 32, 40, 48};
    const size_t counts[] = {0, 0, 1, 1, 2, 3, 5, 7, 8, 9, 63, 257};
    for (int r = 0; r < n_random; ++r) {
        std::vector<Spec> specs((size_t)pick(1, 9));
        for (Spec &s : specs) {
            s.kind = (Kind)pick(0, 3);
            s.size = s.kind == ZEROED ? (pick(0, 1) ? 4 : 8) : all_sizes[pick(0, 7)];
            s.count = counts[pick(0, 11)];
        }
        check(specs, "random");
    }
    printf("layouts %ld segments %ld absent %ld empty %ld failures %ld\n", n_layouts, n_segments, n_absent, n_empty, failures);
    return failures ? 1 : 0;
}
