// call_tables.h — the small device tables of one call, packed into one workspace slot: what stands between "the
// arguments are valid" and "the kernel is launched" in mdhip_axis_vectors (reorient.hip), mdhip_mol_moments
// (moments.hip), mdhip_dihedral_angles (dihedrals.hip), mdhip_mol_shape (mol_shape.hip) and mdhip_free_volume
// (free_volume.hip). An entry point names its segments in order — classes | jobs | term weights | term atoms |
// degenerate counters, say — each with the typed device pointer that is to point at it; CallTables computes every
// offset and the size of the slot, upload_tables takes the slot, sets the pointers and issues ONE small copy per
// segment that has a host source and ONE memset per zeroed segment, in the order named. (One copy per segment, not one
// for the table: which copies take the small-copy kernel route is part of a call's behaviour on the stream.
// shell::IntTable of shell_gather.h, whose names these are, packs on the host and copies once.)
// Left out on purpose: velocity_spectrum.hip aligns its tables differently and copies large ones straight from the
// caller's memory; segment_com.hip uploads one of two tables.
// The host part is plain C++17 (no HIP header, no context), in the form of shell_gather.h and group_pairs.h:
// tests/native/call_tables_main.cpp walks it with g++ under sanitizers; the rest is for hipcc only. An unnamed namespace,
// as mol_tile.h.
#pragma once
#include <cstddef>
#include <vector>

namespace {

// ---- host part ------------------------------------------------------------------------------------------------------

struct CallTables {
    static constexpr size_t ABSENT = ~(size_t)0, ALIGN = 8;  // every segment starts ALIGN-aligned
    struct Segment {
        const void *host;  // nullptr: zeroed, or absent
        size_t bytes, off;  // off == ABSENT: an optional segment the caller left out
        void *dev;          // the caller's typed device pointer, set by resolve() through `set`
        void (*set)(void *dev, char *at);
    };
    std::vector<Segment> segments;  // in the order they were named
    size_t total = 0;               // the end of the last segment that takes room: the bytes of the slot

    // n elements from p; n == 0 is an empty segment: it takes no room, and its pointer is that of what follows
    template <class T>
    void add(const T *p, size_t n, const T **d)
    {
        place(p, n * sizeof(T), d, set_as<const T>);
    }
    // an optional table: without one (p == nullptr) the kernels get a null pointer, and it takes no room
    template <class T>
    void add_optional(const T *p, size_t n, const T **d)
    {
        if (p) return add(p, n, d);
        segments.push_back({nullptr, 0, ABSENT, d, set_as<const T>});
    }
    // n elements without a host source that the kernels find zeroed (counters)
    template <class T>
    void add_zeroed(size_t n, T **d)
    {
        place(nullptr, n * sizeof(T), d, set_as<T>);
    }
    void resolve(char *base) const
    {
        for (const Segment &s : segments) s.set(s.dev, s.off == ABSENT ? nullptr : base + s.off);
    }

private:
    template <class T>
    static void set_as(void *dev, char *at)
    {
        *static_cast<T **>(dev) = reinterpret_cast<T *>(at);
    }
    void place(const void *host, size_t bytes, void *dev, void (*set)(void *, char *))
    {
        const size_t off = (total + ALIGN - 1) / ALIGN * ALIGN;
        segments.push_back({host, bytes, off, dev, set});
        if (bytes) total = off + bytes;
    }
};

}  // namespace

#ifdef __HIPCC__
#include "ctx.h"

namespace {

// the tables into workspace `slot`, on the call's stream
inline int upload_tables(mdhip_ctx *ctx, const CallTables &tab, int slot)
{
    MD_WS(d_tab, char, slot, tab.total);
    tab.resolve(d_tab);
    for (const CallTables::Segment &s : tab.segments) {
        if (s.off == CallTables::ABSENT || s.bytes == 0) continue;
        if (!s.host) {
            MD_HIP(hipMemsetAsync(d_tab + s.off, 0, s.bytes, ctx->stream));
        } else if (int rc = mdhip_h2d_small(ctx, d_tab + s.off, s.host, s.bytes)) {
            return rc;
        }
    }
    return MDHIP_OK;
}

}  // namespace
#endif  // __HIPCC__
