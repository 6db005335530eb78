// shell_gather.h — what the shell-search consumers with a candidate list of the caller's share between "the caller hands
// over a candidate list" and "the sweep of shell_search.h runs over it": the integer tables of a call packed into one
// upload (IntTable, upload_ints), the question whether the kernel has to look a hit's atom up at all (shares_an_atom),
// the candidates' coordinate planes (planes_room, gather_kernel, gather) and, at a hit, the self / same-molecule test
// (excluded) and the candidate's coordinates (cand_xyz). angles.hip, bond_order.hip, sdf.hip, aggregates.hip and
// hbonds.hip include this header in place of shell_search.h, behind their `#pragma clang fp contract(off)`. The host
// part is plain C++17 (no HIP header, no context), in the form of group_pairs.h: tests/native/shell_gather_main.cpp
// walks it with g++ under sanitizers; the rest is for hipcc only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace shell {

// ---- host part ------------------------------------------------------------------------------------------------------

// The integer tables of one call, packed back to back for one upload. The caller names its segments in order, each
// with the device pointer that is to point at it; resolve(base) sets those pointers once the table lies at `base`.
// Nobody computes an offset by hand.
struct IntTable {
    static constexpr size_t ABSENT = ~(size_t)0;
    std::vector<int32_t> host;      // the segments, in the order they were named
    std::vector<size_t> off;        // where each begins in `host`; ABSENT: an optional segment the caller left out
    std::vector<const int **> dev;  // what resolve() sets for it

    // n values from p; (nullptr, 0) is an empty segment: it takes no room, and its pointer is that of what follows
    void add(const int32_t *p, size_t n, const int **d)
    {
        off.push_back(host.size()), dev.push_back(d);
        if (n) host.insert(host.end(), p, p + n);
    }
    // an optional table (mol_of): without one (p == nullptr) the kernels get a null pointer
    void add_optional(const int32_t *p, size_t n, const int **d)
    {
        if (p) return add(p, n, d);
        off.push_back(ABSENT), dev.push_back(d);
    }
    // n values value(k), k = 0 .. n - 1 (node_of[atoms[k]], say)
    template <class Value>
    void add_generated(size_t n, Value value, const int **d)
    {
        off.push_back(host.size()), dev.push_back(d);
        host.reserve(host.size() + n);
        for (size_t k = 0; k < n; ++k) host.push_back(value(k));
    }
    void resolve(const int *base) const
    {
        for (size_t s = 0; s < off.size(); ++s) *dev[s] = off[s] == ABSENT ? nullptr : base + off[s];
    }
};

// Is an atom in both lists (indices in [0, n_atoms), checked by the caller)? Then a hit may be the centre itself, and
// the kernel has to look the candidate's atom up; most calls of distinct types need not.
inline bool shares_an_atom(int64_t n_atoms, const int32_t *a, int64_t n_a, const int32_t *b, int64_t n_b)
{
    if (n_a == 0 || n_b == 0) return false;
    std::vector<char> in_b((size_t)n_atoms, 0);
    for (int64_t k = 0; k < n_b; ++k) in_b[(size_t)b[k]] = 1;
    for (int64_t k = 0; k < n_a; ++k)
        if (in_b[(size_t)a[k]]) return true;
    return false;
}

}  // namespace shell

#ifdef __HIPCC__
#include "shell_search.h"

namespace shell {

// ---- device part ----------------------------------------------------------------------------------------------------

// One lane per (frame, candidate): the candidate planes [F][3][n_cand], so that the sweep reads coalesced planes of
// only the atoms that can be a neighbour.
static __global__ __launch_bounds__(256) void gather_kernel(const double *__restrict__ xyz, long long n,
                                                            const int *__restrict__ cand, long long n_cand,
                                                            long long total, double *__restrict__ planes)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long w = i % n_cand, f = i / n_cand;
        const long long a = cand[w];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            planes[((size_t)f * 3 + k) * (size_t)n_cand + w] = xyz[((size_t)f * 3 + k) * (size_t)n + a];
    }
}

// A hit on candidate atom aj is no neighbour of centre atom ci when it is the centre itself or, under exclusion
// (mol_of != nullptr), of the centre's molecule.
__device__ __forceinline__ bool excluded(int aj, int ci, const int *__restrict__ mol_of)
{
    return aj == ci || (mol_of && mol_of[aj] == mol_of[ci]);
}

// the coordinates of candidate a in frame f of the planes [F][3][n_cand]
struct Xyz {
    double x, y, z;
};
__device__ __forceinline__ Xyz cand_xyz(const double *__restrict__ planes, long long n_cand, long long f, long long a)
{
    const double *q = planes + (size_t)f * 3 * (size_t)n_cand;
    return {q[a], q[n_cand + a], q[2 * n_cand + a]};
}

// ---- host launch helpers --------------------------------------------------------------------------------------------

// the table on the device, in workspace `slot`, and its segments' pointers
inline int upload_ints(mdhip_ctx *ctx, const IntTable &tab, int slot)
{
    MD_WS(d_int, int, slot, tab.host.size() * 4);
    tab.resolve(d_int);
    return mdhip_h2d_small(ctx, d_int, tab.host.data(), tab.host.size() * 4);
}

// Room for the planes [n_frames][3][n_cand] (WS_AUX1). Apart from the launch: an entry point takes its workspace in an
// order of its own, ahead of its timers (a buffer that grows waits for the stream), and the hydrogen-bond lifetime
// sizes its pair table from what is free once the planes are in place.
inline int planes_room(mdhip_ctx *ctx, int64_t n_frames, int64_t n_cand, double *&planes)
{
    MD_WS(d_planes, double, WS_AUX1, (size_t)n_frames * 3 * (size_t)n_cand * 8);
    planes = d_planes;
    return MDHIP_OK;
}

// launches gather_kernel into that room (one launch, on the call's stream)
inline int gather(mdhip_ctx *ctx, const double *d_xyz, int64_t n_frames, int64_t n_atoms, const int *d_cand,
                  int64_t n_cand, double *planes)
{
    const size_t total = (size_t)n_frames * (size_t)n_cand;
    const unsigned ggrid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(gather_kernel, dim3(ggrid), dim3(256), 0, ctx->stream, d_xyz, (long long)n_atoms, d_cand,
                       (long long)n_cand, (long long)total, planes);
    MD_HIP(hipGetLastError());
    return MDHIP_OK;
}

}  // namespace shell
#endif  // __HIPCC__
