// aggregates.hip — connected components of the contact graph of structural/aggregates.py (calc_aggregates): which
// nodes (molecules, or atoms) hang together through contacts between listed atoms. The reference has no such function;
// the specification is in DESIGN.md (aggregates) and include/mdhip.h, restated in tests/aggregates_ref.py.
//
// One frame: atom i of list A (class class_a) and atom j of list B (class class_b) are in contact when
// node_of[i] != node_of[j] and shell::rsq(i, j) < rsq_cut[class_a][class_b] (strict; the |d| form of the single wrap;
// an entry <= 0 never links). Every contact makes the two nodes neighbours; label[node] is the smallest node of its
// connected component. Contraction is off in this file.
//
//  1. agg_init_kernel: parent[f][m] = m, one lane per (frame, node).
//  2. shell::gather_kernel (shell_gather.h): the planes [F][3][n_b] of the B atoms, so that the sweep reads coalesced
//     planes.
//  3. agg_union_kernel: the sweep of shell_search.h, A as centres against the B planes, with the largest table entry.
//     A hit (rare) is tested again against the cutoff of its class pair, skipped when both atoms are of one node,
//     counted (one 64-bit add to the frame's counter) and its two nodes united in the frame's parent row (agg_unite).
//  4. agg_flatten_kernel, after the sweep has ended: every node walks to its root and writes it as its label; the
//     roots are counted per frame, one add per wave and frame.
// Nothing is appended anywhere: no capacity, no overflow.

#include <algorithm>

#include "ctx.h"

#pragma clang fp contract(off)

#include "shell_gather.h"

namespace {

constexpr int AGG_MAX_CLASSES = 16;

__global__ __launch_bounds__(256) void agg_init_kernel(int *__restrict__ parent, long long n_nodes, long long total)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x)
        parent[i] = (int)(i % n_nodes);
}

// parent[x] as the memory side holds it (a relaxed agent-scope load goes past this CU's L1). A plain load would do:
// see agg_unite.
__device__ __forceinline__ int agg_parent(const int *parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Unites the trees of u and v in one frame's parent row while other lanes, waves and workgroups do the same.
//
// Invariant: parent[x] <= x for every x, always, and parent[x] changes at most once in a launch: from x (a root) to a
// smaller index, by a compare-and-swap that expects x and executes at the memory side. Nothing else writes the row
// during the sweep: no path compression, no plain store.
//   - Every chain x, parent[x], parent[parent[x]], ... strictly decreases until it meets an entry that points to
//     itself, so there is no cycle and a walk takes at most x steps.
//   - What a load of parent[x] can return is x or the one value it was swapped to. A stale copy (this CU's L1 and the
//     L2 of its XCD are not refreshed by another CU's swap) can only say x, "still a root". The walk then ends at a
//     node that is no longer a root — but it is of the same component as the node the walk began at, and it is the
//     compare-and-swap, not the load, that decides: it succeeds only if parent[hi] really is hi.
//   - A successful swap hooks the root hi under lo < hi, and lo is of v's (or u's) component: the link is a correct
//     union whether or not lo is still a root, and the invariant holds.
//   - A failed swap returns the true parent of hi, which is smaller than hi. The loop goes on from that value in place
//     of hi: the pair (a, b) it carries only ever moves down the two chains, a + b strictly decreases with every failed
//     swap and is bounded by 0, so the loop ends; every iteration is a bounded walk and one swap.
//   - No lane waits for a store of another lane: no lock, no flag, no fence; lanes of one wave may diverge freely.
// Roots are only ever hooked under smaller indices, so when the launch has ended the root of every tree is the
// smallest index of its component.
__device__ __forceinline__ void agg_unite(int *parent, int u, int v)
{
    int a = u, b = v;
    for (;;) {
        for (int p; (p = agg_parent(parent, a)) != a;) a = p;
        for (int p; (p = agg_parent(parent, b)) != b;) b = p;
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int was = atomicCAS(&parent[hi], hi, lo);  // (device scope)
        if (was == hi) return;
        a = was;  // the true parent of hi (< hi); the other end stays
        b = lo;
    }
}

// The per-call tables of the union sweep, on the device.
struct AggTables {
    const int *class_a, *node_a;  // [n_a]: by position in A (the sweep's centre index)
    const int *class_b, *node_b;  // [n_b]: by position in B (the sweep's candidate index)
    const double *rsq_cut;        // [n_ca][n_cb]
    int n_cb;
};

__global__ __launch_bounds__(shell::THREADS) void agg_union_kernel(
    const double *__restrict__ xyz, long long n, const double *__restrict__ planes, long long n_b,
    const double *__restrict__ box, const int *__restrict__ atoms_a, int n_a, AggTables t, double rc2, shell::Grid g,
    long long n_nodes, int *parent, unsigned long long *__restrict__ contacts)
{
    shell::sweep(xyz, n, atoms_a, n_a, planes, 3, n_b, box, rc2, g, [=](const shell::Row &r, size_t, long long b) {
        const int na = t.node_a[r.c], nb = t.node_b[b];
        if (na == nb) return;
        const double cut = t.rsq_cut[t.class_a[r.c] * t.n_cb + t.class_b[b]];
        const shell::Xyz p = shell::cand_xyz(planes, n_b, r.f, b);
        if (!(shell::rsq(r.cx, r.cy, r.cz, p.x, p.y, p.z, r.Lx, r.Ly, r.Lz) < cut)) return;
        atomicAdd(&contacts[r.f], 1ull);
        agg_unite(parent + (size_t)r.f * (size_t)n_nodes, na, nb);
    });
}

// label[f][m] = the root of m in the finished parent rows (plain loads: the sweep's launch has ended), and
// n_components[f] = the number of roots: the lanes of a wave that hold roots of one frame add once.
__global__ __launch_bounds__(256) void agg_flatten_kernel(const int *__restrict__ parent, long long n_nodes,
                                                          long long total, int *__restrict__ label,
                                                          int *__restrict__ n_components)
{
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * blockDim.x; base < total; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        long long f = -1;
        bool root = false;
        if (i < total) {
            f = i / n_nodes;
            const int m = (int)(i - f * n_nodes);
            const int *row = parent + (size_t)f * (size_t)n_nodes;
            int x = m;
            for (int p; (p = row[x]) != x;) x = p;
            label[i] = x;
            root = x == m;
        }
        for (;;) {  // (wave-uniform: every lane of the wave is here, whatever its i)
            const unsigned long long open = __ballot(root);
            if (!open) break;
            const int leader = __ffsll((unsigned long long)open) - 1;
            const long long lf = __shfl(f, leader);
            const bool mine = root && f == lf;
            const unsigned long long same = __ballot(mine);
            if (lane == leader) atomicAdd(&n_components[lf], __popcll(same));
            if (mine) root = false;
        }
    }
}

}  // namespace

extern "C" {

int mdhip_contact_components(mdhip_ctx *ctx, int64_t n_frames, int64_t n_atoms, const double *xyz, int xyz_on_device,
                             const double *box, int32_t n_a, const int32_t *atoms_a, const int32_t *class_a,
                             int32_t n_b, const int32_t *atoms_b, const int32_t *class_b, int32_t n_ca, int32_t n_cb,
                             const double *rsq_cut, int64_t n_nodes, const int32_t *node_of, int32_t *label,
                             int32_t *n_components, uint64_t *n_contacts)
{
    if (!ctx) return MDHIP_EINVAL;
    CallScope cs(ctx);
    MD_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_a >= 0 && n_b >= 0 && n_nodes >= 0, "negative sizes");
    MD_REQUIRE(n_ca >= 1 && n_ca <= AGG_MAX_CLASSES && n_cb >= 1 && n_cb <= AGG_MAX_CLASSES,
               "n_ca and n_cb must be in [1, %d]", AGG_MAX_CLASSES);
    MD_REQUIRE(n_nodes < (1ll << 31), "at most 2^31 - 1 nodes");
    MD_REQUIRE(rsq_cut, "NULL array");
    double rc2 = 0.0;
    for (int k = 0; k < n_ca * n_cb; ++k) rc2 = std::max(rc2, rsq_cut[k]);
    MD_REQUIRE(rc2 > 0.0, "rsq_cut holds no positive cutoff");
    if (n_frames == 0) return cs.end();
    MD_REQUIRE(n_components && n_contacts, "NULL array");
    MD_REQUIRE(label || n_nodes == 0, "NULL array");
    MD_REQUIRE((atoms_a && class_a) || n_a == 0, "NULL array");
    MD_REQUIRE((atoms_b && class_b) || n_b == 0, "NULL array");
    MD_REQUIRE(node_of || (n_a == 0 && n_b == 0), "NULL array");
    memset(n_components, 0, (size_t)n_frames * 4);
    memset(n_contacts, 0, (size_t)n_frames * 8);
    if (n_nodes == 0) {
        MD_REQUIRE(n_a == 0 && n_b == 0, "listed atoms without nodes");
        return cs.end();
    }
    int rc;
    if ((rc = shell::check_indices(ctx, "A atom", n_a, atoms_a, 1, n_atoms))) return rc;
    if ((rc = shell::check_indices(ctx, "B atom", n_b, atoms_b, 1, n_atoms))) return rc;
    for (int32_t k = 0; k < n_a; ++k) {
        MD_REQUIRE(class_a[k] >= 0 && class_a[k] < n_ca, "A atom %d: class %d out of range", (int)k, (int)class_a[k]);
        const int32_t m = node_of[atoms_a[k]];
        MD_REQUIRE(m >= 0 && m < n_nodes, "A atom %d: node %d out of range", (int)k, (int)m);
    }
    for (int32_t k = 0; k < n_b; ++k) {
        MD_REQUIRE(class_b[k] >= 0 && class_b[k] < n_cb, "B atom %d: class %d out of range", (int)k, (int)class_b[k]);
        const int32_t m = node_of[atoms_b[k]];
        MD_REQUIRE(m >= 0 && m < n_nodes, "B atom %d: node %d out of range", (int)k, (int)m);
    }

    MD_HIP(hipSetDevice(ctx->device));
    const size_t n_lab = (size_t)n_frames * (size_t)n_nodes;
    MD_WS(d_parent, int, WS_OUT, n_lab * 4);
    MD_WS(d_label, int, WS_OUT2, n_lab * 4);
    MD_WS(d_ncomp, int, WS_AUX0, (size_t)n_frames * 4);
    MD_WS(d_contacts, unsigned long long, WS_HIST, (size_t)n_frames * 8);
    MD_HIP(hipMemsetAsync(d_ncomp, 0, (size_t)n_frames * 4, ctx->stream));
    MD_HIP(hipMemsetAsync(d_contacts, 0, (size_t)n_frames * 8, ctx->stream));
    const bool pairs = n_a > 0 && n_b > 0;  // (else no contact: every node is its own label)

    // the coordinates, and the tables: ints class_a | node_a [n_a], the B atoms | class_b | node_b [n_b]; doubles rsq_cut
    shell::Inputs in;
    AggTables t{};
    const int *d_atoms_b = nullptr;
    double *d_planes = nullptr;
    if (pairs) {
        if ((rc = shell::stage(ctx, "A atom", n_frames, n_atoms, xyz, xyz_on_device, box, n_a, atoms_a, in)))
            return rc;
        shell::IntTable ints;
        ints.add(class_a, n_a, &t.class_a);
        ints.add_generated(n_a, [&](size_t k) { return node_of[atoms_a[k]]; }, &t.node_a);
        ints.add(atoms_b, n_b, &d_atoms_b);
        ints.add(class_b, n_b, &t.class_b);
        ints.add_generated(n_b, [&](size_t k) { return node_of[atoms_b[k]]; }, &t.node_b);
        if ((rc = shell::upload_ints(ctx, ints, WS_TYPE_J))) return rc;
        MD_WS(d_cut, double, WS_TABLES, (size_t)n_ca * n_cb * 8);
        if ((rc = mdhip_h2d_small(ctx, d_cut, rsq_cut, (size_t)n_ca * n_cb * 8))) return rc;
        if ((rc = shell::planes_room(ctx, n_frames, n_b, d_planes))) return rc;
        t.rsq_cut = d_cut, t.n_cb = (int)n_cb;
    }

    KernelTimer timer(ctx, pairs ? 4 : 2);
    ctx->last_kernel = "agg_union_kernel";
    const unsigned lgrid = (unsigned)std::min<size_t>((n_lab + 255) / 256, (size_t)ctx->cu_count * 32);
    hipLaunchKernelGGL(agg_init_kernel, dim3(lgrid), dim3(256), 0, ctx->stream, d_parent, (long long)n_nodes,
                       (long long)n_lab);
    MD_HIP(hipGetLastError());
    KernelTimer search(ctx, 2, true);  // the gather and the union sweep: the call's aux time
    if (pairs) {
        if ((rc = shell::gather(ctx, in.xyz, n_frames, n_atoms, d_atoms_b, n_b, d_planes))) return rc;
        const shell::Grid g = shell::sweep_grid(ctx, n_frames, n_a, n_b);
        hipLaunchKernelGGL(agg_union_kernel, dim3(g.grid), dim3(shell::THREADS), 0, ctx->stream, in.xyz,
                           (long long)n_atoms, d_planes, (long long)n_b, in.box, in.centres, (int)n_a, t, rc2, g,
                           (long long)n_nodes, d_parent, d_contacts);
        MD_HIP(hipGetLastError());
    }
    search.stop();
    hipLaunchKernelGGL(agg_flatten_kernel, dim3(lgrid), dim3(256), 0, ctx->stream, d_parent, (long long)n_nodes,
                       (long long)n_lab, d_label, d_ncomp);
    MD_HIP(hipGetLastError());
    timer.stop();
    if ((rc = mdhip_result(cs, label, d_label, n_lab * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, n_components, d_ncomp, (size_t)n_frames * 4, 0))) return rc;
    if ((rc = mdhip_result(cs, n_contacts, d_contacts, (size_t)n_frames * 8, 0))) return rc;
    return shell::finish(cs, timer, &search);
}

}  // extern "C"
