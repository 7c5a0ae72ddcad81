// Helpers shared by the mesh units (simplify, raycast, closest, inside, audit, weld, smooth, sample, intersect) and the lattice units
// (components, band, surface): ONE definition of the block-table bisection, the by-value vertex classes, the lock-free union-find and
// its termination argument, and of the small arithmetic and host helpers that every unit needs.  Device helpers are force-inlined
// functions over plain pointers.
//
// What is NOT here, and why.  Every helper was admitted only where the unit's device code compiles to the instructions it had before.
// A helper that takes a LOOP out of a kernel's body does not pass: the compiler simplifies a function before it inlines it, the loop
// reaches the kernel in another shape, and the schedule and the register allocation of the kernel come out differently.  So these
// stay written out in their kernels:
//   the serial loop that clamps the offsets and builds the block tables   k_audit_init, k_weld_init, k_smooth_init, k_simplify_groups,
//                                                                         k_raycast_groups, k_sample_init, k_intersect_groups
//   the probe loops of the vertex table (insertion, lookup)               k_audit_weld / k_audit_lookup, k_weld_insert / k_weld_lookup
//   the scan of the block sums in chunks of 256 with a carry              k_weld_scan, k_smooth_scan
//   the bisection written into a kernel's body                            k_raycast_bin, k_intersect_walk
// The rules they follow are stated here once, beside the helpers they use.
#pragma once
#include "pr_common.h"

namespace pr {

// ---------------------------------------------------------------------------------------------
// Arithmetic with every operation rounded on its own (the headers' rules are stated this way)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mesh_finite(float x) { return __fsub_rn(x, x) == 0.f; }      // (false for an infinity and for a NaN)

__device__ __forceinline__ float mesh_dot(const float* x, const float* y) {
    return __fadd_rn(__fadd_rn(__fmul_rn(x[0], y[0]), __fmul_rn(x[1], y[1])), __fmul_rn(x[2], y[2]));
}
__device__ __forceinline__ void mesh_cross(const float* x, const float* y, float* out) {
    out[0] = __fsub_rn(__fmul_rn(x[1], y[2]), __fmul_rn(x[2], y[1]));
    out[1] = __fsub_rn(__fmul_rn(x[2], y[0]), __fmul_rn(x[0], y[2]));
    out[2] = __fsub_rn(__fmul_rn(x[0], y[1]), __fmul_rn(x[1], y[0]));
}
// equal as VALUES: -0 equals +0, a NaN equals nothing
__device__ __forceinline__ bool mesh_same(const float* x, const float* y) { return x[0] == y[0] && x[1] == y[1] && x[2] == y[2]; }

// ---------------------------------------------------------------------------------------------
// Groups: clamped offsets, block tables, the lane of a block
// ---------------------------------------------------------------------------------------------
// The group sizes live on the device, so the vertex and triangle grids are the host's upper bounds ceil(V / 256) + G and
// ceil(T / 256) + G; 256-lane blocks never span two groups, a block finds its group by bisection of the block table, and the blocks
// behind the last group find none.  The tables are built by one lane, serial over the groups (a handful): offsets that leave
// [0, total] or decrease are CLAMPED, so that no later kernel follows a bad offset out of an array; the block table is the running sum
// of ceil(size / 256).
struct MeshLane {
    int group;                    // -1: the block lies behind the last group
    int first, size;              // the group's first row and its rows
    int local;                    // row inside the group
    bool live;
};

// the lane of block `b` of a vertex or triangle grid: `blk` / `first` are the block table and the clamped offsets of that kind
__device__ __forceinline__ MeshLane mesh_lane(int groups, const int32_t* blk, const int32_t* first, int b) {
    MeshLane l;
    const PR_GLOBAL_AS int32_t* table = as_global(blk);
    l.group = -1;
    l.first = l.size = l.local = 0;
    l.live = false;
    if (b >= table[groups]) return l;
    int lo = 0, hi = groups;                  // table[lo] <= b < table[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] <= b) lo = mid;
        else hi = mid;
    }
    l.group = lo;
    l.first = as_global(first)[lo];
    l.size = as_global(first)[lo + 1] - l.first;
    l.local = (b - table[lo]) * 256 + (int)threadIdx.x;
    l.live = l.local < l.size;
    return l;
}

struct MeshCorners {
    int i[3];
    bool in_range;                // three indices in [0, vsize)
};

// the corners of triangle `local` of the group whose triangles start at row `tfirst`; the indices are checked here
__device__ __forceinline__ MeshCorners mesh_corners(const int32_t* triangles, int tfirst, int local, int vsize) {
    MeshCorners c;
    const PR_GLOBAL_AS int32_t* t = as_global(triangles) + ((size_t)tfirst + local) * 3;
    c.i[0] = t[0];
    c.i[1] = t[1];
    c.i[2] = t[2];
    c.in_range = c.i[0] >= 0 && c.i[0] < vsize && c.i[1] >= 0 && c.i[1] < vsize && c.i[2] >= 0 && c.i[2] < vsize;
    return c;
}

// ---------------------------------------------------------------------------------------------
// The by-value vertex table: one class per set of vertices with equal VALUES (pr_mesh_audit and pr_mesh_weld must agree on it)
// ---------------------------------------------------------------------------------------------
// Per group an open-addressing table of 2 V_g slots - group g owns [2 vfirst[g], 2 vfirst[g + 1]) of the slot array -, keyed by the
// three values of a vertex; a slot holds a vertex index local to the group.  A slot only ever moves to a lower index with the SAME
// values, so a 32-bit word stands for the 96-bit key, and after the insertion kernel every class's slot holds its lowest index: the
// representative.  Integer atomics only; no lane ever waits for another.  A vertex with a component that is not finite has no class.
// The insertion (compare-and-swap on an empty slot, else an atomic minimum on the class's slot) and the lookup (the content of the
// class's slot, read by a later kernel) walk the same probe sequence: from mesh_vertex's slot on, one slot at a time, around the
// region.  TERMINATION: a walk ends at an empty slot or at the class, after at most the region's size: 2 V_g slots hold at most V_g
// classes, so an empty slot always exists.  Which vertices form a class is decided by mesh_vertex and mesh_same_values alone.
constexpr int MESH_EMPTY_VERTEX = 0x7FFFFFFF;              // above every vertex index: an atomic minimum can only lower a slot

struct MeshVertex {
    float x[3];
    bool finite;
    unsigned int at;              // first slot of the probe sequence (local to the group's region)
};

// the values of vertex `row` and the start of its probe sequence in a region of `size` slots; -0 hashes as +0 (they compare equal)
__device__ __forceinline__ MeshVertex mesh_vertex(const float* vertices, size_t row, unsigned int size) {
    MeshVertex v;
    unsigned int bits[3];
    v.finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v.x[a] = as_global(vertices)[row * 3 + a];
        v.finite = v.finite && mesh_finite(v.x[a]);
        bits[a] = v.x[a] == 0.f ? 0u : __float_as_uint(v.x[a]);
    }
    const unsigned long long h = noise_mix(noise_mix((unsigned long long)bits[0] | (unsigned long long)bits[1] << 32) ^ bits[2]);
    v.at = size ? (unsigned int)(h % size) : 0u;
    return v;
}

// whether vertex `index` (local, read from a slot: checked here) of the group that starts at row `first` has the values of `v`
__device__ __forceinline__ bool mesh_same_values(const float* vertices, int first, int size, int index, const MeshVertex& v) {
    if ((unsigned)index >= (unsigned)size) return false;
    const PR_GLOBAL_AS float* o = as_global(vertices) + ((size_t)first + index) * 3;
    return o[0] == v.x[0] && o[1] == v.x[1] && o[2] == v.x[2];
}

// ---------------------------------------------------------------------------------------------
// Lock-free union-find over one int32 parent per element: a negative value is no element, a root points at itself
// ---------------------------------------------------------------------------------------------
// TERMINATION.  No lane ever waits for another lane's progress: there is no spin, no lock and no flag.  The only writes to a parent
// array are its initialisation (a value <= the element's own index), the atomic minima of mesh_uf_unite and the store of a root found
// by a walk, so a slot only ever decreases, stays <= its own index, and a value read from it - however stale - is an ancestor of the
// element in some earlier forest: never a wrong set, at worst a longer walk.  Every loop strictly decreases a non-negative integer:
//   mesh_uf_find    x -> parent[x] < x until parent[x] == x: at most x steps.
//   mesh_uf_unite   each round ends or replaces the larger of (a, b) by a strictly smaller index (the parent somebody else gave it
//                   first) and walks down from there: a + b falls every round, so at most a + b rounds.  Going on with the returned
//                   parent - not giving up - is what keeps the link that parent stood for.
// (reads that race with the atomics of a uniting kernel go to the coherent level)
__device__ __forceinline__ int mesh_uf_parent(const PR_GLOBAL_AS int32_t* slot) {
    return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int mesh_uf_find(const PR_GLOBAL_AS int32_t* parent, int x) {
    // x strictly falls; the unsigned comparison also ends the walk on a negative value, which no element's chain holds
    for (int up = mesh_uf_parent(parent + x); (unsigned)up < (unsigned)x; up = mesh_uf_parent(parent + x)) x = up;
    return x;
}

__device__ __forceinline__ void mesh_uf_unite(PR_GLOBAL_AS int32_t* parent, int a, int b) {
    a = mesh_uf_find(parent, a);
    b = mesh_uf_find(parent, b);
    while (a != b) {                               // a + b strictly falls
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int was = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (was == a) return;                      // a was a root and now hangs under b
        a = mesh_uf_find(parent, was);             // was < a: somebody re-parented a first - that parent must meet b too
        b = mesh_uf_find(parent, b);
    }
}

// ---------------------------------------------------------------------------------------------
// Host: workspace plans and checks
// ---------------------------------------------------------------------------------------------
// the next region of a workspace plan: `bytes` from *at on, every region 256-byte aligned
static inline size_t workspace_region(size_t* at, size_t bytes) {
    const size_t begin = *at;
    *at += (bytes + 255) / 256 * 256;
    return begin;
}

static inline bool host_finite(float x) { return x - x == 0.f; }

// the checks of a caller's workspace, in this order; `who` names the entry point
static inline int check_workspace(const char* who, void* workspace, size_t given, size_t needed) {
    PR_REQUIRE(workspace != nullptr, "%s: NULL workspace", who);
    PR_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    if (given < needed) {
        set_error("workspace too small: %zu bytes given, %zu needed", given, needed);
        return PR_ERR_INVALID;
    }
    return PR_OK;
}

}  // namespace pr
