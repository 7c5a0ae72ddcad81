// Connected components of density lattices (pr_label_components, include/playrender.h): the inside set {sigma > level} under the
// 14-neighbourhood of the seven Freudenthal edge directions pr_extract_surface places vertices on, labelled by the smallest flat
// index of each component, measured, ranked and blanked out - floater removal and capping for the mesh and the occupancy bits.
//
// A lock-free union-find over one int32 parent per point (`label`: -1 outside, else an index <= the point's own; a root points
// at itself).  4 + keep_largest launches on the caller's stream, all kernels:
//   k_components_init     label = head of the point's z-run inside its block, size = 0; zeroes counts and the rank winners
//   k_components_merge    unites every point with its inside neighbours (atomic minimum into the larger root's slot)
//   k_components_flatten  label = root, size[root] += 1 (summed per wave and block first), counts[0..1]
//   k_components_select   one per rank r < keep_largest: 64-bit atomic maximum of (size << 32 | ~label) below rank r - 1's winner
//   k_components_write    labels, sizes, sigma_out, counts[2..3]
// Lanes: one per lattice point, 256-lane blocks that never span two groups.  Integer atomics only: every output is deterministic.
//
// TERMINATION.  No lane ever waits for another lane's progress: there is no spin, no lock and no flag in this file.  The union-find
// is mesh_uf_find / mesh_uf_unite (mesh_dev.h, which holds their termination argument); its premise holds here: the only writes to
// `label` are the init kernel's (the head of a run: <= the point's own index), atomic minima (merge) and the store of a root found by
// a walk (flatten).  The wave sum of k_components_flatten retires at least one pending lane per pass and is bounded by 64 passes as
// written.
#include "mesh_dev.h"

namespace pr {

constexpr unsigned COMPONENTS_DX = 0x59, COMPONENTS_DY = 0x6A, COMPONENTS_DZ = 0x74;     // bit d: direction d steps along the axis
constexpr int COMPONENTS_MAX_RANKS = 8;          // keep_largest <= 8: one launch per rank

struct ComponentsParams {
    int groups, nx, ny, nz;
    int points;                   // P = nx ny nz
    int blocks;                   // blocks per group, ceil(P / 256)
    float level, fill;
    int close_border, min_points, keep_largest;
    const float* sigma;           // (G, P)
    int32_t* labels; int32_t* sizes; float* sigma_out;     // (G, P) each, or NULL
    int32_t* counts;              // (G, 4) inside points, components, kept components, kept points: zeroed by init, then summed
    // workspace
    int32_t* label;               // (G, P) parent, at the end root, local to the group; -1 outside
    int32_t* size;                // (G, P) points of the component, at its root
    unsigned long long* winners;  // (G, 8) key of the component of rank r, 0 = there is none
};

struct ComponentsLane {
    int group, p, i, j, k;
    bool live, border;
};

__device__ __forceinline__ ComponentsLane components_lane(const ComponentsParams& c) {
    ComponentsLane l;
    l.group = (int)blockIdx.x / c.blocks;
    l.p = ((int)blockIdx.x - l.group * c.blocks) * 256 + (int)threadIdx.x;
    l.live = l.p < c.points;
    const int q = l.live ? l.p : 0;
    l.k = q % c.nz;
    l.j = (q / c.nz) % c.ny;
    l.i = q / (c.nz * c.ny);
    l.border = l.i == 0 || l.i == c.nx - 1 || l.j == 0 || l.j == c.ny - 1 || l.k == 0 || l.k == c.nz - 1;
    return l;
}

// ranking key of a component: larger first; size descending, ties by label ascending.  Never 0 (size >= 1).
__device__ __forceinline__ unsigned long long components_key(int size, int label) {
    return (unsigned long long)(unsigned)size << 32 | (unsigned)~label;
}

__device__ __forceinline__ bool components_kept(const ComponentsParams& c, int group, int size, int label) {
    if (size < c.min_points) return false;
    if (c.keep_largest == 0) return true;
    return components_key(size, label) >= as_global(c.winners)[(size_t)group * COMPONENTS_MAX_RANKS + c.keep_largest - 1];
}

// inclusive maximum scan over the 256 threads of a block.  lds: >= 4 ints.
__device__ __forceinline__ int components_block_max_scan(int v, int* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, o);
    }
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v = max(v, lds[w]);
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(256) void k_components_init(ComponentsParams c) {
    __shared__ int lds[4];
    __shared__ unsigned char inside_of[256];
    const ComponentsLane l = components_lane(c);
    const size_t at = (size_t)l.group * c.points + (l.live ? l.p : 0);
    bool inside = false;
    if (l.live) inside = as_global(c.sigma)[at] > c.level && !(c.close_border && l.border);
    inside_of[threadIdx.x] = inside ? 1 : 0;
    __syncthreads();
    // a point whose backward z neighbour is an inside lane of this block starts under the head of that run (a smaller index)
    const bool joined = inside && l.k > 0 && threadIdx.x > 0 && inside_of[threadIdx.x - 1];
    const int head = components_block_max_scan(inside && !joined ? l.p : -1, lds);
    if (l.live) {
        as_global(c.label)[at] = inside ? head : -1;
        as_global(c.size)[at] = 0;
    }
    if ((int)blockIdx.x == l.group * c.blocks) {
        if (threadIdx.x < 4) as_global(c.counts)[(size_t)l.group * 4 + threadIdx.x] = 0;
        if (threadIdx.x < COMPONENTS_MAX_RANKS) as_global(c.winners)[(size_t)l.group * COMPONENTS_MAX_RANKS + threadIdx.x] = 0ull;
    }
}

__global__ __launch_bounds__(256) void k_components_merge(ComponentsParams c) {
    const ComponentsLane l = components_lane(c);
    if (!l.live) return;
    PR_GLOBAL_AS int32_t* label = as_global(c.label) + (size_t)l.group * c.points;
    // (inside <=> label >= 0, which no kernel after init changes: plain reads)
    if (label[l.p] < 0) return;
    const bool back = l.k > 0 && label[l.p - 1] >= 0;
    if (back && threadIdx.x == 0) mesh_uf_unite(label, l.p, l.p - 1);      // the z edge into the previous block
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        if (d == 2) continue;                      // z: the init kernel's runs and the line above
        const int di = COMPONENTS_DX >> d & 1, dj = COMPONENTS_DY >> d & 1, dk = COMPONENTS_DZ >> d & 1;
        if (l.i + di >= c.nx || l.j + dj >= c.ny || l.k + dk >= c.nz) continue;
        const int q = l.p + (di * c.ny + dj) * c.nz + dk;
        if (label[q] < 0) continue;
        // both backward z neighbours inside: p ~ p - 1 and q ~ q - 1 along z, and lane p - 1 unites p - 1 with q - 1 (or defers
        // the same way, down to the start of the run)
        if (back && label[q - 1] >= 0) continue;
        mesh_uf_unite(label, l.p, q);
    }
}

__global__ __launch_bounds__(256) void k_components_flatten(ComponentsParams c) {
    __shared__ int lds[4];
    __shared__ int block_root, block_sum;
    const ComponentsLane l = components_lane(c);
    PR_GLOBAL_AS int32_t* label = as_global(c.label) + (size_t)l.group * c.points;
    PR_GLOBAL_AS int32_t* size = as_global(c.size) + (size_t)l.group * c.points;
    int root = -1;
    if (l.live && label[l.p] >= 0) {
        root = mesh_uf_find(label, l.p);        // (no unions in this kernel: the roots are final)
        label[l.p] = root;
    }
    if (threadIdx.x == 0) {
        block_root = -1;
        block_sum = 0;
    }
    __syncthreads();
    if (root >= 0) atomicMax(&block_root, root);   // one root of the block is summed in LDS, the common case of a large component
    __syncthreads();
    const int shared_root = block_root;
    const int lane = threadIdx.x & 63;
    int pending = root;
    for (int pass = 0; pass < 64; ++pass) {        // every pass retires the lanes that share the first pending lane's root
        const unsigned long long todo = __ballot(pending >= 0);
        if (!todo) break;
        const int first = __ffsll((long long)todo) - 1;
        const int r = __shfl(pending, first, 64);
        const unsigned long long same = __ballot(pending == r);
        if (lane == first) {
            if (r == shared_root) atomicAdd(&block_sum, __popcll(same));
            else __hip_atomic_fetch_add(size + r, __popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (pending == r) pending = -1;
    }
    int inside_total, root_total;
    block_exclusive_scan_256(root >= 0 ? 1 : 0, lds, &inside_total);
    block_exclusive_scan_256(root >= 0 && root == l.p ? 1 : 0, lds, &root_total);     // (the barriers inside also order block_sum)
    if (threadIdx.x == 0 && inside_total) {
        PR_GLOBAL_AS int32_t* counts = as_global(c.counts) + (size_t)l.group * 4;
        __hip_atomic_fetch_add(size + shared_root, block_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(counts + 0, inside_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (root_total) __hip_atomic_fetch_add(counts + 1, root_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_components_select(ComponentsParams c, int rank) {
    __shared__ unsigned long long best_of[4];
    const ComponentsLane l = components_lane(c);
    PR_GLOBAL_AS unsigned long long* winners = as_global(c.winners) + (size_t)l.group * COMPONENTS_MAX_RANKS;
    const unsigned long long below = rank ? winners[rank - 1] : ~0ull;         // 0: there is no component of rank - 1
    unsigned long long key = 0;
    if (l.live && below) {
        const size_t at = (size_t)l.group * c.points + l.p;
        if (as_global(c.label)[at] == l.p) {
            key = components_key(as_global(c.size)[at], l.p);
            if (key >= below) key = 0;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(key >> 32), d, 64), lo = (unsigned)__shfl_xor((int)key, d, 64);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0) best_of[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long best = best_of[0];
        for (int w = 1; w < 4; ++w) best = best_of[w] > best ? best_of[w] : best;
        if (best) __hip_atomic_fetch_max(winners + rank, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_components_write(ComponentsParams c) {
    __shared__ int lds[4];
    const ComponentsLane l = components_lane(c);
    const size_t first = (size_t)l.group * c.points;
    int label = -1, size = 0;
    bool kept = false;
    if (l.live) {
        label = as_global(c.label)[first + l.p];
        if (label >= 0) {
            size = as_global(c.size)[first + label];
            kept = components_kept(c, l.group, size, label);
        }
        if (c.labels) as_global(c.labels)[first + l.p] = label;
        if (c.sizes) as_global(c.sizes)[first + l.p] = size;
        if (c.sigma_out) {                         // (sigma_out may be sigma: a lane reads its own value before it writes it)
            const unsigned bits = as_global(reinterpret_cast<const unsigned*>(c.sigma))[first + l.p];
            const bool capped = c.close_border && l.border && __uint_as_float(bits) > c.level;
            as_global(reinterpret_cast<unsigned*>(c.sigma_out))[first + l.p] = (label >= 0 && !kept) || capped ? __float_as_uint(c.fill) : bits;
        }
    }
    int kept_roots, kept_points;
    block_exclusive_scan_256(kept && label == l.p ? 1 : 0, lds, &kept_roots);
    block_exclusive_scan_256(kept ? 1 : 0, lds, &kept_points);
    if (threadIdx.x == 0 && kept_points) {
        PR_GLOBAL_AS int32_t* counts = as_global(c.counts) + (size_t)l.group * 4;
        if (kept_roots) __hip_atomic_fetch_add(counts + 2, kept_roots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(counts + 3, kept_points, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct ComponentsPlan {
    size_t label, size, winners, bytes;
    int points, blocks;
};

// Host checks of both entry points: no device work.
static int plan_components(const pr_components_t* c, const char* who, ComponentsPlan* plan) {
    PR_REQUIRE(c != nullptr, "%s: NULL description", who);
    PR_REQUIRE(c->groups >= 1, "%s: groups %d (>= 1)", who, c->groups);
    double total = (double)c->groups;
    long points = 1;
    for (int a = 0; a < 3; ++a) {
        PR_REQUIRE(c->points[a] >= 1, "%s: points[%d] = %d (>= 1)", who, a, c->points[a]);
        total *= (double)c->points[a];
        PR_REQUIRE(total < 2147483648.0, "%s: lattice too large: groups x points must stay below 2^31 (labels and sizes are int32)", who);
        points *= c->points[a];
    }
    PR_REQUIRE(c->level == c->level, "%s: level is NaN", who);
    PR_REQUIRE((c->flags & ~(uint32_t)PR_COMPONENTS_CLOSE_BORDER) == 0, "%s: flags 0x%x (unknown bits)", who, c->flags);
    PR_REQUIRE(c->keep_largest >= 0 && c->keep_largest <= PR_COMPONENTS_MAX_KEEP, "%s: keep_largest %d (0..%d)", who, c->keep_largest,
               PR_COMPONENTS_MAX_KEEP);
    PR_REQUIRE(c->min_points >= 0, "%s: min_points %d (>= 0)", who, c->min_points);
    PR_REQUIRE(c->sigma != nullptr, "%s: NULL sigma", who);
    PR_REQUIRE(c->counts != nullptr, "%s: NULL counts (counts is always written)", who);
    if (c->sigma_out) {
        PR_REQUIRE(c->fill <= c->level, "%s: fill %g must be <= level %g (and not NaN): a blanked point has to be outside", who,
                   (double)c->fill, (double)c->level);
        const uintptr_t in = (uintptr_t)c->sigma, out = (uintptr_t)c->sigma_out, bytes = (uintptr_t)(total * sizeof(float));
        PR_REQUIRE(in == out || in + bytes <= out || out + bytes <= in,
                   "%s: sigma_out overlaps sigma partially (in place - the same pointer - or disjoint)", who);
    }
    plan->points = (int)points;
    plan->blocks = (int)((points + 255) / 256);
    const size_t lattice = (size_t)c->groups * (size_t)points;
    size_t at = 0;
    plan->label = workspace_region(&at, lattice * sizeof(int32_t));
    plan->size = workspace_region(&at, lattice * sizeof(int32_t));
    plan->winners = workspace_region(&at, (size_t)c->groups * COMPONENTS_MAX_RANKS * sizeof(unsigned long long));
    plan->bytes = at;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_components_workspace_size(const pr_components_t* c, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_components_workspace_size: NULL bytes");
    pr::ComponentsPlan plan;
    PR_TRY(pr::plan_components(c, "pr_components_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_label_components(const pr_components_t* c, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    static_assert(COMPONENTS_MAX_RANKS == PR_COMPONENTS_MAX_KEEP, "one winner slot per rank");
    ComponentsPlan plan;
    PR_TRY(plan_components(c, "pr_label_components", &plan));
    PR_TRY(check_workspace("pr_label_components", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    ComponentsParams p;
    memset(&p, 0, sizeof(p));
    p.groups = c->groups;
    p.nx = c->points[0];
    p.ny = c->points[1];
    p.nz = c->points[2];
    p.points = plan.points;
    p.blocks = plan.blocks;
    p.level = c->level;
    p.fill = c->fill;
    p.close_border = (c->flags & PR_COMPONENTS_CLOSE_BORDER) ? 1 : 0;
    p.min_points = c->min_points;
    p.keep_largest = c->keep_largest;
    p.sigma = c->sigma;
    p.labels = c->labels;
    p.sizes = c->sizes;
    p.sigma_out = c->sigma_out;
    p.counts = c->counts;
    p.label = (int32_t*)(ws + plan.label);
    p.size = (int32_t*)(ws + plan.size);
    p.winners = (unsigned long long*)(ws + plan.winners);
    const unsigned grid = (unsigned)((long)c->groups * plan.blocks);
    hipLaunchKernelGGL(k_components_init, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_components_merge, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_components_flatten, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    for (int rank = 0; rank < c->keep_largest; ++rank) {
        hipLaunchKernelGGL(k_components_select, dim3(grid), dim3(256), 0, st, p, rank);
        PR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_components_write, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
