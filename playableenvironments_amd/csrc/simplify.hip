// Simplification of extracted meshes by vertex clustering on a uniform grid (pr_simplify_mesh, include/playrender.h states the rule).
//
// Twelve launches on the caller's stream, all kernels:
//   k_simplify_init       zeroes the cluster sums and the counts, empties the duplicate table
//   k_simplify_groups     one lane: the clamped per-group offsets and the first vertex / triangle block of every group
//   k_simplify_cluster    per vertex: its cell; per run of equal cells in a wave: 64-bit integer atomics into the dense
//                         per-(group, cell) sums
//   k_simplify_mark       per cell: occupied?  block sums                       -> k_scan_blocks_group
//   k_simplify_vertices   per cell: output index (replaces the member count), position, normal
//   k_simplify_map        per vertex: cell -> output index (workspace and vertex_map)
//   k_simplify_triangles  per triangle: map, test, rotate; insert the 63-bit key into the group's open-addressing table
//                         (compare-and-swap on the key word, then an atomic minimum of the triangle's row on the slot)
//   k_simplify_survivors  per triangle: does it hold its key's minimum?  block sums   -> k_scan_blocks_group
//   k_simplify_offsets    per group: both output offsets and the two counts that are differences of them
//   k_simplify_emit       per triangle: the survivors, in input order (not launched without out_triangles)
// Lanes: one per element, 256-lane blocks that never span two groups.  The group sizes live on the device, so the vertex and triangle
// grids are the host's upper bounds ceil(V / 256) + G and ceil(T / 256) + G; a block finds its group by bisection of the block table
// (mesh_lane, mesh_dev.h) and the blocks behind the last group only report a zero sum.  Integer atomics only.  No lane ever waits for another: an insertion
// probes at most the 2 T_g slots of its group's region, which hold at most T_g keys.
#include "mesh_dev.h"

#include <math.h>

namespace pr {

constexpr unsigned long long SIMPLIFY_EMPTY = ~0ull;       // (a key has 63 bits)
constexpr int SIMPLIFY_NO_TRIANGLE = 0x7FFFFFFF;

struct SimplifyParams {
    int groups, V, T, keep;
    float origin[3], cell[3];
    int cells[3];
    int C, D;                     // cells per group, blocks of 256 cells per group
    int BV, BT;                   // launched vertex / triangle blocks
    int max_vertices, max_triangles;
    const float* vertices; const float* normals; const int32_t* triangles;
    const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    float* out_vertices; float* out_normals; int32_t* out_triangles; int32_t* vertex_map;
    int32_t* counts; int32_t* out_vertex_offsets; int32_t* out_triangle_offsets;
    // workspace
    int32_t* cnt;                 // (G, C) members of the cell, then (k_simplify_vertices) its output index local to the group or -1
    unsigned long long* fsum;     // (G, C, 3) sums of f (two's complement is irrelevant: f >= 0)
    unsigned long long* nsum;     // (G, C, 3) sums of the quantised normal components, two's complement; NULL without normals
    int32_t* vmap;                // (V) cell of the vertex, then (k_simplify_map) its output index
    int32_t* tslot;               // (T) table slot of the triangle's key, 0 with KEEP_DUPLICATES, -1: dropped
    unsigned long long* keys;     // (2 T) group g owns the slots [2 tfirst[g], 2 tfirst[g + 1])
    int32_t* tmin;                // (2 T) lowest row with the slot's key
    int32_t* vfirst; int32_t* tfirst;   // (G + 1) the offsets, clamped
    int32_t* vblk; int32_t* tblk;       // (G + 1) first block of the group
    int32_t* csum; int32_t* coff;       // (G D)
    int32_t* tsum; int32_t* toff;       // (BT)
    int32_t* totals;              // [clusters, output triangles]
};

__global__ __launch_bounds__(256) void k_simplify_init(SimplifyParams s) {
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t cells = (size_t)s.groups * s.C, slots = 2 * (size_t)s.T, counts = 4 * (size_t)s.groups;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += stride) {
        as_global(s.cnt)[i] = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) as_global(s.fsum)[3 * i + a] = 0ull;
        if (s.nsum) {
#pragma unroll
            for (int a = 0; a < 3; ++a) as_global(s.nsum)[3 * i + a] = 0ull;
        }
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += stride) {
        as_global(s.keys)[i] = SIMPLIFY_EMPTY;
        as_global(s.tmin)[i] = SIMPLIFY_NO_TRIANGLE;
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < counts; i += stride) as_global(s.counts)[i] = 0;
}

// One lane, serial over the groups (a handful): offsets that leave [0, total] or decrease are clamped, so that no later kernel
// follows a bad offset out of an array; the block tables are the running sums of ceil(size / 256).
__global__ __launch_bounds__(64) void k_simplify_groups(SimplifyParams s) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int v = 0, t = 0, vb = 0, tb = 0;
    for (int g = 0; g <= s.groups; ++g) {
        const int v_before = v, t_before = t;
        v = min(s.V, max(v, as_global(s.vertex_offsets)[g]));
        t = min(s.T, max(t, as_global(s.triangle_offsets)[g]));
        if (g > 0) {
            vb += (v - v_before + 255) / 256;
            tb += (t - t_before + 255) / 256;
        }
        as_global(s.vfirst)[g] = v;
        as_global(s.tfirst)[g] = t;
        as_global(s.vblk)[g] = vb;
        as_global(s.tblk)[g] = tb;
    }
}

// The mesher lists vertices lattice point by lattice point, so neighbouring lanes often share a cell: every run of equal cells inside
// a wave is summed with a segmented scan first (a lane's terms are below 2^23, 64 of them fit an int) and only the last lane of the run
// goes to memory.  Integer sums: the grouping does not show in the result.
__global__ __launch_bounds__(256) void k_simplify_cluster(SimplifyParams s) {
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    int cell = -1;
    int sum[7] = {0, 0, 0, 0, 0, 0, 0};       // members, f, quantised normal
    if (l.live) {
        const size_t row = (size_t)l.first + l.local;
        const PR_GLOBAL_AS float* v = as_global(s.vertices) + row * 3;
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float top = (float)s.cells[a];
            float q = __fdiv_rn(__fsub_rn(v[a], s.origin[a]), s.cell[a]);
            if (!(q >= 0.f)) q = 0.f;
            if (q > top) q = top;
            c[a] = min((int)q, s.cells[a] - 1);
            const float w = __fsub_rn(q, (float)c[a]);
            sum[1 + a] = (int)(long long)__fmul_rn(w, 1048576.f);
        }
        cell = (c[0] * s.cells[1] + c[1]) * s.cells[2] + c[2];
        sum[0] = 1;
        if (s.nsum) {
            const PR_GLOBAL_AS float* n = as_global(s.normals) + row * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float x = n[a];
                sum[4 + a] = fabsf(x) <= 4.f ? (int)__float2ll_rn(__fmul_rn(x, 1048576.f)) : 0;       // (a NaN fails the comparison)
            }
        }
        as_global(s.vmap)[row] = cell;
    }
    const int lane = (int)threadIdx.x & 63;
    const int cell_before = __shfl_up(cell, 1, 64), cell_after = __shfl_down(cell, 1, 64);       // (every lane takes part)
    int head = lane == 0 || cell_before != cell ? 1 : 0;                  // the lane begins a run; becomes: the sum reaches back to one
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int head_before = __shfl_up(head, d, 64);
        int before[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) before[i] = __shfl_up(sum[i], d, 64);
        if (lane >= d && !head) {
#pragma unroll
            for (int i = 0; i < 7; ++i) sum[i] += before[i];
            head = head_before;
        }
    }
    const bool last = lane == 63 || cell_after != cell;
    if (cell < 0 || !last) return;
    const size_t at = (size_t)l.group * s.C + cell;
    __hip_atomic_fetch_add(as_global(s.cnt) + at, sum[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (sum[1 + a])
            __hip_atomic_fetch_add(as_global(s.fsum) + 3 * at + a, (unsigned long long)sum[1 + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s.nsum) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (sum[4 + a])
                __hip_atomic_fetch_add(as_global(s.nsum) + 3 * at + a, (unsigned long long)(long long)sum[4 + a], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_simplify_mark(SimplifyParams s) {
    __shared__ int lds[4];
    const int group = (int)blockIdx.x / s.D;
    const int cell = ((int)blockIdx.x - group * s.D) * 256 + (int)threadIdx.x;
    const int occupied = cell < s.C && as_global(s.cnt)[(size_t)group * s.C + cell] > 0 ? 1 : 0;
    int total;
    block_exclusive_scan_256(occupied, lds, &total);
    if (threadIdx.x == 0) as_global(s.csum)[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_simplify_vertices(SimplifyParams s) {
    __shared__ int lds[4];
    const int group = (int)blockIdx.x / s.D;
    const int cell = ((int)blockIdx.x - group * s.D) * 256 + (int)threadIdx.x;
    const bool live = cell < s.C;
    const size_t at = (size_t)group * s.C + (live ? cell : 0);
    const int n = live ? as_global(s.cnt)[at] : 0;
    int total;
    const int out = as_global(s.coff)[blockIdx.x] + block_exclusive_scan_256(n > 0 ? 1 : 0, lds, &total);
    if (!live) return;
    as_global(s.cnt)[at] = n > 0 ? out - as_global(s.coff)[(size_t)group * s.D] : -1;
    if (n <= 0 || !s.out_vertices || out >= s.max_vertices) return;
    const int c[3] = {cell / (s.cells[1] * s.cells[2]), (cell / s.cells[2]) % s.cells[1], cell % s.cells[2]};
    const double members = __dmul_rn((double)n, 1048576.0);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mean = __ddiv_rn((double)(long long)as_global(s.fsum)[3 * at + a], members);
        as_global(s.out_vertices)[(size_t)out * 3 + a] =
            (float)__dadd_rn((double)s.origin[a], __dmul_rn(__dadd_rn((double)c[a], mean), (double)s.cell[a]));
    }
    if (s.out_normals) {
        double S[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) S[a] = (double)(long long)as_global(s.nsum)[3 * at + a];
        const double length = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(S[0], S[0]), __dmul_rn(S[1], S[1])), __dmul_rn(S[2], S[2])));
#pragma unroll
        for (int a = 0; a < 3; ++a) as_global(s.out_normals)[(size_t)out * 3 + a] = length == 0.0 ? 0.f : (float)__ddiv_rn(S[a], length);
    }
}

__global__ __launch_bounds__(256) void k_simplify_map(SimplifyParams s) {
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (!l.live) return;
    const size_t row = (size_t)l.first + l.local;
    const int index = as_global(s.cnt)[(size_t)l.group * s.C + as_global(s.vmap)[row]];
    as_global(s.vmap)[row] = index;
    if (s.vertex_map) as_global(s.vertex_map)[row] = index;
}

// The corners of triangle `row` of the lane's group as output indices, rotated so that the smallest comes first.
// Returns 0: kept, 1: degenerate, 2: an input index outside [0, V_g).
__device__ __forceinline__ int simplify_corners(const SimplifyParams& s, const MeshLane& l, size_t row, int* o) {
    const PR_GLOBAL_AS int32_t* t = as_global(s.triangles) + row * 3;
    const int vfirst = as_global(s.vfirst)[l.group];
    const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
    const int i0 = t[0], i1 = t[1], i2 = t[2];
    if (i0 < 0 || i0 >= vsize || i1 < 0 || i1 >= vsize || i2 < 0 || i2 >= vsize) return 2;
    const PR_GLOBAL_AS int32_t* map = as_global(s.vmap) + vfirst;
    const int a = map[i0], b = map[i1], c = map[i2];
    if (a == b || b == c || a == c) return 1;
    if (a < b && a < c) { o[0] = a; o[1] = b; o[2] = c; }
    else if (b < c) { o[0] = b; o[1] = c; o[2] = a; }
    else { o[0] = c; o[1] = a; o[2] = b; }
    return 0;
}

__global__ __launch_bounds__(256) void k_simplify_triangles(SimplifyParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    int state = -1;
    if (l.live) {
        const size_t row = (size_t)l.first + l.local;
        int o[3];
        state = simplify_corners(s, l, row, o);
        int slot = -1;
        if (state == 0 && s.keep) slot = 0;
        if (state == 0 && !s.keep) {
            const unsigned long long key = (unsigned long long)o[0] | (unsigned long long)o[1] << 21 | (unsigned long long)o[2] << 42;
            const unsigned int size = 2u * (unsigned int)l.size;
            const size_t region = 2 * (size_t)l.first;
            unsigned int at = (unsigned int)(noise_mix(key) % size);
            for (unsigned int probe = 0; probe < size; ++probe) {      // (ends at an empty slot or at the key: at most T_g keys in 2 T_g slots)
                unsigned long long seen = SIMPLIFY_EMPTY;
                const bool won = __hip_atomic_compare_exchange_strong(as_global(s.keys) + region + at, &seen, key, __ATOMIC_RELAXED,
                                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (won || seen == key) {
                    slot = (int)(region + at);
                    __hip_atomic_fetch_min(as_global(s.tmin) + slot, (int)row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                at = at + 1 == size ? 0 : at + 1;
            }
        }
        as_global(s.tslot)[row] = slot;
    }
    int kept, outside;
    block_exclusive_scan_256(state == 0 ? 1 : 0, lds, &kept);
    block_exclusive_scan_256(state == 2 ? 1 : 0, lds, &outside);
    if (threadIdx.x == 0) {
        PR_GLOBAL_AS int32_t* counts = as_global(s.counts) + (size_t)l.group * 4;
        if (kept) __hip_atomic_fetch_add(counts + 1, kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (outside) __hip_atomic_fetch_add(counts + 3, outside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ bool simplify_survives(const SimplifyParams& s, const MeshLane& l) {
    if (!l.live) return false;
    const int row = l.first + l.local;
    const int slot = as_global(s.tslot)[row];
    return slot >= 0 && (s.keep || as_global(s.tmin)[slot] == row);
}

__global__ __launch_bounds__(256) void k_simplify_survivors(SimplifyParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    int total;
    block_exclusive_scan_256(simplify_survives(s, l) ? 1 : 0, lds, &total);
    if (threadIdx.x == 0) as_global(s.tsum)[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_simplify_offsets(SimplifyParams s) {
    const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (g > s.groups) return;
    // (a block behind the last group has the sum 0: its offset is the total)
    auto vertex_offset = [&](int k) { return k < s.groups ? as_global(s.coff)[(size_t)k * s.D] : as_global(s.totals)[0]; };
    auto triangle_offset = [&](int k) {
        const int b = k < s.groups ? as_global(s.tblk)[k] : s.BT;
        return b < s.BT ? as_global(s.toff)[b] : as_global(s.totals)[1];
    };
    const int v = vertex_offset(g), t = triangle_offset(g);
    as_global(s.out_vertex_offsets)[g] = v;
    as_global(s.out_triangle_offsets)[g] = t;
    if (g < s.groups) {
        as_global(s.counts)[(size_t)g * 4 + 0] = vertex_offset(g + 1) - v;
        as_global(s.counts)[(size_t)g * 4 + 2] = triangle_offset(g + 1) - t;
    }
}

__global__ __launch_bounds__(256) void k_simplify_emit(SimplifyParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    const bool survives = simplify_survives(s, l);
    int total;
    const int out = as_global(s.toff)[blockIdx.x] + block_exclusive_scan_256(survives ? 1 : 0, lds, &total);
    if (!survives || out >= s.max_triangles) return;
    int o[3];
    simplify_corners(s, l, (size_t)l.first + l.local, o);
    PR_GLOBAL_AS int32_t* dst = as_global(s.out_triangles) + (size_t)out * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e) dst[e] = o[e];
}

struct SimplifyPlan {
    size_t cnt, fsum, nsum, vmap, tslot, keys, tmin, vfirst, tfirst, vblk, tblk, csum, coff, tsum, toff, totals, bytes;
    int C, D, BV, BT;
};

// Host checks of both entry points: no device work.
static int plan_simplify(const pr_simplify_t* s, const char* who, SimplifyPlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {
        PR_REQUIRE(s->cells[a] >= 1, "%s: cells[%d] = %d (>= 1)", who, a, s->cells[a]);
        cells *= (double)s->cells[a];
        PR_REQUIRE(host_finite(s->cell[a]) && s->cell[a] > 0.f, "%s: cell[%d] = %g (finite, > 0)", who, a, (double)s->cell[a]);
        PR_REQUIRE(host_finite(s->origin[a]), "%s: origin[%d] = %g (finite)", who, a, (double)s->origin[a]);
    }
    PR_REQUIRE(cells <= (double)PR_SIMPLIFY_MAX_CELLS, "%s: %d x %d x %d cells (at most 2^21 = %d)", who, s->cells[0], s->cells[1],
               s->cells[2], PR_SIMPLIFY_MAX_CELLS);
    PR_REQUIRE((s->flags & ~PR_SIMPLIFY_KEEP_DUPLICATES) == 0, "%s: flags 0x%x (PR_SIMPLIFY_KEEP_DUPLICATES or 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->max_vertices >= 0 && s->max_triangles >= 0, "%s: negative capacity (max_vertices %d, max_triangles %d)", who,
               s->max_vertices, s->max_triangles);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->out_vertex_offsets && s->out_triangle_offsets,
               "%s: NULL output offsets (out_vertex_offsets / out_triangle_offsets are always written)", who);
    PR_REQUIRE(s->counts != nullptr, "%s: NULL counts (always written)", who);
    PR_REQUIRE(!s->out_normals || s->normals, "%s: out_normals need normals", who);
    PR_REQUIRE(!s->out_normals || s->out_vertices, "%s: out_normals need out_vertices", who);
    const double G = (double)s->groups;
    PR_REQUIRE((double)s->total_vertices + 256.0 * G < 2147483648.0 && 2.0 * (double)s->total_triangles + 256.0 * G < 2147483648.0 &&
                   G * cells < 2147483648.0,
               "%s: mesh too large: total_vertices + 256 groups, 2 total_triangles + 256 groups and groups x cells must stay below 2^31 "
               "(the counts are int32)", who);
    plan->C = (int)cells;
    plan->D = (plan->C + 255) / 256;
    plan->BV = (s->total_vertices + 255) / 256 + s->groups;
    plan->BT = (s->total_triangles + 255) / 256 + s->groups;
    const size_t GC = (size_t)s->groups * (size_t)plan->C, V = (size_t)s->total_vertices, T = (size_t)s->total_triangles;
    const size_t table = ((size_t)s->groups + 1) * sizeof(int32_t);
    size_t at = 0;
    plan->cnt = workspace_region(&at, 4 * GC);
    plan->fsum = workspace_region(&at, 24 * GC);
    plan->nsum = workspace_region(&at, s->normals ? 24 * GC : 0);
    plan->vmap = workspace_region(&at, 4 * V);
    plan->tslot = workspace_region(&at, 4 * T);
    plan->keys = workspace_region(&at, 16 * T);
    plan->tmin = workspace_region(&at, 8 * T);
    plan->vfirst = workspace_region(&at, table);
    plan->tfirst = workspace_region(&at, table);
    plan->vblk = workspace_region(&at, table);
    plan->tblk = workspace_region(&at, table);
    plan->csum = workspace_region(&at, 4 * (size_t)s->groups * plan->D);
    plan->coff = workspace_region(&at, 4 * (size_t)s->groups * plan->D);
    plan->tsum = workspace_region(&at, 4 * (size_t)plan->BT);
    plan->toff = workspace_region(&at, 4 * (size_t)plan->BT);
    plan->totals = workspace_region(&at, 2 * sizeof(int32_t));
    plan->bytes = at;
    PR_REQUIRE(at < ((size_t)1 << 62), "%s: the workspace sum overflows", who);       // (cannot happen below the bounds above)
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_simplify_workspace_size(const pr_simplify_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_simplify_workspace_size: NULL bytes");
    pr::SimplifyPlan plan;
    PR_TRY(pr::plan_simplify(s, "pr_simplify_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_simplify_mesh(const pr_simplify_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    SimplifyPlan plan;
    PR_TRY(plan_simplify(s, "pr_simplify_mesh", &plan));
    PR_TRY(check_workspace("pr_simplify_mesh", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    SimplifyParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.keep = (s->flags & PR_SIMPLIFY_KEEP_DUPLICATES) ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        p.origin[a] = s->origin[a];
        p.cell[a] = s->cell[a];
        p.cells[a] = s->cells[a];
    }
    p.C = plan.C;
    p.D = plan.D;
    p.BV = plan.BV;
    p.BT = plan.BT;
    p.max_vertices = s->max_vertices;
    p.max_triangles = s->max_triangles;
    p.vertices = s->vertices;
    p.normals = s->normals;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.out_vertices = s->out_vertices;
    p.out_normals = s->out_normals;
    p.out_triangles = s->out_triangles;
    p.vertex_map = s->vertex_map;
    p.counts = s->counts;
    p.out_vertex_offsets = s->out_vertex_offsets;
    p.out_triangle_offsets = s->out_triangle_offsets;
    p.cnt = (int32_t*)(ws + plan.cnt);
    p.fsum = (unsigned long long*)(ws + plan.fsum);
    p.nsum = s->normals ? (unsigned long long*)(ws + plan.nsum) : nullptr;
    p.vmap = (int32_t*)(ws + plan.vmap);
    p.tslot = (int32_t*)(ws + plan.tslot);
    p.keys = (unsigned long long*)(ws + plan.keys);
    p.tmin = (int32_t*)(ws + plan.tmin);
    p.vfirst = (int32_t*)(ws + plan.vfirst);
    p.tfirst = (int32_t*)(ws + plan.tfirst);
    p.vblk = (int32_t*)(ws + plan.vblk);
    p.tblk = (int32_t*)(ws + plan.tblk);
    p.csum = (int32_t*)(ws + plan.csum);
    p.coff = (int32_t*)(ws + plan.coff);
    p.tsum = (int32_t*)(ws + plan.tsum);
    p.toff = (int32_t*)(ws + plan.toff);
    p.totals = (int32_t*)(ws + plan.totals);
    const size_t cells = (size_t)s->groups * plan.C, slots = 2 * (size_t)s->total_triangles;
    const size_t most = cells > slots ? cells : slots;
    const unsigned cell_grid = (unsigned)((long)s->groups * plan.D);
    const unsigned init_grid = (unsigned)((most + 255) / 256 < 65536 ? (most + 255) / 256 : 65536);
    hipLaunchKernelGGL(k_simplify_init, dim3(init_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_simplify_groups, dim3(1), dim3(64), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_simplify_cluster, dim3((unsigned)plan.BV), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_simplify_mark, dim3(cell_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    {
        const int32_t* sums[1] = {p.csum};
        int32_t* offsets[1] = {p.coff};
        int32_t* totals[1] = {p.totals};
        PR_TRY(launch_scan_group(sums, offsets, totals, 1, (int)cell_grid, st));
    }
    hipLaunchKernelGGL(k_simplify_vertices, dim3(cell_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_simplify_map, dim3((unsigned)plan.BV), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_simplify_triangles, dim3((unsigned)plan.BT), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_simplify_survivors, dim3((unsigned)plan.BT), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    {
        const int32_t* sums[1] = {p.tsum};
        int32_t* offsets[1] = {p.toff};
        int32_t* totals[1] = {p.totals + 1};
        PR_TRY(launch_scan_group(sums, offsets, totals, 1, plan.BT, st));
    }
    hipLaunchKernelGGL(k_simplify_offsets, dim3((unsigned)(s->groups / 256 + 1)), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (s->out_triangles) {
        hipLaunchKernelGGL(k_simplify_emit, dim3((unsigned)plan.BT), dim3(256), 0, st, p);
        PR_LAUNCH_CHECK();
    }
    return PR_OK;
}
