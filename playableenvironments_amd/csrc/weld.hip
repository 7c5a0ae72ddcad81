// Welding and compaction of packed triangle meshes (pr_mesh_weld, include/playrender.h states the rule): per group one output vertex
// per class of equal vertex VALUES that a kept triangle refers to (PR_WELD_COMPACT_ONLY: per referenced finite vertex), the kept
// triangles - exactly pr_mesh_audit's candidates - re-indexed, both maps and the counts.
//
// Eight launches on the caller's stream (seven with PR_WELD_COMPACT_ONLY, which has no table), all kernels:
//   k_weld_init       empties the table, zeroes the referenced flags, fills both maps with -1; one lane of block 0 clamps the offsets
//                     and builds the block tables (the rule: mesh_dev.h)
//   k_weld_insert     per vertex: k_audit_weld's insertion into the group's open-addressing table of 2 V_g slots (value mode only)
//   k_weld_lookup     per vertex: its representative - the final content of its key's slot; its own index with PR_WELD_COMPACT_ONLY;
//                     -1 where a component is not finite
//   k_weld_classify   per triangle: kept or dropped; a kept one stores 1 at its three representatives' referenced flags; block sums
//   k_weld_mark       per vertex: a referenced representative?  block sums of those and of the three other kinds of vertex
//   k_weld_scan       two workgroups: the exclusive scans of the vertex and of the triangle block sums, serial over chunks of 256 block
//                     sums with a carry - one level above the blocks, so no size changes its path
//   k_weld_vertices   per vertex block: output indices of its referenced representatives; their rows - positions, normals, attributes -
//                     are copied with consecutive lanes on consecutive words of the block's output rows (attributes in 128-bit
//                     words where the width is a multiple of 4 and both arrays are 16-byte aligned, else in 32-bit words)
//   k_weld_finish     one grid, three block ranges: per triangle the re-indexed corners and the triangle map, per vertex the vertex
//                     map, per group the counts and the output offsets
// Lanes: one per element, wave64, 256-lane blocks that never span two groups (mesh_lane, mesh_dev.h).  The vertex classes are
// pr_mesh_audit's because both units take them from mesh_vertex and mesh_same_values (mesh_dev.h, which also states the table's rule);
// the two probe loops are written out here as in audit.hip.  Integer atomics only, in the insertion; everything later is plain stores
// of values that do not depend on arrival.
#include "mesh_dev.h"

namespace pr {

constexpr int WELD_COUNTS = 8;
constexpr int WELD_MAX_ATTRIBUTE_WIDTH = 4096;
enum { WELD_P_NON_FINITE, WELD_P_MERGED, WELD_P_UNREFERENCED, WELD_PARTIALS };

struct WeldParams {
    int groups, V, T;
    int BV, BT;                   // launched vertex / triangle blocks
    int A;                        // attribute width
    int max_vertices, max_triangles;
    int compact_only;
    int wide;                     // the attribute rows are copied in 128-bit words: A is a multiple of 4, both arrays 16-byte aligned
    const float* vertices; const float* normals; const float* attributes; const int32_t* triangles;
    const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    float* out_vertices; float* out_normals; float* out_attributes; int32_t* out_triangles;
    int32_t* vertex_map; int32_t* triangle_map; int32_t* counts; int32_t* out_vertex_offsets; int32_t* out_triangle_offsets;
    // workspace
    int32_t* vfirst; int32_t* tfirst;   // (G + 1) the offsets, clamped
    int32_t* vblk; int32_t* tblk;       // (G + 1) first block of the group
    int32_t* vslot;               // (2 V) weld table: a vertex index local to the group; group g owns [2 vfirst[g], 2 vfirst[g + 1])
    int32_t* vrep;                // (V) representative of the vertex, local to the group; -1: a component is not finite
    int32_t* vref;                // (V) 1 at a representative that a kept triangle refers to
    int32_t* vout;                // (V) output index (local to the group) of a referenced representative, -1 elsewhere
    int32_t* tkeep;               // (T) 1: kept
    int32_t* vsum; int32_t* voff;       // (BV) referenced representatives per vertex block, (BV + 1) their exclusive scan and the total
    int32_t* tsum; int32_t* toff;       // (BT) kept triangles per triangle block, (BT + 1) their exclusive scan and the total
    int32_t* vpart;               // (BV, 3) per vertex block: the WELD_P_ columns
};

__global__ __launch_bounds__(256) void k_weld_init(WeldParams s) {
    const size_t stride = (size_t)gridDim.x * 256, at = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t V = (size_t)s.V, T = (size_t)s.T;
    if (!s.compact_only)
        for (size_t i = at; i < 2 * V; i += stride) as_global(s.vslot)[i] = MESH_EMPTY_VERTEX;
    for (size_t i = at; i < V; i += stride) {
        as_global(s.vref)[i] = 0;
        if (s.vertex_map) as_global(s.vertex_map)[i] = -1;       // (a row that no clamped group owns keeps this)
    }
    if (s.triangle_map)
        for (size_t i = at; i < T; i += stride) as_global(s.triangle_map)[i] = -1;
    // One lane, serial over the groups (a handful): offsets that leave [0, total] or decrease are clamped, so that no later kernel
    // follows a bad offset out of an array; the block tables are the running sums of ceil(size / 256).
    if (at != 0) return;
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

__global__ __launch_bounds__(256) void k_weld_insert(WeldParams s) {
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (!l.live) return;
    const unsigned int size = 2u * (unsigned int)l.size;
    const MeshVertex v = mesh_vertex(s.vertices, (size_t)l.first + l.local, size);
    if (!v.finite) return;                    // (not inserted: it has no class)
    PR_GLOBAL_AS int32_t* region = as_global(s.vslot) + 2 * (size_t)l.first;
    unsigned int at = v.at;
    for (unsigned int probe = 0; probe < size; ++probe) {      // (ends at an empty slot or at the class: at most V_g classes in 2 V_g slots)
        int seen = MESH_EMPTY_VERTEX;
        if (__hip_atomic_compare_exchange_strong(region + at, &seen, l.local, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (mesh_same_values(s.vertices, l.first, l.size, seen, v)) {
            __hip_atomic_fetch_min(region + at, l.local, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        at = at + 1 == size ? 0 : at + 1;
    }
}

__global__ __launch_bounds__(256) void k_weld_lookup(WeldParams s) {
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (!l.live) return;
    const unsigned int size = 2u * (unsigned int)l.size;
    const size_t row = (size_t)l.first + l.local;
    const MeshVertex v = mesh_vertex(s.vertices, row, size);
    int rep = -1;
    if (v.finite && s.compact_only) rep = l.local;             // (every finite vertex is its own representative)
    else if (v.finite) {
        const PR_GLOBAL_AS int32_t* region = as_global(s.vslot) + 2 * (size_t)l.first;
        unsigned int at = v.at;
        for (unsigned int probe = 0; probe < size; ++probe) {  // (the insertion has finished: the slots hold the minima)
            const int seen = region[at];
            if (seen == MESH_EMPTY_VERTEX) break;
            if (mesh_same_values(s.vertices, l.first, l.size, seen, v)) {
                rep = seen;
                break;
            }
            at = at + 1 == size ? 0 : at + 1;
        }
    }
    as_global(s.vrep)[row] = rep;
}

// The kept triangles are the audit's candidates in BOTH modes.  In value mode equal representatives are equal values and no coordinate
// is read; with PR_WELD_COMPACT_ONLY a representative is an index, so a == b and a == c are decided on the nine coordinates.
__global__ __launch_bounds__(256) void k_weld_classify(WeldParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) {                        // (the whole block: behind the last group, its sum is 0)
        if (threadIdx.x == 0) as_global(s.tsum)[blockIdx.x] = 0;
        return;
    }
    bool kept = false;
    if (l.live) {
        const size_t row = (size_t)l.first + l.local;
        const PR_GLOBAL_AS int32_t* t = as_global(s.triangles) + row * 3;
        const int vfirst = as_global(s.vfirst)[l.group];
        const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
        const int i0 = t[0], i1 = t[1], i2 = t[2];
        int r[3] = {-1, -1, -1};
        if (i0 >= 0 && i0 < vsize && i1 >= 0 && i1 < vsize && i2 >= 0 && i2 < vsize) {
            const PR_GLOBAL_AS int32_t* rep = as_global(s.vrep) + vfirst;
            r[0] = rep[i0];
            r[1] = rep[i1];
            r[2] = rep[i2];
        }
        // a representative is -1 iff a component of the vertex is not finite
        kept = r[0] >= 0 && r[1] >= 0 && r[2] >= 0 && r[0] < vsize && r[1] < vsize && r[2] < vsize;
        if (kept && s.compact_only) {
            const PR_GLOBAL_AS float* v = as_global(s.vertices) + (size_t)vfirst * 3;
            const PR_GLOBAL_AS float* a = v + (size_t)r[0] * 3;
            const PR_GLOBAL_AS float* b = v + (size_t)r[1] * 3;
            const PR_GLOBAL_AS float* c = v + (size_t)r[2] * 3;
            const float ax = a[0], ay = a[1], az = a[2];
            kept = !(ax == b[0] && ay == b[1] && az == b[2]) && !(ax == c[0] && ay == c[1] && az == c[2]);
        } else if (kept) {
            kept = r[0] != r[1] && r[0] != r[2];
        }
        if (kept) {
#pragma unroll
            for (int e = 0; e < 3; ++e) as_global(s.vref)[(size_t)vfirst + r[e]] = 1;      // (every writer stores the same value)
        }
        as_global(s.tkeep)[row] = kept ? 1 : 0;
    }
    int total;
    block_exclusive_scan_256(kept ? 1 : 0, lds, &total);
    if (threadIdx.x == 0) as_global(s.tsum)[blockIdx.x] = total;
}

// 0: not finite, 1: merged into a lower index, 2: a representative without a kept triangle, 3: a referenced representative
__device__ __forceinline__ int weld_vertex_kind(const WeldParams& s, const MeshLane& l) {
    const size_t row = (size_t)l.first + l.local;
    const int rep = as_global(s.vrep)[row];
    if (rep < 0) return 0;
    if (rep != l.local) return 1;
    return as_global(s.vref)[row] != 0 ? 3 : 2;
}

__global__ __launch_bounds__(256) void k_weld_mark(WeldParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (l.group < 0) {                        // (the whole block: behind the last group, its sum is 0)
        if (threadIdx.x == 0) as_global(s.vsum)[blockIdx.x] = 0;
        return;
    }
    const int kind = l.live ? weld_vertex_kind(s, l) : -1;
    int total[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) block_exclusive_scan_256(kind == k ? 1 : 0, lds, &total[k]);
    if (threadIdx.x == 0) {
        as_global(s.vsum)[blockIdx.x] = total[3];
        PR_GLOBAL_AS int32_t* part = as_global(s.vpart) + (size_t)blockIdx.x * WELD_PARTIALS;
        part[WELD_P_NON_FINITE] = total[0];
        part[WELD_P_MERGED] = total[1];
        part[WELD_P_UNREFERENCED] = total[2];
    }
}

// Workgroup 0 scans the BV vertex block sums, workgroup 1 the BT triangle block sums: chunks of 256 in order with a carry, so the
// scan has ONE path for every size; offsets[n] is the total.
__global__ __launch_bounds__(256) void k_weld_scan(WeldParams s) {
    __shared__ int lds[4];
    const PR_GLOBAL_AS int32_t* sums = as_global(blockIdx.x == 0 ? s.vsum : s.tsum);
    PR_GLOBAL_AS int32_t* offsets = as_global(blockIdx.x == 0 ? s.voff : s.toff);
    const int n = blockIdx.x == 0 ? s.BV : s.BT;
    int carry = 0;
    for (int start = 0; start < n; start += 256) {
        const int i = start + (int)threadIdx.x;
        const int v = i < n ? sums[i] : 0;
        int chunk;
        const int ex = block_exclusive_scan_256(v, lds, &chunk);
        if (i < n) offsets[i] = carry + ex;
        carry += chunk;
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

typedef uint32_t weld_word4 __attribute__((ext_vector_type(4)));

// the block's `rows` output rows from `base` on: consecutive lanes on consecutive words of `Word` (32 bits, or 128 where the width and
// both addresses allow it), copied bit for bit; `width` counts Words; 64-bit offsets
template <class Word>
__device__ __forceinline__ void weld_copy_rows(const float* src, float* dst, int width, int first, const int* source, int base, int rows,
                                               int capacity) {
    const PR_GLOBAL_AS Word* in = (const PR_GLOBAL_AS Word*)as_global(src);
    PR_GLOBAL_AS Word* out = (PR_GLOBAL_AS Word*)as_global(dst);
    const int words = rows * width;           // (<= 256 x 4096)
    for (int i = (int)threadIdx.x; i < words; i += 256) {
        const int k = i / width, c = i - k * width;
        if (base + k >= capacity) break;      // (k only grows)
        out[(size_t)(base + k) * (size_t)width + c] = in[((size_t)first + source[k]) * (size_t)width + c];
    }
}

__global__ __launch_bounds__(256) void k_weld_vertices(WeldParams s) {
    __shared__ int lds[4];
    __shared__ int source[256];               // local index of the block's k-th output vertex
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    const bool referenced = l.live && weld_vertex_kind(s, l) == 3;
    int rows;
    const int at = block_exclusive_scan_256(referenced ? 1 : 0, lds, &rows);
    const int base = as_global(s.voff)[blockIdx.x];                           // first output row of the block, over all groups
    const int group_base = as_global(s.voff)[as_global(s.vblk)[l.group]];     // (vblk <= BV, and voff has BV + 1 entries)
    if (l.live) as_global(s.vout)[(size_t)l.first + l.local] = referenced ? base + at - group_base : -1;
    if (!s.out_vertices) return;              // (normals and attributes need it)
    if (referenced) source[at] = l.local;
    __syncthreads();
    weld_copy_rows<uint32_t>(s.vertices, s.out_vertices, 3, l.first, source, base, rows, s.max_vertices);
    if (s.out_normals) weld_copy_rows<uint32_t>(s.normals, s.out_normals, 3, l.first, source, base, rows, s.max_vertices);
    if (s.out_attributes && s.wide)
        weld_copy_rows<weld_word4>(s.attributes, s.out_attributes, s.A / 4, l.first, source, base, rows, s.max_vertices);
    else if (s.out_attributes)
        weld_copy_rows<uint32_t>(s.attributes, s.out_attributes, s.A, l.first, source, base, rows, s.max_vertices);
}

// One grid, three block ranges.  [0, BT): triangle blocks.  [BT, BT + BV): vertex blocks.  [BT + BV, BT + BV + G): a block per group.
__global__ __launch_bounds__(256) void k_weld_finish(WeldParams s) {
    __shared__ int lds[4];
    const int b = (int)blockIdx.x;
    if (b < s.BT) {
        const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, b);
        if (l.group < 0) return;              // (the whole block)
        const size_t row = (size_t)l.first + l.local;
        const bool kept = l.live && as_global(s.tkeep)[row] != 0;
        int total;
        const int out = as_global(s.toff)[b] + block_exclusive_scan_256(kept ? 1 : 0, lds, &total);
        if (!l.live) return;
        if (s.triangle_map) as_global(s.triangle_map)[row] = kept ? out - as_global(s.toff)[as_global(s.tblk)[l.group]] : -1;
        if (!kept || !s.out_triangles || out >= s.max_triangles) return;
        const PR_GLOBAL_AS int32_t* t = as_global(s.triangles) + row * 3;
        const int vfirst = as_global(s.vfirst)[l.group];
        const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
        PR_GLOBAL_AS int32_t* dst = as_global(s.out_triangles) + (size_t)out * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {         // (read again: checked again; a kept triangle passes every check)
            const int i = t[e];
            const int rep = i >= 0 && i < vsize ? as_global(s.vrep)[(size_t)vfirst + i] : -1;
            dst[e] = rep >= 0 && rep < vsize ? as_global(s.vout)[(size_t)vfirst + rep] : -1;
        }
        return;
    }
    if (b < s.BT + s.BV) {
        if (!s.vertex_map) return;
        const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, b - s.BT);
        if (!l.live) return;
        const size_t row = (size_t)l.first + l.local;
        const int rep = as_global(s.vrep)[row];
        as_global(s.vertex_map)[row] = rep >= 0 && rep < l.size ? as_global(s.vout)[(size_t)l.first + rep] : -1;
        return;
    }
    // integers: lane t sums the rows of the group's vertex blocks t, t + 256, ..., the block adds the lanes up
    const int g = b - s.BT - s.BV;
    const int vbegin = as_global(s.vblk)[g], vend = as_global(s.vblk)[g + 1];
    const int tbegin = as_global(s.tblk)[g], tend = as_global(s.tblk)[g + 1];
    int sum[WELD_PARTIALS] = {0, 0, 0}, total[WELD_PARTIALS];
    for (int k = vbegin + (int)threadIdx.x; k < vend; k += 256) {
        const PR_GLOBAL_AS int32_t* part = as_global(s.vpart) + (size_t)k * WELD_PARTIALS;
#pragma unroll
        for (int i = 0; i < WELD_PARTIALS; ++i) sum[i] += part[i];
    }
#pragma unroll
    for (int i = 0; i < WELD_PARTIALS; ++i) block_exclusive_scan_256(sum[i], lds, &total[i]);
    if (threadIdx.x != 0) return;
    // (the blocks behind the last group have the sum 0: the offset of block vblk[G] is the total)
    const int v0 = as_global(s.voff)[vbegin], v1 = as_global(s.voff)[vend];
    const int t0 = as_global(s.toff)[tbegin], t1 = as_global(s.toff)[tend];
    PR_GLOBAL_AS int32_t* counts = as_global(s.counts) + (size_t)g * WELD_COUNTS;
    counts[0] = v1 - v0;
    counts[1] = t1 - t0;
    counts[2] = as_global(s.tfirst)[g + 1] - as_global(s.tfirst)[g] - (t1 - t0);
    counts[3] = total[WELD_P_NON_FINITE];
    counts[4] = total[WELD_P_MERGED];
    counts[5] = total[WELD_P_UNREFERENCED];
    counts[6] = 0;
    counts[7] = 0;
    as_global(s.out_vertex_offsets)[g] = v0;
    as_global(s.out_triangle_offsets)[g] = t0;
    if (g == s.groups - 1) {
        as_global(s.out_vertex_offsets)[s.groups] = v1;
        as_global(s.out_triangle_offsets)[s.groups] = t1;
    }
}

struct WeldPlan {
    size_t vfirst, tfirst, vblk, tblk, vslot, vrep, vref, vout, tkeep, vsum, voff, tsum, toff, vpart, bytes;
    int BV, BT;
};

// Host checks of both entry points: no device work.
static int plan_weld(const pr_mesh_weld_t* s, const char* who, WeldPlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    PR_REQUIRE((s->flags & ~PR_WELD_COMPACT_ONLY) == 0, "%s: unknown flag bits 0x%x (PR_WELD_COMPACT_ONLY or 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->max_vertices >= 0 && s->max_triangles >= 0, "%s: negative capacity (max_vertices %d, max_triangles %d)", who,
               s->max_vertices, s->max_triangles);
    PR_REQUIRE(s->attribute_width >= 0 && s->attribute_width <= WELD_MAX_ATTRIBUTE_WIDTH, "%s: attribute_width %d (0 .. %d)", who,
               s->attribute_width, WELD_MAX_ATTRIBUTE_WIDTH);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->out_vertex_offsets && s->out_triangle_offsets, "%s: NULL offsets (out_vertex_offsets / out_triangle_offsets)", who);
    PR_REQUIRE(s->counts != nullptr, "%s: NULL counts (always written)", who);
    PR_REQUIRE(!s->out_attributes || (s->attributes && s->attribute_width > 0),
               "%s: out_attributes needs attributes and an attribute_width > 0", who);
    PR_REQUIRE(!s->out_normals || s->normals, "%s: out_normals without normals", who);
    PR_REQUIRE((!s->out_normals && !s->out_attributes) || s->out_vertices, "%s: out_normals / out_attributes without out_vertices", who);
    const double G = (double)s->groups;
    PR_REQUIRE(2.0 * (double)s->total_vertices + 256.0 * G < 2147483648.0 && (double)s->total_triangles + 256.0 * G < 2147483648.0,
               "%s: mesh too large: 2 total_vertices + 256 groups and total_triangles + 256 groups must stay below 2^31 "
               "(the table slots and the block counts are int32)", who);
    plan->BV = (s->total_vertices + 255) / 256 + s->groups;
    plan->BT = (s->total_triangles + 255) / 256 + s->groups;
    const size_t V = (size_t)s->total_vertices, T = (size_t)s->total_triangles;
    const size_t table = ((size_t)s->groups + 1) * sizeof(int32_t);
    size_t at = 0;
    plan->vfirst = workspace_region(&at, table);
    plan->tfirst = workspace_region(&at, table);
    plan->vblk = workspace_region(&at, table);
    plan->tblk = workspace_region(&at, table);
    plan->vslot = workspace_region(&at, 8 * V);
    plan->vrep = workspace_region(&at, 4 * V);
    plan->vref = workspace_region(&at, 4 * V);
    plan->vout = workspace_region(&at, 4 * V);
    plan->tkeep = workspace_region(&at, 4 * T);
    plan->vsum = workspace_region(&at, 4 * (size_t)plan->BV);
    plan->voff = workspace_region(&at, 4 * ((size_t)plan->BV + 1));
    plan->tsum = workspace_region(&at, 4 * (size_t)plan->BT);
    plan->toff = workspace_region(&at, 4 * ((size_t)plan->BT + 1));
    plan->vpart = workspace_region(&at, (size_t)WELD_PARTIALS * sizeof(int32_t) * (size_t)plan->BV);
    plan->bytes = at;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_mesh_weld_workspace_size(const pr_mesh_weld_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_mesh_weld_workspace_size: NULL bytes");
    pr::WeldPlan plan;
    PR_TRY(pr::plan_weld(s, "pr_mesh_weld_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_mesh_weld(const pr_mesh_weld_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    static_assert(sizeof(pr_mesh_weld_t) == 152, "the header states this size");
    WeldPlan plan;
    PR_TRY(plan_weld(s, "pr_mesh_weld", &plan));
    PR_TRY(check_workspace("pr_mesh_weld", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    WeldParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.BV = plan.BV;
    p.BT = plan.BT;
    p.A = s->attribute_width;
    p.max_vertices = s->max_vertices;
    p.max_triangles = s->max_triangles;
    p.compact_only = (s->flags & PR_WELD_COMPACT_ONLY) ? 1 : 0;
    p.wide = s->attribute_width % 4 == 0 && (((uintptr_t)s->attributes | (uintptr_t)s->out_attributes) & 15) == 0 ? 1 : 0;
    p.vertices = s->vertices;
    p.normals = s->normals;
    p.attributes = s->attributes;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.out_vertices = s->out_vertices;
    p.out_normals = s->out_normals;
    p.out_attributes = s->out_attributes;
    p.out_triangles = s->out_triangles;
    p.vertex_map = s->vertex_map;
    p.triangle_map = s->triangle_map;
    p.counts = s->counts;
    p.out_vertex_offsets = s->out_vertex_offsets;
    p.out_triangle_offsets = s->out_triangle_offsets;
    p.vfirst = (int32_t*)(ws + plan.vfirst);
    p.tfirst = (int32_t*)(ws + plan.tfirst);
    p.vblk = (int32_t*)(ws + plan.vblk);
    p.tblk = (int32_t*)(ws + plan.tblk);
    p.vslot = (int32_t*)(ws + plan.vslot);
    p.vrep = (int32_t*)(ws + plan.vrep);
    p.vref = (int32_t*)(ws + plan.vref);
    p.vout = (int32_t*)(ws + plan.vout);
    p.tkeep = (int32_t*)(ws + plan.tkeep);
    p.vsum = (int32_t*)(ws + plan.vsum);
    p.voff = (int32_t*)(ws + plan.voff);
    p.tsum = (int32_t*)(ws + plan.tsum);
    p.toff = (int32_t*)(ws + plan.toff);
    p.vpart = (int32_t*)(ws + plan.vpart);
    const size_t most = (size_t)s->total_triangles > 2 * (size_t)s->total_vertices ? (size_t)s->total_triangles
                                                                                 : 2 * (size_t)s->total_vertices;
    const unsigned init_grid = (unsigned)((most + 255) / 256 < 65536 ? (most + 255) / 256 + 1 : 65536);
    const dim3 vertex_grid((unsigned)plan.BV), triangle_grid((unsigned)plan.BT);
    hipLaunchKernelGGL(k_weld_init, dim3(init_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (!p.compact_only) {
        hipLaunchKernelGGL(k_weld_insert, vertex_grid, dim3(256), 0, st, p);
        PR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_weld_lookup, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_weld_classify, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_weld_mark, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_weld_scan, dim3(2), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_weld_vertices, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_weld_finish, dim3((unsigned)(plan.BT + plan.BV + s->groups)), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
