// Audit of packed triangle meshes (pr_mesh_audit, include/playrender.h states the rule): per group, whether the directed edges
// balance by vertex VALUE, boundary and non-manifold edges, Euler characteristic, connected shells, area, signed volume and centroid,
// and optionally a shell label per triangle.
//
// Nine launches on the caller's stream (eight without measures), all kernels:
//   k_audit_init      empties both tables, zeroes the flags and the shell sizes, fills labels with -1; one lane of block 0
//                     clamps the offsets and builds the block tables (the rule: mesh_dev.h)
//   k_audit_weld      per vertex: inserts its index into the group's open-addressing table of 2 V_g slots, keyed by the three values;
//                     a slot only ever moves to a lower index with the SAME values, so a 32-bit word stands for the 96-bit key
//   k_audit_lookup    per vertex: its representative = the final content of its key's slot (the lowest index with its values)
//   k_audit_edges     per triangle: candidate or dropped; per side with distinct ends the 62-bit key lo | hi << 31 goes into the
//                     group's table of 6 T_g slots (64-bit compare-and-swap on the key word), then one integer add on the slot's
//                     forward or backward counter and an atomic minimum of the triangle's index on its owner word
//   k_audit_unite     per triangle: unites it with the owner of each of its slots (lock-free union-find, parent <= own index)
//   k_audit_flatten   per triangle: label = root = the lowest triangle of the shell; shell sizes at the roots
//   k_audit_count     per triangle block its 1536 edge slots and its 256 triangles, per vertex block its vertices (two block ranges
//                     of one grid): one row of integer partial sums per block, no atomic on a shared word
//   k_audit_measure   per triangle: the three fp64 terms, reduced per block in a fixed tree, one row of partials per block
//   k_audit_finish    one block per group: the integer partials -> counts, the fp64 partials in a fixed order -> measures
// Lanes: one per element, wave64, 256-lane blocks that never span two groups (mesh_lane, mesh_dev.h).  Integer atomics only; the
// floating-point sums are trees of fixed shape.  No lane ever waits for another: a probe sequence ends after at most the region's size
// (2 V_g slots hold at most V_g keys, 6 T_g slots at most 3 T_g), and the union-find is mesh_uf_find / mesh_uf_unite, shared with
// components.hip; mesh_dev.h holds the vertex table's rule and the union-find's TERMINATION argument.
#include "mesh_dev.h"

#include <math.h>

namespace pr {

constexpr unsigned long long AUDIT_EMPTY_EDGE = ~0ull;     // (a key has 62 bits)
constexpr int AUDIT_NO_TRIANGLE = 0x7FFFFFFF;
constexpr int AUDIT_COUNTS = 12, AUDIT_MEASURES = 8, AUDIT_TERMS = 5;
// columns of a triangle block's integer partials
enum { AUDIT_P_CANDIDATES, AUDIT_P_DROPPED, AUDIT_P_EDGES, AUDIT_P_UNBALANCED, AUDIT_P_BOUNDARY, AUDIT_P_NON_MANIFOLD, AUDIT_P_SHELLS,
       AUDIT_P_LARGEST, AUDIT_PARTIALS };

struct AuditParams {
    int groups, V, T;
    int BV, BT;                   // launched vertex / triangle blocks
    const float* vertices; const int32_t* triangles;
    const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    int32_t* counts; double* measures; int32_t* labels;
    // workspace
    int32_t* vfirst; int32_t* tfirst;   // (G + 1) the offsets, clamped
    int32_t* vblk; int32_t* tblk;       // (G + 1) first block of the group
    int32_t* vslot;               // (2 V) weld table: a vertex index local to the group; group g owns [2 vfirst[g], 2 vfirst[g + 1])
    int32_t* vrep;                // (V) representative of the vertex, local to the group; -1: a component is not finite
    int32_t* vref;                // (V) 1 at a representative that a candidate's side refers to
    unsigned long long* ekey;     // (6 T) edge table keys; group g owns [6 tfirst[g], 6 tfirst[g + 1])
    int32_t* ecnt;                // (6 T, 2) sides running low -> high, high -> low
    int32_t* eown;                // (6 T) lowest triangle (local) with a side on the slot's edge
    int32_t* tslot;               // (T, 3) slot of each side, -1: none
    int32_t* parent;              // (T) union-find parent, local to the group; -1: dropped
    int32_t* tsize;               // (T) triangles of the shell, at its root
    double* partial;              // (BT, 5) per block: area, volume, area-weighted corner means
    int32_t* tpart;               // (BT, 8) per triangle block: the AUDIT_P_ columns (sums; the last one a maximum)
    int32_t* vpart;               // (BV) per vertex block: referenced representatives
};

__global__ __launch_bounds__(256) void k_audit_init(AuditParams s) {
    const size_t stride = (size_t)gridDim.x * 256, at = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t V = (size_t)s.V, T = (size_t)s.T;
    for (size_t i = at; i < 2 * V; i += stride) as_global(s.vslot)[i] = MESH_EMPTY_VERTEX;
    for (size_t i = at; i < V; i += stride) as_global(s.vref)[i] = 0;
    for (size_t i = at; i < 6 * T; i += stride) {
        as_global(s.ekey)[i] = AUDIT_EMPTY_EDGE;
        as_global(s.ecnt)[2 * i] = 0;
        as_global(s.ecnt)[2 * i + 1] = 0;
        as_global(s.eown)[i] = AUDIT_NO_TRIANGLE;
    }
    for (size_t i = at; i < T; i += stride) {
        as_global(s.tsize)[i] = 0;
        if (s.labels) as_global(s.labels)[i] = -1;           // (a row that no clamped group owns keeps this)
    }
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

__global__ __launch_bounds__(256) void k_audit_weld(AuditParams s) {
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

__global__ __launch_bounds__(256) void k_audit_lookup(AuditParams s) {
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (!l.live) return;
    const unsigned int size = 2u * (unsigned int)l.size;
    const size_t row = (size_t)l.first + l.local;
    const MeshVertex v = mesh_vertex(s.vertices, row, size);
    int rep = -1;
    if (v.finite) {
        const PR_GLOBAL_AS int32_t* region = as_global(s.vslot) + 2 * (size_t)l.first;
        unsigned int at = v.at;
        for (unsigned int probe = 0; probe < size; ++probe) {  // (the weld kernel has finished: the slots hold the minima)
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

__global__ __launch_bounds__(256) void k_audit_edges(AuditParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    bool candidate = false;
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
        // a representative is -1 iff a component of the vertex is not finite, and equal iff the values are
        candidate = r[0] >= 0 && r[1] >= 0 && r[2] >= 0 && r[0] < vsize && r[1] < vsize && r[2] < vsize && r[0] != r[1] && r[0] != r[2];
        const unsigned int size = 6u * (unsigned int)l.size;
        const size_t region = 6 * (size_t)l.first;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int u = r[e], w = r[e == 2 ? 0 : e + 1];
            int slot = -1;
            if (candidate && u != w) {
                const int low = min(u, w), high = max(u, w);
                const unsigned long long key = (unsigned long long)low | (unsigned long long)high << 31;
                unsigned int at = (unsigned int)(noise_mix(key) % size);
                for (unsigned int probe = 0; probe < size; ++probe) {  // (ends at an empty slot or at the key: at most 3 T_g keys in 6 T_g slots)
                    unsigned long long seen = AUDIT_EMPTY_EDGE;
                    const bool won = __hip_atomic_compare_exchange_strong(as_global(s.ekey) + region + at, &seen, key, __ATOMIC_RELAXED,
                                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (won || seen == key) {
                        slot = (int)(region + at);
                        __hip_atomic_fetch_add(as_global(s.ecnt) + 2 * (size_t)slot + (u == low ? 0 : 1), 1, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_min(as_global(s.eown) + slot, l.local, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                    at = at + 1 == size ? 0 : at + 1;
                }
                as_global(s.vref)[(size_t)vfirst + u] = 1;             // (every writer stores the same value)
                as_global(s.vref)[(size_t)vfirst + w] = 1;
            }
            as_global(s.tslot)[row * 3 + e] = slot;
        }
        as_global(s.parent)[row] = candidate ? l.local : -1;
    }
    int candidates, dropped;
    block_exclusive_scan_256(candidate ? 1 : 0, lds, &candidates);
    block_exclusive_scan_256(l.live && !candidate ? 1 : 0, lds, &dropped);
    if (threadIdx.x == 0) {
        as_global(s.tpart)[(size_t)blockIdx.x * AUDIT_PARTIALS + AUDIT_P_CANDIDATES] = candidates;
        as_global(s.tpart)[(size_t)blockIdx.x * AUDIT_PARTIALS + AUDIT_P_DROPPED] = dropped;
    }
}

__global__ __launch_bounds__(256) void k_audit_unite(AuditParams s) {
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (!l.live) return;
    const size_t row = (size_t)l.first + l.local;
    PR_GLOBAL_AS int32_t* parent = as_global(s.parent) + l.first;
    if (parent[l.local] < 0) return;          // (candidate <=> parent >= 0, which no kernel after k_audit_edges changes)
    const long long lowest = 6 * (long long)l.first, highest = lowest + 6 * (long long)l.size;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int slot = as_global(s.tslot)[row * 3 + e];
        if (slot < lowest || slot >= highest) continue;
        const int owner = as_global(s.eown)[slot];
        // the owner is a candidate of this group with a side on the same edge, and no higher than this triangle
        if (owner >= 0 && owner < l.local && parent[owner] >= 0) mesh_uf_unite(parent, l.local, owner);
    }
}

__global__ __launch_bounds__(256) void k_audit_flatten(AuditParams s) {
    __shared__ int block_root, block_sum;
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    PR_GLOBAL_AS int32_t* parent = as_global(s.parent) + l.first;
    PR_GLOBAL_AS int32_t* size = as_global(s.tsize) + l.first;
    int root = -1;
    if (l.live && parent[l.local] >= 0) {
        root = mesh_uf_find(parent, l.local);   // (no unions in this kernel: the roots are final)
        parent[l.local] = root;
    }
    if (l.live && s.labels) as_global(s.labels)[(size_t)l.first + l.local] = root;
    if (threadIdx.x == 0) {
        block_root = -1;
        block_sum = 0;
    }
    __syncthreads();
    if (root >= 0) atomicMax(&block_root, root);   // one root of the block is summed in LDS, the common case of a large shell
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
    __syncthreads();
    if (threadIdx.x == 0 && shared_root >= 0 && block_sum)
        __hip_atomic_fetch_add(size + shared_root, block_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One grid, two block ranges.  [0, BT): triangle block b, the k-th of its group, counts the edge slots [1536 k, 1536 k + 1536) of the
// group's region - six per lane - and the roots among its 256 triangles.  [BT, BT + BV): vertex blocks.  Every block writes its own row
// of partial sums: hundreds of thousands of blocks adding to one word of counts would queue up behind one another.
__global__ __launch_bounds__(256) void k_audit_count(AuditParams s) {
    __shared__ int lds[4];
    __shared__ int block_largest;
    const int b = (int)blockIdx.x;
    if (b >= s.BT) {
        const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, b - s.BT);
        if (l.group < 0) return;              // (the whole block)
        int referenced = 0, total;
        if (l.live) {
            const size_t row = (size_t)l.first + l.local;
            referenced = as_global(s.vrep)[row] == l.local && as_global(s.vref)[row] != 0 ? 1 : 0;
        }
        block_exclusive_scan_256(referenced, lds, &total);
        if (threadIdx.x == 0) as_global(s.vpart)[b - s.BT] = total;
        return;
    }
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, b);
    if (l.group < 0) return;                  // (the whole block)
    int sum[5] = {0, 0, 0, 0, 0};
    const long long slots = 6 * (long long)l.size, begin = 6 * (long long)(l.local - (int)threadIdx.x);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const long long local = begin + 256 * j + (int)threadIdx.x;
        if (local >= slots) continue;
        const size_t slot = 6 * (size_t)l.first + (size_t)local;
        if (as_global(s.ekey)[slot] == AUDIT_EMPTY_EDGE) continue;
        const int f = as_global(s.ecnt)[2 * slot], r = as_global(s.ecnt)[2 * slot + 1];
        sum[0] += 1;
        sum[1] += f != r ? 1 : 0;
        sum[2] += f + r == 1 ? 1 : 0;
        sum[3] += f + r > 2 ? 1 : 0;
    }
    if (threadIdx.x == 0) block_largest = 0;
    __syncthreads();
    if (l.live) {
        const size_t row = (size_t)l.first + l.local;
        if (as_global(s.parent)[row] == l.local) {
            sum[4] = 1;
            atomicMax(&block_largest, as_global(s.tsize)[row]);        // (LDS)
        }
    }
    PR_GLOBAL_AS int32_t* part = as_global(s.tpart) + (size_t)b * AUDIT_PARTIALS;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        int total;
        block_exclusive_scan_256(sum[i], lds, &total);                 // (its barriers also order block_largest)
        if (threadIdx.x == 0) part[AUDIT_P_EDGES + i] = total;
    }
    if (threadIdx.x == 0) part[AUDIT_P_LARGEST] = block_largest;
}

// The header's tree over the 256 lanes of a block: in every wave, for d = 32, 16, 8, 4, 2, 1, lane i takes x_i + x_(i + d) - lane 0
// then holds the wave's sum -, and the block's sum is ((w_0 + w_1) + w_2) + w_3.  Valid in thread 0.  lds: >= 4 doubles.
__device__ __forceinline__ double audit_block_sum(double x, double* lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = x + __shfl_down(x, d, 64);
    __syncthreads();                          // (the previous use of lds has been read)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ __launch_bounds__(256) void k_audit_measure(AuditParams s) {
    __shared__ double lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    double term[AUDIT_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (l.live && as_global(s.parent)[(size_t)l.first + l.local] >= 0) {       // a candidate: its indices are in range
        const PR_GLOBAL_AS int32_t* t = as_global(s.triangles) + ((size_t)l.first + l.local) * 3;
        const int vfirst = as_global(s.vfirst)[l.group];
        const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
        const int i0 = t[0], i1 = t[1], i2 = t[2];
        if (i0 >= 0 && i0 < vsize && i1 >= 0 && i1 < vsize && i2 >= 0 && i2 < vsize) {      // (read again: checked again)
            const PR_GLOBAL_AS float* v = as_global(s.vertices) + (size_t)vfirst * 3;
            double a[3], b[3], c[3], e1[3], e2[3], n[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                a[x] = (double)v[(size_t)i0 * 3 + x];
                b[x] = (double)v[(size_t)i1 * 3 + x];
                c[x] = (double)v[(size_t)i2 * 3 + x];
                e1[x] = b[x] - a[x];
                e2[x] = c[x] - a[x];
            }
            n[0] = e1[1] * e2[2] - e1[2] * e2[1];
            n[1] = e1[2] * e2[0] - e1[0] * e2[2];
            n[2] = e1[0] * e2[1] - e1[1] * e2[0];
            const double area = 0.5 * __dsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            const double m0 = b[1] * c[2] - b[2] * c[1], m1 = b[2] * c[0] - b[0] * c[2], m2 = b[0] * c[1] - b[1] * c[0];
            term[0] = area;
            term[1] = ((a[0] * m0 + a[1] * m1) + a[2] * m2) / 6.0;
#pragma unroll
            for (int x = 0; x < 3; ++x) term[2 + x] = area * (((a[x] + b[x]) + c[x]) / 3.0);
        }
    }
#pragma unroll
    for (int q = 0; q < AUDIT_TERMS; ++q) {
        const double total = audit_block_sum(term[q], lds);
        if (threadIdx.x == 0) as_global(s.partial)[(size_t)blockIdx.x * AUDIT_TERMS + q] = total;
    }
}

// One block per group.  Integers: lane t sums the rows of the group's triangle blocks t, t + 256, ... and of its vertex blocks, the
// block adds the lanes up (any order gives the same integers).  Measures: lane t sums the fp64 partials of the group's blocks t,
// t + 256, t + 512, ... in that order, starting from 0; the 256 lane sums go through the block tree.
__global__ __launch_bounds__(256) void k_audit_finish(AuditParams s) {
    __shared__ double lds[4];
    __shared__ int ilds[4];
    __shared__ int group_largest;
    const int g = (int)blockIdx.x;
    const int begin = as_global(s.tblk)[g], end = as_global(s.tblk)[g + 1];
    int sum[AUDIT_PARTIALS] = {0, 0, 0, 0, 0, 0, 0, 0}, referenced = 0;
    for (int b = begin + (int)threadIdx.x; b < end; b += 256) {
        const PR_GLOBAL_AS int32_t* part = as_global(s.tpart) + (size_t)b * AUDIT_PARTIALS;
#pragma unroll
        for (int i = 0; i < AUDIT_P_LARGEST; ++i) sum[i] += part[i];
        sum[AUDIT_P_LARGEST] = max(sum[AUDIT_P_LARGEST], part[AUDIT_P_LARGEST]);
    }
    for (int b = as_global(s.vblk)[g] + (int)threadIdx.x; b < as_global(s.vblk)[g + 1]; b += 256) referenced += as_global(s.vpart)[b];
    if (threadIdx.x == 0) group_largest = 0;
    __syncthreads();
    if (sum[AUDIT_P_LARGEST] > 0) atomicMax(&group_largest, sum[AUDIT_P_LARGEST]);       // (LDS)
    int total[AUDIT_P_LARGEST], vertices;
#pragma unroll
    for (int i = 0; i < AUDIT_P_LARGEST; ++i) block_exclusive_scan_256(sum[i], ilds, &total[i]);
    block_exclusive_scan_256(referenced, ilds, &vertices);             // (the barriers inside also order group_largest)
    if (threadIdx.x == 0) {
        PR_GLOBAL_AS int32_t* counts = as_global(s.counts) + (size_t)g * AUDIT_COUNTS;
        counts[0] = total[AUDIT_P_CANDIDATES];
        counts[1] = total[AUDIT_P_DROPPED];
        counts[2] = vertices;
        counts[3] = total[AUDIT_P_EDGES];
        counts[4] = total[AUDIT_P_UNBALANCED];
        counts[5] = total[AUDIT_P_BOUNDARY];
        counts[6] = total[AUDIT_P_NON_MANIFOLD];
        counts[7] = vertices - total[AUDIT_P_EDGES] + total[AUDIT_P_CANDIDATES];
        counts[8] = total[AUDIT_P_SHELLS];
        counts[9] = group_largest;
        counts[10] = 0;
        counts[11] = 0;
    }
    if (!s.measures) return;
    double measure[AUDIT_TERMS];
#pragma unroll
    for (int q = 0; q < AUDIT_TERMS; ++q) {
        double lane_sum = 0.0;
        for (int b = begin + (int)threadIdx.x; b < end; b += 256) lane_sum = lane_sum + as_global(s.partial)[(size_t)b * AUDIT_TERMS + q];
        measure[q] = audit_block_sum(lane_sum, lds);
    }
    if (threadIdx.x == 0) {
        PR_GLOBAL_AS double* m = as_global(s.measures) + (size_t)g * AUDIT_MEASURES;
        m[0] = measure[0];
        m[1] = measure[1];
#pragma unroll
        for (int x = 0; x < 3; ++x) m[2 + x] = measure[0] > 0.0 ? measure[2 + x] / measure[0] : 0.0;
#pragma unroll
        for (int x = 5; x < AUDIT_MEASURES; ++x) m[x] = 0.0;
    }
}

struct AuditPlan {
    size_t vfirst, tfirst, vblk, tblk, vslot, vrep, vref, ekey, ecnt, eown, tslot, parent, tsize, partial, tpart, vpart, bytes;
    int BV, BT;
};

// Host checks of both entry points: no device work.
static int plan_audit(const pr_mesh_audit_t* s, const char* who, AuditPlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    PR_REQUIRE(s->flags == 0, "%s: flags 0x%x (no flag is defined: 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->counts != nullptr, "%s: NULL counts (always written)", who);
    const double G = (double)s->groups;
    PR_REQUIRE(2.0 * (double)s->total_vertices + 256.0 * G < 2147483648.0 && 6.0 * (double)s->total_triangles + 256.0 * G < 2147483648.0,
               "%s: mesh too large: 2 total_vertices + 256 groups and 6 total_triangles + 256 groups must stay below 2^31 "
               "(the table slots are int32)", who);
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
    plan->ekey = workspace_region(&at, 48 * T);
    plan->ecnt = workspace_region(&at, 48 * T);
    plan->eown = workspace_region(&at, 24 * T);
    plan->tslot = workspace_region(&at, 12 * T);
    plan->parent = workspace_region(&at, 4 * T);
    plan->tsize = workspace_region(&at, 4 * T);
    plan->partial = workspace_region(&at, (size_t)AUDIT_TERMS * sizeof(double) * (size_t)plan->BT);
    plan->tpart = workspace_region(&at, (size_t)AUDIT_PARTIALS * sizeof(int32_t) * (size_t)plan->BT);
    plan->vpart = workspace_region(&at, sizeof(int32_t) * (size_t)plan->BV);
    plan->bytes = at;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_mesh_audit_workspace_size(const pr_mesh_audit_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_mesh_audit_workspace_size: NULL bytes");
    pr::AuditPlan plan;
    PR_TRY(pr::plan_audit(s, "pr_mesh_audit_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_mesh_audit(const pr_mesh_audit_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    static_assert(sizeof(pr_mesh_audit_t) == 72, "the header states this size");
    AuditPlan plan;
    PR_TRY(plan_audit(s, "pr_mesh_audit", &plan));
    PR_TRY(check_workspace("pr_mesh_audit", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    AuditParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.BV = plan.BV;
    p.BT = plan.BT;
    p.vertices = s->vertices;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.counts = s->counts;
    p.measures = s->measures;
    p.labels = s->labels;
    p.vfirst = (int32_t*)(ws + plan.vfirst);
    p.tfirst = (int32_t*)(ws + plan.tfirst);
    p.vblk = (int32_t*)(ws + plan.vblk);
    p.tblk = (int32_t*)(ws + plan.tblk);
    p.vslot = (int32_t*)(ws + plan.vslot);
    p.vrep = (int32_t*)(ws + plan.vrep);
    p.vref = (int32_t*)(ws + plan.vref);
    p.ekey = (unsigned long long*)(ws + plan.ekey);
    p.ecnt = (int32_t*)(ws + plan.ecnt);
    p.eown = (int32_t*)(ws + plan.eown);
    p.tslot = (int32_t*)(ws + plan.tslot);
    p.parent = (int32_t*)(ws + plan.parent);
    p.tsize = (int32_t*)(ws + plan.tsize);
    p.partial = (double*)(ws + plan.partial);
    p.tpart = (int32_t*)(ws + plan.tpart);
    p.vpart = (int32_t*)(ws + plan.vpart);
    const size_t most = 6 * (size_t)s->total_triangles > 2 * (size_t)s->total_vertices ? 6 * (size_t)s->total_triangles
                                                                                     : 2 * (size_t)s->total_vertices;
    const unsigned init_grid = (unsigned)((most + 255) / 256 < 65536 ? (most + 255) / 256 + 1 : 65536);
    const dim3 vertex_grid((unsigned)plan.BV), triangle_grid((unsigned)plan.BT);
    hipLaunchKernelGGL(k_audit_init, dim3(init_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_audit_weld, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_audit_lookup, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_audit_edges, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_audit_unite, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_audit_flatten, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_audit_count, dim3((unsigned)(plan.BT + plan.BV)), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (s->measures) {
        hipLaunchKernelGGL(k_audit_measure, triangle_grid, dim3(256), 0, st, p);
        PR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_audit_finish, dim3((unsigned)s->groups), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
