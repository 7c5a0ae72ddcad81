// Triangle-triangle intersection of packed meshes on the cell grid of pr_raycast_build (pr_mesh_intersect; include/playrender.h
// states the rule, DESIGN.md 28 holds the argument that the grid changes nothing).
//
// Five launches on the caller's stream for a counting call, six for an emitting one, all kernels:
//   k_intersect_groups   one lane: the clamped per-group offsets of both mesh sets and the first query block of every group
//   k_intersect_walk     (counting) one lane per query triangle, 256-lane blocks that never span two groups (the block table of
//                        mesh_dev.h): the lane tests the group's loose list, then walks the cells its box overlaps and tests their
//                        lists; it writes count and first
//   k_intersect_mark     per 256 packed rows: rows that no clamped group owns get count 0 / first -1; the block sum of the counts
//                                                                                          -> k_scan_blocks_group
//   k_intersect_offsets  per row: the exclusive sum (workspace, and pair_offsets where given); the element behind the last row is P
//   k_intersect_walk     (emitting, only with `pairs`) the same walk again: pair k of a row goes to slot offset + k
// A tight target listed in several cells of a query's range is tested in ONE of them - the cell of max(g(min T), g(min Q)) per axis,
// which lies in both ranges whenever the boxes overlap -: a sum, unlike a minimum, is not idempotent.  No lane waits for another, no
// LDS outside the scans, no atomics.
#include "mesh_dev.h"

#include <math.h>

namespace pr {

constexpr float INTERSECT_CONDITION = 9.5367431640625e-07f;   // 2^-20: det^2 at or below this fraction of |e1|^2 |e2|^2 |d|^2 is noise

struct IntersectParams {
    int groups, V, T, QV, QT;
    int self;
    float origin[3], cell[3];
    int cells[3];
    int C, C1;                    // cells per group, lists per group (C + 1)
    int max_references, max_pairs;
    int rows;                     // QT + 1: the rows of the offsets
    const float* vertices; const int32_t* triangles;
    const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    const int32_t* cell_offsets; const int32_t* references;
    const float* q_vertices; const int32_t* q_triangles;
    const int32_t* q_vertex_offsets; const int32_t* q_triangle_offsets;
    const float* transform;
    int32_t* count; int32_t* first; int32_t* pair_offsets; int32_t* pairs; float* segments;
    // workspace
    int32_t* vfirst; int32_t* tfirst;                      // (G + 1) clamped offsets of the targets
    int32_t* qvfirst; int32_t* qtfirst; int32_t* qtblk;    // (G + 1) clamped offsets of the queries, first query block
    int32_t* off;                 // (QT + 1) exclusive sums of count
    int32_t* bsum; int32_t* boff; // (NB)
    int32_t* total;               // [P]
};

// One lane, serial over the groups: offsets that leave [0, total] or decrease are clamped (the rule: mesh_dev.h).
__global__ __launch_bounds__(64) void k_intersect_groups(IntersectParams s) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int v = 0, t = 0, qv = 0, qt = 0, qb = 0;
    for (int g = 0; g <= s.groups; ++g) {
        const int qt_before = qt;
        v = min(s.V, max(v, as_global(s.vertex_offsets)[g]));
        t = min(s.T, max(t, as_global(s.triangle_offsets)[g]));
        qv = min(s.QV, max(qv, as_global(s.q_vertex_offsets)[g]));
        qt = min(s.QT, max(qt, as_global(s.q_triangle_offsets)[g]));
        if (g > 0) qb += (qt - qt_before + 255) / 256;
        as_global(s.vfirst)[g] = v;
        as_global(s.tfirst)[g] = t;
        as_global(s.qvfirst)[g] = qv;
        as_global(s.qtfirst)[g] = qt;
        as_global(s.qtblk)[g] = qb;
    }
}

// A triangle as one side of the pair rule: corners, e1 = b - a, e2 = c - a, ee = (e1 . e1) (e2 . e2), the box.
struct IxTriangle { float a[3], b[3], c[3], e1[3], e2[3], ee, lo[3], hi[3]; };

__device__ __forceinline__ void ix_prepare(IxTriangle& x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x.e1[k] = __fsub_rn(x.b[k], x.a[k]);
        x.e2[k] = __fsub_rn(x.c[k], x.a[k]);
        x.lo[k] = fminf(fminf(x.a[k], x.b[k]), x.c[k]);
        x.hi[k] = fmaxf(fmaxf(x.a[k], x.b[k]), x.c[k]);
    }
    x.ee = __fmul_rn(mesh_dot(x.e1, x.e1), mesh_dot(x.e2, x.e2));
}

// The header's ray-triangle test of the edge o -> e against y with t in [0, 1], no culling, and the conditioning clause.
__device__ __forceinline__ bool ix_edge(const float* o, const float* e, const IxTriangle& y, float* point) {
    float d[3], sv[3], p[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = __fsub_rn(e[k], o[k]);
        sv[k] = __fsub_rn(o[k], y.a[k]);
    }
    mesh_cross(d, y.e2, p);
    const float det = mesh_dot(y.e1, p);
    if (!(det > 0.f || det < 0.f)) return false;
    if (!(__fmul_rn(det, det) > __fmul_rn(INTERSECT_CONDITION, __fmul_rn(y.ee, mesh_dot(d, d))))) return false;
    const float u = __fdiv_rn(mesh_dot(sv, p), det);
    mesh_cross(sv, y.e1, q);
    const float v = __fdiv_rn(mesh_dot(d, q), det);
    const float t = __fdiv_rn(mesh_dot(y.e2, q), det);
    if (!(u >= 0.f && v >= 0.f && __fadd_rn(u, v) <= 1.f && t >= 0.f && t <= 1.f)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) point[k] = __fadd_rn(o[k], __fmul_rn(t, d[k]));
    return true;
}

// Whether `at` is the cell of max(g(min T), g(min Q)) on one axis - the one cell in which a tight pair is tested.
__device__ __forceinline__ bool ix_own_cell(float tlo, float origin, float cell, float gq, int cells, int at) {
    const float p = fmaxf(__fdiv_rn(__fsub_rn(tlo, origin), cell), gq);
    return p >= 0.f && p < (float)cells && (int)p == at;
}

// One axis of the query's walk: g(min Q) and the inclusive cell range; false if the box misses the grid's box on this axis.
__device__ __forceinline__ bool ix_cell_range(float qlo, float qhi, float origin, float cell, int cells, float* gq, int* lo, int* hi) {
    const float top = (float)cells;
    *gq = __fdiv_rn(__fsub_rn(qlo, origin), cell);
    const float high = __fdiv_rn(__fsub_rn(qhi, origin), cell);
    const bool ok = high >= 0.f && *gq < top;
    *lo = ok ? (int)fmaxf(*gq, 0.f) : 0;                                   // (0 <= the argument < cells)
    *hi = ok ? min((int)fminf(high, top), cells - 1) : -1;
    return ok;
}

// The contact segment so far, in scalars and updated with selects only: an array whose element is chosen by a condition becomes
// private memory.
struct IxSegment { float p0x, p0y, p0z, p1x, p1y, p1z, far; int n; };

__device__ __forceinline__ void ix_add(IxSegment& seg, const float* point) {
    const bool first = seg.n == 0;
    seg.p0x = first ? point[0] : seg.p0x;
    seg.p0y = first ? point[1] : seg.p0y;
    seg.p0z = first ? point[2] : seg.p0z;
    const float r[3] = {__fsub_rn(point[0], seg.p0x), __fsub_rn(point[1], seg.p0y), __fsub_rn(point[2], seg.p0z)};
    const float d2 = mesh_dot(r, r);
    const bool better = first || d2 > seg.far;                             // (the earliest point on ties)
    seg.far = first ? 0.f : (better ? d2 : seg.far);
    seg.p1x = better ? point[0] : seg.p1x;
    seg.p1y = better ? point[1] : seg.p1y;
    seg.p1z = better ? point[2] : seg.p1z;
    ++seg.n;
}

// EDGE(Q -> T) or EDGE(T -> Q).  `all`: every accepted test adds its point to `seg`, in the header's order; otherwise the first ends it.
__device__ __forceinline__ bool ix_edges(const IxTriangle& q, const IxTriangle& t, bool all, IxSegment& seg) {
    float point[3];
    seg.p0x = seg.p0y = seg.p0z = seg.p1x = seg.p1y = seg.p1z = seg.far = 0.f;
    seg.n = 0;
    if (ix_edge(q.a, q.b, t, point)) { ix_add(seg, point); if (!all) return true; }
    if (ix_edge(q.b, q.c, t, point)) { ix_add(seg, point); if (!all) return true; }
    if (ix_edge(q.c, q.a, t, point)) { ix_add(seg, point); if (!all) return true; }
    if (ix_edge(t.a, t.b, q, point)) { ix_add(seg, point); if (!all) return true; }
    if (ix_edge(t.b, t.c, q, point)) { ix_add(seg, point); if (!all) return true; }
    if (ix_edge(t.c, t.a, q, point)) { ix_add(seg, point); if (!all) return true; }
    return seg.n > 0;
}

__global__ __launch_bounds__(256) void k_intersect_walk(IntersectParams s, int emit) {
    const int b = (int)blockIdx.x;
    const PR_GLOBAL_AS int32_t* table = as_global(s.qtblk);
    if (b >= table[s.groups]) return;           // (the whole block: it lies behind the last group)
    int g = 0, top = s.groups;                  // table[g] <= b < table[top]
    while (top - g > 1) {
        const int mid = (g + top) >> 1;
        if (table[mid] <= b) g = mid;
        else top = mid;
    }
    const int qtfirst = as_global(s.qtfirst)[g], qtsize = as_global(s.qtfirst)[g + 1] - qtfirst;
    const int qvfirst = as_global(s.qvfirst)[g], qvsize = as_global(s.qvfirst)[g + 1] - qvfirst;
    const int tfirst = as_global(s.tfirst)[g], tsize = as_global(s.tfirst)[g + 1] - tfirst;
    const int vfirst = as_global(s.vfirst)[g], vsize = as_global(s.vfirst)[g + 1] - vfirst;
    const int local = (b - table[g]) * 256 + (int)threadIdx.x;
    if (local >= qtsize) return;
    const size_t row = (size_t)qtfirst + local;
    const PR_GLOBAL_AS float* qvertices = as_global(s.q_vertices) + (size_t)qvfirst * 3;
    const PR_GLOBAL_AS float* vertices = as_global(s.vertices) + (size_t)vfirst * 3;
    const PR_GLOBAL_AS int32_t* triangles = as_global(s.triangles) + (size_t)tfirst * 3;
    const PR_GLOBAL_AS int32_t* offsets = as_global(s.cell_offsets) + (size_t)g * s.C1;

    // the query triangle: three indices in range, nine finite coordinates after the transform
    IxTriangle q;
    bool candidate;
    {
        const PR_GLOBAL_AS int32_t* tri = as_global(s.q_triangles) + row * 3;
        const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
        candidate = i0 >= 0 && i0 < qvsize && i1 >= 0 && i1 < qvsize && i2 >= 0 && i2 < qvsize;
        if (candidate) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                q.a[k] = qvertices[(size_t)i0 * 3 + k];
                q.b[k] = qvertices[(size_t)i1 * 3 + k];
                q.c[k] = qvertices[(size_t)i2 * 3 + k];
            }
            if (s.transform) {
                const PR_GLOBAL_AS float* m = as_global(s.transform) + (size_t)g * 12;
                float a[3], bb[3], c[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float m0 = m[k * 4 + 0], m1 = m[k * 4 + 1], m2 = m[k * 4 + 2], m3 = m[k * 4 + 3];
                    a[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m0, q.a[0]), __fmul_rn(m1, q.a[1])), __fmul_rn(m2, q.a[2])), m3);
                    bb[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m0, q.b[0]), __fmul_rn(m1, q.b[1])), __fmul_rn(m2, q.b[2])), m3);
                    c[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m0, q.c[0]), __fmul_rn(m1, q.c[1])), __fmul_rn(m2, q.c[2])), m3);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    q.a[k] = a[k];
                    q.b[k] = bb[k];
                    q.c[k] = c[k];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) candidate = candidate && mesh_finite(q.a[k]) && mesh_finite(q.b[k]) && mesh_finite(q.c[k]);
        }
    }
    int found = 0, lowest = -1;
    if (candidate) {
        ix_prepare(q);
        const int base = emit ? as_global(s.off)[row] : 0;
        const bool all = emit && s.segments != nullptr;
        float gq0 = 0.f, gq1 = 0.f, gq2 = 0.f;                             // g(min Q), set in front of the cell walk (scalars: no private array)
        // One target of a list.  cx >= 0: the cell being visited - the pair is tested there only if it is the cell of
        // max(g(min T), g(min Q)) on every axis.
        auto test = [&](int index, int cx, int cy, int cz) {
            const PR_GLOBAL_AS int32_t* tri = triangles + (size_t)index * 3;
            const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
            if (i0 < 0 || i0 >= vsize || i1 < 0 || i1 >= vsize || i2 < 0 || i2 >= vsize) return;
            if (s.self && index == local) return;
            IxTriangle t;
            bool finite = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t.a[k] = vertices[(size_t)i0 * 3 + k];
                t.b[k] = vertices[(size_t)i1 * 3 + k];
                t.c[k] = vertices[(size_t)i2 * 3 + k];
                finite = finite && mesh_finite(t.a[k]) && mesh_finite(t.b[k]) && mesh_finite(t.c[k]);
            }
            if (!finite || mesh_same(t.a, t.b) || mesh_same(t.a, t.c)) return;                           // no candidate, dead
            bool box = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t.lo[k] = fminf(fminf(t.a[k], t.b[k]), t.c[k]);
                t.hi[k] = fmaxf(fmaxf(t.a[k], t.b[k]), t.c[k]);
                box = box && q.lo[k] <= t.hi[k] && t.lo[k] <= q.hi[k];
            }
            if (!box) return;
            if (cx >= 0 && !(ix_own_cell(t.lo[0], s.origin[0], s.cell[0], gq0, s.cells[0], cx) &&
                             ix_own_cell(t.lo[1], s.origin[1], s.cell[1], gq1, s.cells[1], cy) &&
                             ix_own_cell(t.lo[2], s.origin[2], s.cell[2], gq2, s.cells[2], cz)))
                return;                                                    // counted in another cell
            if (s.self && (mesh_same(q.a, t.a) || mesh_same(q.a, t.b) || mesh_same(q.a, t.c) || mesh_same(q.b, t.a) || mesh_same(q.b, t.b) ||
                           mesh_same(q.b, t.c) || mesh_same(q.c, t.a) || mesh_same(q.c, t.b) || mesh_same(q.c, t.c)))
                return;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t.e1[k] = __fsub_rn(t.b[k], t.a[k]);
                t.e2[k] = __fsub_rn(t.c[k], t.a[k]);
            }
            t.ee = __fmul_rn(mesh_dot(t.e1, t.e1), mesh_dot(t.e2, t.e2));
            IxSegment seg;
            if (!ix_edges(q, t, all, seg)) return;
            if (emit) {
                const long long slot = (long long)base + found;
                if (slot >= 0 && slot < (long long)s.max_pairs) {
                    as_global(s.pairs)[slot * 2 + 0] = local;
                    as_global(s.pairs)[slot * 2 + 1] = index;
                    if (s.segments) {
                        PR_GLOBAL_AS float* row6 = as_global(s.segments) + slot * 6;
                        row6[0] = seg.p0x; row6[1] = seg.p0y; row6[2] = seg.p0z;
                        row6[3] = seg.p1x; row6[4] = seg.p1y; row6[5] = seg.p1z;
                    }
                }
            }
            ++found;
            lowest = lowest < 0 ? index : min(lowest, index);
        };
        auto test_list = [&](int list, int cx, int cy, int cz) {
            const int begin = max(offsets[list], 0), end = min(offsets[list + 1], s.max_references);
            for (int r = begin; r < end; ++r) {
                const int index = as_global(s.references)[r];
                if (index >= 0 && index < tsize) test(index, cx, cy, cz);
            }
        };
        test_list(s.C, -1, -1, -1);
        // The cells the query's box overlaps; a box that misses the grid's box meets no tight target.
        int x0, x1, y0, y1, z0, z1;
        bool inside = offsets[s.C] > offsets[0];                          // (block-uniform) the group has a reference outside its loose list
        inside = ix_cell_range(q.lo[0], q.hi[0], s.origin[0], s.cell[0], s.cells[0], &gq0, &x0, &x1) && inside;
        inside = ix_cell_range(q.lo[1], q.hi[1], s.origin[1], s.cell[1], s.cells[1], &gq1, &y0, &y1) && inside;
        inside = ix_cell_range(q.lo[2], q.hi[2], s.origin[2], s.cell[2], s.cells[2], &gq2, &z0, &z1) && inside;
        if (inside) {
            for (int x = x0; x <= x1; ++x)
                for (int y = y0; y <= y1; ++y)
                    for (int z = z0; z <= z1; ++z) test_list((x * s.cells[1] + y) * s.cells[2] + z, x, y, z);
        }
    }
    if (!emit) {
        as_global(s.count)[row] = found;
        if (s.first) as_global(s.first)[row] = lowest;
    }
}

// Rows of the packed query order that no clamped group owns are no candidates: count 0, first -1.  Then the block sums.
__global__ __launch_bounds__(256) void k_intersect_mark(IntersectParams s) {
    __shared__ int lds[4];
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    int value = 0;
    if (i < s.QT) {
        const bool owned = i >= as_global(s.qtfirst)[0] && i < as_global(s.qtfirst)[s.groups];
        if (owned) {
            value = as_global(s.count)[i];
        } else {
            as_global(s.count)[i] = 0;
            if (s.first) as_global(s.first)[i] = -1;
        }
    }
    int total;
    block_exclusive_scan_256(value, lds, &total);
    if (threadIdx.x == 0) as_global(s.bsum)[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_intersect_offsets(IntersectParams s) {
    __shared__ int lds[4];
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    int total;
    const int at = as_global(s.boff)[blockIdx.x] + block_exclusive_scan_256(i < s.QT ? as_global(s.count)[i] : 0, lds, &total);
    if (i < s.rows) {                                                      // (the rows behind the last one count 0: row QT receives P)
        as_global(s.off)[i] = at;
        if (s.pair_offsets) as_global(s.pair_offsets)[i] = at;
    }
}

struct IntersectPlan {
    size_t vfirst, tfirst, qvfirst, qtfirst, qtblk, off, bsum, boff, total, bytes;
    int C, QV, QT, BQ, NB, self;
};

// Host checks shared by the two entry points: no device work.
static int plan_intersect(const pr_mesh_intersect_t* s, const char* who, IntersectPlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {
        PR_REQUIRE(s->cells[a] >= 1 && s->cells[a] <= PR_RAYCAST_MAX_AXIS_CELLS, "%s: cells[%d] = %d (1 .. %d)", who, a, s->cells[a],
                   PR_RAYCAST_MAX_AXIS_CELLS);
        cells *= (double)s->cells[a];
        PR_REQUIRE(host_finite(s->cell[a]) && s->cell[a] > 0.f, "%s: cell[%d] = %g (finite, > 0)", who, a, (double)s->cell[a]);
        PR_REQUIRE(host_finite(s->origin[a]), "%s: origin[%d] = %g (finite)", who, a, (double)s->origin[a]);
    }
    PR_REQUIRE(cells <= (double)PR_RAYCAST_MAX_CELLS, "%s: %d x %d x %d cells (at most 2^21 = %d)", who, s->cells[0], s->cells[1],
               s->cells[2], PR_RAYCAST_MAX_CELLS);
    PR_REQUIRE((s->flags & ~PR_INTERSECT_SELF) == 0, "%s: flags 0x%x (PR_INTERSECT_SELF or 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->q_total_vertices >= 0 && s->q_total_triangles >= 0, "%s: negative total (q_total_vertices %d, q_total_triangles %d)",
               who, s->q_total_vertices, s->q_total_triangles);
    PR_REQUIRE(s->max_references >= 0 && s->max_pairs >= 0, "%s: negative capacity (max_references %d, max_pairs %d)", who,
               s->max_references, s->max_pairs);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->cell_offsets != nullptr, "%s: NULL cell_offsets", who);
    PR_REQUIRE(s->references || s->max_references == 0, "%s: NULL references with max_references %d", who, s->max_references);
    plan->self = (s->flags & PR_INTERSECT_SELF) ? 1 : 0;
    if (plan->self) {
        PR_REQUIRE(s->transform == nullptr, "%s: PR_INTERSECT_SELF with a transform", who);
        PR_REQUIRE((!s->q_vertices || s->q_vertices == s->vertices) && (!s->q_triangles || s->q_triangles == s->triangles) &&
                       (!s->q_vertex_offsets || s->q_vertex_offsets == s->vertex_offsets) &&
                       (!s->q_triangle_offsets || s->q_triangle_offsets == s->triangle_offsets),
                   "%s: PR_INTERSECT_SELF with foreign query pointers (NULL or the targets')", who);
        PR_REQUIRE(s->q_total_vertices == s->total_vertices && s->q_total_triangles == s->total_triangles,
                   "%s: PR_INTERSECT_SELF with other query totals (%d, %d; the targets' are %d, %d)", who, s->q_total_vertices,
                   s->q_total_triangles, s->total_vertices, s->total_triangles);
    } else {
        PR_REQUIRE(s->q_vertices != nullptr, "%s: NULL q_vertices", who);
        PR_REQUIRE(s->q_triangles != nullptr, "%s: NULL q_triangles", who);
        PR_REQUIRE(s->q_vertex_offsets && s->q_triangle_offsets, "%s: NULL offsets (q_vertex_offsets / q_triangle_offsets)", who);
    }
    PR_REQUIRE(s->count != nullptr, "%s: NULL count (always written)", who);
    PR_REQUIRE(!s->segments || s->pairs, "%s: segments needs pairs", who);
    const double G = (double)s->groups;
    PR_REQUIRE((double)s->total_triangles + 256.0 * G < 2147483648.0 && G * (cells + 1.0) + 256.0 < 2147483648.0 &&
                   (double)s->q_total_triangles + 256.0 * G < 2147483648.0,
               "%s: too large: total_triangles + 256 groups, q_total_triangles + 256 groups and groups x (cells + 1) + 256 must stay "
               "below 2^31 (the counts are int32)", who);
    plan->C = (int)cells;
    plan->QV = s->q_total_vertices;
    plan->QT = s->q_total_triangles;
    plan->BQ = (plan->QT + 255) / 256 + s->groups;
    plan->NB = plan->QT / 256 + 1;                         // (covers the element behind the last row, which receives P)
    const size_t table = ((size_t)s->groups + 1) * sizeof(int32_t);
    size_t at = 0;
    plan->vfirst = workspace_region(&at, table);
    plan->tfirst = workspace_region(&at, table);
    plan->qvfirst = workspace_region(&at, table);
    plan->qtfirst = workspace_region(&at, table);
    plan->qtblk = workspace_region(&at, table);
    plan->off = workspace_region(&at, 4 * ((size_t)plan->QT + 1));
    plan->bsum = workspace_region(&at, 4 * (size_t)plan->NB);
    plan->boff = workspace_region(&at, 4 * (size_t)plan->NB);
    plan->total = workspace_region(&at, sizeof(int32_t));
    plan->bytes = at;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_mesh_intersect_workspace_size(const pr_mesh_intersect_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_mesh_intersect_workspace_size: NULL bytes");
    pr::IntersectPlan plan;
    PR_TRY(pr::plan_intersect(s, "pr_mesh_intersect_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_mesh_intersect(const pr_mesh_intersect_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    IntersectPlan plan;
    PR_TRY(plan_intersect(s, "pr_mesh_intersect", &plan));
    PR_TRY(check_workspace("pr_mesh_intersect", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    IntersectParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.QV = plan.QV;
    p.QT = plan.QT;
    p.self = plan.self;
    for (int a = 0; a < 3; ++a) {
        p.origin[a] = s->origin[a];
        p.cell[a] = s->cell[a];
        p.cells[a] = s->cells[a];
    }
    p.C = plan.C;
    p.C1 = plan.C + 1;
    p.max_references = s->references ? s->max_references : 0;
    p.max_pairs = s->pairs ? s->max_pairs : 0;
    p.rows = plan.QT + 1;
    p.vertices = s->vertices;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.cell_offsets = s->cell_offsets;
    p.references = s->references;
    p.q_vertices = plan.self ? s->vertices : s->q_vertices;
    p.q_triangles = plan.self ? s->triangles : s->q_triangles;
    p.q_vertex_offsets = plan.self ? s->vertex_offsets : s->q_vertex_offsets;
    p.q_triangle_offsets = plan.self ? s->triangle_offsets : s->q_triangle_offsets;
    p.transform = s->transform;
    p.count = s->count;
    p.first = s->first;
    p.pair_offsets = s->pair_offsets;
    p.pairs = s->pairs;
    p.segments = s->segments;
    p.vfirst = (int32_t*)(ws + plan.vfirst);
    p.tfirst = (int32_t*)(ws + plan.tfirst);
    p.qvfirst = (int32_t*)(ws + plan.qvfirst);
    p.qtfirst = (int32_t*)(ws + plan.qtfirst);
    p.qtblk = (int32_t*)(ws + plan.qtblk);
    p.off = (int32_t*)(ws + plan.off);
    p.bsum = (int32_t*)(ws + plan.bsum);
    p.boff = (int32_t*)(ws + plan.boff);
    p.total = (int32_t*)(ws + plan.total);
    hipLaunchKernelGGL(k_intersect_groups, dim3(1), dim3(64), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_intersect_walk, dim3((unsigned)plan.BQ), dim3(256), 0, st, p, 0);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_intersect_mark, dim3((unsigned)plan.NB), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    {
        const int32_t* sums[1] = {p.bsum};
        int32_t* offsets[1] = {p.boff};
        int32_t* totals[1] = {p.total};
        PR_TRY(launch_scan_group(sums, offsets, totals, 1, plan.NB, st));
    }
    hipLaunchKernelGGL(k_intersect_offsets, dim3((unsigned)plan.NB), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (s->pairs && s->max_pairs > 0) {
        hipLaunchKernelGGL(k_intersect_walk, dim3((unsigned)plan.BQ), dim3(256), 0, st, p, 1);
        PR_LAUNCH_CHECK();
    }
    return PR_OK;
}
