// Closest-point queries against packed triangle meshes on the cell grid of pr_raycast_build (pr_closest_query; include/playrender.h
// states the rule, DESIGN.md 22 holds the exactness argument).
//
// One launch: k_closest_query, one lane per point, wave64, 256-lane blocks that never span two groups.  The lane tests the group's
// loose list, takes the cell of its point (clamped into the grid) and visits the grid's cells shell by shell - shell r holds the cells
// at Chebyshev index distance exactly r from the start cell - testing each cell's list, until the best squared distance so far is at
// most (r cmin)^2, or (r cmin)^2 exceeds the squared radius, or no shell is left.  A triangle listed in several cells is tested
// several times: a minimum is idempotent.  No lane waits for another, no LDS, no atomics.
#include "mesh_dev.h"

#include <math.h>

namespace pr {

struct ClosestParams {
    int groups, V, T;
    float origin[3], cell[3];
    int cells[3];
    int C, C1;                    // cells per group, lists per group (C + 1)
    int max_references;
    int points_n, point_blocks;   // per group
    float cmin;                   // the smallest cell size
    float radius2;                // max_distance * max_distance, one fp32 product
    const float* vertices; const int32_t* triangles;
    const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    const int32_t* cell_offsets; const int32_t* references;
    const float* points;
    float* distance; int32_t* triangle; float* point; float* barycentric;
};

struct ClosestBest { float d2, v, w, q[3]; int index; };

// Ericson's region walk with every operation written out (the header's rule).  The six dot products and va, vb, vc are computed for
// every pair in front of the chain - a lane that left early would wait for its wave anyway -; the header's chain of conditions then
// chooses the region, and only that region's quotients are computed.  A better (dist2, index) replaces `best`.
__device__ __forceinline__ void closest_test(const PR_GLOBAL_AS float* vertices, int vsize, const PR_GLOBAL_AS int32_t* triangles,
                                             int index, const float* p, float radius2, ClosestBest& best) {
    const PR_GLOBAL_AS int32_t* tri = triangles + (size_t)index * 3;
    const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
    if (i0 < 0 || i0 >= vsize || i1 < 0 || i1 >= vsize || i2 < 0 || i2 >= vsize) return;
    float a[3], b[3], c[3], ab[3], ac[3], bc[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = vertices[(size_t)i0 * 3 + k];
        b[k] = vertices[(size_t)i1 * 3 + k];
        c[k] = vertices[(size_t)i2 * 3 + k];
    }
    if ((a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) || (a[0] == c[0] && a[1] == c[1] && a[2] == c[2])) return;      // dead
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = __fsub_rn(b[k], a[k]);
        ac[k] = __fsub_rn(c[k], a[k]);
        bc[k] = __fsub_rn(c[k], b[k]);
        ap[k] = __fsub_rn(p[k], a[k]);
        bp[k] = __fsub_rn(p[k], b[k]);
        cp[k] = __fsub_rn(p[k], c[k]);
    }
    const float d1 = mesh_dot(ab, ap), d2 = mesh_dot(ac, ap), d3 = mesh_dot(ab, bp), d4 = mesh_dot(ac, bp), d5 = mesh_dot(ab, cp), d6 = mesh_dot(ac, cp);
    const float vc = __fsub_rn(__fmul_rn(d1, d4), __fmul_rn(d3, d2));
    const float vb = __fsub_rn(__fmul_rn(d5, d2), __fmul_rn(d1, d6));
    const float va = __fsub_rn(__fmul_rn(d3, d6), __fmul_rn(d5, d4));
    const float e43 = __fsub_rn(d4, d3), e56 = __fsub_rn(d5, d6);
    float v, w, q[3];
    if (d1 <= 0.f && d2 <= 0.f) {                                          // vertex a
        v = 0.f; w = 0.f;
        q[0] = a[0]; q[1] = a[1]; q[2] = a[2];
    } else if (d3 >= 0.f && d4 <= d3) {                                    // vertex b
        v = 1.f; w = 0.f;
        q[0] = b[0]; q[1] = b[1]; q[2] = b[2];
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                      // edge ab
        v = __fdiv_rn(d1, __fsub_rn(d1, d3)); w = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = __fadd_rn(a[k], __fmul_rn(v, ab[k]));
    } else if (d6 >= 0.f && d5 <= d6) {                                    // vertex c
        v = 0.f; w = 1.f;
        q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {                      // edge ac
        v = 0.f; w = __fdiv_rn(d2, __fsub_rn(d2, d6));
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = __fadd_rn(a[k], __fmul_rn(w, ac[k]));
    } else if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) {                    // edge bc
        w = __fdiv_rn(e43, __fadd_rn(e43, e56)); v = __fsub_rn(1.f, w);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = __fadd_rn(b[k], __fmul_rn(w, bc[k]));
    } else {                                                               // interior (and every NaN)
        const float denom = __fadd_rn(__fadd_rn(va, vb), vc);
        v = __fdiv_rn(vb, denom); w = __fdiv_rn(vc, denom);
        if (!(v >= 0.f)) v = 0.f;                                          // clamped into the triangle, whatever the rounding of va, vb, vc
        if (v > 1.f) v = 1.f;
        if (!(w >= 0.f)) w = 0.f;
        const float top = __fsub_rn(1.f, v);
        if (w > top) w = top;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = __fadd_rn(__fadd_rn(a[k], __fmul_rn(v, ab[k])), __fmul_rn(w, ac[k]));
    }
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = __fsub_rn(p[k], q[k]);
    const float dist2 = mesh_dot(r, r);
    if (!(dist2 <= radius2 && dist2 < INFINITY)) return;
    if (dist2 < best.d2 || (dist2 == best.d2 && index < best.index) || best.index < 0) {
        best.d2 = dist2;
        best.v = v;
        best.w = w;
        best.q[0] = q[0]; best.q[1] = q[1]; best.q[2] = q[2];
        best.index = index;
    }
}

__global__ __launch_bounds__(256) void k_closest_query(ClosestParams s) {
    const int g = (int)blockIdx.x / s.point_blocks;
    const int n = ((int)blockIdx.x - g * s.point_blocks) * 256 + (int)threadIdx.x;
    if (n >= s.points_n) return;
    // the group's clamped slices (block-uniform: scalar loads; the groups are a handful)
    int vfirst = 0, tfirst = 0, vend = 0, tend = 0;
    for (int k = 0; k <= g + 1; ++k) {
        vfirst = vend;
        tfirst = tend;
        vend = min(s.V, max(vend, as_global(s.vertex_offsets)[k]));
        tend = min(s.T, max(tend, as_global(s.triangle_offsets)[k]));
    }
    const int vsize = vend - vfirst, tsize = tend - tfirst;
    const PR_GLOBAL_AS float* vertices = as_global(s.vertices) + (size_t)vfirst * 3;
    const PR_GLOBAL_AS int32_t* triangles = as_global(s.triangles) + (size_t)tfirst * 3;
    const PR_GLOBAL_AS int32_t* offsets = as_global(s.cell_offsets) + (size_t)g * s.C1;
    const size_t row = (size_t)g * s.points_n + n;
    float p[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = as_global(s.points)[row * 3 + a];
        finite = finite && mesh_finite(p[a]);
    }
    ClosestBest best = {INFINITY, 0.f, 0.f, {0.f, 0.f, 0.f}, -1};
    auto test_list = [&](int list) {
        const int begin = max(offsets[list], 0), end = min(offsets[list + 1], s.max_references);
        for (int r = begin; r < end; ++r) {
            const int index = as_global(s.references)[r];
            if (index >= 0 && index < tsize) closest_test(vertices, vsize, triangles, index, p, s.radius2, best);
        }
    };
    // A point with a component that is not finite is accepted by no triangle.
    if (finite) {
        test_list(s.C);
        if (offsets[s.C] > offsets[0]) {                                   // (block-uniform) the group has a reference outside its loose list
            int c0[3];
            int last = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float at = __fdiv_rn(__fsub_rn(p[a], s.origin[a]), s.cell[a]);
                const float top = (float)(s.cells[a] - 1);
                if (!(at >= 0.f)) at = 0.f;
                if (at > top) at = top;
                c0[a] = (int)at;
                last = max(last, max(c0[a], s.cells[a] - 1 - c0[a]));
            }
            for (int r = 0; r <= last; ++r) {
                const int x0 = max(c0[0] - r, 0), x1 = min(c0[0] + r, s.cells[0] - 1);
                const int y0 = max(c0[1] - r, 0), y1 = min(c0[1] + r, s.cells[1] - 1);
                const int z0 = max(c0[2] - r, 0), z1 = min(c0[2] + r, s.cells[2] - 1);
                for (int x = x0; x <= x1; ++x) {
                    for (int y = y0; y <= y1; ++y) {
                        const int base = (x * s.cells[1] + y) * s.cells[2];
                        if (max(abs(x - c0[0]), abs(y - c0[1])) == r) {    // a cell column of the shell's x or y faces
                            for (int z = z0; z <= z1; ++z) test_list(base + z);
                        } else {                                           // (r > 0) only the two z faces
                            if (c0[2] - r >= 0) test_list(base + c0[2] - r);
                            if (c0[2] + r < s.cells[2]) test_list(base + c0[2] + r);
                        }
                    }
                }
                const float reach = __fmul_rn((float)r, s.cmin);
                const float reach2 = __fmul_rn(reach, reach);
                if ((best.index >= 0 && best.d2 <= reach2) || reach2 > s.radius2) break;
            }
        }
    }
    const bool hit = best.index >= 0;
    as_global(s.distance)[row] = hit ? __fsqrt_rn(best.d2) : INFINITY;
    if (s.triangle) as_global(s.triangle)[row] = best.index;
    if (s.point) {
#pragma unroll
        for (int a = 0; a < 3; ++a) as_global(s.point)[row * 3 + a] = hit ? best.q[a] : 0.f;
    }
    if (s.barycentric) {
        as_global(s.barycentric)[row * 2 + 0] = hit ? best.v : 0.f;
        as_global(s.barycentric)[row * 2 + 1] = hit ? best.w : 0.f;
    }
}


}  // namespace pr

extern "C" int pr_closest_query(const pr_closest_t* s, void* stream) {
    using namespace pr;
    const char* who = "pr_closest_query";
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
    PR_REQUIRE(s->flags == 0, "%s: flags 0x%x (no flag is defined: 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->max_references >= 0, "%s: negative capacity (max_references %d)", who, s->max_references);
    PR_REQUIRE(s->count >= 0, "%s: negative point count (count %d)", who, s->count);
    PR_REQUIRE(s->max_distance >= 0.f, "%s: max_distance %g (not NaN, >= 0; +inf is allowed)", who, (double)s->max_distance);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->cell_offsets != nullptr, "%s: NULL cell_offsets", who);
    PR_REQUIRE(s->references || s->max_references == 0, "%s: NULL references with max_references %d", who, s->max_references);
    PR_REQUIRE(s->points != nullptr, "%s: NULL points", who);
    PR_REQUIRE(s->distance != nullptr, "%s: NULL distance (always written)", who);
    PR_REQUIRE(!s->point || s->triangle, "%s: point needs triangle", who);
    PR_REQUIRE(!s->barycentric || s->triangle, "%s: barycentric needs triangle", who);
    const double G = (double)s->groups;
    PR_REQUIRE((double)s->total_triangles + 256.0 * G < 2147483648.0 && G * (cells + 1.0) + 256.0 < 2147483648.0 &&
                   G * ((double)s->count + 256.0) < 2147483648.0,
               "%s: too large: total_triangles + 256 groups, groups x (cells + 1) + 256 and groups x (count + 256) must stay below 2^31 "
               "(the counts are int32)", who);
    if (s->count == 0) return PR_OK;
    ClosestParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.cmin = s->cell[0];
    for (int a = 0; a < 3; ++a) {
        p.origin[a] = s->origin[a];
        p.cell[a] = s->cell[a];
        p.cells[a] = s->cells[a];
        p.cmin = s->cell[a] < p.cmin ? s->cell[a] : p.cmin;
    }
    p.C = (int)cells;
    p.C1 = p.C + 1;
    p.max_references = s->references ? s->max_references : 0;
    p.points_n = s->count;
    p.point_blocks = (s->count + 255) / 256;
    p.radius2 = s->max_distance * s->max_distance;
    p.vertices = s->vertices;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.cell_offsets = s->cell_offsets;
    p.references = s->references;
    p.points = s->points;
    p.distance = s->distance;
    p.triangle = s->triangle;
    p.point = s->point;
    p.barycentric = s->barycentric;
    hipLaunchKernelGGL(k_closest_query, dim3((unsigned)(s->groups * p.point_blocks)), dim3(256), 0, (hipStream_t)stream, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
