// Inside / outside queries against packed triangle meshes on the cell grid of pr_raycast_build (pr_inside_query; include/playrender.h
// states the rule, DESIGN.md 23 holds the argument that the walk changes nothing).
//
// One launch: k_inside_query<K>, K = the axis of the call, one lane per point, wave64, 256-lane blocks that never span two groups.  The
// lane sums the rule over the group's loose list and over the cells of its column (s_i, s_j, max(s_k, 0) .. cells_k - 1); a triangle
// listed in several cells of the column is summed in the first of them that the lane visits.  Per candidate: exact fp32 rejections,
// then per edge a float64 filter, then the exact sign of the expanded determinant (an expansion sum in registers: every index is a
// compile-time constant, there is no scratch).  No lane waits for another, no LDS, no atomics.
#include "mesh_dev.h"

#include <math.h>

namespace pr {

constexpr float INSIDE_PAD = 0.0625f;                          // RAYCAST_PAD of raycast.hip: the twin of raycast_classify's `low`
constexpr double INSIDE_FILTER = 3.3306690738754716e-16;       // (3 + 16 e) e, e = 2^-53: Shewchuk's stage-A bound of orient2d

struct InsideParams {
    int groups, V, T;
    float origin[3], cell[3];
    int cells[3];
    int C, C1;                    // cells per group, lists per group (C + 1)
    int max_references;
    int points_n, point_blocks;   // per group
    const float* vertices; const int32_t* triangles;
    const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    const int32_t* cell_offsets; const int32_t* references;
    const float* points;
    int32_t* winding; int32_t* crossings;
};

// s + e = a + b exactly (Knuth; no branch, no condition on the magnitudes)
__device__ __forceinline__ void in_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// The sign of the exact value of E = (v_i - u_i) (p_j - u_j) - (v_j - u_j) (p_i - u_i), fp32 inputs, with the header's tie rule.
// Filter: E in float64 against its forward error bound.  Fallback: the six products of the expanded determinant (the two u_i u_j
// cancel) are products of two 24-bit significands - exact in a double, and far from its exponent limits -; they are summed into a
// non-overlapping expansion by Shewchuk's grow-expansion (1 + 2 + 3 + 4 + 5 error-free additions), whose highest non-zero component
// has the sign of the sum.
__device__ __forceinline__ int in_edge_sign(float ui, float uj, float vi, float vj, float pi, float pj) {
    const double dui = (double)ui, duj = (double)uj, dvi = (double)vi, dvj = (double)vj, dpi = (double)pi, dpj = (double)pj;
    const double left = (dvi - dui) * (dpj - duj), right = (dvj - duj) * (dpi - dui);
    const double det = left - right;
    const double bound = INSIDE_FILTER * (fabs(left) + fabs(right));
    if (det > bound) return 1;
    if (-det > bound) return -1;
    const double t[6] = {dvi * dpj, -(dvi * duj), -(dui * dpj), -(dvj * dpi), dvj * dui, duj * dpi};
    double h[6] = {t[0], 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int n = 1; n < 6; ++n) {
        double q = t[n];
#pragma unroll
        for (int m = 0; m < n; ++m) {
            double sum, err;
            in_two_sum(q, h[m], sum, err);
            h[m] = err;
            q = sum;
        }
        h[n] = q;
    }
    double top = h[0];
#pragma unroll
    for (int n = 1; n < 6; ++n) top = h[n] != 0.0 ? h[n] : top;
    if (top > 0.0) return 1;
    if (top < 0.0) return -1;
    if (uj != vj) return uj > vj ? 1 : -1;                              // E = 0: the perturbation (p_i + eps, p_j + eps^2)
    if (vi != ui) return vi > ui ? 1 : -1;
    return 0;
}

// One candidate of the rule against p; K is the ray's axis.  A triangle read from the list of cell m of the column (`tight`) is summed
// only where m = max(lo_k, start): lo_k, the low cell of its padded box on axis K, is recomputed with the expression of
// raycast_classify (raycast.hip), its twin - the same three quotients, the same minimum, the same pad, the same cast.
template <int K>
__device__ __forceinline__ void inside_test(const InsideParams& s, const PR_GLOBAL_AS float* vertices, int vsize,
                                            const PR_GLOBAL_AS int32_t* triangles, int index, const float* p, bool tight, int m, int start,
                                            int& winding, int& crossings) {
    constexpr int I = (K + 1) % 3, J = (K + 2) % 3;
    const PR_GLOBAL_AS int32_t* tri = triangles + (size_t)index * 3;
    const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
    if (i0 < 0 || i0 >= vsize || i1 < 0 || i1 >= vsize || i2 < 0 || i2 >= vsize) return;
    float a[3], b[3], c[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        a[x] = vertices[(size_t)i0 * 3 + x];
        b[x] = vertices[(size_t)i1 * 3 + x];
        c[x] = vertices[(size_t)i2 * 3 + x];
    }
    if (tight) {                                                        // summed once per column: in the cell max(lo_k, start)
        const float ga = __fdiv_rn(__fsub_rn(a[K], s.origin[K]), s.cell[K]);
        const float gb = __fdiv_rn(__fsub_rn(b[K], s.origin[K]), s.cell[K]);
        const float gc = __fdiv_rn(__fsub_rn(c[K], s.origin[K]), s.cell[K]);
        const float low = __fsub_rn(fminf(fminf(ga, gb), gc), INSIDE_PAD);
        if (!(low >= 0.f && low <= (float)s.cells[K])) return;          // (not tight in this grid: a stale list)
        if (m != max((int)low, start)) return;
    }
    if ((a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) || (a[0] == c[0] && a[1] == c[1] && a[2] == c[2])) return;      // dead
    bool finite = true;
#pragma unroll
    for (int x = 0; x < 3; ++x) finite = finite && mesh_finite(a[x]) && mesh_finite(b[x]) && mesh_finite(c[x]);
    if (!finite) return;
    // exact rejections (closed intervals)
    if (p[I] < fminf(fminf(a[I], b[I]), c[I]) || p[I] > fmaxf(fmaxf(a[I], b[I]), c[I])) return;
    if (p[J] < fminf(fminf(a[J], b[J]), c[J]) || p[J] > fmaxf(fmaxf(a[J], b[J]), c[J])) return;
    if (fmaxf(fmaxf(a[K], b[K]), c[K]) <= p[K]) return;
    const int o = in_edge_sign(a[I], a[J], b[I], b[J], p[I], p[J]);
    if (o == 0) return;
    if (in_edge_sign(b[I], b[J], c[I], c[J], p[I], p[J]) != o) return;
    if (in_edge_sign(c[I], c[J], a[I], a[J], p[I], p[J]) != o) return;
    // the ahead test in float64, in the header's order
    double e1[3], e2[3], d[3], n[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        e1[x] = (double)b[x] - (double)a[x];
        e2[x] = (double)c[x] - (double)a[x];
        d[x] = (double)p[x] - (double)a[x];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double S = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    const bool ahead = o > 0 ? S < 0.0 : S > 0.0;
    if (!ahead) return;
    winding += o;
    crossings += 1;
}

template <int K>
__global__ __launch_bounds__(256) void k_inside_query(InsideParams s) {
    constexpr int I = (K + 1) % 3, J = (K + 2) % 3;
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
    int winding = 0, crossings = 0;
    auto test_list = [&](int list, bool tight, int m, int start) {
        const int begin = max(offsets[list], 0), end = min(offsets[list + 1], s.max_references);
        for (int r = begin; r < end; ++r) {
            const int index = as_global(s.references)[r];
            if (index >= 0 && index < tsize) inside_test<K>(s, vertices, vsize, triangles, index, p, tight, m, start, winding, crossings);
        }
    };
    // A point with a component that is not finite tests nothing.
    if (finite) {
        test_list(s.C, false, 0, 0);
        const float gi = __fdiv_rn(__fsub_rn(p[I], s.origin[I]), s.cell[I]);
        const float gj = __fdiv_rn(__fsub_rn(p[J], s.origin[J]), s.cell[J]);
        const float gk = __fdiv_rn(__fsub_rn(p[K], s.origin[K]), s.cell[K]);
        if (gi >= 0.f && gi < (float)s.cells[I] && gj >= 0.f && gj < (float)s.cells[J] && gk < (float)s.cells[K]) {
            int at[3];
            at[I] = (int)gi;
            at[J] = (int)gj;
            const int start = gk >= 0.f ? (int)gk : 0;                  // max(s_k, 0)
            for (int m = start; m < s.cells[K]; ++m) {
                at[K] = m;
                test_list((at[0] * s.cells[1] + at[1]) * s.cells[2] + at[2], true, m, start);
            }
        }
    }
    as_global(s.winding)[row] = winding;
    if (s.crossings) as_global(s.crossings)[row] = crossings;
}


}  // namespace pr

extern "C" int pr_inside_query(const pr_inside_t* s, void* stream) {
    using namespace pr;
    const char* who = "pr_inside_query";
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
    PR_REQUIRE(s->axis >= 0 && s->axis <= 2, "%s: axis %d (0, 1 or 2)", who, s->axis);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->max_references >= 0, "%s: negative capacity (max_references %d)", who, s->max_references);
    PR_REQUIRE(s->count >= 0, "%s: negative point count (count %d)", who, s->count);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->cell_offsets != nullptr, "%s: NULL cell_offsets", who);
    PR_REQUIRE(s->references || s->max_references == 0, "%s: NULL references with max_references %d", who, s->max_references);
    PR_REQUIRE(s->points != nullptr, "%s: NULL points", who);
    PR_REQUIRE(s->winding != nullptr, "%s: NULL winding (always written)", who);
    const double G = (double)s->groups;
    PR_REQUIRE((double)s->total_triangles + 256.0 * G < 2147483648.0 && G * (cells + 1.0) + 256.0 < 2147483648.0 &&
                   G * ((double)s->count + 256.0) < 2147483648.0,
               "%s: too large: total_triangles + 256 groups, groups x (cells + 1) + 256 and groups x (count + 256) must stay below 2^31 "
               "(the counts are int32)", who);
    if (s->count == 0) return PR_OK;
    InsideParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    for (int a = 0; a < 3; ++a) {
        p.origin[a] = s->origin[a];
        p.cell[a] = s->cell[a];
        p.cells[a] = s->cells[a];
    }
    p.C = (int)cells;
    p.C1 = p.C + 1;
    p.max_references = s->references ? s->max_references : 0;
    p.points_n = s->count;
    p.point_blocks = (s->count + 255) / 256;
    p.vertices = s->vertices;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.cell_offsets = s->cell_offsets;
    p.references = s->references;
    p.points = s->points;
    p.winding = s->winding;
    p.crossings = s->crossings;
    const dim3 blocks((unsigned)(s->groups * p.point_blocks));
    if (s->axis == 0) hipLaunchKernelGGL(k_inside_query<0>, blocks, dim3(256), 0, (hipStream_t)stream, p);
    else if (s->axis == 1) hipLaunchKernelGGL(k_inside_query<1>, blocks, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(k_inside_query<2>, blocks, dim3(256), 0, (hipStream_t)stream, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
