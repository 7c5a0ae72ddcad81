// Closest-hit ray queries against packed triangle meshes on a uniform cell grid (pr_raycast_build / pr_raycast_query,
// include/playrender.h states the rule; DESIGN.md 21 holds the exactness argument).
//
// Build, six launches on the caller's stream (seven when emitting), all kernels:
//   k_raycast_init      zeroes the per-(group, cell) counts
//   k_raycast_groups    one lane: the clamped per-group offsets and the first triangle block of every group
//   k_raycast_bin       per triangle: its class (dead, loose, tight) and, tight, the cells its padded box overlaps; one integer
//                       atomic per (triangle, cell) on the cell's count
//   k_raycast_mark      per 256 cells: the block sum of the counts                       -> k_scan_blocks_group
//   k_raycast_offsets   per cell: cell_offsets, and the same value as the cell's cursor (replaces the count)
//   k_raycast_bin       (emitting, not launched without `references`) per (triangle, cell): the cursor's next slot receives the
//                       triangle.  The order inside a cell is the order of arrival; the query takes a minimum.
// Lanes: one per triangle, 256-lane blocks that never span two groups (the block table of mesh_dev.h).  A triangle that overlaps
// many cells is a serial loop in its lane.  Every group has C + 1 lists: its C cells and, last, the loose list that every ray of the
// group tests.
//
// Query, one launch: k_raycast_query, one lane per ray, wave64.  The lane tests the loose list, clips the ray to the grid's box and
// walks the cells front to back (3D-DDA in cell units); every plane-crossing time is computed from the plane's integer index, so no
// error accumulates along the walk.  No lane waits for another, no LDS, no atomics.
#include "mesh_dev.h"

#include <math.h>

namespace pr {

constexpr float RAYCAST_PAD = 0.0625f;                 // a sixteenth of a cell around every triangle's box
constexpr float RAYCAST_SLIVER = 9.5367431640625e-07f; // 2^-20: |e1 x e2|^2 at or below this fraction of |e1|^2 |e2|^2 is a sliver

struct RaycastParams {
    int groups, V, T;
    int cull;
    float origin[3], cell[3];
    int cells[3];
    int C, C1;                    // cells per group, lists per group (C + 1)
    int lists;                    // groups x C1
    int BT;                       // launched triangle blocks
    int NB;                       // blocks of 256 lists
    int max_references;
    int rays, ray_blocks;         // per group
    float t_min, t_max;
    const float* vertices; const int32_t* triangles;
    const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    int32_t* cell_offsets; int32_t* references;
    const float* origins; const float* directions;
    float* t; int32_t* triangle; float* barycentric;
    // workspace (build)
    int32_t* cnt;                 // (G, C1) triangles of the list, then (k_raycast_offsets) the list's cursor
    int32_t* vfirst; int32_t* tfirst; int32_t* tblk;       // (G + 1) clamped offsets, first triangle block
    int32_t* bsum; int32_t* boff; // (NB)
    int32_t* total;               // [R]
};

__global__ __launch_bounds__(256) void k_raycast_init(RaycastParams s) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)s.lists; i += stride) as_global(s.cnt)[i] = 0;
}

// One lane, serial over the groups: offsets that leave [0, total] or decrease are clamped (the rule: mesh_dev.h).
__global__ __launch_bounds__(64) void k_raycast_groups(RaycastParams s) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int v = 0, t = 0, tb = 0;
    for (int g = 0; g <= s.groups; ++g) {
        const int t_before = t;
        v = min(s.V, max(v, as_global(s.vertex_offsets)[g]));
        t = min(s.T, max(t, as_global(s.triangle_offsets)[g]));
        if (g > 0) tb += (t - t_before + 255) / 256;
        as_global(s.vfirst)[g] = v;
        as_global(s.tfirst)[g] = t;
        as_global(s.tblk)[g] = tb;
    }
}

// Class of a triangle and, tight, its inclusive cell range.  0: dead (never accepted by any finite ray: an index outside [0, V_g),
// or a == b or a == c as values, which makes det exactly zero), 1: loose (a vertex that is not finite, a sliver, or a padded box that
// is not inside the grid's box: every comparison below is false on a NaN, which lands here), 2: tight.
__device__ __forceinline__ int raycast_classify(const RaycastParams& s, const PR_GLOBAL_AS float* vertices, int vsize,
                                                const PR_GLOBAL_AS int32_t* tri, int* lo, int* hi) {
    const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
    if (i0 < 0 || i0 >= vsize || i1 < 0 || i1 >= vsize || i2 < 0 || i2 >= vsize) return 0;
    float a[3], b[3], c[3], e1[3], e2[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = vertices[(size_t)i0 * 3 + k];
        b[k] = vertices[(size_t)i1 * 3 + k];
        c[k] = vertices[(size_t)i2 * 3 + k];
    }
    if ((a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) || (a[0] == c[0] && a[1] == c[1] && a[2] == c[2])) return 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = __fsub_rn(b[k], a[k]);
        e2[k] = __fsub_rn(c[k], a[k]);
    }
    mesh_cross(e1, e2, n);
    const bool shaped = mesh_dot(n, n) > __fmul_rn(RAYCAST_SLIVER, __fmul_rn(mesh_dot(e1, e1), mesh_dot(e2, e2)));
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float ga = __fdiv_rn(__fsub_rn(a[k], s.origin[k]), s.cell[k]);
        const float gb = __fdiv_rn(__fsub_rn(b[k], s.origin[k]), s.cell[k]);
        const float gc = __fdiv_rn(__fsub_rn(c[k], s.origin[k]), s.cell[k]);
        const float low = __fsub_rn(fminf(fminf(ga, gb), gc), RAYCAST_PAD);
        const float high = __fadd_rn(fmaxf(fmaxf(ga, gb), gc), RAYCAST_PAD);
        const bool ok = mesh_finite(ga) && mesh_finite(gb) && mesh_finite(gc) && low >= 0.f && high <= (float)s.cells[k];
        inside = inside && ok;
        lo[k] = ok ? (int)low : 0;                                  // (0 <= low <= high <= cells: the casts truncate = floor)
        hi[k] = ok ? min((int)high, s.cells[k] - 1) : 0;
    }
    return shaped && inside ? 2 : 1;
}

// Counting (fill == 0): one atomic increment per (triangle, list).  Emitting (fill == 1): the cursor's next slot receives the triangle.
__global__ __launch_bounds__(256) void k_raycast_bin(RaycastParams s, int fill) {
    const int b = (int)blockIdx.x;
    const PR_GLOBAL_AS int32_t* table = as_global(s.tblk);
    if (b >= table[s.groups]) return;           // (the whole block: it lies behind the last group)
    int g = 0, top = s.groups;                  // table[g] <= b < table[top]
    while (top - g > 1) {
        const int mid = (g + top) >> 1;
        if (table[mid] <= b) g = mid;
        else top = mid;
    }
    const int tfirst = as_global(s.tfirst)[g], tsize = as_global(s.tfirst)[g + 1] - tfirst;
    const int vfirst = as_global(s.vfirst)[g], vsize = as_global(s.vfirst)[g + 1] - vfirst;
    const int local = (b - table[g]) * 256 + (int)threadIdx.x;
    if (local >= tsize) return;
    int lo[3], hi[3];
    const int kind = raycast_classify(s, as_global(s.vertices) + (size_t)vfirst * 3, vsize,
                                      as_global(s.triangles) + ((size_t)tfirst + local) * 3, lo, hi);
    if (kind == 0) return;
    PR_GLOBAL_AS int32_t* lists = as_global(s.cnt) + (size_t)g * s.C1;
    auto put = [&](int list) {
        const int at = __hip_atomic_fetch_add(lists + list, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fill && at >= 0 && at < s.max_references) as_global(s.references)[at] = local;
    };
    if (kind == 1) {
        put(s.C);
        return;
    }
    for (int x = lo[0]; x <= hi[0]; ++x)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int z = lo[2]; z <= hi[2]; ++z) put((x * s.cells[1] + y) * s.cells[2] + z);
}

__global__ __launch_bounds__(256) void k_raycast_mark(RaycastParams s) {
    __shared__ int lds[4];
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    int total;
    block_exclusive_scan_256(i < s.lists ? as_global(s.cnt)[i] : 0, lds, &total);
    if (threadIdx.x == 0) as_global(s.bsum)[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_raycast_offsets(RaycastParams s) {
    __shared__ int lds[4];
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const bool live = i < s.lists;
    int total;
    const int at = as_global(s.boff)[blockIdx.x] + block_exclusive_scan_256(live ? as_global(s.cnt)[i] : 0, lds, &total);
    if (live) {
        as_global(s.cell_offsets)[i] = at;
        as_global(s.cnt)[i] = at;
    }
    if (i == s.lists) as_global(s.cell_offsets)[i] = at;          // (the lists behind the last one count 0: this is R)
}

struct RaycastHit { float t, u, v; int index; };

// Moeller-Trumbore with divisions, every operation written out (the header's rule); a better (t, index) replaces `best`.
__device__ __forceinline__ void raycast_test(const RaycastParams& s, const PR_GLOBAL_AS float* vertices, int vsize,
                                             const PR_GLOBAL_AS int32_t* triangles, int index, const float* o, const float* d,
                                             RaycastHit& best) {
    const PR_GLOBAL_AS int32_t* tri = triangles + (size_t)index * 3;
    const int i0 = tri[0], i1 = tri[1], i2 = tri[2];
    if (i0 < 0 || i0 >= vsize || i1 < 0 || i1 >= vsize || i2 < 0 || i2 >= vsize) return;
    float a[3], e1[3], e2[3], sv[3], p[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = vertices[(size_t)i0 * 3 + k];
        e1[k] = __fsub_rn(vertices[(size_t)i1 * 3 + k], a[k]);
        e2[k] = __fsub_rn(vertices[(size_t)i2 * 3 + k], a[k]);
        sv[k] = __fsub_rn(o[k], a[k]);
    }
    mesh_cross(d, e2, p);
    const float det = mesh_dot(e1, p);
    if (!(det > 0.f || (!s.cull && det < 0.f))) return;
    const float u = __fdiv_rn(mesh_dot(sv, p), det);
    mesh_cross(sv, e1, q);
    const float v = __fdiv_rn(mesh_dot(d, q), det);
    const float t = __fdiv_rn(mesh_dot(e2, q), det);
    if (!(u >= 0.f && v >= 0.f && __fadd_rn(u, v) <= 1.f && t >= s.t_min && t <= s.t_max)) return;
    if (t < best.t || (t == best.t && index < best.index) || best.index < 0) {
        best.t = t;
        best.u = u;
        best.v = v;
        best.index = index;
    }
}

__global__ __launch_bounds__(256) void k_raycast_query(RaycastParams s) {
    const int g = (int)blockIdx.x / s.ray_blocks;
    const int ray = ((int)blockIdx.x - g * s.ray_blocks) * 256 + (int)threadIdx.x;
    if (ray >= s.rays) return;
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
    const size_t row = (size_t)g * s.rays + ray;
    float o[3], d[3], og[3], dg[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = as_global(s.origins)[row * 3 + a];
        d[a] = as_global(s.directions)[row * 3 + a];
        og[a] = __fdiv_rn(__fsub_rn(o[a], s.origin[a]), s.cell[a]);
        dg[a] = __fdiv_rn(d[a], s.cell[a]);
        finite = finite && mesh_finite(o[a]) && mesh_finite(d[a]);
    }
    RaycastHit best = {INFINITY, 0.f, 0.f, -1};
    auto test_list = [&](int list) {
        const int begin = max(offsets[list], 0), end = min(offsets[list + 1], s.max_references);
        for (int r = begin; r < end; ++r) {
            const int index = as_global(s.references)[r];
            if (index >= 0 && index < tsize) raycast_test(s, vertices, vsize, triangles, index, o, d, best);
        }
    };
    // A ray with a component that is not finite, or with the direction (0, 0, 0), is accepted by no triangle.
    if (finite && (d[0] != 0.f || d[1] != 0.f || d[2] != 0.f)) {
        test_list(s.C);
        bool walk = mesh_finite(og[0]) && mesh_finite(og[1]) && mesh_finite(og[2]) && mesh_finite(dg[0]) && mesh_finite(dg[1]) && mesh_finite(dg[2]);
        float tlo = s.t_min, thi = s.t_max;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float top = (float)s.cells[a];
            if (dg[a] != 0.f) {
                const float ta = __fdiv_rn(__fsub_rn(0.f, og[a]), dg[a]), tb = __fdiv_rn(__fsub_rn(top, og[a]), dg[a]);
                tlo = fmaxf(tlo, fminf(ta, tb));
                thi = fminf(thi, fmaxf(ta, tb));
            } else if (!(og[a] >= 0.f && og[a] <= top)) {
                walk = false;
            }
        }
        if (walk && tlo <= thi) {
            int i[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float at = __fadd_rn(og[a], __fmul_rn(tlo, dg[a]));
                const float last = (float)(s.cells[a] - 1);
                if (!(at >= 0.f)) at = 0.f;
                if (at > last) at = last;
                i[a] = (int)at;
            }
            const int most = s.cells[0] + s.cells[1] + s.cells[2];
            for (int step = 0; step <= most; ++step) {
                float tout = INFINITY;
                int axis = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (dg[a] != 0.f) {
                        const float plane = (float)(i[a] + (dg[a] > 0.f ? 1 : 0));
                        const float te = __fdiv_rn(__fsub_rn(plane, og[a]), dg[a]);
                        if (te < tout) {
                            tout = te;
                            axis = a;
                        }
                    }
                }
                test_list((i[0] * s.cells[1] + i[1]) * s.cells[2] + i[2]);
                if (best.t <= tout || !(tout < thi)) break;        // every t up to tout has been covered by a visited cell
                const int next = i[axis] + (dg[axis] > 0.f ? 1 : -1);
                if (next < 0 || next >= s.cells[axis]) break;
                i[axis] = next;
            }
        }
    }
    as_global(s.t)[row] = best.t;
    if (s.triangle) as_global(s.triangle)[row] = best.index;
    if (s.barycentric) {
        as_global(s.barycentric)[row * 2 + 0] = best.u;
        as_global(s.barycentric)[row * 2 + 1] = best.v;
    }
}

struct RaycastPlan {
    size_t cnt, vfirst, tfirst, tblk, bsum, boff, total, bytes;
    int C, C1, lists, BT, NB;
};

// Host checks shared by the three entry points: no device work.
static int plan_raycast(const pr_raycast_t* s, const char* who, RaycastPlan* plan) {
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
    PR_REQUIRE((s->flags & ~PR_RAYCAST_CULL_BACK) == 0, "%s: flags 0x%x (PR_RAYCAST_CULL_BACK or 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->max_references >= 0, "%s: negative capacity (max_references %d)", who, s->max_references);
    PR_REQUIRE(s->rays >= 0, "%s: negative ray count (rays %d)", who, s->rays);
    PR_REQUIRE(s->t_min == s->t_min && s->t_max == s->t_max, "%s: NaN window (t_min %g, t_max %g)", who, (double)s->t_min,
               (double)s->t_max);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->cell_offsets != nullptr, "%s: NULL cell_offsets", who);
    const double G = (double)s->groups;
    PR_REQUIRE((double)s->total_triangles + 256.0 * G < 2147483648.0 && G * (cells + 1.0) + 256.0 < 2147483648.0 &&
                   G * ((double)s->rays + 256.0) < 2147483648.0,
               "%s: too large: total_triangles + 256 groups, groups x (cells + 1) + 256 and groups x (rays + 256) must stay below 2^31 "
               "(the counts are int32)", who);
    plan->C = (int)cells;
    plan->C1 = plan->C + 1;
    plan->lists = s->groups * plan->C1;
    plan->BT = (s->total_triangles + 255) / 256 + s->groups;
    plan->NB = plan->lists / 256 + 1;                      // (covers the element behind the last list, which receives R)
    const size_t table = ((size_t)s->groups + 1) * sizeof(int32_t);
    size_t at = 0;
    plan->cnt = workspace_region(&at, 4 * (size_t)plan->lists);
    plan->vfirst = workspace_region(&at, table);
    plan->tfirst = workspace_region(&at, table);
    plan->tblk = workspace_region(&at, table);
    plan->bsum = workspace_region(&at, 4 * (size_t)plan->NB);
    plan->boff = workspace_region(&at, 4 * (size_t)plan->NB);
    plan->total = workspace_region(&at, sizeof(int32_t));
    plan->bytes = at;
    return PR_OK;
}

static void raycast_params(const pr_raycast_t* s, const RaycastPlan& plan, RaycastParams* p) {
    memset(p, 0, sizeof(*p));
    p->groups = s->groups;
    p->V = s->total_vertices;
    p->T = s->total_triangles;
    p->cull = (s->flags & PR_RAYCAST_CULL_BACK) ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        p->origin[a] = s->origin[a];
        p->cell[a] = s->cell[a];
        p->cells[a] = s->cells[a];
    }
    p->C = plan.C;
    p->C1 = plan.C1;
    p->lists = plan.lists;
    p->BT = plan.BT;
    p->NB = plan.NB;
    p->max_references = s->references ? s->max_references : 0;
    p->rays = s->rays;
    p->ray_blocks = (s->rays + 255) / 256;
    p->t_min = s->t_min;
    p->t_max = s->t_max;
    p->vertices = s->vertices;
    p->triangles = s->triangles;
    p->vertex_offsets = s->vertex_offsets;
    p->triangle_offsets = s->triangle_offsets;
    p->cell_offsets = s->cell_offsets;
    p->references = s->references;
    p->origins = s->origins;
    p->directions = s->directions;
    p->t = s->t;
    p->triangle = s->triangle;
    p->barycentric = s->barycentric;
}

}  // namespace pr

extern "C" int pr_raycast_workspace_size(const pr_raycast_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_raycast_workspace_size: NULL bytes");
    pr::RaycastPlan plan;
    PR_TRY(pr::plan_raycast(s, "pr_raycast_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_raycast_build(const pr_raycast_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    RaycastPlan plan;
    PR_TRY(plan_raycast(s, "pr_raycast_build", &plan));
    PR_TRY(check_workspace("pr_raycast_build", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    RaycastParams p;
    raycast_params(s, plan, &p);
    p.cnt = (int32_t*)(ws + plan.cnt);
    p.vfirst = (int32_t*)(ws + plan.vfirst);
    p.tfirst = (int32_t*)(ws + plan.tfirst);
    p.tblk = (int32_t*)(ws + plan.tblk);
    p.bsum = (int32_t*)(ws + plan.bsum);
    p.boff = (int32_t*)(ws + plan.boff);
    p.total = (int32_t*)(ws + plan.total);
    const unsigned init_grid = (unsigned)(plan.NB < 65536 ? plan.NB : 65536);
    hipLaunchKernelGGL(k_raycast_init, dim3(init_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_raycast_groups, dim3(1), dim3(64), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_raycast_bin, dim3((unsigned)plan.BT), dim3(256), 0, st, p, 0);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_raycast_mark, dim3((unsigned)plan.NB), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    {
        const int32_t* sums[1] = {p.bsum};
        int32_t* offsets[1] = {p.boff};
        int32_t* totals[1] = {p.total};
        PR_TRY(launch_scan_group(sums, offsets, totals, 1, plan.NB, st));
    }
    hipLaunchKernelGGL(k_raycast_offsets, dim3((unsigned)plan.NB), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (s->references && s->max_references > 0) {
        hipLaunchKernelGGL(k_raycast_bin, dim3((unsigned)plan.BT), dim3(256), 0, st, p, 1);
        PR_LAUNCH_CHECK();
    }
    return PR_OK;
}

extern "C" int pr_raycast_query(const pr_raycast_t* s, void* stream) {
    using namespace pr;
    RaycastPlan plan;
    PR_TRY(plan_raycast(s, "pr_raycast_query", &plan));
    PR_REQUIRE(s->t != nullptr, "pr_raycast_query: NULL t (always written)");
    PR_REQUIRE(!s->barycentric || s->triangle, "pr_raycast_query: barycentric needs triangle");
    PR_REQUIRE(s->references || s->max_references == 0, "pr_raycast_query: NULL references with max_references %d", s->max_references);
    PR_REQUIRE(s->origins && s->directions, "pr_raycast_query: NULL rays (origins / directions)");
    if (s->rays == 0) return PR_OK;
    RaycastParams p;
    raycast_params(s, plan, &p);
    hipLaunchKernelGGL(k_raycast_query, dim3((unsigned)(s->groups * p.ray_blocks)), dim3(256), 0, (hipStream_t)stream, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
