// Triangle meshes of density lattices (pr_extract_surface, include/playrender.h): marching tetrahedra on the Freudenthal (Kuhn)
// split of every lattice cube.  Degenerate by design: a lattice value exactly equal to `level` is outside, the vertices of the
// edges that end there coincide and some triangles have zero area - they are kept, the mesh stays topologically closed.
//
// Five launches on the caller's stream, all kernels: k_surface_classify (crossing mask per point, triangle count per cube, two
// block sums), the block scan of both sums (k_scan_blocks_group), k_surface_offsets (the per-group offsets and the totals),
// k_surface_vertices (vertex base per point, positions, normals), k_surface_triangles (indices).  A count-only call ends behind
// the third.  Lanes: one per lattice point, 256-lane blocks that never span two groups.
#include "mesh_dev.h"

namespace pr {

// Edge direction d = 0..6 leaves a point along (DX, DY, DZ) bit d: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).
// Cube corner c: 0 = the origin, c = d + 1 = the far end of direction d.
constexpr unsigned DX_BITS = 0x59, DY_BITS = 0x6A, DZ_BITS = 0x74;

// The case table, generated from the rule (never typed in).  Tetrahedron t belongs to the t-th axis permutation p in
// lexicographic order and has the corners v0 = 0, v1 = e_p0, v2 = v1 + e_p1, v3 = (1,1,1); case bit i = v_i inside.
//   one corner a alone on its side: one triangle on the edges (a, b), b ascending;
//   two inside a < b, two outside c < d: the quad (a,c) (a,d) (b,d) (b,c) as (q0,q1,q2) (q0,q2,q3).
// Orientation, per triangle, with every crossing at its edge midpoint (integers): the normal (P1 - P0) x (P2 - P0) must have a
// positive dot product with |inside| sum(outside corners) - |outside| sum(inside corners); otherwise the last two entries swap.
// row[t][case]: bits 0-1 = triangles, entry e = 0..5 (triangle e / 3) at bits 4 + 6 e: cube corner of the edge's lower end (3 bits),
// direction (3 bits).  corner[t][i]: cube corner of v_i.
struct SurfaceTable {
    unsigned long long row[6][16];
    unsigned char corner[6][4];
};

constexpr int surface_corner_of(int x, int y, int z) {     // cube corner of an offset in {0,1}^3
    for (int d = 0; d < 7; ++d)
        if ((int)(DX_BITS >> d & 1) == x && (int)(DY_BITS >> d & 1) == y && (int)(DZ_BITS >> d & 1) == z) return d + 1;
    return 0;
}

constexpr SurfaceTable make_surface_table() {
    SurfaceTable T = {};
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int t = 0; t < 6; ++t) {
        int v[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}};
        v[1][perms[t][0]] = 1;
        v[2][perms[t][0]] = 1;
        v[2][perms[t][1]] = 1;
        for (int i = 0; i < 4; ++i) T.corner[t][i] = (unsigned char)surface_corner_of(v[i][0], v[i][1], v[i][2]);
        for (int mask = 0; mask < 16; ++mask) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int i = 0; i < 4; ++i) {
                if (mask >> i & 1) in[ni++] = i;
                else out[no++] = i;
            }
            int tri[2][3][2] = {};        // [triangle][entry][edge end]
            int count = 0;
            if (ni == 1 || ni == 3) {
                const int lone = ni == 1 ? in[0] : out[0];
                int e = 0;
                for (int b = 0; b < 4; ++b)
                    if (b != lone) {
                        tri[0][e][0] = lone;
                        tri[0][e][1] = b;
                        ++e;
                    }
                count = 1;
            } else if (ni == 2) {
                const int q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                for (int k = 0; k < 2; ++k)
                    for (int e = 0; e < 3; ++e) {
                        tri[k][e][0] = q[pick[k][e]][0];
                        tri[k][e][1] = q[pick[k][e]][1];
                    }
                count = 2;
            }
            int outward[3] = {};
            for (int a = 0; a < 3; ++a) {
                for (int i = 0; i < no; ++i) outward[a] += ni * v[out[i]][a];
                for (int i = 0; i < ni; ++i) outward[a] -= no * v[in[i]][a];
            }
            unsigned long long row = (unsigned long long)count;
            for (int k = 0; k < count; ++k) {
                int P[3][3] = {};         // twice the midpoints
                for (int e = 0; e < 3; ++e)
                    for (int a = 0; a < 3; ++a) P[e][a] = v[tri[k][e][0]][a] + v[tri[k][e][1]][a];
                int u[3] = {}, w[3] = {};
                for (int a = 0; a < 3; ++a) {
                    u[a] = P[1][a] - P[0][a];
                    w[a] = P[2][a] - P[0][a];
                }
                const int dot = (u[1] * w[2] - u[2] * w[1]) * outward[0] + (u[2] * w[0] - u[0] * w[2]) * outward[1] +
                                (u[0] * w[1] - u[1] * w[0]) * outward[2];
                const int order[3] = {0, dot > 0 ? 1 : 2, dot > 0 ? 2 : 1};
                for (int e = 0; e < 3; ++e) {
                    const int a = tri[k][order[e]][0], b = tri[k][order[e]][1];
                    const int lo = a < b ? a : b, hi = a < b ? b : a;          // the corners form a chain: the lower index is the lower end
                    const int d = surface_corner_of(v[hi][0] - v[lo][0], v[hi][1] - v[lo][1], v[hi][2] - v[lo][2]) - 1;
                    row |= (unsigned long long)(T.corner[t][lo] | d << 3) << (4 + 6 * (3 * k + e));
                }
            }
            T.row[t][mask] = row;
        }
    }
    return T;
}

__constant__ SurfaceTable g_surface_table = make_surface_table();

struct SurfaceParams {
    int groups, nx, ny, nz;
    int points;                   // P = nx ny nz
    int blocks;                   // blocks per group, ceil(P / 256)
    float level;
    const float* sigma;           // (G, P)
    const float* ax; const float* ay; const float* az;
    int max_vertices, max_triangles;
    float* vertices; float* normals; int32_t* triangles;
    int32_t* vertex_offsets; int32_t* triangle_offsets;
    // workspace
    uint8_t* mask;                // (G, P) crossing bits of the seven edges that leave the point
    uint8_t* tcount;              // (G, P) triangles of the cube whose origin the point is (0: not an origin)
    int32_t* base;                // (G, P) first vertex of the point, local to the group
    int32_t* vsum; int32_t* tsum; // (G blocks) block sums
    int32_t* voff; int32_t* toff; // (G blocks) their exclusive scans
    int32_t* totals;              // [V, T]
};

struct SurfaceLane {
    int group, p, i, j, k;
    bool live, hx, hy, hz;        // the point exists; it has a forward neighbour along x / y / z
};

__device__ __forceinline__ SurfaceLane surface_lane(const SurfaceParams& s) {
    SurfaceLane l;
    l.group = (int)blockIdx.x / s.blocks;
    l.p = ((int)blockIdx.x - l.group * s.blocks) * 256 + (int)threadIdx.x;
    l.live = l.p < s.points;
    const int q = l.live ? l.p : 0;
    l.k = q % s.nz;
    l.j = (q / s.nz) % s.ny;
    l.i = q / (s.nz * s.ny);
    l.hx = l.live && l.i + 1 < s.nx;
    l.hy = l.live && l.j + 1 < s.ny;
    l.hz = l.live && l.k + 1 < s.nz;
    return l;
}

// offset (points) of cube corner c from the cube's origin
__device__ __forceinline__ int surface_corner_offset(const SurfaceParams& s, int c) {
    const unsigned b = 1u << c >> 1;           // bit d = c - 1, nothing for the origin
    return ((DX_BITS & b) ? s.ny * s.nz : 0) + ((DY_BITS & b) ? s.nz : 0) + ((DZ_BITS & b) ? 1 : 0);
}

__device__ __forceinline__ int surface_row_triangles(int flags) {     // triangles of the cube with the corner flags (bit c = corner c inside)
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) c |= (flags >> g_surface_table.corner[t][i] & 1) << i;
        n += (int)(g_surface_table.row[t][c] & 3ull);
    }
    return n;
}

__global__ __launch_bounds__(256) void k_surface_classify(SurfaceParams s) {
    __shared__ int lds[4];
    const SurfaceLane l = surface_lane(s);
    int mask = 0, triangles = 0;
    if (l.live) {
        const PR_GLOBAL_AS float* sig = as_global(s.sigma) + (size_t)l.group * s.points + l.p;
        const bool in0 = sig[0] > s.level;
        int flags = in0 ? 1 : 0;
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            const bool exists = (!(DX_BITS >> d & 1) || l.hx) && (!(DY_BITS >> d & 1) || l.hy) && (!(DZ_BITS >> d & 1) || l.hz);
            if (exists) {
                const bool in = sig[surface_corner_offset(s, d + 1)] > s.level;
                flags |= (in ? 1 : 0) << (d + 1);
                mask |= (in != in0 ? 1 : 0) << d;
            }
        }
        if (l.hx && l.hy && l.hz) triangles = surface_row_triangles(flags);
        const size_t at = (size_t)l.group * s.points + l.p;
        as_global(s.mask)[at] = (uint8_t)mask;
        as_global(s.tcount)[at] = (uint8_t)triangles;
    }
    int vertex_total, triangle_total;
    block_exclusive_scan_256(__popc(mask), lds, &vertex_total);
    block_exclusive_scan_256(triangles, lds, &triangle_total);
    if (threadIdx.x == 0) {
        as_global(s.vsum)[blockIdx.x] = vertex_total;
        as_global(s.tsum)[blockIdx.x] = triangle_total;
    }
}

__global__ __launch_bounds__(256) void k_surface_offsets(SurfaceParams s) {
    const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (g < s.groups) {
        as_global(s.vertex_offsets)[g] = as_global(s.voff)[(size_t)g * s.blocks];
        as_global(s.triangle_offsets)[g] = as_global(s.toff)[(size_t)g * s.blocks];
    } else if (g == s.groups) {
        as_global(s.vertex_offsets)[g] = as_global(s.totals)[0];
        as_global(s.triangle_offsets)[g] = as_global(s.totals)[1];
    }
}

// lattice gradient at point (i, j, k): per axis (s[+1] - s[-1]) / (x[+1] - x[-1]), one-sided at the two ends
__device__ __forceinline__ void surface_gradient(const SurfaceParams& s, const PR_GLOBAL_AS float* lattice, int i, int j, int k, float* g) {
    const PR_GLOBAL_AS float* c = lattice + ((size_t)i * s.ny + j) * s.nz + k;
    const int i0 = max(i - 1, 0), i1 = min(i + 1, s.nx - 1);
    const int j0 = max(j - 1, 0), j1 = min(j + 1, s.ny - 1);
    const int k0 = max(k - 1, 0), k1 = min(k + 1, s.nz - 1);
    const int sx = s.ny * s.nz, sy = s.nz;
    g[0] = __fdiv_rn(__fsub_rn(c[(i1 - i) * sx], c[(i0 - i) * sx]), __fsub_rn(as_global(s.ax)[i1], as_global(s.ax)[i0]));
    g[1] = __fdiv_rn(__fsub_rn(c[(j1 - j) * sy], c[(j0 - j) * sy]), __fsub_rn(as_global(s.ay)[j1], as_global(s.ay)[j0]));
    g[2] = __fdiv_rn(__fsub_rn(c[k1 - k], c[k0 - k]), __fsub_rn(as_global(s.az)[k1], as_global(s.az)[k0]));
}

__global__ __launch_bounds__(256) void k_surface_vertices(SurfaceParams s) {
    __shared__ int lds[4];
    const SurfaceLane l = surface_lane(s);
    const size_t at = (size_t)l.group * s.points + (l.live ? l.p : 0);
    const int mask = l.live ? as_global(s.mask)[at] : 0;
    int block_total;
    const int first_of_group = as_global(s.voff)[(size_t)l.group * s.blocks];
    int vertex = as_global(s.voff)[blockIdx.x] + block_exclusive_scan_256(__popc(mask), lds, &block_total);
    if (!l.live) return;
    as_global(s.base)[at] = vertex - first_of_group;
    if (!s.vertices || !mask) return;
    const PR_GLOBAL_AS float* lattice = as_global(s.sigma) + (size_t)l.group * s.points;
    const float sa = lattice[l.p];
    const float pa[3] = {as_global(s.ax)[l.i], as_global(s.ay)[l.j], as_global(s.az)[l.k]};
    float ga[3] = {0.f, 0.f, 0.f};
    if (s.normals) surface_gradient(s, lattice, l.i, l.j, l.k, ga);
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        if (!(mask >> d & 1)) continue;
        const int row = vertex++;
        if (row >= s.max_vertices) return;
        const int di = DX_BITS >> d & 1, dj = DY_BITS >> d & 1, dk = DZ_BITS >> d & 1;
        const float sb = lattice[l.p + surface_corner_offset(s, d + 1)];
        float t = __fdiv_rn(__fsub_rn(s.level, sa), __fsub_rn(sb, sa));
        if (!(t >= 0.f)) t = 0.f;
        if (t > 1.f) t = 1.f;
        const float pb[3] = {di ? as_global(s.ax)[l.i + 1] : pa[0], dj ? as_global(s.ay)[l.j + 1] : pa[1], dk ? as_global(s.az)[l.k + 1] : pa[2]};
        PR_GLOBAL_AS float* v = as_global(s.vertices) + (size_t)row * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = __fadd_rn(pa[a], __fmul_rn(t, __fsub_rn(pb[a], pa[a])));
        if (s.normals) {
            float gb[3], n[3];
            surface_gradient(s, lattice, l.i + di, l.j + dj, l.k + dk, gb);
#pragma unroll
            for (int a = 0; a < 3; ++a) n[a] = -__fadd_rn(ga[a], __fmul_rn(t, __fsub_rn(gb[a], ga[a])));
            const float length = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(n[0], n[0]), __fmul_rn(n[1], n[1])), __fmul_rn(n[2], n[2])));
            const bool ok = length > 0.f && length < __builtin_huge_valf();          // (a NaN length fails both)
            PR_GLOBAL_AS float* o = as_global(s.normals) + (size_t)row * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) o[a] = ok ? __fdiv_rn(n[a], length) : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void k_surface_triangles(SurfaceParams s) {
    __shared__ int lds[4];
    const SurfaceLane l = surface_lane(s);
    const size_t group_first = (size_t)l.group * s.points;
    const int count = l.live ? as_global(s.tcount)[group_first + l.p] : 0;
    int block_total;
    int triangle = as_global(s.toff)[blockIdx.x] + block_exclusive_scan_256(count, lds, &block_total);
    if (!count) return;           // (count > 0: the point is the origin of a cube, all of its corners exist)
    const PR_GLOBAL_AS uint8_t* mask = as_global(s.mask) + group_first + l.p;
    const PR_GLOBAL_AS int32_t* base = as_global(s.base) + group_first + l.p;
    // corner flags from the origin's own flag and its crossing bits
    const int m0 = mask[0];
    const int in0 = as_global(s.sigma)[group_first + l.p] > s.level ? 1 : 0;
    const int flags = (in0 ? 0xFF : 0) ^ (m0 << 1);
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) c |= (flags >> g_surface_table.corner[t][i] & 1) << i;
        const unsigned long long row = g_surface_table.row[t][c];
        const int n = (int)(row & 3ull);
        for (int k = 0; k < n; ++k) {
            const int out = triangle++;
            if (out >= s.max_triangles) return;
            PR_GLOBAL_AS int32_t* dst = as_global(s.triangles) + (size_t)out * 3;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int entry = (int)(row >> (4 + 6 * (3 * k + e))) & 63;
                const int off = surface_corner_offset(s, entry & 7), d = entry >> 3;
                dst[e] = base[off] + __popc((int)mask[off] & ((1 << d) - 1));
            }
        }
    }
}

struct SurfacePlan {
    size_t mask, tcount, base, vsum, tsum, voff, toff, totals, bytes;
    int points, blocks;
};

// Host checks of both entry points: no device work.
static int plan_surface(const pr_surface_t* s, const char* who, SurfacePlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    long points = 1;
    for (int a = 0; a < 3; ++a) {
        PR_REQUIRE(s->points[a] >= 2, "%s: points[%d] = %d (a lattice has at least 2 points per axis)", who, a, s->points[a]);
        points *= s->points[a];
        PR_REQUIRE(12.0 * (double)s->groups * (double)points < 2147483648.0,
                   "%s: lattice too large: 12 x groups x points must stay below 2^31 (the counts are int32)", who);
    }
    PR_REQUIRE(s->level == s->level, "%s: level is NaN", who);
    PR_REQUIRE(s->flags == 0, "%s: flags 0x%x (must be 0)", who, s->flags);
    PR_REQUIRE(s->sigma != nullptr, "%s: NULL sigma", who);
    PR_REQUIRE(s->axis[0] && s->axis[1] && s->axis[2], "%s: NULL axis", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets are always written)", who);
    PR_REQUIRE(s->max_vertices >= 0 && s->max_triangles >= 0, "%s: negative capacity (max_vertices %d, max_triangles %d)", who,
               s->max_vertices, s->max_triangles);
    PR_REQUIRE(!s->normals || s->vertices, "%s: normals need vertices", who);
    plan->points = (int)points;
    plan->blocks = (int)((points + 255) / 256);
    const size_t lattice = (size_t)s->groups * (size_t)points, sums = (size_t)s->groups * plan->blocks * sizeof(int32_t);
    size_t at = 0;
    plan->mask = workspace_region(&at, lattice);
    plan->tcount = workspace_region(&at, lattice);
    plan->base = workspace_region(&at, lattice * sizeof(int32_t));
    plan->vsum = workspace_region(&at, sums);
    plan->tsum = workspace_region(&at, sums);
    plan->voff = workspace_region(&at, sums);
    plan->toff = workspace_region(&at, sums);
    plan->totals = workspace_region(&at, 2 * sizeof(int32_t));
    plan->bytes = at;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_surface_workspace_size(const pr_surface_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_surface_workspace_size: NULL bytes");
    pr::SurfacePlan plan;
    PR_TRY(pr::plan_surface(s, "pr_surface_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_extract_surface(const pr_surface_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    SurfacePlan plan;
    PR_TRY(plan_surface(s, "pr_extract_surface", &plan));
    PR_TRY(check_workspace("pr_extract_surface", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    SurfaceParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.nx = s->points[0];
    p.ny = s->points[1];
    p.nz = s->points[2];
    p.points = plan.points;
    p.blocks = plan.blocks;
    p.level = s->level;
    p.sigma = s->sigma;
    p.ax = s->axis[0];
    p.ay = s->axis[1];
    p.az = s->axis[2];
    p.max_vertices = s->max_vertices;
    p.max_triangles = s->max_triangles;
    p.vertices = s->vertices;
    p.normals = s->normals;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.mask = (uint8_t*)(ws + plan.mask);
    p.tcount = (uint8_t*)(ws + plan.tcount);
    p.base = (int32_t*)(ws + plan.base);
    p.vsum = (int32_t*)(ws + plan.vsum);
    p.tsum = (int32_t*)(ws + plan.tsum);
    p.voff = (int32_t*)(ws + plan.voff);
    p.toff = (int32_t*)(ws + plan.toff);
    p.totals = (int32_t*)(ws + plan.totals);
    const unsigned grid = (unsigned)((long)s->groups * plan.blocks);
    hipLaunchKernelGGL(k_surface_classify, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    const int32_t* sums[2] = {p.vsum, p.tsum};
    int32_t* offsets[2] = {p.voff, p.toff};
    int32_t* totals[2] = {p.totals, p.totals + 1};
    PR_TRY(launch_scan_group(sums, offsets, totals, 2, (int)grid, st));
    hipLaunchKernelGGL(k_surface_offsets, dim3((unsigned)(s->groups / 256 + 1)), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (!s->vertices && !s->triangles) return PR_OK;          // count-only call
    hipLaunchKernelGGL(k_surface_vertices, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (s->triangles) {
        hipLaunchKernelGGL(k_surface_triangles, dim3(grid), dim3(256), 0, st, p);
        PR_LAUNCH_CHECK();
    }
    return PR_OK;
}
