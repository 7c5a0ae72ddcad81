// Placement of the vertices of simplified meshes by quadric error (pr_mesh_place, include/playrender.h states the rule): per cluster
// the area-weighted plane quadric of the input triangles that touch it, as nine int64 sums around the stored vertex; per merged vertex
// the regularised 3 x 3 solve by a written-out adjugate in fp64; per merged triangle whether the move turned it.
//
// Four launches on the caller's stream (three without merged triangles), all kernels:
//   k_place_init         zeroes the sums, the contribution counts and the output counts; one lane of block 0 clamps the four offset
//                        arrays and builds the four block tables (the rule: mesh_dev.h)
//   k_place_accumulate   per input triangle: valid or counted; per distinct cluster of its corners the nine coefficients; per run of
//                        equal clusters in a wave: 64-bit integer atomics into the cluster's sums
//   k_place_solve        per merged vertex: the solve, the move or the stored words; the moved / kept counts
//   k_place_turned       per merged triangle: N . N' < 0 (not launched without merged triangles)
// Lanes: one per element, wave64, 256-lane blocks that never span two groups (mesh_lane, mesh_dev.h; a triangle's checked corners are
// mesh_corners).  Integer atomics only.  fp64 with every operation written out (__d*_rn): nothing contracts.
#include "mesh_dev.h"

namespace pr {

constexpr double PLACE_QUANTUM = 68719476736.0;           // 2^36: a coefficient is summed as llrint(q 2^36)
constexpr double PLACE_UNQUANTUM = 1.0 / 68719476736.0;   // (exact)
constexpr double PLACE_LIMIT = 65536.0;                   // 2^16: a contribution with a larger coefficient is skipped
constexpr int PLACE_SUMS = 9;

struct MeshPlaceParams {
    int groups, V, T, VO, TO;
    double h, regularisation, max_move[3];
    const float* vertices; const int32_t* triangles; const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    const int32_t* vertex_map; const float* merged_vertices; const int32_t* merged_vertex_offsets;
    const int32_t* merged_triangles; const int32_t* merged_triangle_offsets;
    float* out_vertices; int32_t* counts;
    // workspace
    int32_t* vfirst; int32_t* tfirst; int32_t* mfirst; int32_t* ufirst;   // (G + 1) the offsets, clamped: input vertices, input triangles,
    int32_t* vblk; int32_t* tblk; int32_t* mblk; int32_t* ublk;           // merged vertices, merged triangles; (G + 1) first block of the group
    unsigned long long* sums;     // (VO, 9) two's complement
    int32_t* contributions;       // (VO)
};

__device__ __forceinline__ bool place_finite(double x) { return __dsub_rn(x, x) == 0.0; }

// x y - z w, a difference of two products
__device__ __forceinline__ double place_det2(double x, double y, double z, double w) { return __dsub_rn(__dmul_rn(x, y), __dmul_rn(z, w)); }
// (x0 y0 + x1 y1) + x2 y2
__device__ __forceinline__ double place_dot(double x0, double x1, double x2, double y0, double y1, double y2) {
    return __dadd_rn(__dadd_rn(__dmul_rn(x0, y0), __dmul_rn(x1, y1)), __dmul_rn(x2, y2));
}

__global__ __launch_bounds__(256) void k_place_init(MeshPlaceParams s) {
    const size_t stride = (size_t)gridDim.x * 256, at = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t sums = (size_t)PLACE_SUMS * s.VO, counts = 4 * (size_t)s.groups;
    for (size_t i = at; i < sums; i += stride) as_global(s.sums)[i] = 0ull;
    for (size_t i = at; i < (size_t)s.VO; i += stride) as_global(s.contributions)[i] = 0;
    for (size_t i = at; i < counts; i += stride) as_global(s.counts)[i] = 0;
    // One lane, serial over the groups (a handful): offsets that leave [0, total] or decrease are clamped, so that no later kernel
    // follows a bad offset out of an array; the block tables are the running sums of ceil(size / 256).
    if (at != 0) return;
    int v = 0, t = 0, m = 0, u = 0, vb = 0, tb = 0, mb = 0, ub = 0;
    for (int g = 0; g <= s.groups; ++g) {
        const int v_before = v, t_before = t, m_before = m, u_before = u;
        v = min(s.V, max(v, as_global(s.vertex_offsets)[g]));
        t = min(s.T, max(t, as_global(s.triangle_offsets)[g]));
        m = min(s.VO, max(m, as_global(s.merged_vertex_offsets)[g]));
        if (s.merged_triangles) u = min(s.TO, max(u, as_global(s.merged_triangle_offsets)[g]));
        if (g > 0) {
            vb += (v - v_before + 255) / 256;
            tb += (t - t_before + 255) / 256;
            mb += (m - m_before + 255) / 256;
            ub += (u - u_before + 255) / 256;
        }
        as_global(s.vfirst)[g] = v;
        as_global(s.tfirst)[g] = t;
        as_global(s.mfirst)[g] = m;
        as_global(s.ufirst)[g] = u;
        as_global(s.vblk)[g] = vb;
        as_global(s.tblk)[g] = tb;
        as_global(s.mblk)[g] = mb;
        as_global(s.ublk)[g] = ub;
    }
}

// The mesher lists triangles lattice cell by lattice cell, so neighbouring lanes share clusters.  A lane orders its distinct clusters
// ascending - neighbours with the same set then hold the same cluster in the same slot -, and per slot every run of equal clusters
// inside a wave is summed with a segmented scan first; only the last lane of a run goes to memory.  A coefficient is below 2^52 in
// magnitude and the sums are taken modulo 2^64: the grouping does not show in the result.
__global__ __launch_bounds__(256) void k_place_accumulate(MeshPlaceParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    int bad = 0;                              // an invalid triangle, or the skipped contributions of a valid one
    int j0 = -1, j1 = -1, j2 = -1;            // the distinct clusters of the corners, ascending, -1 behind them
    double a[3], b[3], c[3];
    size_t mfirst = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = b[k] = c[k] = 0.0;
    if (l.live) {
        const int vfirst = as_global(s.vfirst)[l.group];
        const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
        mfirst = (size_t)as_global(s.mfirst)[l.group];
        const int msize = as_global(s.mfirst)[l.group + 1] - (int)mfirst;
        const MeshCorners t = mesh_corners(s.triangles, l.first, l.local, vsize);
        bool valid = t.in_range;
        if (valid) {
            const PR_GLOBAL_AS float* v = as_global(s.vertices) + (size_t)vfirst * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = v[(size_t)t.i[0] * 3 + k], y = v[(size_t)t.i[1] * 3 + k], z = v[(size_t)t.i[2] * 3 + k];
                valid = valid && mesh_finite(x) && mesh_finite(y) && mesh_finite(z);
                a[k] = (double)x;
                b[k] = (double)y;
                c[k] = (double)z;
            }
        }
        if (!valid) bad = 1;
        else {
            const PR_GLOBAL_AS int32_t* map = as_global(s.vertex_map) + vfirst;
            int p = map[t.i[0]], q = map[t.i[1]], r = map[t.i[2]];
            if ((unsigned)p >= (unsigned)msize) p = -1;      // (a map entry out of range contributes nothing)
            if ((unsigned)q >= (unsigned)msize) q = -1;
            if ((unsigned)r >= (unsigned)msize) r = -1;
            if (q == p) q = -1;
            if (r == p || r == q) r = -1;
            // ascending with the -1 entries last: as unsigned values
            unsigned int x = (unsigned)p, y = (unsigned)q, z = (unsigned)r;
            if (x > y) { const unsigned int w = x; x = y; y = w; }
            if (y > z) { const unsigned int w = y; y = z; z = w; }
            if (x > y) { const unsigned int w = x; x = y; y = w; }
            j0 = (int)x;
            j1 = (int)y;
            j2 = (int)z;
        }
    }
    const int lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int slot = 0; slot < 3; ++slot) {
        int j = slot == 0 ? j0 : (slot == 1 ? j1 : j2);
        long long sum[PLACE_SUMS + 1];
#pragma unroll
        for (int i = 0; i <= PLACE_SUMS; ++i) sum[i] = 0;
        if (j >= 0) {
            const PR_GLOBAL_AS float* mv = as_global(s.merged_vertices) + (mfirst + (size_t)j) * 3;
            double pa[3], e1[3], e2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double m = (double)mv[k];
                pa[k] = __ddiv_rn(__dsub_rn(a[k], m), s.h);
                e1[k] = __dsub_rn(__ddiv_rn(__dsub_rn(b[k], m), s.h), pa[k]);
                e2[k] = __dsub_rn(__ddiv_rn(__dsub_rn(c[k], m), s.h), pa[k]);
            }
            const double n0 = place_det2(e1[1], e2[2], e1[2], e2[1]);
            const double n1 = place_det2(e1[2], e2[0], e1[0], e2[2]);
            const double n2 = place_det2(e1[0], e2[1], e1[1], e2[0]);
            const double L = __dsqrt_rn(place_dot(n0, n1, n2, n0, n1, n2));
            const double d = -place_dot(n0, n1, n2, pa[0], pa[1], pa[2]);
            double q[PLACE_SUMS];
            q[0] = __ddiv_rn(__dmul_rn(n0, n0), L);
            q[1] = __ddiv_rn(__dmul_rn(n0, n1), L);
            q[2] = __ddiv_rn(__dmul_rn(n0, n2), L);
            q[3] = __ddiv_rn(__dmul_rn(n1, n1), L);
            q[4] = __ddiv_rn(__dmul_rn(n1, n2), L);
            q[5] = __ddiv_rn(__dmul_rn(n2, n2), L);
            q[6] = __ddiv_rn(__dmul_rn(d, n0), L);
            q[7] = __ddiv_rn(__dmul_rn(d, n1), L);
            q[8] = __ddiv_rn(__dmul_rn(d, n2), L);
            bool good = place_finite(L) && L > 0.0;
#pragma unroll
            for (int i = 0; i < PLACE_SUMS; ++i) good = good && __builtin_fabs(q[i]) <= PLACE_LIMIT;      // (a NaN fails the comparison)
            if (good) {
#pragma unroll
                for (int i = 0; i < PLACE_SUMS; ++i) sum[i] = __double2ll_rn(__dmul_rn(q[i], PLACE_QUANTUM));
                sum[PLACE_SUMS] = 1;
            } else {
                ++bad;
                j = -1;
            }
        }
        const int before = __shfl_up(j, 1, 64), after = __shfl_down(j, 1, 64);          // (every lane takes part)
        int head = lane == 0 || before != j ? 1 : 0;                  // the lane begins a run; becomes: the sum reaches back to one
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const int head_before = __shfl_up(head, step, 64);
            long long from[PLACE_SUMS + 1];
#pragma unroll
            for (int i = 0; i <= PLACE_SUMS; ++i) from[i] = __shfl_up(sum[i], step, 64);
            if (lane >= step && !head) {
#pragma unroll
                for (int i = 0; i <= PLACE_SUMS; ++i) sum[i] += from[i];
                head = head_before;
            }
        }
        const bool last = lane == 63 || after != j;
        if (j >= 0 && last) {
            const size_t row = mfirst + (size_t)j;
#pragma unroll
            for (int i = 0; i < PLACE_SUMS; ++i)
                if (sum[i])
                    __hip_atomic_fetch_add(as_global(s.sums) + row * PLACE_SUMS + i, (unsigned long long)sum[i], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(as_global(s.contributions) + row, (int)sum[PLACE_SUMS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    int total;
    block_exclusive_scan_256(bad, lds, &total);
    if (threadIdx.x == 0 && total)
        __hip_atomic_fetch_add(as_global(s.counts) + (size_t)l.group * 4 + 2, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_place_solve(MeshPlaceParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.mblk, s.mfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    int moved = 0;
    if (l.live) {
        const size_t row = (size_t)l.first + l.local;
        const PR_GLOBAL_AS uint32_t* stored = (const PR_GLOBAL_AS uint32_t*)as_global(s.merged_vertices) + row * 3;
        uint32_t word[3] = {stored[0], stored[1], stored[2]};
        if (as_global(s.contributions)[row] > 0) {
            double S[PLACE_SUMS];
#pragma unroll
            for (int i = 0; i < PLACE_SUMS; ++i)
                S[i] = __dmul_rn((double)(long long)as_global(s.sums)[row * PLACE_SUMS + i], PLACE_UNQUANTUM);
            const double lambda = __ddiv_rn(__dmul_rn(s.regularisation, __dadd_rn(__dadd_rn(S[0], S[3]), S[5])), 3.0);
            const double m00 = __dadd_rn(S[0], lambda), m01 = S[1], m02 = S[2], m11 = __dadd_rn(S[3], lambda), m12 = S[4],
                         m22 = __dadd_rn(S[5], lambda);
            const double r0 = -S[6], r1 = -S[7], r2 = -S[8];
            const double c00 = place_det2(m11, m22, m12, m12), c01 = place_det2(m02, m12, m01, m22), c02 = place_det2(m01, m12, m02, m11);
            const double c11 = place_det2(m00, m22, m02, m02), c12 = place_det2(m01, m02, m00, m12), c22 = place_det2(m00, m11, m01, m01);
            const double det = place_dot(m00, m01, m02, c00, c01, c02);
            double y[3];
            y[0] = __ddiv_rn(place_dot(c00, c01, c02, r0, r1, r2), det);
            y[1] = __ddiv_rn(place_dot(c01, c11, c12, r0, r1, r2), det);
            y[2] = __ddiv_rn(place_dot(c02, c12, c22, r0, r1, r2), det);
            bool moves = place_finite(det) && det > 0.0;
            double t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t[k] = __dmul_rn(s.h, y[k]);
                moves = moves && place_finite(y[k]) && !(__builtin_fabs(t[k]) > s.max_move[k]);
            }
            if (moves) {
                moved = 1;
#pragma unroll
                for (int k = 0; k < 3; ++k) word[k] = __float_as_uint((float)__dadd_rn((double)__uint_as_float(word[k]), t[k]));
            }
        }
        PR_GLOBAL_AS uint32_t* out = (PR_GLOBAL_AS uint32_t*)as_global(s.out_vertices) + row * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = word[k];
    }
    int total_moved, total_kept;
    block_exclusive_scan_256(moved, lds, &total_moved);
    block_exclusive_scan_256(l.live && !moved ? 1 : 0, lds, &total_kept);
    if (threadIdx.x == 0) {
        PR_GLOBAL_AS int32_t* counts = as_global(s.counts) + (size_t)l.group * 4;
        if (total_moved) __hip_atomic_fetch_add(counts + 0, total_moved, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (total_kept) __hip_atomic_fetch_add(counts + 1, total_kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// N = (b - a) x (c - a) of the rows i of `v`, in fp64
__device__ __forceinline__ void place_normal(const PR_GLOBAL_AS float* v, const int* i, double* N) {
    double e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = (double)v[(size_t)i[0] * 3 + k];
        e1[k] = __dsub_rn((double)v[(size_t)i[1] * 3 + k], a);
        e2[k] = __dsub_rn((double)v[(size_t)i[2] * 3 + k], a);
    }
    N[0] = place_det2(e1[1], e2[2], e1[2], e2[1]);
    N[1] = place_det2(e1[2], e2[0], e1[0], e2[2]);
    N[2] = place_det2(e1[0], e2[1], e1[1], e2[0]);
}

__global__ __launch_bounds__(256) void k_place_turned(MeshPlaceParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.ublk, s.ufirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    int turned = 0;
    if (l.live) {
        const int mfirst = as_global(s.mfirst)[l.group];
        const int msize = as_global(s.mfirst)[l.group + 1] - mfirst;
        const MeshCorners t = mesh_corners(s.merged_triangles, l.first, l.local, msize);
        if (t.in_range) {
            double N[3], M[3];
            place_normal(as_global(s.merged_vertices) + (size_t)mfirst * 3, t.i, N);
            place_normal(as_global((const float*)s.out_vertices) + (size_t)mfirst * 3, t.i, M);
            turned = place_dot(N[0], N[1], N[2], M[0], M[1], M[2]) < 0.0 ? 1 : 0;
        }
    }
    int total;
    block_exclusive_scan_256(turned, lds, &total);
    if (threadIdx.x == 0 && total)
        __hip_atomic_fetch_add(as_global(s.counts) + (size_t)l.group * 4 + 3, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct MeshPlacePlan {
    size_t table[8], sums, contributions, bytes;
    int BT, BM, BU;
};

// Host checks of both entry points: no device work.
static int plan_place(const pr_mesh_place_t* s, const char* who, MeshPlacePlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    PR_REQUIRE(s->flags == 0, "%s: unknown flag bits 0x%x (0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0 && s->total_merged_vertices >= 0 && s->total_merged_triangles >= 0,
               "%s: negative total (total_vertices %d, total_triangles %d, total_merged_vertices %d, total_merged_triangles %d)", who,
               s->total_vertices, s->total_triangles, s->total_merged_vertices, s->total_merged_triangles);
    PR_REQUIRE(host_finite(s->scale) && s->scale > 0.f, "%s: scale %g (finite, > 0)", who, (double)s->scale);
    PR_REQUIRE(host_finite(s->regularisation) && s->regularisation > 0.f, "%s: regularisation %g (finite, > 0)", who,
               (double)s->regularisation);
    for (int a = 0; a < 3; ++a)
        PR_REQUIRE(host_finite(s->max_move[a]) && s->max_move[a] >= 0.f, "%s: max_move[%d] = %g (finite, >= 0)", who, a,
                   (double)s->max_move[a]);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets && s->merged_vertex_offsets,
               "%s: NULL offsets (vertex_offsets / triangle_offsets / merged_vertex_offsets)", who);
    PR_REQUIRE(s->vertex_map != nullptr, "%s: NULL vertex_map", who);
    PR_REQUIRE(s->merged_vertices != nullptr, "%s: NULL merged_vertices", who);
    PR_REQUIRE(s->out_vertices != nullptr, "%s: NULL out_vertices (always written)", who);
    PR_REQUIRE(s->counts != nullptr, "%s: NULL counts (always written)", who);
    PR_REQUIRE((s->merged_triangles == nullptr) == (s->merged_triangle_offsets == nullptr),
               "%s: merged_triangles and merged_triangle_offsets go together (both or neither)", who);
    PR_REQUIRE((const void*)s->out_vertices != (const void*)s->vertices && (const void*)s->out_vertices != (const void*)s->merged_vertices,
               "%s: out_vertices is an input (vertices or merged_vertices)", who);
    const double G = 256.0 * (double)s->groups, limit = 2147483648.0;
    PR_REQUIRE((double)s->total_vertices + G < limit && (double)s->total_triangles + G < limit &&
                   (double)s->total_merged_vertices + G < limit && (double)s->total_merged_triangles + G < limit,
               "%s: mesh too large: every total + 256 groups must stay below 2^31 (the block counts are int32)", who);
    plan->BT = (s->total_triangles + 255) / 256 + s->groups;
    plan->BM = (s->total_merged_vertices + 255) / 256 + s->groups;
    plan->BU = (s->total_merged_triangles + 255) / 256 + s->groups;
    const size_t VO = (size_t)s->total_merged_vertices;
    const size_t table = ((size_t)s->groups + 1) * sizeof(int32_t);
    size_t at = 0;
    for (int i = 0; i < 8; ++i) plan->table[i] = workspace_region(&at, table);
    plan->sums = workspace_region(&at, 8 * (size_t)PLACE_SUMS * VO);
    plan->contributions = workspace_region(&at, 4 * VO);
    plan->bytes = at;
    PR_REQUIRE(at < ((size_t)1 << 62), "%s: the workspace sum overflows", who);       // (cannot happen below the bounds above)
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_mesh_place_workspace_size(const pr_mesh_place_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_mesh_place_workspace_size: NULL bytes");
    pr::MeshPlacePlan plan;
    PR_TRY(pr::plan_place(s, "pr_mesh_place_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_mesh_place(const pr_mesh_place_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    static_assert(sizeof(pr_mesh_place_t) == 136, "the header states this size");
    MeshPlacePlan plan;
    PR_TRY(plan_place(s, "pr_mesh_place", &plan));
    PR_TRY(check_workspace("pr_mesh_place", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    MeshPlaceParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.VO = s->total_merged_vertices;
    p.TO = s->merged_triangles ? s->total_merged_triangles : 0;
    p.h = (double)s->scale;
    p.regularisation = (double)s->regularisation;
    for (int a = 0; a < 3; ++a) p.max_move[a] = (double)s->max_move[a];
    p.vertices = s->vertices;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.vertex_map = s->vertex_map;
    p.merged_vertices = s->merged_vertices;
    p.merged_vertex_offsets = s->merged_vertex_offsets;
    p.merged_triangles = s->merged_triangles;
    p.merged_triangle_offsets = s->merged_triangle_offsets;
    p.out_vertices = s->out_vertices;
    p.counts = s->counts;
    p.vfirst = (int32_t*)(ws + plan.table[0]);
    p.tfirst = (int32_t*)(ws + plan.table[1]);
    p.mfirst = (int32_t*)(ws + plan.table[2]);
    p.ufirst = (int32_t*)(ws + plan.table[3]);
    p.vblk = (int32_t*)(ws + plan.table[4]);
    p.tblk = (int32_t*)(ws + plan.table[5]);
    p.mblk = (int32_t*)(ws + plan.table[6]);
    p.ublk = (int32_t*)(ws + plan.table[7]);
    p.sums = (unsigned long long*)(ws + plan.sums);
    p.contributions = (int32_t*)(ws + plan.contributions);
    const size_t words = (size_t)PLACE_SUMS * (size_t)s->total_merged_vertices;
    const unsigned init_grid = (unsigned)((words + 255) / 256 < 65536 ? (words + 255) / 256 + 1 : 65536);
    hipLaunchKernelGGL(k_place_init, dim3(init_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_place_accumulate, dim3((unsigned)plan.BT), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_place_solve, dim3((unsigned)plan.BM), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (s->merged_triangles) {
        hipLaunchKernelGGL(k_place_turned, dim3((unsigned)plan.BU), dim3(256), 0, st, p);
        PR_LAUNCH_CHECK();
    }
    return PR_OK;
}
