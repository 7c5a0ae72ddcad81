// Smoothing of packed, welded triangle meshes (pr_mesh_smooth, include/playrender.h states the rule): per group the vertex-to-triangle
// incidence lists of the valid triangles, `steps` Jacobi steps of the triangle umbrella with alternating factors (Taubin), area-weighted
// vertex normals of the result, the lists as a CSR, a state word per vertex and the counts.  Identity is by INDEX.
//
// Nine launches plus one per step on the caller's stream, all kernels:
//   k_smooth_init       zeroes the per-vertex counts and cursors, copies the positions into out_vertices (and into the second buffer when
//                       there are steps), fills out_normals with zeros and vertex_state with -1; one lane of block 0 clamps the offsets
//                       and builds the block tables (the rule: mesh_dev.h)
//   k_smooth_count      per triangle: valid or dropped, an atomic add on its three vertices' counts; the kept flag with the three
//                       positions the atomics returned; block sums
//   k_smooth_sums       per vertex block: the sum of its counts
//   k_smooth_scan       one workgroup: the exclusive scan of the block sums, serial over chunks of 256 with a carry - one level above
//                       the blocks, so no size changes its path
//   k_smooth_offsets    per vertex: the first entry of its list
//   k_smooth_fill       per valid triangle: its index into its three vertices' lists, at the positions the count kept (behind
//                       position 1023 of a list: at an atomic cursor per vertex)
//   k_smooth_classify   per vertex: insertion sort of its list in place when k <= max_degree, the border test, the state; block partials
//   k_smooth_step       (`steps` times) per movable vertex: the ordered umbrella mean and the step, from one buffer into the other
//   k_smooth_normals    per vertex with 1 <= k <= max_degree: the ordered sum of its triangles' cross products, normalised
//   k_smooth_finish     one grid, two block ranges: the CSR outputs (if asked for), per group the counts
// Lanes: one per element, wave64, 256-lane blocks that never span two groups (mesh_lane, mesh_dev.h; a triangle's checked corners are
// mesh_corners).  Integer atomics only, in the count and in the fill; the sort removes the order of arrival from every list that
// anything later reads in order.
#include "mesh_dev.h"

namespace pr {

constexpr int SMOOTH_COUNTS = 8;
constexpr int SMOOTH_MAX_STEPS = 4096;
constexpr int SMOOTH_MAX_DEGREE = 256;
constexpr int SMOOTH_KEPT = 1 << 30;          // the kept flag of a triangle; bits 0 .. 29: three list positions of 10 bits
constexpr int SMOOTH_SLOT_LIMIT = 1023;      // a position at or above this is not kept: the fill takes it from the vertex's cursor
constexpr int SMOOTH_SHORT = 12;             // lists up to this length are classified in registers
enum { SMOOTH_HAS_TRIANGLES = 1, SMOOTH_BORDER = 2, SMOOTH_PINNED = 4, SMOOTH_OVER_DEGREE = 8, SMOOTH_NOT_FINITE = 16, SMOOTH_MOVABLE = 32 };
enum { SMOOTH_P_MOVABLE, SMOOTH_P_LONE, SMOOTH_P_BORDER, SMOOTH_P_OVER_DEGREE, SMOOTH_P_NOT_FINITE, SMOOTH_P_LARGEST, SMOOTH_PARTIALS };

struct SmoothParams {
    int groups, V, T;
    int BV, BT;                   // launched vertex / triangle blocks
    int CB;                       // blocks of k_smooth_finish that write the CSR outputs (0 without them)
    int steps, max_degree, pin_border;
    float lambda, mu;
    const float* vertices; const int32_t* triangles; const int32_t* vertex_offsets; const int32_t* triangle_offsets; const uint8_t* pinned;
    float* out_vertices; float* out_normals; int32_t* incidence_offsets; int32_t* incidence; int32_t* vertex_state; int32_t* counts;
    // workspace
    int32_t* vfirst; int32_t* tfirst;   // (G + 1) the offsets, clamped
    int32_t* vblk; int32_t* tblk;       // (G + 1) first block of the group
    int32_t* vcount;              // (V) k: valid triangles with a corner at the vertex
    int32_t* voffset;             // (V + 1) first entry of the vertex's list, over all groups
    int32_t* vcursor;             // (V) entries filled so far behind position SMOOTH_SLOT_LIMIT
    int32_t* list;                // (3 T) the lists: triangle indices local to the group
    int32_t* tkeep;               // (T) SMOOTH_KEPT if valid, and the list positions of its three corners
    float* second;                // (V, 3) the other position buffer
    int32_t* vstate;              // (V) the state bits
    int32_t* vsum; int32_t* voff;       // (BV) list entries per vertex block, (BV + 1) their exclusive scan and the total
    int32_t* tsum;                // (BT) valid triangles per triangle block
    int32_t* vpart;               // (BV, 6) per vertex block: the SMOOTH_P_ columns
};

__global__ __launch_bounds__(256) void k_smooth_init(SmoothParams s) {
    const size_t stride = (size_t)gridDim.x * 256, at = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t V = (size_t)s.V;
    for (size_t i = at; i < V; i += stride) {
        as_global(s.vcount)[i] = 0;
        as_global(s.vcursor)[i] = 0;
        if (s.vertex_state) as_global(s.vertex_state)[i] = -1;   // (a row that no clamped group owns keeps this)
    }
    // bit for bit, every row: an immovable vertex and a row that no clamped group owns are never written again
    const PR_GLOBAL_AS uint32_t* in = (const PR_GLOBAL_AS uint32_t*)as_global(s.vertices);
    PR_GLOBAL_AS uint32_t* out = (PR_GLOBAL_AS uint32_t*)as_global(s.out_vertices);
    PR_GLOBAL_AS uint32_t* second = (PR_GLOBAL_AS uint32_t*)as_global(s.second);
    for (size_t i = at; i < 3 * V; i += stride) {
        const uint32_t word = in[i];
        out[i] = word;
        if (s.steps > 0) second[i] = word;
        if (s.out_normals) as_global(s.out_normals)[i] = 0.f;
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

__global__ __launch_bounds__(256) void k_smooth_count(SmoothParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) {                        // (the whole block: behind the last group, its sum is 0)
        if (threadIdx.x == 0) as_global(s.tsum)[blockIdx.x] = 0;
        return;
    }
    bool valid = false;
    if (l.live) {
        const int vfirst = as_global(s.vfirst)[l.group];
        const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
        const MeshCorners c = mesh_corners(s.triangles, l.first, l.local, vsize);
        valid = c.in_range && c.i[0] != c.i[1] && c.i[0] != c.i[2] && c.i[1] != c.i[2];
        if (valid) {
            const PR_GLOBAL_AS float* v = as_global(s.vertices) + (size_t)vfirst * 3;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const PR_GLOBAL_AS float* p = v + (size_t)c.i[e] * 3;
                valid = valid && mesh_finite(p[0]) && mesh_finite(p[1]) && mesh_finite(p[2]);
            }
        }
        // the value an atomic returns is a position in the vertex's list that nobody else gets: kept, 10 bits per corner, beside the
        // flag, so that the fill needs no second atomic (positions from SMOOTH_SLOT_LIMIT on are handed out by a cursor there)
        int packed = 0;
        if (valid) {
            packed = SMOOTH_KEPT;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int at = __hip_atomic_fetch_add(as_global(s.vcount) + (size_t)vfirst + c.i[e], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                packed |= (at < 0 || at > SMOOTH_SLOT_LIMIT ? SMOOTH_SLOT_LIMIT : at) << (10 * e);
            }
        }
        as_global(s.tkeep)[(size_t)l.first + l.local] = packed;
    }
    int total;
    block_exclusive_scan_256(valid ? 1 : 0, lds, &total);
    if (threadIdx.x == 0) as_global(s.tsum)[blockIdx.x] = total;
}

// k of the lane's vertex as the count kernel left it, kept inside [0, 3 T_g] (a triangle adds at most three)
__device__ __forceinline__ int smooth_degree(const SmoothParams& s, const MeshLane& l) {
    const int tsize = as_global(s.tfirst)[l.group + 1] - as_global(s.tfirst)[l.group];
    const int k = as_global(s.vcount)[(size_t)l.first + l.local];
    return k < 0 ? 0 : (k > tsize ? tsize : k);
}

__global__ __launch_bounds__(256) void k_smooth_sums(SmoothParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (l.group < 0) {                        // (the whole block: behind the last group, its sum is 0)
        if (threadIdx.x == 0) as_global(s.vsum)[blockIdx.x] = 0;
        return;
    }
    int total;
    block_exclusive_scan_256(l.live ? smooth_degree(s, l) : 0, lds, &total);
    if (threadIdx.x == 0) as_global(s.vsum)[blockIdx.x] = total;
}

// One workgroup scans the BV block sums: chunks of 256 in order with a carry, so the scan has ONE path for every size; voff[BV] is
// the total (at most 3 T: every valid triangle adds three entries).
__global__ __launch_bounds__(256) void k_smooth_scan(SmoothParams s) {
    __shared__ int lds[4];
    const PR_GLOBAL_AS int32_t* sums = as_global(s.vsum);
    PR_GLOBAL_AS int32_t* offsets = as_global(s.voff);
    const int n = s.BV;
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

__global__ __launch_bounds__(256) void k_smooth_offsets(SmoothParams s) {
    __shared__ int lds[4];
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    int total;
    const int ex = block_exclusive_scan_256(l.live ? smooth_degree(s, l) : 0, lds, &total);
    if (l.live) as_global(s.voffset)[(size_t)l.first + l.local] = as_global(s.voff)[blockIdx.x] + ex;
}

// the list of vertex `row` with k entries: its first entry, or -1 if the list would leave the 3 T entries (never, unless the workspace
// was damaged: checked where it is read)
__device__ __forceinline__ long long smooth_list_begin(const SmoothParams& s, size_t row, int k) {
    const int begin = as_global(s.voffset)[row];
    if (begin < 0 || (long long)begin + k > 3ll * s.T) return -1;
    return begin;
}

__global__ __launch_bounds__(256) void k_smooth_fill(SmoothParams s) {
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (!l.live) return;
    const int packed = as_global(s.tkeep)[(size_t)l.first + l.local];
    if (!(packed & SMOOTH_KEPT)) return;
    const int vfirst = as_global(s.vfirst)[l.group];
    const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
    const MeshCorners c = mesh_corners(s.triangles, l.first, l.local, vsize);      // (read again: checked again)
    if (!c.in_range) return;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const size_t row = (size_t)vfirst + c.i[e];
        const int k = as_global(s.vcount)[row];
        int at = (packed >> (10 * e)) & SMOOTH_SLOT_LIMIT;
        if (at == SMOOTH_SLOT_LIMIT)          // (a list of more than SMOOTH_SLOT_LIMIT triangles: the positions behind come from the cursor)
            at += __hip_atomic_fetch_add(as_global(s.vcursor) + row, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (at < 0 || at >= k) continue;      // (never for a valid triangle: the count kernel counted it)
        const long long begin = smooth_list_begin(s, row, k);
        if (begin >= 0) as_global(s.list)[begin + at] = l.local;
    }
}

struct SmoothOthers {
    int x, y;                     // the others of the vertex in the triangle, local to the group; -1: the triangle cannot be read
};

// the others of vertex `v` (local) in triangle `t` (local, read from a list: checked here) of group `g`
__device__ __forceinline__ SmoothOthers smooth_others(const SmoothParams& s, int tfirst, int tsize, int vsize, int t, int v) {
    SmoothOthers o;
    o.x = o.y = -1;
    if ((unsigned)t >= (unsigned)tsize) return o;
    const MeshCorners c = mesh_corners(s.triangles, tfirst, t, vsize);
    if (!c.in_range) return o;
    if (v == c.i[0]) { o.x = c.i[1]; o.y = c.i[2]; }
    else if (v == c.i[1]) { o.x = c.i[2]; o.y = c.i[0]; }
    else { o.x = c.i[0]; o.y = c.i[1]; }
    return o;
}

__global__ __launch_bounds__(256) void k_smooth_classify(SmoothParams s) {
    __shared__ int lds[4];
    __shared__ int largest[256];
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block: k_smooth_finish reads the partials of the groups' blocks only)
    int state = 0, k = 0;
    if (l.live) {
        const size_t row = (size_t)l.first + l.local;
        const int tfirst = as_global(s.tfirst)[l.group];
        const int tsize = as_global(s.tfirst)[l.group + 1] - tfirst;
        k = smooth_degree(s, l);
        const PR_GLOBAL_AS float* p = as_global(s.vertices) + row * 3;
        const bool finite = mesh_finite(p[0]) && mesh_finite(p[1]) && mesh_finite(p[2]);
        const bool pinned = s.pinned && as_global(s.pinned)[row] != 0;
        const long long begin = smooth_list_begin(s, row, k);
        const bool listed = k >= 1 && k <= s.max_degree && begin >= 0;
        bool border = false;
        if (listed) {
            PR_GLOBAL_AS int32_t* list = as_global(s.list) + begin;
            for (int i = 1; i < k; ++i) {     // insertion sort, ascending: at most k (k - 1) / 2 <= k max_degree comparisons
                const int t = list[i];
                int j = i;
                while (j > 0 && list[j - 1] > t) {
                    list[j] = list[j - 1];
                    --j;
                }
                list[j] = t;
            }
            // border: some vertex occurs exactly once among the 2 k others.  Up to SMOOTH_SHORT triangles (nearly every list of an
            // extracted mesh) the others are read once into registers and compared there; a longer list reads them k times.
            if (k <= SMOOTH_SHORT) {
                int x[SMOOTH_SHORT], y[SMOOTH_SHORT];
#pragma unroll
                for (int i = 0; i < SMOOTH_SHORT; ++i) {
                    x[i] = y[i] = -1;
                    if (i < k) {
                        const SmoothOthers o = smooth_others(s, tfirst, tsize, l.size, list[i], l.local);
                        x[i] = o.x;
                        y[i] = o.y;
                    }
                }
#pragma unroll
                for (int i = 0; i < SMOOTH_SHORT; ++i) {
                    int nx = 0, ny = 0;
#pragma unroll
                    for (int j = 0; j < SMOOTH_SHORT; ++j) {
                        const bool in = j < k;
                        nx += (in && x[j] == x[i] ? 1 : 0) + (in && y[j] == x[i] ? 1 : 0);
                        ny += (in && x[j] == y[i] ? 1 : 0) + (in && y[j] == y[i] ? 1 : 0);
                    }
                    border = border || (i < k && (nx == 1 || ny == 1));
                }
            }
            for (int i = 0; k > SMOOTH_SHORT && i < k && !border; ++i) {
                const SmoothOthers mine = smooth_others(s, tfirst, tsize, l.size, list[i], l.local);
                int nx = 0, ny = 0;
                for (int j = 0; j < k; ++j) {
                    const SmoothOthers o = smooth_others(s, tfirst, tsize, l.size, list[j], l.local);
                    nx += (o.x == mine.x ? 1 : 0) + (o.y == mine.x ? 1 : 0);
                    ny += (o.x == mine.y ? 1 : 0) + (o.y == mine.y ? 1 : 0);
                    if (nx > 1 && ny > 1) break;                 // (the counts only grow: neither can end at 1)
                }
                border = nx == 1 || ny == 1;
            }
        }
        state = (k >= 1 ? SMOOTH_HAS_TRIANGLES : 0) | (border ? SMOOTH_BORDER : 0) | (pinned ? SMOOTH_PINNED : 0) |
                (k > s.max_degree ? SMOOTH_OVER_DEGREE : 0) | (finite ? 0 : SMOOTH_NOT_FINITE);
        if (finite && listed && !pinned && !(border && s.pin_border)) state |= SMOOTH_MOVABLE;
        as_global(s.vstate)[row] = state;
        if (s.vertex_state) as_global(s.vertex_state)[row] = state;
    }
    const int flags[5] = {state & SMOOTH_MOVABLE, l.live && k == 0 && !(state & SMOOTH_NOT_FINITE) ? 1 : 0, state & SMOOTH_BORDER,
                          state & SMOOTH_OVER_DEGREE, state & SMOOTH_NOT_FINITE};
    int total[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) block_exclusive_scan_256(flags[i] ? 1 : 0, lds, &total[i]);
    largest[threadIdx.x] = k;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) largest[threadIdx.x] = max(largest[threadIdx.x], largest[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        PR_GLOBAL_AS int32_t* part = as_global(s.vpart) + (size_t)blockIdx.x * SMOOTH_PARTIALS;
        part[SMOOTH_P_MOVABLE] = total[0];
        part[SMOOTH_P_LONE] = total[1];
        part[SMOOTH_P_BORDER] = total[2];
        part[SMOOTH_P_OVER_DEGREE] = total[3];
        part[SMOOTH_P_NOT_FINITE] = total[4];
        part[SMOOTH_P_LARGEST] = largest[0];
    }
}

// One step: p' = p + f (mean - p) with the ordered umbrella mean, from `src` into `dst`.  A vertex that is not movable is not written:
// both buffers hold its input words since k_smooth_init.
__global__ __launch_bounds__(256) void k_smooth_step(SmoothParams s, const float* src, float* dst, float f) {
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (!l.live) return;
    const size_t row = (size_t)l.first + l.local;
    if (!(as_global(s.vstate)[row] & SMOOTH_MOVABLE)) return;
    const int tfirst = as_global(s.tfirst)[l.group];
    const int tsize = as_global(s.tfirst)[l.group + 1] - tfirst;
    const int k = smooth_degree(s, l);
    const long long begin = smooth_list_begin(s, row, k);
    if (k < 1 || k > s.max_degree || begin < 0) return;          // (never for a movable vertex)
    const PR_GLOBAL_AS int32_t* list = as_global(s.list) + begin;
    const PR_GLOBAL_AS float* from = as_global(src) + (size_t)l.first * 3;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < k; ++i) {
        const SmoothOthers o = smooth_others(s, tfirst, tsize, l.size, list[i], l.local);
        if (o.x < 0) return;                  // (never: the list holds valid triangles)
        const PR_GLOBAL_AS float* x = from + (size_t)o.x * 3;
        const PR_GLOBAL_AS float* y = from + (size_t)o.y * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[a] = i == 0 ? x[a] : __fadd_rn(acc[a], x[a]);
            acc[a] = __fadd_rn(acc[a], y[a]);
        }
    }
    const float n = (float)(2 * k);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = from[(size_t)l.local * 3 + a];
        const float mean = __fdiv_rn(acc[a], n);
        as_global(dst)[row * 3 + a] = __fadd_rn(p, __fmul_rn(f, __fsub_rn(mean, p)));
    }
}

__global__ __launch_bounds__(256) void k_smooth_normals(SmoothParams s) {
    if (!s.out_normals) return;
    const MeshLane l = mesh_lane(s.groups, s.vblk, s.vfirst, (int)blockIdx.x);
    if (!l.live) return;
    const size_t row = (size_t)l.first + l.local;
    const int state = as_global(s.vstate)[row];
    const int tfirst = as_global(s.tfirst)[l.group];
    const int tsize = as_global(s.tfirst)[l.group + 1] - tfirst;
    const int k = smooth_degree(s, l);
    const long long begin = smooth_list_begin(s, row, k);
    float N[3] = {0.f, 0.f, 0.f};
    bool covered = (state & SMOOTH_HAS_TRIANGLES) && !(state & SMOOTH_OVER_DEGREE) && k >= 1 && k <= s.max_degree && begin >= 0;
    if (covered) {
        const PR_GLOBAL_AS int32_t* list = as_global(s.list) + begin;
        const PR_GLOBAL_AS float* v = as_global(s.out_vertices) + (size_t)l.first * 3;
        for (int i = 0; i < k; ++i) {
            const int t = list[i];
            if ((unsigned)t >= (unsigned)tsize) { covered = false; break; }      // (never)
            const MeshCorners c = mesh_corners(s.triangles, tfirst, t, l.size);
            if (!c.in_range) { covered = false; break; }
            const PR_GLOBAL_AS float* a = v + (size_t)c.i[0] * 3;
            const PR_GLOBAL_AS float* b = v + (size_t)c.i[1] * 3;
            const PR_GLOBAL_AS float* cc = v + (size_t)c.i[2] * 3;
            float e1[3], e2[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                e1[d] = __fsub_rn(b[d], a[d]);
                e2[d] = __fsub_rn(cc[d], a[d]);
            }
            const float n0 = __fsub_rn(__fmul_rn(e1[1], e2[2]), __fmul_rn(e1[2], e2[1]));
            const float n1 = __fsub_rn(__fmul_rn(e1[2], e2[0]), __fmul_rn(e1[0], e2[2]));
            const float n2 = __fsub_rn(__fmul_rn(e1[0], e2[1]), __fmul_rn(e1[1], e2[0]));
            N[0] = i == 0 ? n0 : __fadd_rn(N[0], n0);
            N[1] = i == 0 ? n1 : __fadd_rn(N[1], n1);
            N[2] = i == 0 ? n2 : __fadd_rn(N[2], n2);
        }
    }
    float out[3] = {0.f, 0.f, 0.f};
    if (covered) {
        // sqrtf, not __fsqrt_rn: the latter compiles to the bare v_sqrt_f32 (1 ulp), sqrtf to its correctly rounded refinement
        const float length = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(N[0], N[0]), __fmul_rn(N[1], N[1])), __fmul_rn(N[2], N[2])));
        if (mesh_finite(length) && length > 0.f) {
#pragma unroll
            for (int d = 0; d < 3; ++d) out[d] = __fdiv_rn(N[d], length);
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) as_global(s.out_normals)[row * 3 + d] = out[d];
}

// One grid, two block ranges.  [0, CB): the CSR outputs, each block striding over the V + 1 offsets and then over the entries.
// [CB, CB + G): a block per group.
__global__ __launch_bounds__(256) void k_smooth_finish(SmoothParams s) {
    __shared__ int lds[4];
    __shared__ int largest[256];
    const int b = (int)blockIdx.x;
    if (b < s.CB) {
        const size_t stride = (size_t)s.CB * 256, at = (size_t)b * 256 + threadIdx.x;
        const int total = min(max(as_global(s.voff)[s.BV], 0), 3 * s.T);     // (3 T < 2^31)
        const int owned_from = as_global(s.vfirst)[0], owned_to = as_global(s.vfirst)[s.groups];
        // the clamped offsets do not decrease: the rows that no group owns lie in front of the first group and behind the last one
        for (size_t i = at; i <= (size_t)s.V; i += stride)
            as_global(s.incidence_offsets)[i] = (int)i < owned_from ? 0 : ((int)i >= owned_to ? total : as_global(s.voffset)[i]);
        for (size_t i = at; i < (size_t)total; i += stride) as_global(s.incidence)[i] = as_global(s.list)[i];
        return;
    }
    // integers: lane t sums the rows of the group's blocks t, t + 256, ..., the block adds the lanes up
    const int g = b - s.CB;
    const int vbegin = as_global(s.vblk)[g], vend = as_global(s.vblk)[g + 1];
    const int tbegin = as_global(s.tblk)[g], tend = as_global(s.tblk)[g + 1];
    int sum[SMOOTH_PARTIALS] = {0, 0, 0, 0, 0, 0}, total[SMOOTH_PARTIALS];
    for (int k = vbegin + (int)threadIdx.x; k < vend; k += 256) {
        const PR_GLOBAL_AS int32_t* part = as_global(s.vpart) + (size_t)k * SMOOTH_PARTIALS;
#pragma unroll
        for (int i = 0; i < SMOOTH_P_LARGEST; ++i) sum[i] += part[i];
        sum[SMOOTH_P_LARGEST] = max(sum[SMOOTH_P_LARGEST], part[SMOOTH_P_LARGEST]);
    }
    int valid = 0, valid_total;
    for (int k = tbegin + (int)threadIdx.x; k < tend; k += 256) valid += as_global(s.tsum)[k];
#pragma unroll
    for (int i = 0; i < SMOOTH_P_LARGEST; ++i) block_exclusive_scan_256(sum[i], lds, &total[i]);
    block_exclusive_scan_256(valid, lds, &valid_total);
    largest[threadIdx.x] = sum[SMOOTH_P_LARGEST];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) largest[threadIdx.x] = max(largest[threadIdx.x], largest[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    PR_GLOBAL_AS int32_t* counts = as_global(s.counts) + (size_t)g * SMOOTH_COUNTS;
    counts[0] = valid_total;
    counts[1] = as_global(s.tfirst)[g + 1] - as_global(s.tfirst)[g] - valid_total;
    counts[2] = total[SMOOTH_P_MOVABLE];
    counts[3] = total[SMOOTH_P_LONE];
    counts[4] = total[SMOOTH_P_BORDER];
    counts[5] = total[SMOOTH_P_OVER_DEGREE];
    counts[6] = total[SMOOTH_P_NOT_FINITE];
    counts[7] = largest[0];
}

struct SmoothPlan {
    size_t vfirst, tfirst, vblk, tblk, vcount, voffset, vcursor, list, tkeep, second, vstate, vsum, voff, tsum, vpart, bytes;
    int BV, BT;
};

// Host checks of both entry points: no device work.
static int plan_smooth(const pr_mesh_smooth_t* s, const char* who, SmoothPlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    PR_REQUIRE((s->flags & ~PR_SMOOTH_PIN_BORDER) == 0, "%s: unknown flag bits 0x%x (PR_SMOOTH_PIN_BORDER or 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->steps >= 0 && s->steps <= SMOOTH_MAX_STEPS, "%s: steps %d (0 .. %d)", who, s->steps, SMOOTH_MAX_STEPS);
    PR_REQUIRE(s->max_degree >= 1 && s->max_degree <= SMOOTH_MAX_DEGREE, "%s: max_degree %d (1 .. %d)", who, s->max_degree,
               SMOOTH_MAX_DEGREE);
    PR_REQUIRE(s->lambda - s->lambda == 0.f && s->mu - s->mu == 0.f, "%s: lambda / mu not finite (%g, %g)", who, (double)s->lambda,
               (double)s->mu);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->out_vertices != nullptr, "%s: NULL out_vertices (always written)", who);
    PR_REQUIRE(s->counts != nullptr, "%s: NULL counts (always written)", who);
    PR_REQUIRE((s->incidence_offsets == nullptr) == (s->incidence == nullptr),
               "%s: incidence_offsets and incidence go together (both or neither)", who);
    PR_REQUIRE((const void*)s->out_vertices != (const void*)s->vertices, "%s: out_vertices == vertices (the steps read the input)", who);
    const double G = (double)s->groups;
    PR_REQUIRE(3.0 * (double)s->total_triangles + 256.0 * G < 2147483648.0 && (double)s->total_vertices + 256.0 * G < 2147483648.0,
               "%s: mesh too large: 3 total_triangles + 256 groups and total_vertices + 256 groups must stay below 2^31 "
               "(the list entries and the block counts are int32)", who);
    plan->BV = (s->total_vertices + 255) / 256 + s->groups;
    plan->BT = (s->total_triangles + 255) / 256 + s->groups;
    const size_t V = (size_t)s->total_vertices, T = (size_t)s->total_triangles;
    const size_t table = ((size_t)s->groups + 1) * sizeof(int32_t);
    size_t at = 0;
    plan->vfirst = workspace_region(&at, table);
    plan->tfirst = workspace_region(&at, table);
    plan->vblk = workspace_region(&at, table);
    plan->tblk = workspace_region(&at, table);
    plan->vcount = workspace_region(&at, 4 * V);
    plan->voffset = workspace_region(&at, 4 * (V + 1));
    plan->vcursor = workspace_region(&at, 4 * V);
    plan->list = workspace_region(&at, 12 * T);
    plan->tkeep = workspace_region(&at, 4 * T);
    plan->second = workspace_region(&at, 12 * V);
    plan->vstate = workspace_region(&at, 4 * V);
    plan->vsum = workspace_region(&at, 4 * (size_t)plan->BV);
    plan->voff = workspace_region(&at, 4 * ((size_t)plan->BV + 1));
    plan->tsum = workspace_region(&at, 4 * (size_t)plan->BT);
    plan->vpart = workspace_region(&at, (size_t)SMOOTH_PARTIALS * sizeof(int32_t) * (size_t)plan->BV);
    plan->bytes = at;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_mesh_smooth_workspace_size(const pr_mesh_smooth_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_mesh_smooth_workspace_size: NULL bytes");
    pr::SmoothPlan plan;
    PR_TRY(pr::plan_smooth(s, "pr_mesh_smooth_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_mesh_smooth(const pr_mesh_smooth_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    static_assert(sizeof(pr_mesh_smooth_t) == 120, "the header states this size");
    SmoothPlan plan;
    PR_TRY(plan_smooth(s, "pr_mesh_smooth", &plan));
    PR_TRY(check_workspace("pr_mesh_smooth", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    SmoothParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.BV = plan.BV;
    p.BT = plan.BT;
    p.steps = s->steps;
    p.max_degree = s->max_degree;
    p.pin_border = (s->flags & PR_SMOOTH_PIN_BORDER) ? 1 : 0;
    p.lambda = s->lambda;
    p.mu = s->mu;
    p.vertices = s->vertices;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.pinned = s->pinned;
    p.out_vertices = s->out_vertices;
    p.out_normals = s->out_normals;
    p.incidence_offsets = s->incidence_offsets;
    p.incidence = s->incidence;
    p.vertex_state = s->vertex_state;
    p.counts = s->counts;
    p.vfirst = (int32_t*)(ws + plan.vfirst);
    p.tfirst = (int32_t*)(ws + plan.tfirst);
    p.vblk = (int32_t*)(ws + plan.vblk);
    p.tblk = (int32_t*)(ws + plan.tblk);
    p.vcount = (int32_t*)(ws + plan.vcount);
    p.voffset = (int32_t*)(ws + plan.voffset);
    p.vcursor = (int32_t*)(ws + plan.vcursor);
    p.list = (int32_t*)(ws + plan.list);
    p.tkeep = (int32_t*)(ws + plan.tkeep);
    p.second = (float*)(ws + plan.second);
    p.vstate = (int32_t*)(ws + plan.vstate);
    p.vsum = (int32_t*)(ws + plan.vsum);
    p.voff = (int32_t*)(ws + plan.voff);
    p.tsum = (int32_t*)(ws + plan.tsum);
    p.vpart = (int32_t*)(ws + plan.vpart);
    const size_t words = 3 * (size_t)s->total_vertices;
    const unsigned init_grid = (unsigned)((words + 255) / 256 < 65536 ? (words + 255) / 256 + 1 : 65536);
    const size_t csr = 3 * (size_t)s->total_triangles > (size_t)s->total_vertices + 1 ? 3 * (size_t)s->total_triangles
                                                                                    : (size_t)s->total_vertices + 1;
    p.CB = s->incidence ? (int)((csr + 255) / 256 < 65536 ? (csr + 255) / 256 : 65536) : 0;
    const dim3 vertex_grid((unsigned)plan.BV), triangle_grid((unsigned)plan.BT);
    hipLaunchKernelGGL(k_smooth_init, dim3(init_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_smooth_count, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_smooth_sums, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_smooth_scan, dim3(1), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_smooth_offsets, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_smooth_fill, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_smooth_classify, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    // Jacobi on two buffers: step 0 reads the input, every later step the buffer that the step before wrote; the last step writes
    // out_vertices (k_smooth_init has written the input's words to both, so a vertex that does not move is right in either)
    for (int step = 0; step < s->steps; ++step) {
        const bool to_out = (s->steps - 1 - step) % 2 == 0;
        const float* src = step == 0 ? s->vertices : (to_out ? p.second : s->out_vertices);
        float* dst = to_out ? s->out_vertices : p.second;
        hipLaunchKernelGGL(k_smooth_step, vertex_grid, dim3(256), 0, st, p, src, dst, step % 2 == 0 ? s->lambda : s->mu);
        PR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_smooth_normals, vertex_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_smooth_finish, dim3((unsigned)(p.CB + s->groups)), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
