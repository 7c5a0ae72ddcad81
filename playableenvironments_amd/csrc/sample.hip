// Area-weighted point samples of packed triangle meshes (pr_mesh_sample, include/playrender.h states the rule): per group the fp64
// areas of the valid triangles, their largest, integer weights floor(area / A_max * 2^32), the inclusive uint64 prefix sums of the
// weights, and per sample a Philox draw, a bisection over the prefix sums, integer-folded barycentrics and the interpolated rows.
// No output depends on the execution order: the only floating-point reduction is a maximum, every sum is an integer sum.
//
// Seven launches on the caller's stream, eight with out_attributes, all kernels:
//   k_sample_init       one lane clamps the offsets and builds the triangle block table (the rule: mesh_dev.h)
//   k_sample_area       per triangle: valid or dropped, the fp64 area (-1 for a dropped one) into the 8-byte slot of the triangle;
//                       per block the largest area and the number of valid triangles
//   k_sample_max        a block per group: A_max and the counts of valid and dropped triangles
//   k_sample_weight     per triangle: the weight; per block the uint64 sum of the weights and the number of valid triangles of weight 0
//   k_sample_scan       a block per group: the exclusive scan of the group's block sums, serial over chunks of 256 with a carry - one
//                       level above the blocks, so no size changes its path; W(g), counts [2] and [3], the measures
//   k_sample_prefix     per triangle: the weight again, the block's inclusive scan plus the block's offset: W_t over the area
//   k_sample_draw       a lane per sample: Philox, the pick, the bisection (at most 31 steps; its first levels are shared by every
//                       lane of the group), the point, the triangle, the barycentrics and the normal (three columns: the lane's own
//                       gather, as for the position); the record (triangle, U, V) of the sample for the row pass
//   k_sample_rows       (with out_attributes) lanes run across the columns: a flat index over (sample, column unit), a unit being four
//                       columns where C and the two addresses allow 16-byte accesses, else one; the three corner rows are read as
//                       whole coalesced rows and the output is written as one contiguous stream
// Blocks of 256 triangles never span two groups (mesh_lane, mesh_dev.h).  No atomics.
#include "mesh_dev.h"

namespace pr {

constexpr int SAMPLE_COUNTS = 4;
constexpr int SAMPLE_MEASURES = 2;
constexpr int SAMPLE_MAX_WIDTH = 4096;
constexpr unsigned SAMPLE_ONE = 1u << 24;     // the barycentric unit
typedef int sample_int4 __attribute__((ext_vector_type(4)));    // (a native vector, as f32x4_t: storable through an address-space pointer)

struct SampleParams {
    int groups, V, T;
    int BT;                       // launched triangle blocks
    int samples, width, face, vec;    // n per group, C, face normals, 16-byte row accesses
    unsigned int k0, k1;          // the Philox key: noise_mix(seed)
    unsigned long long first;
    const float* vertices; const int32_t* triangles; const int32_t* vertex_offsets; const int32_t* triangle_offsets;
    const float* normals; const float* attributes;
    float* points; int32_t* triangle; float* barycentric; float* out_normals; float* out_attributes; int32_t* counts; double* measures;
    // workspace
    int32_t* vfirst; int32_t* tfirst;   // (G + 1) the offsets, clamped
    int32_t* tblk;                // (G + 1) first block of the group
    double* area;                 // (T) the area, -1 for a dropped triangle; then, as uint64, W_t
    double* bmax;                 // (BT) largest area of the block
    int32_t* bvalid; int32_t* bzero;    // (BT) valid triangles / valid triangles of weight 0 of the block
    unsigned long long* bsum;     // (BT) sum of the block's weights
    unsigned long long* boff;     // (BT) sum of the weights of the group's blocks in front of the block
    double* gmax;                 // (G) A_max
    unsigned long long* gtotal;   // (G) W(g)
    int32_t* record;              // (G n, 4) per sample: triangle (local, -1: none), U, V, 0
};

// One lane, serial over the groups (a handful): offsets that leave [0, total] or decrease are clamped, so that no later kernel follows
// a bad offset out of an array; the block table is the running sum of ceil(size / 256).
__global__ __launch_bounds__(64) void k_sample_init(SampleParams s) {
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

// mesh_corners of the call's triangles.  It takes the parameter block and reads the pointer itself: handed the pointer, k_sample_rows
// loads its kernel arguments in another order.
__device__ __forceinline__ MeshCorners sample_corners(const SampleParams& s, int tfirst, int local, int vsize) {
    return mesh_corners(s.triangles, tfirst, local, vsize);
}

// the largest of the block's 256 values (none is NaN), valid in every thread.  lds: >= 4 doubles.
__device__ __forceinline__ double sample_block_max(double x, double* lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(x, d, 64);
        x = o > x ? o : x;
    }
    __syncthreads();                          // (the previous use of lds has been read)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    const double a = lds[0] > lds[1] ? lds[0] : lds[1], b = lds[2] > lds[3] ? lds[2] : lds[3];
    return a > b ? a : b;
}

// exclusive scan of uint64 over the 256 threads of a block; `total` = block sum.  lds: >= 4 words.
__device__ __forceinline__ unsigned long long sample_block_scan(unsigned long long v, unsigned long long* lds, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                          // (the previous use of lds has been read)
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned long long base = 0;
    for (int w = 0; w < wave; ++w) base += lds[w];
    *total = lds[0] + lds[1] + lds[2] + lds[3];
    return base + inc - v;
}

__global__ __launch_bounds__(256) void k_sample_area(SampleParams s) {
    __shared__ double lds[4];
    __shared__ int ilds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block: nothing reads the rows of a block behind the last group)
    double area = -1.0;
    if (l.live) {
        const int vfirst = as_global(s.vfirst)[l.group];
        const int vsize = as_global(s.vfirst)[l.group + 1] - vfirst;
        const MeshCorners c = sample_corners(s, l.first, l.local, vsize);
        bool valid = c.in_range && c.i[0] != c.i[1] && c.i[0] != c.i[2] && c.i[1] != c.i[2];
        if (valid) {
            const PR_GLOBAL_AS float* v = as_global(s.vertices) + (size_t)vfirst * 3;
            float p[3][3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    p[e][x] = v[(size_t)c.i[e] * 3 + x];
                    valid = valid && mesh_finite(p[e][x]);
                }
            }
            if (valid) {                      // k_audit_measure's area: every product and difference rounded on its own
                double e1[3], e2[3];
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    e1[x] = __dsub_rn((double)p[1][x], (double)p[0][x]);
                    e2[x] = __dsub_rn((double)p[2][x], (double)p[0][x]);
                }
                const double n0 = __dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1]));
                const double n1 = __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2]));
                const double n2 = __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]));
                area = __dmul_rn(0.5, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(n0, n0), __dmul_rn(n1, n1)), __dmul_rn(n2, n2))));
            }
        }
        as_global(s.area)[(size_t)l.first + l.local] = area;
    }
    const double largest = sample_block_max(area < 0.0 ? 0.0 : area, lds);
    int valid_total;
    block_exclusive_scan_256(area >= 0.0 ? 1 : 0, ilds, &valid_total);
    if (threadIdx.x == 0) {
        as_global(s.bmax)[blockIdx.x] = largest;
        as_global(s.bvalid)[blockIdx.x] = valid_total;
    }
}

__global__ __launch_bounds__(256) void k_sample_max(SampleParams s) {
    __shared__ double lds[4];
    __shared__ int ilds[4];
    const int g = (int)blockIdx.x;
    const int begin = as_global(s.tblk)[g], end = as_global(s.tblk)[g + 1];
    double largest = 0.0;
    int valid = 0, valid_total;
    for (int b = begin + (int)threadIdx.x; b < end; b += 256) {
        const double x = as_global(s.bmax)[b];
        largest = x > largest ? x : largest;
        valid += as_global(s.bvalid)[b];
    }
    largest = sample_block_max(largest, lds);
    block_exclusive_scan_256(valid, ilds, &valid_total);
    if (threadIdx.x != 0) return;
    as_global(s.gmax)[g] = largest;
    as_global(s.counts)[(size_t)g * SAMPLE_COUNTS + 0] = valid_total;
    as_global(s.counts)[(size_t)g * SAMPLE_COUNTS + 1] = as_global(s.tfirst)[g + 1] - as_global(s.tfirst)[g] - valid_total;
}

// the weight of a triangle of area `area` (-1: dropped) in a group whose largest area is `largest`; *valid: it is a valid triangle
__device__ __forceinline__ unsigned long long sample_weight(double area, double largest, bool* valid) {
    *valid = area >= 0.0;
    if (!(area >= 0.0) || !(largest > 0.0) || area > largest) return 0;       // (area > largest: never, unless the workspace was damaged)
    return (unsigned long long)__dmul_rn(__ddiv_rn(area, largest), 4294967296.0);     // (the quotient is in [0, 1]: at most 2^32)
}

__global__ __launch_bounds__(256) void k_sample_weight(SampleParams s) {
    __shared__ unsigned long long lds[4];
    __shared__ int ilds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    unsigned long long w = 0, total;
    bool valid = false;
    if (l.live) w = sample_weight(as_global(s.area)[(size_t)l.first + l.local], as_global(s.gmax)[l.group], &valid);
    sample_block_scan(w, lds, &total);
    int zero_total;
    block_exclusive_scan_256(valid && w == 0 ? 1 : 0, ilds, &zero_total);
    if (threadIdx.x == 0) {
        as_global(s.bsum)[blockIdx.x] = total;
        as_global(s.bzero)[blockIdx.x] = zero_total;
    }
}

// A block per group scans the group's block sums: chunks of 256 in order with a carry, so the scan has ONE path for every size.
__global__ __launch_bounds__(256) void k_sample_scan(SampleParams s) {
    __shared__ unsigned long long lds[4];
    __shared__ int ilds[4];
    const int g = (int)blockIdx.x;
    const int begin = as_global(s.tblk)[g], end = as_global(s.tblk)[g + 1];
    unsigned long long carry = 0;
    int zero = 0, zero_total;
    for (int start = begin; start < end; start += 256) {
        const int b = start + (int)threadIdx.x;
        unsigned long long chunk;
        const unsigned long long ex = sample_block_scan(b < end ? as_global(s.bsum)[b] : 0ull, lds, &chunk);
        if (b < end) {
            as_global(s.boff)[b] = carry + ex;
            zero += as_global(s.bzero)[b];
        }
        carry += chunk;
    }
    block_exclusive_scan_256(zero, ilds, &zero_total);
    if (threadIdx.x != 0) return;
    const double largest = as_global(s.gmax)[g];
    const bool empty = carry == 0;
    as_global(s.gtotal)[g] = carry;
    as_global(s.counts)[(size_t)g * SAMPLE_COUNTS + 2] = zero_total;
    as_global(s.counts)[(size_t)g * SAMPLE_COUNTS + 3] = empty ? 0 : s.samples;
    as_global(s.measures)[(size_t)g * SAMPLE_MEASURES + 0] = empty ? 0.0 : largest;
    as_global(s.measures)[(size_t)g * SAMPLE_MEASURES + 1] =
        empty ? 0.0 : __dmul_rn(__dmul_rn((double)carry, largest), 2.3283064365386962890625e-10);      // 2^-32
}

__global__ __launch_bounds__(256) void k_sample_prefix(SampleParams s) {
    __shared__ unsigned long long lds[4];
    const MeshLane l = mesh_lane(s.groups, s.tblk, s.tfirst, (int)blockIdx.x);
    if (l.group < 0) return;                  // (the whole block)
    unsigned long long w = 0, total;
    bool valid;
    if (l.live) w = sample_weight(as_global(s.area)[(size_t)l.first + l.local], as_global(s.gmax)[l.group], &valid);
    const unsigned long long ex = sample_block_scan(w, lds, &total);
    if (l.live) ((PR_GLOBAL_AS unsigned long long*)as_global(s.area))[(size_t)l.first + l.local] = as_global(s.boff)[blockIdx.x] + ex + w;
}

struct SampleDraw {
    unsigned int U, V;            // the folded barycentric integers: b1 = U 2^-24, b2 = V 2^-24, b0 = (2^24 - U - V) 2^-24
    unsigned long long r;
};

__device__ __forceinline__ SampleDraw sample_draw(const SampleParams& s, int g, int i) {
    const unsigned long long j = s.first + (unsigned long long)i;
    unsigned int x[4];
    philox4x32_10((unsigned int)j, (unsigned int)(j >> 32), (unsigned int)g, 0u, s.k0, s.k1, x);
    SampleDraw d;
    d.r = (unsigned long long)x[0] | ((unsigned long long)x[1] << 32);
    d.U = x[2] >> 8;
    d.V = x[3] >> 8;
    if (d.U + d.V > SAMPLE_ONE) {             // the fold, in integers
        d.U = SAMPLE_ONE - d.U;
        d.V = SAMPLE_ONE - d.V;
    }
    return d;
}

// ((b0 a) + (b1 b)) + (b2 c), every operation rounded on its own
__device__ __forceinline__ float sample_mix(float b0, float b1, float b2, float a, float b, float c) {
    return __fadd_rn(__fadd_rn(__fmul_rn(b0, a), __fmul_rn(b1, b)), __fmul_rn(b2, c));
}

__device__ __forceinline__ void sample_normalise(const float* N, float* out) {
    // sqrtf, not __fsqrt_rn: the latter compiles to the bare v_sqrt_f32 (1 ulp), sqrtf to its correctly rounded refinement
    const float length = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(N[0], N[0]), __fmul_rn(N[1], N[1])), __fmul_rn(N[2], N[2])));
    const bool fine = mesh_finite(length) && length > 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) out[d] = fine ? __fdiv_rn(N[d], length) : 0.f;
}

__global__ __launch_bounds__(256) void k_sample_draw(SampleParams s) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= (long long)s.groups * s.samples) return;
    const int g = (int)(at / s.samples), i = (int)(at - (long long)g * s.samples);
    const int tfirst = as_global(s.tfirst)[g], tsize = as_global(s.tfirst)[g + 1] - tfirst;
    const int vfirst = as_global(s.vfirst)[g], vsize = as_global(s.vfirst)[g + 1] - vfirst;
    const unsigned long long W = as_global(s.gtotal)[g];
    const SampleDraw d = sample_draw(s, g, i);
    int t = -1;
    float b1 = 0.f, b2 = 0.f, point[3] = {0.f, 0.f, 0.f}, normal[3] = {0.f, 0.f, 0.f};
    unsigned int U = 0, V = 0;
    if (W != 0 && tsize > 0) {
        const unsigned long long pick = __umul64hi(d.r, W);
        const PR_GLOBAL_AS unsigned long long* prefix = (const PR_GLOBAL_AS unsigned long long*)as_global(s.area) + tfirst;
        int lo = 0, hi = tsize;               // the first triangle with W_t > pick lies in [lo, hi]: at most 31 steps
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (prefix[mid] > pick) hi = mid;
            else lo = mid + 1;
        }
        if (lo < tsize) {                     // (always: W_last = W > pick - unless the workspace was damaged)
            const MeshCorners c = sample_corners(s, tfirst, lo, vsize);
            if (c.in_range) {                 // (always: only a valid triangle has a weight)
                t = lo;
                U = d.U;
                V = d.V;
                b1 = (float)U * 5.9604644775390625e-8f;
                b2 = (float)V * 5.9604644775390625e-8f;
                const float b0 = (float)(SAMPLE_ONE - U - V) * 5.9604644775390625e-8f;
                const PR_GLOBAL_AS float* v = as_global(s.vertices) + (size_t)vfirst * 3;
                const PR_GLOBAL_AS float* a = v + (size_t)c.i[0] * 3;
                const PR_GLOBAL_AS float* b = v + (size_t)c.i[1] * 3;
                const PR_GLOBAL_AS float* cc = v + (size_t)c.i[2] * 3;
#pragma unroll
                for (int x = 0; x < 3; ++x) point[x] = sample_mix(b0, b1, b2, a[x], b[x], cc[x]);
                if (s.out_normals) {
                    float N[3];
                    if (s.face) {
                        float e1[3], e2[3];
#pragma unroll
                        for (int x = 0; x < 3; ++x) {
                            e1[x] = __fsub_rn(b[x], a[x]);
                            e2[x] = __fsub_rn(cc[x], a[x]);
                        }
                        N[0] = __fsub_rn(__fmul_rn(e1[1], e2[2]), __fmul_rn(e1[2], e2[1]));
                        N[1] = __fsub_rn(__fmul_rn(e1[2], e2[0]), __fmul_rn(e1[0], e2[2]));
                        N[2] = __fsub_rn(__fmul_rn(e1[0], e2[1]), __fmul_rn(e1[1], e2[0]));
                    } else {
                        const PR_GLOBAL_AS float* n = as_global(s.normals) + (size_t)vfirst * 3;
#pragma unroll
                        for (int x = 0; x < 3; ++x)
                            N[x] = sample_mix(b0, b1, b2, n[(size_t)c.i[0] * 3 + x], n[(size_t)c.i[1] * 3 + x], n[(size_t)c.i[2] * 3 + x]);
                    }
                    sample_normalise(N, normal);
                }
            }
        }
    }
    const size_t row = (size_t)at;
#pragma unroll
    for (int x = 0; x < 3; ++x) as_global(s.points)[row * 3 + x] = point[x];
    if (s.triangle) as_global(s.triangle)[row] = t;
    if (s.barycentric) {
        as_global(s.barycentric)[row * 2 + 0] = b1;
        as_global(s.barycentric)[row * 2 + 1] = b2;
    }
    if (s.out_normals) {
#pragma unroll
        for (int x = 0; x < 3; ++x) as_global(s.out_normals)[row * 3 + x] = normal[x];
    }
    const sample_int4 record = {t, (int)U, (int)V, 0};
    *(PR_GLOBAL_AS sample_int4*)(as_global(s.record) + row * 4) = record;
}

// Lanes across the columns.  Work item w of the flat index covers unit w % L of sample w / L, L = C / 4 units of four columns (vec) or
// C units of one: consecutive lanes read consecutive words of a corner row and write consecutive words of the output.
template <int VEC>
__global__ __launch_bounds__(256) void k_sample_rows(SampleParams s) {
    const unsigned long long L = (unsigned long long)(s.width / VEC);
    const unsigned long long total = (unsigned long long)s.groups * (unsigned long long)s.samples * L;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long w = (unsigned long long)blockIdx.x * 256 + threadIdx.x; w < total; w += stride) {
        const unsigned long long sample = w / L;
        const int unit = (int)(w - sample * L);
        const int g = (int)(sample / (unsigned long long)s.samples);
        const sample_int4 rec = *(const PR_GLOBAL_AS sample_int4*)(as_global(s.record) + sample * 4);
        const int tfirst = as_global(s.tfirst)[g], tsize = as_global(s.tfirst)[g + 1] - tfirst;
        const int vfirst = as_global(s.vfirst)[g], vsize = as_global(s.vfirst)[g + 1] - vfirst;
        float out[VEC];
#pragma unroll
        for (int x = 0; x < VEC; ++x) out[x] = 0.f;
        const unsigned int U = (unsigned int)rec.y, V = (unsigned int)rec.z;
        // the record is read from the workspace: checked here
        if (rec.x >= 0 && rec.x < tsize && U <= SAMPLE_ONE && V <= SAMPLE_ONE && U + V <= SAMPLE_ONE) {
            const MeshCorners c = sample_corners(s, tfirst, rec.x, vsize);
            if (c.in_range) {
                const float b1 = (float)U * 5.9604644775390625e-8f, b2 = (float)V * 5.9604644775390625e-8f;
                const float b0 = (float)(SAMPLE_ONE - U - V) * 5.9604644775390625e-8f;
                const PR_GLOBAL_AS float* rows = as_global(s.attributes) + (size_t)vfirst * s.width + (size_t)unit * VEC;
                const PR_GLOBAL_AS float* a = rows + (size_t)c.i[0] * s.width;
                const PR_GLOBAL_AS float* b = rows + (size_t)c.i[1] * s.width;
                const PR_GLOBAL_AS float* cc = rows + (size_t)c.i[2] * s.width;
                if constexpr (VEC == 4) {
                    const f32x4_t ra = *(const PR_GLOBAL_AS f32x4_t*)a, rb = *(const PR_GLOBAL_AS f32x4_t*)b, rc = *(const PR_GLOBAL_AS f32x4_t*)cc;
                    out[0] = sample_mix(b0, b1, b2, ra.x, rb.x, rc.x);
                    out[1] = sample_mix(b0, b1, b2, ra.y, rb.y, rc.y);
                    out[2] = sample_mix(b0, b1, b2, ra.z, rb.z, rc.z);
                    out[3] = sample_mix(b0, b1, b2, ra.w, rb.w, rc.w);
                } else {
                    out[0] = sample_mix(b0, b1, b2, a[0], b[0], cc[0]);
                }
            }
        }
        PR_GLOBAL_AS float* to = as_global(s.out_attributes) + w * VEC;        // (sample * C + unit * VEC)
        if constexpr (VEC == 4) {
            const f32x4_t row = {out[0], out[1], out[2], out[3]};
            *(PR_GLOBAL_AS f32x4_t*)to = row;
        } else {
            to[0] = out[0];
        }
    }
}

struct SamplePlan {
    size_t vfirst, tfirst, tblk, area, bmax, bvalid, bzero, bsum, boff, gmax, gtotal, record, bytes;
    int BT;
};

// Host checks of both entry points: no device work.
static int plan_sample(const pr_mesh_sample_t* s, const char* who, SamplePlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    PR_REQUIRE((s->flags & ~PR_SAMPLE_FACE_NORMALS) == 0, "%s: unknown flag bits 0x%x (PR_SAMPLE_FACE_NORMALS or 0)", who, s->flags);
    PR_REQUIRE(s->total_vertices >= 0 && s->total_triangles >= 0, "%s: negative total (total_vertices %d, total_triangles %d)", who,
               s->total_vertices, s->total_triangles);
    PR_REQUIRE(s->samples >= 0, "%s: samples %d (>= 0)", who, s->samples);
    PR_REQUIRE((double)s->groups * (double)s->samples < 2147483648.0, "%s: groups * samples must stay below 2^31 (%d * %d)", who, s->groups,
               s->samples);
    PR_REQUIRE(s->vertices != nullptr, "%s: NULL vertices", who);
    PR_REQUIRE(s->triangles != nullptr, "%s: NULL triangles", who);
    PR_REQUIRE(s->vertex_offsets && s->triangle_offsets, "%s: NULL offsets (vertex_offsets / triangle_offsets)", who);
    PR_REQUIRE(s->points != nullptr, "%s: NULL points (always written)", who);
    PR_REQUIRE(s->counts != nullptr, "%s: NULL counts (always written)", who);
    PR_REQUIRE(s->measures != nullptr, "%s: NULL measures (always written)", who);
    PR_REQUIRE(!s->out_attributes || s->attributes, "%s: out_attributes without attributes", who);
    PR_REQUIRE(!s->attributes || (s->attribute_width >= 1 && s->attribute_width <= SAMPLE_MAX_WIDTH), "%s: attribute_width %d (1 .. %d)",
               who, s->attribute_width, SAMPLE_MAX_WIDTH);
    PR_REQUIRE(!s->out_normals || s->normals || (s->flags & PR_SAMPLE_FACE_NORMALS),
               "%s: out_normals needs normals or PR_SAMPLE_FACE_NORMALS", who);
    PR_REQUIRE((double)s->total_triangles + 256.0 * (double)s->groups < 2147483648.0,
               "%s: mesh too large: total_triangles + 256 groups must stay below 2^31 (the block counts are int32)", who);
    const void* in[6] = {s->vertices, s->triangles, s->vertex_offsets, s->triangle_offsets, s->normals, s->attributes};
    const void* out[7] = {s->points, s->triangle, s->barycentric, s->out_normals, s->out_attributes, s->counts, s->measures};
    for (int o = 0; o < 7; ++o)
        for (int i = 0; i < 6; ++i) PR_REQUIRE(out[o] == nullptr || out[o] != in[i], "%s: an output aliases an input", who);
    plan->BT = (s->total_triangles + 255) / 256 + s->groups;
    const size_t T = (size_t)s->total_triangles, B = (size_t)plan->BT, G = (size_t)s->groups;
    const size_t table = (G + 1) * sizeof(int32_t);
    size_t at = 0;
    plan->vfirst = workspace_region(&at, table);
    plan->tfirst = workspace_region(&at, table);
    plan->tblk = workspace_region(&at, table);
    plan->area = workspace_region(&at, 8 * T);
    plan->bmax = workspace_region(&at, 8 * B);
    plan->bvalid = workspace_region(&at, 4 * B);
    plan->bzero = workspace_region(&at, 4 * B);
    plan->bsum = workspace_region(&at, 8 * B);
    plan->boff = workspace_region(&at, 8 * B);
    plan->gmax = workspace_region(&at, 8 * G);
    plan->gtotal = workspace_region(&at, 8 * G);
    plan->record = workspace_region(&at, 16 * G * (size_t)s->samples);
    plan->bytes = at;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_mesh_sample_workspace_size(const pr_mesh_sample_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_mesh_sample_workspace_size: NULL bytes");
    pr::SamplePlan plan;
    PR_TRY(pr::plan_sample(s, "pr_mesh_sample_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_mesh_sample(const pr_mesh_sample_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    static_assert(sizeof(pr_mesh_sample_t) == 144, "the header states this size");
    SamplePlan plan;
    PR_TRY(plan_sample(s, "pr_mesh_sample", &plan));
    PR_TRY(check_workspace("pr_mesh_sample", workspace, workspace_bytes, plan.bytes));
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    SampleParams p;
    memset(&p, 0, sizeof(p));
    p.groups = s->groups;
    p.V = s->total_vertices;
    p.T = s->total_triangles;
    p.BT = plan.BT;
    p.samples = s->samples;
    p.width = s->attributes ? s->attribute_width : 0;
    p.face = (s->flags & PR_SAMPLE_FACE_NORMALS) ? 1 : 0;
    p.vec = p.width % 4 == 0 && (((uintptr_t)s->attributes | (uintptr_t)s->out_attributes) & 15) == 0;
    const unsigned long long key = noise_mix(s->seed);
    p.k0 = (unsigned int)key;
    p.k1 = (unsigned int)(key >> 32);
    p.first = s->first_sample;
    p.vertices = s->vertices;
    p.triangles = s->triangles;
    p.vertex_offsets = s->vertex_offsets;
    p.triangle_offsets = s->triangle_offsets;
    p.normals = s->normals;
    p.attributes = s->attributes;
    p.points = s->points;
    p.triangle = s->triangle;
    p.barycentric = s->barycentric;
    p.out_normals = s->out_normals;
    p.out_attributes = s->out_attributes;
    p.counts = s->counts;
    p.measures = s->measures;
    p.vfirst = (int32_t*)(ws + plan.vfirst);
    p.tfirst = (int32_t*)(ws + plan.tfirst);
    p.tblk = (int32_t*)(ws + plan.tblk);
    p.area = (double*)(ws + plan.area);
    p.bmax = (double*)(ws + plan.bmax);
    p.bvalid = (int32_t*)(ws + plan.bvalid);
    p.bzero = (int32_t*)(ws + plan.bzero);
    p.bsum = (unsigned long long*)(ws + plan.bsum);
    p.boff = (unsigned long long*)(ws + plan.boff);
    p.gmax = (double*)(ws + plan.gmax);
    p.gtotal = (unsigned long long*)(ws + plan.gtotal);
    p.record = (int32_t*)(ws + plan.record);
    const size_t drawn = (size_t)s->groups * (size_t)s->samples;
    const dim3 triangle_grid((unsigned)plan.BT), group_grid((unsigned)s->groups);
    const dim3 draw_grid((unsigned)(drawn ? (drawn + 255) / 256 : 1));      // (no sample: one block that returns)
    hipLaunchKernelGGL(k_sample_init, dim3(1), dim3(64), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_area, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_max, group_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_weight, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_scan, group_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_prefix, triangle_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_draw, draw_grid, dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (s->out_attributes) {
        const size_t items = drawn * (size_t)(p.width / (p.vec ? 4 : 1));
        const dim3 row_grid((unsigned)(items ? ((items + 255) / 256 < 65536 ? (items + 255) / 256 : 65536) : 1));
        if (p.vec) hipLaunchKernelGGL(k_sample_rows<4>, row_grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL(k_sample_rows<1>, row_grid, dim3(256), 0, st, p);
        PR_LAUNCH_CHECK();
    }
    return PR_OK;
}
