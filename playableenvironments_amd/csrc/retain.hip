// Retained per-sample state of chosen objects across evaluation frames (pr_render_forward_retained, include/playrender.h): the
// cache plan, the host digest, and the small kernels around the renderer's own launches - probe (compare the cached keys with the
// call's inputs), decide (reuse flags, invalidation), gate (row counts of reused objects -> 0), commit + seal (store the keys): six launches per call
// and one gate per level, whatever the number of retained objects.
#include "pr_common.h"

#include <stddef.h>

namespace pr {

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
static_assert(sizeof(RetainHeader) <= 256, "the cache header is one 256-byte region");

// Feature-row width of a level's compact rows, as make_plan sizes them.
static int feat_row_floats(const pr_call_t& c, const pr_object_t* objs, const pr_object_model_t& m) {
    if (!defer_active(c, objs)) return m.output_features;
    ModelDims d;
    if (compute_dims(m, &d) != PR_OK) return m.output_features;
    return hidden_row_floats(d.W2);
}

int make_retain_plan(const pr_call_t& c, const pr_object_t* objs, uint32_t mask, RetainPlan* plan) {
    memset(plan, 0, sizeof(*plan));
    size_t off = align_up(sizeof(RetainHeader));
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align_up(bytes);
        return at;
    };
    const size_t N = (size_t)c.frames, nr = N * (size_t)c.rays;
    plan->origins = take(4 * N * 3);
    plan->directions = take(4 * nr * 3);
    const int ntypes = c.use_fine ? 2 : 1;
    for (int k = 0; k < c.objects; ++k) {
        if (!((mask >> k) & 1u)) continue;
        RetainObjectPlan& o = plan->obj[k];
        o.w2o = take(4 * N * 12);
        o.presence = take(4 * N);
        o.style = take(4 * N * (size_t)objs[k].coarse.style_features);
        o.deformation = take(4 * N * (size_t)objs[k].coarse.deformation_features);
        for (int t = 0; t < ntypes; ++t) {
            const pr_object_model_t& m = t ? objs[k].fine : objs[k].coarse;
            ModelDims d;
            PR_TRY(compute_dims(m, &d));
            o.bn[t][0] = take(4 * (size_t)d.W);
            o.bn[t][1] = take(4 * (size_t)d.W);
            o.bn[t][2] = take(4 * (size_t)d.W2);
            o.bn[t][3] = take(4 * (size_t)d.W2);
            o.occ[t] = m.kind == 1 ? (size_t)-1 : take(4 * N * (size_t)RETAIN_OCC_WORDS);
        }
        for (int t = 0; t < ntypes; ++t) {
            const pr_object_model_t& m = t ? objs[k].fine : objs[k].coarse;
            const size_t cap = nr * (size_t)m.positions;
            o.t[t] = take(4 * cap);
            o.sigma[t] = take(4 * cap);
            o.slot[t] = take(4 * cap);
            o.dispmag[t] = m.has_bender ? take(4 * cap) : (size_t)-1;
            o.feat[t] = take(4 * cap * (size_t)feat_row_floats(c, objs, m));
        }
    }
    plan->bytes = off;
    return PR_OK;
}

// FNV-1a over what the host sees of the retained objects and the call
static uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

static uint64_t host_digest(const pr_call_t& c, const pr_object_t* objs, const pr_occupancy_t* occ, const pr_fine_guide_t* guide,
                            const pr_retained_t& r) {
    uint64_t h = 0xCBF29CE484222325ull;
    const uint32_t honoured = (c.flags & (PR_FLAG_CANONICAL_POSE | PR_FLAG_FIX_OVERLAPS | PR_FLAG_SIGMOID_FEATURES)) |
                              (gate_active(c) ? PR_FLAG_GATE_HEAD : 0u) | (defer_active(c, objs) ? PR_FLAG_DEFER_PROJECTION : 0u);
    const int32_t head[8] = {(int32_t)honoured, c.precision, c.frames, c.rays, c.objects, c.use_fine ? 1 : 0, (int32_t)r.object_mask, 0};
    h = fnv(h, head, sizeof(head));
    h = fnv(h, &r.host_key, sizeof(r.host_key));
    // the fine guide: a retained object's fine arrays are a function of its parameters too (the threshold by its bit pattern)
    uint32_t fg[3] = {0u, 0u, 0u};
    if (guide && guide->object_mask) {
        fg[0] = guide->object_mask;
        fg[1] = (uint32_t)guide->guard;
        memcpy(&fg[2], &guide->threshold, sizeof(float));
    }
    h = fnv(h, fg, sizeof(fg));
    const size_t scalars = offsetof(pr_object_model_t, backbone);   // kind .. bn_eps: dimensions, octave weights, box, depth range
    for (int k = 0; k < c.objects; ++k) {
        if (!((r.object_mask >> k) & 1u)) continue;
        h = fnv(h, &k, sizeof(k));
        h = fnv(h, &objs[k].coarse, scalars);
        if (c.use_fine) {
            h = fnv(h, &objs[k].fine, scalars);
            h = fnv(h, &c.positions_fine[k], sizeof(int32_t));
        }
        for (int t = 0; t < (c.use_fine ? 2 : 1); ++t) {
            int32_t g[5] = {0, 0, 0, 0, 0};
            const pr_occupancy_grid_t* grid = occ ? (t ? &occ->fine[k] : &occ->coarse[k]) : nullptr;
            if (grid && grid->bits) {
                g[0] = 1; g[1] = grid->cells[0]; g[2] = grid->cells[1]; g[3] = grid->cells[2]; g[4] = grid->words;
            }
            h = fnv(h, g, sizeof(g));
        }
    }
    return h;
}

static int occ_key_words(const pr_occupancy_grid_t& g) {
    return (int)(((long)g.cells[0] * g.cells[1] * g.cells[2] + 31) / 32);
}

// Host checks of pr_render_forward_retained: no device work, so that a refusal precedes everything else.  Fills `ctx`.
int validate_retained(const pr_call_t& c, const pr_object_t* objs, const pr_occupancy_t* occ, const pr_fine_guide_t* guide,
                      const pr_retained_t* r, const pr_outputs_t* coarse, const pr_outputs_t* fine, RetainCtx* ctx) {
    PR_REQUIRE(!(c.flags & PR_FLAG_PERTURB), "retention applies to unperturbed evaluation calls only: PR_FLAG_PERTURB is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_TRAIN_BN), "retention applies to evaluation calls only: PR_FLAG_TRAIN_BN is set (the running statistics move)");
    PR_REQUIRE(!(c.flags & PR_FLAG_SAVE_FOR_BACKWARD), "retention applies to evaluation calls only: PR_FLAG_SAVE_FOR_BACKWARD is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_NAIVE_MLP), "retention is not supported with PR_FLAG_NAIVE_MLP");
    bool noise = c.noise_coarse.integrate_global || c.noise_fine.integrate_global;
    for (int k = 0; k < PR_MAX_OBJECTS; ++k) noise = noise || c.noise_coarse.integrate[k] || c.noise_fine.integrate[k];
    PR_REQUIRE(!noise, "retention applies to unperturbed evaluation calls only: an integrate-noise pointer is set");
    PR_REQUIRE((r->object_mask >> c.objects) == 0,
               "retained object_mask 0x%x names an object at or beyond objects = %d", r->object_mask, c.objects);
    const pr_outputs_t* outs[2] = {coarse, c.use_fine ? fine : nullptr};
    for (int k = 0; k < c.objects; ++k) {
        if (!((r->object_mask >> k) & 1u)) continue;
        for (int t = 0; t < 2; ++t)
            PR_REQUIRE(!(outs[t] && outs[t]->sample_delta[k]),
                       "object %d is retained: its sample_delta export must be NULL (the dense displacement is not cached)", k);
        for (int t = 0; t < (c.use_fine ? 2 : 1); ++t) {
            const pr_object_model_t& m = t ? objs[k].fine : objs[k].coarse;
            PR_REQUIRE(m.bn1_mean && m.bn1_var && m.bn4_mean && m.bn4_var, "object %d is retained: BatchNorm running statistics missing", k);
            const pr_occupancy_grid_t* g = occ ? (t ? &occ->fine[k] : &occ->coarse[k]) : nullptr;
            if (g && g->bits)
                PR_REQUIRE(occ_key_words(*g) <= RETAIN_OCC_WORDS,
                           "object %d is retained: its occupancy grid has more than %d cells (the cache keeps a copy of the bits)", k,
                           RETAIN_OCC_WORDS * 32);
        }
    }
    PR_REQUIRE(r->cache != nullptr && ((uintptr_t)r->cache & 255) == 0, "retained cache must be a 256-byte aligned device pointer");
    PR_TRY(make_retain_plan(c, objs, r->object_mask, &ctx->plan));
    PR_REQUIRE(r->cache_bytes >= ctx->plan.bytes, "retained cache too small: %zu bytes given, %zu needed", r->cache_bytes, ctx->plan.bytes);
    ctx->base = static_cast<char*>(r->cache);
    ctx->hdr = reinterpret_cast<RetainHeader*>(r->cache);
    ctx->mask = r->object_mask;
    ctx->digest = host_digest(c, objs, occ, guide, *r);
    ctx->reused = r->reused;
    ctx->occupancy = occ;
    return PR_OK;
}

// ---------------------------------------------------------------------------------------------
// Key segments: a (rows, row_words) block of the call's inputs - rows `stride` elements apart, 32-bit words or bytes - and its
// compact copy in the cache (one word per element).
// ---------------------------------------------------------------------------------------------
struct RetainSeg {
    const void* cur;
    uint32_t* cached;
    int stride;           // elements between rows of `cur`
    int rows, row_words;
    short bytes;          // 1: `cur` holds bytes (object_in_scene)
    short object;         // the key this segment belongs to: -1 the camera, k = retained object k
};
// the segments of a call travel by value in the kernel arguments: 2 of the camera, at most 4 + 2 * 5 per retained object
constexpr int RETAIN_MAX_SEGS = 2 + 14 * PR_MAX_OBJECTS;
struct RetainJob {
    RetainSeg seg[RETAIN_MAX_SEGS];
    int count;
};
static_assert(sizeof(RetainSeg) == 32 && sizeof(RetainJob) + 16 <= 4096, "the segment table must fit the kernel argument segment");

__device__ __forceinline__ uint32_t seg_word(const RetainSeg& s, size_t i) {
    const size_t r = i / (size_t)s.row_words, col = i - r * (size_t)s.row_words;
    const size_t at = r * (size_t)s.stride + col;
    return s.bytes ? (uint32_t) static_cast<const uint8_t*>(s.cur)[at] : static_cast<const uint32_t*>(s.cur)[at];
}

// contiguous word segments whose two addresses allow 16-byte loads
__device__ __forceinline__ bool seg_vector(const RetainSeg& s) {
    return s.rows == 1 && !s.bytes && (((uintptr_t)s.cur | (uintptr_t)s.cached) & 15) == 0;
}

// ONE launch for every key of the call, grid (blocks, segments).  Compares segment blockIdx.y with its cached copy as 32-bit
// words; a wave that saw a difference ORs one bit into the mismatch word of the segment's key.
__global__ __launch_bounds__(256) void k_retain_probe(RetainJob job, RetainHeader* hdr) {
    const RetainSeg& s = job.seg[blockIdx.y];
    const size_t total = (size_t)s.rows * (size_t)s.row_words;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    bool differs = false;
    size_t done = 0;
    if (seg_vector(s)) {
        const uint4* a = static_cast<const uint4*>(s.cur);
        const uint4* b = reinterpret_cast<const uint4*>(s.cached);
        const size_t n16 = total / 4;
        for (size_t i = first; i < n16; i += step) {
            const uint4 x = a[i], y = b[i];
            differs = differs || x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
        }
        done = n16 * 4;
    }
    for (size_t i = done + first; i < total; i += step) differs = differs || seg_word(s, i) != s.cached[i];
    if (__ballot(differs) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&hdr->mismatch[s.object + 1], 1u);
}

// The same geometry, copying: the keys of the camera (always) and of every retained object that this call rendered.
__global__ __launch_bounds__(256) void k_retain_commit(RetainJob job, const RetainHeader* hdr) {
    const RetainSeg& s = job.seg[blockIdx.y];
    if (s.object >= 0 && hdr->reuse[s.object]) return;
    const size_t total = (size_t)s.rows * (size_t)s.row_words;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    size_t done = 0;
    if (seg_vector(s)) {
        const uint4* a = static_cast<const uint4*>(s.cur);
        uint4* b = reinterpret_cast<uint4*>(s.cached);
        const size_t n16 = total / 4;
        for (size_t i = first; i < n16; i += step) b[i] = a[i];
        done = n16 * 4;
    }
    for (size_t i = done + first; i < total; i += step) s.cached[i] = seg_word(s, i);
}

// One wave, behind the probe: object k is reused iff the cache is valid and the digest, the camera and its key all match.  An
// object that is not reused loses its valid state HERE, before any kernel of the call overwrites its arrays; a camera or digest
// mismatch takes the whole cache's.  Leaves the mismatch words zero for the next call.
__global__ __launch_bounds__(64) void k_retain_decide(RetainHeader* hdr, uint32_t mask, int objects, uint32_t digest_lo, uint32_t digest_hi,
                                                      int32_t* reused) {
    const int k = threadIdx.x;
    const bool frame_ok = hdr->valid == 1u && hdr->digest[0] == digest_lo && hdr->digest[1] == digest_hi && hdr->mismatch[0] == 0u;
    if (k < PR_MAX_OBJECTS) {
        const bool retained = k < objects && ((mask >> k) & 1u);
        const bool ok = retained && frame_ok && hdr->obj_valid[k] == 1u && hdr->mismatch[1 + k] == 0u;
        hdr->reuse[k] = ok ? 1 : 0;
        if (!ok) hdr->obj_valid[k] = 0u;
        if (reused && k < objects) reused[k] = ok ? 1 : 0;
    }
    __syncthreads();
    if (k <= PR_MAX_OBJECTS) hdr->mismatch[k] = 0u;
    if (k == 0 && !frame_ok) hdr->valid = 0u;
}

// Behind the block scans of a level: a reused object reaches the MLP launch as an object with zero rows.
__global__ __launch_bounds__(64) void k_retain_gate(const RetainHeader* hdr, int32_t* totals, uint32_t mask, int first, int count) {
    const int k = first + threadIdx.x;
    if (threadIdx.x >= count || !((mask >> k) & 1u)) return;
    if (hdr->reuse[k]) totals[k] = 0;
}

// The last launch of the call, behind the key copies: the rendered objects, the camera key and the digest become valid.
__global__ __launch_bounds__(64) void k_retain_seal(RetainHeader* hdr, uint32_t mask, int objects, uint32_t digest_lo, uint32_t digest_hi) {
    const int k = threadIdx.x;
    if (k < objects && ((mask >> k) & 1u) && !hdr->reuse[k]) hdr->obj_valid[k] = 1u;
    if (k == 0) {
        hdr->digest[0] = digest_lo;
        hdr->digest[1] = digest_hi;
        hdr->valid = 1u;
    }
}

__global__ __launch_bounds__(64) void k_retain_reset(uint32_t* header) { header[threadIdx.x] = 0u; }

static RetainSeg make_seg(const void* cur, char* base, size_t at, int rows, int row_words, long stride, int bytes, int object) {
    RetainSeg s;
    s.cur = cur; s.cached = reinterpret_cast<uint32_t*>(base + at); s.stride = (int)stride; s.rows = rows; s.row_words = row_words;
    s.bytes = (short)bytes; s.object = (short)object;
    return s;
}

// The key segments of the call: the camera's, then those of every retained object.  *blocks: grid width for the longest one.
static int build_job(const pr_call_t& c, const pr_object_t* objs, const RetainCtx& rc, RetainJob* job, unsigned* blocks) {
    memset(job, 0, sizeof(*job));
    int n = 0;
    const int N = c.frames, K = c.objects;
    PR_REQUIRE((long)N * c.rays * 3 < (1L << 31), "retention: too many rays");
    job->seg[n++] = make_seg(c.ray_origins, rc.base, rc.plan.origins, 1, N * 3, 0, 0, -1);
    job->seg[n++] = make_seg(c.ray_directions, rc.base, rc.plan.directions, 1, N * c.rays * 3, 0, 0, -1);
    for (int k = 0; k < K; ++k) {
        if (!((rc.mask >> k) & 1u)) continue;
        const RetainObjectPlan& o = rc.plan.obj[k];
        const int S = objs[k].coarse.style_features, D = objs[k].coarse.deformation_features;
        job->seg[n++] = make_seg(c.w2o + (size_t)k * 12, rc.base, o.w2o, N, 12, (long)K * 12, 0, k);
        job->seg[n++] = make_seg(c.object_in_scene + k, rc.base, o.presence, N, 1, K, 1, k);
        if (S > 0) job->seg[n++] = make_seg(c.style + (size_t)k * S, rc.base, o.style, N, S, (long)K * S, 0, k);
        if (D > 0) job->seg[n++] = make_seg(c.deformation + (size_t)k * D, rc.base, o.deformation, N, D, (long)K * D, 0, k);
        for (int t = 0; t < (c.use_fine ? 2 : 1); ++t) {
            const pr_object_model_t& m = t ? objs[k].fine : objs[k].coarse;
            ModelDims d;
            PR_TRY(compute_dims(m, &d));
            job->seg[n++] = make_seg(m.bn1_mean, rc.base, o.bn[t][0], 1, d.W, 0, 0, k);
            job->seg[n++] = make_seg(m.bn1_var, rc.base, o.bn[t][1], 1, d.W, 0, 0, k);
            job->seg[n++] = make_seg(m.bn4_mean, rc.base, o.bn[t][2], 1, d.W2, 0, 0, k);
            job->seg[n++] = make_seg(m.bn4_var, rc.base, o.bn[t][3], 1, d.W2, 0, 0, k);
            const pr_occupancy_grid_t* g = rc.occupancy ? (t ? &rc.occupancy->fine[k] : &rc.occupancy->coarse[k]) : nullptr;
            if (g && g->bits) job->seg[n++] = make_seg(g->bits, rc.base, o.occ[t], N, occ_key_words(*g), g->words, 0, k);
        }
    }
    job->count = n;      // <= RETAIN_MAX_SEGS by construction
    size_t most = 1;
    for (int i = 0; i < n; ++i) {
        const size_t total = (size_t)job->seg[i].rows * (size_t)job->seg[i].row_words;
        if (total > most) most = total;
    }
    const size_t b = (most + 1023) / 1024;       // four words per thread where the loads are 16 bytes wide
    *blocks = (unsigned)(b > 256 ? 256 : b);
    return PR_OK;
}

// Two launches: the probe over every key segment of the call, then the decision.
int launch_retain_probe(const pr_call_t& c, const pr_object_t* objs, const RetainCtx& rc, hipStream_t s) {
    static thread_local RetainJob job;
    unsigned blocks = 1;
    PR_TRY(build_job(c, objs, rc, &job, &blocks));
    hipLaunchKernelGGL(k_retain_probe, dim3(blocks, job.count), dim3(256), 0, s, job, rc.hdr);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_retain_decide, dim3(1), dim3(64), 0, s, rc.hdr, rc.mask, c.objects, (uint32_t)rc.digest, (uint32_t)(rc.digest >> 32),
                       rc.reused);
    PR_LAUNCH_CHECK();
    return PR_OK;
}

int launch_retain_gate(const RetainCtx& rc, int32_t* totals, int first, int count, hipStream_t s) {
    hipLaunchKernelGGL(k_retain_gate, dim3(1), dim3(64), 0, s, rc.hdr, totals, rc.mask, first, count);
    PR_LAUNCH_CHECK();
    return PR_OK;
}

// Two launches: the key copies, then the seal.
int launch_retain_commit(const pr_call_t& c, const pr_object_t* objs, const RetainCtx& rc, hipStream_t s) {
    static thread_local RetainJob job;
    unsigned blocks = 1;
    PR_TRY(build_job(c, objs, rc, &job, &blocks));
    hipLaunchKernelGGL(k_retain_commit, dim3(blocks, job.count), dim3(256), 0, s, job, rc.hdr);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_retain_seal, dim3(1), dim3(64), 0, s, rc.hdr, rc.mask, c.objects, (uint32_t)rc.digest, (uint32_t)(rc.digest >> 32));
    PR_LAUNCH_CHECK();
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_retained_size(const pr_call_t* call, const pr_object_t* objects, uint32_t object_mask, size_t* bytes) {
    PR_REQUIRE(call && objects && bytes, "pr_retained_size: NULL argument");
    PR_TRY(pr::validate_call(*call, objects));
    PR_REQUIRE((object_mask >> call->objects) == 0, "retained object_mask 0x%x names an object at or beyond objects = %d", object_mask,
               call->objects);
    pr::RetainPlan plan;
    PR_TRY(pr::make_retain_plan(*call, objects, object_mask, &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_retained_reset(void* cache, size_t cache_bytes, void* stream) {
    PR_REQUIRE(cache != nullptr && ((uintptr_t)cache & 255) == 0, "retained cache must be a 256-byte aligned device pointer");
    PR_REQUIRE(cache_bytes >= 256, "retained cache too small: %zu bytes given, the header alone takes 256", cache_bytes);
    hipLaunchKernelGGL(pr::k_retain_reset, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<uint32_t*>(cache));
    PR_LAUNCH_CHECK();
    return PR_OK;
}
