// Host orchestration of one renderer call (the body of ObjectComposer.forward,
// model/object_composer.py:786-892) and the small introspection entry points of the C ABI.
#include "pr_common.h"

#include <stdarg.h>

#include <atomic>
#include <mutex>
#include <vector>

namespace pr {

// ---------------------------------------------------------------------------------------------
// Kernel timing
// ---------------------------------------------------------------------------------------------
struct ProfileRecord { int category; hipEvent_t start, stop; };
static std::atomic<bool> g_profile_on{false};   // bench-only switch; launches read it relaxed, no lock on the product path
static std::vector<ProfileRecord> g_profile;
static std::mutex g_profile_mutex;

int prepare_kernel(const void* kernel, int lds_bytes, int* cu_count) {
    struct Entry { const void* kernel; int device; int cus; };
    static std::vector<Entry> done;
    static std::mutex guard;
    int dev = 0;
    PR_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(guard);
    for (const Entry& e : done)
        if (e.kernel == kernel && e.device == dev) {
            if (cu_count) *cu_count = e.cus;
            return PR_OK;
        }
    PR_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    hipDeviceProp_t prop;
    PR_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    done.push_back(Entry{kernel, dev, prop.multiProcessorCount});
    if (cu_count) *cu_count = prop.multiProcessorCount;
    return PR_OK;
}

// Every zero fill of the library is this kernel, never hipMemsetAsync: recorded into a HIP graph a memset becomes a memset NODE,
// and on ROCm 7.0.2 memset nodes stop executing after a few back-to-back replays followed by a host synchronisation (with the
// runtime's AQL packet capture on; DESIGN.md "Recorded training step") - a kernel node does not.
__global__ __launch_bounds__(256) void k_zero_fill(uint4* dst16, size_t n16, uint32_t* tail, size_t ntail) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst16[i] = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < ntail; i += (size_t)gridDim.x * 256) tail[i] = 0u;
}

int launch_zero_fill(void* dst, size_t bytes, hipStream_t s) {
    if (bytes == 0) return PR_OK;
    PR_REQUIRE((bytes & 3) == 0 && ((uintptr_t)dst & 3) == 0, "zero fill: %zu bytes at a misaligned address", bytes);
    // 16-byte stores where the address allows them, 4-byte stores for the rest (and for small misaligned regions as a whole)
    const bool aligned = ((uintptr_t)dst & 15) == 0;
    const size_t n16 = aligned ? bytes / 16 : 0;
    const size_t ntail = (bytes - n16 * 16) / 4;
    size_t blocks = ((n16 > ntail ? n16 : ntail) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_zero_fill, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<uint4*>(dst), n16,
                       reinterpret_cast<uint32_t*>(static_cast<char*>(dst) + n16 * 16), ntail);
    PR_LAUNCH_CHECK();
    return PR_OK;
}

// Geometry-only calls: the density of a skybox model is a constant, so its samples need no MLP launch - what the tile loop's
// skybox branch writes (10 where the object is present, empty_alpha where it is not, for every sample that owns a compact row).
__global__ __launch_bounds__(256) void k_skybox_sigma(SkyboxSigmaParams p) {
    const PR_GLOBAL_AS int32_t* slot = as_global(p.slot);
    const PR_GLOBAL_AS uint8_t* present = as_global(p.in_scene);
    PR_GLOBAL_AS float* sigma = as_global(p.sigma);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.samples; i += (long)gridDim.x * 256) {
        if (slot[i] < 0) continue;
        const long frame = i / p.samples_per_frame;
        sigma[i] = present[(size_t)frame * p.in_scene_stride] ? 10.0f : p.empty_alpha;
    }
}

int launch_skybox_sigma(const SkyboxSigmaParams& p, hipStream_t s) {
    if (p.samples <= 0) return PR_OK;
    long blocks = (p.samples + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_skybox_sigma, dim3((unsigned)blocks), dim3(256), 0, s, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}

ProfileScope::ProfileScope(int category, hipStream_t s) : category_(category), stream_(s), start_(nullptr), active_(false) {
    if (!g_profile_on.load(std::memory_order_relaxed)) return;
    if (hipEventCreate(&start_) != hipSuccess) return;
    if (hipEventRecord(start_, stream_) != hipSuccess) {
        (void)hipEventDestroy(start_);
        return;
    }
    active_ = true;
}

ProfileScope::~ProfileScope() {
    if (!active_) return;
    hipEvent_t stop;
    if (hipEventCreate(&stop) != hipSuccess) return;
    if (hipEventRecord(stop, stream_) != hipSuccess) {
        (void)hipEventDestroy(stop);
        (void)hipEventDestroy(start_);
        return;
    }
    std::lock_guard<std::mutex> lock(g_profile_mutex);
    g_profile.push_back(ProfileRecord{category_, start_, stop});
}

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

// ---------------------------------------------------------------------------------------------
// Workspace plan (structs in pr_common.h)
// ---------------------------------------------------------------------------------------------
static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

int validate_call(const pr_call_t& c, const pr_object_t* objs) {
    PR_REQUIRE(c.frames > 0 && c.rays > 0, "empty call: %d frames x %d rays", c.frames, c.rays);
    PR_REQUIRE(c.objects >= 1 && c.objects <= PR_MAX_OBJECTS, "objects %d out of range 1..%d", c.objects, PR_MAX_OBJECTS);
    PR_REQUIRE(c.static_objects >= 0 && c.static_objects <= c.objects, "static_objects %d out of range", c.static_objects);
    PR_REQUIRE((long)c.frames * c.rays < (1L << 31), "too many rays in one call");
    PR_REQUIRE(c.ray_origins && c.ray_directions && c.w2o && c.style && c.deformation && c.object_in_scene,
               "NULL input pointer");
    PR_REQUIRE(c.precision == PR_PRECISION_FP32 || c.precision == PR_PRECISION_F16X3 || c.precision == PR_PRECISION_F16,
               "unknown precision %d", c.precision);
    PR_REQUIRE(!(c.precision != PR_PRECISION_FP32 && (c.flags & PR_FLAG_TRAIN_BN)),
               "the fp16 kernels have no train-mode BatchNorm phases: use PR_PRECISION_FP32 for training");
    PR_REQUIRE(!(c.precision != PR_PRECISION_FP32 && (c.flags & PR_FLAG_SAVE_FOR_BACKWARD)),
               "differentiable calls run on the exact kernel: use PR_PRECISION_FP32 with PR_FLAG_SAVE_FOR_BACKWARD");
    PR_REQUIRE(!(c.flags & PR_FLAG_SAVE_FOR_BACKWARD) || !(c.flags & PR_FLAG_NAIVE_MLP), "the scalar debugging kernel saves nothing");
    for (int k = 0; k < c.objects; ++k) {
        const pr_object_model_t& m = objs[k].coarse;
        PR_REQUIRE(m.positions >= 1, "object %d: positions_count_coarse %d", k, m.positions);
        PR_REQUIRE(c.linspace_coarse[k] != nullptr, "object %d: linspace_coarse missing", k);
        PR_REQUIRE(objs[k].packed_coarse != nullptr, "object %d: packed coarse weights missing", k);
        PR_REQUIRE((long)c.frames * c.rays * (long)m.positions < (1L << 31), "too many samples in one call");
        if (c.use_fine) {
            PR_REQUIRE(c.positions_fine[k] >= 1, "object %d: positions_count_fine %d", k, c.positions_fine[k]);
            PR_REQUIRE(objs[k].fine.positions == m.positions + c.positions_fine[k],
                       "object %d: fine model positions %d != %d + %d", k, objs[k].fine.positions, m.positions,
                       c.positions_fine[k]);
            PR_REQUIRE(objs[k].packed_fine != nullptr, "object %d: packed fine weights missing", k);
            PR_REQUIRE(c.linspace_fine[k] != nullptr || c.noise_coarse.pdf[k] != nullptr ||
                           ((c.flags & PR_FLAG_DEVICE_NOISE) && (c.flags & PR_FLAG_PERTURB)),
                       "object %d: linspace_fine missing", k);
            PR_REQUIRE((long)c.frames * c.rays * (long)objs[k].fine.positions < (1L << 31), "too many samples in one call");
        }
    }
    if (c.flags & PR_FLAG_FIX_OVERLAPS) {
        for (int t = 0; t < (c.use_fine ? 2 : 1); ++t)
            for (int s = 0; s < c.static_objects; ++s)
                for (int d = c.static_objects; d < c.objects; ++d) {
                    const int ps = t ? objs[s].fine.positions : objs[s].coarse.positions;
                    const int pd = t ? objs[d].fine.positions : objs[d].coarse.positions;
                    // the reference indexes the dynamic list with the static P - 1 (object_composer.py:322)
                    PR_REQUIRE(ps <= pd, "overlap fix: static object %d has more positions (%d) than dynamic object %d (%d); "
                               "the reference raises IndexError here", s, ps, d, pd);
                }
    }
    return PR_OK;
}

// The sigma-gated feature head applies to calls whose compositing weights are a function of the raw densities alone:
// evaluation without perturbation noise, nothing saved for a backward pass, fused (unphased) MLP launches.
bool gate_active(const pr_call_t& c) {
    if (!(c.flags & PR_FLAG_GATE_HEAD) || (c.flags & PR_FLAG_GEOMETRY_ONLY)) return false;      // (a geometry-only call has no head to gate)
    if (c.flags & (PR_FLAG_PERTURB | PR_FLAG_TRAIN_BN | PR_FLAG_SAVE_FOR_BACKWARD | PR_FLAG_NAIVE_MLP)) return false;
    for (int k = 0; k < c.objects; ++k)
        if (c.noise_coarse.integrate[k] || c.noise_fine.integrate[k]) return false;
    return !c.noise_coarse.integrate_global && !c.noise_fine.integrate_global;
}

// The deferred projection (features_head.6 applied per ray, behind the compositing sums) needs the projected layer to be linear in
// the composited rows and the fused fp32 evaluation kernels: no sigmoid between the layer and the sum, no phased (training /
// differentiable) launches, not the scalar debugging kernel, not the split-precision tiers (their kernels write full rows).  Every
// object model has the three-layer head (pr_object_model_t holds no other); the pooled rows of a ray have one width, so the models
// of the call share layers_width.  Noise changes the weights only: perturbed calls are eligible.
bool defer_active(const pr_call_t& c, const pr_object_t* objs) {
    if (!(c.flags & PR_FLAG_DEFER_PROJECTION) || (c.flags & PR_FLAG_GEOMETRY_ONLY)) return false;   // (nor rows to project)
    if (c.flags & (PR_FLAG_SAVE_FOR_BACKWARD | PR_FLAG_TRAIN_BN | PR_FLAG_SIGMOID_FEATURES | PR_FLAG_NAIVE_MLP)) return false;
    if (c.precision != PR_PRECISION_FP32) return false;
    for (int k = 0; k < c.objects; ++k) {
        if (objs[k].coarse.layers_width != objs[0].coarse.layers_width) return false;
        if (c.use_fine && objs[k].fine.layers_width != objs[0].coarse.layers_width) return false;
    }
    return true;
}

int make_plan(const pr_call_t& c, const pr_object_t* objs, Plan* plan) {
    memset(plan, 0, sizeof(*plan));
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align_up(bytes);
        return at;
    };
    const size_t nr = (size_t)c.frames * c.rays;
    plan->nblocks256 = (int)((nr + 255) / 256);
    plan->block_sums = take(sizeof(int32_t) * plan->nblocks256 * c.objects);       // one region per object: the objects of a
    plan->block_offsets = take(sizeof(int32_t) * plan->nblocks256 * c.objects);    // call are placed / compacted by shared launches
    size_t max_cap = 0;
    size_t feat_bytes[2] = {0, 0};
    size_t div_t0 = 0, div_t = 0;   // divergence tangent scratch (shared by the bender objects)
    const int ntypes = c.use_fine ? 2 : 1;
    for (int t = 0; t < ntypes; ++t) {
        TypePlan& tp = plan->type[t];
        tp.totals = take(sizeof(int32_t) * PR_MAX_OBJECTS);
        tp.zero_begin = off;
        tp.head_counts = take(sizeof(int32_t) * 3 * PR_MAX_OBJECTS);
        if (c.flags & (PR_FLAG_TRAIN_BN | PR_FLAG_SAVE_FOR_BACKWARD))
            for (int k = 0; k < c.objects; ++k) {
                const pr_object_model_t& m = t ? objs[k].fine : objs[k].coarse;
                SavedPlan& sv = tp.saved[k];
                sv.stats = take(sizeof(double) * 4 * MAX_WIDTH);
                sv.stat_count = take(sizeof(int32_t) * 4);
                if ((c.flags & PR_FLAG_SAVE_FOR_BACKWARD) && m.has_bender) sv.div = take(sizeof(float) * nr * m.positions);
            }
        tp.zero_bytes = off - tp.zero_begin;
        for (int k = 0; k < c.objects; ++k) {
            const pr_object_model_t& m = t ? objs[k].fine : objs[k].coarse;
            ModelDims d;
            PR_TRY(compute_dims(m, &d));
            tp.positions[k] = m.positions;
            const size_t cap = nr * m.positions;
            if (cap > max_cap) max_cap = cap;
            tp.t[k] = take(sizeof(float) * cap);
            tp.sigma[k] = take(sizeof(float) * cap);
            tp.slot[k] = take(sizeof(int32_t) * cap);
            tp.dispmag[k] = m.has_bender ? take(sizeof(float) * cap) : (size_t)-1;
            tp.adain[k] = take(sizeof(float) * (size_t)c.frames * adain_row_floats(d));
            tp.feat[k] = feat_bytes[t];  // relative to the feature arena
            // (a geometry-only call writes no feature row: no arena)
            if (!(c.flags & PR_FLAG_GEOMETRY_ONLY))
                feat_bytes[t] += align_up(sizeof(float) * cap * (defer_active(c, objs) ? hidden_row_floats(d.W2) : m.output_features));
            if (c.flags & PR_FLAG_SAVE_FOR_BACKWARD) {
                // everything the backward pass re-reads, per object instance (compact rows, worst-case capacity)
                SavedPlan& sv = tp.saved[k];
                sv.rec_pos = take(sizeof(float) * 3 * cap);
                sv.rec_flat = take(sizeof(int32_t) * cap);
                sv.row_flags = take(sizeof(int32_t) * cap);
                sv.enc = take(sizeof(float) * cap * d.enc_pad);
                sv.act = take(sizeof(float) * cap * d.Wpad * m.backbone_count);
                sv.bits = take(relu_bits_bytes(cap, d.Wpad) * (size_t)m.backbone_count);
                sv.h1 = take(sizeof(float) * cap * d.Wpad);
                sv.h2 = take(sizeof(float) * cap * d.W2pad);
                sv.batch = take(sizeof(float) * 4 * MAX_WIDTH);
                if (m.has_bender) {
                    if (cap * d.bin_pad > div_t0) div_t0 = cap * d.bin_pad;
                    if (cap * d.BWpad > div_t) div_t = cap * d.BWpad;
                    sv.bin = take(sizeof(float) * cap * d.bin_pad);
                    sv.bact = take(sizeof(float) * cap * d.BWpad * m.bender_count);
                    sv.bbits = take(relu_bits_bytes(cap, d.BWpad) * (size_t)m.bender_count);
                    sv.braw = take(sizeof(float) * 3 * cap);
                    sv.delta = take(sizeof(float) * 3 * cap);
                }
            }
        }
    }
    plan->rec_pos = take(sizeof(float) * 3 * max_cap);
    plan->rec_flat = take(sizeof(int32_t) * max_cap);
    if (group_active(c)) {
        // one launch evaluates every object of a model type: each object keeps its own compact sample records
        // (the coarse and the fine pass of an object share them: the coarse launch has finished before the fine fill)
        for (int k = 0; k < c.objects; ++k) {
            size_t cap = nr * objs[k].coarse.positions;
            if (c.use_fine && nr * objs[k].fine.positions > cap) cap = nr * objs[k].fine.positions;
            plan->rec_pos_k[k] = take(sizeof(float) * 3 * cap);
            plan->rec_flat_k[k] = take(sizeof(int32_t) * cap);
        }
    }
    if (gate_active(c)) {   // per-workgroup stacks of pending live rows (sigma-gated head)
        plan->pend_act = take(sizeof(float) * (size_t)MAX_RESIDENT_TILES * TILE_M * MAX_WIDTH);
        plan->pend_meta = take(sizeof(int32_t) * (size_t)MAX_RESIDENT_TILES * TILE_M * 2);
    }
    if (defer_active(c, objs)) {   // per object the row sums under its own and under the global weights (shared by the model types)
        ModelDims d0;
        PR_TRY(compute_dims(objs[0].coarse, &d0));
        plan->pooled = take(sizeof(float) * 2 * (size_t)c.objects * nr * hidden_row_floats(d0.W2));
    }
    if (c.flags & (PR_FLAG_TRAIN_BN | PR_FLAG_SAVE_FOR_BACKWARD)) {   // the phased launch structure (see make_train_job)
        plan->h1 = take(sizeof(float) * max_cap * MAX_WIDTH);
        plan->h2 = take(sizeof(float) * max_cap * (MAX_WIDTH / 2 + 32));
        plan->row_flags = take(sizeof(int32_t) * max_cap);
        plan->batch_stats = take(sizeof(float) * 4 * MAX_WIDTH);
    }
    // coarse and fine feature rows share one arena: the coarse rows are dead once the coarse
    // compositing pass has run, before the first fine MLP is launched.
    if (div_t) {
        plan->div_t0 = take(sizeof(float) * div_t0);
        plan->div_ta = take(sizeof(float) * div_t);
        plan->div_tb = take(sizeof(float) * div_t);
    }
    if (c.flags & PR_FLAG_SAVE_FOR_BACKWARD) {
        // the backward pass needs the feature rows of both model types
        for (int t = 0; t < ntypes; ++t) {
            const size_t arena = take(feat_bytes[t]);
            for (int k = 0; k < c.objects; ++k) plan->type[t].feat[k] += arena;
        }
    } else {
        const size_t arena = take(feat_bytes[0] > feat_bytes[1] ? feat_bytes[0] : feat_bytes[1]);
        for (int t = 0; t < ntypes; ++t)
            for (int k = 0; k < c.objects; ++k) plan->type[t].feat[k] += arena;
    }
    plan->bytes = off;
    return PR_OK;
}

// Evaluation calls run the objects of a model type as ONE grouped launch (k_mlp_mfma_group / k_mlp_split_group).
bool group_active(const pr_call_t& c) {
    return !(c.flags & (PR_FLAG_TRAIN_BN | PR_FLAG_SAVE_FOR_BACKWARD | PR_FLAG_NAIVE_MLP)) && c.objects > 1;
}

// Differentiable calls (everything saved per object) with several objects: phase 1 of the phased launches is grouped as well.
bool group_train_active(const pr_call_t& c) {
    return (c.flags & PR_FLAG_SAVE_FOR_BACKWARD) && !(c.flags & PR_FLAG_NAIVE_MLP) && c.objects > 1;
}

void bbox_split(const pr_object_model_t& m, float* lo, float* hi, float* size) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = m.bbox[2 * a];
        hi[a] = m.bbox[2 * a + 1];
        if (size) size[a] = m.bbox[2 * a + 1] - m.bbox[2 * a];   // BoundingBox.get_size, fp32 subtraction
    }
}

// The per-sample arrays of object k at level t: in the workspace, or - a retained object - in the caller's cache.
struct SampleArrays { float* t; float* sigma; int32_t* slot; float* dispmag; float* feat; };
static SampleArrays sample_arrays(const Plan& plan, char* ws, const RetainCtx* rc, int t, int k, bool has_bender) {
    SampleArrays a;
    if (rc && ((rc->mask >> k) & 1u)) {
        const RetainObjectPlan& o = rc->plan.obj[k];
        a.t = reinterpret_cast<float*>(rc->base + o.t[t]);
        a.sigma = reinterpret_cast<float*>(rc->base + o.sigma[t]);
        a.slot = reinterpret_cast<int32_t*>(rc->base + o.slot[t]);
        a.dispmag = has_bender ? reinterpret_cast<float*>(rc->base + o.dispmag[t]) : nullptr;
        a.feat = reinterpret_cast<float*>(rc->base + o.feat[t]);
        return a;
    }
    const TypePlan& tp = plan.type[t];
    a.t = reinterpret_cast<float*>(ws + tp.t[k]);
    a.sigma = reinterpret_cast<float*>(ws + tp.sigma[k]);
    a.slot = reinterpret_cast<int32_t*>(ws + tp.slot[k]);
    a.dispmag = has_bender ? reinterpret_cast<float*>(ws + tp.dispmag[k]) : nullptr;
    a.feat = reinterpret_cast<float*>(ws + tp.feat[k]);
    return a;
}

// ---------------------------------------------------------------------------------------------
// Fine guide (pr_fine_guide_t): the keep bits of the guided objects, one 256-byte aligned (N, R, words) region per object
// ---------------------------------------------------------------------------------------------
struct GuidePlan {
    size_t at[PR_MAX_OBJECTS];       // byte offset of object k's bits ((size_t)-1: not guided)
    int words[PR_MAX_OBJECTS];       // ceil((Pc_k + Pf_k) / 32)
    size_t bytes;
};
static int make_guide_plan(const pr_call_t& c, const pr_object_t* objs, uint32_t mask, GuidePlan* plan) {
    PR_REQUIRE((mask >> c.objects) == 0, "fine guide object_mask 0x%x names an object at or beyond objects = %d", mask, c.objects);
    PR_REQUIRE(mask == 0 || c.use_fine, "a fine guide needs a hierarchical call: use_fine is 0");
    size_t off = 0;
    for (int k = 0; k < PR_MAX_OBJECTS; ++k) {
        plan->at[k] = (size_t)-1;
        plan->words[k] = 0;
        if (k >= c.objects || !((mask >> k) & 1u)) continue;
        PR_REQUIRE(objs[k].fine.kind != 1 && objs[k].coarse.kind != 1, "fine guide: object %d is a skybox model (its density is a constant)", k);
        plan->words[k] = (objs[k].fine.positions + 31) / 32;
        plan->at[k] = off;
        off += align_up(sizeof(uint32_t) * (size_t)c.frames * c.rays * plan->words[k]);
    }
    plan->bytes = off;
    return PR_OK;
}

// Host checks of pr_render_forward_guided: no device work, so that a refusal precedes everything else.  A guide without objects is no guide.
static int validate_guide(const pr_call_t& c, const pr_object_t* objs, const pr_fine_guide_t* g, GuidePlan* plan) {
    PR_REQUIRE(!(c.flags & PR_FLAG_PERTURB), "the fine guide applies to unperturbed evaluation calls only: PR_FLAG_PERTURB is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_TRAIN_BN), "the fine guide applies to evaluation calls only: PR_FLAG_TRAIN_BN is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_SAVE_FOR_BACKWARD), "the fine guide applies to evaluation calls only: PR_FLAG_SAVE_FOR_BACKWARD is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_NAIVE_MLP), "the fine guide is not supported with PR_FLAG_NAIVE_MLP");
    bool noise = c.noise_coarse.integrate_global || c.noise_fine.integrate_global;
    for (int k = 0; k < PR_MAX_OBJECTS; ++k) noise = noise || c.noise_coarse.integrate[k] || c.noise_fine.integrate[k];
    PR_REQUIRE(!noise, "the fine guide applies to unperturbed evaluation calls only: an integrate-noise pointer is set");
    PR_TRY(make_guide_plan(c, objs, g->object_mask, plan));
    PR_REQUIRE(g->guard >= 0, "fine guide: guard %d is negative", g->guard);
    PR_REQUIRE(g->threshold == g->threshold, "fine guide: the threshold is NaN");
    PR_REQUIRE(g->scratch != nullptr && ((uintptr_t)g->scratch & 255) == 0, "fine guide scratch must be a 256-byte aligned device pointer");
    PR_REQUIRE(g->scratch_bytes >= plan->bytes, "fine guide scratch too small: %zu bytes given, %zu needed", g->scratch_bytes, plan->bytes);
    return PR_OK;
}

// ---------------------------------------------------------------------------------------------
// One renderer call: per level the stages sampling -> evaluation -> compositing -> exports ("Host stages")
// ---------------------------------------------------------------------------------------------
// What the stages of a call share.
struct CallState {
    const pr_call_t& c; const pr_object_t* objs; const pr_occupancy_t* occupancy; const RetainCtx* rc;
    const pr_fine_guide_t* guide; const GuidePlan* gplan; const pr_outputs_t* const* outs; const pr_geometry_t* const* geos;
    char* ws; const Plan& plan; hipStream_t s;
    bool geo;             // geometry-only call: density-only MLP launches (none for a skybox model), compositing ends behind the global weights
    bool naive, gate, defer, save;
    bool phased;          // training / differentiable call: three MLP phases around the two BatchNorm reductions
    bool grouped;         // evaluation call with several objects: one launch per stage for all of them
    bool train_grouped;   // differentiable call with several objects: the same for placement, the phases and the divergence
    int terms;            // fp16 terms per product of the split-precision tiers
    template <class T> T* at(size_t offset) const { return reinterpret_cast<T*>(ws + offset); }
};

// Object k at level t: everything the stages read of it, resolved once.
struct ObjectLevel {
    int k, P;
    size_t cap;                       // frames * rays * P: the rows of every per-sample array, the row bound of every launch
    const pr_object_model_t* m; const float* packed; ModelDims d; PackedLayout l;
    SampleArrays arr, coarse;         // (coarse: the arrays of the object's coarse level - fine level only)
    const int32_t* skip;              // retained object: its jobs return at once when the cached state is reused (NULL: never)
    uint32_t* keep; int keep_words;   // fine level of a guided object: the keep bits the resampler writes and the fill reads (NULL: not guided)
    OccGrid occ;                      // empty-space skipping: the same grid at the count and the fill site (bits == NULL without one)
    float* adain; const SavedPlan* sv;
    float* rec_pos; int32_t* rec_flat;                               // compact sample records
    int32_t* block_sums; int32_t* block_offsets; int32_t* total;
};

static int make_object_level(const CallState& cs, int t, int k, ObjectLevel* o) {
    const pr_object_t& obj = cs.objs[k];
    const TypePlan& tp = cs.plan.type[t];
    o->k = k;
    o->m = t ? &obj.fine : &obj.coarse;
    o->packed = static_cast<const float*>(t ? obj.packed_fine : obj.packed_coarse);
    PR_TRY(compute_dims(*o->m, &o->d));
    PR_TRY(compute_layout(*o->m, o->d, &o->l));
    o->P = o->m->positions; o->cap = (size_t)cs.c.frames * cs.c.rays * o->P;
    o->arr = sample_arrays(cs.plan, cs.ws, cs.rc, t, k, o->m->has_bender != 0);
    if (t) o->coarse = sample_arrays(cs.plan, cs.ws, cs.rc, 0, k, obj.coarse.has_bender != 0);
    o->skip = (cs.rc && ((cs.rc->mask >> k) & 1u)) ? &cs.rc->hdr->reuse[k] : nullptr;
    const bool guided = cs.guide && t == 1 && cs.gplan->at[k] != (size_t)-1;
    o->keep = guided ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(cs.guide->scratch) + cs.gplan->at[k]) : nullptr;
    o->keep_words = guided ? cs.gplan->words[k] : 0;
    PR_TRY(make_occ_grid(cs.occupancy ? (t ? &cs.occupancy->fine[k] : &cs.occupancy->coarse[k]) : nullptr, *o->m, k, t ? "fine" : "coarse", &o->occ));
    o->adain = cs.at<float>(tp.adain[k]);
    o->sv = &tp.saved[k];
    // a differentiable call keeps every object's records, grouped evaluation launches read them side by side; every other call
    // evaluates one object after the other on the shared pair
    o->rec_pos = cs.at<float>(cs.save ? o->sv->rec_pos : cs.grouped ? cs.plan.rec_pos_k[k] : cs.plan.rec_pos);
    o->rec_flat = cs.at<int32_t>(cs.save ? o->sv->rec_flat : cs.grouped ? cs.plan.rec_flat_k[k] : cs.plan.rec_flat);
    o->block_sums = cs.at<int32_t>(cs.plan.block_sums) + (size_t)k * cs.plan.nblocks256;
    o->block_offsets = cs.at<int32_t>(cs.plan.block_offsets) + (size_t)k * cs.plan.nblocks256;
    o->total = cs.at<int32_t>(tp.totals) + k;
    return PR_OK;
}

// A phased object (training / differentiable calls): its launch parameters, advanced from phase to phase, and where its BatchNorm state is.
struct TrainJob {
    MlpParams mp; FoldParams fo; const ObjectLevel* o;
    double* stats; int32_t* stat_count; float* batch; float* h1; float* h2;
};

// A level of the call: its objects and the host copies of what its grouped launches take.
struct Level {
    int t; const TypePlan* tp; const pr_noise_t* noise; const pr_outputs_t* out;
    int32_t* totals; int32_t* head_counts;
    ObjectLevel obj[PR_MAX_OBJECTS];
    PlaceParams place[PR_MAX_OBJECTS]; FillParams fill[PR_MAX_OBJECTS]; int32_t* total_ptrs[PR_MAX_OBJECTS];
    MlpParams jobs[PR_MAX_OBJECTS]; int job_rows[PR_MAX_OBJECTS]; FoldParams folds[PR_MAX_OBJECTS];
    int njobs;            // jobs of the level's grouped MLP launch, packed in object order (a geometry-only call leaves skybox models out)
    TrainJob train[PR_MAX_OBJECTS]; BnFoldJobs bn; DivChainJob div[PR_MAX_OBJECTS];
};
static thread_local Level g_level;

// ---- sampling: coarse placement or resampling, block scan, compaction ------------------------------------------------------
// The part PlaceParams, ResampleParams and FillParams share: rays, pose, box, occupancy grid, retention flag.
template <class Params> static Params sampling_params(const CallState& cs, const ObjectLevel& o) {
    Params p;
    memset(&p, 0, sizeof(p));
    p.frames = cs.c.frames; p.rays = cs.c.rays; p.objects = cs.c.objects; p.object_index = o.k;
    p.ray_origins = cs.c.ray_origins; p.ray_directions = cs.c.ray_directions; p.w2o = cs.c.w2o; p.in_scene = cs.c.object_in_scene;
    bbox_split(*o.m, p.lo, p.hi, nullptr);
    p.occ = o.occ; p.skip = o.skip;
    return p;
}

static PlaceParams place_params(const CallState& cs, const ObjectLevel& o) {
    PlaceParams pp = sampling_params<PlaceParams>(cs, o);
    pp.positions = o.P;
    pp.z_near_min = o.m->z_near_min; pp.z_far_max = o.m->z_far_max; pp.empty_alpha = o.m->empty_space_alpha;
    pp.linspace = cs.c.linspace_coarse[o.k];
    pp.jitter = perturb_noise(cs.c.noise_coarse.jitter[o.k], cs.c, NOISE_JITTER, 0, o.k);
    pp.t = o.arr.t; pp.sigma = o.arr.sigma; pp.dispmag = o.arr.dispmag; pp.block_sums = o.block_sums;
    return pp;
}

static ResampleParams resample_params(const CallState& cs, const ObjectLevel& o) {
    const pr_call_t& c = cs.c;
    ResampleParams rp = sampling_params<ResampleParams>(cs, o);
    rp.pc = cs.objs[o.k].coarse.positions; rp.pf = c.positions_fine[o.k];
    rp.empty_alpha = o.m->empty_space_alpha;
    rp.t_coarse = o.coarse.t; rp.sigma_coarse = o.coarse.sigma;
    rp.alpha_noise = perturb_noise(c.noise_coarse.alpha[o.k], c, NOISE_ALPHA, 0, o.k);
    rp.u_fixed = c.linspace_fine[o.k];
    rp.u_random = perturb_noise(c.noise_coarse.pdf[o.k], c, NOISE_PDF, 0, o.k);
    rp.t_fine = o.arr.t; rp.sigma_fine = o.arr.sigma; rp.dispmag_fine = o.arr.dispmag; rp.block_sums = o.block_sums;
    if (o.keep) {
        rp.keep = o.keep; rp.keep_words = o.keep_words; rp.guard = cs.guide->guard; rp.threshold = cs.guide->threshold;
    }
    return rp;
}

static FillParams fill_params(const CallState& cs, const ObjectLevel& o) {
    FillParams fp = sampling_params<FillParams>(cs, o);
    fp.positions = o.P;
    fp.t = o.arr.t; fp.block_offsets = o.block_offsets; fp.rec_pos = o.rec_pos; fp.rec_flat = o.rec_flat; fp.slot = o.arr.slot;
    fp.keep = o.keep; fp.keep_words = o.keep_words;
    return fp;
}

// One object: its three launches.
static int sample_object(const CallState& cs, const Level& L, const ObjectLevel& o) {
    if (L.t == 0) PR_TRY(launch_place_coarse(place_params(cs, o), cs.s));
    else PR_TRY(launch_resample(resample_params(cs, o), cs.s));
    PR_TRY(launch_scan(o.block_sums, o.block_offsets, o.total, cs.plan.nblocks256, cs.s));
    return launch_fill(fill_params(cs, o), cs.s);
}

// Coarse placement, block scan and compaction of every object of the call: three launches for all of them.
static int sample_level_grouped(const CallState& cs, Level& L) {
    for (int k = 0; k < cs.c.objects; ++k) {
        L.place[k] = place_params(cs, L.obj[k]);
        L.fill[k] = fill_params(cs, L.obj[k]);
        L.total_ptrs[k] = L.obj[k].total;
    }
    return launch_placement_group(L.place, L.fill, L.total_ptrs, cs.c.objects, cs.s);
}

// ---- evaluation: style affine + BatchNorm fold, the MLP --------------------------------------------------------------------
// The fused (phase 0) launch parameters of an object and the fold of its AdaIN table.
static int mlp_params(const CallState& cs, const Level& L, const ObjectLevel& o, MlpParams* mp_out, FoldParams* fo_out) {
    const pr_call_t& c = cs.c;
    const pr_object_model_t& m = *o.m;
    const ModelDims& d = o.d;
    const int K = c.objects, k = o.k;
    FoldParams& fo = *fo_out;
    memset(&fo, 0, sizeof(fo));
    fo.frames = c.frames; fo.objects = K; fo.object_index = k;
    fo.style = c.style; fo.S = m.style_features;
    fo.affine1 = m.affine1; fo.bn1_mean = m.bn1_mean; fo.bn1_var = m.bn1_var;
    fo.affine4 = m.affine4; fo.bn4_mean = m.bn4_mean; fo.bn4_var = m.bn4_var;
    fo.eps = m.bn_eps;
    fo.W = d.W; fo.Wpad = d.Wpad; fo.W2 = d.W2; fo.W2pad = d.W2pad;
    fo.table = o.adain; fo.row_floats = adain_row_floats(d);
    MlpParams& mp = *mp_out;
    memset(&mp, 0, sizeof(mp));
    // training calls with PR_FLAG_SPLIT_BACKWARD: phase 1 of the grouped launches reads the fp16-pair packings
    const bool split3 = cs.train_grouped && (c.flags & PR_FLAG_SPLIT_BACKWARD) && cs.save;
    PR_TRY(build_mlp_layers(m, d, o.l, o.packed, &mp, split3));
    mp.rec_pos = o.rec_pos; mp.rec_flat = o.rec_flat; mp.total = o.total;
    mp.samples_per_frame = c.rays * o.P; mp.positions = o.P; mp.rays = c.rays;
    mp.canonical = (c.flags & PR_FLAG_CANONICAL_POSE) ? 1 : 0;
    bbox_split(m, mp.lo, mp.hi, mp.size);
    mp.empty_alpha = m.empty_space_alpha;
    mp.in_scene = c.object_in_scene + k; mp.in_scene_stride = K;
    mp.ray_directions = c.ray_directions; mp.ray_origins = c.ray_origins;
    mp.w2o = c.w2o + (size_t)k * 12; mp.w2o_stride = K * 12;
    mp.deformation = c.deformation + (size_t)k * m.deformation_features; mp.deformation_stride = K * m.deformation_features;
    // (a geometry-only call folds no AdaIN table: it feeds the feature head only)
    mp.adain = cs.geo ? nullptr : o.adain; mp.adain_stride = fo.row_floats;
    mp.sigma = o.arr.sigma; mp.dispmag = o.arr.dispmag; mp.feat = cs.geo ? nullptr : o.arr.feat;
    if (cs.defer) {     // the kernels stop behind features_head.4 and write [h | 1] rows
        mp.n_layers = mp.n_backbone + 2;
        mp.F = hidden_row_floats(d.W2);
        mp.ones_col = d.W2;
    }
    if (cs.gate) {
        mp.gate = 1; mp.head_count = L.head_counts + k;
        mp.pend_act = cs.at<float>(cs.plan.pend_act);
        mp.pend_meta = cs.at<int32_t>(cs.plan.pend_meta);
    }
    mp.tile_counter = L.head_counts + PR_MAX_OBJECTS + k;
    if (L.out && L.out->sample_delta[k] && m.has_bender) mp.delta_dense = L.out->sample_delta[k];
    return PR_OK;
}

// The job of the level's grouped launch (rows: every launcher derives its own tile count).
static int add_job(Level& L, const ObjectLevel& o, const MlpParams& mp) {
    L.jobs[L.njobs] = mp;
    L.job_rows[L.njobs++] = (int)o.cap;
    return PR_OK;
}

// Geometry-only: a skybox model's constant density needs no MLP launch, the others run the density-only kernels.
static int evaluate_geometry_object(const CallState& cs, Level& L, const ObjectLevel& o, const MlpParams& mp) {
    if (o.m->kind == 1) {
        SkyboxSigmaParams sp;
        memset(&sp, 0, sizeof(sp));
        sp.samples = (long)o.cap; sp.samples_per_frame = cs.c.rays * o.P;
        sp.slot = o.arr.slot; sp.in_scene = cs.c.object_in_scene + o.k; sp.in_scene_stride = cs.c.objects;
        sp.empty_alpha = o.m->empty_space_alpha; sp.sigma = o.arr.sigma;
        return launch_skybox_sigma(sp, cs.s);
    }
    if (cs.grouped) return add_job(L, o, mp);
    if (cs.c.precision != PR_PRECISION_FP32) return launch_mlp_split_sigma(mp, (int)o.cap, cs.terms, cs.s);
    return launch_mlp_sigma(mp, (int)o.cap, cs.s);
}

// Evaluation: the fused kernels - gated, stopping in front of the deferred projection, split precision or the scalar one.
static int evaluate_fused_object(const CallState& cs, Level& L, const ObjectLevel& o, const MlpParams& mp, const FoldParams& fo) {
    if (cs.grouped) {       // folded and evaluated together once every object of the level is prepared
        L.folds[L.njobs] = fo;
        return add_job(L, o, mp);
    }
    if (cs.rc) PR_TRY(launch_retain_gate(*cs.rc, L.totals, o.k, 1, cs.s));
    PR_TRY(launch_adain_fold(fo, cs.s));
    if (cs.c.precision != PR_PRECISION_FP32 && !cs.naive) return launch_mlp_split(mp, (int)o.cap, cs.terms, cs.s);
    return launch_mlp(mp, (int)o.cap, cs.naive, o.m, cs.s);
}

// ---- the phased path -------------------------------------------------------------------------------------------------------
// BatchNorm in training mode: the batch statistics of the first (second) AdaIN layer are a reduction over every evaluated sample
// of this object call, between two matmuls.  Differentiable eval-mode calls (SAVE without TRAIN_BN) use the same phases - they
// leave the pre-BatchNorm activations h1 / h2 behind for the backward pass - with the running statistics frozen.
static void make_train_job(const CallState& cs, const ObjectLevel& o, const MlpParams& fused, const FoldParams& fo, TrainJob* J) {
    const SavedPlan& sv = *o.sv;
    const Plan& plan = cs.plan;
    J->mp = fused; J->fo = fo; J->o = &o;
    J->stats = cs.at<double>(sv.stats);               // (zeroed by the fill at the top of the level)
    J->stat_count = cs.at<int32_t>(sv.stat_count);
    J->batch = cs.at<float>(cs.save ? sv.batch : plan.batch_stats);
    J->h1 = cs.at<float>(cs.save ? sv.h1 : plan.h1); J->h2 = cs.at<float>(cs.save ? sv.h2 : plan.h2);
    MlpParams& mp = J->mp;
    mp.row_flags = cs.at<int32_t>(cs.save ? sv.row_flags : plan.row_flags);
    mp.stat_count = J->stat_count;
    if (cs.save) {
        mp.save_enc = cs.at<float>(sv.enc);
        mp.save_act = cs.at<float>(sv.act); mp.save_act_stride = o.cap * o.d.Wpad;
        mp.save_bits = cs.at<unsigned char>(sv.bits); mp.save_bits_stride = relu_bits_bytes(o.cap, o.d.Wpad);
        if (o.m->has_bender) {
            mp.save_bin = cs.at<float>(sv.bin);
            mp.save_bact = cs.at<float>(sv.bact); mp.save_bact_stride = o.cap * o.d.BWpad;
            mp.save_bbits = cs.at<unsigned char>(sv.bbits); mp.save_bbits_stride = relu_bits_bytes(o.cap, o.d.BWpad);
            mp.save_braw = cs.at<float>(sv.braw); mp.save_delta = cs.at<float>(sv.delta);
        }
    }
    mp.phase = 1; mp.h_out = J->h1; mp.h_out_width = o.d.Wpad; mp.stats = J->stats;
}

// BatchNorm stage s of a job (1: behind phase 1, 2: behind phase 2): where the sums are, the running statistics and the affine
// they belong to, where the batch values go and where the layer's scale and shift sit in a row of the AdaIN table.
struct BnStage {
    const double* stats; int width, width_pad;
    float* running_mean; float* running_var; long long* batches; const pr_linear_t* affine;
    float* batch_mean; float* batch_var;
    int g_off, b_off;
};
// ... and the job's launch parameters advanced to phase s + 1.
static BnStage next_bn_stage(TrainJob& J, int s) {
    const ModelDims& d = J.o->d;
    const pr_object_model_t& m = *J.o->m;
    float* batch = J.batch + (s - 1) * 2 * MAX_WIDTH;
    MlpParams& mp = J.mp;
    if (s == 1) {
        mp.phase = 2; mp.h_in = J.h1; mp.h_in_width = d.Wpad; mp.h_out = J.h2; mp.h_out_width = d.W2pad; mp.stats = J.stats + 2 * MAX_WIDTH;
        return BnStage{J.stats, d.W, d.Wpad, m.bn1_mean, m.bn1_var, (long long*)m.bn1_batches, &m.affine1, batch, batch + MAX_WIDTH, 0, d.Wpad};
    }
    mp.phase = 3; mp.h_in = J.h2; mp.h_in_width = d.W2pad; mp.h_out = nullptr;
    return BnStage{J.stats + 2 * MAX_WIDTH, d.W2, d.W2pad, m.bn4_mean, m.bn4_var, (long long*)m.bn4_batches, &m.affine4, batch,
                   batch + MAX_WIDTH, 2 * d.Wpad, 2 * d.Wpad + d.W2pad};
}

// The fields BnFinalizeParams and BnFoldJob share.
template <class Params> static void set_bn_stage(Params& p, const CallState& cs, const TrainJob& J, const BnStage& b) {
    memset(&p, 0, sizeof(p));
    p.stats = b.stats; p.count = J.stat_count; p.width = b.width; p.width_pad = b.width_pad; p.momentum = 0.1f;
    p.running_mean = b.running_mean; p.running_var = b.running_var; p.num_batches_tracked = b.batches;
    p.batch_mean = b.batch_mean; p.batch_var = b.batch_var;
    p.frozen = (cs.c.flags & PR_FLAG_TRAIN_BN) ? 0 : 1;
}

// The Hutchinson probes of an object's divergence estimate: explicit, or generated for training calls with a graph (the reference
// draws them whenever it trains with a graph, object_composer.py:597); neither: the divergence stays zero.
static bool divergence_probes(const CallState& cs, const Level& L, const TrainJob& J, NoiseRef* probes) {
    if (!(cs.save && J.o->m->has_bender)) return false;
    *probes = make_noise(L.noise->divergence[J.o->k], cs.c, NOISE_DIVERGENCE, L.t, J.o->k);
    if (!(cs.c.flags & PR_FLAG_TRAIN_BN)) probes->generate = 0;
    return probes->ptr || probes->generate;
}

// The fields DivergenceParams and DivChainJob share.
template <class Params> static void set_divergence(Params& q, const CallState& cs, const TrainJob& J, const NoiseRef& probes) {
    const ObjectLevel& o = *J.o;
    memset(&q, 0, sizeof(q));
    q.total = o.total; q.rec_flat = o.rec_flat; q.row_flags = J.mp.row_flags; q.rec_pos = o.rec_pos;
    q.noise = probes; q.positions = o.P;
    q.bin = J.mp.save_bin; q.bin_pad = o.d.bin_pad; q.benc = o.d.benc; q.b_octaves = o.m->bender_octaves;
    q.BW = o.d.BW; q.BWpad = o.d.BWpad; q.b_count = o.m->bender_count; q.b_skip = o.m->bender_skip;
    q.braw = J.mp.save_braw;
    bbox_split(*o.m, q.lo, q.hi, nullptr);
    q.canonical = (cs.c.flags & PR_FLAG_CANONICAL_POSE) ? 1 : 0;
    q.div = cs.at<float>(o.sv->div);      // (zeroed by the fill at the top of the level)
}

// What follows the last phase of one object: the normalised-sample count, and its divergence estimate one product per layer.
static int finish_train_object(const CallState& cs, const Level& L, const TrainJob& J) {
    if (L.out && L.out->normalised_samples)
        PR_CHECK_HIP(hipMemcpyAsync(L.out->normalised_samples + J.o->k, J.stat_count, sizeof(int32_t), hipMemcpyDeviceToDevice, cs.s));
    NoiseRef probes;
    if (!divergence_probes(cs, L, J, &probes)) return PR_OK;
    DivergenceParams dp;
    set_divergence(dp, cs, J, probes);
    dp.max_rows = (int)J.o->cap;
    dp.bacts = J.mp.save_bact; dp.bact_stride = J.mp.save_bact_stride; dp.bin_real = J.o->d.bin;
    dp.layers = J.o->m->bender; dp.out_head = J.o->m->bender_out;
    dp.t0 = cs.at<float>(cs.plan.div_t0); dp.ta = cs.at<float>(cs.plan.div_ta); dp.tb = cs.at<float>(cs.plan.div_tb);
    return launch_divergence(dp, cs.s);
}

// One object at a time: phase 1, statistics and fold, phase 2, statistics and fold, phase 3, divergence.
static int evaluate_phased_object(const CallState& cs, const Level& L, TrainJob& J) {
    const int rows = (int)J.o->cap;
    PR_TRY(launch_mlp(J.mp, rows, false, J.o->m, cs.s));
    for (int stage = 1; stage <= 2; ++stage) {
        const BnStage b = next_bn_stage(J, stage);
        BnFinalizeParams bf;
        set_bn_stage(bf, cs, J, b);
        PR_TRY(launch_bn_finalize(bf, cs.s));
        // (behind stage 1 the second layer is still folded with the running statistics as placeholders)
        if (stage == 1) { J.fo.bn1_mean = b.batch_mean; J.fo.bn1_var = b.batch_var; }
        else { J.fo.bn4_mean = b.batch_mean; J.fo.bn4_var = b.batch_var; }
        PR_TRY(launch_adain_fold(J.fo, cs.s));
        PR_TRY(launch_mlp(J.mp, rows, false, J.o->m, cs.s));
    }
    return finish_train_object(cs, L, J);
}

// Differentiable calls with several objects: every phase, the statistics with their fold and the divergence chains of the ray
// benders are one launch each for all objects.
static int evaluate_phased_group(const CallState& cs, Level& L) {
    const pr_call_t& c = cs.c;
    const int K = c.objects;
    PR_TRY(launch_mlp_group(L.jobs, L.job_rows, K, cs.s));                  // phase 1 of every object
    for (int stage = 1; stage <= 2; ++stage) {
        for (int k = 0; k < K; ++k) {
            TrainJob& J = L.train[k];
            const pr_object_model_t& m = *J.o->m;
            const BnStage st = next_bn_stage(J, stage);
            BnFoldJob& b = L.bn.job[k];
            set_bn_stage(b, cs, J, st);
            b.style = c.style + (size_t)k * m.style_features; b.style_stride = K * m.style_features; b.S = m.style_features;
            b.frames = c.frames; b.eps = m.bn_eps;
            b.table = J.o->adain; b.row_floats = J.mp.adain_stride;
            b.affine = *st.affine; b.g_off = st.g_off; b.b_off = st.b_off;
            if (stage == 2) b.normalised_out = (L.out && L.out->normalised_samples) ? L.out->normalised_samples + k : nullptr;
            J.mp.split3 = 0;     // (the head phases read fp32 fragments)
            L.jobs[k] = J.mp;
        }
        PR_TRY(launch_bn_fold_group(L.bn, K, cs.s));
        PR_TRY(launch_mlp_group(L.jobs, L.job_rows, K, cs.s));
    }
    long div_rows[PR_MAX_OBJECTS];
    int div_jobs = 0;
    for (int k = 0; k < K; ++k) {
        const TrainJob& J = L.train[k];
        const ObjectLevel& o = *J.o;
        NoiseRef probes;
        if (!divergence_probes(cs, L, J, &probes)) continue;
        if (!div_chain_supported(o.d.BWpad, o.d.bin_pad)) {
            PR_TRY(finish_train_object(cs, L, J));          // (unusually wide bender: one product per layer)
            continue;
        }
        DivChainJob& q = L.div[div_jobs];
        set_divergence(q, cs, J, probes);
        q.bbits = J.mp.save_bbits; q.bbits_stride = J.mp.save_bbits_stride;
        for (int j = 0; j < o.m->bender_count; ++j) q.seg0[j] = Seg{o.packed + o.l.b_seg_off[j][0], (j == 0 ? o.d.bin_pad : o.d.BWpad) / 8, 0};
        q.seg1 = Seg{o.packed + o.l.b_seg_off[o.m->bender_skip][1], o.d.bin_pad / 8, 0};
        q.w_out = o.packed + o.l.b_out_off;
        q.tile_counter = L.head_counts + 2 * PR_MAX_OBJECTS + k;
        div_rows[div_jobs++] = (long)o.cap;
    }
    return div_jobs ? launch_div_chain_group(L.div, div_rows, div_jobs, cs.s) : PR_OK;
}

// ---- evaluation of a level -------------------------------------------------------------------------------------------------
// Object k behind its sampling launches: its export fill, then its own MLP launches - or its job in the level's grouped ones.
static int evaluate_object(const CallState& cs, Level& L, int k) {
    const ObjectLevel& o = L.obj[k];
    MlpParams mp; FoldParams fo;
    PR_TRY(mlp_params(cs, L, o, &mp, &fo));
    if (L.out && L.out->sample_delta[k]) PR_TRY(launch_zero_fill(L.out->sample_delta[k], sizeof(float) * 3 * o.cap, cs.s));
    if (cs.geo) return evaluate_geometry_object(cs, L, o, mp);
    if (!cs.phased) return evaluate_fused_object(cs, L, o, mp, fo);
    TrainJob& J = L.train[k];
    make_train_job(cs, o, mp, fo, &J);
    if (!cs.train_grouped) return evaluate_phased_object(cs, L, J);
    return add_job(L, o, J.mp);
}

// The grouped launches of a level, once every object is prepared.
static int evaluate_grouped(const CallState& cs, Level& L) {
    if (cs.train_grouped) return evaluate_phased_group(cs, L);
    if (!cs.grouped || L.njobs == 0) return PR_OK;
    const bool split = cs.c.precision != PR_PRECISION_FP32;
    if (cs.geo)
        return split ? launch_mlp_split_sigma_group(L.jobs, L.job_rows, L.njobs, cs.terms, cs.s)
                     : launch_mlp_sigma_group(L.jobs, L.job_rows, L.njobs, cs.s);
    if (cs.rc) PR_TRY(launch_retain_gate(*cs.rc, L.totals, 0, L.njobs, cs.s));      // (behind the block scans of the level)
    PR_TRY(launch_adain_fold_group(L.folds, L.njobs, cs.s));
    return split ? launch_mlp_split_group(L.jobs, L.job_rows, L.njobs, cs.terms, cs.s) : launch_mlp_group(L.jobs, L.job_rows, L.njobs, cs.s);
}

// ---- compositing -----------------------------------------------------------------------------------------------------------
static int composite_level(const CallState& cs, const Level& L) {
    const pr_call_t& c = cs.c;
    const int K = c.objects, t = L.t;
    CompositeParams cp;
    memset(&cp, 0, sizeof(cp));
    cp.frames = c.frames; cp.rays = c.rays; cp.objects = K; cp.static_objects = c.static_objects;
    cp.F = cs.objs[0].coarse.output_features;
    cp.fix_overlaps = (c.flags & PR_FLAG_FIX_OVERLAPS) ? 1 : 0; cp.sigmoid = (c.flags & PR_FLAG_SIGMOID_FEATURES) ? 1 : 0;
    for (int k = 0; k < K; ++k) cp.total_positions += L.obj[k].P;
    cp.sort_size = 64;
    while (cp.sort_size < cp.total_positions) cp.sort_size <<= 1;
    cp.ray_directions = c.ray_directions;
    cp.noise_global = perturb_noise(L.noise->integrate_global, c, NOISE_INTEGRATE_GLOBAL, t, 0);
    for (int k = 0; k < K; ++k) {
        const ObjectLevel& ol = L.obj[k];
        if (cs.defer) {
            cp.proj_w[k] = ol.packed + ol.l.h6p_off;
            cp.proj_k = projection_k(ol.d.W2);
        }
        CompositeObject& o = cp.obj[k];
        o.t = ol.arr.t; o.sigma = ol.arr.sigma; o.slot = ol.arr.slot; o.dispmag = ol.arr.dispmag;
        o.divergence = (cs.save && ol.m->has_bender) ? cs.at<const float>(ol.sv->div) : nullptr;
        if (o.divergence) cp.any_divergence = 1;
        o.feat = cs.geo ? nullptr : ol.arr.feat;
        o.noise = perturb_noise(L.noise->integrate[k], c, NOISE_INTEGRATE, t, k);
        o.positions = ol.P;
        if (L.out) o.out = L.out->object[k];
    }
    if (L.out) { cp.global = L.out->global; cp.decoder = L.out->decoder; }
    if (cs.defer) {
        cp.out_features = cp.F;
        cp.F = hidden_row_floats(cs.objs[0].coarse.layers_width / 2);
        cp.pooled = cs.at<float>(cs.plan.pooled);
    }
    if (cs.geo) {
        cp.geometry = 1;
        cp.sigmoid = 0;
        if (cs.geos[t]) { cp.visibility = cs.geos[t]->visibility; cp.front_object = cs.geos[t]->front_object; }
    }
    PR_TRY(launch_composite(cp, cs.s));
    return cs.defer ? launch_projection(cp, cs.s) : PR_OK;
}

// ---- optional exports ------------------------------------------------------------------------------------------------------
static int export_level(const CallState& cs, const Level& L) {
    const pr_outputs_t* out = L.out;
    if (!out) return PR_OK;
    const int K = cs.c.objects;
    auto copy = [&](void* dst, const void* src, size_t count) -> int {      // (count 4-byte elements; dst == NULL: not asked for)
        if (dst) PR_CHECK_HIP(hipMemcpyAsync(dst, src, 4 * count, hipMemcpyDeviceToDevice, cs.s));
        return PR_OK;
    };
    for (int k = 0; k < K; ++k) {
        const ObjectLevel& o = L.obj[k];      // (wherever the arrays live)
        PR_TRY(copy(out->sample_t[k], o.arr.t, o.cap));
        PR_TRY(copy(out->sample_sigma[k], o.arr.sigma, o.cap));
        PR_TRY(copy(out->sample_slot[k], o.arr.slot, o.cap));
    }
    PR_TRY(copy(out->evaluated_samples, L.totals, K));
    if (out->head_samples && cs.geo)     // no sample goes through the feature head (a kernel fill: no memset node)
        return launch_zero_fill(out->head_samples, sizeof(int32_t) * K, cs.s);
    // without the gate every evaluated sample goes through the feature head
    return copy(out->head_samples, cs.gate ? L.head_counts : L.totals, K);
}

// What the stages would otherwise refuse with kernels of the call already on the stream: host checks, no device work.
static int validate_stages(const pr_call_t& c, const pr_object_t* objs) {
    // (with PR_FLAG_SAVE_FOR_BACKWARD validate_call has refused the scalar kernel already)
    PR_REQUIRE(!((c.flags & PR_FLAG_NAIVE_MLP) && (c.flags & PR_FLAG_TRAIN_BN)), "the scalar debugging kernel has no train-mode BatchNorm");
    for (int t = 0; t < (c.use_fine ? 2 : 1); ++t)
        for (int k = 0; k < c.objects; ++k) {
            const pr_object_model_t& m = t ? objs[k].fine : objs[k].coarse;
            PR_REQUIRE(m.output_features == objs[0].coarse.output_features, "all objects must share output_features");
            if (group_train_active(c))      // (the grouped statistics-and-fold launch reads them unconditionally)
                PR_REQUIRE(m.affine1.weight && m.affine1.bias && m.bn1_mean && m.bn1_var && m.affine4.weight && m.affine4.bias && m.bn4_mean &&
                               m.bn4_var, "AdaIN parameters missing");
        }
    return PR_OK;
}

// Per level: one fill, then per object sampling and evaluation - the launches of an object back to back, object after object,
// unless the call groups a stage, which then follows the loop as one launch for all objects -, compositing, exports.
static int render(const CallState& cs) {
    const pr_call_t& c = cs.c;
    const int K = c.objects;
    // retention: the first launches compare the cached keys with this call's inputs and set the reuse flags
    if (cs.rc) PR_TRY(launch_retain_probe(c, cs.objs, *cs.rc, cs.s));
    Level& L = g_level;
    for (int t = 0; t < (c.use_fine ? 2 : 1); ++t) {
        L.t = t; L.tp = &cs.plan.type[t]; L.noise = t ? &c.noise_fine : &c.noise_coarse; L.out = cs.outs[t]; L.njobs = 0;
        L.totals = cs.at<int32_t>(L.tp->totals); L.head_counts = cs.at<int32_t>(L.tp->head_counts);
        for (int k = 0; k < K; ++k) PR_TRY(make_object_level(cs, t, k, &L.obj[k]));
        // one fill: feature-head / tile counters, and - training / differentiable calls - every object's batch-statistics
        // accumulators and divergence array
        PR_TRY(launch_zero_fill(cs.ws + L.tp->zero_begin, L.tp->zero_bytes, cs.s));
        // (every object has its own sample records in the calls that group a stage: their coarse placement is grouped too)
        const bool placed = t == 0 && (cs.grouped || cs.train_grouped);
        if (placed) PR_TRY(sample_level_grouped(cs, L));
        for (int k = 0; k < K; ++k) {
            if (!placed) PR_TRY(sample_object(cs, L, L.obj[k]));
            PR_TRY(evaluate_object(cs, L, k));
        }
        PR_TRY(evaluate_grouped(cs, L));
        PR_TRY(composite_level(cs, L));
        PR_TRY(export_level(cs, L));
    }
    // retention: the last launches store the keys of the camera and of every retained object this call rendered
    if (cs.rc) PR_TRY(launch_retain_commit(c, cs.objs, *cs.rc, cs.s));
    return PR_OK;
}

// Host checks of a geometry-only call (PR_FLAG_GEOMETRY_ONLY): no device work, so that a refusal precedes everything else.
static int validate_geometry(const pr_call_t& c, const pr_retained_t* retained, const pr_outputs_t* coarse, const pr_outputs_t* fine) {
    PR_REQUIRE(!(c.flags & PR_FLAG_TRAIN_BN), "a geometry-only call runs no feature head: PR_FLAG_TRAIN_BN is set (batch statistics need the head)");
    PR_REQUIRE(!(c.flags & PR_FLAG_SAVE_FOR_BACKWARD), "a geometry-only call has no backward pass: PR_FLAG_SAVE_FOR_BACKWARD is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_NAIVE_MLP), "a geometry-only call is not supported with PR_FLAG_NAIVE_MLP");
    PR_REQUIRE(retained == nullptr, "a geometry-only call cannot be retained: pr_retained_t is not NULL (the cache layout holds feature rows)");
    const pr_outputs_t* levels[2] = {coarse, c.use_fine ? fine : nullptr};
    for (int t = 0; t < 2; ++t) {
        const pr_outputs_t* o = levels[t];
        if (!o) continue;
        const char* level = t ? "fine" : "coarse";
        for (int k = 0; k < PR_MAX_OBJECTS; ++k)
            PR_REQUIRE(o->object[k].integrated_features == nullptr,
                       "a geometry-only call writes no features: integrated_features of object %d (%s) is not NULL", k, level);
        PR_REQUIRE(o->global.integrated_features == nullptr,
                   "a geometry-only call writes no features: integrated_features of the global entry (%s) is not NULL", level);
        PR_REQUIRE(o->decoder.groups <= 0, "a geometry-only call writes no features: decoder.groups is %d (%s)", o->decoder.groups, level);
    }
    return PR_OK;
}

// Every render entry point ends here (geometry_* : the extras of pr_render_geometry, NULL elsewhere): every refusal, then the stages.
static int render_entry(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                        const pr_retained_t* retained, const pr_fine_guide_t* guide, const pr_outputs_t* coarse,
                        const pr_outputs_t* fine, const pr_geometry_t* geometry_coarse, const pr_geometry_t* geometry_fine,
                        void* workspace, size_t workspace_bytes, void* stream) {
    PR_REQUIRE(call && objects && workspace, "pr_render_forward: NULL argument");
    const pr_call_t& c = *call;
    PR_TRY(validate_occupancy(c, objects, occupancy));
    PR_TRY(validate_call(c, objects));
    if (c.flags & PR_FLAG_GEOMETRY_ONLY) PR_TRY(validate_geometry(c, retained, coarse, fine));
    if (guide && guide->object_mask == 0) guide = nullptr;
    GuidePlan gplan;
    if (guide) PR_TRY(validate_guide(c, objects, guide, &gplan));
    static thread_local RetainCtx ctx;
    if (retained) PR_TRY(validate_retained(c, objects, occupancy, guide, retained, coarse, fine, &ctx));
    PR_TRY(validate_stages(c, objects));
    Plan plan;
    PR_TRY(make_plan(c, objects, &plan));
    if (workspace_bytes < plan.bytes) {
        set_error("workspace too small: %zu bytes given, %zu needed", workspace_bytes, plan.bytes);
        return PR_ERR_WORKSPACE;
    }
    PR_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    const pr_outputs_t* outs[2] = {coarse, fine};
    const pr_geometry_t* geos[2] = {geometry_coarse, geometry_fine};
    const bool save = (c.flags & PR_FLAG_SAVE_FOR_BACKWARD) != 0;
    const CallState cs = {c, objects, occupancy, retained ? &ctx : nullptr, guide, &gplan, outs, geos, static_cast<char*>(workspace), plan,
                          (hipStream_t)stream, (c.flags & PR_FLAG_GEOMETRY_ONLY) != 0, (c.flags & PR_FLAG_NAIVE_MLP) != 0, gate_active(c),
                          defer_active(c, objects), save, save || (c.flags & PR_FLAG_TRAIN_BN), group_active(c), group_train_active(c),
                          c.precision == PR_PRECISION_F16 ? 1 : 3};
    return render(cs);
}

}  // namespace pr

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int pr_workspace_size(const pr_call_t* call, const pr_object_t* objects, size_t* bytes) {
    PR_REQUIRE(call && objects && bytes, "pr_workspace_size: NULL argument");
    PR_TRY(pr::validate_call(*call, objects));
    pr::Plan plan;
    PR_TRY(pr::make_plan(*call, objects, &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_render_forward(const pr_call_t* call, const pr_object_t* objects, const pr_outputs_t* coarse,
                                 const pr_outputs_t* fine, void* workspace, size_t workspace_bytes, void* stream) {
    return pr_render_forward_culled(call, objects, nullptr, coarse, fine, workspace, workspace_bytes, stream);
}

extern "C" int pr_render_forward_culled(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                                        const pr_outputs_t* coarse, const pr_outputs_t* fine, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    return pr_render_forward_retained(call, objects, occupancy, nullptr, coarse, fine, workspace, workspace_bytes, stream);
}

extern "C" int pr_render_forward_retained(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                                          const pr_retained_t* retained, const pr_outputs_t* coarse, const pr_outputs_t* fine,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    return pr_render_forward_guided(call, objects, occupancy, retained, nullptr, coarse, fine, workspace, workspace_bytes, stream);
}

extern "C" int pr_fine_guide_size(const pr_call_t* call, const pr_object_t* objects, uint32_t object_mask, size_t* bytes) {
    PR_REQUIRE(call && objects && bytes, "pr_fine_guide_size: NULL argument");
    PR_TRY(pr::validate_call(*call, objects));
    pr::GuidePlan plan;
    PR_TRY(pr::make_guide_plan(*call, objects, object_mask, &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_render_forward_guided(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                                        const pr_retained_t* retained, const pr_fine_guide_t* guide, const pr_outputs_t* coarse,
                                        const pr_outputs_t* fine, void* workspace, size_t workspace_bytes, void* stream) {
    return pr::render_entry(call, objects, occupancy, retained, guide, coarse, fine, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int pr_render_geometry(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                                  const pr_fine_guide_t* guide, const pr_outputs_t* coarse, const pr_outputs_t* fine,
                                  const pr_geometry_t* geometry_coarse, const pr_geometry_t* geometry_fine, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    PR_REQUIRE(call && objects && workspace, "pr_render_geometry: NULL argument");
    PR_REQUIRE(call->flags & PR_FLAG_GEOMETRY_ONLY, "pr_render_geometry needs PR_FLAG_GEOMETRY_ONLY in pr_call_t.flags");
    return pr::render_entry(call, objects, occupancy, nullptr, guide, coarse, fine, geometry_coarse, geometry_fine, workspace,
                            workspace_bytes, stream);
}

namespace pr {
__global__ __launch_bounds__(256) void k_noise_fill(NoiseRef n, int normal, long count, float* out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256)
        out[i] = normal ? noise_normal(n, i, 1, 0) : noise_uniform(n, i, 1, 0);
}
}  // namespace pr

extern "C" int pr_noise_fill(uint64_t seed, int32_t kind, int32_t type, int32_t object, int64_t count, float* out, void* stream) {
    PR_REQUIRE(kind >= 0 && kind <= 5 && (type == 0 || type == 1) && object >= 0 && object < PR_MAX_OBJECTS, "pr_noise_fill: bad stream");
    if (count <= 0) return PR_OK;
    PR_REQUIRE(out != nullptr, "pr_noise_fill: NULL output");
    pr_call_t c;
    memset(&c, 0, sizeof(c));
    c.flags = PR_FLAG_DEVICE_NOISE | PR_FLAG_PERTURB;
    c.noise_seed = seed;
    c.rays = 1;
    pr::NoiseRef n = pr::make_noise(nullptr, c, kind, type, object);
    n.rays = n.total_rays = 1;      // element i is "ray i, element 0 of 1": the flat tensor index
    const int normal = (kind == pr::NOISE_JITTER || kind == pr::NOISE_PDF) ? 0 : 1;
    const long blocks = (count + 255) / 256;
    hipLaunchKernelGGL(pr::k_noise_fill, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, (hipStream_t)stream, n, normal,
                       (long)count, out);
    PR_LAUNCH_CHECK();
    return PR_OK;
}

extern "C" int pr_profile_enable(int enable) {
    pr::g_profile_on.store(enable != 0, std::memory_order_relaxed);
    return PR_OK;
}

extern "C" int pr_profile_collect(double* milliseconds, int32_t* launches) {
    PR_REQUIRE(milliseconds && launches, "pr_profile_collect: NULL argument");
    std::lock_guard<std::mutex> lock(pr::g_profile_mutex);
    for (int c = 0; c < PR_PROFILE_CATEGORIES; ++c) {
        milliseconds[c] = 0.0;
        launches[c] = 0;
    }
    for (auto& r : pr::g_profile) {
        PR_CHECK_HIP(hipEventSynchronize(r.stop));
        float ms = 0.f;
        PR_CHECK_HIP(hipEventElapsedTime(&ms, r.start, r.stop));
        if (r.category >= 0 && r.category < PR_PROFILE_CATEGORIES) {
            milliseconds[r.category] += ms;
            launches[r.category] += 1;
        }
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    pr::g_profile.clear();
    return PR_OK;
}

// Node census of a recorded HIP graph (child graphs included): what EnvironmentModel.frame_replay asks before it trusts a
// recording that holds launches of modules this library does not own (see include/playrender.h).
namespace pr {
static int census_of(hipGraph_t graph, int32_t* counts, int depth) {
    size_t n = 0;
    PR_CHECK_HIP(hipGraphGetNodes(graph, nullptr, &n));
    if (n == 0) return PR_OK;
    std::vector<hipGraphNode_t> nodes(n);
    PR_CHECK_HIP(hipGraphGetNodes(graph, nodes.data(), &n));
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType type;
        PR_CHECK_HIP(hipGraphNodeGetType(nodes[i], &type));
        counts[0] += 1;
        if (type == hipGraphNodeTypeKernel) counts[1] += 1;
        else if (type == hipGraphNodeTypeMemset) counts[2] += 1;
        else if (type == hipGraphNodeTypeMemcpy) counts[3] += 1;
        else if (type == hipGraphNodeTypeGraph && depth < 8) {
            hipGraph_t child = nullptr;
            PR_CHECK_HIP(hipGraphChildGraphNodeGetGraph(nodes[i], &child));
            const int status = census_of(child, counts, depth + 1);
            if (status != PR_OK) return status;
        }
    }
    return PR_OK;
}
}  // namespace pr

extern "C" int pr_graph_node_census(void* graph, int32_t* counts) {
    PR_REQUIRE(graph && counts, "pr_graph_node_census: NULL pointer");
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    return pr::census_of((hipGraph_t)graph, counts, 0);
}

extern "C" int pr_abi_version(void) { return PR_ABI_VERSION; }

extern "C" const char* pr_last_error(void) { return pr::g_error; }

extern "C" int pr_device_info(int32_t* compute_units, int32_t* lds_bytes, char* arch_name, size_t arch_name_len) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        pr::set_error("no HIP device visible");
        return PR_ERR_NO_DEVICE;
    }
    int dev = 0;
    PR_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    PR_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int32_t)prop.maxSharedMemoryPerMultiProcessor;
    if (arch_name && arch_name_len) {
        strncpy(arch_name, prop.gcnArchName, arch_name_len - 1);
        arch_name[arch_name_len - 1] = 0;
    }
    return PR_OK;
}
