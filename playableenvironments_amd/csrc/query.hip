// Point queries of one object model's fields (pr_query_field): density, style-modulated feature and ray-bender displacement at
// explicit object-frame positions - RayBendingStyleNerfModel.forward in evaluation mode
// (model/nerf_models/ray_bending_style_nerf_model.py:137-219).
//
// The evaluation itself is the renderer's fused MLP kernel (mlp.hip / mlp_split.hip), which consumes compact sample records.  A
// query is a different FRONT END - k_query_count / k_query_fill build the records from the given positions instead of from rays
// (closed-interval box test, boolean compaction in flat order) - and a different BACK END - k_query_scatter takes the compact
// feature rows to the dense per-point layout instead of compositing them.  The query is driven as frames = G, rays = M,
// positions = 1, so a record's flat index is the flat point index and its frame is its group.
#include "pr_common.h"

namespace pr {

struct QueryGeom {
    long total;                    // G * M
    const float* positions;        // (G*M, 3)
    float lo[3], hi[3];
    float empty_alpha;
    float inside_sigma;            // density of the in-box points (skybox density-only queries, which evaluate nothing)
    int32_t* block_sums;           // per 256-point block: points inside the box
    const int32_t* block_offsets;  // their exclusive scan
    float* rec_pos;                // (cap, 3)
    int32_t* rec_flat;             // (cap)
    int32_t* slot;                 // (G*M) workspace copy (read by k_query_scatter)
    int32_t* slot_out;             // (G*M) caller's copy or NULL
    float* sigma;                  // (G*M)
    float* displacement;           // (G*M, 3) or NULL
    int32_t* counters;             // caller's [rows through the backbone, rows through the feature head] or NULL
    int backbone_rows, head_rows;  // 1: the in-box points go through the backbone / the feature head
    // constants of the MLP launch, written by block 0 of k_query_count
    float* identity;               // 12 floats: the top three rows of an identity w2o (skybox input of the tile loop)
    uint32_t* present;             // one word of ones: the all-present in_scene entry every group reads
    int32_t* tile_counter;         // zeroed: the evaluation launch claims its tiles from it
};

// position of point g (one lane per point: the 12-byte rows of a wave are 768 contiguous bytes) and its box decision
__device__ __forceinline__ bool query_point(const QueryGeom& q, long g, float* x, float* y, float* z) {
    if (g >= q.total) return false;
    const PR_GLOBAL_AS float* p = as_global(q.positions) + (size_t)g * 3;
    *x = p[0];
    *y = p[1];
    *z = p[2];
    return in_box(*x, *y, *z, q.lo, q.hi);   // closed interval (ray_bending_style_nerf_model.py:62-85)
}

__global__ __launch_bounds__(256) void k_query_count(QueryGeom q) {
    __shared__ int lds[4];
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    float x, y, z;
    const int inside = __popcll(__ballot(query_point(q, g, &x, &y, &z)));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = inside;
    __syncthreads();
    if (threadIdx.x == 0) as_global(q.block_sums)[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
    if (blockIdx.x == 0) {
        if (threadIdx.x < 12) as_global(q.identity)[threadIdx.x] = (threadIdx.x % 5 == 0) ? 1.0f : 0.0f;
        if (threadIdx.x == 12) as_global(q.present)[0] = 0x01010101u;
        if (threadIdx.x == 13) as_global(q.tile_counter)[0] = 0;
    }
}

// Compact records in flat point order (the order of the reference's boolean-mask indexing), the slot array, and the
// not-evaluated values of EVERY point: the MLP kernel overwrites the rows it evaluates.
__global__ __launch_bounds__(256) void k_query_fill(QueryGeom q) {
    __shared__ int lds[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    float x = 0.f, y = 0.f, z = 0.f;
    const bool inside = query_point(q, g, &x, &y, &z);
    const unsigned long long ballot = __ballot(inside);
    if (lane == 0) lds[wave] = __popcll(ballot);
    __syncthreads();
    int base = as_global(q.block_offsets)[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += lds[w];
    const int mine = base + __popcll(ballot & ((1ull << lane) - 1ull));
    if (g < q.total) {
        if (inside) {
            PR_GLOBAL_AS float* rp = as_global(q.rec_pos) + (size_t)mine * 3;
            rp[0] = x;
            rp[1] = y;
            rp[2] = z;
            as_global(q.rec_flat)[mine] = (int32_t)g;
        }
        const int slot = inside ? mine : -1;
        as_global(q.slot)[g] = slot;
        if (q.slot_out) as_global(q.slot_out)[g] = slot;
        as_global(q.sigma)[g] = inside ? q.inside_sigma : q.empty_alpha;
        if (q.displacement) {
            PR_GLOBAL_AS float* dp = as_global(q.displacement) + (size_t)g * 3;
            dp[0] = 0.f;
            dp[1] = 0.f;
            dp[2] = 0.f;
        }
    }
    if (q.counters && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        // the last block's offset + its own count = every point inside the box
        const int total = as_global(q.block_offsets)[blockIdx.x] + lds[0] + lds[1] + lds[2] + lds[3];
        as_global(q.counters)[0] = q.backbone_rows ? total : 0;
        as_global(q.counters)[1] = q.head_rows ? total : 0;
    }
}

// Compact feature rows (cap, F) -> dense (G*M, F), zero rows where slot < 0.  The only query kernel whose traffic matters
// (2 x 4F bytes per point): consecutive lanes move consecutive 16-byte pieces of a row (F / 4 pieces per row, a wave spans
// 64 / (F / 4) rows), both sides streamed past the caches' retention (each byte is touched once).
struct QueryScatter {
    long total;              // G * M
    int F;
    const int32_t* slot;
    const float* feat;
    float* out;
};

__global__ __launch_bounds__(256) void k_query_scatter(QueryScatter q) {
    const int f4 = q.F >> 2;
    const long pieces = q.total * f4;
    const PR_GLOBAL_AS int32_t* slot = as_global(q.slot);
    const PR_GLOBAL_AS f32x4_t* feat = reinterpret_cast<const PR_GLOBAL_AS f32x4_t*>(as_global(q.feat));
    PR_GLOBAL_AS f32x4_t* out = reinterpret_cast<PR_GLOBAL_AS f32x4_t*>(as_global(q.out));
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < pieces; idx += (long)gridDim.x * 256) {
        const long row = idx / f4;
        const int c = (int)(idx - row * f4);
        const int s = slot[row];
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        if (s >= 0) v = __builtin_nontemporal_load(feat + (size_t)s * f4 + c);
        __builtin_nontemporal_store(v, out + idx);
    }
}

// feature widths that are no multiple of 4 (or rows that are not 16-byte aligned): one float per lane
__global__ __launch_bounds__(256) void k_query_scatter_scalar(QueryScatter q) {
    const long elements = q.total * q.F;
    const PR_GLOBAL_AS int32_t* slot = as_global(q.slot);
    const PR_GLOBAL_AS float* feat = as_global(q.feat);
    PR_GLOBAL_AS float* out = as_global(q.out);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < elements; idx += (long)gridDim.x * 256) {
        const long row = idx / q.F;
        const int c = (int)(idx - row * q.F);
        const int s = slot[row];
        out[idx] = s >= 0 ? feat[(size_t)s * q.F + c] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
static size_t query_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct QueryPlan {
    size_t consts, block_sums, block_offsets, rec_pos, rec_flat, slot, adain, feat, bytes;
    int nblocks;
    bool evaluate;     // some kernel of the MLP runs (everything but a skybox density-only query)
};

static int validate_query(const pr_query_t& q, const pr_object_model_t& m) {
    PR_REQUIRE(q.groups > 0, "query: groups %d must be positive", q.groups);
    PR_REQUIRE(q.points > 0, "query: points %d must be positive", q.points);
    PR_REQUIRE((long)q.groups * q.points < (1L << 31), "query: too many points in one call (%d groups x %d points >= 2^31)", q.groups,
               q.points);
    PR_REQUIRE((q.flags & ~(uint32_t)PR_FLAG_CANONICAL_POSE) == 0, "query: unsupported flags 0x%x (PR_FLAG_CANONICAL_POSE or 0)", q.flags);
    PR_REQUIRE(q.precision == PR_PRECISION_FP32 || q.precision == PR_PRECISION_F16X3 || q.precision == PR_PRECISION_F16,
               "unknown precision %d", q.precision);
    PR_REQUIRE(q.positions != nullptr, "query: positions missing");
    PR_REQUIRE(q.style != nullptr, "query: style missing");
    PR_REQUIRE(q.deformation != nullptr || !m.has_bender, "query: deformation missing");
    PR_REQUIRE(q.sigma != nullptr, "query: sigma output missing");
    PR_REQUIRE(m.kind == 0 || m.kind == 1, "query: unknown model kind %d", m.kind);
    if (m.kind == 1) {
        PR_REQUIRE(q.ray_origins != nullptr, "query: a skybox model needs ray_origins");
        PR_REQUIRE(q.ray_directions != nullptr, "query: a skybox model needs ray_directions");
    }
    return PR_OK;
}

static int make_query_plan(const pr_query_t& q, const pr_object_model_t& m, QueryPlan* plan) {
    ModelDims d;
    PR_TRY(compute_dims(m, &d));
    const size_t cap = (size_t)q.groups * q.points;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += query_align(bytes);
        return at;
    };
    memset(plan, 0, sizeof(*plan));
    plan->nblocks = (int)((cap + 255) / 256);
    plan->evaluate = q.features != nullptr || m.kind == 0;
    plan->consts = take(256);                                  // identity w2o rows | in_scene word | tile counter | total
    plan->block_sums = take(sizeof(int32_t) * plan->nblocks);
    plan->block_offsets = take(sizeof(int32_t) * plan->nblocks);
    plan->rec_pos = take(sizeof(float) * 3 * cap);
    plan->rec_flat = take(sizeof(int32_t) * cap);
    plan->slot = take(sizeof(int32_t) * cap);
    if (q.features) {
        plan->adain = take(sizeof(float) * (size_t)q.groups * adain_row_floats(d));
        plan->feat = take(sizeof(float) * cap * m.output_features);
    }
    plan->bytes = off;
    return PR_OK;
}

static int query(const pr_query_t& q, const pr_object_model_t& m, const float* packed, char* ws, const QueryPlan& plan,
                 hipStream_t s) {
    ModelDims d;
    PackedLayout l;
    PR_TRY(compute_dims(m, &d));
    PR_TRY(compute_layout(m, d, &l));
    const long total = (long)q.groups * q.points;
    float* identity = reinterpret_cast<float*>(ws + plan.consts);
    uint32_t* present = reinterpret_cast<uint32_t*>(ws + plan.consts + 64);
    int32_t* tile_counter = reinterpret_cast<int32_t*>(ws + plan.consts + 128);
    int32_t* rows = reinterpret_cast<int32_t*>(ws + plan.consts + 192);
    int32_t* block_sums = reinterpret_cast<int32_t*>(ws + plan.block_sums);
    int32_t* block_offsets = reinterpret_cast<int32_t*>(ws + plan.block_offsets);
    int32_t* slot = reinterpret_cast<int32_t*>(ws + plan.slot);
    float* feat = q.features ? reinterpret_cast<float*>(ws + plan.feat) : nullptr;

    QueryGeom g;
    memset(&g, 0, sizeof(g));
    g.total = total;
    g.positions = q.positions;
    bbox_split(m, g.lo, g.hi, nullptr);
    g.empty_alpha = m.empty_space_alpha;
    g.inside_sigma = plan.evaluate ? m.empty_space_alpha : 10.0f;   // (overwritten by the MLP kernel where it evaluates)
    g.block_sums = block_sums; g.block_offsets = block_offsets;
    g.rec_pos = reinterpret_cast<float*>(ws + plan.rec_pos);
    g.rec_flat = reinterpret_cast<int32_t*>(ws + plan.rec_flat);
    g.slot = slot; g.slot_out = q.slot;
    g.sigma = q.sigma; g.displacement = q.displacement;
    g.counters = q.counters;
    g.backbone_rows = plan.evaluate ? 1 : 0;
    g.head_rows = q.features ? 1 : 0;
    g.identity = identity; g.present = present; g.tile_counter = tile_counter;
    {
        ProfileScope scope(5, s);
        hipLaunchKernelGGL(k_query_count, dim3(plan.nblocks), dim3(256), 0, s, g);
        PR_LAUNCH_CHECK();
        PR_TRY(launch_scan(block_sums, block_offsets, rows, plan.nblocks, s));
        hipLaunchKernelGGL(k_query_fill, dim3(plan.nblocks), dim3(256), 0, s, g);
        PR_LAUNCH_CHECK();
    }
    if (!plan.evaluate) return PR_OK;

    MlpParams mp;
    memset(&mp, 0, sizeof(mp));
    PR_TRY(build_mlp_layers(m, d, l, packed, &mp));
    mp.rec_pos = g.rec_pos; mp.rec_flat = g.rec_flat; mp.total = rows;
    mp.samples_per_frame = q.points; mp.positions = 1; mp.rays = q.points;
    mp.canonical = (q.flags & PR_FLAG_CANONICAL_POSE) ? 1 : 0;
    bbox_split(m, mp.lo, mp.hi, mp.size);
    mp.empty_alpha = m.empty_space_alpha;
    mp.in_scene = reinterpret_cast<const uint8_t*>(present); mp.in_scene_stride = 0;      // every group: present
    mp.ray_directions = q.ray_directions; mp.ray_origins = q.ray_origins;
    mp.w2o = identity; mp.w2o_stride = 0;                                                   // positions are object-frame already
    mp.deformation = q.deformation; mp.deformation_stride = m.deformation_features;
    mp.adain = q.features ? reinterpret_cast<const float*>(ws + plan.adain) : nullptr;
    mp.adain_stride = adain_row_floats(d);
    mp.sigma = q.sigma; mp.feat = feat;
    mp.delta_dense = (m.has_bender && q.displacement) ? q.displacement : nullptr;
    // gate = 0: the renderer's sigma-gated head skips rows with density <= 0 because compositing never reads them; the model
    // returns features for every in-box point
    mp.tile_counter = tile_counter;
    const int terms = q.precision == PR_PRECISION_F16 ? 1 : 3;
    if (q.features) {
        FoldParams fo;
        memset(&fo, 0, sizeof(fo));
        fo.frames = q.groups; fo.objects = 1; fo.object_index = 0;
        fo.style = q.style; fo.S = m.style_features;
        fo.affine1 = m.affine1; fo.bn1_mean = m.bn1_mean; fo.bn1_var = m.bn1_var;
        fo.affine4 = m.affine4; fo.bn4_mean = m.bn4_mean; fo.bn4_var = m.bn4_var;
        fo.eps = m.bn_eps;
        fo.W = d.W; fo.Wpad = d.Wpad; fo.W2 = d.W2; fo.W2pad = d.W2pad;
        fo.table = reinterpret_cast<float*>(ws + plan.adain); fo.row_floats = adain_row_floats(d);
        PR_TRY(launch_adain_fold(fo, s));
        if (q.precision != PR_PRECISION_FP32) PR_TRY(launch_mlp_split(mp, (int)total, terms, s));
        else PR_TRY(launch_mlp(mp, (int)total, false, &m, s));
        QueryScatter sc;
        sc.total = total; sc.F = m.output_features; sc.slot = slot; sc.feat = feat; sc.out = q.features;
        const bool vec = (sc.F & 3) == 0 && ((uintptr_t)q.features & 15) == 0;
        const long work = vec ? total * (sc.F >> 2) : total * sc.F;
        long blocks = (work + 255) / 256;
        if (blocks > 16384) blocks = 16384;
        ProfileScope scope(5, s);
        if (vec) hipLaunchKernelGGL(k_query_scatter, dim3((unsigned)blocks), dim3(256), 0, s, sc);
        else hipLaunchKernelGGL(k_query_scatter_scalar, dim3((unsigned)blocks), dim3(256), 0, s, sc);
        PR_LAUNCH_CHECK();
    } else {
        if (q.precision != PR_PRECISION_FP32) PR_TRY(launch_mlp_split_sigma(mp, (int)total, terms, s));
        else PR_TRY(launch_mlp_sigma(mp, (int)total, s));
    }
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_query_workspace_size(const pr_query_t* q, const pr_object_model_t* model, size_t* bytes) {
    PR_REQUIRE(q && model && bytes, "pr_query_workspace_size: NULL argument");
    PR_TRY(pr::validate_query(*q, *model));
    pr::QueryPlan plan;
    PR_TRY(pr::make_query_plan(*q, *model, &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_query_field(const pr_query_t* q, const pr_object_model_t* model, const void* packed, void* workspace,
                              size_t workspace_bytes, void* stream) {
    PR_REQUIRE(q && model, "pr_query_field: NULL argument");
    PR_TRY(pr::validate_query(*q, *model));
    pr::QueryPlan plan;
    PR_TRY(pr::make_query_plan(*q, *model, &plan));
    if (workspace_bytes < plan.bytes) {
        pr::set_error("workspace too small: %zu bytes given, %zu needed", workspace_bytes, plan.bytes);
        return PR_ERR_WORKSPACE;
    }
    PR_REQUIRE(workspace != nullptr, "pr_query_field: workspace missing");
    PR_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    PR_REQUIRE(packed != nullptr || !plan.evaluate, "pr_query_field: packed weights missing");
    return pr::query(*q, *model, static_cast<const float*>(packed), static_cast<char*>(workspace), plan, (hipStream_t)stream);
}
