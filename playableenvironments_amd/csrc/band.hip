// Density lattices evaluated only in a band around the level set (pr_band_plan / pr_band_fill, include/playrender.h): the front end
// and the back end around an unchanged field evaluation.  The caller evaluates the field at the SKELETON (every stride-th point per
// axis and the last one); pr_band_plan finds the skeleton cells the level set passes through (MIXED), grows them by `guard` cells
// (ACTIVE) and lists every other point of an active cell - the BAND - in a fixed order; the caller evaluates the field there;
// pr_band_fill scatters those values and copies a skeleton value to everything else.
//
// pr_band_plan: k_band_mixed (a lane per cell: the 8 corner flags), k_band_active (a lane per cell: the guard neighbourhood, the block
// sums of both cell counts), k_band_count (a lane per lattice point: the block sums of the band flags), the block scan
// (k_scan_blocks_group), k_band_offsets (a block per group: offsets and counts) and - unless the call only counts - k_band_emit (a
// lane per point: index and position rows).  pr_band_fill: k_band_fill (a lane per point).  256-lane blocks that never span two groups.
// A point's class is recomputed from the active bytes where it is needed (at most 8 byte reads): no per-point array is kept.
#include "mesh_dev.h"

namespace pr {

struct BandParams {
    int groups, nx, ny, nz;
    int points, blocks;           // P = nx ny nz; point blocks per group, ceil(P / 256)
    int stride, guard;
    int cx, cy, cz;
    int cells, cell_blocks;       // C = cx cy cz; cell blocks per group, ceil(C / 256)
    float level;
    int max_points;
    float* sigma;                 // (G, P)
    const float* ax; const float* ay; const float* az;
    const float* values;          // (max_points), fill call
    int32_t* point_offsets; int32_t* counts;
    uint8_t* active_out; int32_t* point_index; float* positions; uint8_t* exact;
    // workspace
    uint8_t* mixed;               // (G, C)
    uint8_t* active;              // (G, C)
    int32_t* msum; int32_t* asum; // (G cell_blocks) block sums of the mixed / active cells
    int32_t* psum; int32_t* poff; // (G blocks) block sums of the band points, their exclusive scan
    int32_t* total;               // [band points of all groups]
};

// One axis of a lattice point: is its index a skeleton index, and which cells [lo, hi] contain it (two on an inner skeleton index).
struct BandAxis {
    int lo, hi;
    bool skeleton;
};

__device__ __forceinline__ BandAxis band_axis(int i, int n, int r, int cells) {
    BandAxis a;
    const int q = i / r;
    const bool multiple = q * r == i;
    a.skeleton = multiple || i == n - 1;
    a.lo = (multiple && i > 0) ? q - 1 : q;        // (i == n - 1, no multiple: q is the short last cell)
    a.hi = min(q, cells - 1);
    return a;
}

enum { BAND_SKELETON = 0, BAND_BAND = 1, BAND_FILLED = 2, BAND_NONE = 3 };

struct BandLane {
    int group, p;
    int kind;                     // BAND_*; BAND_NONE: the lane has no point
    int source;                   // flat index of the lower corner of the lowest-indexed cell that contains the point
    int i, j, k;
};

// The lane of a point kernel and the class of its point.
__device__ __forceinline__ BandLane band_lane(const BandParams& s) {
    BandLane l;
    l.group = (int)blockIdx.x / s.blocks;
    l.p = ((int)blockIdx.x - l.group * s.blocks) * 256 + (int)threadIdx.x;
    l.kind = BAND_NONE;
    l.source = l.i = l.j = l.k = 0;
    if (l.p >= s.points) return l;
    l.k = l.p % s.nz;
    l.j = (l.p / s.nz) % s.ny;
    l.i = l.p / (s.nz * s.ny);
    const BandAxis x = band_axis(l.i, s.nx, s.stride, s.cx), y = band_axis(l.j, s.ny, s.stride, s.cy), z = band_axis(l.k, s.nz, s.stride, s.cz);
    l.source = ((x.lo * s.stride) * s.ny + y.lo * s.stride) * s.nz + z.lo * s.stride;
    if (x.skeleton && y.skeleton && z.skeleton) {
        l.kind = BAND_SKELETON;
        return l;
    }
    const PR_GLOBAL_AS uint8_t* active = as_global(s.active) + (size_t)l.group * s.cells;
    int any = 0;
    for (int a = x.lo; a <= x.hi; ++a)
        for (int b = y.lo; b <= y.hi; ++b)
            for (int c = z.lo; c <= z.hi; ++c) any |= active[(a * s.cy + b) * s.cz + c];
    l.kind = any ? BAND_BAND : BAND_FILLED;
    return l;
}

struct BandCell {
    int group, cell, a, b, c;
    bool live;
};

__device__ __forceinline__ BandCell band_cell(const BandParams& s) {
    BandCell l;
    l.group = (int)blockIdx.x / s.cell_blocks;
    l.cell = ((int)blockIdx.x - l.group * s.cell_blocks) * 256 + (int)threadIdx.x;
    l.live = l.cell < s.cells;
    const int q = l.live ? l.cell : 0;
    l.c = q % s.cz;
    l.b = (q / s.cz) % s.cy;
    l.a = q / (s.cz * s.cy);
    return l;
}

__global__ __launch_bounds__(256) void k_band_mixed(BandParams s) {
    const BandCell l = band_cell(s);
    if (!l.live) return;
    const PR_GLOBAL_AS float* sig = as_global(s.sigma) + (size_t)l.group * s.points;
    const int x[2] = {l.a * s.stride, min((l.a + 1) * s.stride, s.nx - 1)};
    const int y[2] = {l.b * s.stride, min((l.b + 1) * s.stride, s.ny - 1)};
    const int z[2] = {l.c * s.stride, min((l.c + 1) * s.stride, s.nz - 1)};
    int inside = 0;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner)
        inside += sig[(x[corner >> 2] * s.ny + y[corner >> 1 & 1]) * s.nz + z[corner & 1]] > s.level ? 1 : 0;
    as_global(s.mixed)[(size_t)l.group * s.cells + l.cell] = (inside > 0 && inside < 8) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_band_active(BandParams s) {
    __shared__ int lds[4];
    const BandCell l = band_cell(s);
    int mixed = 0, active = 0;
    if (l.live) {
        const PR_GLOBAL_AS uint8_t* m = as_global(s.mixed) + (size_t)l.group * s.cells;
        mixed = m[l.cell];
        const int a0 = max(l.a - s.guard, 0), a1 = min(l.a + s.guard, s.cx - 1);
        const int b0 = max(l.b - s.guard, 0), b1 = min(l.b + s.guard, s.cy - 1);
        const int c0 = max(l.c - s.guard, 0), c1 = min(l.c + s.guard, s.cz - 1);
        for (int a = a0; a <= a1 && !active; ++a)
            for (int b = b0; b <= b1 && !active; ++b)
                for (int c = c0; c <= c1; ++c) active |= m[(a * s.cy + b) * s.cz + c];
        const size_t at = (size_t)l.group * s.cells + l.cell;
        as_global(s.active)[at] = (uint8_t)active;
        if (s.active_out) as_global(s.active_out)[at] = (uint8_t)active;
    }
    int mixed_total, active_total;
    block_exclusive_scan_256(mixed, lds, &mixed_total);
    block_exclusive_scan_256(active, lds, &active_total);
    if (threadIdx.x == 0) {
        as_global(s.msum)[blockIdx.x] = mixed_total;
        as_global(s.asum)[blockIdx.x] = active_total;
    }
}

__global__ __launch_bounds__(256) void k_band_count(BandParams s) {
    __shared__ int lds[4];
    const BandLane l = band_lane(s);
    int total;
    block_exclusive_scan_256(l.kind == BAND_BAND ? 1 : 0, lds, &total);
    if (threadIdx.x == 0) as_global(s.psum)[blockIdx.x] = total;
}

// One block per group: the group's offset and counts.  (The last group also writes the total.)
__global__ __launch_bounds__(256) void k_band_offsets(BandParams s) {
    __shared__ int lds[4];
    const int g = (int)blockIdx.x;
    int mixed = 0, active = 0;
    for (int b = (int)threadIdx.x; b < s.cell_blocks; b += 256) {
        mixed += as_global(s.msum)[(size_t)g * s.cell_blocks + b];
        active += as_global(s.asum)[(size_t)g * s.cell_blocks + b];
    }
    int mixed_total, active_total;
    block_exclusive_scan_256(mixed, lds, &mixed_total);
    block_exclusive_scan_256(active, lds, &active_total);
    if (threadIdx.x != 0) return;
    const int total = as_global(s.total)[0];
    const int first = as_global(s.poff)[(size_t)g * s.blocks];
    const int next = g + 1 < s.groups ? as_global(s.poff)[(size_t)(g + 1) * s.blocks] : total;
    as_global(s.point_offsets)[g] = first;
    if (g + 1 == s.groups) as_global(s.point_offsets)[s.groups] = total;
    PR_GLOBAL_AS int32_t* counts = as_global(s.counts) + (size_t)g * 4;
    counts[0] = s.cells;
    counts[1] = mixed_total;
    counts[2] = active_total;
    counts[3] = next - first;
}

__global__ __launch_bounds__(256) void k_band_emit(BandParams s) {
    __shared__ int lds[4];
    const BandLane l = band_lane(s);
    const bool band = l.kind == BAND_BAND;
    int total;
    const int row = as_global(s.poff)[blockIdx.x] + block_exclusive_scan_256(band ? 1 : 0, lds, &total);
    if (!band || row >= s.max_points) return;
    if (s.point_index) as_global(s.point_index)[row] = l.p;
    if (s.positions) {
        PR_GLOBAL_AS float* o = as_global(s.positions) + (size_t)row * 3;
        o[0] = as_global(s.ax)[l.i];
        o[1] = as_global(s.ay)[l.j];
        o[2] = as_global(s.az)[l.k];
    }
}

// Values move as 32-bit words: a copy keeps every bit of a NaN.
__global__ __launch_bounds__(256) void k_band_fill(BandParams s) {
    __shared__ int lds[4];
    const BandLane l = band_lane(s);
    const bool band = l.kind == BAND_BAND;
    int total;
    const int row = as_global(s.poff)[blockIdx.x] + block_exclusive_scan_256(band ? 1 : 0, lds, &total);
    if (l.kind == BAND_NONE) return;
    const size_t at = (size_t)l.group * s.points + l.p;
    PR_GLOBAL_AS uint32_t* lattice = (PR_GLOBAL_AS uint32_t*)as_global(s.sigma);
    const bool listed = band && row < s.max_points;
    if (listed) lattice[at] = ((const PR_GLOBAL_AS uint32_t*)as_global(s.values))[row];
    else if (l.kind != BAND_SKELETON) lattice[at] = lattice[(size_t)l.group * s.points + l.source];       // (a skeleton entry: never written by anyone)
    if (s.exact) as_global(s.exact)[at] = (l.kind == BAND_SKELETON || listed) ? 1 : 0;
}

struct BandPlan {
    size_t mixed, active, msum, asum, psum, poff, total, bytes;
    int points, blocks, cells[3], cell_count, cell_blocks;
};

// Host checks of the three entry points: no device work.
static int plan_band(const pr_band_t* s, const char* who, BandPlan* plan) {
    PR_REQUIRE(s != nullptr, "%s: NULL description", who);
    PR_REQUIRE(s->groups >= 1, "%s: groups %d (>= 1)", who, s->groups);
    double lattice = (double)s->groups;
    for (int a = 0; a < 3; ++a) {
        PR_REQUIRE(s->points[a] >= 2, "%s: points[%d] = %d (a lattice has at least 2 points per axis)", who, a, s->points[a]);
        lattice *= (double)s->points[a];
    }
    PR_REQUIRE(lattice < 2147483648.0, "%s: lattice too large: groups x points must stay below 2^31 (the indices are int32)", who);
    PR_REQUIRE(s->stride >= PR_BAND_MIN_STRIDE && s->stride <= PR_BAND_MAX_STRIDE, "%s: stride %d (must be in [%d, %d])", who, s->stride,
               PR_BAND_MIN_STRIDE, PR_BAND_MAX_STRIDE);
    PR_REQUIRE(s->guard >= 0 && s->guard <= PR_BAND_MAX_GUARD, "%s: guard %d (must be in [0, %d])", who, s->guard, PR_BAND_MAX_GUARD);
    PR_REQUIRE(s->level == s->level, "%s: level is NaN", who);
    PR_REQUIRE(s->flags == 0, "%s: flags 0x%x (must be 0)", who, s->flags);
    PR_REQUIRE(s->sigma != nullptr, "%s: NULL sigma", who);
    PR_REQUIRE(s->axis[0] && s->axis[1] && s->axis[2], "%s: NULL axis", who);
    PR_REQUIRE(s->point_offsets != nullptr, "%s: NULL point_offsets (always written)", who);
    PR_REQUIRE(s->counts != nullptr, "%s: NULL counts (always written)", who);
    PR_REQUIRE(s->max_points >= 0, "%s: negative capacity (max_points %d)", who, s->max_points);
    long points = 1, cells = 1;
    for (int a = 0; a < 3; ++a) {
        plan->cells[a] = (s->points[a] - 2) / s->stride + 1;          // ceil((n - 1) / stride)
        points *= s->points[a];
        cells *= plan->cells[a];
    }
    plan->points = (int)points;
    plan->blocks = (int)((points + 255) / 256);
    plan->cell_count = (int)cells;
    plan->cell_blocks = (int)((cells + 255) / 256);
    const size_t G = (size_t)s->groups;
    size_t at = 0;
    plan->mixed = workspace_region(&at, G * (size_t)cells);
    plan->active = workspace_region(&at, G * (size_t)cells);
    plan->msum = workspace_region(&at, G * plan->cell_blocks * sizeof(int32_t));
    plan->asum = workspace_region(&at, G * plan->cell_blocks * sizeof(int32_t));
    plan->psum = workspace_region(&at, G * plan->blocks * sizeof(int32_t));
    plan->poff = workspace_region(&at, G * plan->blocks * sizeof(int32_t));
    plan->total = workspace_region(&at, sizeof(int32_t));
    plan->bytes = at;
    return PR_OK;
}

static int band_params(const pr_band_t* s, const char* who, void* workspace, size_t workspace_bytes, BandPlan* plan, BandParams* p) {
    PR_TRY(plan_band(s, who, plan));
    PR_REQUIRE(workspace != nullptr, "%s: NULL workspace", who);
    PR_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    if (workspace_bytes < plan->bytes) {
        set_error("%s: workspace too small: %zu bytes given, %zu needed", who, workspace_bytes, plan->bytes);
        return PR_ERR_INVALID;
    }
    char* ws = (char*)workspace;
    memset(p, 0, sizeof(*p));
    p->groups = s->groups;
    p->nx = s->points[0];
    p->ny = s->points[1];
    p->nz = s->points[2];
    p->points = plan->points;
    p->blocks = plan->blocks;
    p->stride = s->stride;
    p->guard = s->guard;
    p->cx = plan->cells[0];
    p->cy = plan->cells[1];
    p->cz = plan->cells[2];
    p->cells = plan->cell_count;
    p->cell_blocks = plan->cell_blocks;
    p->level = s->level;
    p->max_points = s->max_points;
    p->sigma = s->sigma;
    p->ax = s->axis[0];
    p->ay = s->axis[1];
    p->az = s->axis[2];
    p->values = s->values;
    p->point_offsets = s->point_offsets;
    p->counts = s->counts;
    p->active_out = s->active;
    p->point_index = s->point_index;
    p->positions = s->positions;
    p->exact = s->exact;
    p->mixed = (uint8_t*)(ws + plan->mixed);
    p->active = (uint8_t*)(ws + plan->active);
    p->msum = (int32_t*)(ws + plan->msum);
    p->asum = (int32_t*)(ws + plan->asum);
    p->psum = (int32_t*)(ws + plan->psum);
    p->poff = (int32_t*)(ws + plan->poff);
    p->total = (int32_t*)(ws + plan->total);
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_band_workspace_size(const pr_band_t* s, size_t* bytes) {
    PR_REQUIRE(bytes != nullptr, "pr_band_workspace_size: NULL bytes");
    pr::BandPlan plan;
    PR_TRY(pr::plan_band(s, "pr_band_workspace_size", &plan));
    *bytes = plan.bytes;
    return PR_OK;
}

extern "C" int pr_band_plan(const pr_band_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    BandPlan plan;
    BandParams p;
    PR_TRY(band_params(s, "pr_band_plan", workspace, workspace_bytes, &plan, &p));
    hipStream_t st = (hipStream_t)stream;
    const unsigned cell_grid = (unsigned)((long)s->groups * plan.cell_blocks), grid = (unsigned)((long)s->groups * plan.blocks);
    hipLaunchKernelGGL(k_band_mixed, dim3(cell_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_band_active, dim3(cell_grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_band_count, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    const int32_t* sums[1] = {p.psum};
    int32_t* offsets[1] = {p.poff};
    int32_t* totals[1] = {p.total};
    PR_TRY(launch_scan_group(sums, offsets, totals, 1, (int)grid, st));
    hipLaunchKernelGGL(k_band_offsets, dim3((unsigned)s->groups), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    if (!s->point_index && !s->positions) return PR_OK;          // nothing to list (the active bytes are written above)
    hipLaunchKernelGGL(k_band_emit, dim3(grid), dim3(256), 0, st, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}

extern "C" int pr_band_fill(const pr_band_t* s, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace pr;
    BandPlan plan;
    BandParams p;
    PR_TRY(band_params(s, "pr_band_fill", workspace, workspace_bytes, &plan, &p));
    PR_REQUIRE(s->values != nullptr || s->max_points == 0, "pr_band_fill: NULL values with max_points %d", s->max_points);
    hipLaunchKernelGGL(k_band_fill, dim3((unsigned)((long)s->groups * plan.blocks)), dim3(256), 0, (hipStream_t)stream, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
