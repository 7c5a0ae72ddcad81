// Occupancy grids for empty-space skipping (pr_occupancy_build, include/playrender.h): a density lattice becomes one bit per
// cell, which the renderer's kept-sample predicate (sample_kept, pr_common.h) reads at its three cull sites.
#include "pr_common.h"

namespace pr {

// One thread per cell, cells in flat (x, y, z) order, 256 per workgroup.  A cell is occupied iff any lattice value of any cell
// within `dilate` cells of it (Chebyshev distance, clipped at the box) is > threshold: the (2d + 1)^3 dilation of "any of the
// cell's s^3 values is > threshold".  A wave's ballot is two finished words; cells past the end vote 0, so the tail bits are 0
// and every word is written exactly once (no zero fill, no atomics: an update may overwrite the bits in place).
__global__ __launch_bounds__(256) void k_occupancy_build(const float* __restrict__ sigma, int nx, int ny, int nz, int s, float threshold,
                                                         int dilate, int words, uint32_t* __restrict__ bits) {
    const int cells = nx * ny * nz;
    const int cell = blockIdx.x * 256 + threadIdx.x;
    const size_t sy = (size_t)nz * s, sx = sy * (size_t)ny * s;          // lattice strides (floats)
    const float* lattice = sigma + (size_t)blockIdx.y * sx * (size_t)nx * s;
    bool occupied = false;
    if (cell < cells) {
        const int cz = cell % nz, cy = (cell / nz) % ny, cx = cell / (nz * ny);
        const int x0 = max(cx - dilate, 0) * s, x1 = (min(cx + dilate, nx - 1) + 1) * s;
        const int y0 = max(cy - dilate, 0) * s, y1 = (min(cy + dilate, ny - 1) + 1) * s;
        const int z0 = max(cz - dilate, 0) * s, z1 = (min(cz + dilate, nz - 1) + 1) * s;
        for (int x = x0; x < x1 && !occupied; ++x)
            for (int y = y0; y < y1 && !occupied; ++y) {
                const float* row = lattice + x * sx + y * sy;
                for (int z = z0; z < z1; ++z) occupied = occupied || row[z] > threshold;
            }
    }
    const unsigned long long vote = __ballot(occupied);
    const int lane = threadIdx.x & 63;
    const int word = (cell - lane) >> 5;          // first word of this wave's 64 cells
    if (lane == 0 && word < words) bits[(size_t)blockIdx.y * words + word] = (uint32_t)vote;
    if (lane == 32 && word + 1 < words) bits[(size_t)blockIdx.y * words + word + 1] = (uint32_t)(vote >> 32);
}

static bool occ_present(const pr_occupancy_t* occ, int objects, int use_fine) {
    if (!occ) return false;
    for (int k = 0; k < objects && k < PR_MAX_OBJECTS; ++k)
        if (occ->coarse[k].bits || (use_fine && occ->fine[k].bits)) return true;
    return false;
}

// Host checks of pr_render_forward_culled: no device work, so that a refusal precedes everything else.
int validate_occupancy(const pr_call_t& c, const pr_object_t* objs, const pr_occupancy_t* occ) {
    if (!occ_present(occ, c.objects, c.use_fine)) return PR_OK;
    PR_REQUIRE(!(c.flags & PR_FLAG_PERTURB), "occupancy grids cull unperturbed evaluation calls only: PR_FLAG_PERTURB is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_TRAIN_BN), "occupancy grids cull evaluation calls only: PR_FLAG_TRAIN_BN is set (batch statistics need every row)");
    PR_REQUIRE(!(c.flags & PR_FLAG_SAVE_FOR_BACKWARD), "occupancy grids cull evaluation calls only: PR_FLAG_SAVE_FOR_BACKWARD is set");
    PR_REQUIRE(!(c.flags & PR_FLAG_NAIVE_MLP), "occupancy grids are not supported with PR_FLAG_NAIVE_MLP");
    bool noise = c.noise_coarse.integrate_global || c.noise_fine.integrate_global;
    for (int k = 0; k < PR_MAX_OBJECTS; ++k) noise = noise || c.noise_coarse.integrate[k] || c.noise_fine.integrate[k];
    PR_REQUIRE(!noise, "occupancy grids cull unperturbed evaluation calls only: an integrate-noise pointer is set");
    PR_REQUIRE(c.objects >= 1 && c.objects <= PR_MAX_OBJECTS, "objects %d out of range 1..%d", c.objects, PR_MAX_OBJECTS);
    for (int k = 0; k < c.objects; ++k)
        for (int t = 0; t < (c.use_fine ? 2 : 1); ++t) {
            OccGrid g;
            PR_TRY(make_occ_grid(t ? &occ->fine[k] : &occ->coarse[k], t ? objs[k].fine : objs[k].coarse, k, t ? "fine" : "coarse", &g));
        }
    return PR_OK;
}

int make_occ_grid(const pr_occupancy_grid_t* g, const pr_object_model_t& m, int object, const char* level, OccGrid* out) {
    memset(out, 0, sizeof(*out));
    if (!g || !g->bits) return PR_OK;
    PR_REQUIRE(m.kind != 1, "object %d (%s): skybox models are never culled (occupancy bits must be NULL)", object, level);
    long cells = 1;
    for (int a = 0; a < 3; ++a) {
        PR_REQUIRE(g->cells[a] >= 1 && g->cells[a] <= 4096, "object %d (%s): occupancy cells[%d] = %d out of range 1..4096", object, level, a,
                   g->cells[a]);
        cells *= g->cells[a];
        const float lo = m.bbox[2 * a], hi = m.bbox[2 * a + 1];
        PR_REQUIRE(hi > lo, "object %d (%s): the bounding box has an empty axis %d ([%g, %g]): it cannot carry an occupancy grid", object,
                   level, a, (double)lo, (double)hi);
        out->n[a] = g->cells[a];
        out->scale[a] = (float)g->cells[a] / (hi - lo);
    }
    PR_REQUIRE(cells < (1L << 30), "object %d (%s): too many occupancy cells", object, level);
    PR_REQUIRE((long)g->words * 32 >= cells, "object %d (%s): occupancy words %d hold fewer than %ld cells", object, level, g->words, cells);
    out->bits = g->bits;
    out->words = g->words;
    return PR_OK;
}

}  // namespace pr

extern "C" int pr_occupancy_build(const float* sigma, int32_t groups, const int32_t* cells, int32_t supersample, float threshold,
                                  int32_t dilate, uint32_t* bits, void* stream) {
    PR_REQUIRE(cells != nullptr, "pr_occupancy_build: NULL cells");
    PR_REQUIRE(groups >= 1 && groups <= 65535, "pr_occupancy_build: groups %d out of range 1..65535", groups);
    PR_REQUIRE(supersample >= 1 && dilate >= 0, "pr_occupancy_build: supersample %d (>= 1) / dilate %d (>= 0)", supersample, dilate);
    long total = 1, lattice = 1;
    for (int a = 0; a < 3; ++a) {
        PR_REQUIRE(cells[a] >= 1 && cells[a] <= 4096, "pr_occupancy_build: cells[%d] = %d out of range 1..4096", a, cells[a]);
        total *= cells[a];
        lattice *= (long)cells[a] * supersample;
    }
    PR_REQUIRE(total < (1L << 30) && lattice < (1L << 30), "pr_occupancy_build: grid too large (%ld cells, %ld lattice points)", total, lattice);
    PR_REQUIRE(sigma && bits, "pr_occupancy_build: NULL pointer");
    const int words = (int)((total + 31) / 32);
    const unsigned blocks = (unsigned)(((long)words * 32 + 255) / 256);
    hipLaunchKernelGGL(pr::k_occupancy_build, dim3(blocks, (unsigned)groups), dim3(256), 0, (hipStream_t)stream, sigma, cells[0], cells[1],
                       cells[2], supersample, threshold, dilate, words, bits);
    PR_LAUNCH_CHECK();
    return PR_OK;
}
