// Alpha compositing: per-object integration and the cross-object merge (ObjectComposer.integrate,
// compose, fix_object_overlap; model/object_composer.py:153-214, :295-447, :724-784).
//
// One workgroup per ray (one wave for short lists, four for long ones).  All K per-object sample lists of the ray are
// staged in LDS; the merged list is ordered by (t, concatenation index) - a rank merge of the already sorted lists, a
// bitonic network as the fallback - i.e. the merge is STABLE in object order, which is how ties are defined for this
// renderer (the reference calls torch.sort without stable=True; ties only occur between samples that carry zero alpha,
// see DESIGN.md).  The per-sample 192-channel features are never materialised per ray: they are read exactly once
// from the compact MLP output rows of the in-box samples and accumulated against both the per-object and the global
// weights.  The exclusive cumulative product of the transmittances is a wave-level multiplicative scan (the
// reference's cumprod is sequential; the association differs at the ulp level only).
#include "pr_common.h"
#include "composite_dev.h"

namespace pr {

struct CompositeSmem {
    float* tt;      // t per concatenated entry (after the overlap fix)
    float* sg;      // raw sigma per entry (after the overlap fix)
    float* dm;      // |displacement| per entry (after the overlap fix)
    float* wo;      // per-object weight per entry
    float* wg;      // global weight per entry (indexed by concatenation index)
    float* al;      // alpha scratch
    float* dv;      // |divergence estimate| per entry (after the overlap fix)
    int* sl;        // compact feature row per entry (-1: outside the box)
    unsigned int* key;   // entry index per merged rank
};
// The feature pass reuses key / tt / al for its compacted lists (row, own weight, global weight): the ranks, the depths and the
// sorted-order weights are dead behind the barrier that ends the global pass (wg and the outputs have been written from them).  A list
// occupies entries of its own (object, part) only, so lists never overlap; what the compaction reads - sl, wo, wg (the storage of sg) -
// are three other arrays, never written in that pass.  Hence neither the shared pass nor pooled_row_sums needs a barrier between a
// wave's compaction and its reads.

constexpr int MAX_FCHUNK = 4;  // F <= 256 channels, 64 lanes

// weights[j] = alpha[j] * prod_{i<j} (1 - alpha[i] + 1e-10)  over al[0..n), in place.
// Blocks of 64 consecutive entries are scanned across the wave (log steps), the running product is
// carried from block to block.  (The reference's cumprod is sequential; the association differs at
// the ulp level only.)
__device__ __forceinline__ void transmittance_weights(float* al, int n, int lane) {
    float carry = 1.0f;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const float a = (j < n) ? al[j] : 0.f;
        float incl = (j < n) ? __fadd_rn(__fsub_rn(1.0f, a), 1e-10f) : 1.0f;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float o = __shfl_up(incl, d, 64);
            if (lane >= d) incl *= o;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        if (j < n) al[j] = a * (carry * excl);
        carry *= __shfl(incl, 63, 64);
    }
}

constexpr int ROWS_IN_FLIGHT = 8;       // feature rows a wave loads before it accumulates them (the compositing pass below)

// weights[j] = alpha[j] * prod_{i<j} (...) over al[0..n) by CW waves: wave w scans the contiguous segment
// [w * seg, (w + 1) * seg) (seg a multiple of 64) from a unit carry, the segment products are exchanged through
// `totals` and folded in afterwards.
__device__ __forceinline__ float sigmoid_of(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int CW>
__device__ __forceinline__ void transmittance_weights_block(float* al, int n, float* totals, int wave, int lane) {
    if (CW == 1) {
        transmittance_weights(al, n, lane);
        return;
    }
    const int seg = (((n + CW - 1) / CW) + 63) & ~63;
    const int begin = wave * seg;
    const int end = (begin + seg < n) ? begin + seg : n;
    float carry = 1.0f;
    for (int base = begin; base < end; base += 64) {
        const int j = base + lane;
        const float a = (j < end) ? al[j] : 0.f;
        float incl = (j < end) ? __fadd_rn(__fsub_rn(1.0f, a), 1e-10f) : 1.0f;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float o = __shfl_up(incl, d, 64);
            if (lane >= d) incl *= o;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        if (j < end) al[j] = a * (carry * excl);
        carry *= __shfl(incl, 63, 64);
    }
    if (lane == 0) totals[wave] = carry;
    __syncthreads();
    float before = 1.0f;
    for (int w = 0; w < wave; ++w) before *= totals[w];
    if (wave > 0)
        for (int j = begin + lane; j < end; j += 64) al[j] *= before;
    __syncthreads();
}

// sum over the workgroup of a per-thread value, in a fixed order (waves 0 .. CW - 1); every thread receives it
template <int CW>
__device__ __forceinline__ float block_sum(float v, float* scratch, int wave, int lane) {
    v = wave_sum(v);
    if (CW == 1) return v;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    float total = 0.f;
    for (int w = 0; w < CW; ++w) total += scratch[w];
    return total;
}

// The per-wave channel sums `acc` (lane l owns the channels l + 64 c) added in wave order and stored by wave 0 as the F floats at dst.
template <int CW>
__device__ __forceinline__ void store_channel_sums(float (&acc)[MAX_FCHUNK], float* dst, int F, float* scratch, int wave, int lane) {
    if (CW > 1) {
#pragma unroll
        for (int c = 0; c < MAX_FCHUNK; ++c) {      // one 64-channel chunk at a time: 1 KB of scratch
            if (64 * c >= F) break;
            __syncthreads();
            scratch[wave * 64 + lane] = acc[c];
            __syncthreads();
            if (wave == 0)
                for (int w = 1; w < CW; ++w) acc[c] = __fadd_rn(acc[c], scratch[w * 64 + lane]);
        }
    }
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < MAX_FCHUNK; ++c) {
            const int ch = lane + 64 * c;
            if (ch < F) dst[ch] = acc[c];
        }
    }
}

constexpr int POOLED_ROWS_IN_FLIGHT = 8;   // as above, for the per-object pass of the deferred calls (four channels per lane and row)

// Feature pass of the deferred calls (p.pooled, CW > 1): every sum of such a call belongs to ONE object - its rows under its own
// weights go to pooled[2 k], under the global weights to pooled[2 k + 1] - so object k is the business of wave k % CW alone: no
// cross-wave sum, no scratch, no barrier.  The wave walks the object's parts j = 0, 1, ... - [j part, (j + 1) part), the ranges the
// waves 0, 1, ... own in the shared pass of k_composite - compacts each part and sums it from a fresh pair of accumulators in list
// order, then folds the parts in part order: tot = part 0, tot = tot + part 1, ...  That is the shared pass's wave-order sum, bit for
// bit.  A part that does not exist (j part >= P: the waves beyond the list in the shared pass) is skipped; exact, because an
// accumulator that starts at +0 and only ever adds never becomes -0 (+0 + -0 = +0 under round-to-nearest), so the `+ 0.0f` the shared
// pass spends on such a wave changes no bit.
// A row is F floats, F a multiple of 4 (launch_projection requires it), rows and pooled blocks are 16-byte aligned (the workspace
// plan aligns every array to 256 bytes): lane l < F / 4 reads the channels 4 l .. 4 l + 3 of a row as one 16-byte load.  Every
// channel keeps its own chain acc = acc + w * v over the list.
// LDS: the part lists go to key / tt / al at [off + j part, off + j part + count), inside the entries of this (object, part), so the
// lists of different waves never overlap; sl / wo / wg (= sg), which the compaction reads, are other arrays.  See CompositeSmem.
template <int CW>
__device__ __forceinline__ void pooled_row_sums(const CompositeParams& p, const CompositeSmem& sm, const long g, const int wave, const int lane) {
    // the four channels of a lane as one vector (two packed operations each): a product is rounded, then the sum - never fused
#pragma clang fp contract(off)
    const int F = p.F;
    const bool owner = 4 * lane < F;       // this lane holds four channels
    const int col4 = owner ? lane : 0;     // (the other lanes read lane 0's channels again - no divergent load - and store nothing)
    const bool want_global = p.global.integrated_features || p.decoder.groups > 0;
    int* lrow = reinterpret_cast<int*>(sm.key);
    float* lw1 = sm.tt;
    float* lw2 = sm.al;
    int off = 0;
#pragma unroll 1
    for (int k = 0; k < p.objects; off += p.obj[k].positions, ++k) {
        if (k % CW != wave) continue;
        const CompositeObject& o = p.obj[k];
        const int P = o.positions;
        const int part = (((P + CW - 1) / CW) + 63) & ~63;
        f32x4_t toto = {0.f, 0.f, 0.f, 0.f}, totg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int begin = 0; begin < P; begin += part) {
            const int end = (begin + part < P) ? begin + part : P;
            int count = 0;
#pragma unroll 1
            for (int base = begin; base < end; base += 64) {
                const int i = base + lane;
                bool take = false;
                int row = -1;
                float w1 = 0.f, w2 = 0.f;
                if (i < end) {
                    row = sm.sl[off + i];
                    w1 = sm.wo[off + i];
                    w2 = sm.wg[off + i];
                    take = row >= 0 && (w1 != 0.f || w2 != 0.f);
                }
                const unsigned long long m = __ballot(take);
                if (take) {
                    const int pos = off + begin + count + __popcll(m & ((1ull << lane) - 1ull));
                    lrow[pos] = row;
                    lw1[pos] = w1;
                    lw2[pos] = w2;
                }
                count += __popcll(m);
            }
            // (the list is written and read by this wave only: no barrier needed in between)
            const int* rows_w = lrow + off + begin;
            const float* w1_w = lw1 + off + begin;
            const float* w2_w = lw2 + off + begin;
            f32x4_t acco = {0.f, 0.f, 0.f, 0.f}, accg = {0.f, 0.f, 0.f, 0.f};
            int i = 0;
#pragma unroll 1
            for (; i + POOLED_ROWS_IN_FLIGHT <= count; i += POOLED_ROWS_IN_FLIGHT) {
                // lane u < POOLED_ROWS_IN_FLIGHT fetches list entry i + u; the entries are handed round as scalars, so a row address is a
                // scalar base plus this lane's 16 bytes and the weights need no vector register per row
                const int u0 = lane < POOLED_ROWS_IN_FLIGHT ? lane : 0;
                const int row_l = rows_w[i + u0];
                const int w1_l = __float_as_int(w1_w[i + u0]), w2_l = __float_as_int(w2_w[i + u0]);
                f32x4_t v[POOLED_ROWS_IN_FLIGHT];
#pragma unroll
                for (int u = 0; u < POOLED_ROWS_IN_FLIGHT; ++u) {
                    const float* row = o.feat + (size_t)__builtin_amdgcn_readlane(row_l, u) * F;
                    v[u] = as_global(reinterpret_cast<const f32x4_t*>(row))[col4];
                }
#pragma unroll
                for (int u = 0; u < POOLED_ROWS_IN_FLIGHT; ++u) {
                    const float w1 = __int_as_float(__builtin_amdgcn_readlane(w1_l, u)), w2 = __int_as_float(__builtin_amdgcn_readlane(w2_l, u));
                    acco = acco + v[u] * w1;
                    accg = accg + v[u] * w2;
                }
            }
#pragma unroll 1
            for (; i < count; ++i) {
                const float* row = o.feat + (size_t)__builtin_amdgcn_readfirstlane(rows_w[i]) * F;
                const f32x4_t v = as_global(reinterpret_cast<const f32x4_t*>(row))[col4];
                const float w1 = w1_w[i], w2 = w2_w[i];
                acco = acco + v * w1;
                accg = accg + v * w2;
            }
            if (begin == 0) {
                toto = acco;
                totg = accg;
            } else {
                toto = toto + acco;
                totg = totg + accg;
            }
        }
        if (owner) {
            float* own = p.pooled + ((size_t)(2 * k) * gridDim.x + g) * F + 4 * lane;
            if (o.out.integrated_features) *as_global(reinterpret_cast<f32x4_t*>(own)) = toto;
            if (want_global) *as_global(reinterpret_cast<f32x4_t*>(own + (size_t)gridDim.x * F)) = totg;
        }
    }
}

// CW waves per ray.  Lists of a few hundred entries per ray keep the LDS footprint of a ray at tens of KB, i.e. a
// handful of rays per CU: with one wave per ray the latency-bound phases (staging, scans, merge) and the number of
// feature rows in flight were what set the kernel's time.  Wave w integrates the objects w, w + CW, ...; staging, the
// overlap fix, the merge, the global list and the feature rows are shared by all waves.
template <int CW>
__global__ __launch_bounds__(64 * CW) void k_composite(CompositeParams p) {
    extern __shared__ __attribute__((aligned(16))) char raw_smem[];
    constexpr int CT = 64 * CW;
    const int S = p.sort_size;
    CompositeSmem sm;
    const int A = (p.total_positions + 63) & ~63;   // per-entry arrays (the sort keys need the power of two S)
    sm.key = reinterpret_cast<unsigned int*>(raw_smem);
    sm.tt = reinterpret_cast<float*>(sm.key + S);
    sm.sg = sm.tt + A;
    sm.dm = sm.sg + A;
    sm.wo = sm.dm + A;
    sm.wg = sm.sg;       // the raw sigmas are dead once the merged list's alphas exist, which is before its weights do
    sm.al = sm.wo + A;
    // the divergence column exists only in differentiable training calls (keeps the eval footprint at 6 arrays)
    const bool use_div = p.any_divergence != 0;
    sm.dv = use_div ? sm.al + A : nullptr;
    sm.sl = reinterpret_cast<int*>(sm.al + (use_div ? 2 * A : A));
    float* scratch = reinterpret_cast<float*>(sm.sl + A);   // [CW * 64] cross-wave reductions
    // 64-bit sort scratch of the calls that always take the bitonic network (overlap fix), 8-byte aligned
    unsigned long long* wide = p.fix_overlaps ? reinterpret_cast<unsigned long long*>(scratch + 4 * 64) : nullptr;

    const int tid = threadIdx.x, lane = tid & 63;
    // wave-uniform by construction: as a scalar it keeps the per-object parameter reads (p.obj[k]) on the scalar path
    const int wave = (CW == 1) ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);
    const long g = blockIdx.x;
    const float* d = p.ray_directions + (size_t)g * 3;
    // |d| of the world-frame direction (integrate receives the untransformed directions, :880/:886)
    const float norm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
    const int PT = p.total_positions;

    // ---- stage every object's list ---------------------------------------------------------------
    {
        int off = 0;
        for (int k = 0; k < p.objects; ++k) {
            const CompositeObject& o = p.obj[k];
            const int P = o.positions;
            const size_t base = (size_t)g * P;
            for (int i = tid; i < P; i += CT) {
                sm.tt[off + i] = o.t[base + i];
                sm.sg[off + i] = o.sigma[base + i];
                sm.sl[off + i] = o.slot[base + i];
                sm.dm[off + i] = o.dispmag ? o.dispmag[base + i] : 0.f;
                if (use_div) sm.dv[off + i] = o.divergence ? fabsf(o.divergence[base + i]) : 0.f;
            }
            off += P;
        }
    }
    __syncthreads();

    // ---- integrate every object on its own: wave w takes the objects w, w + CW, ... ------------------
    // (wave-private data between the barriers: the alphas live in al[off ..), the object's own slice)
    for (int round = 0; round * CW < p.objects; ++round) {
        const int k = round * CW + wave;
        const bool mine = k < p.objects;
        int off = 0;
        for (int q = 0; q < k && q < p.objects; ++q) off += p.obj[q].positions;
        const CompositeObject& o = p.obj[mine ? k : 0];
        const int P = mine ? o.positions : 0;
        const size_t base = (size_t)g * P;
        float adiv = 0.f;   // sum alpha |div|  (object_composer.py:768-769, alphas detached)
        for (int i = lane; i < P; i += 64) {
            const float dt = (i < P - 1) ? __fsub_rn(sm.tt[off + i + 1], sm.tt[off + i]) : 1e10f;
            float raw = sm.sg[off + i];
            if (noise_present(o.noise)) raw = __fadd_rn(raw, noise_normal(o.noise, g, P, i));
            const float a = alpha_of(raw, __fmul_rn(dt, norm));
            sm.al[off + i] = a;
            if (use_div) adiv += a * sm.dv[off + i];
        }
        adiv = wave_sum(adiv);
        __syncthreads();
        if (mine) transmittance_weights(sm.al + off, P, lane);
        __syncthreads();
        float depth = 0.f, opacity = 0.f, dmag = 0.f;
        for (int i = lane; i < P; i += 64) {
            const float w = sm.al[off + i];
            sm.wo[off + i] = w;
            if (o.out.weights) o.out.weights[base + i] = w;
            depth += w * sm.tt[off + i];
            opacity += w;
            dmag += w * sm.dm[off + i];
        }
        depth = wave_sum(depth);
        opacity = wave_sum(opacity);
        dmag = wave_sum(dmag);
        if (mine && lane == 0) {
            if (o.out.depth) o.out.depth[g] = depth;
            if (o.out.opacity) o.out.opacity[g] = opacity;
            if (o.out.disparity) o.out.disparity[g] = disparity_of(depth, opacity);
            if (o.out.integrated_displacements_magnitude) o.out.integrated_displacements_magnitude[g] = dmag / (float)P;
            if (o.out.integrated_divergence) o.out.integrated_divergence[g] = adiv / (float)P;
        }
    }
    __syncthreads();

    // ---- static/dynamic overlap fix (fix_object_overlap, :295-397) ------------------------------
    // Static samples whose ORIGINAL t lies in [t_dyn[0], t_dyn[P_static - 1]) (searchsorted, left)
    // get sigma = -10, t = 0, displacement = 0.  The upper bound indexes the dynamic list with the
    // STATIC object's P - 1: reference behaviour, reproduced on purpose.
    if (p.fix_overlaps) {
        int dyn_off0 = 0;
        for (int k = 0; k < p.static_objects; ++k) dyn_off0 += p.obj[k].positions;
        int soff = 0;
        for (int s = 0; s < p.static_objects; ++s) {
            const int Ps = p.obj[s].positions;
            unsigned int masked_bits = 0;  // bit m <-> entry tid + CT m of this static list (Ps <= 2048)
            int doff = dyn_off0;
            for (int dd = p.static_objects; dd < p.objects; ++dd) {
                const float b0 = sm.tt[doff + 0];
                const float b1 = sm.tt[doff + Ps - 1];
                int lo0 = 0, hi0 = Ps;   // lower_bound(t_static, b0)
                while (lo0 < hi0) {
                    const int mid = (lo0 + hi0) >> 1;
                    if (sm.tt[soff + mid] < b0) lo0 = mid + 1; else hi0 = mid;
                }
                int lo1 = 0, hi1 = Ps;   // lower_bound(t_static, b1)
                while (lo1 < hi1) {
                    const int mid = (lo1 + hi1) >> 1;
                    if (sm.tt[soff + mid] < b1) lo1 = mid + 1; else hi1 = mid;
                }
                int m = 0;
                for (int i = tid; i < Ps; i += CT, ++m)
                    if (i >= lo0 && i < lo1) masked_bits |= 1u << m;
                doff += p.obj[dd].positions;
            }
            __syncthreads();  // every thread has finished searching the ORIGINAL t of this list
            int m = 0;
            for (int i = tid; i < Ps; i += CT, ++m) {
                if ((masked_bits >> m) & 1u) {
                    sm.tt[soff + i] = 0.f;
                    sm.sg[soff + i] = -10.0f;
                    sm.dm[soff + i] = 0.f;
                    if (use_div) sm.dv[soff + i] = 0.f;
                }
            }
            __syncthreads();
            soff += Ps;
        }
    }

    // ---- merge: order by (t, concatenation index) ------------------------------------------------
    {
        int counts[PR_MAX_OBJECTS];
        for (int k = 0; k < p.objects; ++k) counts[k] = p.obj[k].positions;
        order_entries(sm.key, sm.tt, counts, p.objects, PT, S, !p.fix_overlaps, tid, CT, wide);
    }

    // ---- global alphas / weights in sorted order -------------------------------------------------
    const size_t gbase = (size_t)g * PT;
    float gdiv = 0.f;
    for (int j = tid; j < PT; j += CT) {
        const int e = (int)sm.key[j];
        float dt = 1e10f;
        if (j < PT - 1) {
            const int en = (int)sm.key[j + 1];
            dt = __fsub_rn(sm.tt[en], sm.tt[e]);
        }
        float raw = sm.sg[e];
        if (noise_present(p.noise_global)) raw = __fadd_rn(raw, noise_normal(p.noise_global, g, PT, j));
        sm.al[j] = alpha_of(raw, __fmul_rn(dt, norm));
        if (use_div) gdiv += sm.al[j] * sm.dv[e];
    }
    __syncthreads();
    transmittance_weights_block<CW>(sm.al, PT, scratch, wave, lane);   // al now holds the sorted-order weights
    if (CW == 1) __syncthreads();
    {
        float depth = 0.f, opacity = 0.f, dmag = 0.f;
        for (int j = tid; j < PT; j += CT) {
            const int e = (int)sm.key[j];
            const float w = sm.al[j];
            sm.wg[e] = w;
            if (p.global.weights) p.global.weights[gbase + j] = w;
            depth += w * sm.tt[e];
            opacity += w;
            dmag += w * sm.dm[e];
        }
        depth = block_sum<CW>(depth, scratch, wave, lane);
        opacity = block_sum<CW>(opacity, scratch, wave, lane);
        dmag = block_sum<CW>(dmag, scratch, wave, lane);
        if (use_div) gdiv = block_sum<CW>(gdiv, scratch, wave, lane);
        if (tid == 0) {
            if (p.global.depth) p.global.depth[g] = depth;
            if (p.global.opacity) p.global.opacity[g] = opacity;
            if (p.global.disparity) p.global.disparity[g] = disparity_of(depth, opacity);
            if (p.global.integrated_displacements_magnitude)
                p.global.integrated_displacements_magnitude[g] = dmag / (float)PT;
            if (p.global.integrated_divergence) p.global.integrated_divergence[g] = gdiv / (float)PT;
        }
    }
    __syncthreads();

    // ---- geometry-only calls end here (PR_FLAG_GEOMETRY_ONLY; a parameter: uniform over the launch) -------------
    // visibility[g][k] = the global weights of object k's entries summed (wg is indexed by concatenation index: the objects'
    // offsets in concatenation order), in a fixed order; front_object = the lowest k that holds the ray's largest visibility,
    // -1 when none is > 0 (a NaN is never greater)
    if (p.geometry) {
        if (p.visibility != nullptr || p.front_object != nullptr) {
            float best = 0.f;
            int front = -1;
            int goff = 0;
            for (int k = 0; k < p.objects; ++k) {
                const int P = p.obj[k].positions;
                float v = 0.f;
                for (int i = tid; i < P; i += CT) v += sm.wg[goff + i];
                v = block_sum<CW>(v, scratch, wave, lane);
                if (tid == 0 && p.visibility != nullptr) as_global(p.visibility)[(size_t)g * p.objects + k] = v;
                if (v > best) {
                    best = v;
                    front = k;
                }
                goff += P;
            }
            if (tid == 0 && p.front_object != nullptr) as_global(p.front_object)[g] = front;
        }
        return;
    }

    // ---- features of a deferred call: one object per wave (the barrier above is the only one this pass needs: wo, wg, sl are complete)
    if (CW > 1 && p.pooled != nullptr) {
        pooled_row_sums<CW>(p, sm, g, wave, lane);
        return;       // (the global features and the decoder maps are written by the projection kernel)
    }

    // ---- features: one pass over the compact MLP rows --------------------------------------------
    // Per object the contributing samples (inside the box, non-zero weight) are compacted into per-wave lists (wave w
    // takes the w-th contiguous part of the object's samples; the sort keys are dead by now, their storage is reused),
    // then consumed ROWS_IN_FLIGHT rows at a time.  Every wave accumulates all F channels of its part; the parts are added
    // in wave order.
    const int F = p.F;
    const bool defer = p.pooled != nullptr;
    int* lrow = reinterpret_cast<int*>(sm.key);   // the ranks and the depths are dead by now
    float* lw1 = sm.tt;
    float accg[MAX_FCHUNK];
#pragma unroll
    for (int c = 0; c < MAX_FCHUNK; ++c) accg[c] = 0.f;
    int off = 0;
    for (int k = 0; k < p.objects; ++k) {
        const CompositeObject& o = p.obj[k];
        const int P = o.positions;
        const int part = (((P + CW - 1) / CW) + 63) & ~63;
        const int begin = wave * part;
        const int end = (begin + part < P) ? begin + part : P;
        __syncthreads();
        int count = 0;
        float bare1 = 0.f, bare2 = 0.f;   // PR_FLAG_SIGMOID_FEATURES: weights of the samples without a feature row (raw feature 0)
        for (int base = begin; base < end; base += 64) {
            const int i = base + lane;
            bool take = false;
            int row = -1;
            float w1 = 0.f, w2 = 0.f;
            if (i < end) {
                row = sm.sl[off + i];
                w1 = sm.wo[off + i];
                w2 = sm.wg[off + i];
                take = row >= 0 && (w1 != 0.f || w2 != 0.f);
                if (p.sigmoid && row < 0) {
                    bare1 += w1;
                    bare2 += w2;
                }
            }
            const unsigned long long m = __ballot(take);
            if (take) {
                const int pos = off + begin + count + __popcll(m & ((1ull << lane) - 1ull));
                lrow[pos] = row;
                lw1[pos] = w1;
                sm.al[pos] = w2;
            }
            count += __popcll(m);
        }
        // (the list of a wave is written and read by that wave only: no barrier needed in between)
        const int* rows_w = lrow + off + begin;
        const float* w1_w = lw1 + off + begin;
        const float* w2_w = sm.al + off + begin;
        float acco[MAX_FCHUNK];
#pragma unroll
        for (int c = 0; c < MAX_FCHUNK; ++c) acco[c] = 0.f;
        int i = 0;
        for (; i + ROWS_IN_FLIGHT <= count; i += ROWS_IN_FLIGHT) {
            float v[ROWS_IN_FLIGHT][MAX_FCHUNK];
#pragma unroll
            for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
                const float* f = o.feat + (size_t)rows_w[i + u] * F;
#pragma unroll
                for (int c = 0; c < MAX_FCHUNK; ++c) {
                    const int ch = lane + 64 * c;
                    v[u][c] = (ch < F) ? f[ch] : 0.f;
                    if (p.sigmoid) v[u][c] = sigmoid_of(v[u][c]);
                }
            }
#pragma unroll
            for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
                const float w1 = w1_w[i + u], w2 = w2_w[i + u];
#pragma unroll
                for (int c = 0; c < MAX_FCHUNK; ++c) {
                    acco[c] = __fadd_rn(acco[c], __fmul_rn(w1, v[u][c]));
                    accg[c] = __fadd_rn(accg[c], __fmul_rn(w2, v[u][c]));
                }
            }
        }
        for (; i < count; ++i) {
            const float* f = o.feat + (size_t)rows_w[i] * F;
            const float w1 = w1_w[i], w2 = w2_w[i];
#pragma unroll
            for (int c = 0; c < MAX_FCHUNK; ++c) {
                const int ch = lane + 64 * c;
                float v = (ch < F) ? f[ch] : 0.f;
                if (p.sigmoid) v = sigmoid_of(v);
                acco[c] = __fadd_rn(acco[c], __fmul_rn(w1, v));
                accg[c] = __fadd_rn(accg[c], __fmul_rn(w2, v));
            }
        }
        if (p.sigmoid) {      // sigmoid(0) = 0.5 for the samples that have no row; every lane owns channels, so all of them add
            bare1 = wave_sum(bare1);
            bare2 = wave_sum(bare2);
#pragma unroll
            for (int c = 0; c < MAX_FCHUNK; ++c) {
                acco[c] = __fadd_rn(acco[c], 0.5f * bare1);
                accg[c] = __fadd_rn(accg[c], 0.5f * bare2);
            }
        }
        // deferred projection (p.pooled): the rows are hidden rows [h | 1]; the sums of THIS object under its own and under the
        // global weights go to the pooled blocks 2 k and 2 k + 1, launch_projection applies [W6 | b6] of the object's model
        if (o.out.integrated_features)
            store_channel_sums<CW>(acco, defer ? p.pooled + ((size_t)(2 * k) * gridDim.x + g) * F : o.out.integrated_features + (size_t)g * F, F,
                                   scratch, wave, lane);
        if (defer) {
            if (p.global.integrated_features || p.decoder.groups > 0)
                store_channel_sums<CW>(accg, p.pooled + ((size_t)(2 * k + 1) * gridDim.x + g) * F, F, scratch, wave, lane);
#pragma unroll
            for (int c = 0; c < MAX_FCHUNK; ++c) accg[c] = 0.f;
        }
        off += P;
    }
    if (defer) return;       // (the global features and the decoder maps are written by the projection kernel)
    if (p.global.integrated_features) store_channel_sums<CW>(accg, p.global.integrated_features + (size_t)g * F, F, scratch, wave, lane);
    if (p.decoder.groups > 0) {
        // decoder layout: this ray is cell (r / width, r % width) of its group's grid; its channels go to the channels-first
        // map of the group (neighbouring rays = neighbouring workgroups fill neighbouring columns of every plane)
        if (CW > 1 && !p.global.integrated_features) {     // the cross-wave sums have not been formed yet
#pragma unroll
            for (int c = 0; c < MAX_FCHUNK; ++c) {
                if (64 * c >= F) break;
                __syncthreads();
                scratch[wave * 64 + lane] = accg[c];
                __syncthreads();
                if (wave == 0)
                    for (int w = 1; w < CW; ++w) accg[c] = __fadd_rn(accg[c], scratch[w * 64 + lane]);
            }
        }
        if (wave == 0) {
            const int frame = (int)(g / p.rays);
            int r = (int)(g - (long)frame * p.rays);
            int grp = 0;
            while (grp < p.decoder.groups - 1 && r >= p.decoder.rays[grp]) r -= p.decoder.rays[grp++];
            const int c0 = p.decoder.channel_begin[grp], c1 = p.decoder.channel_end[grp];
            const size_t cells = (size_t)p.decoder.rays[grp];
            float* map = p.decoder.map[grp] + (size_t)frame * (c1 - c0) * cells + r;
#pragma unroll
            for (int c = 0; c < MAX_FCHUNK; ++c) {
                const int ch = lane + 64 * c;
                if (ch >= c0 && ch < c1 && ch < F) map[(size_t)(ch - c0) * cells] = accg[c];
            }
        }
    }
}

int launch_composite(const CompositeParams& p, hipStream_t s) {
    PR_REQUIRE(p.F <= 64 * MAX_FCHUNK, "output_features %d exceeds %d", p.F, 64 * MAX_FCHUNK);
    PR_REQUIRE(p.sort_size >= p.total_positions && (p.sort_size & (p.sort_size - 1)) == 0, "bad sort size");
    for (int k = 0; k < p.objects; ++k)
        PR_REQUIRE(p.obj[k].positions <= 64 * 32, "positions per ray %d too large for the overlap mask", p.obj[k].positions);
    const size_t lds = (size_t)p.sort_size * 4 + (size_t)((p.total_positions + 63) & ~63) * (p.any_divergence ? 7 : 6) * 4 +
                       sizeof(float) * 4 * 64 + (p.fix_overlaps ? (size_t)p.sort_size * 8 : 0);
    PR_REQUIRE(lds <= 156 * 1024, "too many samples per ray for the compositing kernel (%d)", p.total_positions);
    if (p.decoder.groups > 0) {
        PR_REQUIRE(p.decoder.groups <= PR_MAX_DECODER_GROUPS, "decoder layout: %d groups (max %d)", p.decoder.groups, PR_MAX_DECODER_GROUPS);
        long sum = 0;
        for (int i = 0; i < p.decoder.groups; ++i) {
            PR_REQUIRE(p.decoder.rays[i] > 0 && p.decoder.width[i] > 0 && p.decoder.rays[i] % p.decoder.width[i] == 0,
                       "decoder layout: group %d has %d rays in rows of %d", i, p.decoder.rays[i], p.decoder.width[i]);
            PR_REQUIRE(p.decoder.channel_begin[i] >= 0 && p.decoder.channel_begin[i] < p.decoder.channel_end[i] && p.decoder.channel_end[i] <= (p.pooled ? p.out_features : p.F),
                       "decoder layout: group %d channel range [%d, %d) outside 0..%d", i, p.decoder.channel_begin[i], p.decoder.channel_end[i], p.pooled ? p.out_features : p.F);
            PR_REQUIRE(p.decoder.map[i] != nullptr, "decoder layout: group %d has no map", i);
            sum += p.decoder.rays[i];
        }
        PR_REQUIRE(sum == p.rays, "decoder layout: the groups hold %ld rays, the call has %d", sum, p.rays);
    }
    const long total = (long)p.frames * p.rays;
    ProfileScope scope(1, s);
    // four waves per ray once the lists are long enough to keep them busy; short lists (a few dozen entries) stay on one
    if (p.total_positions >= 256) {
        PR_TRY(prepare_kernel(reinterpret_cast<const void*>(&k_composite<4>), 156 * 1024, nullptr));   // the block-wide vote of order_entries owns a little static LDS
        hipLaunchKernelGGL(k_composite<4>, dim3((unsigned)total), dim3(256), lds, s, p);
    } else {
        PR_TRY(prepare_kernel(reinterpret_cast<const void*>(&k_composite<1>), 156 * 1024, nullptr));
        hipLaunchKernelGGL(k_composite<1>, dim3((unsigned)total), dim3(64), lds, s, p);
    }
    PR_LAUNCH_CHECK();
    return PR_OK;
}

// ---------------------------------------------------------------------------------------------
// Deferred projection (PR_FLAG_DEFER_PROJECTION): features_head.6 once per ray, behind the compositing sums.
//   object k:  integrated_features[ray] = [W6 | b6]_model(k) . pooled[2 k][ray]
//   global:    integrated_features[ray] = sum_k [W6 | b6]_model(k) . pooled[2 k + 1][ray]      (one accumulator chain, object order)
// A workgroup owns 64 rays and all output channels: wave w the 32-column blocks w and w + 4 for both 32-row blocks, like the MLP
// tile.  The pooled rows of one object are staged in LDS (zero-padded to the K step), the packed [W6 | b6 | 0] rows come from L2
// (100 KB per model, shared by every workgroup), 16 bytes of K per lane and load: lane (r, half) holds k = 8 q + 4 half + e of row /
// column r, for both operands of v_mfma_f32_32x32x2_f32.  The decoder layout of the global features is emitted here for these calls.
// ---------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int PJ_ROWS = 64;
constexpr int PJ_KMAX = MAX_WIDTH / 2 + 8;        // projection_k(W / 2) <= this
constexpr int PJ_LDA = PJ_KMAX + 4;
constexpr int PJ_TILE = PJ_ROWS * PJ_LDA;          // floats of one staged 64-ray tile
constexpr int PJ_LDS_BYTES = 2 * PJ_TILE * (int)sizeof(float);   // object k under its own and under the global weights: 70 KB, two workgroups per CU

// 64 pooled rows of one block, zero-padded to the K step and beyond the last ray, into LDS
__device__ __forceinline__ void stage_pooled_tile(float* S, const float* A, long row0, long total, int HW, int k4, int tid) {
    for (int idx = tid; idx < PJ_ROWS * k4; idx += 256) {
        const int row = idx / k4, c = (idx - row * k4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + row < total && c < HW) v = *reinterpret_cast<const float4*>(A + (size_t)row * HW + c);
        *reinterpret_cast<float4*>(S + row * PJ_LDA + c) = v;
    }
}

// One K step (8 floats of K: this lane's four) of a wave's 64 x 32 block: both row blocks against the weight fragment w.
__device__ __forceinline__ void project_step(f32x16 (&acc)[2], const float* a, const f32x4_t w) {
    const float4 x0 = *reinterpret_cast<const float4*>(a);
    const float4 x1 = *reinterpret_cast<const float4*>(a + 32 * PJ_LDA);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, w.x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, w.x, acc[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, w.y, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, w.y, acc[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.z, w.z, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.z, w.z, acc[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.w, w.w, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.w, w.w, acc[1], 0, 0, 0);
}

// Objects in order; object k's two pooled tiles (own weights, global weights) are staged together and multiplied off the SAME weight
// fragments - one pass over [W6 | b6] of the object's model feeds the object's own accumulators (fresh per object) and the global
// accumulators (one chain over the objects) - with the fragment of the next K step loaded before the current one is consumed.  Every
// accumulator sees its products in the order it always did: objects ascending (global), q ascending, x, y, z, w inside a step.
// 128 accumulator registers and two workgroups per CU (launch bounds): one workgroup's staging and stores hide behind the other's MFMAs.
__global__ __launch_bounds__(256, 2) void k_project_features(CompositeParams p) {
    extern __shared__ __attribute__((aligned(16))) float pj_smem[];
    float* SO = pj_smem;              // object k's pooled rows under its own weights
    float* SG = pj_smem + PJ_TILE;    // ... under the global weights
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long total = (long)p.frames * p.rays;
    const long row0 = (long)blockIdx.x * PJ_ROWS;
    const int HW = p.F, PK = p.proj_k, F = p.out_features;
    const int nblk = (F + 31) / 32;
    const int k4 = PK >> 2;
    const bool want_global = p.global.integrated_features != nullptr || p.decoder.groups > 0;
    f32x16 accg[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) accg[a][b][i] = 0.f;
    for (int k = 0; k < p.objects; ++k) {
        float* out = p.obj[k].out.integrated_features;
        const bool own = out != nullptr;
        if (!own && !want_global) continue;
        __syncthreads();     // the previous object's products have finished reading the tiles
        if (own) stage_pooled_tile(SO, p.pooled + ((size_t)(2 * k) * total + row0) * HW, row0, total, HW, k4, tid);
        if (want_global) stage_pooled_tile(SG, p.pooled + ((size_t)(2 * k + 1) * total + row0) * HW, row0, total, HW, k4, tid);
        __syncthreads();
        f32x16 acco[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acco[a][b][i] = 0.f;
        const float* W = p.proj_w[k];
        const int a0 = r * PJ_LDA + 4 * half;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int cb = wave + 4 * blk;
            if (cb >= nblk) continue;
            const auto* wp = as_global(reinterpret_cast<const f32x4_t*>(W + (size_t)(cb * 32 + r) * PK + 4 * half));
            f32x4_t w = wp[0];
            for (int q = 0; q < k4; q += 2) {
                const f32x4_t w_next = wp[q + 2 < k4 ? q + 2 : q];      // (the last step reads its own fragment again)
                if (own) project_step(acco[blk], SO + a0 + 4 * q, w);
                if (want_global) project_step(accg[blk], SG + a0 + 4 * q, w);
                w = w_next;
            }
        }
        // accumulator element i of lane (r, half): tile row (i & 3) + 8 (i >> 2) + 4 half (+ 32 for the second row block), column r - the
        // 32 lanes of a half write 128 consecutive bytes of a row
        if (own) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int col = (wave + 4 * blk) * 32 + r;
                if (col >= F) continue;
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const long g = row0 + 32 * rb + (i & 3) + 8 * (i >> 2) + 4 * half;
                        if (g < total) out[(size_t)g * F + col] = acco[blk][rb][i];
                    }
                }
            }
        }
    }
    if (!want_global) return;
    float* out = p.global.integrated_features;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int col = (wave + 4 * blk) * 32 + r;
        if (col >= F) continue;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long g = row0 + 32 * rb + (i & 3) + 8 * (i >> 2) + 4 * half;
                if (g >= total) continue;
                const float v = accg[blk][rb][i];
                if (out) out[(size_t)g * F + col] = v;
                if (p.decoder.groups > 0) {
                    // decoder layout: this ray is cell (r / width, r % width) of its group's grid (see k_composite)
                    const int frame = (int)(g / p.rays);
                    int rr = (int)(g - (long)frame * p.rays);
                    int grp = 0;
                    while (grp < p.decoder.groups - 1 && rr >= p.decoder.rays[grp]) rr -= p.decoder.rays[grp++];
                    const int c0 = p.decoder.channel_begin[grp], c1 = p.decoder.channel_end[grp];
                    const size_t cells = (size_t)p.decoder.rays[grp];
                    float* map = p.decoder.map[grp] + (size_t)frame * (c1 - c0) * cells + rr;
                    if (col >= c0 && col < c1) map[(size_t)(col - c0) * cells] = v;
                }
            }
        }
    }
}

int launch_projection(const CompositeParams& p, hipStream_t s) {
    PR_REQUIRE(p.pooled != nullptr, "deferred projection without pooled rows");
    PR_REQUIRE(p.proj_k >= p.F && p.proj_k <= PJ_KMAX && (p.proj_k & 7) == 0 && (p.F & 3) == 0, "deferred projection: row of %d floats, K %d",
               p.F, p.proj_k);
    PR_REQUIRE(p.out_features >= 1 && p.out_features <= 256, "deferred projection: output_features %d", p.out_features);
    for (int k = 0; k < p.objects; ++k) PR_REQUIRE(p.proj_w[k] != nullptr, "deferred projection: object %d has no packed matrix", k);
    const long total = (long)p.frames * p.rays;
    ProfileScope scope(1, s);
    PR_TRY(prepare_kernel(reinterpret_cast<const void*>(&k_project_features), PJ_LDS_BYTES, nullptr));
    hipLaunchKernelGGL(k_project_features, dim3((unsigned)((total + PJ_ROWS - 1) / PJ_ROWS)), dim3(256), PJ_LDS_BYTES, s, p);
    PR_LAUNCH_CHECK();
    return PR_OK;
}

}  // namespace pr
