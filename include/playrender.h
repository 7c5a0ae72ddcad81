/*
 * playrender.h - C ABI of libplayrender.so, the MI355X (gfx950) volumetric renderer.
 *
 * The reference (willi-menapace/PlayableEnvironments) is pure Python/PyTorch: the interface this
 * library replaces is the tensor-in / dict-of-tensors-out call
 *     ObjectComposer.forward(ray_origins, ray_directions, focal_normals, transformation_matrix_w2o,
 *                            style, deformation, object_in_scene, perturb, ...)
 * (model/object_composer.py:786-892) plus the ray set-up of
 * EnvironmentModel.forward_from_scene_encoding (model/environment_model.py:1080-1112).  The Python
 * package `playableenvironments_amd` keeps those signatures and marshals raw device pointers into
 * the entry points below through ctypes (see INTEGRATION.md for the binding a maintainer adds).
 *
 * Conventions
 *   - every function returns 0 on success, a negative pr_status on failure; pr_last_error()
 *     returns a thread-local message for the last failure on the calling thread;
 *   - all pointers are DEVICE pointers unless a parameter says "host"; the library never
 *     allocates or frees device memory, never synchronises the device and enqueues all work on
 *     the hipStream_t passed in (void* so that the header needs no HIP include);
 *   - all floating-point data is IEEE fp32, C-contiguous, in the layouts written next to each field;
 *   - "N" = frames (all leading dims of the reference tensors flattened), "R" = rays per frame,
 *     "K" = object instances, "P_k" = samples per ray of object k, "F" = output features.
 */
#ifndef PLAYRENDER_H
#define PLAYRENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PR_ABI_VERSION 5
#define PR_MAX_OBJECTS 8
#define PR_MAX_LAYERS 12
#define PR_MAX_OCTAVES 16

typedef enum pr_status {
    PR_OK = 0,
    PR_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    PR_ERR_WORKSPACE = -2,    /* workspace too small */
    PR_ERR_HIP = -3,          /* a HIP runtime call failed */
    PR_ERR_NO_DEVICE = -4     /* no gfx950 device visible */
} pr_status;

/* flags of pr_call_t.flags */
#define PR_FLAG_PERTURB        1u   /* stratified jitter + alpha noise; noise tensors must be supplied */
#define PR_FLAG_CANONICAL_POSE 2u   /* zero the ray-bender displacements (canonical_pose=True) */
#define PR_FLAG_FIX_OVERLAPS   4u   /* config["model"]["fix_object_overlaps"] */
#define PR_FLAG_NAIVE_MLP      8u   /* debugging: scalar one-thread-per-sample MLP kernel instead of MFMA */
#define PR_FLAG_TRAIN_BN       16u  /* module.training: the AdaIN BatchNorm1d layers normalise with batch statistics of
                                       the evaluated samples of each object call and update running_mean / running_var /
                                       num_batches_tracked in place (model/layers/adain.py:47,58) */

#define PR_FLAG_SAVE_FOR_BACKWARD 32u /* keep every intermediate pr_render_backward needs inside the workspace; the
                                       workspace must stay untouched until the backward call.  With PR_FLAG_TRAIN_BN
                                       the backward pass differentiates the batch statistics (training); without it
                                       the running statistics are constants (a differentiable eval-mode call, e.g.
                                       test-time optimisation of poses or style codes).  PR_PRECISION_FP32 only. */

#define PR_FLAG_GATE_HEAD 64u        /* sigma-gated feature head: samples whose raw density is <= 0 have alpha = 1 - exp(-relu(sigma) dt)
                                       = 0 exactly, so their 192-channel feature rows never reach a compositing sum
                                       (model/object_composer.py:180-214); with this flag the feature head (3 of the 11
                                       matrix products of a sample) runs on the other samples only.  Results are
                                       bit-identical.  Honoured for evaluation calls only - ignored with PR_FLAG_PERTURB
                                       or any integrate-noise pointer (noise is added to the density before the ReLU),
                                       PR_FLAG_TRAIN_BN (batch statistics need every row), PR_FLAG_SAVE_FOR_BACKWARD and
                                       PR_FLAG_NAIVE_MLP. */

#define PR_FLAG_DEVICE_NOISE 128u    /* with PR_FLAG_PERTURB (and for the Hutchinson probes of training calls): every noise tensor whose
                                       pointer in pr_noise_t is NULL is GENERATED inside the kernels that consume it - a
                                       counter-based generator (Philox4x32-10) keyed by pr_call_t.noise_seed and the tensor's
                                       stream id, indexed by the element index, so pr_render_backward regenerates exactly
                                       the forward pass's values and no (N,R,P) noise tensor is materialised (the reference
                                       draws them with torch.rand / torch.randn: utils/lib_3d/ray_helper.py:1275,1380,
                                       model/object_composer.py:553,597,751).  pr_noise_fill writes the same values to a
                                       tensor (tests replay them through the explicit path and the oracle). */

#define PR_FLAG_SIGMOID_FEATURES 512u /* config["model"]["apply_activation"]: the raw features of every sample go through a sigmoid before
                                        they are composited (object_composer.py:548-549, :573-574; RGB-output models).  Applied
                                        where the compositing kernel reads a feature row; samples without a row (outside the box:
                                        raw feature 0) composite sigmoid(0) = 0.5 wherever their weight is not zero. */
#define PR_FLAG_SPLIT_BACKWARD 1024u /* differentiable calls (with PR_FLAG_SAVE_FOR_BACKWARD, on the forward AND the backward call; ABI 5):
                                       the matrix products of pr_render_backward in split precision, fp32 accumulation, every operand an
                                       fp16 pair (x = hi + lo, three fp16 MFMAs per product): the backward chains on the gradient tile
                                       times a power of two chosen per 64-row tile and the weights times 2^8, the weight gradients on
                                       16-row half slabs - gradient rows times a power of two alpha, activation rows times C / alpha, C a
                                       running power of two per work item (all scalings exact).  On the forward call the flag
                                       selects fp16-pair products for phase 1 of a train-mode forward pass too.  The call
                                       stays PR_PRECISION_FP32 (fp32-packed weights, which carry both split forms as well).  Products
                                       that have no split kernel run the exact fp32 one. */
#define PR_FLAG_DEFER_PROJECTION 2048u /* deferred projection: features_head.6 is a Linear with nothing behind it and its rows are only ever
                                       summed under the compositing weights, so sum_i w_i (W6 h_i + b6) = W6 (sum_i w_i h_i) + b6 sum_i w_i.
                                       With this flag the MLP kernels stop behind features_head.4 and write [h, 1] rows (W/2 + 1 floats,
                                       padded to a multiple of 4; the 1 is 0 on the rows the network wrote as zeros), compositing pools
                                       those rows per object under the object's own and under the global weights, and one matrix product
                                       per ray applies [W6 | b6].  Every field except integrated_features and the decoder maps is
                                       bit-identical; those two differ by fp32 re-association.  Honoured for PR_PRECISION_FP32 evaluation
                                       calls only - ignored with PR_FLAG_SAVE_FOR_BACKWARD, PR_FLAG_TRAIN_BN, PR_FLAG_SIGMOID_FEATURES
                                       (the sigmoid sits between the projection and the sum) and PR_FLAG_NAIVE_MLP.  Perturbed calls
                                       are eligible.  The workspace grows by the pooled rows (pr_workspace_size accounts for them). */
#define PR_FLAG_GEOMETRY_ONLY 4096u  /* geometry-only render (depth, opacity, weights, object mattes): the MLP of every object and level stops
                                       behind the density head (after the ray bender and the backbone), no feature row, pending stack or
                                       pooled row exists, compositing ends behind the global weights and the scalar fields.  Every field
                                       the call returns is bit for bit what the full render returns.  pr_workspace_size leaves out the
                                       feature arena, the pending stacks and the pooled rows.  PR_FLAG_GATE_HEAD, PR_FLAG_DEFER_PROJECTION
                                       and PR_FLAG_SIGMOID_FEATURES are ignored.  Honoured by every render entry point; refused
                                       (PR_ERR_INVALID, before any device work): a non-NULL integrated_features pointer in any entry of
                                       either level, decoder.groups > 0, PR_FLAG_TRAIN_BN, PR_FLAG_SAVE_FOR_BACKWARD, PR_FLAG_NAIVE_MLP, a
                                       non-NULL pr_retained_t.  Perturbation, occupancy grids and the fine guide keep their rules.
                                       head_samples is 0 for every object; skybox models (constant density) run no MLP launch. */
#define PR_FLAG_DIVERGENCE_GRAD 256u /* pr_backward_workspace_size / pr_render_backward: gradients of integrated_divergence are
                                       given (pr_entry_grads_t.integrated_divergence); the backward pass then differentiates the
                                       Hutchinson estimate e^T (d delta / dx) e through the ray bender (the reference's double
                                       backward, object_composer.py:582-601 with create_graph=True): one more pass over the
                                       bender with the probe tangents in place of the activations.  Sizes the tangent stack
                                       inside the backward workspace; ignored by pr_render_forward. */

/* One nn.Linear in the reference layout: weight (out_features, in_features) row-major, bias (out) or NULL. */
typedef struct pr_linear_t {
    const float* weight;
    const float* bias;
    int32_t out_features;
    int32_t in_features;
} pr_linear_t;

/*
 * One object model = RayBendingStyleNerfModel (model/nerf_models/ray_bending_style_nerf_model.py:12)
 * with its raw parameter pointers (the nn.Parameter storages, zero copy).
 */
typedef struct pr_object_model_t {
    int32_t kind;                    /* 0 = AdaInStyleNerfModel, 1 = SkyboxAdaInStyleNerfModelV3 */
    int32_t has_bender;              /* 1 = PositionalRayBender, 0 = ZeroedRayBender */
    int32_t positions;               /* samples per ray evaluated by THIS model: P_coarse, or P_coarse + P_fine */
    int32_t style_features;          /* S */
    int32_t deformation_features;    /* D */
    int32_t output_features;         /* F */
    int32_t layers_width;            /* backbone width (256) */
    int32_t backbone_count;          /* 8 */
    int32_t skip_layer_idx;          /* 4 */
    int32_t octaves;                 /* NeRF positional-encoder octaves (10); append_original is required */
    int32_t bender_width;            /* 128 */
    int32_t bender_count;            /* 6 */
    int32_t bender_skip;             /* 3 */
    int32_t bender_octaves;          /* 6 */
    float bender_octave_weights[PR_MAX_OCTAVES]; /* annealing weights evaluated on the host from current_step
                                                    (model/annealable_positional_encoder.py:59-63) */
    float bbox[6];                   /* x_lo, x_hi, y_lo, y_hi, z_lo, z_hi */
    float empty_space_alpha;
    float z_near_min;
    float z_far_max;
    float bn_eps;                    /* 1e-5 */
    /* nerf_model.* */
    pr_linear_t backbone[PR_MAX_LAYERS];
    pr_linear_t alpha_head;          /* weight == NULL for the skybox (sigma == 10) */
    pr_linear_t head0;               /* features_head.0, no bias */
    pr_linear_t affine1;             /* features_head.1.affine_transform (2*W, S) */
    float* bn1_mean;                 /* features_head.1.ada_in.normalization.running_mean (W); written with PR_FLAG_TRAIN_BN */
    float* bn1_var;
    int64_t* bn1_batches;            /* ...num_batches_tracked (int64 scalar) or NULL */
    pr_linear_t head3;               /* features_head.3, no bias (W/2, W) */
    pr_linear_t affine4;             /* features_head.4.affine_transform (W, S) */
    float* bn4_mean;
    float* bn4_var;
    int64_t* bn4_batches;
    pr_linear_t head6;               /* features_head.6 (F, W/2) */
    /* ray_bender.* (ignored when has_bender == 0) */
    pr_linear_t bender[PR_MAX_LAYERS];
    pr_linear_t bender_out;          /* output_head (3, BW), no bias */
} pr_object_model_t;

/* Bytes of the MFMA-fragment-ordered copy of one model's weights (see DESIGN.md "packed weights"). */
int pr_packed_size(const pr_object_model_t* model, size_t* bytes);

/* Gathers the raw parameters into `packed` (device, pr_packed_size bytes, 256-B aligned).  Must be
 * re-run whenever parameter VALUES change; cheap (one pass over ~2.9 MB).
 * precision: PR_PRECISION_FP32 = fp32 MFMA fragments (exact fp32 arithmetic); PR_PRECISION_F16X3 = every weight
 * as an fp16 pair (hi, lo = w - hi) for the split kernel, which evaluates
 * a*w ~ a_hi*w_hi + a_hi*w_lo + a_lo*w_hi with three fp16 MFMAs and fp32 accumulation
 * (~22 significant bits).  Both layouts have the same size.  PR_PRECISION_F16 = the F16X3 layout (the same bytes)
 * evaluated with the a_hi*w_hi product only: plain fp16 operands (11 significant bits each), fp32 accumulation, one
 * MFMA per step instead of three - the throughput tier for interactive play, ~1e-3 relative error on the rendered
 * features (tests/test_gpu.py holds it to >= 40 dB PSNR against the oracle); not for parity checks. */
#define PR_PRECISION_FP32  0
#define PR_PRECISION_F16X3 1
#define PR_PRECISION_F16   2
int pr_pack_model(const pr_object_model_t* model, int32_t precision, void* packed, size_t packed_bytes, void* stream);
/* The same for several models (models[i] -> packed[i] at precisions[i]) in as few launches as their jobs allow: a training step
 * re-packs every model after every optimiser step. */
int pr_pack_models(int32_t count, const pr_object_model_t* const* models, const int32_t* precisions, void* const* packed,
                   const size_t* packed_bytes, void* stream);

/* One object instance of a call: its (shared) coarse / fine models and their packed copies. */
typedef struct pr_object_t {
    pr_object_model_t coarse;
    const void* packed_coarse;
    pr_object_model_t fine;          /* used only when pr_call_t.use_fine != 0 */
    const void* packed_fine;
} pr_object_t;

/* Optional explicit noise of one model type, NULL = not perturbed (required with PR_FLAG_PERTURB). */
typedef struct pr_noise_t {
    const float* jitter[PR_MAX_OBJECTS];      /* coarse only: U[0,1) (N,R,P_k)  ray_helper.py:1275 */
    const float* alpha[PR_MAX_OBJECTS];       /* coarse only: N(0,1) (N,R,P_k)  object_composer.py:553 */
    const float* pdf[PR_MAX_OBJECTS];         /* coarse only: U[0,1) (N,R,Pf_k) ray_helper.py:1380 */
    const float* integrate[PR_MAX_OBJECTS];   /* N(0,1) (N,R,P_k) object_composer.py:880 -> :751 */
    const float* integrate_global;            /* N(0,1) (N,R,sum P_k), applied AFTER the sort, :886 */
    const float* divergence[PR_MAX_OBJECTS];  /* N(0,1) (N,R,P_k,3): Hutchinson probe of compute_approximate_divergence
                                                 (object_composer.py:582-601); read only with PR_FLAG_SAVE_FOR_BACKWARD
                                                 (the reference returns zeros unless it trains with a graph), objects
                                                 with a ray bender only; NULL = divergence left at zero */
} pr_noise_t;

/* Result fields of ObjectComposer.integrate (model/object_composer.py:774-782); any pointer may be NULL. */
typedef struct pr_entry_t {
    float* integrated_features;               /* (N,R,F) */
    float* opacity;                           /* (N,R) */
    float* weights;                           /* (N,R,P) ; global: (N,R,sum P_k) in sorted order */
    float* depth;                             /* (N,R) */
    float* disparity;                         /* (N,R)  NaN where opacity == 0, as the reference */
    float* integrated_displacements_magnitude;/* (N,R) */
    float* integrated_divergence;             /* (N,R)  zeros (eval) */
} pr_entry_t;

/* Optional emission of the global entry's integrated features in the layout the reference's CNN decoder consumes
 * (model/environment_model_multiresolution_backpropagated_decoder.py:67-106, environment_model_backpropagated_autoencoder.py
 * :128-168): the rays of a call are the concatenation of `groups` row-major grids (the strided grids of a full frame, or
 * the strided patches of a training call, smallest stride first); group i owns the feature channels
 * [channel_begin[i], channel_end[i]) and receives them as a channels-first map.  Replaces split_strided_patch_ray_samples /
 * fold_strided_tensors + split_features_by_layer + permute (two passes over the feature map) by the compositing kernel's
 * own stores. */
#define PR_MAX_DECODER_GROUPS 4
typedef struct pr_decoder_layout_t {
    int32_t groups;                               /* 0 = off */
    int32_t rays[PR_MAX_DECODER_GROUPS];          /* rays of each group; their sum must be R */
    int32_t width[PR_MAX_DECODER_GROUPS];         /* grid width of each group (rays[i] % width[i] == 0) */
    int32_t channel_begin[PR_MAX_DECODER_GROUPS];
    int32_t channel_end[PR_MAX_DECODER_GROUPS];
    float* map[PR_MAX_DECODER_GROUPS];            /* (N, channel_end - channel_begin, rays / width, width) */
} pr_decoder_layout_t;

typedef struct pr_outputs_t {
    pr_entry_t object[PR_MAX_OBJECTS];
    pr_entry_t global;
    /* optional exports of intermediate per-sample state, for stage-level parity tests */
    float* sample_t[PR_MAX_OBJECTS];          /* (N,R,P_k) sample depths */
    float* sample_sigma[PR_MAX_OBJECTS];      /* (N,R,P_k) raw sigma incl. empty_space_alpha fill */
    int32_t* sample_slot[PR_MAX_OBJECTS];     /* (N,R,P_k) compact row of the sample, -1 = outside the box */
    int32_t* evaluated_samples;               /* (K) number of samples sent through the MLP */
    int32_t* normalised_samples;              /* (K) PR_FLAG_TRAIN_BN: samples that entered the batch statistics */
    float* sample_delta[PR_MAX_OBJECTS];      /* (N,R,P_k,3) ray-bender displacement of every sample (zeros outside the
                                                 box / without a bender), input of pr_expected_positions */
    int32_t* head_samples;                    /* (K) number of samples sent through the feature head: evaluated_samples
                                                 unless PR_FLAG_GATE_HEAD skipped the ones with density <= 0 */
    pr_decoder_layout_t decoder;              /* global.integrated_features additionally in decoder layout (groups = 0: off) */
} pr_outputs_t;

typedef struct pr_call_t {
    int32_t frames;                  /* N */
    int32_t rays;                    /* R */
    int32_t objects;                 /* K */
    int32_t static_objects;          /* first `static_objects` instances are static (overlap fix) */
    int32_t use_fine;                /* 1 = hierarchical pass with the fine models (all objects) */
    uint32_t flags;
    int32_t precision;               /* PR_PRECISION_*: must match the precision the objects' weights were packed with */
    int32_t reserved_;
    const float* ray_origins;        /* (N,3) world frame */
    const float* ray_directions;     /* (N,R,3) world frame, not normalised */
    const float* w2o;                /* (N,K,3,4) top three rows of transformation_matrix_w2o */
    const float* style;              /* (N,K,S) */
    const float* deformation;        /* (N,K,D) */
    const uint8_t* object_in_scene;  /* (N,K) */
    const float* linspace_coarse[PR_MAX_OBJECTS]; /* torch.linspace(0,1,P_k) evaluated by the host (P_k) */
    const float* linspace_fine[PR_MAX_OBJECTS];   /* torch.linspace(0,1,Pf_k) */
    int32_t positions_fine[PR_MAX_OBJECTS];       /* Pf_k (resampled positions, use_fine only) */
    pr_noise_t noise_coarse;
    pr_noise_t noise_fine;           /* only .integrate / .integrate_global / .divergence are read */
    uint64_t noise_seed;             /* PR_FLAG_DEVICE_NOISE: seed of the call's generated noise */
    int32_t noise_ray_offset;        /* PR_FLAG_DEVICE_NOISE, calls that are a ray range [offset, offset + R) of a larger */
    int32_t noise_total_rays;        /* render of noise_total_rays rays per frame (0 = this call is the whole render) */
    const uint64_t* noise_seed_device; /* PR_FLAG_DEVICE_NOISE: NULL, or the seed as ONE device word that the kernels read when they run
                                        (noise_seed is then ignored): a call recorded into a HIP graph draws fresh noise on
                                        every replay if the word is rewritten between replays.  pr_render_backward must find the
                                        value its forward call saw. */
} pr_call_t;

/* Workspace bytes pr_render_forward needs for this call (host computation, no device work). */
int pr_workspace_size(const pr_call_t* call, const pr_object_t* objects, size_t* bytes);

/*
 * The renderer: sample placement -> AABB cull + compaction -> fused MLP -> (hierarchical resampling
 * -> fused MLP) -> per-object and cross-object compositing.  `coarse` receives the result of the
 * coarse models, `fine` (may be NULL unless use_fine) the hierarchical pass.
 */
int pr_render_forward(const pr_call_t* call, const pr_object_t* objects,
                      const pr_outputs_t* coarse, const pr_outputs_t* fine,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * Empty-space skipping for evaluation renders.  A grid divides the model's bounding box into cells[0] x cells[1] x cells[2] cells
 * and holds one bit per cell and frame: bit (cell & 31) of word bits[n * words + (cell >> 5)], cell = (c_x * cells[1] + c_y) *
 * cells[2] + c_z.  A sample at object-frame position x = o + d t (the unbent position the box test uses) is kept iff it passes
 * the closed-interval box test and the bit of its cell is 1, with, in fp32 and without contraction,
 *     u_a = (x_a - lo_a) * s_a,   s_a = (float)cells[a] / (hi_a - lo_a),   c_a = min(cells[a] - 1, (int)u_a).
 * A culled sample is treated exactly like a sample outside the box: slot -1, density empty_space_alpha, feature row 0,
 * displacement 0; it keeps its depth and takes part in compositing, the overlap fix and the resampler's CDF.  The grid of the
 * coarse model culls the coarse pass, the grid of the fine model the merged coarse + resampled positions of the fine pass.
 * bits == NULL: the object is not culled at that level.  A grid on a skybox model (kind == 1) or on a model whose box has an
 * empty axis (hi <= lo) is refused.
 */
typedef struct pr_occupancy_grid_t {
    const uint32_t* bits;            /* (N, words) device, or NULL */
    int32_t cells[3];
    int32_t words;                   /* words between frames, >= ceil(cells[0] * cells[1] * cells[2] / 32) */
} pr_occupancy_grid_t;

typedef struct pr_occupancy_t {
    pr_occupancy_grid_t coarse[PR_MAX_OBJECTS];
    pr_occupancy_grid_t fine[PR_MAX_OBJECTS];     /* read only when pr_call_t.use_fine != 0 */
} pr_occupancy_t;

/*
 * pr_render_forward with occupancy grids (occupancy == NULL: exactly pr_render_forward).  Unperturbed evaluation calls only: with
 * any grid set, PR_FLAG_PERTURB, an integrate-noise pointer, PR_FLAG_TRAIN_BN, PR_FLAG_SAVE_FOR_BACKWARD and PR_FLAG_NAIVE_MLP
 * are refused (PR_ERR_INVALID).  pr_workspace_size is unchanged (culling only shrinks the row counts); evaluated_samples /
 * head_samples report the counts after culling.  The bits are read when the kernels run: a call recorded into a HIP graph sees
 * what pr_occupancy_build last wrote into them.
 */
int pr_render_forward_culled(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                             const pr_outputs_t* coarse, const pr_outputs_t* fine,
                             void* workspace, size_t workspace_bytes, void* stream);

/*
 * Retained per-sample state, for evaluation frames on a camera that stands still.  The per-sample state of an object - t, sigma,
 * slot, dispmag and the compact feature rows of both levels - is a function of the camera rays, the object's own w2o / style /
 * deformation / presence rows, its weights and BatchNorm running statistics and its occupancy bits, and of nothing else; the
 * compositing kernel only reads it.  With a pr_retained_t the arrays of the objects in object_mask live in `cache` instead of the
 * workspace, next to a copy of everything they depend on.  The first launch of the call compares those copies with the call's inputs
 * BITWISE (32-bit words: a NaN equals the same NaN) on the device; an object whose key, the camera key and the host digest all match
 * skips placement, compaction, resampling and the MLP (its jobs return at once, its row count is forced to 0) and only compositing
 * reads its cached arrays - the result is bit for bit what the call would have recomputed.  Every other retained object is rendered
 * by the same kernels as without retention, writing into the cache, and the last launches of the call store its key.  An object
 * that is not reused is marked invalid before anything overwrites its arrays.  No host read-back: a call recorded into a HIP graph
 * holds both outcomes.  Every fill and flag write is a kernel (no memset node).
 *
 * What the device cannot see is the caller's: host_key must change whenever the VALUES of the retained objects' packed weights
 * change.  The library adds a digest of what it sees on the host (honoured flags, precision, N, R, K, use_fine, positions, the scalar
 * fields of the models incl. box, depth range and octave weights, occupancy cell counts, object_mask, the parameters of a fine guide); another digest: nothing reused.
 *
 * Cache layout (private; every region 256-byte aligned; pr_retained_size is their sum): a 256-byte header; ray_origins (N,3) and
 * ray_directions (N,R,3); per retained object w2o (N,12), presence (N words), style (N,S), deformation (N,D); per level bn1 mean /
 * var (W), bn4 mean / var (W/2) and - unless the model is a skybox - N x 8192 words of occupancy bits (a grid on a retained object
 * may have at most 64^3 = 262144 cells); per level t, sigma, slot (N R P_k words each), dispmag (the same, models with a bender) and
 * the feature rows (N R P_k rows of output_features floats, or of W/2 + 1 rounded up to 4 when the deferred projection is active).
 * pr_workspace_size is unchanged: the workspace regions of retained objects go unused.
 *
 * evaluated_samples / head_samples report THIS call's MLP work: 0 for a reused object.  Refused (PR_ERR_INVALID, before any device
 * work): PR_FLAG_PERTURB or an integrate-noise pointer, PR_FLAG_TRAIN_BN, PR_FLAG_SAVE_FOR_BACKWARD, PR_FLAG_NAIVE_MLP, a mask bit
 * at or beyond `objects`, a misaligned or too small cache, a sample_delta export of a retained object (the dense displacement is not
 * cached).
 */
typedef struct pr_retained_t {
    uint32_t object_mask;   /* bit k: object k of the call is retained */
    uint32_t reserved_;
    uint64_t host_key;      /* caller's epoch of what the device cannot see: packed weight values of the retained objects' models */
    void*    cache;         /* device, 256-byte aligned, pr_retained_size bytes, owned by the caller, untouched between calls */
    size_t   cache_bytes;
    int32_t* reused;        /* out (K) device or NULL: 1 = the object's cached state was used by this call, 0 = it was rendered */
} pr_retained_t;
/* Bytes of the cache for this call and mask (host computation, no device work). */
int pr_retained_size(const pr_call_t* call, const pr_object_t* objects, uint32_t object_mask, size_t* bytes);
/* Marks a cache invalid: one kernel launch on `stream`.  Required once before the first use. */
int pr_retained_reset(void* cache, size_t cache_bytes, void* stream);
/* pr_render_forward_culled with retention (retained == NULL: exactly pr_render_forward_culled; occupancy may be NULL). */
int pr_render_forward_retained(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                               const pr_retained_t* retained, const pr_outputs_t* coarse, const pr_outputs_t* fine,
                               void* workspace, size_t workspace_bytes, void* stream);

/*
 * Fine guide: the fine pass of the objects in object_mask evaluates a merged (coarse + resampled) sample only where the coarse pass
 * found density near it.  For one ray let tc[0 .. Pc - 1] be the coarse depths and s[i] the raw coarse density as the resampler reads
 * it (the coarse model's sigma, or empty_space_alpha for an object that is absent from the frame); coarse sample i is LIVE iff
 * s[i] > threshold.  A merged sample at depth t has j = max(0, #{i : tc[i] <= t} - 1) (comparisons only) and is kept iff some i in
 * [j - guard, j + 1 + guard] (clipped to [0, Pc - 1]) is live AND it passes the box test and the fine occupancy bit, if any.  A
 * sample the guide drops is treated exactly like a sample outside the box: slot -1, density empty_space_alpha, feature row 0,
 * displacement 0; it keeps its depth and takes part in compositing and the overlap fix.  The coarse pass is untouched;
 * evaluated_samples / head_samples of the fine level report the counts after culling.  This is an APPROXIMATION that is only as good
 * as the coarse model's agreement with the fine one (nothing about it is conservative); threshold = -inf keeps every sample.
 *
 * scratch holds one keep bit per merged sample - bit (i & 31) of word (i >> 5) of the ray's ceil((Pc_k + Pf_k) / 32) words - for the
 * guided objects in ascending order, each object's (N, R, words) region rounded up to 256 bytes: pr_fine_guide_size is the sum of
 * align256(4 * N * R * ceil((Pc_k + Pf_k) / 32)) over the objects of the mask.  Every word is written by the resampler before the
 * compaction reads it (no memset, no atomics); the scratch holds nothing between calls and must not be shared by calls in flight.
 * Retention: a retained object that is reused skips both kernels; object_mask, guard and the bits of threshold enter the
 * retained cache's host digest (another guide: nothing reused).
 *
 * Unperturbed evaluation calls with use_fine only.  Refused (PR_ERR_INVALID, before any device work) with a non-zero object_mask:
 * PR_FLAG_PERTURB or an integrate-noise pointer, PR_FLAG_TRAIN_BN, PR_FLAG_SAVE_FOR_BACKWARD, PR_FLAG_NAIVE_MLP, use_fine == 0, a mask
 * bit at or beyond `objects` or on a skybox model (kind == 1), guard < 0, a NaN threshold, a misaligned or too small scratch.
 * object_mask == 0: exactly a NULL guide.
 */
typedef struct pr_fine_guide_t {
    uint32_t object_mask;   /* bit k: the fine pass of object k is guided */
    int32_t  guard;         /* >= 0: coarse samples the live window extends to either side */
    float    threshold;     /* a coarse sample is live iff its raw density is > threshold (0: alpha exactly 0 below) */
    uint32_t reserved_;
    uint32_t* scratch;      /* device, 256-byte aligned, pr_fine_guide_size bytes, caller-owned */
    size_t   scratch_bytes;
} pr_fine_guide_t;
/* Bytes of the scratch for this call and mask (host computation, no device work). */
int pr_fine_guide_size(const pr_call_t* call, const pr_object_t* objects, uint32_t object_mask, size_t* bytes);
/* pr_render_forward_retained with a fine guide (guide == NULL: exactly pr_render_forward_retained; occupancy and retained may be
 * NULL).  pr_workspace_size is unchanged. */
int pr_render_forward_guided(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                             const pr_retained_t* retained, const pr_fine_guide_t* guide, const pr_outputs_t* coarse,
                             const pr_outputs_t* fine, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Geometry-only render (PR_FLAG_GEOMETRY_ONLY, required here: PR_ERR_INVALID without it): pr_render_forward_guided without a
 * `retained` argument plus two optional per-level outputs (each pr_geometry_t pointer and each of its fields may be NULL):
 *   visibility (N,R,K): visibility[n][r][k] = sum of the GLOBAL merged-list weights of the entries that belong to object k - the
 *     object's alpha matte under occlusion; sum_k visibility = the global opacity up to fp32 association.  Samples the overlap fix
 *     masked count for their object with weight 0.
 *   front_object (N,R): the lowest k whose visibility is the ray's maximum, -1 when no visibility is > 0 (a NaN is never greater).
 * Every fill is a kernel: the call can be recorded into a HIP graph.
 */
typedef struct pr_geometry_t {
    float* visibility;      /* (N,R,K) or NULL */
    int32_t* front_object;  /* (N,R) or NULL */
} pr_geometry_t;
int pr_render_geometry(const pr_call_t* call, const pr_object_t* objects, const pr_occupancy_t* occupancy,
                       const pr_fine_guide_t* guide, const pr_outputs_t* coarse, const pr_outputs_t* fine,
                       const pr_geometry_t* geometry_coarse, const pr_geometry_t* geometry_fine,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * Builds occupancy bits from a density lattice: sigma (groups, cells[0] * s, cells[1] * s, cells[2] * s) with supersample factor
 * s >= 1.  A cell is occupied iff any of its s^3 lattice values is > threshold; the occupied set is then grown by `dilate` >= 0
 * cells over the full (2 dilate + 1)^3 neighbourhood, clipped at the box.  bits (groups, ceil(cells[0] * cells[1] * cells[2] / 32)):
 * every word is written (tail bits 0) by ONE kernel launch - no memset, capturable into a HIP graph.
 */
int pr_occupancy_build(const float* sigma, int32_t groups, const int32_t* cells /* host, 3 */, int32_t supersample,
                       float threshold, int32_t dilate, uint32_t* bits, void* stream);

/*
 * Triangle meshes of density lattices: marching tetrahedra on the Freudenthal (Kuhn) split of every lattice cube - indexed,
 * watertight inside the lattice, consistently oriented (triangle normals point from matter to empty space).
 *   Lattice: sigma (G, nx, ny, nz), z fastest; point (i, j, k) sits at (axis[0][i], axis[1][j], axis[2][k]) - rectilinear, shared by
 *     the groups, never computed with.  A point is INSIDE iff sigma > level (a NaN is never inside; a value equal to level is outside).
 *   Edges: seven directions d = 0..6 leave a point: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).  An edge whose far end is
 *     on the lattice CROSSES when exactly one end is inside; it then carries one vertex, from its lower end a and far end b in fp32
 *     without contraction: t = (level - s_a) / (s_b - s_a); t = 0 unless t >= 0; t = 1 if t > 1; v = p_a + t (p_b - p_a) per axis.
 *   Normals (optional): g = lattice gradient, per axis (s[i+1] - s[i-1]) / (x[i+1] - x[i-1]), one-sided at the two ends;
 *     n = -(g_a + t (g_b - g_a)) divided by its fp32 length sqrt((n0 n0 + n1 n1) + n2 n2); (0,0,0) when the length is 0 or not finite.
 *   Tetrahedra: six per cube, one per axis permutation p in lexicographic order, corners v0 = 0, v1 = e_p0, v2 = v1 + e_p1,
 *     v3 = (1,1,1).  One corner alone on its side: one triangle; two and two: a quad as two triangles; orientation fixed per case.
 *   Order: vertices by group, flat index of the lower end (i ny + j) nz + k, d; triangles by group, flat index of the cube origin,
 *     tetrahedron, triangle of the case; indices are LOCAL to the group's vertex slice.
 *   Degenerate on purpose: where lattice values equal `level` the vertices of several edges coincide and some triangles have zero
 *     area; they are kept (the mesh stays topologically closed).  A surface that reaches the lattice border is open there.
 * An element at or beyond its capacity is not written; the offsets always hold the true totals.  With vertices, normals and
 * triangles all NULL the call only counts.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with P = nx ny nz and B = ceil(P / 256):
 *   G P (crossing masks) + G P (triangle counts) + 4 G P (vertex bases) + 4 x 4 G B (block sums and their scans) + 8 (totals).
 * Five kernel launches on `stream` (three when counting), no memset, no memcpy, no allocation, no synchronisation: capturable
 * into a HIP graph.
 */
typedef struct pr_surface_t {
    int32_t groups;              /* G >= 1 */
    int32_t points[3];           /* lattice points per axis, each >= 2 */
    float level;                 /* inside iff sigma > level; NaN refused */
    uint32_t flags;              /* 0 */
    const float* sigma;          /* (G, nx, ny, nz) */
    const float* axis[3];        /* (nx) (ny) (nz) coordinates, shared by the groups */
    int32_t max_vertices;        /* rows of vertices / normals, >= 0 */
    int32_t max_triangles;       /* rows of triangles, >= 0 */
    float* vertices;             /* (max_vertices, 3) or NULL */
    float* normals;              /* (max_vertices, 3) or NULL; needs vertices */
    int32_t* triangles;          /* (max_triangles, 3) or NULL; indices local to the group */
    int32_t* vertex_offsets;     /* (G + 1), always written: group g owns [off[g], off[g+1]) */
    int32_t* triangle_offsets;   /* (G + 1), always written */
} pr_surface_t;
/* Host computation, no device work.  12 G nx ny nz must stay below 2^31 (the counts are int32). */
int pr_surface_workspace_size(const pr_surface_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_surface_workspace_size bytes. */
int pr_extract_surface(const pr_surface_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Connected components of density lattices: labels, sizes, and a lattice with the unwanted components blanked out - floater removal
 * and capping in front of pr_extract_surface and pr_occupancy_build.
 *   Lattice: sigma (G, nx, ny, nz), z fastest, each extent >= 1; the flat index of a point inside its group is p = (i ny + j) nz + k.
 *   Inside: a point is INSIDE iff sigma > level - the comparison of pr_extract_surface and pr_occupancy_build (a NaN is never inside;
 *     a value equal to level is outside).  With PR_COMPONENTS_CLOSE_BORDER a point with any index equal to 0 or to its extent - 1 is
 *     outside, whatever its value.
 *   Connectivity: two inside points are adjacent iff they differ by plus or minus one of the seven edge directions of
 *     pr_extract_surface: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) - 14 neighbours, deliberately not symmetric under
 *     reflection: (0,0,0) and (1,1,0) are adjacent, (1,0,0) and (0,1,0) are not.  These are exactly the edges that carry mesh vertices:
 *     two points of different components never share a mesh edge, so removing a component removes its triangles and moves no vertex
 *     of any other component.
 *   Label: of an inside point the smallest flat index p of its component (local to the group), of an outside point -1: independent
 *     of the execution order.  Size: the number of points of the component.
 *   Selection: min_points >= 0 and keep_largest in [0, PR_COMPONENTS_MAX_KEEP], 0 = off.  The components of a group are ranked by
 *     size descending, ties by label ascending; a component is KEPT iff size >= min_points and (keep_largest == 0 or
 *     rank < keep_largest).  The cap of 8 is a design limit: every rank is one kernel launch, the cap bounds the launch count.
 *   Outputs - any pointer may be NULL except counts:
 *     labels (G, nx, ny, nz) int32;
 *     sizes (G, nx, ny, nz) int32: at every inside point the size of its component, 0 outside;
 *     sigma_out (G, nx, ny, nz): `fill` at every inside point of a component that is not kept and, with CLOSE_BORDER, at every border
 *       point whose value is > level; everywhere else the input value bit for bit (NaN payloads included).  sigma_out == sigma (in
 *       place) is allowed, a partial overlap is refused.  fill <= level is required (a NaN fill is refused);
 *     counts (G, 4) int32, always written: inside points, components, kept components, kept points.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with P = nx ny nz:
 *   4 G P (parents, then labels) + 4 G P (sizes) + 64 G (the keys of the eight largest components).
 * 4 + keep_largest kernel launches on `stream` (initialise, merge, flatten and measure, one selection pass per rank, write), no memset,
 * no memcpy, no allocation, no synchronisation: capturable into a HIP graph.  Integer atomics only: the outputs are deterministic.
 * No kernel ever waits for the progress of another lane (csrc/components.hip, TERMINATION).
 * Refused (PR_ERR_INVALID, before any device work): NULL sigma or counts, groups < 1, an extent < 1, a NaN level, unknown flag bits,
 * keep_largest outside [0, 8], min_points < 0, with sigma_out a NaN fill or fill > level or a partial overlap with sigma,
 * G nx ny nz >= 2^31, a misaligned or too small workspace.
 */
#define PR_COMPONENTS_CLOSE_BORDER 1u
#define PR_COMPONENTS_MAX_KEEP 8
typedef struct pr_components_t {
    int32_t groups;              /* G >= 1 */
    int32_t points[3];           /* lattice points per axis, each >= 1 */
    float level;                 /* inside iff sigma > level; NaN refused */
    uint32_t flags;              /* PR_COMPONENTS_CLOSE_BORDER or 0 */
    int32_t min_points;          /* >= 0; 0 = off */
    int32_t keep_largest;        /* 0 .. PR_COMPONENTS_MAX_KEEP; 0 = off */
    float fill;                  /* written to blanked points of sigma_out; <= level */
    uint32_t reserved_;
    const float* sigma;          /* (G, nx, ny, nz) */
    int32_t* labels;             /* (G, nx, ny, nz) or NULL */
    int32_t* sizes;              /* (G, nx, ny, nz) or NULL */
    float* sigma_out;            /* (G, nx, ny, nz) or NULL; may be sigma itself */
    int32_t* counts;             /* (G, 4), always written */
} pr_components_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_components_workspace_size(const pr_components_t* c, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_components_workspace_size bytes. */
int pr_label_components(const pr_components_t* c, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Density lattices evaluated only in a band around the level set: the front end (pr_band_plan) and the back end (pr_band_fill) around
 * a field evaluation that stays the caller's.  An opt-in approximation: the field is evaluated at a coarse SKELETON of the lattice and
 * then only where a skeleton cell saw the level set; a feature thinner than the stride that no skeleton cell sees as mixed is lost,
 * and `guard` does not bring it back.
 *   Lattice: sigma (G, nx, ny, nz), z fastest, every extent >= 2; point (i, j, k) sits at (axis[0][i], axis[1][j], axis[2][k]) -
 *     rectilinear, shared by the groups, never computed with.  The flat index of a point inside its group is p = (i ny + j) nz + k.  A
 *     point is INSIDE iff sigma > level (a NaN is never inside; a value equal to level is outside).
 *   Skeleton: stride r in [PR_BAND_MIN_STRIDE, PR_BAND_MAX_STRIDE].  Along an axis of n points the skeleton indices are 0, r, 2r, ...
 *     below n, plus n - 1 if it is not among them (the last cell may be shorter).  A SKELETON POINT has all three indices in these
 *     sets.  A CELL is the box between two consecutive skeleton indices on every axis, closed; there are (cx, cy, cz) cells,
 *     c = ceil((n - 1) / r) per axis, cell (a, b, c) has the flat index (a cy + b) cz + c.  On entry the lattice holds the field's value
 *     at every skeleton point; every other entry is ignored.
 *   Active cells: a cell is MIXED iff at least one of its 8 corner skeleton values is inside and at least one is not.  A cell is ACTIVE
 *     iff some cell within Chebyshev distance `guard` (in [0, PR_BAND_MAX_GUARD], clipped at the cell grid) is mixed.
 *   Band: a point belongs to the BAND iff it is not a skeleton point and at least one cell that contains it is active (a point on
 *     cell faces belongs to up to 8 cells).  The band points are listed by group, then by ascending flat index: the order does not
 *     depend on the execution.
 * pr_band_plan writes point_offsets (G + 1) - group g owns the rows [off[g], off[g+1]) - and counts (G, 4) = cells, mixed cells,
 *   active cells, band points; always.  Optionally: active (G, cx, cy, cz) bytes (1 = active), point_index (the flat index in the group
 *   of every band point) and positions (rows, 3), read from the axes without arithmetic, up to max_points rows: an element at or beyond
 *   the capacity is not written, the offsets always hold the true totals.  With active, point_index and positions all NULL the call only
 *   counts.  values and exact are not looked at.
 * pr_band_fill takes the same description, the same workspace - untouched since the plan call - and values (max_points): the field at
 *   the listed points, row by row.  It writes values to their lattice entries; every remaining non-skeleton point receives the bits
 *   of the skeleton value at the lower corner of the lowest-indexed cell that contains it - a copy, never arithmetic (NaN payloads
 *   included).  Such a point lies in unmixed cells only, so the copy is on the side of `level` that all of its cells agree on.
 *   Skeleton entries are never written.  Optionally exact (G, nx, ny, nz) bytes: 1 at skeleton and band points, 0 at filled ones.
 *   active, point_index and positions are not looked at.  The number of band points lives on the device: the host cannot compare it
 *   with max_points, which must be at least point_offsets[G].  values is never read at or beyond max_points; a band point whose row
 *   is not there is filled like a point outside the band (exact 0).
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with P = nx ny nz, B = ceil(P / 256), C = cx cy cz and
 *   D = ceil(C / 256):  G C (mixed cells) + G C (active cells) + 2 x 4 G D (block sums of both) + 2 x 4 G B (block sums of the band
 *   points and their scan) + 4 (the total).
 * pr_band_plan: six kernel launches on `stream` (five when point_index and positions are NULL); pr_band_fill: one.  No memset, no
 * memcpy, no allocation, no synchronisation: capturable into a HIP graph.  No atomics: the outputs are deterministic.
 * Refused (PR_ERR_INVALID, before any device work; by pr_band_workspace_size too, except the workspace itself): NULL sigma, axis,
 * point_offsets or counts, groups < 1, an extent < 2, stride or guard out of range, a NaN level, non-zero flags, a negative max_points,
 * G nx ny nz >= 2^31, a NULL, misaligned or too small workspace; by pr_band_fill NULL values with max_points > 0.
 */
#define PR_BAND_MIN_STRIDE 2
#define PR_BAND_MAX_STRIDE 64
#define PR_BAND_MAX_GUARD 8
typedef struct pr_band_t {
    int32_t groups;              /* G >= 1 */
    int32_t points[3];           /* lattice points per axis, each >= 2 */
    float level;                 /* inside iff sigma > level; NaN refused */
    uint32_t flags;              /* 0 */
    int32_t stride;              /* PR_BAND_MIN_STRIDE .. PR_BAND_MAX_STRIDE */
    int32_t guard;               /* 0 .. PR_BAND_MAX_GUARD */
    int32_t max_points;          /* rows of point_index / positions (plan) or of values (fill), >= 0 */
    uint32_t reserved_;
    float* sigma;                /* (G, nx, ny, nz): read at the skeleton points; written by pr_band_fill everywhere else */
    const float* axis[3];        /* (nx) (ny) (nz) coordinates, shared by the groups */
    const float* values;         /* fill: (max_points) the field at the listed points; NULL only with max_points == 0 */
    int32_t* point_offsets;      /* plan: (G + 1), always written */
    int32_t* counts;             /* plan: (G, 4), always written */
    uint8_t* active;             /* plan: (G, cx, cy, cz) or NULL */
    int32_t* point_index;        /* plan: (max_points) or NULL */
    float* positions;            /* plan: (max_points, 3) or NULL */
    uint8_t* exact;              /* fill: (G, nx, ny, nz) or NULL */
} pr_band_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_band_workspace_size(const pr_band_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_band_workspace_size bytes. */
int pr_band_plan(const pr_band_t* s, void* workspace, size_t workspace_bytes, void* stream);
int pr_band_fill(const pr_band_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Simplification of extracted meshes by vertex clustering on a uniform grid (Rossignac-Borrel): every vertex goes to the grid cell
 * that contains it, a cell's vertices become one vertex at their mean, triangles that lose a corner that way or repeat another one
 * disappear.  Integer accumulation throughout: the result does not depend on the execution order.
 *   Input: G meshes packed as pr_extract_surface leaves them - vertices (V, 3) fp32, optional normals (V, 3), triangles (T, 3) int32
 *     LOCAL to their group, vertex_offsets (G + 1), triangle_offsets (G + 1), all on the device; group g owns the rows
 *     [off[g], off[g+1]) and has V_g = off[g+1] - off[g] vertices.  total_vertices / total_triangles are V and T as host values
 *     (vertex_offsets[G], triangle_offsets[G]): the host sizes the launches and the workspace with them; offsets that leave
 *     [0, V] / [0, T] or decrease are clamped, never followed out of the arrays.
 *   Grid: origin[3], cell[3] (finite, > 0), cells[3] (each >= 1, product <= PR_SIMPLIFY_MAX_CELLS = 2^21), shared by the groups.
 *   Cell of a vertex, per axis in fp32 without contraction: q = (v - origin) / cell; q = 0 unless q >= 0 (NaN and negatives);
 *     q = (float)cells if q > (float)cells; c = min((int)q, cells - 1); w = q - (float)c, in [0, 1]; f = (int64)(w 2^20) - the product
 *     is exact, then truncated.  Flat cell index (c0 cells[1] + c1) cells[2] + c2.  Every vertex of a group's slice is clustered,
 *     whether or not a triangle refers to it.
 *   Cluster sums, per (group, cell): the member count n and the three int64 sums F of f.
 *   Output vertices: one per occupied cell, ordered by group, then flat cell index.  Position per axis in fp64 without contraction,
 *     then rounded to fp32: (double)origin + ((double)c + (double)F / ((double)n 1048576.0)) (double)cell - the mean of the members
 *     up to the 2^-20-of-a-cell quantisation.
 *   Output normals (optional; they need input normals): a component x of a member normal contributes llrint(x 2^20) if |x| <= 4,
 *     else 0 (a NaN contributes 0).  With S the three int64 sums as doubles, len = sqrt((S0 S0 + S1 S1) + S2 S2); the normal is
 *     (float)(S / len), and (0,0,0) when len == 0.
 *   Triangles: one with an index outside [0, V_g) is dropped and counted.  Each corner is replaced by its cluster's output index, local
 *     to the group; a triangle with two equal corners is dropped (degenerate).  The rest are rotated cyclically so that the smallest
 *     index comes first - the orientation is kept.  Among triangles with the same rotated triple only the one with the lowest input
 *     index survives; with PR_SIMPLIFY_KEEP_DUPLICATES all of them do.  (a,b,c) and (a,c,b) are not duplicates of each other: both
 *     stay.  Output order is input order.  Output vertices that no surviving triangle refers to are kept.
 *   Other outputs: vertex_map (V) int32, optional: the output index of every input vertex, local to its group.  counts (G, 4) int32,
 *     always written: clusters, non-degenerate triangles, output triangles, triangles dropped for an index out of range.
 *     out_vertex_offsets / out_triangle_offsets (G + 1), always written with the true totals.
 * An element at or beyond its capacity is not written.  With out_vertices, out_normals, out_triangles and vertex_map all NULL the call
 * only counts.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with C = cells[0] cells[1] cells[2], D = ceil(C / 256),
 *   BV = ceil(V / 256) + G and BT = ceil(T / 256) + G (upper bounds of the blocks of 256 vertices / triangles, none across two groups):
 *   4 G C (member counts, then output indices) + 24 G C (position sums) + 24 G C (normal sums; 0 without input normals) +
 *   4 V (cell, then output index of every vertex) + 4 T (table slot of every triangle) + 16 T (table keys, 2 T slots) +
 *   8 T (table minima) + 4 x 4 (G + 1) (per group: first vertex, first triangle, first vertex block, first triangle block) +
 *   2 x 4 G D (block sums of the occupied cells and their scan) + 2 x 4 BT (block sums of the surviving triangles and their scan) +
 *   8 (the totals).
 * Twelve kernel launches on `stream` (eleven when counting), no memset, no memcpy, no allocation, no synchronisation: capturable into
 * a HIP graph.  Integer atomics only.  The duplicate table's layout depends on the order of arrival, its minima - the result - do not.
 * Refused (PR_ERR_INVALID, before any device work; by pr_simplify_workspace_size too, except the workspace itself): NULL vertices,
 * triangles, offsets (in or out) or counts, groups < 1, a cells entry < 1 or a product above 2^21, a cell size that is not finite or
 * not > 0, a non-finite origin, unknown flag bits, a negative capacity or total, out_normals without normals or without out_vertices,
 * totals so large that an int32 count or the workspace sum overflows (V + 256 G or 2 T + 256 G at or above 2^31, a workspace of
 * 2^62 bytes or more), a NULL, misaligned or too small workspace.
 */
#define PR_SIMPLIFY_KEEP_DUPLICATES 1u
#define PR_SIMPLIFY_MAX_CELLS 2097152
typedef struct pr_simplify_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V = vertex_offsets[G], as a host value, >= 0 */
    int32_t total_triangles;              /* T = triangle_offsets[G], as a host value, >= 0 */
    uint32_t flags;                       /* PR_SIMPLIFY_KEEP_DUPLICATES or 0 */
    float origin[3];                      /* finite */
    float cell[3];                        /* finite, > 0 */
    int32_t cells[3];                     /* each >= 1, product <= PR_SIMPLIFY_MAX_CELLS */
    int32_t max_vertices;                 /* rows of out_vertices / out_normals, >= 0 */
    int32_t max_triangles;                /* rows of out_triangles, >= 0 */
    uint32_t reserved_;
    const float* vertices;                /* (V, 3) */
    const float* normals;                 /* (V, 3) or NULL */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    float* out_vertices;                  /* (max_vertices, 3) or NULL */
    float* out_normals;                   /* (max_vertices, 3) or NULL; needs normals and out_vertices */
    int32_t* out_triangles;               /* (max_triangles, 3) or NULL; indices local to the group */
    int32_t* vertex_map;                  /* (V) or NULL */
    int32_t* counts;                      /* (G, 4), always written */
    int32_t* out_vertex_offsets;          /* (G + 1), always written */
    int32_t* out_triangle_offsets;        /* (G + 1), always written */
} pr_simplify_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_simplify_workspace_size(const pr_simplify_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_simplify_workspace_size bytes. */
int pr_simplify_mesh(const pr_simplify_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Closest-hit ray queries against packed meshes: pr_raycast_build sorts the triangles of G meshes into a uniform cell grid,
 * pr_raycast_query casts N rays per group through it.  The result is DEFINED as that of the exhaustive search below; the grid may
 * change the time and never the bits (inside the domain stated under "Guarantee").
 *   Mesh input, read as pr_simplify_mesh reads it: vertices (V, 3) fp32, triangles (T, 3) int32 LOCAL to their group, vertex_offsets
 *     (G + 1), triangle_offsets (G + 1), all on the device; total_vertices / total_triangles are V and T as host values; offsets that
 *     leave [0, V] / [0, T] or decrease are clamped, never followed.  A triangle with an index outside [0, V_g) is never hit.
 *   Rays: origins (G, N, 3) and directions (G, N, 3) fp32 in the meshes' frame, not normalised; t_min, t_max: two fp32 per call, not
 *     NaN, +-inf allowed.
 *   The test of one ray (o, d) against one triangle (a, b, c): fp32, no contraction, dot products as (x0 y0 + x1 y1) + x2 y2, cross
 *     products componentwise ((x cross y)_0 = x1 y2 - x2 y1, cyclic):
 *       e1 = b - a, e2 = c - a, p = d cross e2, det = e1 . p, s = o - a,
 *       u = (s . p) / det, q = s cross e1, v = (d . q) / det, t = (e2 . q) / det.
 *     Accepted iff det < 0 or det > 0 (with PR_RAYCAST_CULL_BACK: det > 0 - the ray enters matter; the mesher orients triangles from
 *     matter to empty space), and u >= 0, v >= 0, u + v <= 1, t >= t_min, t <= t_max.  Every comparison is false on a NaN: a NaN or
 *     zero direction, a NaN origin, or a triangle with a == b or a == c never hits.
 *   Result per ray: among the accepted triangles of the ray's own group, the one with the smallest t, and among equal t (as numbers)
 *     the one with the lowest index.  Outputs: t (G, N) fp32, +inf for a miss; triangle (G, N) int32 local to the group, -1 for a
 *     miss, optional; barycentric (G, N, 2) = (u, v), zeros for a miss, optional (needs triangle).
 *   NOT WATERTIGHT: a ray through a shared edge or vertex can be accepted by both neighbours (then the lower index wins) or by neither.
 *   Grid: origin[3], cell[3] (finite, > 0), cells[3] (each 1 .. PR_RAYCAST_MAX_AXIS_CELLS = 1024, product <= PR_RAYCAST_MAX_CELLS =
 *     2^21), shared by the groups.  Grid coordinate of x on axis k: (x_k - origin_k) / cell_k in fp32; cell (i0, i1, i2) is the cube
 *     [i, i + 1] of grid coordinates and has the flat index (i0 cells[1] + i1) cells[2] + i2.
 *   Lists: every group has C + 1 of them, C = cells[0] cells[1] cells[2]: one per cell and, last (list C), the LOOSE list, which
 *     every ray of the group tests.  A triangle is
 *       dead  (in no list) iff it has an index outside [0, V_g), or a == b or a == c as values (det is then exactly zero);
 *       tight iff n = e1 cross e2 has n . n > 2^-20 ((e1 . e1) (e2 . e2)) and on every axis its three grid coordinates are finite
 *             and low = min - 1/16 >= 0, high = max + 1/16 <= cells_k; it is then in the list of every cell with
 *             (int)low <= i_k <= min((int)high, cells_k - 1) on all three axes - the box padded by a sixteenth of a cell;
 *       loose otherwise (a vertex that is not finite, a sliver, a padded box that is not inside the grid's box).
 *     A triangle may overlap any number of cells, at the price of a serial loop in its lane.
 *   Build outputs, caller-owned: cell_offsets (G (C + 1) + 1) int32, always written - list l of group g owns references
 *     [cell_offsets[g (C + 1) + l], cell_offsets[g (C + 1) + l + 1]), and the last element is R, the number of references;
 *     references (max_references) int32 or NULL: triangle indices local to the group.  The order inside a list is the order of arrival
 *     and differs from run to run; the query's result does not, because it takes a minimum.  R is only known on the device: a call
 *     with references == NULL only counts, one read-back of cell_offsets[G (C + 1)] follows, then an exactly sized emitting call.
 *     Nothing at or beyond max_references is written.  R must stay below 2^31.  A built grid serves any number of queries.
 *   Query: one lane per ray.  A ray with a component that is not finite or with d = 0 is a miss.  Otherwise the lane tests the loose
 *     list, clips [t_min, t_max] to the grid's box in grid coordinates (og = (o - origin) / cell, dg = d / cell; an axis with
 *     dg = 0 only checks 0 <= og <= cells), starts in the cell of og + t dg at the clipped start, and walks: the exit time of the
 *     current cell is the smallest (plane - og_k) / dg_k over the axes with dg_k != 0, plane = i_k + 1 for dg_k > 0 and i_k otherwise;
 *     it tests the cell's list, stops if the best t so far is <= the exit time or the exit time is >= the clipped end, and otherwise
 *     steps along that axis, stopping when it leaves the grid.  At most cells[0] + cells[1] + cells[2] steps; no lane waits for another.
 *     References outside [0, max_references) or [0, T_g) are skipped: a stale or foreign grid costs correctness, never memory safety.
 *   Guarantee (argument: DESIGN.md 21.2): the outputs equal the exhaustive search bit for bit if (1) the ray's origin lies within
 *     2^12 cells of the grid's origin on every axis and the clip times are finite, and (2) every test of a TIGHT triangle that the
 *     exhaustive search accepts is well conditioned: with L = max(|o - a|, |e1|, |e2|) and rho = |det| / (|e1| |e2| |d|) (Euclidean),
 *     rho >= 2^-16 and L / rho <= 2^12 min(cell).  Loose triangles need no condition.  Outside this domain the call is memory-safe and
 *     terminates, and a hit it reports is a hit of the rule - but a closer one may have been missed.
 * pr_raycast_workspace_size / pr_raycast_build workspace bytes = the sum of these regions, each rounded up to 256 bytes, with
 *   NB = floor(G (C + 1) / 256) + 1: 4 G (C + 1) (list counts, then cursors) + 3 x 4 (G + 1) (per group: first vertex, first triangle,
 *   first triangle block) + 2 x 4 NB (block sums of the counts and their scan) + 4 (the total).  The query needs no workspace.
 * Kernels only on `stream` (six for a counting build, seven for an emitting one, one for a query): no memset, no memcpy, no allocation,
 * no synchronisation - build and query are each capturable into a HIP graph.  Integer atomics only.
 * Refused (PR_ERR_INVALID, before any device work, by all three entry points): NULL vertices, triangles, offsets or cell_offsets,
 * groups < 1, a cells entry outside 1 .. 1024 or a product above 2^21, a cell size that is not finite or not > 0, a non-finite origin,
 * unknown flag bits, a negative total, capacity or ray count, a NaN t_min or t_max, totals at which an int32 count overflows
 * (T + 256 G, G (C + 1) + 256 or G (N + 256) at or above 2^31); by the build a NULL, misaligned or too small workspace; by the query a
 * NULL t, barycentric without triangle, NULL origins or directions, NULL references with max_references > 0.  rays == 0 and
 * total_triangles == 0 are valid: nothing is launched, or every ray misses.
 */
#define PR_RAYCAST_CULL_BACK 1u
#define PR_RAYCAST_MAX_AXIS_CELLS 1024
#define PR_RAYCAST_MAX_CELLS 2097152
typedef struct pr_raycast_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V = vertex_offsets[G], as a host value, >= 0 */
    int32_t total_triangles;              /* T = triangle_offsets[G], as a host value, >= 0 */
    uint32_t flags;                       /* PR_RAYCAST_CULL_BACK or 0 (read by the query) */
    float origin[3];                      /* finite */
    float cell[3];                        /* finite, > 0 */
    int32_t cells[3];                     /* each 1 .. PR_RAYCAST_MAX_AXIS_CELLS, product <= PR_RAYCAST_MAX_CELLS */
    int32_t max_references;               /* rows of references, >= 0 */
    int32_t rays;                         /* N per group, >= 0 (query) */
    float t_min;                          /* not NaN (query) */
    float t_max;                          /* not NaN (query) */
    uint32_t reserved_;
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    int32_t* cell_offsets;                /* (G (C + 1) + 1): written by the build, read by the query */
    int32_t* references;                  /* (max_references): written by the build (NULL: count only), read by the query */
    const float* origins;                 /* query: (G, N, 3) */
    const float* directions;              /* query: (G, N, 3) */
    float* t;                             /* query: (G, N), always written */
    int32_t* triangle;                    /* query: (G, N) or NULL */
    float* barycentric;                   /* query: (G, N, 2) or NULL; needs triangle */
} pr_raycast_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_raycast_workspace_size(const pr_raycast_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_raycast_workspace_size bytes. */
int pr_raycast_build(const pr_raycast_t* s, void* workspace, size_t workspace_bytes, void* stream);
int pr_raycast_query(const pr_raycast_t* s, void* stream);

/*
 * Closest-point queries against packed meshes on the grid of pr_raycast_build: pr_closest_query finds, for N points per group, the
 * closest point of the group's mesh within max_distance.  It reads the mesh, the grid and the lists (cell_offsets, references) that a
 * finished EMITTING pr_raycast_build left with the caller, and builds nothing of its own.  The result is DEFINED as that of the
 * exhaustive search below; the grid may change the time and never the bits (inside the domain stated under "Guarantee").
 *   Mesh and grid input: as pr_raycast_t (same fields, same clamping of offsets, same grid coordinates and lists).
 *   Points: points (G, N, 3) fp32 in the meshes' frame, N = count; max_distance: one fp32 per call, not NaN, >= 0, +inf allowed.
 *   Candidates of a point of group g: the triangles of group g that pr_raycast_build does not classify as dead.  DEAD triangles - an
 *     index outside [0, V_g), or a == b or a == c as values - are in no list and are no candidates here either (they are segments or
 *     points; where the mesher emits them its neighbouring triangles cover their edges).
 *   The closest point q of one triangle (a, b, c) to p is Ericson's region walk: fp32, no contraction, every operation rounded on its
 *     own, dot products as (x0 y0 + x1 y1) + x2 y2:
 *       ab = b - a, ac = c - a, bc = c - b, ap = p - a, bp = p - b, cp = p - c,
 *       d1 = ab . ap, d2 = ac . ap, d3 = ab . bp, d4 = ac . bp, d5 = ab . cp, d6 = ac . cp,
 *       vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.
 *     The first condition that holds, in this order, decides (every comparison is false on a NaN, which ends in the last line):
 *       vertex a   d1 <= 0 and d2 <= 0                            (v, w) = (0, 0)                       q = a (copied)
 *       vertex b   d3 >= 0 and d4 <= d3                           (v, w) = (1, 0)                       q = b (copied)
 *       edge ab    vc <= 0 and d1 >= 0 and d3 <= 0                v = d1 / (d1 - d3), w = 0             q = a + v ab
 *       vertex c   d6 >= 0 and d5 <= d6                           (v, w) = (0, 1)                       q = c (copied)
 *       edge ac    vb <= 0 and d2 >= 0 and d6 <= 0                v = 0, w = d2 / (d2 - d6)             q = a + w ac
 *       edge bc    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0      w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
 *                                                                                                       q = b + w bc
 *       interior   otherwise                                      v = vb / ((va + vb) + vc), w = vc / ((va + vb) + vc), then clamped:
 *                                                                 v = 0 unless v >= 0, v = 1 if v > 1, w = 0 unless w >= 0,
 *                                                                 w = 1 - v if w > 1 - v              q = (a + v ab) + w ac
 *     componentwise, each product and sum rounded.  In every line 0 <= v, w and v + w <= 1 up to one rounding: q is a point of the
 *     triangle whatever region the rounded conditions chose (a wrong region costs optimality, never membership).
 *     r = p - q, dist2 = r . r.  Accepted iff dist2 <= max_distance * max_distance (one fp32 product) and dist2 < +inf.  A point with a component that is not finite is accepted by nothing (r is then infinite or
 *     NaN): it is a miss, and nothing is tested for it.
 *   Result per point: among the accepted candidates of the point's own group, the one with the smallest dist2, and among equal dist2
 *     (as numbers) the one with the lowest index - a point whose closest feature is a shared vertex gets bit-equal dist2 from every
 *     triangle around it, because q is a copy.  Outputs: distance (G, N) fp32 = sqrt(dist2) correctly rounded, +inf for a miss, always
 *     written; triangle (G, N) int32 local to the group, -1 for a miss, optional; point (G, N, 3) = q, zeros for a miss, optional
 *     (needs triangle); barycentric (G, N, 2) = (v, w), with q = a + v (b - a) + w (c - a) up to rounding, zeros for a miss, optional
 *     (needs triangle).
 *   Query: one lane per point.  The lane tests the group's loose list.  If the group has a reference outside its loose list, it takes
 *     the start cell s_k = the integer part of (p_k - origin_k) / cell_k (fp32), clamped into [0, cells_k - 1], and visits the grid's
 *     cells shell by shell: shell r = 0, 1, ... holds the cells inside the grid at Chebyshev index distance exactly r from s.  It tests
 *     the list of every cell of the shell and then stops if, with reach2 = (r cmin) (r cmin) in fp32 (r as fp32, cmin = the smallest
 *     cell[k]; two products),
 *       a candidate was accepted and the best dist2 <= reach2,  or  reach2 > max_distance * max_distance,  or
 *       r = max_k max(s_k, cells_k - 1 - s_k) (no shell is left).
 *     References outside [0, max_references) or [0, T_g), triangle indices outside [0, V_g) and dead triangles are skipped where they
 *     are read: a stale or foreign grid costs correctness, never memory safety.  A triangle listed in several cells is tested several
 *     times; a minimum is idempotent.  A wave runs as long as its slowest point.  With max_distance = +inf a point far from the mesh
 *     visits every shell up to its distance - (2 r + 1)^3 cells; give a finite radius where one is known.
 *   Guarantee (argument: DESIGN.md 22.2): the outputs equal the exhaustive search bit for bit if every coordinate of the point, of
 *     the grid's origin and of the grid's far corner origin + cells cell is at most 2^12 cmin in magnitude (so the point lies within
 *     2^13 cells of the grid's origin, and one fp32 ulp of any coordinate that occurs is at most 2^-11 of a cell), and cmin >= 2^-40
 *     (no squared distance of interest underflows).  There is no conditioning requirement: slivers are loose.  Outside this
 *     domain the call is memory-safe and terminates (the shell loop has the bound above), and a result it reports is an accepted
 *     candidate of the rule - but a closer one may have been missed.
 * One kernel on `stream`, no workspace: no memset, no memcpy, no allocation, no synchronisation, no atomics - capturable as a one-node
 * HIP graph.  sizeof(pr_closest_t) = 152.
 * Refused (PR_ERR_INVALID, before any device work): everything pr_raycast_query refuses about mesh, grid and capacities (NULL
 * vertices, triangles, offsets or cell_offsets, groups < 1, a cells entry outside 1 .. 1024 or a product above 2^21, a cell size that
 * is not finite or not > 0, a non-finite origin, a negative total, capacity or count, NULL references with max_references > 0, T + 256 G
 * or G (C + 1) + 256 at or above 2^31), a NULL distance or points, point or barycentric without triangle, a NaN or negative
 * max_distance, flags other than 0, G (N + 256) at or above 2^31.  count == 0 launches nothing; total_triangles == 0 makes every
 * point a miss.
 */
typedef struct pr_closest_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V = vertex_offsets[G], as a host value, >= 0 */
    int32_t total_triangles;              /* T = triangle_offsets[G], as a host value, >= 0 */
    uint32_t flags;                       /* no flag is defined: 0 */
    float origin[3];                      /* the grid of the build: finite */
    float cell[3];                        /* finite, > 0 */
    int32_t cells[3];                     /* each 1 .. PR_RAYCAST_MAX_AXIS_CELLS, product <= PR_RAYCAST_MAX_CELLS */
    int32_t max_references;               /* rows of references, >= 0 */
    int32_t count;                        /* N per group, >= 0 */
    float max_distance;                   /* not NaN, >= 0, +inf allowed */
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    const int32_t* cell_offsets;          /* (G (C + 1) + 1), as pr_raycast_build wrote them */
    const int32_t* references;            /* (max_references), as an emitting pr_raycast_build wrote them (NULL: max_references 0) */
    const float* points;                  /* (G, N, 3) */
    float* distance;                      /* (G, N), always written */
    int32_t* triangle;                    /* (G, N) or NULL */
    float* point;                         /* (G, N, 3) or NULL; needs triangle */
    float* barycentric;                   /* (G, N, 2) or NULL; needs triangle */
} pr_closest_t;
int pr_closest_query(const pr_closest_t* s, void* stream);

/*
 * Inside / outside queries against packed meshes on the grid of pr_raycast_build: pr_inside_query computes, for N points per group,
 * the winding number of the group's mesh around the point along one coordinate axis - the signed count of the triangles the ray from
 * the point in the +axis direction passes through.  It reads what pr_closest_query reads and builds nothing.  It is WATERTIGHT BY
 * CONSTRUCTION: every decision on which the topology depends is taken in exact arithmetic.  The result is DEFINED as that of the
 * exhaustive sum over all candidates below; the grid may change the time and never the bits - without any domain restriction.
 *   Mesh and grid input: as pr_closest_t (same fields, same clamping of offsets, same grid coordinates and lists, from a finished
 *     EMITTING pr_raycast_build).
 *   Points: points (G, N, 3) fp32 in the meshes' frame, N = count.  axis = k in {0, 1, 2}, one per call; i = (k + 1) mod 3,
 *     j = (k + 2) mod 3.
 *   Candidates of a point of group g: the triangles of group g that pr_raycast_build does not classify as dead (an index outside
 *     [0, V_g), or a == b or a == c as values) and whose nine coordinates are finite.
 *   Edge sign s(u, v) of a directed edge u -> v for the point p: the sign of the EXACT real value of
 *       E = (v_i - u_i) (p_j - u_j) - (v_j - u_j) (p_i - u_i)
 *     - every fp32 input is a rational, nothing is rounded.  If E = 0: the sign of u_j - v_j; if that is 0 too, the sign of
 *     v_i - u_i; if both are 0 (u and v project to one point), 0.  This is the symbolic perturbation p' = (p_i + eps, p_j + eps^2):
 *     s(u, v) = -s(v, u) exactly, and a perturbed point lies on no edge.
 *   Orientation of a candidate (a, b, c): o = s(a, b) if s(a, b) = s(b, c) = s(c, a) != 0, else 0.  Exact: of two triangles that
 *     share an edge by vertex values, with opposite directions, never both and never neither claim a point across that edge.
 *   A candidate with o != 0 is AHEAD of p iff max(a_k, b_k, c_k) > p_k (an exact fp32 comparison) and sign(S) = -o, where S is
 *     computed in float64, every fp32 converted first, no contraction, in this order:
 *       e1 = b - a, e2 = c - a, n = e1 cross e2 ((x cross y)_0 = x1 y2 - x2 y1, cyclic; each component one difference of two
 *       products), d = p - a, S = (n_0 d_0 + n_1 d_1) + n_2 d_2.       S = 0: not ahead.
 *   Result per point: winding (G, N) int32 = the sum of o over the ahead candidates of the point's own group, always written;
 *     crossings (G, N) int32 = their number, optional.  With the mesher's orientation (normals out of matter) a point inside a
 *     closed mesh gets +1.  A point with a component that is not finite gets 0 / 0 and tests nothing.
 *   What is guaranteed: the 2-D decisions are exact.  For a mesh in which every directed edge (by vertex VALUES) occurs as often
 *     as its reverse, the signed coverage of every point - the sum of o over ALL candidates - is 0, and the winding is a
 *     topological invariant up to the float64 ahead test, which can only err for a point within float64 rounding of a triangle's
 *     plane.  For such points - points ON the surface - the three axes may legitimately differ.  What is not: an open mesh (one
 *     that reaches the border of its lattice: cap it, PR_COMPONENTS_CLOSE_BORDER / close_border=True) and a mesh simplified with
 *     its duplicate triangles removed (keep them: PR_SIMPLIFY_KEEP_DUPLICATES / keep_duplicates=True) leave directed edges
 *     unpaired; they get the rule's result, which is then no statement about a solid.
 *   Query: one lane per point.  The lane tests the group's loose list with the rule.  With g_m = (p_m - origin_m) / cell_m in fp32
 *     (the build's two roundings) and the start cell s_m = (int)g_m: if g_i or g_j is outside [0, cells), or g_k >= cells_k, no tight
 *     triangle is tested.  Otherwise the lane visits the cells (s_i, s_j, m), m = max(s_k, 0) .. cells_k - 1, of its column, and a
 *     triangle found in the list of cell m is tested there iff m = max(lo_k, max(s_k, 0)), lo_k = (int)(min of its three grid
 *     coordinates on axis k - 1/16) recomputed with the build's own expression: a triangle listed in several cells of the column
 *     is summed once.  Nothing is missed (argument: DESIGN.md 23.2 - only the monotonicity of fp32 subtraction and division is
 *     used, and the first ahead condition, which rejects every triangle whose cells lie below the start cell).  Per candidate:
 *     exact fp32 rejections first (p_i < min_i, p_i > max_i, likewise on j, max_k <= p_k - closed intervals, the perturbation can
 *     move a boundary point in but never a strictly outside point), then per edge E in float64 with a forward error bound
 *     ((3 + 16 e) e (|left| + |right|), e = 2^-53), then - where the bound does not decide - the exact sign of the six products
 *     of the expanded determinant, each exact in a double, by an expansion sum of fifteen error-free additions.
 *     References outside [0, max_references) or [0, T_g) and triangle indices outside [0, V_g) are skipped where they are read,
 *     and the column loop is bounded by cells_k: a stale or foreign grid costs correctness, never memory safety.
 * One kernel on `stream`, no workspace: no memset, no memcpy, no allocation, no synchronisation, no atomics - capturable as a one-node
 * HIP graph.  Additive entry point: PR_ABI_VERSION is unchanged.  sizeof(pr_inside_t) = 136.
 * Refused (PR_ERR_INVALID, before any device work): everything pr_closest_query refuses about mesh, grid and capacities, NULL points
 * or winding, an axis outside 0 .. 2, flags other than 0, G (N + 256) at or above 2^31.  count == 0 launches nothing;
 * total_triangles == 0 gives zeros.
 */
typedef struct pr_inside_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V = vertex_offsets[G], as a host value, >= 0 */
    int32_t total_triangles;              /* T = triangle_offsets[G], as a host value, >= 0 */
    uint32_t flags;                       /* no flag is defined: 0 */
    float origin[3];                      /* the grid of the build: finite */
    float cell[3];                        /* finite, > 0 */
    int32_t cells[3];                     /* each 1 .. PR_RAYCAST_MAX_AXIS_CELLS, product <= PR_RAYCAST_MAX_CELLS */
    int32_t max_references;               /* rows of references, >= 0 */
    int32_t count;                        /* N per group, >= 0 */
    int32_t axis;                         /* k: 0, 1 or 2 - the ray runs from the point in the +k direction */
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    const int32_t* cell_offsets;          /* (G (C + 1) + 1), as pr_raycast_build wrote them */
    const int32_t* references;            /* (max_references), as an emitting pr_raycast_build wrote them (NULL: max_references 0) */
    const float* points;                  /* (G, N, 3) */
    int32_t* winding;                     /* (G, N), always written */
    int32_t* crossings;                   /* (G, N) or NULL */
} pr_inside_t;
int pr_inside_query(const pr_inside_t* s, void* stream);

/*
 * Audit of packed meshes: pr_mesh_audit says, per group, how a mesh is made up - whether its directed edges balance (what
 * pr_inside_query's guarantee asks of a mesh), its boundary and non-manifold edges, Euler characteristic, connected shells, area,
 * signed volume and centroid, and optionally the shell of every triangle.  It reads a mesh and changes nothing; there is no grid.
 *   Input: G meshes packed as pr_extract_surface / pr_simplify_mesh leave them - vertices (V, 3) fp32, triangles (T, 3) int32 LOCAL
 *     to their group, vertex_offsets (G + 1), triangle_offsets (G + 1), all on the device; total_vertices / total_triangles are V and
 *     T as host values.  Offsets that leave [0, V] / [0, T] or decrease are clamped as pr_simplify_mesh clamps them, never followed.
 *   Candidates: EXACTLY pr_inside_query's - a triangle (a, b, c) of group g whose three indices lie in [0, V_g), whose nine
 *     coordinates are finite, and with neither a == b nor a == c as values.  This is the one definition; pr_inside_query states the
 *     same.  Every other triangle of the group is DROPPED: it is counted and takes no further part.  (b == c is a candidate.)
 *   Vertex identity is by VALUE: two vertices of a group are the same iff their three fp32 components compare equal with ==, so -0
 *     equals +0.  (The mesher gives coinciding vertices where lattice values equal the level; identity by index would call such a
 *     mesh open although pr_inside_query treats it as closed.)  The representative of a class is its lowest vertex index.
 *   Edges: an undirected edge is a pair {r, s} of distinct representatives, r < s.  A candidate has the three sides a -> b, b -> c,
 *     c -> a; a side whose ends have one representative (possible only for b == c) is no edge and is skipped.  Per edge, f is the
 *     number of candidate sides that run r -> s and b the number that run s -> r.
 *   counts (G, 12) int32, always and fully written:
 *       [0] candidates F                    [1] dropped triangles
 *       [2] distinct vertices by value that a side of a candidate refers to, Vr       [3] undirected edges E
 *       [4] unbalanced edges, f != b        [5] boundary edges, f + b == 1            [6] non-manifold edges, f + b > 2
 *       [7] Euler characteristic Vr - E + F [8] shells                                [9] triangles of the largest shell
 *       [10], [11] reserved, 0
 *     "Every directed edge occurs as often as its reverse" holds exactly when counts[4] == 0; a closed oriented manifold - every
 *     directed edge once, its reverse once - also needs counts[5] == counts[6] == 0.
 *   Shells: two candidates are connected if they have a side on the same undirected edge; the shells are the classes of the
 *     transitive closure.  labels (T) int32, optional: for a candidate the lowest triangle index (local to the group) of its shell,
 *     -1 for a dropped triangle and for a row that no clamped group owns.  Neither the algorithm nor the order of arrival shows.
 *   measures (G, 8) fp64, optional: area, signed volume, the three components of the area-weighted centroid of the surface, three
 *     reserved zeros.  Per candidate, in fp64 with every fp32 converted first, no contraction, in this order:
 *       e1 = b - a, e2 = c - a, n = e1 cross e2 ((x cross y)_0 = x1 y2 - x2 y1, cyclic; a component is one difference of two products),
 *       area term    0.5 sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2),
 *       volume term  ((a_0 m_0 + a_1 m_1) + a_2 m_2) / 6 with m = b cross c,
 *       centroid term, per axis k   area (((a_k + b_k) + c_k) / 3).
 *     The sums are taken in a FIXED TREE, so that they are equal from run to run: triangle t of the group (local index) is lane
 *     t mod 256 of block t / 256, lanes without a candidate hold 0; in each of the block's four waves of 64 lanes, for d = 32, 16, 8,
 *     4, 2, 1 in turn lane i takes x_i + x_(i + d) (i + d < 64), and lane 0 then holds the wave's sum w; the block's partial is
 *     ((w_0 + w_1) + w_2) + w_3.  One block per group then sums the partials: its lane j adds, starting from 0, the partials of the
 *     blocks j, j + 256, j + 512, ... in that order, and the 256 lane sums go through the same tree.  The result lies within
 *     T_g 2^-52 sum|term| of the exact sum.  The centroid sums are divided by the area at the end; the centroid is 0 where the area
 *     is not > 0.  No floating-point atomic anywhere.
 *   T = 0 or an empty group gives zeros: its Euler characteristic and shell count are 0.
 *   Memory safety: every index read from the mesh or from a table is range-checked where it is read.  Hostile input may cost the
 *     correctness of the hostile group, never memory safety, and never another group's rows.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with BV = ceil(V / 256) + G and BT = ceil(T / 256) + G
 *   (upper bounds of the blocks of 256 vertices / triangles, none across two groups): 4 x 4 (G + 1) (per group:
 *   first vertex, first triangle, first vertex block, first triangle block) + 8 V (weld table, 2 V slots) + 4 V (representatives) +
 *   4 V (referenced flags) + 48 T (edge keys, 6 T slots) + 48 T (forward and backward counters) + 24 T (edge owners) + 12 T (the three
 *   slots of a triangle) + 4 T (union-find parents) + 4 T (shell sizes) + 40 BT (fp64 block partials) + 32 BT + 4 BV (integer block
 *   partials): 16 bytes per vertex, 140 per triangle.
 * Nine kernel launches on `stream` (eight without measures), no memset, no memcpy, no allocation, no synchronisation: capturable into
 * a HIP graph.  Integer atomics only.  The tables' layouts depend on the order of arrival; no output does.
 * Additive entry points: PR_ABI_VERSION is unchanged.  sizeof(pr_mesh_audit_t) = 72.
 * Refused (PR_ERR_INVALID, before any device work; by pr_mesh_audit_workspace_size too, except the workspace itself): NULL vertices,
 * triangles, offsets or counts, groups < 1, a negative total, flags other than 0 (no flag is defined), 2 V + 256 G or 6 T + 256 G at or
 * above 2^31 (the table slots are int32); by the call only: a NULL, misaligned or too small workspace.
 */
typedef struct pr_mesh_audit_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V = vertex_offsets[G], as a host value, >= 0 */
    int32_t total_triangles;              /* T = triangle_offsets[G], as a host value, >= 0 */
    uint32_t flags;                       /* no flag is defined: 0 */
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    int32_t* counts;                      /* (G, 12), always written */
    double* measures;                     /* (G, 8) or NULL */
    int32_t* labels;                      /* (T) or NULL */
} pr_mesh_audit_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_mesh_audit_workspace_size(const pr_mesh_audit_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_mesh_audit_workspace_size bytes. */
int pr_mesh_audit(const pr_mesh_audit_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Welding and compaction of packed meshes: pr_mesh_weld returns meshes in which identity by index IS identity by value, every vertex
 * is referenced and every triangle is a candidate of pr_mesh_audit - what an OBJ viewer, an adjacency builder or any other reader
 * that trusts indices needs of the meshes that pr_extract_surface, pr_simplify_mesh and Mesh.keep_shells leave.
 *   Input: G meshes packed as pr_extract_surface / pr_simplify_mesh leave them - vertices (V, 3) fp32, optional normals (V, 3) fp32,
 *     optional attributes (V, A) fp32 with attribute_width = A, triangles (T, 3) int32 LOCAL to their group, vertex_offsets (G + 1),
 *     triangle_offsets (G + 1), all on the device; total_vertices / total_triangles are V and T as host values.  Offsets that leave
 *     [0, V] / [0, T] or decrease are clamped as pr_simplify_mesh and pr_mesh_audit clamp them, never followed.
 *   Definitions: pr_mesh_audit's.  The CLASS of a finite vertex is the set of its group's vertices whose three fp32 components
 *     compare equal with == (so -0 equals +0); its REPRESENTATIVE is the lowest index of the class; a vertex with a component that is
 *     not finite has no class.  With the flag PR_WELD_COMPACT_ONLY every finite vertex is its own representative: nothing is merged
 *     and only dead rows go.  A KEPT triangle is exactly a candidate of pr_mesh_audit, in both modes: three indices in [0, V_g), nine
 *     finite coordinates, neither a == b nor a == c as VALUES (b == c stays kept, so that the output's audit equals the input's).
 *     Every other triangle of the group is dropped and counted.
 *   Output vertices: one per representative that at least one kept triangle refers to, ordered by group and then by the
 *     representative's index; the row is the representative's three fp32 words copied bit for bit.  out_normals / out_attributes hold
 *     the REPRESENTATIVE's rows copied bit for bit, NaNs included: there is NO averaging over a class - the rows of the other members
 *     are not read.
 *   Output triangles: the kept ones in input order, each corner replaced by the output index of its representative, local to the
 *     group.  No rotation.
 *   vertex_map (V) int32, optional: the output index (local) of the vertex's representative; -1 if the vertex is not finite or its
 *     representative is unreferenced.  triangle_map (T) int32, optional: the output index (local) of a kept triangle, -1 for a dropped
 *     one.  Rows of either map that no clamped group owns get -1, as labels in pr_mesh_audit.
 *   counts (G, 8) int32, always and fully written:
 *       [0] output vertices        [1] output triangles        [2] dropped triangles        [3] vertices that are not finite
 *       [4] finite vertices merged into a lower index (0 with PR_WELD_COMPACT_ONLY)
 *       [5] representatives that no kept triangle refers to    [6], [7] reserved, 0
 *     V_g = [0] + [3] + [4] + [5] for every group.  Without PR_WELD_COMPACT_ONLY, [0], [1], [2] equal pr_mesh_audit's counts[2], [0],
 *     [1] of the same input.
 *   out_vertex_offsets / out_triangle_offsets (G + 1), always written with the true totals.
 *   An element at or beyond its capacity (max_vertices rows of out_vertices / out_normals / out_attributes, max_triangles rows of
 *     out_triangles) is not written.  With out_vertices, out_normals, out_attributes, out_triangles, vertex_map and triangle_map all
 *     NULL the call only counts.
 *   Memory safety: every index read from the mesh or from a table is range-checked where it is read; rows that no clamped group owns
 *     are never touched apart from the -1 of the maps.  Hostile input may cost the correctness of the hostile group, never memory
 *     safety, and never another group's rows.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with BV = ceil(V / 256) + G and BT = ceil(T / 256) + G
 *   (upper bounds of the blocks of 256 vertices / triangles, none across two groups): 4 x 4 (G + 1) (per group: first vertex, first
 *   triangle, first vertex block, first triangle block) + 8 V (weld table, 2 V slots; reserved but unused with PR_WELD_COMPACT_ONLY) +
 *   4 V (representatives) + 4 V (referenced flags) + 4 V (output indices) + 4 T (kept flags) + 4 BV (vertex block sums) +
 *   4 (BV + 1) (their scan and the total) + 4 BT (triangle block sums) + 4 (BT + 1) (their scan and the total) + 12 BV (per vertex
 *   block: not finite, merged, unreferenced): 20 bytes per vertex, 4 per triangle.
 * Eight kernel launches on `stream` (seven with PR_WELD_COMPACT_ONLY), the same number whether the call emits or only counts; no
 * memset, no memcpy, no allocation, no synchronisation: capturable into a HIP graph.  Integer atomics only.  The table's layout
 * depends on the order of arrival; no output does: a second call gives equal bits everywhere.
 * Additive entry points: PR_ABI_VERSION is unchanged.  sizeof(pr_mesh_weld_t) = 152.
 * Refused (PR_ERR_INVALID, before any device work; by pr_mesh_weld_workspace_size too, except the workspace itself): NULL vertices,
 * triangles, offsets (in or out) or counts, groups < 1, a negative total or capacity, unknown flag bits, attribute_width < 0 or above
 * 4096, out_attributes without attributes or with attribute_width == 0, out_normals without normals, out_normals or out_attributes
 * without out_vertices, 2 V + 256 G or T + 256 G at or above 2^31 (the table slots and the block counts are int32; the workspace sum
 * then stays far below 2^62); by the call only, and last: a NULL, misaligned or too small workspace.
 */
#define PR_WELD_COMPACT_ONLY 1u
typedef struct pr_mesh_weld_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V = vertex_offsets[G], as a host value, >= 0 */
    int32_t total_triangles;              /* T = triangle_offsets[G], as a host value, >= 0 */
    uint32_t flags;                       /* PR_WELD_COMPACT_ONLY or 0 */
    int32_t attribute_width;              /* A, 0 .. 4096 */
    int32_t max_vertices;                 /* rows of out_vertices / out_normals / out_attributes, >= 0 */
    int32_t max_triangles;                /* rows of out_triangles, >= 0 */
    uint32_t reserved_;
    const float* vertices;                /* (V, 3) */
    const float* normals;                 /* (V, 3) or NULL */
    const float* attributes;              /* (V, A) or NULL */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    float* out_vertices;                  /* (max_vertices, 3) or NULL */
    float* out_normals;                   /* (max_vertices, 3) or NULL; needs normals and out_vertices */
    float* out_attributes;                /* (max_vertices, A) or NULL; needs attributes, A > 0 and out_vertices */
    int32_t* out_triangles;               /* (max_triangles, 3) or NULL; indices local to the group */
    int32_t* vertex_map;                  /* (V) or NULL */
    int32_t* triangle_map;                /* (T) or NULL */
    int32_t* counts;                      /* (G, 8), always written */
    int32_t* out_vertex_offsets;          /* (G + 1), always written */
    int32_t* out_triangle_offsets;        /* (G + 1), always written */
} pr_mesh_weld_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_mesh_weld_workspace_size(const pr_mesh_weld_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_mesh_weld_workspace_size bytes. */
int pr_mesh_weld(const pr_mesh_weld_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Smoothing of packed meshes: pr_mesh_smooth builds the vertex-to-triangle incidence lists, runs `steps` Laplacian / Taubin steps on
 * them and returns the positions, the area-weighted vertex normals of the result, the lists as a CSR, a state word per vertex and the
 * counts - the adjacency reader that pr_mesh_weld prepares meshes for.
 *   Input: G meshes packed as pr_mesh_weld leaves them - vertices (V, 3) fp32, triangles (T, 3) int32 LOCAL to their group,
 *     vertex_offsets (G + 1), triangle_offsets (G + 1), optional pinned (V) uint8, all on the device; total_vertices / total_triangles
 *     are V and T as host values.  Offsets that leave [0, V] / [0, T] or decrease are clamped as pr_mesh_weld clamps them, never
 *     followed.  Identity is by INDEX: the call is meant for WELDED meshes.  On an unwelded mesh coinciding vertices are different
 *     vertices, every triangle fan is open, and the surface tears along the seams as soon as a vertex moves.
 *   Definitions: a VALID triangle has three indices in [0, V_g), pairwise different as indices, and nine finite input coordinates;
 *     every other triangle of the group is dropped and counted.  The INCIDENCE LIST of vertex v is the local indices of the valid
 *     triangles with a corner at v in ascending order, k(v) its length.  The OTHERS of v in an incident triangle (a, b, c), as stored,
 *     are (b, c) if v is a, (c, a) if v is b, (a, b) if v is c; the sequence q_1 .. q_2k of v lists these pairs triangle after triangle
 *     in list order (the triangle umbrella: on a closed manifold every neighbour occurs twice, and the mean of q is the uniform
 *     umbrella's).  A BORDER vertex has 1 <= k(v) <= max_degree and some vertex that occurs exactly once in q.  A vertex is MOVABLE if
 *     its three input components are finite, 1 <= k(v) <= max_degree, pinned[v] == 0 (or pinned is NULL), and it is not a border vertex
 *     while PR_SMOOTH_PIN_BORDER is set.
 *   Step s = 0 .. steps - 1 has the factor f = lambda for even s and mu for odd s (Taubin: mu < -lambda < 0; plain Laplacian:
 *     mu == lambda).  A movable vertex is updated per component in fp32, without contraction or fused multiply-add:
 *       acc = q_1, then acc = acc + q_j for j = 2 .. 2k in that order; mean = acc / (float)(2k), correctly rounded;
 *       p' = p + f * (mean - p).
 *     All reads are of the positions before the step (Jacobi, two buffers).  Every other vertex keeps its three words bit for bit.
 *   out_vertices (V, 3): the positions after the last step; a copy with steps == 0; the rows that no clamped group owns are copied too.
 *   out_normals (V, 3), optional: for a vertex with 1 <= k <= max_degree, from the FINAL positions: per incident triangle in list order
 *     n = (b - a) x (c - a) of its stored corners, every component one difference of two products (cyclic, as in pr_mesh_audit:
 *     n0 = e1[1] e2[2] - e1[2] e2[1], ...); N is the first n, the others are added in order; length = sqrt((N0 N0 + N1 N1) + N2 N2),
 *     correctly rounded; the row is N / length if length is finite and > 0, else three zeros, as the mesher writes them.  Three zeros
 *     for every other vertex and for the rows that no clamped group owns.  A normal points from matter to empty space whenever the
 *     triangles do.
 *   incidence_offsets (V + 1) and incidence (3 T), optional, both or neither: the lists as a CSR.  The offsets are entries into
 *     `incidence` over ALL groups, those of a group's vertices are consecutive, and a row that no clamped group owns repeats the running
 *     total (0 in front of the first group, the total behind the last); incidence_offsets[V] is the total.  3 T entries are always room
 *     enough, so there is no counting call; the entries at and behind the total are not written.
 *   vertex_state (V) int32, optional: the sum of  1: k >= 1   2: border   4: pinned by the mask   8: k > max_degree   16: not finite
 *     32: movable.  -1 in the rows that no clamped group owns.
 *   counts (G, 8) int32, always and fully written:
 *       [0] valid triangles        [1] dropped triangles        [2] movable vertices        [3] finite vertices with k = 0
 *       [4] border vertices        [5] vertices with k > max_degree        [6] vertices that are not finite        [7] the largest k
 *   Order: the positions in the lists are handed out by integer atomics, so the order of arrival is arbitrary; every list with
 *     k <= max_degree is then sorted, no output depends on the arrival, and a second call gives equal bits everywhere - WITH ONE EXCEPTION: a list with k > max_degree
 *     is not sorted.  Its segment of `incidence` holds the right SET of triangles in an unspecified order; its vertex is immovable, has
 *     a zero normal and no border bit, and is counted in [5].
 *   Bounded work: a lane sorts at most max_degree entries by insertion, at most 3 T max_degree comparisons in all, and the border
 *     test reads at most max_degree^2 pairs of triangles; no lane waits for another.
 *   Memory safety: every index read from the mesh or from the workspace is range-checked where it is read; rows that no clamped group
 *     owns are only copied.  Hostile input may cost the correctness of the hostile group, never memory safety, and never another
 *     group's rows.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with BV = ceil(V / 256) + G and BT = ceil(T / 256) + G
 *   (upper bounds of the blocks of 256 vertices / triangles, none across two groups): 4 x 4 (G + 1) (per group: first vertex, first
 *   triangle, first vertex block, first triangle block) + 4 V (counts k) + 4 (V + 1) (list offsets) + 4 V (cursors) + 12 T (list
 *   entries) + 4 T (kept flags, with the list positions of the three corners) + 12 V (second position buffer) + 4 V (state) + 4 BV (list entries per vertex block) + 4 (BV + 1)
 *   (their scan and the total) + 4 BT (valid triangles per triangle block) + 24 BV (per vertex block: movable, k = 0, border,
 *   k > max_degree, not finite, largest k): 28 bytes per vertex, 16 per triangle.
 * Nine kernel launches on `stream` with steps == 0, plus ONE per step, whatever the optional outputs; no memset, no memcpy, no
 * allocation, no synchronisation: capturable into a HIP graph.  Integer atomics only, in the count and in the fill.
 * Additive entry points: PR_ABI_VERSION is unchanged.  sizeof(pr_mesh_smooth_t) = 120.
 * Refused (PR_ERR_INVALID, before any device work; by pr_mesh_smooth_workspace_size too, except the workspace itself): NULL vertices,
 * triangles, offsets, out_vertices or counts, groups < 1, a negative total, unknown flag bits, steps outside 0 .. 4096, max_degree
 * outside 1 .. 256, lambda or mu not finite, exactly one of incidence_offsets / incidence, out_vertices == vertices, 3 T + 256 G or
 * V + 256 G at or above 2^31 (the list entries and the block counts are int32); by the call only, and last: a NULL, misaligned or too
 * small workspace.
 */
#define PR_SMOOTH_PIN_BORDER 1u
typedef struct pr_mesh_smooth_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V, as a host value, >= 0 */
    int32_t total_triangles;              /* T, as a host value, >= 0 */
    uint32_t flags;                       /* PR_SMOOTH_PIN_BORDER or 0 */
    int32_t steps;                        /* 0 .. 4096 */
    int32_t max_degree;                   /* 1 .. 256 */
    float lambda;                         /* factor of the even steps, finite */
    float mu;                             /* factor of the odd steps, finite */
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    const uint8_t* pinned;                /* (V) or NULL; != 0: the vertex does not move */
    float* out_vertices;                  /* (V, 3), always written; not `vertices` */
    float* out_normals;                   /* (V, 3) or NULL */
    int32_t* incidence_offsets;           /* (V + 1) or NULL; with incidence */
    int32_t* incidence;                   /* (3 T) or NULL; with incidence_offsets */
    int32_t* vertex_state;                /* (V) or NULL */
    int32_t* counts;                      /* (G, 8), always written */
} pr_mesh_smooth_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_mesh_smooth_workspace_size(const pr_mesh_smooth_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_mesh_smooth_workspace_size bytes. */
int pr_mesh_smooth(const pr_mesh_smooth_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Area-weighted point samples of packed meshes: pr_mesh_sample draws `samples` points per group with probability proportional to
 * triangle area and carries the per-vertex rows (normals, attribute columns) to them - what a surface integral such as the deviation
 * of one mesh from another, or a point cloud with features, is made from.  Everything below is chosen so that NO output depends on
 * the execution order; a restatement in numpy and Python integers reproduces every bit (tests/sample_reference.py).
 *   Input: G meshes packed as pr_mesh_weld leaves them - vertices (V, 3) fp32, triangles (T, 3) int32 LOCAL to their group,
 *     vertex_offsets (G + 1), triangle_offsets (G + 1), optional normals (V, 3) fp32, optional attributes (V, C) fp32 with
 *     C = attribute_width, 1 <= C <= 4096 (ignored when attributes is NULL), all on the device; total_vertices / total_triangles are V
 *     and T as host values.  Offsets that leave [0, V] / [0, T] or decrease are clamped as pr_mesh_weld and pr_mesh_smooth clamp them,
 *     never followed.  Host values: samples = n per group, n >= 0, G n < 2^31; seed; first_sample; flags.
 *   Definitions: a VALID triangle has three indices in [0, V_g), pairwise different as indices, and nine finite coordinates
 *     (pr_mesh_smooth's definition); every other triangle of the group is dropped and counted.  The AREA of a valid triangle is
 *     pr_mesh_audit's, in fp64 without contraction: the corners converted to double, e1 = b - a, e2 = c - a, every component of the
 *     cross product one difference of two products (n0 = e1[1] e2[2] - e1[2] e2[1], cyclic), area = 0.5 sqrt((n0 n0 + n1 n1) + n2 n2),
 *     correctly rounded.  A_max(g) is the largest area of the group (a maximum is exact).  The WEIGHT of a valid triangle is
 *     w_t = (uint64) floor((area_t / A_max) * 2^32) with the correctly rounded fp64 quotient (the scaling is exact); a dropped triangle
 *     has w = 0.  A valid triangle smaller than A_max * 2^-32 therefore has weight 0 too and is NEVER DRAWN; counts[2] says how many
 *     there are.  W_t is the inclusive prefix sum of w within the group in uint64 and W(g) its last value (T < 2^31 and w <= 2^32:
 *     nothing overflows; integer sums are the same in any order).  A group with no valid triangle or with A_max == 0 is EMPTY.
 *   Sample i of group g has the stream index j = first_sample + i modulo 2^64 and the draw
 *       x[0..3] = philox4x32_10(counter = (low32(j), high32(j), g, 0), key = (low32(k), high32(k))),  k = splitmix64 finaliser of seed
 *     (the generator and the key mix of the renderer's noise streams, pr_noise_fill).  So samples [a, b) of one call are samples
 *     [0, b - a) of a call with first_sample advanced by a, and calls with disjoint index ranges draw disjoint streams.
 *     Triangle: r = x[0] | (uint64) x[1] << 32, pick = floor(r W(g) / 2^64), t = the first triangle with W_t > pick: probability
 *     w_t / W(g) to within 2^-63 absolute.  Barycentrics: U = x[2] >> 8, V = x[3] >> 8; if U + V > 2^24 (as integers) then
 *     U = 2^24 - U and V = 2^24 - V; b1 = U 2^-24, b2 = V 2^-24, b0 = (2^24 - U - V) 2^-24, all exact in fp32.
 *     Point formula, per component in fp32 without contraction or fused multiply-add, a, b, c being the rows of the stored corners in
 *     stored order:  p = ((b0 * a) + (b1 * b)) + (b2 * c).
 *   Outputs; the samples of an empty group get triangle -1 and zeros everywhere else:
 *     points (G, n, 3), always written: the point formula on the corner positions.
 *     triangle (G, n) int32, optional: t, local to the group.
 *     barycentric (G, n, 2), optional: (b1, b2) - pr_closest_query's (v, w): the point is a + v (b - a) + w (c - a).
 *     out_normals (G, n, 3), optional.  Without PR_SAMPLE_FACE_NORMALS it needs `normals`: N = the point formula on the three corner
 *       rows, length = sqrt((N0 N0 + N1 N1) + N2 N2) correctly rounded, the row is N / length if length is finite and > 0, else three
 *       zeros.  With PR_SAMPLE_FACE_NORMALS: N = (b - a) x (c - a) of the stored corner positions in fp32 with pr_mesh_smooth's
 *       component formula, normalised the same way; `normals` is ignored.
 *     out_attributes (G, n, C), optional, needs `attributes`: every column through the point formula.
 *     counts (G, 4) int32, always and fully written:
 *       [0] valid triangles    [1] dropped triangles    [2] valid triangles with weight 0    [3] samples drawn: n, 0 for an empty group
 *     measures (G, 2) fp64, always written: [0] A_max, [1] ((double) W(g) * A_max) * 2^-32 - the area the sampler distributes over, a
 *       repeatable stand-in for pr_mesh_audit's area, below it by less than 2^-32 A_max per valid triangle; both 0 for an empty group.
 *   Memory safety: every index read from the mesh or from the workspace is range-checked where it is read; rows that no clamped group
 *     owns are never touched.  Hostile input may cost the correctness of the hostile group, never memory safety, and never another
 *     group's outputs.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with BT = ceil(T / 256) + G (an upper bound of the blocks of
 *   256 triangles, none across two groups): 3 x 4 (G + 1) (per group: first vertex, first triangle, first triangle block) + 8 T (the
 *   area, then W_t) + 8 BT (block maxima) + 4 BT + 4 BT (valid / weight-0 triangles per block) + 8 BT + 8 BT (block weight sums and
 *   their scan) + 8 G + 8 G (A_max, W) + 16 G n (per sample: triangle, U, V).
 * Seven kernel launches on `stream`, EIGHT with out_attributes, whatever else is asked for and also with n == 0; no memset, no memcpy,
 * no allocation, no synchronisation: capturable into a HIP graph.  No atomics; no lane waits for another.
 * Additive entry points: PR_ABI_VERSION is unchanged.  sizeof(pr_mesh_sample_t) = 144.
 * Refused (PR_ERR_INVALID, before any device work; by pr_mesh_sample_workspace_size too, except the workspace itself): NULL vertices,
 * triangles, offsets, points, counts or measures, groups < 1, a negative total, unknown flag bits, samples < 0, G * samples at or above
 * 2^31, out_attributes without attributes, attribute_width outside 1 .. 4096 when attributes is given, out_normals with neither
 * normals nor PR_SAMPLE_FACE_NORMALS, T + 256 G at or above 2^31 (the block counts are int32), an output pointer equal to an input
 * pointer; by the call only, and last: a NULL, misaligned or too small workspace.
 */
#define PR_SAMPLE_FACE_NORMALS 1u
typedef struct pr_mesh_sample_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V, as a host value, >= 0 */
    int32_t total_triangles;              /* T, as a host value, >= 0 */
    uint32_t flags;                       /* PR_SAMPLE_FACE_NORMALS or 0 */
    int32_t samples;                      /* n per group, >= 0, G n < 2^31 */
    int32_t attribute_width;              /* C, 1 .. 4096 with attributes */
    uint64_t seed;                        /* the stream's seed */
    uint64_t first_sample;                /* stream index of sample 0 of every group */
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    const float* normals;                 /* (V, 3) or NULL */
    const float* attributes;              /* (V, C) or NULL */
    float* points;                        /* (G, n, 3), always written */
    int32_t* triangle;                    /* (G, n) or NULL */
    float* barycentric;                   /* (G, n, 2) or NULL */
    float* out_normals;                   /* (G, n, 3) or NULL */
    float* out_attributes;                /* (G, n, C) or NULL; needs attributes */
    int32_t* counts;                      /* (G, 4), always written */
    double* measures;                     /* (G, 2), always written */
} pr_mesh_sample_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_mesh_sample_workspace_size(const pr_mesh_sample_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_mesh_sample_workspace_size bytes. */
int pr_mesh_sample(const pr_mesh_sample_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Intersection of packed meshes on the grid of pr_raycast_build: pr_mesh_intersect finds, for every triangle of a QUERY mesh set, the
 * triangles of the TARGET mesh set of the same group that it cuts, and optionally the pairs and one contact segment per pair - does
 * object A, at its current pose, cut object B, and where; with PR_INTERSECT_SELF: does a mesh cut itself.  It reads what
 * pr_closest_query reads and builds nothing.  The result is DEFINED as that of the exhaustive rule below over all (query, target)
 * pairs of a group, in fixed fp32 arithmetic; the grid may change the time and never the bits - without any domain restriction,
 * because BOX is part of the rule (argument: DESIGN.md 28.2).
 *   Targets: the packed meshes of a finished EMITTING pr_raycast_build, read exactly as pr_closest_t reads them (same fields, same
 *     clamping of offsets, same grid coordinates and lists; references outside [0, max_references) or [0, T_g) are skipped where
 *     they are read: a stale or foreign grid costs correctness, never memory safety).
 *   Queries: a second packed mesh set of the same G - q_vertices (QV, 3) fp32, q_triangles (QT, 3) int32 LOCAL to their group,
 *     q_vertex_offsets (G + 1), q_triangle_offsets (G + 1), all on the device, q_total_vertices / q_total_triangles = QV and QT as host
 *     values, offsets clamped in the same way - and optionally transform (G, 3, 4) fp32, row-major, rows m_k = (m_k0, m_k1, m_k2, m_k3):
 *     query vertex x of group g is used as  x'_k = ((m_k0 x_0 + m_k1 x_1) + m_k2 x_2) + m_k3,  in fp32 without contraction; a NULL
 *     transform uses x itself.  (A static object's grid is built once and the moving object is posed per call.)
 *   Candidates, on both sides: three indices in [0, V_g) / [0, QV_g) and nine finite coordinates - on the query side after the
 *     transform.  A target that pr_raycast_build classifies as dead (a == b or a == c as values) is no candidate.
 *   Pair rule: query triangle Q = (a, b, c) and target triangle T of the same group, both candidates, are a PAIR iff BOX and
 *     (EDGE(Q -> T) or EDGE(T -> Q)) hold.
 *       BOX: on all three axes min(Q) <= max(T) and min(T) <= max(Q), min and max over the three corners, compared as fp32 values.
 *       EDGE(X -> Y): at least one of X's edges is accepted by Y.  X's edges are taken in the order (a, b), (b, c), (c, a), each as
 *         the ray o = start, d = end - start, and the test is pr_raycast_t's test of one ray against one triangle exactly as stated
 *         there (fp32, no contraction, the same dot and cross products, e1, e2, p, det, s, u, q, v, t), with no culling (det < 0 or
 *         det > 0), t_min = 0, t_max = 1, and one more clause, the CONDITIONING clause, with that header's dot-product order:
 *             det * det > 2^-20 * (((e1 . e1) (e2 . e2)) (d . d))        (four fp32 products, left to right as bracketed).
 *       Every comparison is false on a NaN.
 *     The clause is no decoration: neighbouring triangles of a marching-tetrahedra mesh are often coplanar, det is then rounding
 *     noise instead of 0, and without the clause a clean lattice sphere "cuts itself".  Consequences: COPLANAR OVERLAP IS NEVER A
 *     PAIR; the rule is SYMMETRIC - with the roles of the two mesh sets swapped (and the transform applied to the vertices beforehand)
 *     the pair set is transposed -; like pr_raycast_query it is NOT WATERTIGHT along shared edges and vertices: an edge through
 *     another triangle's edge or vertex can be accepted by both neighbours or by neither.
 *   PR_INTERSECT_SELF: the query set IS the target set.  The four query pointers must each be NULL or equal to the target's, the
 *     query totals must equal the target's, transform must be NULL.  A pair is left out if q == t, and if any corner of Q equals any
 *     corner of T as VALUES in the sense of pr_mesh_audit ("Vertex identity is by VALUE": the three fp32 components compare equal
 *     with ==, so -0 equals +0) - neighbours always touch.  Every unordered pair that remains shows up from both sides.
 *   Outputs, all optional except count, rows in the PACKED order of the query triangles:
 *     count (QT) int32: the pairs of the query triangle.   first (QT) int32: the lowest target index among them, or -1.
 *     pair_offsets (QT + 1) int32: the exclusive sums of count; the last element is P, the number of pairs.
 *     pairs (max_pairs, 2) int32: (query, target), both LOCAL to their group; the pairs of packed query row r are the rows
 *       [pair_offsets[r], pair_offsets[r + 1]).  The order inside such a segment of rows is unspecified.
 *     segments (max_pairs, 2, 3) fp32, needs pairs: the accepted edge tests of the pair are taken in the fixed order Q's three edges
 *       against T, then T's three against Q; each gives the point o + t d, per component o_k + t * d_k in fp32 without contraction.
 *       Endpoint 0 is the first such point; endpoint 1 is the point with the largest squared distance from endpoint 0 (r = point -
 *       endpoint 0, r . r in fp32 with the dot-product order above), the earliest on ties: with one accepted test it equals endpoint 0.
 *     Rows of queries that are no candidates, and rows that no clamped group owns, get count 0 and first -1.  Nothing at or beyond
 *     max_pairs is written; count, first and pair_offsets do not depend on max_pairs.
 *   Calling pattern (the build's): P is only known on the device.  A counting call with pairs == NULL writes count, first and
 *     pair_offsets; one read-back of pair_offsets[QT] follows; an exactly sized emitting call ends the sequence (and writes count,
 *     first and pair_offsets again, with the same values).
 *   Query: one lane per query triangle, 256-lane blocks that never span two groups.  The lane tests the group's loose list.  With
 *     g(x) = (x - origin_k) / cell_k in fp32 (the build's two roundings): if on some axis not g(max Q) >= 0 or not g(min Q) < cells_k,
 *     no tight target is tested.  Otherwise the lane visits the cells (int)max(g(min Q), 0) .. min((int)min(g(max Q), cells_k),
 *     cells_k - 1) on every axis, and a triangle found in the list of a cell is tested there iff BOX holds and the cell is
 *     (int)max(g(min T), g(min Q)) on every axis: a target listed in several cells is counted once.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes, with NB = floor(QT / 256) + 1: 5 x 4 (G + 1) (per group:
 *   first vertex and first triangle of both sets, first query block) + 4 (QT + 1) (the exclusive sums) + 2 x 4 NB (block sums of the
 *   counts and their scan) + 4 (the total).
 * Five kernel launches on `stream` for a counting call, six for an emitting one (also with QT == 0), no memset, no memcpy, no
 * allocation, no synchronisation: capturable into a HIP graph.  No atomics.
 * Additive entry points: PR_ABI_VERSION is unchanged.  sizeof(pr_mesh_intersect_t) = 200.
 * Refused (PR_ERR_INVALID, before any device work; by pr_mesh_intersect_workspace_size too, except the workspace itself):
 * everything pr_closest_query refuses about mesh, grid and capacities (NULL vertices, triangles, offsets or cell_offsets, groups < 1,
 * a cells entry outside 1 .. 1024 or a product above 2^21, a cell size that is not finite or not > 0, a non-finite origin, a negative
 * total or capacity, NULL references with max_references > 0, T + 256 G or G (C + 1) + 256 at or above 2^31), a NULL count, segments
 * without pairs, a negative q_total_vertices, q_total_triangles or max_pairs, QT + 256 G at or above 2^31, unknown flag bits; without
 * PR_INTERSECT_SELF NULL q_vertices, q_triangles or query offsets; with it a transform, a foreign query pointer or other query
 * totals; by the call only, and last: a NULL, misaligned or too small workspace.  QT == 0, T == 0 and an empty group are valid.
 */
#define PR_INTERSECT_SELF 1u
typedef struct pr_mesh_intersect_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V = vertex_offsets[G], as a host value, >= 0 */
    int32_t total_triangles;              /* T = triangle_offsets[G], as a host value, >= 0 */
    uint32_t flags;                       /* PR_INTERSECT_SELF or 0 */
    float origin[3];                      /* the grid of the build: finite */
    float cell[3];                        /* finite, > 0 */
    int32_t cells[3];                     /* each 1 .. PR_RAYCAST_MAX_AXIS_CELLS, product <= PR_RAYCAST_MAX_CELLS */
    int32_t max_references;               /* rows of references, >= 0 */
    int32_t q_total_vertices;             /* QV, as a host value, >= 0 (self: V) */
    int32_t q_total_triangles;            /* QT, as a host value, >= 0 (self: T) */
    int32_t max_pairs;                    /* rows of pairs and segments, >= 0 */
    uint32_t reserved_;
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    const int32_t* cell_offsets;          /* (G (C + 1) + 1), as pr_raycast_build wrote them */
    const int32_t* references;            /* (max_references), as an emitting pr_raycast_build wrote them (NULL: max_references 0) */
    const float* q_vertices;              /* (QV, 3); self: NULL or vertices */
    const int32_t* q_triangles;           /* (QT, 3), indices local to the group; self: NULL or triangles */
    const int32_t* q_vertex_offsets;      /* (G + 1); self: NULL or vertex_offsets */
    const int32_t* q_triangle_offsets;    /* (G + 1); self: NULL or triangle_offsets */
    const float* transform;               /* (G, 3, 4) or NULL; self: NULL */
    int32_t* count;                       /* (QT), always written */
    int32_t* first;                       /* (QT) or NULL */
    int32_t* pair_offsets;                /* (QT + 1) or NULL */
    int32_t* pairs;                       /* (max_pairs, 2) or NULL: count only */
    float* segments;                      /* (max_pairs, 2, 3) or NULL; needs pairs */
} pr_mesh_intersect_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_mesh_intersect_workspace_size(const pr_mesh_intersect_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_mesh_intersect_workspace_size bytes. */
int pr_mesh_intersect(const pr_mesh_intersect_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Placement of the vertices of simplified meshes by quadric error (Lindstrom's placement for Rossignac-Borrel clustering):
 * pr_mesh_place moves every vertex of a MERGED mesh - what pr_simplify_mesh made, one vertex per cluster at the mean of its members -
 * to the point that minimises the area-weighted sum of squared distances to the planes of the INPUT triangles that touch the cluster,
 * with a Tikhonov pull toward the stored position.  Convex edges and corners, which the mean rounds off, are kept.  The triangle
 * lists are not touched.
 *   Input: G input meshes packed as pr_simplify_mesh reads them - vertices (V, 3) fp32, triangles (T, 3) int32 LOCAL to their group,
 *     vertex_offsets (G + 1), triangle_offsets (G + 1), all on the device; total_vertices / total_triangles are V and T as host values.
 *     vertex_map (V) int32 as pr_simplify_mesh writes it: the merged index of every input vertex, local to its group.  The merged
 *     mesh: merged_vertices (VO, 3) fp32, merged_vertex_offsets (G + 1), and optionally - both or neither - merged_triangles (TO, 3)
 *     int32 local to their group with merged_triangle_offsets (G + 1); total_merged_vertices / total_merged_triangles are VO and TO as
 *     host values (TO is not read without merged_triangles).  Each of the four offset arrays is clamped on its own as pr_simplify_mesh
 *     clamps: an entry that leaves [0, total] or decreases is clamped, never followed.  Group g then has V_g, T_g, VO_g, TO_g rows.
 *   Host values: scale h (finite, > 0) - the unit of length of the quadric, e.g. the largest cell size -, max_move[3] (finite, >= 0),
 *     regularisation (finite, > 0), flags (0).  h, max_move and regularisation enter the arithmetic as (double) of the fp32 values.
 *   Rule: fp64 without contraction, every operation rounded on its own, sqrt and division correctly rounded.
 *     An input triangle of group g is VALID if its three indices are in [0, V_g) and its nine coordinates are finite; the others are
 *     counted and contribute nothing.  A valid triangle (a, b, c) as stored CONTRIBUTES once to every distinct cluster j among
 *     vertex_map[a], vertex_map[b], vertex_map[c]; a corner whose map entry lies outside [0, VO_g) contributes nothing.  For such a
 *     cluster, with m = merged vertex j of the group as stored (fp32 -> fp64), per component:
 *       a' = (a - m) / h, b' = (b - m) / h, c' = (c - m) / h;   e1 = b' - a', e2 = c' - a';
 *       n0 = e1[1] e2[2] - e1[2] e2[1], n1 = e1[2] e2[0] - e1[0] e2[2], n2 = e1[0] e2[1] - e1[1] e2[0]  (a difference of two products);
 *       L = sqrt((n0 n0 + n1 n1) + n2 n2);   d = -((n0 a'[0] + n1 a'[1]) + n2 a'[2]).
 *     A contribution with L not finite or not > 0 is SKIPPED and counted.  Otherwise its nine coefficients are, each a product divided
 *     by L,  q0 = n0 n0 / L, q1 = n0 n1 / L, q2 = n0 n2 / L, q3 = n1 n1 / L, q4 = n1 n2 / L, q5 = n2 n2 / L, q6 = d n0 / L,
 *     q7 = d n1 / L, q8 = d n2 / L: the plane quadric weighted by twice the area, in units of h around m.  If any |q_i| > 2^16 or is
 *     not finite the contribution is skipped and counted.  Otherwise llrint(q_i 2^36) - the product is exact - is added to the
 *     cluster's nine int64 sums, modulo 2^64, and 1 to its int32 contribution count.  INTEGER SUMS: the order of arrival cannot show.
 *   Per merged vertex with at least one contribution: S_i = (double)(int64 sum i) 2^-36;
 *       lambda = (regularisation ((S0 + S3) + S5)) / 3;   m00 = S0 + lambda, m01 = S1, m02 = S2, m11 = S3 + lambda, m12 = S4,
 *       m22 = S5 + lambda;   r = (-S6, -S7, -S8);
 *       c00 = m11 m22 - m12 m12, c01 = m02 m12 - m01 m22, c02 = m01 m12 - m02 m11, c11 = m00 m22 - m02 m02,
 *       c12 = m01 m02 - m00 m12, c22 = m00 m11 - m01 m01;   det = (m00 c00 + m01 c01) + m02 c02;
 *       y0 = ((c00 r0 + c01 r1) + c02 r2) / det, y1 = ((c01 r0 + c11 r1) + c12 r2) / det, y2 = ((c02 r0 + c12 r1) + c22 r2) / det;
 *       t_k = h y_k.
 *     A planar cluster keeps its tangential position up to the regularisation, an edge cluster slides only along its edge.  The vertex
 *     KEEPS its three stored words, bit for bit, if it has no contribution, if det is not finite or not > 0, if some y_k is not
 *     finite, or if some |t_k| > max_move[k].  Otherwise it MOVES: out_k = (float)(m_k + t_k).
 *   With merged triangles: one whose three indices are in [0, VO_g) is TURNED iff (N0 N0' + N1 N1') + N2 N2' < 0, where
 *     N = (b - a) x (c - a), components as above, in fp64 on the stored merged vertices and N' the same on out_vertices.  Turned
 *     triangles are reported, never repaired.
 *   out_vertices (VO, 3): every row of a clamped group is written; the rows that no clamped group owns are not touched.  It must not
 *     be `vertices` or `merged_vertices`.
 *   counts (G, 4) int32, always and fully written: vertices moved, vertices kept, contributions skipped plus invalid triangles,
 *     triangles turned (0 without merged triangles).
 *   Memory safety: every index read from a mesh or from the map is range-checked where it is read.  Hostile input may cost the
 *     correctness of the hostile group, never memory safety, and never another group's rows.
 * Workspace bytes = the sum of these regions, each rounded up to 256 bytes: 8 x 4 (G + 1) (per group and per kind of row - input
 *   vertices, input triangles, merged vertices, merged triangles -: first row, first block) + 72 VO (nine int64 sums per merged
 *   vertex) + 4 VO (contribution counts).
 * Four kernel launches on `stream` (three without merged triangles), no memset, no memcpy, no allocation, no synchronisation:
 * capturable into a HIP graph.  Integer atomics only.
 * Additive entry points: PR_ABI_VERSION is unchanged.  sizeof(pr_mesh_place_t) = 136.
 * Refused (PR_ERR_INVALID, before any device work; by pr_mesh_place_workspace_size too, except the workspace itself): NULL vertices,
 * triangles, vertex_map, merged_vertices, out_vertices, counts or one of the three required offset arrays, exactly one of
 * merged_triangles / merged_triangle_offsets, groups < 1, a negative total, a scale or regularisation that is not finite or not > 0,
 * a max_move entry that is not finite or negative, flags != 0, out_vertices == vertices or == merged_vertices, V + 256 G,
 * T + 256 G, VO + 256 G or TO + 256 G at or above 2^31 (the block counts are int32), a workspace of 2^62 bytes or more; by the call
 * only, and last: a NULL, misaligned or too small workspace.
 */
typedef struct pr_mesh_place_t {
    int32_t groups;                       /* G >= 1 */
    int32_t total_vertices;               /* V, as a host value, >= 0 */
    int32_t total_triangles;              /* T, as a host value, >= 0 */
    uint32_t flags;                       /* 0 */
    int32_t total_merged_vertices;        /* VO, as a host value, >= 0 */
    int32_t total_merged_triangles;       /* TO, as a host value, >= 0; not read without merged_triangles */
    float scale;                          /* h: finite, > 0 */
    float regularisation;                 /* finite, > 0 */
    float max_move[3];                    /* finite, >= 0 */
    uint32_t reserved_;
    const float* vertices;                /* (V, 3) */
    const int32_t* triangles;             /* (T, 3), indices local to the group */
    const int32_t* vertex_offsets;        /* (G + 1) */
    const int32_t* triangle_offsets;      /* (G + 1) */
    const int32_t* vertex_map;            /* (V): merged index of every input vertex, local to the group */
    const float* merged_vertices;         /* (VO, 3) */
    const int32_t* merged_vertex_offsets; /* (G + 1) */
    const int32_t* merged_triangles;      /* (TO, 3) or NULL; with merged_triangle_offsets */
    const int32_t* merged_triangle_offsets; /* (G + 1) or NULL; with merged_triangles */
    float* out_vertices;                  /* (VO, 3); not an input */
    int32_t* counts;                      /* (G, 4), always written */
} pr_mesh_place_t;
/* Host computation, no device work; refuses everything above that does not concern the workspace. */
int pr_mesh_place_workspace_size(const pr_mesh_place_t* s, size_t* bytes);
/* `workspace`: 256-byte aligned, pr_mesh_place_workspace_size bytes. */
int pr_mesh_place(const pr_mesh_place_t* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Backward pass of pr_render_forward (what torch.autograd does for the reference's op graph when
 * training/trainer_backpropagated_autoencoder.py:349 calls total_loss.backward()).  The forward call must
 * have run with PR_FLAG_SAVE_FOR_BACKWARD (with or without PR_FLAG_TRAIN_BN) on the same `call`, `objects` and
 * `forward_workspace`, which must not have been touched since.  In hierarchical (use_fine) calls the resampled
 * depths are constants (the reference detaches them, ray_helper.py:1340): the fine pass differentiates through the
 * coarse depths it merged in and through the sample positions, the coarse pass through its own results only.
 *
 * Incoming gradients (d loss / d output field, same shapes as pr_entry_t; NULL = zero):
 */
typedef struct pr_entry_grads_t {
    const float* integrated_features;                 /* (N,R,F) */
    const float* opacity;                             /* (N,R) */
    const float* depth;                               /* (N,R) */
    const float* integrated_displacements_magnitude;  /* (N,R): flows into the displacements only, the weights are
                                                         detached there (object_composer.py:772) */
    const float* weights;                             /* (N,R,P) per object, (N,R,sum P) in merged order for the global
                                                         entry: consumers of the compositing weights themselves
                                                         (compute_expected_positions, object_composer.py:603-622) */
    const float* integrated_divergence;               /* (N,R); read with PR_FLAG_DIVERGENCE_GRAD only: flows into the Hutchinson
                                                         estimate (ray bender weights, sample positions), the alphas are
                                                         detached there (object_composer.py:768-769) */
} pr_entry_grads_t;

typedef struct pr_output_grads_t {
    pr_entry_grads_t object[PR_MAX_OBJECTS];
    pr_entry_grads_t global;
    /* gradients of the per-sample exports of pr_outputs_t (NULL = zero): the sample depths and the ray bender's
       displacement vectors, which forward_expected_positions averages (object_composer.py:603-722) */
    const float* sample_t[PR_MAX_OBJECTS];            /* (N,R,P) */
    const float* sample_delta[PR_MAX_OBJECTS];        /* (N,R,P,3); objects with a ray bender */
} pr_output_grads_t;

/* Gradient buffers of one object model, shaped like the parameters (nn.Linear layout).  The library ACCUMULATES
 * (+=) into them: the caller zero-initialises; object instances that share a model pass the same pointers.
 * Any pointer may be NULL (gradient not wanted). */
typedef struct pr_linear_grad_t {
    float* weight;
    float* bias;
} pr_linear_grad_t;

typedef struct pr_model_grads_t {
    pr_linear_grad_t backbone[PR_MAX_LAYERS];
    pr_linear_grad_t alpha_head;
    pr_linear_grad_t head0;
    pr_linear_grad_t affine1;
    pr_linear_grad_t head3;
    pr_linear_grad_t affine4;
    pr_linear_grad_t head6;
    pr_linear_grad_t bender[PR_MAX_LAYERS];
    pr_linear_grad_t bender_out;
} pr_model_grads_t;

typedef struct pr_input_grads_t {
    float* w2o;              /* (N,K,3,4) accumulated; or NULL */
    float* style;            /* (N,K,S)  accumulated; or NULL */
    float* deformation;      /* (N,K,D)  accumulated; or NULL */
    pr_model_grads_t model[PR_MAX_OBJECTS];   /* per object instance (coarse models) */
    pr_model_grads_t model_fine[PR_MAX_OBJECTS]; /* fine models (use_fine calls only) */
    /* gradients of the camera rays (NULL = not wanted): what learnable camera parameters are trained through
       (model/layers/camera_parameters_storage.py; the reference's rays are torch tensors with a graph,
       utils/lib_3d/ray_helper.py:15-52, 1203-1227).  Sample positions x = o + d t, the slab-test depths, the skybox input
       and the sample spacings dt |d| all depend on them. */
    float* ray_origins;      /* (N,3)   accumulated; or NULL */
    float* ray_directions;   /* (N,R,3) accumulated; or NULL */
} pr_input_grads_t;

/* Streams: the call is ordered on `stream` like every other entry point - work enqueued on `stream` before the call precedes
 * it, work enqueued after the call follows all of it.  Inside, calls with several objects run the objects on two lanes: `stream`
 * and one internal stream per device (created on the first such call, kept for the life of the process), forked from `stream`
 * after the compositing backward and joined back into it before the call returns (events, no host synchronisation).  Both
 * workspaces must stay untouched until work enqueued on `stream` after the call would run. */
int pr_backward_workspace_size(const pr_call_t* call, const pr_object_t* objects, size_t* bytes);
int pr_render_backward(const pr_call_t* call, const pr_object_t* objects, const pr_output_grads_t* grads_coarse,
                       const pr_output_grads_t* grads_fine /* NULL unless use_fine */, const pr_input_grads_t* out,
                       void* forward_workspace, size_t forward_workspace_bytes,
                       void* backward_workspace, size_t backward_workspace_bytes, void* stream);

/*
 * The per-sample gradients of the compositing backward (tests and diagnostics): what its kernel left in the backward workspace
 * for the per-object network passes, copied out right behind its launch - the later kernels clear and reuse those buffers.
 * Every pointer may be NULL (not wanted); objects beyond call->objects are ignored.  One struct per level.
 */
typedef struct pr_sample_grads_t {
    float* sigma[PR_MAX_OBJECTS];                   /* (N,R,P_k) d loss / d raw density, summed over the object's own entry and
                                                       the global entry */
    float* t[PR_MAX_OBJECTS];                       /* (N,R,P_k) d loss / d sample depth (through the spacings and `depth`) */
    float* displacement_magnitude[PR_MAX_OBJECTS];  /* (N,R,P_k) d loss / d |delta|; objects with a ray bender, ignored otherwise */
    float* features[PR_MAX_OBJECTS];                /* (N,R,P_k,F) dense d loss / d feature row; zeros where sample_slot < 0 */
    float* norm;                                    /* (N,R) d loss / d |d| through the sample spacings of every entry */
    float* feature_rows[PR_MAX_OBJECTS];            /* (N,R,P_k,F) dense: the forward pass's feature rows the kernel read (the
                                                       input of the stage no forward export carries); zeros where sample_slot < 0 */
} pr_sample_grads_t;

/* pr_render_backward plus the exports above (`exports_coarse` / `exports_fine`: NULL = none; with both NULL this IS
 * pr_render_backward: no additional launch).  Additive entry point: PR_ABI_VERSION is unchanged. */
int pr_render_backward_exported(const pr_call_t* call, const pr_object_t* objects, const pr_output_grads_t* grads_coarse,
                                const pr_output_grads_t* grads_fine /* NULL unless use_fine */, const pr_input_grads_t* out,
                                void* forward_workspace, size_t forward_workspace_bytes,
                                void* backward_workspace, size_t backward_workspace_bytes, void* stream,
                                const pr_sample_grads_t* exports_coarse, const pr_sample_grads_t* exports_fine);

/*
 * Camera rays (RayHelper.create_camera_rays + pixel selection + transform_rays, ray_helper.py:15-52,
 * :433-482, :1203-1227): for frame n and ray r with pixel (rows[r], cols[r]),
 *   d_cam = ((col - W/2)/f_n, -(row - H/2)/f_n, -1),  d_world = R_n d_cam,  o_world = t_n.
 * c2w (N,3,4); focals (N) already multiplied by focal_length_multiplier; rows/cols int32 (R), shared
 * by all frames, or (N,R) - one pixel list per frame, as the random samplers of the reference produce
 * (sample_rays_strided_patch :236, sample_rays_weighted :611, sample_rays :730) - when
 * per_frame_pixels != 0.
 */
int pr_camera_rays(int32_t frames, int32_t rays, int32_t height, int32_t width, int32_t per_frame_pixels,
                   const float* c2w, const float* focals, const int32_t* rows, const int32_t* cols,
                   float* ray_origins, float* ray_directions, float* focal_normals, void* stream);

/*
 * Strided patch pixels (RayHelper.sample_rays_strided_patch, utils/lib_3d/ray_helper.py:236-431): per frame one random patch
 * centre drawn from the bounding-box weight image (object k adds weights[k] / area_k over its pixel-aligned box), clamped into
 * the image and aligned to the grid of the largest stride; then for every stride s_i (ascending) a p_i x p_i pixel grid with
 * p_i = patch_size * s_0 / s_i, row-major, strides concatenated: rows / cols (N, sum p_i^2) int32.  boxes (N,4,K) normalised
 * [left, top, right, bottom]; weights (K); u (N) the uniform draws in [0, 1), one per frame.
 */
int pr_patch_pixels(int32_t frames, int32_t objects, int32_t height, int32_t width, int32_t patch_size, int32_t stride_count,
                    const int32_t* strides /* host */, const float* boxes, const float* weights, const float* u,
                    int32_t* rows, int32_t* cols, void* stream);

/*
 * Pose matrices: (rotation (x, y, z Euler angles, radians), translation) -> the 4x4 transform [R t; 0 1] with R = Ry (Rx Rz)
 * (Transformations3D.homogeneous_rotation_translation, utils/lib_3d/transformations_3d.py:69-96) and its inverse
 * [R^T  -R^T t; 0 1] (the reference calls torch.inverse on it: environment_model.py:221, :1078).  rotations, translations
 * (count,3); matrices, inverses (count,4,4).  Used for the cameras (c2w / w2c) and the objects (o2w / w2o) of a call.
 */
int pr_pose_matrices(int32_t count, const float* rotations, const float* translations, float* matrices, float* inverses,
                     void* stream);
/* Its backward pass: g_matrices / g_inverses (count,4,4) or NULL -> g_rotations, g_translations (count,3), written. */
int pr_pose_matrices_backward(int32_t count, const float* rotations, const float* translations, const float* g_matrices,
                              const float* g_inverses, float* g_rotations, float* g_translations, void* stream);

/* Scene set-up of an evaluation call in ONE launch - replaces, for tensors without a graph, the span of
 * EnvironmentModel.forward_from_scene_encoding between the scene encoding and the composer call (reference:
 * model/environment_model.py:1066-1112: Transformations3D.homogeneous_rotation_translation + torch.inverse for cameras and objects,
 * compute_object_bounding_boxes :234-327, compute_object_axes_projection :329-404) and the permutes that bring the reference's
 * (..., 3 | S | D, K) scene tensors into the renderer's layouts.  Arithmetic = pr_pose_matrices + pr_project_points, bit for bit.
 * frames = product of the leading dims incl. observations; renderer frame n = frame * cameras + camera. */
typedef struct {
    int32_t frames, cameras, objects, box_points_per_object, style_features, deformation_features, height, width;
    float focal_multiplier;          /* config["data"]["focal_length_multiplier"] */
    float upsample_factor;           /* boxes (and the rays) use focals * multiplier * upsample_factor */
    int32_t axes_with_upsampled_focals; /* 0: the axes use focals * multiplier (forward_from_scene_encoding), 1: the upsampled ones */
    const float* camera_rotations;   /* (frames, cameras, 3) */
    const float* camera_translations;
    const float* focals;             /* (frames, cameras) */
    const float* object_rotations;   /* (frames, 3, objects): the reference's trailing-object layout */
    const float* object_translations;
    const float* style;              /* (frames, S, objects) */
    const float* deformation;        /* (frames, D, objects) */
    const uint8_t* object_in_scene;  /* (frames, objects) bool */
    const float* box_points;         /* (objects, box_points_per_object, 3) object-frame corner + edge points */
    const float* axes_points;        /* (objects, 4, 3) origin + unit axes */
    float* boxes;                    /* out (frames, cameras, 4, objects) [left, top, right, bottom], clamped to [0, 1] */
    float* projected_points;         /* out (frames, cameras, box_points_per_object, 2, objects), clamped */
    float* axes;                     /* out (frames, cameras, 4, 2, objects), not clamped */
    float* camera34;                 /* out (frames * cameras, 3, 4): the c2w rows pr_camera_rays takes */
    float* render_focals;            /* out (frames * cameras) */
    float* w2o34;                    /* out (frames * cameras, objects, 3, 4): pr_call_t.w2o */
    float* style_nks;                /* out (frames * cameras, objects, S): pr_call_t.style */
    float* deformation_nkd;          /* out (frames * cameras, objects, D): pr_call_t.deformation */
    uint8_t* present;                /* out (frames * cameras, objects): pr_call_t.object_in_scene */
} pr_scene_setup_t;
int pr_scene_setup(const pr_scene_setup_t* setup, void* stream);
/*
 * Backward of pr_scene_setup's renderer inputs, one launch (a TRAINING call through the fused scene set-up): the gradients
 * pr_render_backward leaves in the renderer's layouts - g_w2o34 (frames x cameras, objects, 3, 4), g_style_nks (.., objects,
 * S), g_deformation_nkd (.., objects, D); any may be NULL = zero - are summed over the cameras of a frame and taken to the
 * scene tensors' layouts: g_rotations / g_translations (frames, 3, objects) through the pose matrices' backward (w2o is the
 * rigid inverse of [R t; 0 1], R = Ry (Rx Rz): /root/reference/utils/lib_3d/transformations_3d.py:69-96 and torch.inverse at
 * /root/reference/model/environment_model.py:221), g_style (frames, S, objects), g_deformation (frames, D, objects).  Outputs
 * that are NULL are skipped (rotations and translations come together).  What torch.autograd does for the reference through
 * ~150 small tensor ops (model/environment_model.py:206-232).
 */
int pr_scene_setup_backward(int32_t frames, int32_t cameras, int32_t objects, int32_t style_features, int32_t deformation_features,
                            const float* object_rotations, const float* object_translations, const float* g_w2o34,
                            const float* g_style_nks, const float* g_deformation_nkd, float* g_rotations, float* g_translations,
                            float* g_style, float* g_deformation, void* stream);

/*
 * Projects object-frame points into the cameras of their frame (EnvironmentModel.compute_object_bounding_boxes /
 * compute_object_axes_projection, model/environment_model.py:234-404).  points (K,P,3); o2w (F,K,4,4); w2c (F,C,4,4);
 * focals (F,C) -> projected (F,C,P,2,K): image coordinates normalised to [0,1] ((v + size/2) / size, x right, y down).
 * boxes (F,C,4,K) [left, top, right, bottom] or NULL: with boxes, points behind the camera do not bound the box and both
 * outputs are clamped to [0,1]; without, the projections are left as they are (the axes variant).
 */
int pr_project_points(int32_t frames, int32_t cameras, int32_t objects, int32_t points_per_object, const float* points,
                      const float* o2w, const float* w2c, const float* focals, int32_t height, int32_t width,
                      float* projected, float* boxes, void* stream);

/*
 * ObjectComposer.compute_expected_positions (model/object_composer.py:603-622) for object `object_index` of a call:
 *   expected[n][r] = sum_i w_i (o + d t_i + delta_i) / (sum_i w_i + 1e-8)      (object frame)
 * with o, d the w2o-transformed ray (RayHelper.transform_rays), t / weights (N,R,P) as produced by pr_render_forward
 * (sample_t export, object entry weights) and delta (N,R,P,3) or NULL.  expected: (N,R,3).
 */
int pr_expected_positions(int32_t frames, int32_t rays, int32_t objects, int32_t object_index, int32_t positions,
                          const float* ray_origins, const float* ray_directions, const float* w2o, const float* t,
                          const float* weights, const float* delta, float* expected, void* stream);

/*
 * The values PR_FLAG_DEVICE_NOISE generates for one noise tensor, written out: element i of the tensor with `kind`
 * (0 stratified jitter U[0,1), 1 coarse density noise N(0,1), 2 inverse-CDF positions U[0,1), 3 per-object density noise
 * N(0,1), 4 merged-list density noise N(0,1), 5 Hutchinson probes N(0,1)) of model type `type` (0 coarse / 1 fine) and
 * object `object`.  count elements, fp32.
 */
int pr_noise_fill(uint64_t seed, int32_t kind, int32_t type, int32_t object, int64_t count, float* out, void* stream);

/*
 * Region-of-interest max pooling: the crop the reference's object encoders and pose estimators take from the
 * observations before their small ResNets - torchvision.ops.roi_pool(observations, boxes, input_size) at
 * model/object_encoder_v4.py:121, model/object_encoder_v5.py:121 and model/object_parameters_encoder_v4.py:131
 * (torchvision 0.9.1, a dependency outside the reference tree; the operator's published definition is restated in
 * csrc/roi_pool.hip and oracle/roi_pool_oracle.py).  input (N,C,H,W); boxes (K,5) = [image index, x1, y1, x2, y2] in
 * input pixels times spatial_scale; output (K,C,ph,pw); argmax (K,C,ph,pw) int32 flat h*W + w of the selected element,
 * -1 for an empty bin, or NULL.  The backward call ACCUMULATES grad_output into grad_input (N,C,H,W) at the argmax
 * positions (the caller zero-initialises).
 */
int pr_roi_pool_forward(int32_t images, int32_t channels, int32_t height, int32_t width, const float* input,
                        int32_t rois, const float* boxes, int32_t pooled_height, int32_t pooled_width,
                        float spatial_scale, float* output, int32_t* argmax, void* stream);
int pr_roi_pool_backward(int32_t images, int32_t channels, int32_t height, int32_t width, int32_t rois,
                         const float* boxes, int32_t pooled_height, int32_t pooled_width, const float* grad_output,
                         const int32_t* argmax, float* grad_input, void* stream);

/*
 * Point queries of ONE object model's fields: density, style-modulated feature and ray-bender displacement at explicit
 * OBJECT-frame positions of its box - RayBendingStyleNerfModel.forward in evaluation mode (running BatchNorm statistics;
 * model/nerf_models/ray_bending_style_nerf_model.py:137-219): closed-interval box test on the given position, boolean compaction
 * in flat order, ray bender (+ clamp, + canonical pose), second box test on the bent position, backbone, density head, style
 * feature head; (0 | empty_space_alpha | 0) for every point that is not evaluated.  The skybox model (kind == 1) reads the ray
 * origin of the group and the direction of the point, returns density 10 and still obeys the box test on `positions`.
 * The evaluation is the renderer's fused MLP kernel on compact records built from the positions (the query runs as frames = G,
 * rays = M, one position per ray); unlike a render the feature head runs on EVERY in-box point (no sigma gate: the model returns
 * features where the density is not positive too).  With features == NULL the feature head is not run at all (8 of the 11 matrix
 * products of a point remain; a skybox density-only query evaluates nothing).  model->positions is ignored.  World-frame
 * positions are the caller's to transform (w2o).  No gradients.
 */
typedef struct pr_query_t {
    int32_t groups;              /* G: one style / deformation row (and, skybox, one ray origin) per group */
    int32_t points;              /* M points per group; G * M < 2^31 */
    uint32_t flags;              /* PR_FLAG_CANONICAL_POSE or 0; anything else: PR_ERR_INVALID */
    int32_t precision;           /* PR_PRECISION_*: what `packed` was packed with */
    const float* positions;      /* (G,M,3) OBJECT-frame positions */
    const float* ray_origins;    /* (G,3)   kind == 1 (skybox) only, object frame; else NULL */
    const float* ray_directions; /* (G,M,3) kind == 1 only, need not be normalised; else NULL */
    const float* style;          /* (G,S) */
    const float* deformation;    /* (G,D) */
    float* features;             /* out (G,M,F), or NULL = density-only query: the feature head is NOT run */
    float* sigma;                /* out (G,M) raw density; empty_space_alpha outside the box */
    float* displacement;         /* out (G,M,3) or NULL; zeros outside the box / without a bender */
    int32_t* slot;               /* out (G,M) or NULL: compact row of the point, -1 = outside the box (as sample_slot) */
    int32_t* counters;           /* out [2] or NULL: rows sent through the backbone, rows sent through the feature head */
} pr_query_t;
/* Workspace bytes of the query (host computation, no device work). */
int pr_query_workspace_size(const pr_query_t* q, const pr_object_model_t* model, size_t* bytes);
/* `packed`: pr_pack_model(model, q->precision, ...).  `workspace`: 256-byte aligned, pr_query_workspace_size bytes.  Kernel launches on
 * `stream` only (every fill is a kernel): capturable into a HIP graph. */
int pr_query_field(const pr_query_t* q, const pr_object_model_t* model, const void* packed,
                   void* workspace, size_t workspace_bytes, void* stream);

/*
 * Kernel timing for bench.py: while enabled, the launches of the dominant kernels are bracketed by
 * hipEventRecord on the launch stream.  Categories: 0 = fused MLP (k_mlp_mfma / k_mlp_split / k_mlp_head),
 * 1 = forward compositing (k_composite), 2 = backward dX products (k_gemm_nn), 3 = backward dW products
 * (k_gemm_tn + its reduction), 4 = backward compositing (k_composite_bwd), 5 = the front and back end of pr_query_field
 * (k_query_count + block scan + k_query_fill, k_query_scatter; its MLP launch counts as 0), 6 = hierarchical resampling (k_resample with
 * the fill of its block sums), 7 = compaction launched per object (k_fill: the fine level, and the coarse level of calls that place
 * their objects one by one).
 * pr_profile_collect synchronises the recorded events, returns the summed milliseconds and launch
 * counts per category (host arrays of PR_PROFILE_CATEGORIES) and clears the list.
 */
#define PR_PROFILE_CATEGORIES 8
int pr_profile_enable(int enable);
int pr_profile_collect(double* milliseconds, int32_t* launches);

/*
 * Measures the fp32 matrix-core rate this device sustains: every CU runs 8 waves of dependent
 * v_mfma_f32_32x32x2_f32 chains (2 accumulators per wave, the occupancy of the renderer's MLP kernel)
 * for `iterations` x 8 MFMAs; returns TFLOP/s from HIP events.  SYNCHRONISES the stream (probe only).
 * random_operands != 0 feeds full-range pseudo-random mantissas that change every iteration (the
 * chip sustains a lower matrix rate on such data than on constant operands).
 */
int pr_probe_mfma_f32(int32_t iterations, int32_t random_operands, double* tflops, double* milliseconds, void* stream);
/* Same for the fp16 matrix cores with the split-precision kernel's issue pattern (4 accumulators, 6
 * v_mfma_f32_32x32x16_f16 per step); TFLOP/s counts hardware fp16 FLOPs (3 per emulated fp32 FLOP). */
int pr_probe_mfma_f16(int32_t iterations, int32_t random_operands, double* tflops, double* milliseconds, void* stream);

/*
 * Adam / AdamW update of ONE flat fp32 tensor in place - the arena every trainable parameter of the renderer is a view of
 * (parallel.flatten_parameters).  Replaces, for that tensor, the optimiser step of the reference's trainers
 * (torch.optim.Adam built at /root/reference/training/trainer.py:62-75 and stepped at :207-216): torch's fused multi-tensor
 * kernel deals one block per 65 536 elements (32 blocks for the 2.1 M parameters of the minecraft renderers: 0.10 ms);
 * this launch covers the tensor with one thread per four elements.  Arithmetic and update order of torch.optim.Adam
 * (amsgrad = False): see csrc/optim.hip.  `step` = the step count AFTER this update (>= 1), by value; or `step_device`
 * != NULL: a device float holding the count BEFORE the update, incremented on the stream first (optimisers recorded into a
 * HIP graph).  grad_scale / found_inf: optional device floats of torch.amp.GradScaler (NULL: plain update).
 */
int pr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int32_t decoupled_weight_decay, int32_t maximize, double step, float* step_device,
                 const float* grad_scale, const float* found_inf, void* stream);

/*
 * Node census of a recorded HIP graph: counts[0] = all nodes, [1] = kernel nodes, [2] = memset nodes, [3] = memcpy nodes
 * (child graphs included).  `graph` is a hipGraph_t (torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph()).  Host-only: no
 * launch, no synchronisation.  Why it exists: on ROCm 7.0.2 with the runtime's AQL packet capture the MEMSET nodes of a
 * replayed graph stop executing once the host has synchronised between replays (torch's multi-block reductions zero their
 * semaphores with one).  This library never records a memset (every zero fill is a kernel), but the automatic evaluation-frame
 * recording of the host side (EnvironmentModel.frame_replay, the drop-in for model/environment_model.py:581-651) also records
 * whatever encoder / decoder modules the caller injected - a recording with memset nodes is only replayed when the runtime
 * switch DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 is set, otherwise the call stays eager.
 */
int pr_graph_node_census(void* graph, int32_t* counts);

/* Library / device introspection. */
int pr_abi_version(void);
const char* pr_last_error(void);
int pr_device_info(int32_t* compute_units, int32_t* lds_bytes, char* arch_name, size_t arch_name_len);

#ifdef __cplusplus
}
#endif
#endif /* PLAYRENDER_H */
