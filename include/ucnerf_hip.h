/*
 * ucnerf_hip.h -- C ABI of libucnerf_hip.so: the MI355X (gfx950) implementation of UC-NeRF's
 * ray-marching volume-render hot path.
 *
 * The reference (wrld/UC-NeRF) is pure Python/PyTorch and has no FFI of its own; each entry point below
 * replaces one torch-op sequence of the reference's hot path (file:line cited per function, paths relative
 * to the reference tree).  A binding for any host language only needs this header: plain pointers and
 * sizes, no torch types.  The Python host side in uc_nerf_amd/ binds it with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the field name ends in _host;
 *   - all arrays are dense, row-major, float32 unless stated; index outputs are int64 (as torch's);
 *   - every function is asynchronous on `stream` (a hipStream_t passed as void*), allocates nothing,
 *     is re-entrant, and returns 0 on success or a negative UCNERF_E* code; ucnerf_last_error() returns
 *     a thread-local description of the last failure;
 *   - arguments are checked before anything is launched: a NULL params pointer, a NULL required array, a size outside the documented range and a
 *     NEGATIVE count are UCNERF_EINVAL; a count of ZERO rays / samples / rows is an empty batch -- success, nothing launched, no pointer read
 *     (torch hands empty tensors to the reference's functions the same way);
 *   - "sample" = one depth sample on one ray; M = N_rays * S samples, ray-major (sample s of ray r at
 *     index r*S + s).
 */
#ifndef UCNERF_HIP_H
#define UCNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UCNERF_ABI_VERSION 6

#define UCNERF_OK 0
#define UCNERF_EINVAL (-1)   /* bad argument (null pointer, unsupported size/config) */
#define UCNERF_EHIP (-2)     /* HIP runtime error at launch */

const char* ucnerf_last_error(void);
int ucnerf_abi_version(void);
/* sizeof() of a params struct by name ("ucnerf_mlp_params", ...), -1 if unknown: lets a binding check its mirror. */
int ucnerf_sizeof(const char* struct_name);
/* Number of compute units of the current device (grid sizing for persistent kernels); <0 on error. */
int ucnerf_device_cus(void);
/* The compile-time parameters this binary was built with, as "NAME=value NAME=value ..." (structural parameters of the kernels:
 * UCNERF_BF16_BW, UCNERF_BF16_NBUF, UCNERF_MLP_WAVES, UCNERF_CHAIN_WAVES, ...; the wrong-result timing switches of rounds 1-3 were taken out of
 * the sources in round 4).  The host side checks the production values (tests/test_abi_host.py). */
const char* ucnerf_build_flags(void);
/* Diagnostics: how many ucnerf_render_fused_fwd calls of this process let the gather-fused launch composite (and re-sample) its rays in its own
 * tail instead of launching K7 / K8 / K9 behind it -- passes of at most three rounds of 32-sample tiles, derived or given coordinates, any number of
 * samples per ray up to 256 (csrc/render.hip: tail_fits; the
 * outputs are bit-identical either way).  The environment variable UCNERF_FUSED_TAIL=0 (read once, at the first use) starts the process with
 * that route off; ucnerf_set_fused_tail(0 / 1) switches it at run time and returns the previous setting (thread-safe). */
int64_t ucnerf_fused_tail_launches(void);
int32_t ucnerf_set_fused_tail(int32_t on);
/* 1 when a pass of n rays x S samples is of the size that takes that route on the current device (the other conditions are the caller's to know:
 * gather-fused precision, fp32 channel-last sources, no max_blocks).  A host uses it to decide whether to hand the pass its ray
 * generation too (gen_rays / gen_depths): on the tail route the blocks generate their own rays at no measurable cost. */
int32_t ucnerf_fused_tail_fits(int32_t n, int32_t S);
/* The same for a COARSE pass that also draws the next pass's n_samples depths (ucnerf_render_params.resample): the library's own decision for
 * that pass (size AND the re-sampling limits: S - 1 <= 128 bins, S + n_samples <= 512), so that a host that folds the ray generation into the
 * pass exactly when it takes the tail route decides as the library does (round 4's advisor finding). */
int32_t ucnerf_fused_tail_fits_resample(int32_t n, int32_t S, int32_t n_samples);
/* Should a fine pass of n rays take its n_coarse coarse depths' network outputs from the coarse pass and evaluate the n_fine new depths only
 * (ucnerf_composite_merged_fwd composites the two row sets)?  1, except where the pass over all n_coarse + n_fine depths is of the size that
 * takes the tail route above: that pass is one launch already, and the reuse would put a compositing launch back behind it.  Like
 * ucnerf_fused_tail_fits it speaks of the size alone; with the tail route switched off it is 1 at every size. */
int32_t ucnerf_reuse_coarse_pays(int32_t n, int32_t n_coarse, int32_t n_fine);
/* Digest of the sources, headers and flags this binary was linked from (uc_nerf_amd/build.py: source_hash()): a host can tell a library
 * that does not belong to the tree it sits in (tests/test_abi_host.py), and __graft_entry__.build() rebuilds one that was not linked on
 * the machine it runs on. */
const char* ucnerf_source_hash(void);
/* HIP timing events for measuring kernels inside a call chain (bench harness): create / record on a stream /
 * elapsed milliseconds between two recorded events (waits for `stop`) / destroy. */
void* ucnerf_event_create(void);
int ucnerf_event_record(void* event, void* stream);
int ucnerf_event_elapsed_ms(void* start, void* stop, float* ms_host);
int ucnerf_event_destroy(void* event);

/* ------------------------------------------------------------------------------------------------
 * a1  ray generation -- data/ray_utils.py:12-53, utils/utils.py:217-271 (get_rays_mvs, deterministic and
 *     given-pixel branches), utils/run_nerf_helpers.py:248-257 (OpenGL variant).
 *     d_cam = ((x-K02)/K00, (y-K12)/K11, 1)  [opengl: ((x-W/2)/f, -(y-H/2)/f, -1)],  rays_d = d_cam @ R^T.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n;            /* rays to generate */
    int32_t H, W;         /* image size (grid mode / opengl) */
    int32_t grid_start;   /* grid mode (xs == NULL): first flattened row-major pixel index */
    int32_t opengl;       /* 0: intrinsic-matrix +z convention, 1: single-focal -z convention */
    float K[9];           /* 3x3 intrinsics, row-major (opengl: K[0] = focal) */
    float c2w[12];        /* 3x4 camera-to-world, row-major */
    const float* xs;      /* [n] pixel columns, or NULL for grid mode */
    const float* ys;      /* [n] pixel rows */
    float* rays_d;        /* [n,3] out */
    float* rays_o;        /* [n,3] out or NULL (origin is c2w[:,3] for every ray) */
    float* pix;           /* [2,n] out (row, col) or NULL */
    float w2c_dir[12];    /* with `angle`: rotation of the view-direction feature (see ucnerf_dir_feature) */
    float* angle;         /* [n,3] out or NULL: (d/|d|) @ R_dir^T of the generated rays, same values as ucnerf_dir_feature
                             on rays_d with has_ref = 1 -- saves that launch in the render passes (ucnerf_render_params.dir_feat) */
} ucnerf_ray_gen_params;
int ucnerf_ray_gen(const ucnerf_ray_gen_params* p, void* stream);

/* a2  LLFF NDC warp of rays -- data/ray_utils.py:56-94 (variant 0: focal[2], d2 = 1-o2),
 *     utils/run_nerf_helpers.py:277-294 (variant 1: scalar focal, d2 = -2 near/o_z). */
typedef struct {
    int32_t n, H, W, variant;
    float focal_x, focal_y, near;
    const float* rays_o;  /* [n,3] */
    const float* rays_d;  /* [n,3] */
    float* out_o;         /* [n,3] */
    float* out_d;         /* [n,3] */
} ucnerf_ndc_rays_params;
int ucnerf_ndc_rays(const ucnerf_ndc_rays_params* p, void* stream);

/* view-direction feature of rendering() -- network/renderer.py:232-238,163-174:
 *   cos = |d|,  angle = (d/cos) @ R_ref^T   (R_ref == NULL: angle = d/cos). */
typedef struct {
    int32_t n;
    int32_t has_ref;
    int32_t repeat;       /* 0/1: angle is [n,3]; S > 1: every ray's row is written S times -> [n*S,3] (per-sample form) */
    float w2c_ref[12];
    const float* rays_d;  /* [n,3] */
    float* angle;         /* [n,3] (or [n*repeat,3]) out */
    float* cos_angle;     /* [n] out or NULL */
    const float* w2c_ref_dev; /* optional DEVICE pointer to the same matrix, row-major with 4 columns (a 3x4 or 4x4 tensor): used
                                 instead of w2c_ref when non-NULL (has_ref is then implied), so that a caller holding the pose
                                 on the device -- rendering() gets pose_ref['w2cs'] as a device tensor -- need not read it back */
} ucnerf_dir_feature_params;
int ucnerf_dir_feature(const ucnerf_dir_feature_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a3  depth sampling -- data/ray_utils.py:152-197 (ray_marcher) and the live cascade sampler
 *     utils/utils.py:393-397,684-706 (three uniform sets, sorted, stratified).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, S;
    int32_t lindisp;
    float perturb;        /* > 0: z = lower + (upper-lower) * perturb * noise */
    float near, far;      /* used when rays == NULL: every ray samples [near, far] (pts must be NULL) */
    const float* rays;    /* [n,8] = (o, d, near, far), or NULL */
    const float* noise;   /* [n,S] uniform [0,1) draws, required when perturb > 0 */
    float* z;             /* [n,S] out */
    float* pts;           /* [n,S,3] out or NULL */
} ucnerf_sample_stratified_params;
int ucnerf_sample_stratified(const ucnerf_sample_stratified_params* p, void* stream);

/* a1 + a3 in one launch: the rays of ucnerf_ray_gen and their stratified depths (scalar near / far form: rays = pts = NULL) --
 * data/ray_utils.py:32-53 followed by :176-194, as ray_marcher chains them.  Same results as the two calls. */
int ucnerf_ray_gen_sample(const ucnerf_ray_gen_params* rays, const ucnerf_sample_stratified_params* depths, void* stream);

typedef struct {
    int32_t n, S;         /* S must be a multiple of 3, S <= 768 */
    const float* near_far;/* [n,6] = (near_1, far_1, near_2, far_2, near_3, far_3) per ray */
    const float* t_rand;  /* [n,S] uniform draws, or NULL for no jitter */
    const float* rays_o;  /* [3] shared origin, used when pts != NULL */
    const float* rays_d;  /* [n,3] */
    float* z;             /* [n,S] out (sorted then jittered) */
    float* pts;           /* [n,S,3] out or NULL */
} ucnerf_sample_cascade_params;
int ucnerf_sample_cascade(const ucnerf_sample_cascade_params* p, void* stream);

/* a1 + a3 + a4 of the EVALUATION loop in one launch (ABI v5) -- utils/utils.py:600-739 (build_rays_test), called once per 1024-pixel chunk by
 * train.py:251-256: rays through pixels grid_start .. grid_start + n - 1 of the flattened HxW grid (get_rays_mvs, isRandom=False), the three
 * per-ray cascade ranges read from the stages' depth hypotheses at (row, col) // (4, 2, 1) (first and last plane), 3 x S/3 uniform depths
 * sorted and stratified-jittered, the world points and their four normalised copies (get_ndc_coordinate).  Same values as ucnerf_ray_gen ->
 * ucnerf_sample_cascade -> ucnerf_ndc_project, bit for bit.  The camera matrices and the scene range are read from DEVICE memory -- the caller
 * holds them as device tensors, nothing is read back to the host per chunk. */
typedef struct {
    int32_t n, S;              /* rays of the chunk; samples per ray (multiple of 3, <= 768) */
    int32_t H, W, grid_start;
    int32_t dv_d[3], dv_h[3], dv_w[3];   /* sizes of depth_values[k] */
    const float* K;            /* [3,3] intrinsics of the rendered view (device) */
    const float* c2w;          /* [>=3,4] camera-to-world of the rendered view (device, rows 4 floats apart) */
    const float* w2c_ref;      /* [>=3,4] reference view (device) */
    const float* K_ref;        /* [3,3] (device) */
    const float* near_far_ref; /* [2] scene range (near, far) (device) */
    const float* depth_values[3];  /* [D_k,h_k,w_k] hypotheses of cascade stage k + 1 (device) */
    const float* t_rand;       /* [n,S] uniform draws, or NULL for no jitter */
    float* rays_o;             /* [3] out or NULL: c2w[:3,3] */
    float* rays_d;             /* [n,3] out */
    float* near_far;           /* [n,6] out or NULL: (near_1, far_1, near_2, far_2, near_3, far_3) per ray */
    float* z;                  /* [n,S] out */
    float* pts;                /* [n,S,3] out */
    float* ndc1;               /* [n,S,3] out: stage copies and the scene-normalised copy */
    float* ndc2;
    float* ndc3;
    float* ndc;
} ucnerf_build_rays_test_params;
int ucnerf_build_rays_test(const ucnerf_build_rays_test_params* p, void* stream);

/* a1 + a3 + a4 of the TRAINING step in one launch (added to ABI v6; nothing above moved) -- utils/utils.py:400-597 (build_rays) with the pixel
 * samplers it calls, :169-215 (get_rays_with_random_patches, confidence picks), :245-247 (get_rays_mvs, uniform pixels) and :304
 * (get_rays_mvs_coord): R = P ps^2 + n_uniform + n_coord rays, in the reference's order --
 *   rays 0 .. P/2 ps^2:   patch k = r / ps^2, row-major inside the patch: cell_r = clamp((sel0[k] / W) / ps, 0, H/ps - 2),
 *                         cell_c = clamp((sel0[k] % W) / ps, 0, W/ps - 2), row = cell_r ps + shift[k][0] + (r % ps^2) / ps,
 *                         col = cell_c ps + shift[k][1] + (r % ps^2) % ps (the clamp keeps a patch with shifts in [0, ps) inside the image);
 *   the next P/2 ps^2:    the same with sel1 and shift[P/2 + k];
 *   the next n_uniform:   (uy[i], ux[i]);
 *   the last n_coord:     (coords[i][0], coords[i][1]), rows coord_stride floats apart.
 * Per ray: the direction through the float pixel, the integer pixel by truncation (pix, what .long() gives), the colour imgs[0,0,:,row,col],
 * and from there what the evaluation builder above does -- the three ranges at (row, col) // (4, 2, 1) with each volume's own row width (a padded
 * stage-3 volume is indexed without an offset, as the reference does), the sorted and jittered depths, the world points and their four
 * normalised copies.  Same values as the per-segment ray_gen calls, torch indexing, sample_cascade and ndc_project, bit for bit.  The draws
 * (torch.multinomial, numpy's shifts, torch.randint, torch.rand) stay the caller's; sel0 / sel1 are what torch.multinomial returns on the device
 * and are never read back.  Index reads are clamped into the image: a pick, shift or coordinate outside it (the reference raises) cannot
 * fault, its values are unspecified.  UCNERF_EINVAL: a negative count, odd P, ps < 1, H / ps < 2 or W / ps < 2 with P > 0, S no multiple
 * of 3 or above 768, a depth_values[k] smaller than the image at its resolution, R S 3 or R 6 beyond int32, a NULL required array.  R = 0
 * is success, nothing launched; any segment may be empty (its arrays are then not read). */
struct ucnerf_build_rays_train_params {
    int32_t S;                 /* samples per ray (multiple of 3, <= 768) */
    int32_t H, W;
    int32_t P, ps;             /* patches (even: P/2 from each map), patch edge */
    int32_t n_uniform, n_coord;
    int32_t coord_stride;      /* floats between the rows of coords */
    int32_t dv_d[3], dv_h[3], dv_w[3];   /* sizes of depth_values[k] */
    int64_t img_stride_c, img_stride_h, img_stride_w;   /* ELEMENT strides of the channel, row and column axes of imgs */
    const float* K;            /* [3,3] intrinsics of the rendered view (device) */
    const float* c2w;          /* [>=3,4] camera-to-world of the rendered view (device, rows 4 floats apart) */
    const float* w2c_ref;      /* [>=3,4] reference view (device) */
    const float* K_ref;        /* [3,3] (device) */
    const float* near_far_ref; /* [2] scene range (near, far) (device) */
    const float* depth_values[3];  /* [D_k,h_k,w_k] hypotheses of cascade stage k + 1 */
    const float* imgs;         /* element (0, 0, 0) of the image imgs[0,0]: 3 channels x H x W under the strides above */
    const int64_t* sel0;       /* [P/2] flattened-pixel picks from the confidence map */
    const int64_t* sel1;       /* [P/2] picks from the uncertainty map */
    const int32_t* shift;      /* [P,2] (row, col) shift of each patch inside its cell */
    const float* ux;           /* [n_uniform] columns */
    const float* uy;           /* [n_uniform] rows */
    const float* coords;       /* [n_coord,2] (row, col) */
    const float* t_rand;       /* [R,S] uniform draws, or NULL for no jitter */
    float* rays_o;             /* [3] out: c2w[:3,3] */
    float* rays_d;             /* [R,3] out */
    float* colors;             /* [R,3] out */
    int64_t* pix;              /* [2,R] out (row, col) */
    float* near_far;           /* [R,6] out or NULL */
    float* z;                  /* [R,S] out */
    float* pts;                /* [R,S,3] out */
    float* ndc1;               /* [R,S,3] out: stage copies and the scene-normalised copy */
    float* ndc2;
    float* ndc3;
    float* ndc;
};
typedef struct ucnerf_build_rays_train_params ucnerf_build_rays_train_params;
int ucnerf_build_rays_train(const ucnerf_build_rays_train_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a4  world -> reference-view normalised coordinates -- utils/utils.py:323-373 (get_ndc_coordinate).
 *     p_cam = p R^T + T; |z|<1e-4 -> 1e-4; q = p_cam K^T; xy = q.xy/q.z / inv_scale;
 *     z_k = (q.z - near_k)/(far_k - near_k) for k in {stage1, stage2, stage3, ndc}.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t m;            /* points */
    int32_t has_w2c;
    int32_t sample_2d;    /* 1: write only out_ndc = (x, y, raw z) */
    int32_t nf_stride;    /* elements between consecutive points in near/far arrays: 1 (per point) or 0 (broadcast) */
    float w2c[12];
    float K[9];
    float inv_scale[2];   /* (W-1, H-1) */
    float near, far;      /* scene range for the 'ndc' copy */
    const float* pts;     /* [m,3] */
    const float* near_1; const float* far_1;   /* [m] (or [1] when nf_stride == 0) */
    const float* near_2; const float* far_2;
    const float* near_3; const float* far_3;
    float* out_stage1;    /* [m,3] */
    float* out_stage2;
    float* out_stage3;
    float* out_ndc;
} ucnerf_ndc_project_params;
int ucnerf_ndc_project(const ucnerf_ndc_project_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a5  positional encoding -- network/models.py:20-71 (layout 0, "live": [x | sin(2^k x) k<L | cos ...]),
 *     utils/run_nerf_helpers.py:23-71 (layout 1, interleaved [x | sin f0 | cos f0 | sin f1 ...]).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t m;            /* 3-vectors */
    int32_t n_freqs;
    int32_t layout;
    const float* x;       /* [m,3] */
    float* out;           /* [m, 3 + 6*n_freqs] */
} ucnerf_embed_params;
int ucnerf_embed(const ucnerf_embed_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ABI v5: the gather sources in the layout the fast kernels read ("channel-last": one voxel / pixel = contiguous channels), EACH IN ITS OWN
 * ALLOCATION -- what a producer's convolutions write when they run in torch's channels_last / channels_last_3d memory formats
 * (network/mvs_models.py:624-646: cost_regularization -> volume_feature_no_ref per stage, FeatureNet -> img_feats; new tensors every training
 * step, train.py:136-163), read IN PLACE.  ucnerf_gather_repack builds the same layouts from the reference's channel-major tensors for the
 * sources that are not handed over this way.
 *   vol[k]    [D,h,w,8]           = the memory of a [1,8,D,h,w] tensor in channels_last_3d            16-byte aligned
 *   img_feat  [V,H,W,8]           = a [V,8,H,W] tensor in channels_last                                16-byte aligned
 *   imgs      [V,H,W,rgb_stride]  rgb_stride = 3 (a [V,3,H,W] tensor in channels_last; 4-byte aligned) or 4 (r,g,b,pad: what the repack writes)
 * bf16 = 1: every array holds bf16 instead of fp32 (rgb_stride must be 4; SURVEY.md 8 configs[4] "bf16 features").
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const void* vol[3];
    const void* img_feat;
    const void* imgs;
    int32_t rgb_stride;
    int32_t bf16;
} ucnerf_cl_sources;
/* Gradients of the differentiable ones among them, in the same layouts (fp32, 16-byte aligned, ACCUMULATED into: zero them first); any may be NULL */
typedef struct {
    float* vol[3];      /* [D,h,w,8] */
    float* img_feat;    /* [V,H,W,8] */
} ucnerf_cl_grads;

/* ------------------------------------------------------------------------------------------------
 * a7  feature gather -- network/renderer.py:177-212 (gen_pts_feats) = utils/utils.py:833-893
 *     (index_point_feature: 3 trilinear volume lookups + bilinear confidence, align_corners=False, border)
 *     + utils/utils.py:742-799 (build_color_volume: per source view bilinear rgb + in-mask + 8-ch image
 *     features, align_corners=True, border).  Feature vector per sample, F = 24 + 12*V + 1:
 *       [0:8] stage1 | [8:16] stage2 | [16:24] stage3 | [24:24+4V] (r,g,b,mask) x V | [..+8V] img_feat x V | conf
 *     Sources are read in the reference's own layouts.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t m;                 /* samples */
    int32_t V;                 /* source views (reference view_num - 1), 1..8 */
    int32_t H, W;              /* image / confidence / img_feat size */
    int32_t vol_d[3], vol_h[3], vol_w[3];   /* cascade volume sizes, 8 channels each */
    int32_t out_tiled;         /* 0: feats [m,F] row-major; 1: [ceil(m/32)][F][32] (MLP tile layout) */
    int32_t unit_mask;         /* 0 = everything; else bit k selects unit k: 0..2 cascade volumes, 3 confidence,
                                  4+i source view i (rgb+mask and image features).  Sources of unselected units may be NULL. */
    const float* pts;          /* [m,3] world points */
    const float* ndc1;         /* [m,3] stage coordinates in ~[0,1] (ucnerf_ndc_project outputs) */
    const float* ndc2;
    const float* ndc3;
    const float* vol[3];       /* [8,D,h,w] */
    const float* conf;         /* [H,W] */
    const float* imgs;         /* [V,3,H,W] */
    const float* img_feat;     /* [V,8,H,W] */
    const float* w2cs;         /* [V,12] rows 0..2 of each 4x4 */
    const float* intrinsics;   /* [V,9] */
    float* feats;              /* out */
    float* u_out;              /* optional [m] out: the per-sample uncertainty u = 1 - (sampled confidence) that the MLP
                                  blends its two heads with (network/models.py:149); written by the confidence unit */
} ucnerf_feat_gather_params;
int ucnerf_feat_gather_fwd(const ucnerf_feat_gather_params* p, void* stream);

/* Backward of the gather w.r.t. its differentiable sources (the reference's autograd reaches the three
 * volumes, img_feat and confidence through grid_sample; positions and images get no gradient,
 * SURVEY.md 3.2).  Gradients are ACCUMULATED (atomic add) into the g_* buffers: zero them first. */
typedef struct {
    ucnerf_feat_gather_params fwd;   /* same geometry/inputs as the forward call (feats unused) */
    const float* g_feats;            /* [m,F] row-major upstream gradient */
    float* g_vol[3];                 /* [8,D,h,w] or NULL to skip */
    float* g_conf;                   /* [H,W] or NULL */
    float* g_img_feat;               /* [V,8,H,W] or NULL */
    float* scratch;                  /* optional, ucnerf_feat_gather_bwd_scratch_floats() floats, 16-byte aligned: the
                                        volume / image-feature gradients are then accumulated channel-LAST in it (eight
                                        lanes add the 32 contiguous bytes of one corner instead of eight scattered
                                        cache lines) and added to g_vol / g_img_feat by a transposing pass.  Contents
                                        are overwritten.  NULL: atomics go straight to the channel-major outputs. */
    ucnerf_cl_grads g_cl;            /* ABI v5, per source: a gradient array in the CHANNEL-LAST layout of ucnerf_cl_sources.  A source whose entry is
                                        set has its gradient ACCUMULATED there (zero it first) and its g_vol[k] / g_img_feat entry is ignored: no
                                        scratch, no memset, no transposing pass for it -- for callers whose sources live channel-last
                                        (ucnerf_render_params.cl handed over in place).  Entries left NULL take the route above. */
} ucnerf_feat_gather_bwd_params;
int ucnerf_feat_gather_bwd(const ucnerf_feat_gather_bwd_params* p, void* stream);
int64_t ucnerf_feat_gather_bwd_scratch_floats(const ucnerf_feat_gather_params* p);

/* ------------------------------------------------------------------------------------------------
 * a6 (+a5 fused)  the uncertainty-conditioned MLP -- network/models.py:138-184 driven by
 *     network/renderer.py:78-106 (run_network_mvs; batchify's netchunk loop is unnecessary here).
 *     Fixed architecture: D=6, W=128, skip after layer 4, multires 10 / 4 (63 + F + 27 inputs).
 *     Weights are consumed as a pre-packed MFMA operand stream built by ucnerf_mlp_pack from the flat
 *     parameter vector (concatenation of the reference state_dict tensors in state_dict order).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_src;        /* V = view_num - 1 */
    int32_t pe_layout;    /* 0 live (network/models.py), 1 interleaved (run_nerf_helpers.py) */
    int32_t precision;    /* 0: f32 -- exact fp32 MFMA (v_mfma_f32_32x32x2_f32); forward, backward, every input mode.
                             1: bf16x3 -- every product as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on the bf16 matrix cores
                                (v_mfma_f32_32x32x16_bf16, fp32 accumulate): inference forward only; rendered outputs
                                stay within 1e-5 of fp64 (the parity bar is 1e-4), ~2.9x the f32 throughput.
                             2: bf16 -- the hi*hi term only (plain bf16 operands, fp32 accumulate; same packed stream as 1):
                                inference forward only, NOT within the 1e-4 parity bar (rendered error ~3e-3, > 50 dB PSNR
                                against the f32 render); offered because the reference configuration names bf16.
                             3: bf16x3 with the feature gather INSIDE the MLP kernel: the stream is packed in the
                                order that kernel's lane halves produce the bias nets' operands and serves ucnerf_render_fused_fwd
                                only (channel-last sources, coordinates derived from (ray, depth) or handed over -- pts_in ... ndc_in --,
                                no kept features, no per-sample uncertainty); ucnerf_mlp_fwd refuses it.  Same arithmetic as 1. */
    int32_t operand;      /* (ABI v6) the 16-bit terms of precisions 1 .. 3 -- the packed stream and the kernels that read it must agree:
                             0: bf16 (8 significant bits per term; any float32 range).  The default.
                             1: fp16 (v_mfma_f32_32x32x16_f16: 11 significant bits per term at the same matrix-core rate, so the three-product
                                split holds ~22 bits -- rendered outputs at float32 level where the bf16 split is at 16 .. 17 bits).  fp16's RANGE
                                is the price.  ACTIVATIONS are converted toward zero, so one beyond 131 008 is clamped -- finite, but wrong
                                (float32 itself resolves no more than 1e-2 of it) -- and never becomes an infinity.  That holds for the activation
                                side ONLY: a WEIGHT beyond 65 504 is packed as hi = inf, lo = -inf and its products are NaN (the packers round to
                                nearest and do not clamp).  A term below 6e-5 is held with an absolute resolution of 3e-8.  None of this is reported
                                by these calls; the guarded calls below (ucnerf_*_guarded) detect the overflow side on the device.  Inference forward
                                only (ucnerf_mlp_fwd_train refuses it).  Ignored by precision 0. */
} ucnerf_mlp_config;

/* Sizes: floats in the flat parameter vector, floats (4-byte units) of the packed stream, int32 entries of the pack
 * index (<0 on bad config).  Stream and index depend on cfg.precision. */
int64_t ucnerf_mlp_param_count(const ucnerf_mlp_config* cfg);
int64_t ucnerf_mlp_stream_count(const ucnerf_mlp_config* cfg);
int64_t ucnerf_mlp_index_count(const ucnerf_mlp_config* cfg);
/* Host-side: fills idx_host[index_count] with the flat-parameter index feeding each stream element (-1 = zero pad;
 * bf16x3: bit 30 selects the low part of the split). */
int ucnerf_mlp_pack_index(const ucnerf_mlp_config* cfg, int32_t* idx_host);
/* Device-side: builds the packed stream from the flat parameters; idx is the device copy of the table above. */
int ucnerf_mlp_pack(const ucnerf_mlp_config* cfg, const float* flat_params, const int32_t* idx, float* stream_out, void* stream);
/* The same from parameters that live in SEPARATE device tensors (a torch module's, in state_dict order: their concatenation is the flat
 * vector), without first concatenating them: tensor_ptrs_host / tensor_numel_host are HOST arrays of n_tensors (<= 48) device pointers
 * and element counts.  Lets a drop-in re-pack from the live parameters in every call -- in-place writes through `.data` (the reference's
 * own weights_init, network/models.py:15-17) leave no trace a cache could key on. */
int ucnerf_mlp_pack_tensors(const ucnerf_mlp_config* cfg, int32_t n_tensors, const void* const* tensor_ptrs_host, const int64_t* tensor_numel_host,
                            const int32_t* idx, float* stream_out, void* stream);
/* Transpose of the pack for gradients: g_flat[idx[i]] += g_stream[i] (g_flat zeroed by the caller). */
int ucnerf_mlp_unpack_grad(const float* g_stream, const int32_t* idx, float* g_flat, int64_t n, void* stream);

typedef struct {
    ucnerf_mlp_config cfg;
    int32_t m;                 /* samples */
    int32_t S;                 /* samples per ray (view dir of sample s is dirs[s / S]); dirs_per_sample: ignored */
    int32_t dirs_per_sample;   /* 1: dirs is [m,3] */
    int32_t feats_tiled;       /* feats layout, see ucnerf_feat_gather_params.out_tiled */
    int32_t max_blocks;        /* 0 = auto (persistent grid sized from the CU count) */
    int32_t encoded;           /* 1: pts / dirs rows already hold the 63 / 27 encoded values (cfg.pe_layout order), as in
                                  UCNeRF.forward(x) of the reference; implies dirs_per_sample, row-major feats */
    int32_t pts_stride;        /* floats between consecutive rows of pts / dirs / row-major feats; 0 = dense (3 or 63, */
    int32_t dirs_stride;       /*   3 or 27, F).  Lets all three point into one [m, 63+F+27] matrix. */
    int32_t feat_stride;
    const float* pts;          /* [m,3] the 'ndc' coordinates fed to the positional encoding */
    const float* dirs;         /* [m/S,3] or [m,3] view-direction feature */
    const float* feats;        /* [m,F] or tiled */
    const float* wstream;      /* packed weights (ucnerf_mlp_pack) */
    float* raw;                /* [m,4] out: rgb (after sigmoid), sigma (after relu) */
} ucnerf_mlp_params;
int ucnerf_mlp_fwd(const ucnerf_mlp_params* p, void* stream);

/* The guarded fp16 split (additive to ABI v6: no struct changes; the guard is a property of the CALL, cfg.operand stays 0 / 1).
 *
 * `status` / `run_if` is one 4-byte-aligned 32-bit word in DEVICE memory, owned, zeroed and kept alive by the caller.  The library only ever ORs
 * bits into it (vector-memory atomics) -- it is sticky until the caller clears it:
 *     bit 0: a guarded forward formed an fp16 hi term of magnitude 65 504 from an activation or input (any |x| >= 65 504, infinities and NaNs
 *            included).  Conservative: values are only clamped from 131 008 on; flagging early costs a replay, never a wrong result.
 *     bit 1: a guarded pack met a weight whose fp16 hi term is not finite or reaches 65 504.
 * What is NOT detected: terms below 6e-5 (fp16's subnormal side) lose relative precision exactly as with the unguarded fp16 terms; they stay within
 * the absolute parity bar and raise no flag.
 *
 * ucnerf_*_guarded: the call of the same name on fp16 terms (cfg.operand must be 1, precision 1 .. 3) with range detection; same outputs, bit for bit,
 *     as the unguarded call.  Nothing is written to `status` when nothing left the range.
 * ucnerf_*_if: the call of the same name (any operand; in practice 0, bf16 terms) whose MLP / pack kernels first read *run_if and do nothing when it
 *     is zero: enqueued directly behind the guarded call of the same pass, with run_if = status and a bf16-term stream, it re-renders the pass on
 *     bf16 terms exactly when something saturated -- no host synchronisation.  The result is then bit-identical to the plain bf16-term call, else
 *     to the plain fp16-term call.  ucnerf_render_fused_fwd_if repeats the whole pass from the same inputs: its launches around the MLP (direction
 *     features, gather, compositing, re-sampling) are not conditional and rewrite the values already there when the MLP launch was skipped; it
 *     records no events.
 * A null word is UCNERF_EINVAL, like a negative count.  Inference forward only. */
int ucnerf_mlp_fwd_guarded(const ucnerf_mlp_params* p, uint32_t* status, void* stream);
int ucnerf_mlp_fwd_if(const ucnerf_mlp_params* p, const uint32_t* run_if, void* stream);
int ucnerf_mlp_pack_guarded(const ucnerf_mlp_config* cfg, const float* flat_params, const int32_t* idx, float* stream_out, uint32_t* status, void* stream);
int ucnerf_mlp_pack_if(const ucnerf_mlp_config* cfg, const float* flat_params, const int32_t* idx, float* stream_out, const uint32_t* run_if, void* stream);
int ucnerf_mlp_pack_tensors_guarded(const ucnerf_mlp_config* cfg, int32_t n_tensors, const void* const* tensor_ptrs_host, const int64_t* tensor_numel_host,
                                    const int32_t* idx, float* stream_out, uint32_t* status, void* stream);
int ucnerf_mlp_pack_tensors_if(const ucnerf_mlp_config* cfg, int32_t n_tensors, const void* const* tensor_ptrs_host, const int64_t* tensor_numel_host,
                               const int32_t* idx, float* stream_out, const uint32_t* run_if, void* stream);

/* Backward (autograd of network/models.py:138-184): re-runs the forward keeping the per-layer activations (unless
 * saved_valid), then walks the layers backwards (bwd_mode).  Produces d(feats) and ACCUMULATES the parameter gradients
 * into g_flat, a vector laid out exactly like the flat parameter vector (zero it first).  The three parameter
 * sets the reference never uses (pts_bias_confidence_1, feature_linear_1, confi_linear) get no contribution.
 * Positions and view directions receive no gradient (the reference path is non-differentiable there).
 *
 * READABLE EXTENT.  bwd_mode 0 forms every parameter gradient in one launch that fetches its fp32 row operands in 16-byte pieces: four columns,
 * starting at a column that is a multiple of four, from rows that need only be 4-byte aligned.  A piece that reaches past the operand's last
 * column is fetched whole and the lanes outside the operand are replaced by zero bits before use (selected, not multiplied: whatever is read
 * there, a NaN pattern included, reaches no result), but the bytes must be READABLE:
 *     fwd.encoded = 1:  the 63 encoded point columns are read as 16 pieces, the 27 direction columns as 7 -- the last piece of a row ends ONE
 *         float behind it.  Inside a [m, 63+F+27] matrix that float is the next column or the next row; behind the last row of `dirs` (the
 *         end of that matrix) and behind the last row of a separate `pts` buffer it lies outside the rows: 4 readable bytes are required
 *         behind row m-1 of `pts` and of `dirs` (the torch wrapper copies x into a buffer four floats longer).
 *     fwd.encoded = 0:  pts / dirs are encoded into the workspace first (rows padded to 64 / 32 floats there): nothing is read behind them,
 *         and pts_stride / dirs_stride must be 0 or 3.
 *     feats, row-major: the pieces cover columns [0, 24+4V) and [24+4V, 24+12V), both whole pieces: nothing is read behind column F-1, whatever
 *         feat_stride.  feats, tile layout: whole tiles are read, the padding rows of the last tile included (they belong to the layout:
 *         ceil(m/32)*32*F floats); their values reach no result.
 *     g_raw, flat_params, wstream: read exactly.  The workspace is read only where the call (or ucnerf_mlp_fwd_train) wrote it: it may hold
 *         anything on entry, apart from the activations under saved_valid = 1.
 * bwd_mode 1 reads single elements of every operand: no bytes outside the rows described here.  Neither mode writes outside g_feats' F columns per
 * row, g_flat's param_count floats and the workspace's ucnerf_mlp_bwd_workspace_floats() floats. */
typedef struct {
    ucnerf_mlp_params fwd;     /* forward arguments (feats row-major [m,F], or tiled with bwd_mode 0); raw is not written */
    const float* g_raw;        /* [m,4] upstream gradient */
    const float* flat_params;  /* [param_count] the parameters the wstream was packed from */
    float* g_feats;            /* [m,F] out, rows g_feat_stride floats apart (every one of the F columns written) */
    int32_t g_feat_stride;     /* 0 = F */
    float* g_flat;             /* [param_count] accumulated */
    float* workspace;          /* scratch, ucnerf_mlp_bwd_workspace_floats() floats, 16-byte aligned: kept activations, gradient sets, and the
                                  state of the two merges, which the call zeroes itself -- bwd_mode 0: the weight-gradient launch's 16 chunk
                                  counters; bwd_mode 1: the head kernel's arrival counter, behind its 256 rows of 1032 block sums (about 264 k
                                  floats of the workspace whatever m is).  ONE WORKSPACE PER CALL IN FLIGHT, in either mode: two calls that
                                  share one corrupt each other's merge */
    int32_t saved_valid;       /* 1: `workspace` already holds the activations of THIS forward, written by
                                  ucnerf_mlp_fwd_train with the same arguments -- the backward then skips its own forward */
    int32_t bwd_mode;          /* 0: register-resident gradient chain (ONE kernel walks the network backwards per 32-sample tile, data
                                  gradients as split-bf16 products on the matrix cores, fp32 accumulate: 2^-16 relative) + one
                                  weight-gradient GEMM per layer;  1: layer-by-layer exact-fp32 data-gradient GEMMs (round 1/2 path) */
} ucnerf_mlp_bwd_params;
int64_t ucnerf_mlp_bwd_workspace_floats(const ucnerf_mlp_config* cfg, int32_t m);
int ucnerf_mlp_bwd(const ucnerf_mlp_bwd_params* p, void* stream);
/* Training forward: ucnerf_mlp_fwd (f32 or bf16x3 precision, features row-major or tiled) that also keeps the per-layer activations in `bwd_workspace`
 * (ucnerf_mlp_bwd_workspace_floats floats), for a following ucnerf_mlp_bwd with saved_valid = 1 and THE SAME bwd_mode: for bwd_mode 0 the ten
 * [m,128] sets are kept as 24-bit floats (sign, exponent, 15 mantissa bits: the 16 significant bits the chain's and the weight-gradient launch's
 * split-bf16 operands carry -- three quarters of the bytes every kernel of the step moves), for bwd_mode 1 as fp32. */
int ucnerf_mlp_fwd_train(const ucnerf_mlp_params* p, float* bwd_workspace, int32_t bwd_mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a9  alpha compositing -- network/renderer.py:25-36,109-140 (variant 0 "live": alpha = 1-exp(-sigma),
 *     rgb/sigma already activated, dists ignored) and utils/run_nerf_helpers.py:343-390 (variant 1:
 *     alpha = 1-exp(-relu(sigma+noise)*dists), rgb = sigmoid(raw), dists = dz*|d|, last = 1e10).
 *     T_i = prod_{j<i} (1-alpha_j+1e-10), w = alpha*T.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, S;
    int32_t variant;
    int32_t white_bkgd;
    const float* raw;      /* [n,S,4] */
    const float* z;        /* [n,S] */
    const float* rays_d;   /* [n,3]  (variant 1) */
    const float* noise;    /* [n,S] or NULL (variant 1) */
    float* rgb_map;        /* [n,3] */
    float* depth_map;      /* [n] */
    float* acc_map;        /* [n] or NULL */
    float* disp_map;       /* [n] or NULL */
    float* weights;        /* [n,S] or NULL */
    float* var;            /* [n] unbiased variance of the weights, or NULL (variant 0 only) */
    const float* u;        /* optional [n,S] per-sample uncertainty (ucnerf_feat_gather_params.u_out) ... */
    float* wu;             /* ... and [n] out: sum_i w_i u_i, the composited uncertainty of the ray (a build extra: the
                              reference keeps u per sample only, network/models.py:149,177-178) */
} ucnerf_composite_params;
int ucnerf_composite_fwd(const ucnerf_composite_params* p, void* stream);

typedef struct {
    ucnerf_composite_params fwd;   /* inputs as in the forward call; outputs unused */
    const float* g_rgb;        /* [n,3] or NULL */
    const float* g_depth;      /* [n] or NULL */
    const float* g_acc;        /* [n] or NULL */
    const float* g_weights;    /* [n,S] or NULL */
    float* g_raw;              /* [n,S,4] out */
} ucnerf_composite_bwd_params;
int ucnerf_composite_bwd(const ucnerf_composite_bwd_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a8  inverse-CDF sampling -- data/ray_utils.py:98-141 == utils/run_nerf_helpers.py:298-341, with the
 *     uniform draws u given, and the sorted merge of data/ray_utils.py:219.
 *     Reproduces torch-CPU's accumulation orders (vectorised row sum, float64 cumsum) so that
 *     inds == torch.searchsorted(cdf, u, right=True) bit for bit.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n;
    int32_t n_bins;        /* L = bins per ray; weights per ray = L-1; 2 <= L <= 1024 */
    int32_t n_samples;     /* M draws per ray, M <= 1024 */
    int32_t u_stride;      /* n_samples (per-ray draws) or 0 (one shared row, e.g. linspace) */
    int32_t n_merge;       /* z_merge entries per ray (0: no merge), n_merge + M <= 2048 */
    int32_t from_coarse;   /* 1: the hierarchical recipe of data/ray_utils.py:216-217 in one call -- z_merge holds the
                              coarse depths z[n,S], weights the coarse weights w[n,S]; bins = .5*(z[:-1]+z[1:]) (so
                              n_bins = S-1) and the pdf uses w[:, 1:-1].  bins may then be NULL. */
    const float* bins;     /* [n,L] */
    const float* weights;  /* [n,L-1]  (from_coarse: [n,S]) */
    const float* u;        /* [n,M] or [M] */
    const float* z_merge;  /* [n,n_merge] values to merge with the samples, or NULL */
    float* samples;        /* [n,M] out or NULL */
    int64_t* inds;         /* [n,M] out or NULL */
    float* cdf;            /* [n,L] out or NULL */
    float* z_sorted;       /* [n,n_merge+M] out: sort(cat(samples, z_merge)), or NULL */
    int32_t* merge_rank;   /* [n,M+n_merge] out or NULL (needs z_sorted): position in z_sorted of element i of
                              cat(samples, z_merge) -- the permutation of that sort, for ucnerf_merge_rows */
} ucnerf_sample_pdf_params;
int ucnerf_sample_pdf(const ucnerf_sample_pdf_params* p, void* stream);

/* a9 of the coarse pass + a8 in ONE launch -- network/renderer.py:109-140 followed by data/ray_utils.py:216-219, as the hierarchical renderer
 * chains them (data/ray_utils.py:199-224): the wave that composites a ray re-samples it from the weights it has just computed.  `c` is the
 * compositing call (live variant, no uncertainty inputs), `s` the re-sampling in its from_coarse form with n == c->n, n_merge == c->S,
 * n_bins == c->S - 1 and 3 <= c->S <= 1024 (the limit of ucnerf_composite_fwd); s->weights is ignored (the composite's weights, also written to c->weights when that is non-NULL) and s->z_merge, when
 * given, must equal c->z.  Results are those of ucnerf_composite_fwd(c) followed by ucnerf_sample_pdf(s with weights = c->weights), bit for bit. */
int ucnerf_composite_sample_pdf(const ucnerf_composite_params* c, const ucnerf_sample_pdf_params* s, void* stream);

/* Applies the permutation of a sorted merge to per-sample rows: out[r][rank[r][i]] = cat(a[r], b[r])[i].
 * Lets the fine pass of the hierarchical renderer (data/ray_utils.py:199-224) evaluate the network on the NEW depths
 * only and take the coarse depths' outputs from the coarse pass: the merged rows are bit-identical to re-evaluating
 * all of them, because a sample's network output depends on nothing but that sample. */
typedef struct {
    int32_t n, na, nb, width;  /* rows per ray in a / b, floats per row (1..8) */
    const float* a;            /* [n,na,width] rows of the first na elements of the concatenation */
    const float* b;            /* [n,nb,width] */
    const int32_t* rank;       /* [n,na+nb] */
    float* out;                /* [n,na+nb,width] */
} ucnerf_merge_rows_params;
int ucnerf_merge_rows(const ucnerf_merge_rows_params* p, void* stream);

/* a9 over the rows of a sorted merge, read where they are (added to ABI v6; nothing above moved): what ucnerf_merge_rows into out [n,na+nb,4]
 * followed by ucnerf_composite_fwd (live variant) on `out` and `z` produces, bit for bit, from ONE launch and with no merged array written or
 * read back.  The wave that composites a ray inverts the ray's rank row in LDS (inv[rank[j]] = j for j in cat(a, b) order) and fetches merged
 * position i from row inv[i] of raw_a or raw_b; lane split, scan, reduction order and arithmetic are those of ucnerf_composite_fwd.
 * The hierarchical renderer's fine pass (data/ray_utils.py:199-224) with the network evaluated on the new depths only: raw_a = their outputs,
 * raw_b = the coarse pass's, rank = ucnerf_sample_pdf_params.merge_rank, z = its z_sorted.
 * 1 <= na + nb <= 1024, na >= 0, nb >= 0; raw_a / raw_b 16-byte aligned (either may be NULL when its row count is 0).  `rank` must hold a
 * permutation of 0 .. na+nb-1 per ray: the producer guarantees it and it is NOT checked (any other contents give undefined outputs, never an
 * access outside the arrays named here).
 * (Declared with a struct tag, like ucnerf_depth_hypotheses_params: mirrored in _lib.ADDED_STRUCTS.) */
struct ucnerf_composite_merged_params {
    int32_t n, na, nb;         /* rays; rows per ray in raw_a / raw_b */
    int32_t white_bkgd;
    const float* raw_a;        /* [n,na,4] rows of the first na elements of the concatenation */
    const float* raw_b;        /* [n,nb,4] */
    const int32_t* rank;       /* [n,na+nb]: position in z of element j of cat(a, b) */
    const float* z;            /* [n,na+nb] the sorted merged depths */
    float* rgb_map;            /* [n,3] */
    float* depth_map;          /* [n] */
    float* acc_map;            /* [n] or NULL */
    float* disp_map;           /* [n] or NULL */
    float* weights;            /* [n,na+nb] or NULL, in merged order */
    float* var;                /* [n] or NULL (needs na + nb >= 2) */
    const float* u;            /* optional [n,na+nb] per-sample uncertainty in merged order ... */
    float* wu;                 /* ... and [n] out: sum_i w_i u_i */
};
typedef struct ucnerf_composite_merged_params ucnerf_composite_merged_params;
int ucnerf_composite_merged_fwd(const ucnerf_composite_merged_params* p, void* stream);

/* Backward of ucnerf_composite_merged_fwd (added to ABI v6; nothing above moved): the gradients of the rows of a sorted merge, read and written
 * where they are.  g_raw_a / g_raw_b are, bit for bit, what three steps in sequence give -- ucnerf_merge_rows of raw_a / raw_b into [n,na+nb,4],
 * ucnerf_composite_bwd (live variant) on that array and `z`, and taking row rank[j] of its g_raw for row j of cat(g_raw_a, g_raw_b) -- from ONE
 * launch, with neither the merged rows nor their gradients in memory.  The wave that owns a ray inverts the ray's rank row in LDS as the forward
 * does, loads merged position i from row inv[i] of raw_a or raw_b and stores its gradient to the same row of g_raw_a or g_raw_b; lane split
 * (ceil((na+nb)/64) -> 1, 2, 3, 4, 8, 16 samples per lane), scans and arithmetic are those of ucnerf_composite_bwd.  rank is a permutation, so
 * every gradient row is written exactly once: no atomics, no zero fill, and a second call into the same buffers gives the same bits.
 * The upstream gradients are in merged order (the order of the forward's outputs); the results are in the order of raw_a / raw_b.
 * 1 <= na + nb <= 1024, na >= 0, nb >= 0; raw_a / raw_b / g_raw_a / g_raw_b 16-byte aligned (a side may be NULL when its row count is 0).  As
 * in the forward `rank` is NOT checked: other contents than a permutation give undefined values, never an access outside the arrays named here.
 * (Declared with a struct tag: mirrored in _lib.ADDED_STRUCTS.) */
struct ucnerf_composite_merged_bwd_params {
    int32_t n, na, nb;         /* rays; rows per ray in raw_a / raw_b */
    int32_t white_bkgd;
    const float* raw_a;        /* [n,na,4] the forward's inputs ... */
    const float* raw_b;        /* [n,nb,4] */
    const int32_t* rank;       /* [n,na+nb] */
    const float* z;            /* [n,na+nb] */
    const float* g_rgb;        /* [n,3] or NULL */
    const float* g_depth;      /* [n] or NULL */
    const float* g_acc;        /* [n] or NULL */
    const float* g_weights;    /* [n,na+nb] or NULL, in merged order */
    float* g_raw_a;            /* [n,na,4] out, in the order of raw_a */
    float* g_raw_b;            /* [n,nb,4] out, in the order of raw_b */
};
typedef struct ucnerf_composite_merged_bwd_params ucnerf_composite_merged_bwd_params;
int ucnerf_composite_merged_bwd(const ucnerf_composite_merged_bwd_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * f2   the step in front of the path: cost-volume assembly and depth regression of one cascade stage.
 *      ucnerf_cost_volume replaces the loop of network/mvs_models.py:609-626: homo_warp (utils/utils.py:1105-1172,
 *      nearest-neighbour grid_sample, border padding, align_corners=True) of every source view's feature map onto the
 *      D x Hp x Wp hypotheses of the target view, the in-frustum count and the variance volume handed to the
 *      regularisation network.  (The warped-image volume of :614,617 is never used by the reference and is not built.)
 *      ucnerf_depth_regress replaces network/mvs_models.py:629-646: softmax over depth (+ optional initial logits),
 *      expected depth, 4-tap photometric confidence, cropped by `pad`.
 *      Non-finite inputs land where torch's own ops put them: a NaN or +-inf projected coordinate picks the pixel F.grid_sample picks (NaN: index
 *      0 of the axis; +-inf: the clamped end) and counts as outside the view; a NaN or +inf logit, or a pixel of -inf logits only, makes the
 *      pixel's probabilities, depth AND confidence NaN (clamp(0, 1) keeps a NaN); an infinite g_variance gives inf * v_i - inf * mean per view,
 *      the sum of the two terms autograd adds.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t V, C, H, W;        /* source feature maps [V,C,H,W] */
    int32_t D, pad;            /* hypotheses on the padded target grid: Hp = H + 2 pad, Wp = W + 2 pad */
    const float* feats;        /* [V,C,H,W] */
    const float* proj;         /* [V,12]: (src_proj @ ref_proj_inv)[:3], row-major 3x4 */
    const float* depth_values; /* [D,Hp,Wp] */
    float* variance;           /* [C,D,Hp,Wp] */
    float* count;              /* [D,Hp,Wp] = 1 / (1 + views that see the voxel), or NULL */
} ucnerf_cost_volume_params;
int ucnerf_cost_volume(const ucnerf_cost_volume_params* p, void* stream);

typedef struct {
    int32_t D, Hp, Wp, pad;
    const float* prob_pre;     /* [D,Hp,Wp] logits from the regularisation network */
    const float* prob_init;    /* [D,Hp,Wp] added to the logits, or NULL */
    const float* depth_values; /* [D,Hp,Wp] */
    float* prob_volume;        /* [D,Hp,Wp] softmax over D */
    float* depth;              /* [Hp - 2 pad, Wp - 2 pad] */
    float* confidence;         /* [Hp - 2 pad, Wp - 2 pad] */
} ucnerf_depth_regress_params;
int ucnerf_depth_regress(const ucnerf_depth_regress_params* p, void* stream);

/* Backward of the two kernels above (what autograd sends through them in the reference: into the source feature maps
 * through the variance volume -- the sampling grid and the mask count carry no gradient, nearest-neighbour lookup -- and
 * into the regularisation network's logits through depth and photometric confidence; floor(E[d]) and the clamp's
 * inactive side pass nothing). */
typedef struct {
    ucnerf_cost_volume_params fwd;   /* variance / count are not used */
    const float* g_variance;         /* [C,D,Hp,Wp] */
    float* g_feats;                  /* [V,C,H,W], accumulated into (float atomics) */
} ucnerf_cost_volume_bwd_params;
int ucnerf_cost_volume_bwd(const ucnerf_cost_volume_bwd_params* p, void* stream);

typedef struct {
    ucnerf_depth_regress_params fwd; /* prob_volume = the forward's output (read); depth / confidence are not used */
    const float* g_depth;            /* [Hp - 2 pad, Wp - 2 pad] or NULL */
    const float* g_confidence;       /* [Hp - 2 pad, Wp - 2 pad] or NULL */
    float* g_prob_pre;               /* [D,Hp,Wp] (also the gradient of prob_init) */
} ucnerf_depth_regress_bwd_params;
int ucnerf_depth_regress_bwd(const ucnerf_depth_regress_bwd_params* p, void* stream);

/* The link between two cascade stages (added to ABI v6; nothing above moved): the depth hypotheses depth_values [D, h + 2 pad, w + 2 pad] of a
 * stage from the previous stage's depth map -- network/mvs_models.py:536-573 (get_cur_depth_range_samples / get_depth_range_samples) as
 * CascadeMVSNet.forward strings them together, network/mvs_models.py:693-762: bilinear up-sampling of the depth to the full resolution H x W, a
 * clamped band around it, D equally spaced samples per pixel, trilinear interpolation down to the stage's h x w (the depth axis keeps its size:
 * identity), and DepthNet's replicate padding (:598).  One launch; the full-resolution volume of the reference is never stored.
 *   MAP mode (cur_depth given; stages 2 and 3), every interpolation under torch's align_corners=False rule
 *   (src = max((dst + 0.5) * n_in / n_out - 0.5, 0), taps floor(src) and min(floor(src) + 1, n_in - 1), weights 1 - l and l):
 *     c(Y, X)   = bilinear sample of cur_depth [h0, w0] at full-resolution pixel (Y, X)
 *     mn        = max(c - D / 2 * interval_pixel, near),  mx = min(c + D / 2 * interval_pixel, far),
 *                 interval_pixel = k * (far - near), or k * interval[0] where the caller holds the interval as a device value of its own
 *     s_d(Y, X) = mn + d * (mx - mn) / (D - 1)
 *     out[d, y + pad, x + pad] = bilinear sample of s_d at (y, x) of the h x w grid; the border of `pad` pixels repeats the edge value.
 *     Sizes: h0 <= H, w0 <= W, h <= H, w <= W (any ratio, integer or not).
 *     Non-finite depths land where torch's own ops put them: max / min are torch.clamp's, so a NaN c gives NaN mn and mx (not the full band
 *     [near, far]); every tap is multiplied by its weight, a zero weight included (0 * NaN = 0 * inf = NaN); and the depth axis has the taps d and
 *     min(d + 1, D - 1) with the weights 1 and 0, as an interpolation that keeps a size has in torch: out[d] is NaN where a tap of plane d or
 *     of the next plane is not finite.  No finite value depends on any of this.  (The backward: both pass_lo and pass_hi are 0 on a NaN c, as in
 *     torch's clamp backward, so a finite g_out gives a finite g_cur_depth whatever cur_depth holds.)
 *   ROW mode (row given; stage 1): mn = row[0], mx = row[D_in - 1], the same s_d for every pixel; H, W, h0, w0, k, near_far, interval are not read.
 * Exactly one of cur_depth / row is non-NULL.  near and far are read on the device (near_far[0], near_far[1]): no host copy of a device
 * value on this path.  D >= 2.  An output of zero elements (h + 2 pad == 0 or w + 2 pad == 0) is success, nothing launched.  Backward (map mode, into
 * cur_depth; near_far and interval get none, row mode has no tensor to differentiate): ucnerf_depth_hypotheses_bwd below.
 * (Declared with a struct tag: the closing line of every typedef above is what tests/test_abi_host.py matches against the v6 struct table of
 *  uc_nerf_amd/_lib.py, which stays as it was; this struct is mirrored in _lib.ADDED_STRUCTS.) */
struct ucnerf_depth_hypotheses_params {
    int32_t D, h, w, pad;      /* output [D, h + 2 pad, w + 2 pad] */
    int32_t H, W;              /* intermediate (full) resolution; map mode */
    int32_t h0, w0;            /* size of cur_depth; map mode */
    int32_t D_in;              /* length of row; row mode */
    float k;                   /* interval_pixel = k * (far - near); CascadeMVSNet passes depth_interals_ratio[stage] / 48 */
    const float* cur_depth;    /* [h0, w0] or NULL */
    const float* row;          /* [D_in] or NULL */
    const float* near_far;     /* [2] = (near, far); map mode */
    const float* interval;     /* [1] or NULL (= far - near); map mode */
    float* out;                /* [D, h + 2 pad, w + 2 pad] */
};
typedef struct ucnerf_depth_hypotheses_params ucnerf_depth_hypotheses_params;
int ucnerf_depth_hypotheses(const ucnerf_depth_hypotheses_params* p, void* stream);

/* The gradients the reference's plain torch expressions carry along depth regression -> depth_values -> depth hypotheses -> previous depth
 * (CascadeMVSNet with grad_method="undetach", network/mvs_models.py:715-722; both added to ABI v6, nothing above moved).
 *
 * ucnerf_depth_regress_bwd_values: depth = sum_d prob_volume[d] * depth_values[d], cropped by `pad`, so
 *   g_depth_values[d, y + pad, x + pad] = prob_volume[d, y + pad, x + pad] * g_depth[y, x], and prob_volume * 0 on the border of `pad` pixels
 *   (the crop drops it: 0 for a finite probability, NaN for a NaN one, as torch's slice backward gives); the confidence does not depend on
 *   depth_values.  Every element of g_depth_values is written.  D, Hp, Wp, pad >= 0, Hp >= 2 pad,
 *   Wp >= 2 pad, Hp * Wp < 2^31; a volume of zero elements is success, nothing launched; g_depth is read only where the cropped map is not empty.
 *
 * ucnerf_depth_hypotheses_bwd: the backward of ucnerf_depth_hypotheses in MAP mode, g_out [D, h + 2 pad, w + 2 pad] -> g_cur_depth [h0, w0],
 *   OVERWRITTEN (not accumulated).  `fwd` holds the forward's parameters (row must be NULL; out is not read).  Per padded output position
 *   ("column") G0 = sum_d g_d and G1 = sum_d g_d * d / (D - 1); a border column's sums fold onto the edge column it repeats (a corner edge column
 *   collects the whole (pad + 1)^2 block).  Inner column (y, x) gives ly[a] * lx[b] * ((G0 - G1) * pass_lo + G1 * pass_hi) to each of its 2 x 2
 *   full-resolution taps (Y_a, X_b), with pass_lo = (c - half >= near), pass_hi = (c + half <= far), c the forward's own bilinear sample of
 *   cur_depth there and half = D / 2 * interval_pixel: TIES PASS, as the backward of torch's clamp does.  Each full-resolution pixel hands its
 *   sum on to its 2 x 2 taps in cur_depth with the up-sampling weights.  Where both taps of an axis are the same pixel (edge clamp, 1-pixel axis)
 *   both weights count.
 *   Three launches, every one a GATHER over the destinations whose taps include the pixel a thread owns (a conservative candidate range from the
 *   scale, membership decided by the forward's own tap rule): no atomics, a fixed summation order, the same bits from every launch.
 *   `scratch`: ucnerf_depth_hypotheses_bwd_scratch_floats(&fwd) = 2 h w + H W floats (the column sums and the full-resolution gradient,
 *   327 KB + at most 655 KB at 256 x 320), the caller's allocation on the stream of the call; < 0 on bad sizes.
 *   Validation as the forward's (negative sizes, D >= 2, the cover conditions, plane < 2^31 and H W < 2^31) comes first; then an empty g_cur_depth
 *   (h0 == 0 or w0 == 0) is success with nothing launched and no pointer read; then NULL pointers are refused; an empty g_out with a non-empty
 *   g_cur_depth zero-fills it.
 * (Both structs are declared with a struct tag and mirrored in _lib.ADDED_STRUCTS.) */
struct ucnerf_depth_regress_bwd_values_params {
    int32_t D, Hp, Wp, pad;
    const float* prob_volume;  /* [D,Hp,Wp] the forward's output */
    const float* g_depth;      /* [Hp - 2 pad, Wp - 2 pad] */
    float* g_depth_values;     /* [D,Hp,Wp] out */
};
typedef struct ucnerf_depth_regress_bwd_values_params ucnerf_depth_regress_bwd_values_params;
int ucnerf_depth_regress_bwd_values(const ucnerf_depth_regress_bwd_values_params* p, void* stream);

struct ucnerf_depth_hypotheses_bwd_params {
    struct ucnerf_depth_hypotheses_params fwd;  /* map mode: cur_depth, near_far (and interval) as the forward had them; row NULL; out not read */
    const float* g_out;        /* [D, h + 2 pad, w + 2 pad] */
    float* scratch;            /* ucnerf_depth_hypotheses_bwd_scratch_floats(&fwd) floats */
    float* g_cur_depth;        /* [h0, w0] out, overwritten */
};
typedef struct ucnerf_depth_hypotheses_bwd_params ucnerf_depth_hypotheses_bwd_params;
int64_t ucnerf_depth_hypotheses_bwd_scratch_floats(const ucnerf_depth_hypotheses_params* fwd);
int ucnerf_depth_hypotheses_bwd(const ucnerf_depth_hypotheses_bwd_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * e1   evaluation metrics on the device -- utils/evaluation.py:8-74 (compute_errors, depth_evaluation) and :76-101 (rgb_evaluation: PSNR and
 *      SSIM; LPIPS below: the library supplies the AlexNet feature stack and the distance, the caller the weights).  The rendered images and
 *      depth maps stay where the render pass left them; one small vector per call is all a host has to read.
 * ---------------------------------------------------------------------------------------------- */
/* Workspace of ucnerf_depth_eval and of ucnerf_image_eval on n images of H x W pixels, in floats (the larger of the two: one allocation serves
 * both): the digit histograms of the selection, the per-block partial sums and counts of the reductions.  < 0 on a bad argument. */
int64_t ucnerf_eval_workspace_floats(int32_t n, int32_t H, int32_t W);

/* depth_evaluation (utils/evaluation.py:29-74) without its host loop.  valid(i) = gt > min_depth && gt < max_depth && (mask == NULL || mask != 0);
 *   ratio = median(gt over all valid pixels of all images) / median(pred over the same pixels): the EXACT float32 medians as numpy forms them
 *           (odd count: the middle value; even count N: fl(fl(a + b) / 2) of ranks N/2 - 1 and N/2), found by an 8-bit radix selection on
 *           order-preserving keys -- 4 histogram launches and 4 one-block pick launches, integer counts only (reproducible), nothing compacted;
 *   per image and valid pixel, in float32 and in the reference's order: p = clamp(pred * ratio, min_depth, max_depth), t = max(gt / p, p / gt),
 *           the counts of t < 1.25, < 1.5625, < 1.953125 and the sums of (gt - p)^2, (log gt - log p)^2, |gt - p| / gt, (gt - p)^2 / gt: per-block
 *           partials, summed in a fixed order by a second launch (no float atomics: the same bits on every run).
 * raw != 0 is compute_errors (:8-26) on its own: every pixel valid, p = pred as given, no medians (mask, min_depth, max_depth not read).
 * out [4 + 12 n] 32-bit words:
 *   out[0] ratio (float; NaN when no pixel is valid; 1 with raw)   out[1] int32: 1 when no pixel of any image is valid
 *   out[2], out[3] the two medians (gt, pred)
 *   per image i at out + 4 + 12 i: int32 valid count, count(a1), count(a2), count(a3); float abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 (each mean =
 *   sum / float(count), rmse = sqrt(mean); a_k = float(count_k) / float(count)); int32 flag: 1 when the image has no valid pixel (its seven
 *   values are then NaN, and the reference leaves it out of the mean over images).
 * n, H, W >= 1, n <= 65535 and n * H * W < 2^31; a NULL gt / pred / workspace / out, a workspace not 8-byte aligned and min_depth > max_depth are UCNERF_EINVAL.
 * 10 launches + 1 memset (3 launches with raw), whatever the data; nothing is read back.  NaN depths are never valid; a NaN PREDICTION on a
 * valid pixel sorts above +inf here, where numpy's median would answer NaN. */
struct ucnerf_depth_eval_params {
    int32_t n, H, W;
    int32_t raw;               /* 1: compute_errors on gt / pred as they are */
    float min_depth, max_depth;
    const float* gt;           /* [n,H,W] */
    const float* pred;         /* [n,H,W] */
    const uint8_t* mask;       /* [n,H,W] or NULL */
    float* workspace;          /* ucnerf_eval_workspace_floats(n, H, W) floats, 8-byte aligned */
    float* out;                /* [4 + 12 n] words, see above */
};
typedef struct ucnerf_depth_eval_params ucnerf_depth_eval_params;
int ucnerf_depth_eval(const ucnerf_depth_eval_params* p, void* stream);

/* rgb_evaluation's per-image numbers (utils/evaluation.py:82-83, :89-96) for images gt, pred [n,3,H,W]:
 *   mse  = float32 sum of (gt - pred)^2 over the image / float(3 H W)  (per-block partials, fixed order);   psnr = -10 log10(mse);
 *   ssim = skimage.metrics.structural_similarity(data_range=1, channel_axis=2, everything else default): uniform 7 x 7 window per channel,
 *          C1 = 1e-4, C2 = 9e-4, sample covariances v = 49/48 (uxx - ux ux), S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
 *          the mean of S over the windows that lie inside the image, then over the channels.  Window sums, S and its sums are carried in fp64
 *          (products of two float32 values are exact there), the result is rounded to float32 once;
 *   gt_max = the largest gt value of the image (what the reference's `assert gts.max() <= 1` needs).
 * out [n,4] = (mse, psnr, ssim, gt_max).  1 <= n <= 65535, H >= 7, W >= 7 (skimage refuses a smaller image too; with no_ssim
 * any H, W >= 1), 3 n H W < 2^31.  3 launches (2 with no_ssim). */
struct ucnerf_image_eval_params {
    int32_t n, H, W;
    int32_t no_ssim;           /* 1: the image error alone (ssim = NaN); any H, W >= 1 */
    const float* gt;           /* [n,3,H,W] */
    const float* pred;         /* [n,3,H,W] */
    float* workspace;          /* ucnerf_eval_workspace_floats(n, H, W) floats, 8-byte aligned */
    float* out;                /* [n,4] */
};
typedef struct ucnerf_image_eval_params ucnerf_image_eval_params;
int ucnerf_image_eval(const ucnerf_image_eval_params* p, void* stream);

/* LPIPS, net = 'alex' (utils/evaluation.py:85-88, :97; the `lpips` package v0.1 on torchvision's AlexNet `features`), inference only, float32,
 * no atomics: every sum has one fixed order, two calls give the same bits.  (Added to ABI v6; nothing above moved.)
 *
 * ucnerf_conv2d_bias_relu: y[n,cout,OH,OW] = relu?(conv2d(x[n,cin,H,W], w[cout,cin,K,K], stride, zero pad) + bias), OH = (H + 2 pad - K) / stride + 1,
 *   an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation).  Any cin, cout >= 1; 1 <= K <= 11; cin K K < 2^22;
 *   cin H W < 2^31; n OH OW < 2^31 - 64.  `packed` is the weight as ucnerf_conv2d_pack wrote it (ucnerf_conv2d_packed_floats(cin, cout, K)
 *   floats: [cout tile of 64][k padded to a multiple of 32][64] weights, zero where there is none, then one int32 tap code per k).
 *   ACCUMULATION ORDER over k = (cin K + ky) K + kx: within the j-th run of 32 consecutive k, S_j = the fmaf chain over ascending k from +0;
 *   then T = (((+0 + S_0) + S_1) + ...) over ascending j; y = T + bias; with relu != 0, y > 0 ? y : +0 (a NaN stays).  A tap that falls into the
 *   padding is an operand of exactly +0 (so is every k past cin K K): it adds +0, or NaN where its weight is not finite, as torch's does.
 *   shift / scale (both or neither, [cin]): the input is read as (x - shift[c]) / scale[c] (IEEE division) where it is INSIDE the image; the
 *   padding stays 0 -- LPIPS' scaling layer in front of a padded convolution.
 * ucnerf_maxpool2d: 3 x 3 window, stride 2, no pad, floor mode, on `planes` maps of H x W (H, W >= 3): OH = (H - 3) / 2 + 1.  Any float
 *   values (the first tap starts the maximum, -inf is a value like any other; a NaN in the window is the result, as in torch).
 * ucnerf_lpips_layer: one launch, one block per pair i.  Per pixel n0 = f0 / (sqrt(sum_c f0^2) + 1e-10), n1 likewise,
 *   d = sum_c lin[c] (n0[c] - n1[c])^2.  The channel sums are float32 in a fixed order that depends on h w alone: G lanes share a pixel (G = the
 *   smallest power of two with h w G >= 4096, at most 64), lane g adds the channels g, g + G, ... in ascending order, an xor butterfly folds the
 *   G partial sums.  The mean of d over the h w pixels is carried in fp64 (lane, wave tree, waves in order) and rounded once;
 *   out[i] = mean (accumulate == 0) or out[i] + mean (accumulate != 0).  The normalised maps are never stored.  A pixel
 *   whose features are all zero gives 0 / 1e-10 = 0: it contributes exactly 0.  d(f0, f1) and d(f1, f0) are the same bits.
 * ucnerf_lpips_alex: the whole chain for n pairs a, b [n,3,H,W] (values in [-1, 1]):
 *     scaling (in conv1's operand load) -> conv1 3->64 11x11 /4 pad 2 + ReLU = level 0 -> pool -> conv2 64->192 5x5 pad 2 + ReLU = level 1 -> pool
 *     -> conv3 192->384 3x3 pad 1 + ReLU = level 2 -> conv4 384->256 + ReLU = level 3 -> conv5 256->256 + ReLU = level 4;
 *     out[i] = ((((d_0 + d_1) + d_2) + d_3) + d_4), d_l = ucnerf_lpips_layer of level l with lin[l].  13 launches; out needs no initial value.
 *   MINIMUM SIDE 31: conv1 gives o1 = (H - 7) / 4 + 1, the first pool p1 = (o1 - 3) / 2 + 1, conv2 keeps p1, and the second pool needs
 *   p1 >= 3, so o1 >= 7, (H - 7) / 4 >= 6, H >= 31 (then p1 = 3 and the last three levels are 1 x 1).  A smaller H or W is UCNERF_EINVAL.
 *   workspace: ucnerf_lpips_workspace_floats(n, H, W) floats (the five levels and the two pooled maps of 2 n images; < 0 on a bad argument);
 *   every word of it that is read has been written by the same call.
 * Everywhere: a NULL params or required array and a negative count are UCNERF_EINVAL; n == 0 (planes == 0) is success, nothing launched. */
struct ucnerf_conv2d_pack_params {
    int32_t cin, cout, K, reserved;
    const float* weight;       /* [cout,cin,K,K] */
    float* packed;             /* ucnerf_conv2d_packed_floats(cin, cout, K) floats, overwritten */
};
typedef struct ucnerf_conv2d_pack_params ucnerf_conv2d_pack_params;
int64_t ucnerf_conv2d_packed_floats(int32_t cin, int32_t cout, int32_t K);
int ucnerf_conv2d_pack(const ucnerf_conv2d_pack_params* p, void* stream);

struct ucnerf_conv2d_params {
    int32_t n, cin, H, W, cout, K, stride, pad;
    int32_t relu;              /* 1: max(y, 0) */
    int32_t reserved;
    const float* x;            /* [n,cin,H,W] */
    const float* packed;       /* from ucnerf_conv2d_pack with the same cin, cout, K */
    const float* bias;         /* [cout] */
    const float* shift;        /* [cin] or NULL */
    const float* scale;        /* [cin] or NULL */
    float* y;                  /* [n,cout,OH,OW] */
};
typedef struct ucnerf_conv2d_params ucnerf_conv2d_params;
int ucnerf_conv2d_bias_relu(const ucnerf_conv2d_params* p, void* stream);

struct ucnerf_maxpool2d_params {
    int64_t planes;            /* n * C */
    int32_t H, W;
    const float* x;            /* [planes,H,W] */
    float* y;                  /* [planes,OH,OW] */
};
typedef struct ucnerf_maxpool2d_params ucnerf_maxpool2d_params;
int ucnerf_maxpool2d(const ucnerf_maxpool2d_params* p, void* stream);

struct ucnerf_lpips_layer_params {
    int32_t n, C, h, w;
    int32_t accumulate;        /* 0: out[i] = mean d; 1: out[i] += mean d */
    int32_t reserved;
    const float* f0;           /* [n,C,h,w] */
    const float* f1;           /* [n,C,h,w] */
    const float* lin;          /* [C] */
    float* out;                /* [n] */
};
typedef struct ucnerf_lpips_layer_params ucnerf_lpips_layer_params;
int ucnerf_lpips_layer(const ucnerf_lpips_layer_params* p, void* stream);

struct ucnerf_lpips_alex_params {
    int32_t n, H, W, reserved;
    const float* a;            /* [n,3,H,W] */
    const float* b;            /* [n,3,H,W] */
    const float* packed[5];    /* conv1 .. conv5, from ucnerf_conv2d_pack */
    const float* bias[5];      /* [64], [192], [384], [256], [256] */
    const float* lin[5];       /* the same lengths */
    const float* shift;        /* [3] */
    const float* scale;        /* [3] */
    float* workspace;          /* ucnerf_lpips_workspace_floats(n, H, W) floats */
    float* out;                /* [n] */
};
typedef struct ucnerf_lpips_alex_params ucnerf_lpips_alex_params;
int64_t ucnerf_lpips_workspace_floats(int32_t n, int32_t H, int32_t W);
int ucnerf_lpips_alex(const ucnerf_lpips_alex_params* p, void* stream);

/* The 3-D convolutions of CasMVSNet's cost regularisation (network/mvs_models.py:110-195 Conv3d / Deconv3d, :412-443 CostRegNet), inference only,
 * float32, NCDHW contiguous in and out, no atomics: every sum has one fixed order, two calls give the same bits and an image's result does not
 * depend on the batch it is in.  (Added to ABI v6; nothing above moved.)
 *
 * ucnerf_conv3d: y = act(conv(x) + bias[co]) (+ skip); act = max(., 0) with relu != 0 (a NaN stays), the identity otherwise; skip (NULL or a
 *   tensor of y's shape) is added AFTER the activation.  An implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation):
 *   16-row channel tiles for cout <= 16, 32-row tiles above; cout == 1 of the forward form runs as a VALU kernel in the same order.
 *   transposed == 0: y[n,cout,OD,OH,OW], O = (I + 2 pad - K) / stride + 1, cubic K of 1 or 3, stride 1 or 2, zero padding 0 <= pad <= 64,
 *     weight [cout,cin,K,K,K].
 *   transposed == 1: conv_transpose3d with K = 3, stride = 2, pad = 1, output_padding = 1 (no other), weight [cin,cout,3,3,3]; y[n,cout,2D,2H,2W].
 *     The output voxels are handled in 8 parity classes (od & 1, oh & 1, ow & 1); a class multiplies only its 1, 2, 4 or 8 live taps.
 *   `packed` is the weight as ucnerf_conv3d_pack wrote it, `packed_floats` its size = ucnerf_conv3d_packed_floats(cin, cout, K, transposed): per
 *     class [channel tile][k padded to a multiple of 32][16 or 32 rows] weights, zero where there is none, then one int32 tap code per k.
 *   Limits: cin <= 2^16; cin D H W, cout OD OH OW < 2^31; n * voxels < 2^31 - 1024.
 *   ACCUMULATION ORDER: k = ci * taps + t, t = (kd K + kh) K + kw (the flat index of the weight's row; for the transposed form the live taps of the
 *     class in that same order).  Within the j-th run of 32 consecutive k, S_j = the fmaf chain over ascending k from +0; then
 *     T = (((+0 + S_0) + S_1) + ...) over ascending j; y = T + bias; the activation; then + skip.  A tap outside the volume contributes +0.
 *   UCNERF_EINVAL before any device call: NULL params or required array, negative n, non-positive cin / cout / D / H / W, a K / stride / pad /
 *     transposed combination outside the above, packed_floats that does not match.  n == 0 is success, nothing launched. */
struct ucnerf_conv3d_pack_params {
    int32_t cin, cout, K, transposed;
    const float* weight;       /* [cout,cin,K,K,K], transposed: [cin,cout,3,3,3] */
    float* packed;             /* ucnerf_conv3d_packed_floats(cin, cout, K, transposed) floats, overwritten */
};
typedef struct ucnerf_conv3d_pack_params ucnerf_conv3d_pack_params;
int64_t ucnerf_conv3d_packed_floats(int32_t cin, int32_t cout, int32_t K, int32_t transposed);   /* < 0 on a bad argument */
int ucnerf_conv3d_pack(const ucnerf_conv3d_pack_params* p, void* stream);

struct ucnerf_conv3d_params {
    int32_t n, cin, D, H, W, cout, K, stride, pad;
    int32_t relu;              /* 1: max(y, 0) */
    int32_t transposed;        /* 1: the transposed form */
    int32_t reserved;
    int64_t packed_floats;     /* floats `packed` holds */
    const float* x;            /* [n,cin,D,H,W] */
    const float* packed;       /* from ucnerf_conv3d_pack with the same cin, cout, K, transposed */
    const float* bias;         /* [cout] */
    const float* skip;         /* y's shape, or NULL */
    float* y;                  /* [n,cout,OD,OH,OW] */
};
typedef struct ucnerf_conv3d_params ucnerf_conv3d_params;
int ucnerf_conv3d(const ucnerf_conv3d_params* p, void* stream);

/* Batch-statistic batch-norm: what nn.BatchNorm2d / 3d computes in training mode, forward only, for the CNNs above under train() + no_grad (the
 * reference's validation_step runs its consistency learner that way, train.py:226-243).  (Added to ABI v6; nothing above moved.)
 * y is a contiguous float32 [n, C, S] tensor, S the product of the spatial sizes; a channel has N = n S values, numbered i = img * S + offset.
 * Two launches, ucnerf_bn_stats then ucnerf_bn_apply, on one stream; nothing is read back, no atomics, every store a plain vector store: two
 * calls give the same bits, and the pair can sit inside a captured graph.
 * ONE CODE PATH (csrc/bn.hip): these entry points and the two backward ones below ARE G = 1 of the grouped entry points at the end of this header --
 * the struct is copied behind G = 1 and the same checks and the same four kernels run; only the name in front of an error text differs
 * (so a workspace that is too small is now reported as "G C P = 1 x C x P" where these entries used to say "C P = C x P").
 *
 * ucnerf_bn_partials(n, S) = P = min(32, ceil(N / 4096)), the partial slots per channel; < 0 on a bad argument (n or S < 1, N < 2 or above the
 *   limit below).  Pure host.  Slice j of a channel is the values [j L, min((j + 1) L, N)) with L = ceil(N / P) rounded up to a multiple of 4;
 *   every slice is non-empty, the last may be shorter.
 * ucnerf_bn_stats: workspace[(c P + j) * 3 + 0 .. 2] = (count, mean, M2) of slice j of channel c as float64, M2 = sum (y - mean)^2.
 *   SUMMATION ORDER, all in float64, the values converted exactly.  merge(a, b), Chan's pairwise update: b empty -> a; otherwise n = na + nb,
 *   r = nb / n, d = mean_b - mean_a, mean = mean_a + d r, M2 = (M2_a + M2_b) + (d d)(na r), separate multiplications and additions.
 *   The slice is walked in quads of four consecutive values, quad q at j L + 4 q.  Thread t of 1024 takes, as its k-th chunk, the quads
 *   (4 k + u) 1024 + t, u = 0 .. 3: over the chunk's values inside the slice, in ascending i, sum = (((0 + v) + v) + ...), mean = sum / count, then
 *   M2 = (((0 + (v - mean)^2) + ...) in the same order; the thread's triple = merge(merge(merge(empty, chunk 0), chunk 1), ...).  Lanes: for
 *   d = 1, 2, 4, 8, 16, 32 lane l < 64 - d becomes merge(lane l, lane l + d) with the values of before the step; lane 0 holds the wave's triple.
 *   Waves: merge(.. merge(wave 0, wave 1) .., wave 15).
 * ucnerf_bn_apply: every block folds merge(.. merge(triple 0, triple 1) .., triple P - 1) of its channel, in float64, and so holds the same
 *   mu = mean and sigma^2 = M2 / N (biased), each rounded ONCE to float32.  Then in float32: s = weight[c] / sqrt(sigma^2 + eps), IEEE division
 *   and square root; out = act(fma(y - mu, s, bias[c])) (+ skip), act = max(., 0) with relu != 0 (a NaN stays), the identity otherwise; skip
 *   (NULL or a tensor of y's shape) is added AFTER the activation.  out may be y itself (not a shifted overlap).  One block per channel also
 *   writes saved_mean[c] = mu, saved_var[c] = sigma^2, running_mean[c] = (1 - m) running_mean[c] + m mu and running_var[c] =
 *   (1 - m) running_var[c] + m u, u = M2 / (N - 1) rounded once to float32 (the unbiased variance), in float32 with separate multiplications
 *   and additions; one thread of the launch adds 1 to the int64 *num_batches_tracked.
 * Both are memory-bound: stats reads |y| once, apply reads |y| (+ |skip|) and writes |y|; accesses are 16 bytes per lane where S % 4 == 0 and
 *   the arrays are 16-byte aligned, 4 bytes otherwise (the same values in the same order either way).
 * UCNERF_EINVAL before any device call: NULL params or required array, n / C / S < 1, N < 2, N > 2^31 - 2^20, C > 65535, a product that
 *   overflows, eps <= 0, momentum outside (0, 1], workspace_triples < C P, a workspace or num_batches_tracked that is not 8-byte aligned. */
int64_t ucnerf_bn_partials(int64_t n, int64_t S);
struct ucnerf_bn_stats_params {
    int64_t n, C, S;
    int64_t workspace_triples; /* triples (3 float64 each) the workspace holds, at least C P */
    const float* y;            /* [n,C,S] */
    double* workspace;         /* [C,P,3], overwritten */
};
typedef struct ucnerf_bn_stats_params ucnerf_bn_stats_params;
int ucnerf_bn_stats(const ucnerf_bn_stats_params* p, void* stream);

struct ucnerf_bn_apply_params {
    int64_t n, C, S;
    int64_t workspace_triples;
    float eps, momentum;
    int32_t relu;              /* 1: max(., 0) before the skip addition */
    int32_t reserved;
    const float* y;            /* [n,C,S], as ucnerf_bn_stats read it */
    const double* workspace;   /* as ucnerf_bn_stats wrote it for the same n, C, S */
    const float* weight;       /* gamma [C] */
    const float* bias;         /* beta [C] */
    const float* skip;         /* y's shape, or NULL */
    float* out;                /* y's shape; may be y */
    float* saved_mean;         /* [C], overwritten */
    float* saved_var;          /* [C], overwritten: the biased variance */
    float* running_mean;       /* [C], updated */
    float* running_var;        /* [C], updated with the unbiased variance */
    int64_t* num_batches_tracked;   /* one int64 on the device, incremented */
};
typedef struct ucnerf_bn_apply_params ucnerf_bn_apply_params;
int ucnerf_bn_apply(const ucnerf_bn_apply_params* p, void* stream);

/* Training CostRegNet on the device: the weight gradient of ucnerf_conv3d and the backward of the batch-statistic batch-norm with its ReLU.
 * (Added to ABI v6; nothing above moved.)  The INPUT gradient of a convolution needs no entry point of its own: it is ucnerf_conv3d on
 * grad_y with the weight presented the other way round (uc_nerf_amd.ops.conv3d_dgrad).
 *
 * ucnerf_conv3d_wgrad: grad_weight of one layer, K = 3 only (K = 1 is refused with UCNERF_EINVAL), float32, NCDHW contiguous.  D, H, W are the
 *   sizes of the layer's INPUT x in both forms.  Both forms are one computation over a small grid s = (sd, sh, sw) and a big one,
 *   out[a][b][t] = sum over (img, s) of A[img,a,s] B[img,b, stride s - pad + t], t = (td, th, tw) = the flat tap 9 td + 3 th + tw, a tap outside
 *   the big grid contributing +0:
 *     transposed == 0 (stride 1 or 2, 0 <= pad <= 64, weight [cout,cin,3,3,3]): A = grad_y [n,cout,OD,OH,OW], O = (I + 2 pad - 3) / stride + 1,
 *       B = x [n,cin,D,H,W]; grad_weight [cout,cin,27].
 *     transposed == 1 (stride 2, pad 1, output_padding 1, weight [cin,cout,3,3,3]): A = x [n,cin,D,H,W], B = grad_y [n,cout,2D,2H,2W];
 *       grad_weight [cin,cout,27].
 *   Exact fp32 products and fp32 accumulation on v_mfma_f32_16x16x4_f32 for every shape (a side with one channel is padded to a 16-row tile
 *   like any other), both operands staged through LDS 32 voxels at a time.  The voxels v = img S + s (S = the small grid's size, V = n S of
 *   them) are the reduction dimension and are cut into chunks; no atomics, every store a plain vector store, two calls give the same bits.
 *   SUMMATION ORDER (fixed, part of the interface).  Ca, Cb = the channels of A and B; tiles = ceil(Ca / 16) ceil(Cb / 16);
 *     C0 = min(ceil(V / 32), max(1, ceil(512 / tiles))); the chunk length L = 32 ceil(V / (32 C0)); chunks = ceil(V / L); chunk c is the voxels
 *     [c L, min((c + 1) L, V)).  Within a chunk P_c = one fmaf chain from +0 over ascending v (the MFMA adds four consecutive voxels per
 *     instruction, the lowest first; a tap outside the big grid enters as the product a * +0).  grad_weight = (((+0 + P_0) + P_1) + ...) over
 *     ascending c, by a second launch.
 *   workspace: ucnerf_conv3d_wgrad_workspace_floats(...) = chunks Ca Cb 27 floats, laid out [chunk][a][t][b], every element overwritten; < 0 on a
 *     bad argument; pure host.  Limits: cin, cout <= 2^16; Ca S, Cb big < 2^31 per image; V < 2^31 - 1024; cin cout 27 < 2^31.
 *   UCNERF_EINVAL before any device call: NULL params or array, negative n, non-positive cin / cout / D / H / W, K != 3, a stride / pad /
 *     transposed combination outside the above, workspace_floats that does not match the query.  n == 0 is success, nothing launched.
 *
 * ucnerf_bn_bwd_reduce then ucnerf_bn_bwd_apply: the backward of ucnerf_bn_stats / ucnerf_bn_apply (with the ReLU, without the skip: the skip's
 *   gradient is g itself).  g = the gradient of the layer's output, y = the convolution's raw output the forward normalised, saved_mean = mu
 *   and saved_var = sigma^2 as the forward wrote them.  The same slices as the forward (P = ucnerf_bn_partials(n, S)), a float64 workspace
 *   [C, P, 2], no atomics, nothing read back, two calls give the same bits.
 *   Per element, in float32: s = weight[c] / sqrt(sigma^2 + eps) and z = fma(y - mu, s, bias[c]), the very expressions of ucnerf_bn_apply (IEEE
 *   division and square root), so z is the forward's pre-activation value bit for bit; the mask m = relu ? !(z <= 0) : 1 (torch's threshold
 *   rule: a NaN passes); gm = m ? g : 0.  Everything after that is FLOAT64 per element, the values converted exactly, separate multiplications
 *   and additions, and rounded once to float32 at the store.
 *   reduce: workspace[(c P + j) 2 + 0 .. 1] = (A_j, B_j) = (sum gm, sum gm (y - mu)) over slice j.  Order: thread t of 1024 adds its values in
 *     the order the forward's thread walks them (chunk k, quads (4 k + u) 1024 + t, ascending i), from 0; lanes: for d = 1, 2, .. 32 lane
 *     l < 64 - d adds lane l + d's value of before the step; waves: ((wave 0 + wave 1) + ...) ascending.
 *   apply: every block folds A = ((A_0 + A_1) + ...), B likewise, ascending; r = 1 / sqrt(sigma^2 + eps), k1 = A / N, k2 = r r B / N,
 *     sg = weight[c] r, all float64; grad_y = sg ((gm - k1) - (y - mu) k2); one block per channel writes grad_bias[c] = A and
 *     grad_weight[c] = B r, each rounded once.  grad_y may be g itself (not a shifted overlap).
 *   Both are memory-bound: reduce reads |g| + |y|, apply reads them again and writes |y|.
 *   UCNERF_EINVAL before any device call: as ucnerf_bn_stats (shape, limits, alignment), NULL arrays, eps <= 0, workspace_pairs < C P. */
struct ucnerf_conv3d_wgrad_params {
    int32_t n, cin, D, H, W, cout, K, stride, pad;   /* of the layer: x is [n,cin,D,H,W] */
    int32_t transposed;
    int64_t workspace_floats;  /* floats `workspace` holds = ucnerf_conv3d_wgrad_workspace_floats(the same arguments) */
    const float* x;            /* [n,cin,D,H,W] */
    const float* grad_y;       /* the layer output's gradient: [n,cout,OD,OH,OW], transposed [n,cout,2D,2H,2W] */
    float* workspace;          /* overwritten */
    float* grad_weight;        /* [cout,cin,3,3,3], transposed [cin,cout,3,3,3], overwritten */
};
typedef struct ucnerf_conv3d_wgrad_params ucnerf_conv3d_wgrad_params;
int64_t ucnerf_conv3d_wgrad_workspace_floats(int32_t n, int32_t cin, int32_t cout, int32_t D, int32_t H, int32_t W, int32_t K, int32_t stride, int32_t pad,
                                             int32_t transposed);
int ucnerf_conv3d_wgrad(const ucnerf_conv3d_wgrad_params* p, void* stream);

struct ucnerf_bn_bwd_reduce_params {
    int64_t n, C, S;
    int64_t workspace_pairs;   /* pairs (2 float64 each) the workspace holds, at least C P */
    float eps;
    int32_t relu;              /* 1: the forward applied max(., 0) */
    const float* g;            /* [n,C,S] */
    const float* y;            /* [n,C,S], the forward's input */
    const float* saved_mean;   /* [C] */
    const float* saved_var;    /* [C] */
    const float* weight;       /* gamma [C] */
    const float* bias;         /* beta [C] */
    double* workspace;         /* [C,P,2], overwritten */
};
typedef struct ucnerf_bn_bwd_reduce_params ucnerf_bn_bwd_reduce_params;
int ucnerf_bn_bwd_reduce(const ucnerf_bn_bwd_reduce_params* p, void* stream);

struct ucnerf_bn_bwd_apply_params {
    int64_t n, C, S;
    int64_t workspace_pairs;
    float eps;
    int32_t relu;
    const float* g;
    const float* y;
    const float* saved_mean;
    const float* saved_var;
    const float* weight;
    const float* bias;
    const double* workspace;   /* as ucnerf_bn_bwd_reduce wrote it for the same arguments */
    float* grad_y;             /* [n,C,S]; may be g */
    float* grad_weight;        /* [C], overwritten */
    float* grad_bias;          /* [C], overwritten */
};
typedef struct ucnerf_bn_bwd_apply_params ucnerf_bn_bwd_apply_params;
int ucnerf_bn_bwd_apply(const ucnerf_bn_bwd_apply_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * e2   a whole validation image on the device -- train.py:274-288 (the reference pulls every rendered chunk to the host, concatenates, clamps and
 *      permutes there) and utils/utils.py:58-77 (visualize_depth: numpy normalisation, cv2.applyColorMap, PIL, ToTensor).  Here a chunk is
 *      written straight into the image planes the metrics above read, the depth range is kept in a two-word cell on the device, and the
 *      depth picture is one launch.  (Added to ABI v6; nothing above moved.  Structs declared with a tag: mirrored in _lib.ADDED_STRUCTS.)
 *      No entry point synchronises the stream or reads anything back; all stores are plain vector stores and global atomics.
 *
 *   The range cell: two uint32 words in DEVICE memory, owned by the caller, holding the smallest and the largest order key folded in so far
 *   (key(f) = bits ^ 0xffffffff for a negative f, bits ^ 0x80000000 otherwise: unsigned order is float order, -0.0 right below +0.0).  What is
 *   folded is nan_to_num(depth) as numpy's float32: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX.  One workgroup reduces the pixels it covers
 *   (ucnerf_image_group_pixels of them) and issues one atomicMin and one atomicMax.  ucnerf_minmax_reset empties the cell: (0xffffffff, 0),
 *   which reads back as (NaN, NaN).  ucnerf_minmax_read decodes the cell into two floats (min, max) on the device.  The values equal numpy's
 *   min / max of nan_to_num bit for bit, except that the zero numpy returns may carry the other sign (-0.0 == +0.0).
 *
 *   ucnerf_image_put: one rendered chunk into the image.  Chunk pixel i is image pixel q = first_pixel + i of the flattened H x W grid:
 *     rgb_chw[c * pixels + q] = min(max(rgb[i][c], 0), 1) by comparison, torch.clamp's semantics: a NaN stays NaN, -0.0 stays -0.0;
 *     depth_hw[q] = depth[i], unchanged;  the chunk's depths are folded into `minmax` when that is non-NULL.
 *     Chunks may arrive in any order; chunks that overlap leave the later launch's values.  UCNERF_EINVAL, checked on the host before
 *     anything is launched: a negative n, first_pixel or pixels, first_pixel + n > pixels (an overrun), a NULL required array.  n == 0 is
 *     success, nothing launched.
 *   ucnerf_depth_minmax: the same fold for any map of `count` elements (a ground-truth depth that did not come through ucnerf_image_put).
 *   ucnerf_depth_colormap: visualize_depth's arithmetic, in float32 and rounding for rounding as numpy does it:
 *     x = nan_to_num(depth);  t = (x - mi) / d (an IEEE division);  v = 255 * t (a second rounding, never fused with the first);
 *     index = uint8(v), truncated toward zero;  color[c * count + i] = float(table[index][c]) / 255 (an IEEE division: what ToTensor does).
 *     The range comes from the cell (minmax non-NULL; utils/utils.py:66-68): mi = min, d = (max - min) + float32(1e-8), all in float32 --
 *     or from the host (minmax NULL; the reference's minmax= argument, a pair of Python floats): mi = float32(range_host[0]),
 *     d = float32(range_host[1] - range_host[0] + 1e-8) formed in double.
 *     THE ONE PLACE THIS IS STRICTER THAN NUMPY: the uint8 conversion of a NaN or of a value outside 0 .. 255 is undefined there (and differs
 *     between machines); here a NaN gives 0, a v below 0 gives 0 and a v above 255 gives 255.
 *     Channel c is column c of the table as it stands.  The reference hands cv2's B, G, R rows to PIL as if they were R, G, B, so with a table
 *     in OpenCV's column order channel 0 of the picture is OpenCV's blue -- that is what the reference shows, and it is kept.
 *     Either of index / color may be NULL (not both); table is read only for color. */
int32_t ucnerf_image_group_pixels(void);   /* pixels one workgroup of the three kernels covers (1024) */
int ucnerf_minmax_reset(uint32_t* minmax, void* stream);
int ucnerf_minmax_read(const uint32_t* minmax, float* out, void* stream);   /* out [2] = (min, max) */

struct ucnerf_image_put_params {
    int32_t n;                 /* pixels of the chunk */
    int32_t first_pixel;       /* flattened row-major index of the chunk's first pixel */
    int32_t pixels;            /* H * W */
    const float* rgb;          /* [n,3] */
    const float* depth;        /* [n] */
    float* rgb_chw;            /* [3, pixels] */
    float* depth_hw;           /* [pixels] */
    uint32_t* minmax;          /* [2] range cell, or NULL */
};
typedef struct ucnerf_image_put_params ucnerf_image_put_params;
int ucnerf_image_put(const ucnerf_image_put_params* p, void* stream);

struct ucnerf_depth_minmax_params {
    int32_t count;
    const float* depth;        /* [count] */
    uint32_t* minmax;          /* [2] range cell, folded into (reset it first) */
};
typedef struct ucnerf_depth_minmax_params ucnerf_depth_minmax_params;
int ucnerf_depth_minmax(const ucnerf_depth_minmax_params* p, void* stream);

struct ucnerf_depth_colormap_params {
    int32_t count;
    double range_host[2];      /* (mi, ma) as the caller's Python floats; read when minmax is NULL */
    const float* depth;        /* [count] */
    const uint32_t* minmax;    /* [2] range cell, or NULL */
    const uint8_t* table;      /* [256,3] colours, or NULL when color is NULL */
    uint8_t* index;            /* [count] out, or NULL */
    float* color;              /* [3, count] out, or NULL */
};
typedef struct ucnerf_depth_colormap_params ucnerf_depth_colormap_params;
int ucnerf_depth_colormap(const ucnerf_depth_colormap_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * d1   one training / validation sample out of a scene that is resident on the device -- data/scared.py:387-522 (ScaredDataset.__getitem__: PIL,
 *      ToTensor, Normalize, four cv2 resizes, 3 V projection matrices and their inverses, a shuffled keypoint list, then the DataLoader's collation
 *      and a host-to-device copy) and train.py:61-70 (unpreprocess).  Everything that is constant per FRAME is computed once on the host with the
 *      reference's own calls and uploaded (uc_nerf_amd/data/scene.py); what is left per SAMPLE is this one launch.  (Added to ABI v6; nothing above
 *      moved.  Struct declared with a tag: mirrored in _lib.ADDED_STRUCTS.)  The entry point does not synchronise the stream and reads nothing
 *      back; all stores are plain vector stores.
 *
 *   Resident inputs (N frames of H x W pixels):
 *     frames       uint8, frame f at byte f * frame_stride, [H,W,3] interleaved; frame_stride >= 3 H W and a multiple of 4, the array itself 4-byte
 *                  aligned and frame_stride * N bytes long (the bytes are read as whole dwords, four pixels = three dwords per thread)
 *     depth_img, weight_img   [N,H,W]   the sparse depth map and the normalised weight map
 *     row1, col1, row2, col2  int32 [h1], [w1], [h2], [w2]: source row / column of every row / column of the two nearest-neighbour pyramid levels
 *     kp_depth, kp_weight [K], kp_coord int32 [K,2] = (h, w): the keypoint lists of all frames, concatenated; the target's are kp_first .. + n_kp - 1
 *     c2w, w2c [N,4,4]; intrinsic [N,3,3]; affine, affine_inv [N,3,4,4]; ref_proj_inv [N,4,4]
 *   view_ids[0] is the target, view_ids[1 .. V-1] the sources (the target may be among them).  With f = view_ids[v]:
 *     images[v][c][q]       = ((float(u) / 255.0f) - mean[c]) / std[c],  u = frames[f][q][c]: an IEEE division (ToTensor), a float32 subtraction and
 *                             a second IEEE division (Normalize's sub_().div_()); three roundings, nothing contracted, no reciprocal multiply
 *     images_unpre[v][c][q] = (images[v][c][q] - unpre_mean[c]) / unpre_std[c], the same way (images_unpre may be NULL: not written)
 *     sd1[y][x] = depth_img[target][row1[y]][col1[x]], sd2 with row2 / col2; wt1, wt2 the same from weight_img
 *     rays_depth[i] = [[d, d, d], [w, w, w], [h, w_, 1]] of keypoint kp_first + perm[i], i < n_rows: what the reference's concatenate gives,
 *                     [n,3,3] (its comment says 4 x 3; the code makes three rows).  A perm[i] outside 0 .. n_kp - 1 reads nothing: the row is NaN.
 *     c2ws, w2cs, intrinsics, affine_mat, affine_mat_inv: the rows of frame f;  near_fars[v] = (near, far);  view_ids_out[v] = f (int64)
 *     proj_mats[0] = the first three rows of the identity;  proj_mats[v] = (affine[f][2] @ ref_proj_inv[target])[:3] for v >= 1, element (r, c) =
 *                     fmaf(a[r][3], b[3][c], fmaf(a[r][2], b[2][c], fmaf(a[r][1], b[1][c], a[r][0] * b[0][c]))): k = 0 .. 3 in ascending order
 *                     from a first product (torch.matmul's order is the BLAS's; this one is fixed)
 *   UCNERF_EINVAL, checked on the host before anything is launched: a negative count or size, H W > 2^24, V outside 1..9, a view id outside
 *   0 .. N-1, n_rows > 1024 or n_rows > n_kp, a keypoint segment that overruns kp_total, a pyramid level larger than the image, frame_stride too small or not a multiple of 4, a NULL
 *   required pointer (kp_* and perm are required only when n_rows > 0; images_unpre is optional).  n_rows == 0 is legal: a frame without keypoints
 *   gives an empty rays_depth.  Bound: latency (V H W 3 bytes in, 4 to 8 times that out: a few microseconds of traffic). */
struct ucnerf_sample_assemble_params {
    int32_t N, H, W, V;
    int32_t h1, w1, h2, w2;    /* pyramid levels: (H / 4, W / 4) and (H / 2, W / 2) in the reference */
    int32_t frame_stride;      /* bytes between frames */
    int32_t kp_total;          /* K: keypoints of all frames */
    int32_t kp_first, n_kp;    /* the target's segment of the keypoint lists: kp_first + n_kp <= kp_total */
    int32_t n_rows;            /* rows of rays_depth: min(n_kp, 1024) in the reference */
    int32_t view_ids[9];
    float mean[3], std[3];     /* Normalize's */
    float unpre_mean[3], unpre_std[3];
    float near_far[2];
    const uint8_t* frames;
    const float* depth_img;
    const float* weight_img;
    const int32_t* row1;
    const int32_t* col1;
    const int32_t* row2;
    const int32_t* col2;
    const float* kp_depth;
    const float* kp_weight;
    const int32_t* kp_coord;
    const int32_t* perm;       /* [>= n_rows] distinct indices below n_kp */
    const float* c2w;
    const float* w2c;
    const float* intrinsic;
    const float* affine;
    const float* affine_inv;
    const float* ref_proj_inv;
    float* images;             /* [V,3,H,W] */
    float* images_unpre;       /* [V,3,H,W], or NULL */
    float* sd1;                /* [h1,w1] */
    float* sd2;                /* [h2,w2] */
    float* wt1;
    float* wt2;
    float* rays_depth;         /* [n_rows,3,3] */
    float* c2ws;               /* [V,4,4] */
    float* w2cs;
    float* intrinsics;         /* [V,3,3] */
    float* affine_mat;         /* [V,3,4,4] */
    float* affine_mat_inv;
    float* proj_mats;          /* [V,3,4] */
    float* near_fars;          /* [V,2] */
    int64_t* view_ids_out;     /* [V] */
};
typedef struct ucnerf_sample_assemble_params ucnerf_sample_assemble_params;
int ucnerf_sample_assemble(const ucnerf_sample_assemble_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * f3   the cascade depth loss on the device -- network/mvs_models.py:512-529 (cas_mvsnet_loss) without its boolean-mask indexing: est[mask],
 *      gt[mask] and w[w > 0] compact, compaction needs the element counts on the host, and a step that reads the device back cannot be captured
 *      into a graph.  Here the counts stay on the device.  (Added to ABI v6; nothing above moved.  Structs declared with a tag: mirrored in
 *      _lib.ADDED_STRUCTS.)
 *
 *   per stage s (1 to 3 stages, est / gt / w [n[s]] each):
 *     valid(i)   = gt[i] > 0  (a NaN is not valid);   positive(j) = w[j] > 0
 *     the k-th valid element in row-major order is paired with the k-th positive weight in row-major order -- NOT with the weight at its
 *     own pixel (the two coincide only where both maps are positive at exactly the same pixels)
 *     term(i)    = smooth-L1, beta 1, of d = est[i] - gt[i]:  0.5 d^2 for |d| < 1, |d| - 0.5 otherwise
 *     stage_loss[s] = sum over valid i of term(i) * weight(i)  /  float(count[s]),   count[s] = the number of valid elements
 *   total = ((0 + stage_w[0] stage_loss[0]) + stage_w[1] stage_loss[1]) + ...      (the reference's order)
 *   with_weight == 0: the weights are not read (w may be NULL) and wpair is 1 on the valid elements.
 *
 *   Edge semantics
 *     - no valid element: stage_loss[s] = 0 / 0 = NaN, as torch's mean of an empty tensor; the NaN propagates into total.
 *     - with weights on, count[s] != the number of positive weights (torch raises there, which a device cannot do without a read-back):
 *       stage_loss[s] = NaN, wpair = NaN on the valid elements (so the gradients are NaN there too), and bit s of *status is set.  *status is a
 *       caller-provided device word, only ever OR-ed into (sticky); it may be NULL.
 *       THE ONE DIFFERENCE FROM TORCH: where exactly one of the two counts is 1, torch broadcasts the single value; this is a mismatch here.
 *     - n_stages outside 1..3, an n[s] outside 1..2^30, a NULL required pointer: UCNERF_EINVAL (a stage of zero elements is NOT an empty batch:
 *       its loss would be NaN, which only a launch can write).
 *
 *   One launch of ONE workgroup of 1024 threads, the stages one after the other, so that `total` is formed in the same launch by the thread
 *   that holds the stage losses: no workgroup waits for, polls or signals another.  Per stage: wave v owns the contiguous run of
 *   ceil(ceil(n / 64) / 16) tiles of 64 elements from v times that on (contiguous runs keep ranks in row-major order; a tile is one coalesced
 *   load); pass 1 counts valid elements and positive weights per wave (ballot + popcount: integers), exclusive offsets over the 16 waves from
 *   LDS; pass 2 writes the positive weights to workspace[rank]; a barrier makes the workgroup's own stores visible to itself; pass 3 reads
 *   workspace[rank] at the valid elements, forms the terms, writes wpair and sums in a fixed order -- per lane over its tiles, a shuffle tree
 *   over the wave, a pairwise tree over the 16 waves.  The order depends on the shapes alone: the same inputs give the same bits.
 *   Bound: latency (one CU; about 1 MB read at the reference's 256 x 320 stage sizes).
 *
 *   ucnerf_cas_loss_bwd: elementwise, grid over all stages, every element of g_est written (no zero fill):
 *     g_est[s][i] = valid(i) ? ((g_total[0] * stage_w[s] (+ g_stage[s])) / float(count[s])) * wpair[s][i] * clamp(est - gt, -1, 1) : 0
 *   g_total and count are read on the device; the division is a division (torch's mean backward), not a multiplication by a reciprocal. */
int64_t ucnerf_cas_loss_workspace_floats(int32_t n_stages, const int32_t* n_host);   /* sum of n[s]; < 0 on a bad argument */

struct ucnerf_cas_loss_params {
    int32_t n_stages;          /* 1..3 */
    int32_t with_weight;
    int32_t n[3];              /* elements per stage */
    float stage_w[3];          /* the reference: 0.5, 1, 2 by the stage number in the key */
    const float* est[3];       /* [n[s]] */
    const float* gt[3];        /* [n[s]] */
    const float* w[3];         /* [n[s]]; not read (may be NULL) when with_weight == 0 */
    float* workspace;          /* ucnerf_cas_loss_workspace_floats(n_stages, n) floats; not used (may be NULL) when with_weight == 0 */
    float* total;              /* [1] */
    float* stage_loss;         /* [n_stages] */
    int32_t* count;            /* [n_stages] valid elements */
    float* wpair[3];           /* [n[s]] the weight each element was paired with, 0 where it is not valid; all NULL: not written */
    int32_t* status;           /* [1] sticky mismatch bits, or NULL */
};
typedef struct ucnerf_cas_loss_params ucnerf_cas_loss_params;
int ucnerf_cas_loss_fwd(const ucnerf_cas_loss_params* p, void* stream);

struct ucnerf_cas_loss_bwd_params {
    int32_t n_stages;
    int32_t n[3];
    float stage_w[3];
    const float* est[3];       /* the forward's inputs ... */
    const float* gt[3];
    const float* wpair[3];     /* ... and outputs */
    const int32_t* count;      /* [n_stages] */
    const float* g_total;      /* [1] */
    const float* g_stage;      /* [n_stages] upstream gradient of stage_loss, or NULL */
    float* g_est[3];           /* [n[s]] out */
};
typedef struct ucnerf_cas_loss_bwd_params ucnerf_cas_loss_bwd_params;
int ucnerf_cas_loss_bwd(const ucnerf_cas_loss_bwd_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a10  one fused render pass -- network/renderer.py:215-255 (rendering) with the projection of
 *      utils/utils.py:716-724 in front: rays + depths -> world points -> stage coordinates -> features ->
 *      PE + MLP -> composite.  Source views = pose entries 1..V of the reference's pose_ref
 *      (the in-place trim of renderer.py:241-243 is host-side behaviour and stays in the Python mirror).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, S;
    int32_t white_bkgd;
    int32_t max_blocks;        /* MLP persistent grid cap, 0 = auto */
    ucnerf_mlp_config cfg;
    /* geometry */
    const float* rays_o;       /* [3] shared origin */
    const float* rays_d;       /* [n,3] */
    const float* z;            /* [n,S] */
    float w2c_ref[12];         /* reference view: projection for the stage/ndc coordinates */
    float K_ref[9];
    float w2c_dir[12];         /* rotation used for the view-direction feature (pose_ref['w2cs'][0] at call time) */
    float near, far;           /* scene range */
    const float* near_far;     /* [n,6] per-ray cascade ranges, or NULL: all stages use (near, far) */
    /* gather sources, see ucnerf_feat_gather_params */
    int32_t H, W;
    int32_t vol_d[3], vol_h[3], vol_w[3];
    const float* vol[3];
    const float* conf;
    const float* imgs;
    const float* img_feat;
    const float* w2cs;         /* [V,12] source views */
    const float* intrinsics;   /* [V,9] */
    const float* wstream;
    ucnerf_cl_sources cl;      /* optional (ABI v5; all five pointers or none): the sources channel-last, each in its own allocation -- handed over
                                  in place by a producer that writes that layout (vol / imgs / img_feat above may then be NULL) and / or built by
                                  ucnerf_gather_repack.  When given and `feats` is NULL, the pass uses the fast gather that reads them and derives the
                                  sample coordinates itself; vol/imgs/img_feat are then not touched.  REQUIRED when
                                  cfg.precision == 3 (the gather then runs inside the MLP kernel: no feature buffer).
                                  cl.bf16 = 1 (bf16 copies, ucnerf_gather_repack with the same flag: 16-byte voxels and feature pixels, 8-byte colours,
                                  values rounded to nearest even) -- SURVEY.md 8 configs[4] "fp32 MLP / bf16 features": half the bytes of every
                                  gather corner, features within bf16 rounding of the fp32 sources'.  Forward only reads differ; the backward
                                  accumulates source gradients in fp32 as before.  With cfg.precision == 3: derived coordinates only */
    /* workspace: ucnerf_render_workspace_floats(n, S, V) floats */
    float* workspace;
    /* outputs */
    float* rgb_map;            /* [n,3] */
    float* depth_map;          /* [n]   (rgb_map and depth_map both NULL, raw given: the pass evaluates the network into raw and composites
                                  nothing -- no compositing launch, no other output; for rows composited by ucnerf_composite_merged_fwd) */
    float* acc_map;            /* [n] or NULL */
    float* weights;            /* [n,S] or NULL */
    float* var;                /* [n] or NULL */
    float* raw;                /* [n,S,4] or NULL (kept for backward) */
    float* feats;              /* [n*S,F] row-major or NULL (kept for backward) */
    /* optional timing hooks: events (ucnerf_event_create) recorded on `stream` right before / after the MLP kernel */
    void* ev_mlp_start;
    void* ev_mlp_stop;
    float* train_workspace;    /* optional (training forward; needs raw and feats): the workspace of the coming
                                  ucnerf_render_fused_bwd call -- the MLP activations are kept there, see
                                  ucnerf_render_bwd_params.saved_valid */
    const float* dir_feat;     /* optional [n,3]: the view-direction feature already computed (ucnerf_ray_gen.angle or
                                  ucnerf_dir_feature with w2c_dir); NULL: the pass computes it itself */
    /* opt-in uncertainty outputs (SURVEY.md 8(a) note): */
    float* u_sampled;          /* [n,S] or NULL: u = 1 - confidence sampled at every depth (network/models.py:149) */
    float* wu_map;             /* [n] or NULL: sum_i w_i u_i */
    /* Coordinates GIVEN by the caller instead of derived from (rays_d, z): what rendering() of the reference receives
     * from build_rays / build_rays_test (network/renderer.py:215-255: rays_pts, rays_ndc).  All five or none; when set,
     * rays_o / rays_d / z are used for the view direction and the compositing only and near_far is ignored. */
    const float* pts_in;       /* [n*S,3] world points */
    const float* ndc1_in;      /* [n*S,3] stage coordinates in ~[0,1] */
    const float* ndc2_in;
    const float* ndc3_in;
    const float* ndc_in;       /* [n*S,3] scene-normalised copy fed to the positional encoding */
    int32_t feats_tiled;       /* layout of `feats` when it is kept: 0 row-major [n*S,F]; 1 the MLP's tile layout [ceil(n*S/32)][F][32]
                                  (ceil(n*S/32)*32*F floats) -- what the training forward reads three times faster (coalesced 128-byte
                                  rows instead of 4-byte pieces of 388-byte rows) and ucnerf_render_fused_bwd (bwd_mode 0) accepts */
    int32_t train_bwd_mode;    /* with train_workspace: the bwd_mode of the coming ucnerf_render_fused_bwd call (it fixes the format the
                                  activations are kept in, see ucnerf_mlp_fwd_train) */
    /* ABI v4: the launches around a coarse pass folded into it (data/ray_utils.py:199-224 chains them; at 512 rays per GPU each ~5-us launch
     * is 4 % of the step) */
    const ucnerf_sample_pdf_params* resample;   /* optional (HOST pointer): the pass's compositing launch also draws the NEXT pass's depths from its
                                  weights -- ucnerf_composite_sample_pdf(this pass's compositing, *resample) instead of ucnerf_composite_fwd;
                                  resample->weights / z_merge may be NULL (implied: this pass's weights and z) */
    const float* w2c_dir_dev;  /* ABI v5, optional DEVICE pointer to the rotation of the view-direction feature, row-major with 4 columns (a [3,4] or
                                  [4,4] tensor): used instead of w2c_dir when dir_feat is NULL and this is set -- rendering() holds
                                  pose_ref['w2cs'][0] on the device and need not read it back.  On the tail route the features are then made
                                  in the blocks' prologues (no ucnerf_dir_feature launch) */
    const ucnerf_ray_gen_params* gen_rays;      /* optional (HOST pointers, both or none; cfg.precision == 3, derived coordinates, xs / ys pixel lists): the */
    const ucnerf_sample_stratified_params* gen_depths;  /* fused launch generates its own rays and stratified depths -- ucnerf_ray_gen_sample folded into the
                                  kernel's per-tile prologue.  rays_d / z / dir_feat of THIS struct are then buffers the launch FILLS (they must
                                  equal gen_rays->rays_d / gen_depths->z / gen_rays->angle; later passes and the compositing read them);
                                  same values as ucnerf_ray_gen_sample, bit for bit */
} ucnerf_render_params;
int64_t ucnerf_render_workspace_floats(int32_t n, int32_t S, int32_t V);
int ucnerf_render_fused_fwd(const ucnerf_render_params* p, void* stream);
/* The guarded fp16 split of a whole pass (see ucnerf_mlp_fwd_guarded): same parameters, plus the status / condition word. */
int ucnerf_render_fused_fwd_guarded(const ucnerf_render_params* p, uint32_t* status, void* stream);
int ucnerf_render_fused_fwd_if(const ucnerf_render_params* p, const uint32_t* run_if, void* stream);
/* Channel-last repack of the gather sources named in `p` (vol[3] -> [D,h,w,8] each, img_feat -> [V,H,W,8], imgs -> [V,H,W,4] = (r,g,b,0); fp32, or
 * bf16 when p->cl.bf16) into `dst` (ucnerf_gather_repack_floats(p) floats, 16-byte aligned), and the pointers of the result into `out` (rgb_stride 4,
 * bf16 as asked).  PER SOURCE: an entry of p->cl that is already set -- a source handed over in place -- is kept as it is (copied to `out`, nothing
 * read or written for it, no room taken in dst; with p->cl.bf16 the in-place entries must hold bf16 too); its reference-layout pointer may be NULL.
 * Redo it whenever the repacked sources change (once per image in evaluation, once per step in training): ~150 MB of traffic for all five. */
int64_t ucnerf_gather_repack_floats(const ucnerf_render_params* p);
int ucnerf_gather_repack(const ucnerf_render_params* p, float* dst, ucnerf_cl_sources* out, void* stream);
/* The same, for the sources named in `source_mask` only (additive to ABI v6): bits 0..2 the volumes, bit 3 the image features, bit 4 the colours;
 * ucnerf_gather_repack is this call with UCNERF_REPACK_ALL.  A source whose bit is clear is neither read nor written: its part of `dst` keeps what an
 * earlier call left there.  The layout of `dst` does not depend on the mask -- `out` receives the entries of the full repack on every call -- and
 * every source that is written gets the very bytes the full repack writes.  A bit that names a source handed over in place is ignored; a null
 * reference-layout pointer is an error only for a source that is written.  source_mask == 0: no launch, UCNERF_OK.  For a caller that knows which
 * sources changed since their copies were made (images stay while volumes and feature maps are replaced: 0x0f instead of all five). */
#define UCNERF_REPACK_ALL 0x1fu
int ucnerf_gather_repack_masked(const ucnerf_render_params* p, float* dst, ucnerf_cl_sources* out, uint32_t source_mask, void* stream);

/* Backward of one render pass: d(rgb_map, depth_map) -> d(parameters), d(volumes, img_feat, confidence).
 * fwd.raw and fwd.feats must point at the buffers the forward call filled (keep them); all g_* outputs are
 * ACCUMULATED (zero them first). */
typedef struct {
    ucnerf_render_params fwd;
    const float* g_rgb;            /* [n,3] */
    const float* g_depth;          /* [n] or NULL */
    const float* flat_params;      /* [param_count] */
    float* g_flat;                 /* [param_count] accumulated */
    float* g_vol[3];               /* accumulated or NULL */
    float* g_conf;
    float* g_img_feat;
    float* workspace;              /* ucnerf_render_bwd_workspace_floats(n, S, V) floats, 16-byte aligned */
    float* gather_scratch;         /* optional: ucnerf_feat_gather_bwd_params.scratch for the gather backward */
    int32_t saved_valid;           /* 1: the forward call was given this `workspace` as fwd.train_workspace (it kept the
                                      MLP activations there), so the backward does not repeat the network forward */
    int32_t bwd_mode;              /* ucnerf_mlp_bwd_params.bwd_mode */
    ucnerf_cl_grads g_cl;          /* ABI v5, per source: ucnerf_feat_gather_bwd_params.g_cl -- source gradients accumulated in the channel-last
                                      layout of the in-place sources (that source's g_vol / g_img_feat entry is then ignored; g_conf as before) */
} ucnerf_render_bwd_params;
int64_t ucnerf_render_bwd_workspace_floats(int32_t n, int32_t S, int32_t V);
int ucnerf_render_fused_bwd(const ucnerf_render_bwd_params* p, void* stream);

/* Gradient fold of the compositing's extra maps (added to ABI v6; nothing above moved): lets a loss on var, disp or the composited uncertainty
 * wu = sum_i w_i u_i (ucnerf_composite_params.var / disp_map / wu) reach the network through the backward kernels there are.  All three maps are
 * functions of weights, depth and acc, whose gradients ucnerf_composite_bwd / ucnerf_composite_merged_bwd accept; this launch adds their
 * chain-rule terms to the upstream gradients of those three, and the existing backward then runs unchanged on the results.  Per ray, S samples:
 *   g_weights_out[i] = g_weights[i] + g_var * (2 * (w_i - mean(w)) / (S - 1)) + g_wu * u_i        (var: unbiased, of torch.var_mean)
 *   g_depth_out      = g_depth + g_disp * (-(disp^2 / acc))                                      (disp = 1 / (depth / acc))
 *   g_acc_out        = g_acc   + g_disp * ((disp^2 / acc) * (depth / acc))
 *   g_u[i]           = g_wu * w_i
 * in fp32, each operation rounded on its own, terms added in the order written; a NULL upstream gradient is zero.  The disp terms are zero at
 * a ray whose depth / acc is <= 1e-10 (the clamp of 1 / max(1e-10, depth / acc) is active) or not finite.  At depth / acc == 1e-10 exactly
 * torch.maximum hands half of the gradient to each side; this kernel hands none -- a tie of measure zero.
 * One 64-lane wave per ray, lane split of ucnerf_composite_fwd (ceil(S/64) -> 1, 2, 3, 4, 8, 16 samples per lane): mean(w) is the forward's
 * acc / S, bit for bit.  Every element of every output is written exactly once -- no atomics, no zero fill; a second call into the same buffers
 * gives the same bits.  The merged route needs nothing else: weights, u and the upstream gradients are in merged order already.
 * 1 <= S <= 1024.  weights, depth, acc, g_depth_out, g_acc_out and g_weights_out are required; u, g_u and every upstream gradient may be NULL.
 * UCNERF_EINVAL: g_var with S < 2, g_wu without u, an output that overlaps an input or another output, a negative count.  n == 0: success.
 * (Declared with a struct tag: mirrored in _lib.ADDED_STRUCTS.) */
struct ucnerf_composite_fold_params {
    int32_t n, S;
    const float* weights;      /* [n,S] the forward's outputs ... */
    const float* depth;        /* [n] */
    const float* acc;          /* [n] */
    const float* u;            /* [n,S] the forward's per-sample uncertainty, or NULL */
    const float* g_var;        /* [n] or NULL: upstream gradients of the extra maps ... */
    const float* g_disp;       /* [n] or NULL */
    const float* g_wu;         /* [n] or NULL (needs u) */
    const float* g_depth;      /* [n] or NULL: ... and of the maps the backward kernels take */
    const float* g_acc;        /* [n] or NULL */
    const float* g_weights;    /* [n,S] or NULL */
    float* g_depth_out;        /* [n] */
    float* g_acc_out;          /* [n] */
    float* g_weights_out;      /* [n,S] */
    float* g_u;                /* [n,S] or NULL: gradient of u (zeros without g_wu) */
};
typedef struct ucnerf_composite_fold_params ucnerf_composite_fold_params;
int ucnerf_composite_fold_grads(const ucnerf_composite_fold_params* p, void* stream);

/* Training FeatureNet on the device: the backward of ucnerf_conv2d_bias_relu for the layers of the feature pyramid (added to ABI v6; nothing
 * above moved; structs declared with a tag: mirrored in _lib.ADDED_STRUCTS).  float32, NCHW contiguous.  No atomics, plain vector stores only,
 * two calls give the same bits.  The INPUT gradient of a stride-1 layer needs no entry point of its own: it is ucnerf_conv2d_bias_relu on grad_y
 * with the weight transposed and flipped, zero bias, no ReLU (uc_nerf_amd.ops.conv2d_dgrad).
 *
 * ucnerf_conv2d_wgrad: grad_weight[co][ci][ky][kx] = sum over (img, oy, ox) of grad_y[img,co,oy,ox] x[img,ci, stride oy - pad + ky, stride ox - pad + kx],
 *   a tap outside the image entering as the product a * +0.  K 1, 3 or 5, pad = (K - 1) / 2, stride 1, or 2 with K 3 or 5;
 *   OH = (H + 2 pad - K) / stride + 1, OW likewise.  Exact fp32 products and fp32 accumulation on v_mfma_f32_16x16x4_f32: rows = cout, columns =
 *   the flat (ci, ky, kx), and the output pixels v = (img OH + oy) OW + ox are the reduction dimension, cut into chunks of whole output rows.
 *   SUMMATION ORDER (fixed, part of the interface).  With / the integer division and ceil(a / b) = (a + b - 1) / b:
 *     OW4 = 4 ceil(OW / 4);  SW = min(OW4, 128);  WP = stride (SW - 1) + K;  CG0 = min(cin, 256 / (K K));
 *     RR = 1 when OW4 > 128 or no larger value fits, else the largest r in 2 .. 128 / OW4 with CG0 ((r - 1) stride + K) WP <= 11264;
 *     CG = min(CG0, 11264 / (((RR - 1) stride + K) WP));  tiles = ceil(cout / 32) ceil(cin / CG);  G = n OH (the rows of all images);
 *     C0 = max(1, min(ceil(G / RR), ceil(512 / tiles)));  the chunk length RC = RR ceil(G / (RR C0)) rows;  chunks = ceil(G / RC); chunk c is the
 *     rows [c RC, min((c + 1) RC, G)), that is the pixels v in [c RC OW, ...).
 *     Within a chunk P_c = one fmaf chain from +0 over ascending v (the MFMA adds four consecutive pixels of a row per instruction, the lowest
 *     first; a row whose length is no multiple of 4 is padded with products +0 * +0, which change no bit).  grad_weight = (((+0 + P_0) + P_1)
 *     + ...) over ascending c, by a second launch.
 *   workspace: ucnerf_conv2d_wgrad_workspace_floats(...) = chunks cout cin K K floats, laid out [chunk][cout][cin K K], every element overwritten;
 *     < 0 on a bad argument; pure host.  Limits: cin, cout <= 2^16; n cin H W, n cout OH OW < 2^31; n OH < 2^31 - 1024; cin cout K K < 2^31.
 *
 * ucnerf_conv2d_dgrad_s2: the input gradient of a stride-2 layer with K 3 or 5 and pad (K - 1) / 2; H and W (of x) even, so OH = H / 2, OW = W / 2
 *   (an odd size is UCNERF_EINVAL).  `weight` is the layer's RAW [cout,cin,K,K] weight: nothing is packed.  By parity class of the input pixel:
 *   py = (iy + pad) & 1, the taps ky = py + 2 jy, jy = 0 .. nky - 1, nky = (K - py + 1) / 2, reach iy from the source row (iy + pad - ky) / 2; px,
 *   jx, nkx likewise.  grad_x[img,ci,iy,ix] = sum over k' = (co nky + jy) nkx + jx, ascending, of grad_y[img,co,(iy + pad - ky) / 2,
 *   (ix + pad - kx) / 2] w[co,ci,ky,kx], a source outside grad_y contributing +0, in the blocked order of ucnerf_conv2d_bias_relu: runs of 32
 *   consecutive k', each an fmaf chain from +0 (the last one may be shorter), T = (((+0 + S_0) + S_1) + ...) ascending.  Exact fp32, one thread per
 *   element.  Limits: n <= 16383; cin <= 65535; n cin H W, cin cout K K < 2^31.
 *
 * ucnerf_conv2d_bias_grad: grad_bias[co] = sum of grad_y[:,co,:,:] ([n,cout,OH,OW]) in float64, rounded once.  Order: thread t of 1024 adds,
 *   image after image, the pixels s = t, t + 1024, ... of the channel's plane ascending, from 0; then for d = 512, 256, .. 1 thread t < d adds
 *   thread t + d's sum.  n cout OH OW < 2^31.
 *
 * UCNERF_EINVAL with ucnerf_last_error before any device call, for all three: NULL params or array, negative n, non-positive sizes, a K /
 *   stride / pad outside the above, an odd H or W (dgrad_s2), workspace_floats that does not match the query (wgrad).  n == 0 is success, nothing
 *   launched. */
struct ucnerf_conv2d_wgrad_params {
    int32_t n, cin, H, W, cout, K, stride, pad;   /* of the layer: x is [n,cin,H,W] */
    int64_t workspace_floats;  /* floats `workspace` holds = ucnerf_conv2d_wgrad_workspace_floats(the same arguments) */
    const float* x;            /* [n,cin,H,W] */
    const float* grad_y;       /* [n,cout,OH,OW] */
    float* workspace;          /* overwritten */
    float* grad_weight;        /* [cout,cin,K,K], overwritten */
};
typedef struct ucnerf_conv2d_wgrad_params ucnerf_conv2d_wgrad_params;
int64_t ucnerf_conv2d_wgrad_workspace_floats(int32_t n, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t K, int32_t stride, int32_t pad);
int ucnerf_conv2d_wgrad(const ucnerf_conv2d_wgrad_params* p, void* stream);

struct ucnerf_conv2d_dgrad_s2_params {
    int32_t n, cin, H, W, cout, K;   /* of the layer: grad_x is [n,cin,H,W] */
    const float* grad_y;       /* [n,cout,H/2,W/2] */
    const float* weight;       /* [cout,cin,K,K], the layer's raw weight */
    float* grad_x;             /* [n,cin,H,W], overwritten */
};
typedef struct ucnerf_conv2d_dgrad_s2_params ucnerf_conv2d_dgrad_s2_params;
int ucnerf_conv2d_dgrad_s2(const ucnerf_conv2d_dgrad_s2_params* p, void* stream);

struct ucnerf_conv2d_bias_grad_params {
    int32_t n, cout, OH, OW;
    const float* grad_y;       /* [n,cout,OH,OW] */
    float* grad_bias;          /* [cout], overwritten */
};
typedef struct ucnerf_conv2d_bias_grad_params ucnerf_conv2d_bias_grad_params;
int ucnerf_conv2d_bias_grad(const ucnerf_conv2d_bias_grad_params* p, void* stream);

/* Grouped batch-statistic batch-norm: the four batch-norm entry points above with the statistics kept PER GROUP OF IMAGES, so that FeatureNet
 * runs once over all the views of a sample and still normalises every view with its own statistics, as the reference's per-view calls do
 * (mvs_models.py:701-704).  (Added to ABI v6; nothing above moved; structs declared with a tag: mirrored in _lib.ADDED_STRUCTS.)
 * y, g, out, skip and grad_y are contiguous float32 [G, n, C, S]; group q is the n images q n .. q n + n - 1, its slab starts at q n C S floats;
 * within a group a channel has N = n S values, numbered as above.  Every struct is its ungrouped counterpart's with G in front.
 *
 * CONTRACT: for every group the values computed are those the ungrouped pair computes on that group's [n,C,S] slab alone, BIT FOR BIT: the same
 *   P = ucnerf_bn_partials(n, S) and the same slices, the same thread / lane / wave / slice merge order in float64, the same single roundings, the
 *   same float32 fma(y - mu, s, bias) with IEEE division and square root.  There is one code path (csrc/bn.hip, four kernels with the group on
 *   the grid's third dimension): the ungrouped entry points copy their struct behind G = 1 and call what these call, so G == 1 IS the ungrouped
 *   entry points in every output, and what a group computes does not depend on G.
 * Workspaces: [G,C,P,3] float64 for the statistics (triple j of channel c of group q at ((q C + c) P + j) 3), [G,C,P,2] for the backward.
 * saved_mean and saved_var are [G,C]: group q's mu and sigma^2.
 * Running statistics: the first block of (channel, group q) writes saved_mean / saved_var [q, c] from its own fold; the first block of
 *   (channel, group 0) also folds, where G > 1, the triples of the other groups (thread q group q, the fold of the apply blocks) and one thread
 *   then applies, in float32 with separate multiplications and additions, for q = 0 .. G - 1 ascending: running_mean = (1 - m) running_mean +
 *   m mu_q, running_var = (1 - m) running_var + m u_q (u_q the unbiased variance rounded once) -- exactly what G successive ungrouped calls on
 *   the slabs leave behind.  One thread of the launch adds G to *num_batches_tracked.
 * Backward: grad_y of group q is the ungrouped backward's on that slab, with saved_mean[q], saved_var[q].  The parameter gradients are sums over
 *   the groups: the block that owns channel c folds every group's pairs as above, (A_q, B_q), r_q = 1 / sqrt(sigma_q^2 + eps), and adds in
 *   float64, q ascending, grad_bias[c] = ((A_0 + A_1) + ...), grad_weight[c] = ((B_0 r_0 + B_1 r_1) + ...), each rounded ONCE to float32.  (These are
 *   not the bits G ungrouped calls followed by float32 additions give: those carry G roundings.)
 * out may be y, grad_y may be g (not a shifted overlap).  No atomics, every store a plain vector store, nothing is read back, two calls give the
 *   same bits, the launches can sit in a captured graph.  16-byte accesses where S % 4 == 0 and the arrays are 16-byte aligned (every group base
 *   then is: a slab is a multiple of four floats), 4-byte ones otherwise, the same values in the same order.
 * UCNERF_EINVAL before any device call: everything the ungrouped entry refuses for (n, C, S) and its arrays, and G < 1, G > 64, G n S above the
 *   limit on N (2^31 - 2^20), a G n C S that overflows, workspace_triples / workspace_pairs < G C P. */
struct ucnerf_bn_stats_groups_params {
    int64_t G, n, C, S;
    int64_t workspace_triples; /* at least G C P */
    const float* y;            /* [G,n,C,S] */
    double* workspace;         /* [G,C,P,3], overwritten */
};
typedef struct ucnerf_bn_stats_groups_params ucnerf_bn_stats_groups_params;
int ucnerf_bn_stats_groups(const ucnerf_bn_stats_groups_params* p, void* stream);

struct ucnerf_bn_apply_groups_params {
    int64_t G, n, C, S;
    int64_t workspace_triples;
    float eps, momentum;
    int32_t relu;
    int32_t reserved;
    const float* y;            /* [G,n,C,S], as ucnerf_bn_stats_groups read it */
    const double* workspace;   /* as ucnerf_bn_stats_groups wrote it for the same G, n, C, S */
    const float* weight;       /* gamma [C] */
    const float* bias;         /* beta [C] */
    const float* skip;         /* y's shape, or NULL */
    float* out;                /* y's shape; may be y */
    float* saved_mean;         /* [G,C], overwritten */
    float* saved_var;          /* [G,C], overwritten: the biased variances */
    float* running_mean;       /* [C], moved G times */
    float* running_var;        /* [C], moved G times */
    int64_t* num_batches_tracked;   /* one int64 on the device, G is added */
};
typedef struct ucnerf_bn_apply_groups_params ucnerf_bn_apply_groups_params;
int ucnerf_bn_apply_groups(const ucnerf_bn_apply_groups_params* p, void* stream);

struct ucnerf_bn_bwd_reduce_groups_params {
    int64_t G, n, C, S;
    int64_t workspace_pairs;   /* at least G C P */
    float eps;
    int32_t relu;
    const float* g;            /* [G,n,C,S] */
    const float* y;            /* [G,n,C,S], the forward's input */
    const float* saved_mean;   /* [G,C] */
    const float* saved_var;    /* [G,C] */
    const float* weight;       /* gamma [C] */
    const float* bias;         /* beta [C] */
    double* workspace;         /* [G,C,P,2], overwritten */
};
typedef struct ucnerf_bn_bwd_reduce_groups_params ucnerf_bn_bwd_reduce_groups_params;
int ucnerf_bn_bwd_reduce_groups(const ucnerf_bn_bwd_reduce_groups_params* p, void* stream);

struct ucnerf_bn_bwd_apply_groups_params {
    int64_t G, n, C, S;
    int64_t workspace_pairs;
    float eps;
    int32_t relu;
    const float* g;
    const float* y;
    const float* saved_mean;
    const float* saved_var;
    const float* weight;
    const float* bias;
    const double* workspace;   /* as ucnerf_bn_bwd_reduce_groups wrote it for the same arguments */
    float* grad_y;             /* [G,n,C,S]; may be g */
    float* grad_weight;        /* [C], overwritten: the sum over the groups */
    float* grad_bias;          /* [C], overwritten: the sum over the groups */
};
typedef struct ucnerf_bn_bwd_apply_groups_params ucnerf_bn_bwd_apply_groups_params;
int ucnerf_bn_bwd_apply_groups(const ucnerf_bn_bwd_apply_groups_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * f4   the colour frames' resize on the device -- `PIL.Image.open(f).resize(self.img_wh, PIL.Image.BILINEAR)` of data/scared.py:450-451,
 *      data/hamlyn.py:507-508 and data/finetune.py:445-446, with Pillow's bits: ImagingResample for 8-bit channels, box=None, reducing_gap=None
 *      (compared byte for byte with Pillow 12.2.0; no other version was checked).  (Added to ABI v6; nothing above moved.  Struct declared with a
 *      tag: mirrored in _lib.ADDED_STRUCTS.)
 *
 *   Per axis, `in` input and `out` output pixels, everything in double (the library is built with -ffp-contract=off: nothing is fused):
 *     scale = in / out;  fs = max(scale, 1.0);  support = 1.0 * fs;  ksize = (int)ceil(support) * 2 + 1
 *     for xx in 0 .. out-1:
 *       center = (xx + 0.5) * scale
 *       start  = max((int)(center - support + 0.5), 0)                 (C truncation)
 *       count  = min((int)(center + support + 0.5), in) - start
 *       w[x]   = tri((x + start - center + 0.5) * (1.0 / fs)), x < count;  tri(a) = 1 - |a| where |a| < 1, else 0
 *       ww     = w[0] + w[1] + ... in ascending x;  w[x] /= ww where ww != 0
 *       k[x]   = (int)(0.5 + w[x] * 4194304.0)  (-0.5 for a negative w, which a triangle never gives);  k[count .. ksize-1] = 0
 *   A pass along an axis, per channel, 32-bit integer accumulator:  out[xx] = clip8((2^21 + sum_x in[start + x] * k[x]) >> 22).
 *   The HORIZONTAL pass runs first and its result is rounded and clipped to uint8; the VERTICAL pass runs on those bytes.  A pass along an axis
 *   whose size does not change is a copy (which is also what its coefficients give: one tap of 2^22).
 *
 *   ucnerf_resize_bilinear_ksize / _coeffs are host arithmetic: no device call, no allocation.  _coeffs writes start [out], count [out] and
 *   k [out][ksize] into the caller's memory and returns ksize.  Both return UCNERF_EINVAL for a size outside 1 .. 2^24 (or a NULL array).
 *
 *   ucnerf_resize_bilinear_u8: N frames in ONE launch, both passes; the uint8 intermediate lives in LDS only; integer arithmetic only.
 *     src   uint8, frame f at byte f * src_frame_stride, [Hin,Win,3] interleaved; 4-byte aligned (its bytes are read as whole dwords; the last,
 *           partial dword of the array is read byte by byte), src_frame_stride >= 3 Hin Win
 *     dst   uint8, frame f at byte f * dst_frame_stride, [H,W,3]; 4-byte aligned, dst_frame_stride >= 3 H W and a multiple of 4 (DeviceScene's
 *           padded storage).  The bytes between 3 H W and the stride are NOT written.
 *     start_x, count_x [W], k_x [W][ksize_x]: the coefficients of (Win, W) in DEVICE memory; start_y, count_y [H], k_y [H][ksize_y] those of
 *           (Hin, H).  Tables that are not the ones _coeffs gives cannot make the kernel read or write outside src / dst (every start and count is
 *           clamped into the tile a workgroup staged); the values are then unspecified.
 *   UCNERF_EINVAL before any launch: NULL params or array, N < 0, N > 65535, a size outside 1 .. 32768 or 3 Hin Win / 3 H W >= 2^31, a stride
 *   below its frame, a dst stride that is no multiple of 4, a misaligned src / dst, a ksize that is not the one the sizes imply, and an axis
 *   with in > UCNERF_RESIZE_MAX_RATIO * out: a workgroup stages the input rows and columns its 8 x 32 output tile reads, and up to that ratio the
 *   stage, the intermediate and the tile's coefficients fit in 64 KB of LDS.  N == 0 is legal and launches nothing.
 *   Bound: the HBM read of the native frames (3 N Hin Win bytes in, 3 N H W out). */
#define UCNERF_RESIZE_MAX_RATIO 16
struct ucnerf_resize_params {
    int32_t N;                 /* frames */
    int32_t Hin, Win;          /* native size */
    int32_t H, W;              /* output size */
    int32_t ksize_x, ksize_y;  /* ucnerf_resize_bilinear_ksize(Win, W), (Hin, H) */
    int32_t reserved;          /* 0 */
    int64_t src_frame_stride;  /* bytes between frames */
    int64_t dst_frame_stride;
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* start_x;
    const int32_t* count_x;
    const int32_t* k_x;
    const int32_t* start_y;
    const int32_t* count_y;
    const int32_t* k_y;
};
typedef struct ucnerf_resize_params ucnerf_resize_params;
int ucnerf_resize_bilinear_ksize(int in, int out);
int ucnerf_resize_bilinear_coeffs(int in, int out, int32_t* start, int32_t* count, int32_t* k);
int ucnerf_resize_bilinear_u8(const ucnerf_resize_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * t1   the training step's three target gathers -- train.py:166-176: sparse_depths[:, r, c] and sparse_weights[:, r, c] over the rays from
 *      n_rays on, dpt[:, r, c] over the patch rays, (r, c) the columns of pixel_coordinates.  ONE launch instead of torch's slices and index
 *      kernels; the entry point does not synchronise the stream and reads nothing back.  (Added to ABI v6; nothing above moved.  Struct
 *      declared with a tag: mirrored in _lib.ADDED_STRUCTS.)
 *
 *     sparse_depths, sparse_weights, dpt   [H,W] float32 maps, read in place
 *     pixel_coordinates   [2, n_total], row 0 the image rows, row 1 the image columns; int64 (coord_is_float = 0) or float32 holding whole
 *                         numbers (coord_is_float = 1).  Both give the same bits.
 *     target_depths[i]  = sparse_depths[r][c], target_weights[i] = sparse_weights[r][c] at column n_rays + i,  i < n_total - n_rays
 *     patch_dpt[j]      = dpt[r][c] at column j,  j < patch_num * patch_size^2
 *   Indexing is torch's advanced indexing: a row in [-H, H) or a column in [-W, W) is taken, a negative one after adding H (W).  Values are
 *   copied, never computed: every bit pattern (NaN payloads, -0.0) arrives as it is.
 *   A coordinate outside that range -- or a float32 coordinate that is no whole number, NaN and the infinities included -- reads nothing: its
 *   element is NaN (0x7fc00000) and one bit of *status is set with an atomic OR: bit 0 for a depth ray, bit 1 for a patch ray.  status may be
 *   NULL (no word is kept).  The word is sticky: the entry point never clears it.  No other element is affected.
 *   UCNERF_EINVAL before any launch: NULL params, a negative count or size, H or W above 2^24, n_total above 2^29, n_rays > n_total,
 *   patch_num * patch_size^2 > n_total, coord_is_float outside {0, 1}; and, when there is an element to write, H or W of 0, a NULL or
 *   misaligned pixel_coordinates, a NULL map or output of a non-empty part.  n_total == n_rays and patch_num == 0 are legal; with both, nothing
 *   is launched.  Bound: launch latency (a few thousand floats a step). */
struct ucnerf_step_targets_params {
    int32_t H, W;
    int32_t n_total;           /* columns of pixel_coordinates */
    int32_t n_rays;            /* the depth rays are the columns n_rays .. n_total - 1 */
    int32_t patch_num, patch_size;
    int32_t coord_is_float;    /* 0: int64 coordinates, 1: float32 */
    int32_t reserved;          /* 0 */
    const float* sparse_depths;
    const float* sparse_weights;
    const float* dpt;
    const void* pixel_coordinates;
    float* target_depths;      /* [n_total - n_rays] */
    float* target_weights;     /* [n_total - n_rays] */
    float* patch_dpt;          /* [patch_num * patch_size^2] */
    uint32_t* status;          /* one sticky word, or NULL */
};
typedef struct ucnerf_step_targets_params ucnerf_step_targets_params;
int ucnerf_step_targets(const ucnerf_step_targets_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * d3   the batch of a FREE camera pose -- what d1 (ucnerf_sample_assemble) gives for a dataset frame, for a pose that is none: the input of a
 *      rendered novel view.  The reference has the path helpers (utils/utils.py: gen_render_path, interp_poses) but no code that feeds such a pose
 *      to its renderer; on the host a novel frame would cost data/scared.py:455-484's four LAPACK inverses, a get_nearest_pose_ids
 *      (data/scared.py:69-106) and an upload.  ONE launch per novel frame; the entry point does not synchronise the stream and reads nothing
 *      back; plain vector loads and stores, no atomics, no scratch.  (Added to ABI v6; nothing above moved.  Struct declared with a tag: mirrored
 *      in _lib.ADDED_STRUCTS.)
 *
 *   Resident inputs as d1's (frames, c2w, w2c, intrinsic, affine, affine_inv of N frames of H x W pixels), and
 *     poses        [P,3,4] camera-to-world [R | t]; pose_index selects one (a host integer: the loop counter of a path)
 *     cand         int32 [n_cand]: the frames that may serve as sources (ids may repeat).  The list lives on the device, so the host cannot check
 *                  it: an entry outside 0 .. N-1 is clamped into that range before it is used
 *     intrinsic_in [3,3] or NULL (= frame 0's resident intrinsic).  ZERO SKEW IS ASSUMED: K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
 *   Source views: d_k = |c2w[cand[k]][:3,3] - t|^2 in float32, dx * dx, then fmaf(dy, dy, .), then fmaf(dz, dz, .).  The V - 1 smallest, in
 *   ascending order; equal distances resolve to the lower position k in cand (stable); a NaN distance sorts after every number, by position.
 *   This is formats.get_nearest_pose_ids with the 'dist' criterion (the square root is monotonic).  f_v = cand[k_(v-1)], v = 1 .. V-1.
 *   Outputs, with the batch-of-one shapes of d1:
 *     c2ws[0]  = the pose with the row 0 0 0 1;  w2cs[0] = the RIGID inverse in closed form, [R^T | -R^T t]: w2c[r][c] = R[c][r],
 *                w2c[r][3] = -fmaf(R[2][r], t[2], fmaf(R[1][r], t[1], R[0][r] * t[0])).  Not an LU inverse: a rotation block that is not
 *                orthonormal gives what the formula gives
 *     intrinsics[0] = K;  K_s = K with rows 0 and 1 divided by 2^(2-s) (exact), s = 0, 1, 2
 *     affine_mat[0][s][r][c] = fmaf(K_s[r][2], w2c[2][c], fmaf(K_s[r][1], w2c[1][c], K_s[r][0] * w2c[0][c])), r < 3; fourth row 0 0 0 1
 *     affine_mat_inv[0][s]   = c2w . diag(K_s^-1, 1) with the analytic K_s^-1 of a zero-skew K:  [r][0] = R[r][0] / fx_s,  [r][1] = R[r][1] / fy_s,
 *                [r][2] = fmaf(-R[r][1], cy_s / fy_s, fmaf(-R[r][0], cx_s / fx_s, R[r][2])),  [r][3] = t[r];  fourth row 0 0 0 1
 *                (IEEE divisions; not a general 4 x 4 inverse)
 *     proj_mats[0] = the first three rows of the identity;  proj_mats[v] = (affine[f_v][2] @ affine_mat_inv[0][2])[:3], d1's order: fmaf over
 *                k = 0 .. 3 ascending from a first product
 *     slots v >= 1 of c2ws, w2cs, intrinsics, affine_mat, affine_mat_inv: the rows of frame f_v, bit for bit;  near_fars[v] = (near, far), all v
 *     view_ids_out = (-1, f_1, .., f_(V-1)) int64
 *     images[v], images_unpre[v] for v >= 1: frame f_v through d1's expressions (the same bits);  slot 0 of both: 0.0f everywhere (a free pose
 *                has no ground truth; nothing on the render path reads slot 0).  images_unpre may be NULL: not written
 *   UCNERF_EINVAL before any launch: NULL params, a negative count or size, P <= 0, pose_index outside 0 .. P-1, V outside 2..9, n_cand < V,
 *   n_cand > 4096, N outside 1..2^20, H W outside 1..2^24, frame_stride too small or not a multiple of 4, a NULL required pointer, a misaligned one.
 *   Bound: latency ((V - 1) H W 3 bytes in, 4 to 8 times V H W 3 bytes out; every workgroup of slots 1 .. V-1 repeats the selection). */
struct ucnerf_novel_assemble_params {
    int32_t N, H, W, V;
    int32_t frame_stride;      /* bytes between frames */
    int32_t P;                 /* poses */
    int32_t pose_index;
    int32_t n_cand;
    float mean[3], std[3];     /* Normalize's */
    float unpre_mean[3], unpre_std[3];
    float near_far[2];
    const uint8_t* frames;
    const float* c2w;
    const float* w2c;
    const float* intrinsic;
    const float* affine;
    const float* affine_inv;
    const float* poses;        /* [P,3,4] */
    const int32_t* cand;       /* [n_cand] */
    const float* intrinsic_in; /* [3,3], or NULL */
    float* images;             /* [V,3,H,W] */
    float* images_unpre;       /* [V,3,H,W], or NULL */
    float* c2ws;               /* [V,4,4] */
    float* w2cs;
    float* intrinsics;         /* [V,3,3] */
    float* affine_mat;         /* [V,3,4,4] */
    float* affine_mat_inv;
    float* proj_mats;          /* [V,3,4] */
    float* near_fars;          /* [V,2] */
    int64_t* view_ids_out;     /* [V] */
};
typedef struct ucnerf_novel_assemble_params ucnerf_novel_assemble_params;
int ucnerf_novel_assemble(const ucnerf_novel_assemble_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * e1   multi-view depth fusion -- from per-view maps (rgb [N,3,H,W], depth [N,H,W]) to a coloured point cloud: the geometric consistency
 *      filter of the MVSNet / CasMVSNet family and a deterministic compaction.  The reference has no fusion code: the rules below are this
 *      project's own.  Neither entry point synchronises the stream or reads anything back; plain vector loads and stores, NO atomics: the
 *      results are bit-identical from launch to launch.  (Added to ABI v6; nothing above moved.  Structs declared with a tag: mirrored in
 *      _lib.ADDED_STRUCTS.)
 *
 * ucnerf_depth_consistency: ONE launch over all N views; a workgroup of 256 pixels lies inside one reference view r and forms r's and its
 * sources' matrices once, in LDS.  Pixel convention of a1 (raygen_device.h): integer pixel (x, y), d_cam = ((x - K02) / K00, (y - K12) / K11, 1) d.
 * ZERO SKEW IS ASSUMED: of an intrinsic only K00, K02, K11, K12 are read.  Of a 4 x 4 matrix only the first three rows are read.
 *   w2cs == NULL: the RIGID inverse of c2ws, formed per workgroup as d3 forms it: w2c[r][c] = R[c][r],
 *                 w2c[r][3] = -fmaf(R[2][r], t[2], fmaf(R[1][r], t[1], R[0][r] * t[0])).  Not an LU inverse.
 * Arithmetic (float32, -ffp-contract=off: every fmaf is written out, every a / b is an IEEE division, sqrtf is correctly rounded):
 *   M . (a, b, c):     row i = fmaf(M[i][2], c, fmaf(M[i][1], b, M[i][0] * a)) + M[i][3]
 *   back(K, x, y, d):  ((x - K02) / K00 * d, (y - K12) / K11 * d, d)
 *   proj(K, Q):        (K00 * Q.x / Q.z + K02, K11 * Q.y / Q.z + K12): product, then division, then sum
 * The reference pixel (x, y) of view r with depth d is VALID iff d is finite and d > 0 and (conf given) conf is finite and conf >= conf_thresh.
 * For every source slot j in ascending order, s = src_ids[r][j]; s < 0, s == r and s >= N are skipped.  With X = c2w_r . back(K_r, x, y, d):
 *   1. Q = w2c_s . X; not consistent unless 0 < Q.z < inf
 *   2. (u, v) = proj(K_s, Q); not consistent unless 0 <= u <= W - 1 and 0 <= v <= H - 1 (a NaN fails the comparison)
 *   3. x0 = floor(u), a = u - x0, y0 = floor(v), b = v - y0 (exact); the four taps in the order (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
 *      (y0 + 1, x0 + 1) with weights (1 - a)(1 - b), a (1 - b), (1 - a) b, a b.  A tap whose weight is 0 is NOT READ (so u == W - 1 and
 *      v == H - 1 read nothing outside the map); a tap with a non-zero weight whose depth is non-finite or <= 0 makes the source not
 *      consistent; d_s = the taps' fmaf(w, depth, acc) in that order from acc = 0
 *   4. Q' = w2c_r . (c2w_s . back(K_s, u, v, d_s)), d' = Q'.z; not consistent unless 0 < d' < inf; (x', y') = proj(K_r, Q')
 *   5. consistent iff sqrtf(fmaf(ey, ey, ex * ex)) < pix_thresh with ex = x' - x, ey = y' - y, and fabsf(d' - d) / d < rel_thresh
 *      (the square root of the sum of squares stands for hypot: pixel distances neither overflow nor underflow it)
 *   count = the number of consistent sources (uint8; S <= 32);  mask = valid and count >= min_views (one byte, 0 or 1);
 *   fused = (d + d'_1 + d'_2 + ..) / (float)(count + 1), the sum accumulated in source order; 0.0f where the reference pixel is not valid.
 *   A rotation block that is not orthonormal gives what the formulas give.  pix_thresh / rel_thresh NaN: nothing is consistent.
 * UCNERF_EINVAL before any launch: NULL params, a negative N, H, W or S, S > 32, H or W above 2^24 / N H W >= 2^31, a NULL required array
 * (src_ids may be NULL when S == 0; conf and w2cs may be NULL).  N == 0, H == 0 or W == 0: success, nothing launched.
 * Bound: latency / gather (4 taps x S sources per pixel, data-dependent footprint); streams 4 (+4) bytes in and 6 bytes out per pixel. */
struct ucnerf_depth_consistency_params {
    int32_t N, H, W, S;
    int32_t min_views;
    float pix_thresh, rel_thresh, conf_thresh;
    const float* depth;        /* [N,H,W] */
    const float* intrinsics;   /* [N,3,3] */
    const float* c2ws;         /* [N,4,4] */
    const float* w2cs;         /* [N,4,4], or NULL: the rigid inverse of c2ws */
    const int32_t* src_ids;    /* [N,S] */
    const float* conf;         /* [N,H,W], or NULL */
    uint8_t* count;            /* [N,H,W] */
    uint8_t* mask;             /* [N,H,W], 0 or 1 */
    float* fused;              /* [N,H,W] */
};
typedef struct ucnerf_depth_consistency_params ucnerf_depth_consistency_params;
int ucnerf_depth_consistency(const ucnerf_depth_consistency_params* p, void* stream);

/* ucnerf_points_compact: the masked pixels as a point cloud, row k = the k-th pixel with mask != 0 in (view, y, x) order.
 *   points[k] = c2w_n . back(K_n, x, y, fused) (world; the expressions above);  colors[k][c] = (uint8)(clamp(rgb[n][c][y][x], 0, 1) * 255.0f + 0.5f),
 *   product then sum in float32, truncated; a NaN colour gives 0.
 *   total (ONE int64 on the device) = the number of masked pixels, whatever `cap` is; rows k >= cap are not written.
 * One ABI call, three kernels on the stream, a counted fixed-order scan: (1) every workgroup counts the mask bytes of its 1024 pixels into
 * workspace[b]; (2) ONE workgroup turns the counts into exclusive offsets in place, 256 counts a pass with a running carry, and writes total;
 * (3) every workgroup ranks its masked pixels (thread order = pixel order) from its offset and stores the rows.  No atomics.
 * workspace: ucnerf_points_compact_workspace_bytes(N H W) bytes, 4-byte aligned (-1 for a negative count).
 * UCNERF_EINVAL before any launch: NULL params, negative N, H, W or cap, H or W above 2^24 / N H W >= 2^31, a NULL required array (points / colors
 * may be NULL when cap == 0), total not 8-byte aligned.  N H W == 0: total = 0 is written (a memset on the stream), nothing else. */
int64_t ucnerf_points_compact_workspace_bytes(int64_t n_pixels);
struct ucnerf_points_compact_params {
    int32_t N, H, W;
    int32_t reserved;
    int64_t cap;               /* rows of points / colors */
    const float* fused;        /* [N,H,W] */
    const uint8_t* mask;       /* [N,H,W] */
    const float* rgb;          /* [N,3,H,W] */
    const float* intrinsics;   /* [N,3,3] */
    const float* c2ws;         /* [N,4,4] */
    int32_t* workspace;
    float* points;             /* [cap,3] */
    uint8_t* colors;           /* [cap,3] */
    int64_t* total;            /* [1] */
};
typedef struct ucnerf_points_compact_params ucnerf_points_compact_params;
int ucnerf_points_compact(const ucnerf_points_compact_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UCNERF_HIP_H */
