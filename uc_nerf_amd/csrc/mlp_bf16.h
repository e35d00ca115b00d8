// What the builds of mlp_bf16.hip (the split-MLP kernels) and mlp_bf16_host.hip (their launchers, compiled once) share: the kernels' by-value
// arguments, the table a build exports, and the entry points the other translation units call.
#pragma once
#include "common.h"
#include "mlp_layout.h"

namespace ucnerf {

constexpr int SLOT_BYTES = 8192;      // two half-steps: [2][hi0, lo0, hi1, lo1][64 lanes][16 B]
constexpr int KS16_PE_PTS = 4, KS16_PE_DIR = 2, KS16_HID = 8;
[[maybe_unused]] constexpr int FUSED_MAX_V = 8;    // (seven and eight views: with a two-slot weight ring, fused_ring_slots)

struct BGeom {
    int F, kd16, kc16, f_img, slots, feat_stride;
    int const_off_bytes;
};

// Row f1 (FUSED): the feature gather runs inside this kernel.  A lane (sample j, half hh) works out its own operands of the two bias
// nets straight from the channel-last sources -- nothing per sample is read but z, nothing is written but raw:
//   stage-1 volume (hh = 0) / stage-2 volume (hh = 1): all eight channels            -> bd step 0
//   stage-3 volume: channels 4hh .. 4hh+3 of all eight corners                       -> bd step 1, elements 0..3
//   source view 2p + hh of pair p: colour + mask -> bd (elements 4..7 of step 1, then two pairs per step), image features -> bc step p
//   reference projection, confidence: both halves (same values)
// Arithmetic and accumulation order per feature are gather_cl.hip's (bit-identical features); the weight stream is packed in this
// operand order (precision 3, build_pack_index_bf16).
struct FusedGather {
    int S, V, H, W;
    int vol_d[3], vol_h[3], vol_w[3];
    // the channel-last sources, each its own array (ABI v5, ucnerf_cl_sources: read in place or repacked); offsets inside one are 32-bit
    const char* vol[3];      // [D,h,w,8]
    const char* feat;        // [V,H,W,8] image features
    const char* col;         // [V,H,W,col_px / 4] colours
    unsigned col_px;         // bytes per colour pixel: 12 or 16 (bf16: 8)
    const float* conf;
    const float* rays_o;
    const float* rays_d;
    const float* z;
    const float* near_far;
    float near, far;
    float w2c_ref[12], K_ref[9];
    const float* w2cs;
    const float* Ks;
    unsigned div_m, div_sh;    // ExactDiv(S), as two plain fields with the divide written out at its four sites in mlp_bf16.hip: an ExactDiv
                               // member with quot() changes the code of the fused kernels (profiles/geometry_header.md)
    // COORDS instantiation: coordinates GIVEN by the caller (what rendering() of the reference receives from build_rays / build_rays_test,
    // network/renderer.py:215-255) instead of derived from (ray, depth): world points, the three stage copies, the encoded copy -- [M,3] each
    const float* pts_in;
    const float* ndc_in[3];
    const float* ndc_enc;
    int s16;                 // the channel-last arrays hold bf16 (ucnerf_cl_sources.bf16): 16-byte voxels / feature pixels, 8-byte colours
    // RAYGEN instantiation (ABI v4 gen_rays / gen_depths: ucnerf_ray_gen_sample folded into this launch): pixels and jitter draws in, and the rays,
    // depths and view-direction features the launch generates are WRITTEN for the launches behind it (compositing, re-sampling, the fine pass)
    const float* gen_xs;     // [n] pixel columns / rows
    const float* gen_ys;
    const float* gen_noise;  // [n,S] or NULL (perturb == 0)
    float gen_K[4];          // K00, K02, K11, K12 of the target camera
    float gen_R[12];         // its c2w, row-major 3x4
    float gen_Q[12];         // rotation of the view-direction feature (w2c_dir)
    float gen_perturb;
    int gen_lindisp;
    float* gen_rays_d;       // [n,3] out
    float* gen_z;            // [n,S] out
    float* gen_angle;        // [n,3] out
    // TAIL instantiation (passes of at most three rounds of tiles): tiles are dealt in whole rays to blocks (tail_rpb rays = tail_rpb * tail_tpr
    // consecutive tiles per block) and, when its last tile is done, a block composites its rays itself (K7, composite_device.h) and -- coarse
    // pass -- draws the fine depths from them (K8 + K9, sample_pdf_device.h): one launch for K3 .. K9 of the pass
    int tail_rpb, tail_tpr, tail_resample;
    int tail_spb;            // samples per block = tail_rpb * S: the block's tiles start at ITS first sample (round 5: S need not be a multiple of 32,
                             // e.g. the 90 cascade samples of rendering()), so a block's last tile may be partly filled
    // view-direction features made in the block's prologue from the rays' directions (round 5: rendering() hands over rays_d and a rotation that
    // lives on the device -- no ucnerf_dir_feature launch): angle = (d / |d|) @ Q^T written to tail_dir_out [n,3], which the tiles then read
    const float* tail_dir_Q;     // [>=3,4] DEVICE, or NULL: the features are given (ucnerf_mlp_params.dirs)
    float* tail_dir_out;
    ucnerf_composite_params tail_c;
    ucnerf_sample_pdf_params tail_s;
};

// ---- what one build of mlp_bf16.hip exports.  uc_nerf_amd/build.py compiles that file nine times: {bf16 terms, fp16 terms, fp16 terms with range
// detection} x {three-term kernels + packers, plain kernels (the hi*hi term only), the TAIL kernels: compiled beside the main object, not after it}.
// A build holds device code and this table, nothing else; mlp_bf16_host.hip picks the table and does everything that does not depend on the build.
typedef void MlpFwdKernel(ucnerf_mlp_params p, BGeom g, int n_tiles, MlpSaved sv, FusedGather fg, unsigned* gword);
typedef void PackFlatKernel(const float* flat, const int32_t* idx, unsigned short* out16, int64_t n16, float* outc, int nc, int nb16, unsigned* gword);
typedef void PackTabKernel(ParamTable t, const int32_t* idx, unsigned short* out16, int64_t n16, float* outc, int nc, int nb16, unsigned* gword);

// the instantiations of mlp_fwd_bf16_kernel, by the launch conditions that select them (each exists per source-view count)
enum MlpVariant {
    MV_ROWS, MV_TILED,                                    // inference on a feature buffer: row-major / tiled          (three-term and plain builds)
    MV_SAVE_F32, MV_SAVE_P24, MV_SAVE_P24_TILED,          // training forward: fp32 sets, 24-bit sets, ... on tiled features  (three-term builds)
    MV_FUSED, MV_FUSED_COORDS, MV_FUSED_S16, MV_FUSED_RAYGEN,      // gather fused: derived / given coordinates, bf16 sources, rays generated (n_src <= 6)
    MV_TAIL, MV_TAIL_COORDS,                              // ... compositing in the tail: derived / given coordinates         (TAIL builds)
    MV_COUNT
};
constexpr bool mlp_variant_fused(int var) { return var >= MV_FUSED; }      // (the kernel's LDS image then holds the gather's tables: lds_fused)

struct Bf16Build {
    MlpFwdKernel* fwd[MV_COUNT][8];       // [variant][n_src - 1]; NULL: not in this build
    PackFlatKernel* pack_flat;            // three-term builds only (the plain kernels read the same stream)
    PackTabKernel* pack_tab;
    const char* build_flags;
    bool guard;                           // UCNERF_SPLIT_GUARD: the kernels' last argument is the status word they OR into (else the optional `run_if` word)
    // launch geometry of this build's tuning switches (UCNERF_BF16_BW, _WPS, _IDLE_SKIP, _NBUF)
    int waves, blocks_per_cu;             // waves per block; blocks per CU = waves per SIMD * 4 / waves per block
    bool spread;                          // fewer tiles than wave slots: one wave per SIMD on every CU first (see launch_bf16)
    size_t lds, lds_fused[8];             // dynamic LDS of a launch; gather-fused: per n_src
};
enum { BF16_X3, BF16_PLAIN, BF16_TAIL, BF16_OBJECTS };              // the three objects of one operand kind ...
enum { OPERAND_BF16, OPERAND_H16, OPERAND_G16, OPERAND_KINDS };     // ... and the kinds: bf16 terms, fp16 terms, fp16 terms with range detection
#define UCNERF_BF16_BUILD(sfx) const Bf16Build* bf16_build_x3##sfx(); const Bf16Build* bf16_build_plain##sfx(); const Bf16Build* bf16_build_tail##sfx();
UCNERF_BF16_BUILD() UCNERF_BF16_BUILD(_h16) UCNERF_BF16_BUILD(_g16)
#undef UCNERF_BF16_BUILD

// ---- mlp_bf16_host.hip: the entry points of mlp.hip, mlp_bwd.hip and render.hip
int build_pack_index_bf16(const ucnerf_mlp_config* cfg, int32_t* idx);
int64_t bf16_index_count(const ucnerf_mlp_config* cfg);
int64_t bf16_stream_floats(const ucnerf_mlp_config* cfg);
int launch_pack_bf16(const ucnerf_mlp_config* cfg, const float* flat, const int32_t* idx, float* out, hipStream_t st);
int launch_pack_bf16_tab(const ucnerf_mlp_config* cfg, const ParamTable& t, const int32_t* idx, float* out, hipStream_t st);
int launch_mlp_fwd_bf16x3(const ucnerf_mlp_params* p, hipStream_t st);          // the three-term kernels
int launch_mlp_fwd_bf16_plain(const ucnerf_mlp_params* p, hipStream_t st);      // the plain ones
// `save`: the training forward -- the activation sets of MlpSaved are written for ucnerf_mlp_bwd (saved_valid = 1)
int launch_mlp_fwd_bf16x3_save(const ucnerf_mlp_params* p, const MlpSaved* save, hipStream_t st);
// called by render.hip: gather + PE + MLP of one pass in ONE launch (row f1), from the channel-last sources and (ray, depth)
// `tail_c` (optional): the launch also composites the pass's rays (and, with `tail_s`, re-samples from them) -- see FusedGather
int launch_mlp_fwd_bf16x3_gather(const ucnerf_render_params* rp, const float* dirs, float* raw, hipStream_t st,
                                 const ucnerf_composite_params* tail_c, const ucnerf_sample_pdf_params* tail_s, float* tail_dir_out);

}  // namespace ucnerf
