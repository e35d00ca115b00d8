// Host side of the split-MLP kernels (mlp_bf16.hip), compiled once: the layout of the weight stream and its pack index, argument checks, launch
// geometry, the choice among the nine builds of the kernels (Bf16Build, mlp_bf16.h) and the one place each kind of kernel is launched from.
#include "mlp_bf16.h"

#include <vector>

namespace ucnerf {

struct Bf16Layout {
    int v, F, kd16, kc16, slots;      // slots = k16-steps per tile (two half-steps each)
    int64_t const_off_bytes, total_bytes;
};

static bool bf16_layout(int v, Bf16Layout* B) {
    if (v < 1 || v > 8) return false;
    B->v = v; B->F = 24 + 12 * v + 1;
    B->kd16 = (24 + 4 * v + 15) / 16; B->kc16 = (8 * v + 15) / 16;
    B->slots = B->kd16 + KS16_PE_PTS + 4 * KS16_HID + (KS16_PE_PTS + KS16_HID) + B->kc16 + KS16_HID + (KS16_HID + KS16_PE_DIR);
    B->const_off_bytes = (int64_t)B->slots * SLOT_BYTES;
    B->total_bytes = B->const_off_bytes + (int64_t)CONST_FLOATS * 4;
    return true;
}

// ------------------------------------------------------------------------------------------------ host: pack index
// idx16[e] for every bf16 element e of the stream: flat parameter index | (part << 30) (part 0 = hi, 1 = lo), -1 = zero.
// Half-steps appear in the order the kernel consumes them (see the schedule in mlp_fwd_bf16_kernel):
//   bd: step-major (q: pair 0, pair 1) | L0: pair-split | L1..L4: pair-split | L5: pair-split over [h 0..3 | pe 0..3 | h 4..7]
//   bc: step-major | ft: pair-split | vc: pair-split over [h 0..7 | dir 0..1]
int build_pack_index_bf16(const ucnerf_mlp_config* cfg, int32_t* idx) {
    Bf16Layout B;
    MlpLayout L;
    if (!bf16_layout(cfg->n_src, &B) || !mlp_layout(cfg->n_src, &L)) return -1;
    const int v = B.v, W = MLP_W;
    const int64_t n16 = (int64_t)B.slots * (SLOT_BYTES / 2);
    for (int64_t i = 0; i < n16 + CONST_FLOATS; ++i) idx[i] = -1;
    int64_t hidx = 0;
    auto put_half = [&](const std::vector<int64_t>& row_base, const int (&col)[2][8], int pair) {
        for (int t = 0; t < 2; ++t)
            for (int part = 0; part < 2; ++part)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int c = col[lane >> 5][j];
                        const int64_t e = (((hidx * 4 + t * 2 + part) * 64) + lane) * 8 + j;
                        idx[e] = c < 0 ? -1 : (int32_t)((row_base[32 * (2 * pair + t) + (lane & 31)] + c) | ((int64_t)part << 30));
                    }
        ++hidx;
    };
    auto rows = [&](int64_t base, int K) { std::vector<int64_t> rb(128); for (int n = 0; n < 128; ++n) rb[n] = base + (int64_t)n * K; return rb; };
    auto nat = [&](int q, int K, int (&col)[2][8]) { for (int hh = 0; hh < 2; ++hh) for (int j = 0; j < 8; ++j) { int f = 16 * q + 8 * hh + j; col[hh][j] = f < K ? f : -1; } };
    auto hid = [&](int q, int base, int (&col)[2][8]) { for (int hh = 0; hh < 2; ++hh) for (int j = 0; j < 8; ++j) col[hh][j] = base + hid_feature16(q >> 1, q & 1, j, hh); };
    auto pe = [&](int q, int nf, int base, int (&col)[2][8]) {
        for (int hh = 0; hh < 2; ++hh)
            for (int j = 0; j < 8; ++j) {
                int kind, a;
                pe_slot(8 * q + j, hh, nf, &kind, &a);
                const int c = pe_column(kind, a, nf, cfg->pe_layout);
                col[hh][j] = c < 0 ? -1 : base + c;
            }
    };
    // precision 3 (the gather runs inside the kernel, fused_operands below): the two bias nets take their operands in the order the
    // lane halves produce them -- bd: [stage 1 | stage 2], [stage 3 ch 0..3, view 0 | ch 4..7, view 1], then two views per half and
    // step (even views in half 0, odd views in half 1); bc: the image features of view 2q + hh in step q
    const bool fused = cfg->precision == 3;
    auto bd_fused = [&](int q, int (&col)[2][8]) {
        for (int hh = 0; hh < 2; ++hh)
            for (int j = 0; j < 8; ++j) {
                int c = -1;
                if (q == 0) c = 8 * hh + j;
                else if (q == 1 && j < 4) c = 16 + 4 * hh + j;
                else {
                    const int pair = q == 1 ? 0 : 1 + 2 * (q - 2) + (j >> 2), view = 2 * pair + hh;
                    if (view < v) c = 24 + 4 * view + (j & 3);
                }
                col[hh][j] = c;
            }
    };
    auto bc_fused = [&](int q, int (&col)[2][8]) {
        for (int hh = 0; hh < 2; ++hh)
            for (int j = 0; j < 8; ++j) col[hh][j] = 2 * q + hh < v ? 8 * (2 * q + hh) + j : -1;
    };
    int col[2][8];
    {   // bd, step-major
        const auto rb = rows(L.p_bdw, 24 + 4 * v);
        for (int q = 0; q < B.kd16; ++q) { if (fused) bd_fused(q, col); else nat(q, 24 + 4 * v, col); put_half(rb, col, 0); put_half(rb, col, 1); }
    }
    {   // L0
        const auto rb = rows(L.p_lw[0], MLP_PE_PTS);
        for (int p = 0; p < 2; ++p) for (int q = 0; q < KS16_PE_PTS; ++q) { pe(q, 10, 0, col); put_half(rb, col, p); }
    }
    for (int l = 1; l < 5; ++l) {
        const auto rb = rows(L.p_lw[l], W);
        for (int p = 0; p < 2; ++p) for (int q = 0; q < KS16_HID; ++q) { hid(q, 0, col); put_half(rb, col, p); }
    }
    {   // L5 on [pe | h]: k order h 0..3, pe 0..3, h 4..7
        const auto rb = rows(L.p_lw[5], W + MLP_PE_PTS);
        for (int p = 0; p < 2; ++p) {
            for (int q = 0; q < 4; ++q) { hid(q, MLP_PE_PTS, col); put_half(rb, col, p); }
            for (int q = 0; q < KS16_PE_PTS; ++q) { pe(q, 10, 0, col); put_half(rb, col, p); }
            for (int q = 4; q < 8; ++q) { hid(q, MLP_PE_PTS, col); put_half(rb, col, p); }
        }
    }
    {   // bc, step-major
        const auto rb = rows(L.p_bcw, 8 * v);
        for (int q = 0; q < B.kc16; ++q) { if (fused) bc_fused(q, col); else nat(q, 8 * v, col); put_half(rb, col, 0); put_half(rb, col, 1); }
    }
    {   // feature_linear
        const auto rb = rows(L.p_fw, W);
        for (int p = 0; p < 2; ++p) for (int q = 0; q < KS16_HID; ++q) { hid(q, 0, col); put_half(rb, col, p); }
    }
    {   // views_linears | view_confi_linears on [feature | dir encoding]: k order h 0..7, dir 0..1
        std::vector<int64_t> rb(128);
        for (int n = 0; n < 64; ++n) { rb[n] = L.p_vw + (int64_t)n * (W + MLP_PE_DIR); rb[64 + n] = L.p_vcw + (int64_t)n * (W + MLP_PE_DIR); }
        for (int p = 0; p < 2; ++p) {
            for (int q = 0; q < KS16_HID; ++q) { hid(q, 0, col); put_half(rb, col, p); }
            for (int q = 0; q < KS16_PE_DIR; ++q) { pe(q, 4, W, col); put_half(rb, col, p); }
        }
    }
    return hidx == 2 * (int64_t)B.slots ? 0 : -1;
}

int64_t bf16_index_count(const ucnerf_mlp_config* cfg) {
    Bf16Layout B;
    if (!bf16_layout(cfg->n_src, &B)) return -1;
    return (int64_t)B.slots * (SLOT_BYTES / 2) + CONST_FLOATS;
}

int64_t bf16_stream_floats(const ucnerf_mlp_config* cfg) {
    Bf16Layout B;
    if (!bf16_layout(cfg->n_src, &B)) return -1;
    return B.total_bytes / 4;
}

// ------------------------------------------------------------------------------------------------ host: which build, which kernel
// ucnerf_mlp_config.operand (ABI v6) selects the terms: 0 = bf16 (hi and lo have float32's range), 1 = fp16 (11-bit hi and lo terms,
// v_mfma_f32_32x32x16_f16; values beyond 65 504 overflow).  Under a guarded entry point (ucnerf_*_guarded: split_guard().mode == GUARD_DETECT)
// the fp16 terms come from the builds with range detection compiled in.  `operand` has been checked (0 or 1) by the entry point.
static const Bf16Build* pick_build(int object, int operand) {
    static const Bf16Build* (*const BUILDS[BF16_OBJECTS][OPERAND_KINDS])() = {
        {bf16_build_x3, bf16_build_x3_h16, bf16_build_x3_g16},
        {bf16_build_plain, bf16_build_plain_h16, bf16_build_plain_g16},
        {bf16_build_tail, bf16_build_tail_h16, bf16_build_tail_g16}};
    return BUILDS[object][operand == 1 ? (split_guard().mode == GUARD_DETECT ? OPERAND_G16 : OPERAND_H16) : OPERAND_BF16]();
}

// (the labels of ensure_dynamic_lds and check_launch: error texts)
static const struct { const char* kernel; const char* launch; } VARIANT_TEXT[MV_COUNT] = {
    /* MV_ROWS */ {"mlp_fwd (bf16)", "mlp_fwd_bf16"},
    /* MV_TILED */ {"mlp_fwd (bf16)", "mlp_fwd_bf16"},
    /* MV_SAVE_F32 */ {"mlp_fwd_train (bf16x3)", "mlp_fwd_train (bf16x3)"},
    /* MV_SAVE_P24 */ {"mlp_fwd_train (bf16x3, 24-bit sets)", "mlp_fwd_train (bf16x3)"},
    /* MV_SAVE_P24_TILED */ {"mlp_fwd_train (bf16x3, tiled features, 24-bit sets)", "mlp_fwd_train (bf16x3)"},
    /* MV_FUSED */ {"mlp_fwd (bf16x3, gather fused)", "mlp_fwd (bf16x3, gather fused)"},
    /* MV_FUSED_COORDS */ {"mlp_fwd (bf16x3, gather fused, given coordinates)", "mlp_fwd (bf16x3, gather fused)"},
    /* MV_FUSED_S16 */ {"mlp_fwd (bf16x3, gather fused, bf16 sources)", "mlp_fwd (bf16x3, gather fused)"},
    /* MV_FUSED_RAYGEN */ {"mlp_fwd (bf16x3, gather fused, rays generated)", "mlp_fwd (bf16x3, gather fused)"},
    /* MV_TAIL */ {"mlp_fwd (bf16x3, gather fused, compositing in the tail)", "mlp_fwd (bf16x3, gather fused, compositing in the tail)"},
    /* MV_TAIL_COORDS */ {"mlp_fwd (bf16x3, gather fused, given coordinates, compositing in the tail)", "mlp_fwd (bf16x3, gather fused, compositing in the tail)"},
};

// THE launch of mlp_fwd_bf16_kernel: every instantiation has one signature.
// One instantiation per source-view count (1..8: SCARED scripts 6, Hamlyn 3, the reference's opt.py default 4, ...):
// with the section lengths known at compile time no instantiation carries the spills of a runtime-length version.
static int launch_mlp_kernel(const Bf16Build* b, MlpVariant var, int blocks, hipStream_t st, const ucnerf_mlp_params& p, const BGeom& g, int n_tiles,
                             const MlpSaved& sv, const FusedGather& fg) {
    const int v = p.cfg.n_src;
    MlpFwdKernel* const kernel = b->fwd[var][v - 1];
    if (!kernel) return fail(UCNERF_EINVAL, "%s: no kernel for %d source views in this build", VARIANT_TEXT[var].kernel, v);
    const size_t lds = mlp_variant_fused(var) ? b->lds_fused[v - 1] : b->lds;
    if (int rc = ensure_dynamic_lds((const void*)kernel, (int)lds, VARIANT_TEXT[var].kernel)) return rc;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * b->waves), lds, st, p, g, n_tiles, sv, fg, split_guard().word);
    return check_launch(VARIANT_TEXT[var].launch);
}

// `object`: BF16_X3 or BF16_PLAIN; `save` (BF16_X3 only): the training forward; `fuse` (BF16_X3 only): the gather runs inside the kernel
static int launch_bf16(int object, const ucnerf_mlp_params* p, const MlpSaved* save, hipStream_t st, const FusedGather* fuse = nullptr) {
    UCNERF_REQUIRE(p, "mlp_fwd: null params");
    if (p->m == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->dirs && p->wstream && p->raw && (fuse || (p->pts && p->feats)), "mlp_fwd: null pointer");
    UCNERF_REQUIRE((p->cfg.precision == 3) == (fuse != nullptr), "mlp_fwd: a weight stream packed with precision 3 serves the render pass with the gather "
                   "fused into the MLP kernel and nothing else (ucnerf_render_fused_fwd)");
    UCNERF_REQUIRE(!p->encoded && !p->pts_stride && !p->dirs_stride, "mlp_fwd (bf16x3): encoded / strided inputs are only available in f32 precision");
    UCNERF_REQUIRE(p->dirs_per_sample || p->S > 0, "mlp_fwd: S must be > 0 when dirs are per ray");
    UCNERF_REQUIRE(((uintptr_t)p->wstream & 15) == 0 && ((uintptr_t)p->raw & 15) == 0, "mlp_fwd: wstream/raw must be 16-byte aligned");
    Bf16Layout B;
    UCNERF_REQUIRE(bf16_layout(p->cfg.n_src, &B), "mlp_fwd: n_src %d outside 1..8", p->cfg.n_src);
    // the guarded split: the build's kernels take the status word (Bf16Build::guard) or the optional condition word of a replay
    const Bf16Build* const b = pick_build(object, p->cfg.operand);
    UCNERF_REQUIRE((split_guard().mode == GUARD_DETECT) == b->guard, "mlp_fwd: range detection is compiled into the guarded fp16-term "
                   "kernels only (ucnerf_*_guarded with cfg.operand 1)");
    UCNERF_REQUIRE(split_guard().mode == GUARD_NONE || (split_guard().word && !save), "mlp_fwd: a guarded or conditional launch needs its status word "
                   "and serves the inference forward");
    const int n_tiles = cdiv(p->m, 32);
    const int cus = device_cus();
    if (cus <= 0) return fail(UCNERF_EHIP, "mlp_fwd: no device");
    int blocks = cdiv(n_tiles, b->waves);
    const int cap = p->max_blocks > 0 ? p->max_blocks : b->blocks_per_cu * cus;
    // fewer tiles than wave slots: rather every CU with one wave per SIMD than half the CUs with two (tiles are dealt wave-major, see the kernel)
    if (b->spread && blocks < cap) { const int spread = cdiv(n_tiles, 4); blocks = spread < cap ? spread : cap; }
    if (blocks > cap) blocks = cap;
    BGeom g;
    g.F = B.F; g.kd16 = B.kd16; g.kc16 = B.kc16; g.f_img = 24 + 4 * B.v; g.slots = B.slots;
    g.feat_stride = p->feat_stride ? p->feat_stride : B.F;
    g.const_off_bytes = (int)B.const_off_bytes;
    const bool tiled = p->feats_tiled != 0;
    MlpSaved sv;
    memset(&sv, 0, sizeof(sv));
    FusedGather fg;
    memset(&fg, 0, sizeof(fg));
    if (fuse) {
        UCNERF_REQUIRE(!save && B.v <= FUSED_MAX_V, "mlp_fwd (gather fused): inference forward, n_src <= %d", FUSED_MAX_V);
        fg = *fuse;
        UCNERF_REQUIRE(!(fg.s16 && fg.pts_in), "mlp_fwd (gather fused): bf16 channel-last sources are served on derived coordinates only (given coordinates: fp32 copies, "
                       "or the two-kernel pass)");
        if (fg.tail_rpb > 0) {      // the launch composites its rays itself (small passes, render.hip): whole rays per block, which it also generates when asked to
            UCNERF_REQUIRE(!fg.s16 && !(fg.gen_xs && (fg.near_far || fg.pts_in)) && p->max_blocks <= 0, "mlp_fwd (gather fused): compositing in the tail goes with fp32 sources (and generated rays with derived coordinates)");
            // the TAIL instantiations (their own objects); coordinates given: what rendering() hands over (network/renderer.py:215-255)
            return launch_mlp_kernel(pick_build(BF16_TAIL, p->cfg.operand), fg.pts_in ? MV_TAIL_COORDS : MV_TAIL, cdiv(fg.tail_c.n, fg.tail_rpb), st, *p, g, n_tiles, sv, fg);
        }
        // rays generated inside the launch (ABI v4 gen_rays / gen_depths): one to six source views (seven and eight spill 24 bytes per lane)
        UCNERF_REQUIRE(!fg.gen_xs || (!fg.s16 && !fg.pts_in && !fg.near_far && B.v <= 6), "mlp_fwd (gather fused): generated rays go with fp32 source copies, derived "
                       "coordinates, the scene's depth range and at most six source views");
        return launch_mlp_kernel(b, fg.pts_in ? MV_FUSED_COORDS : fg.s16 ? MV_FUSED_S16 : fg.gen_xs ? MV_FUSED_RAYGEN : MV_FUSED, blocks, st, *p, g, n_tiles, sv, fg);
    }
    if (save) {
        sv = *save;
        UCNERF_REQUIRE(sv.p24 || !tiled, "mlp_fwd_train (bf16x3): fp32 activation sets serve the layer-by-layer backward, which reads row-major features");
        return launch_mlp_kernel(b, tiled ? MV_SAVE_P24_TILED : sv.p24 ? MV_SAVE_P24 : MV_SAVE_F32, blocks, st, *p, g, n_tiles, sv, fg);
    }
    return launch_mlp_kernel(b, tiled ? MV_TILED : MV_ROWS, blocks, st, *p, g, n_tiles, sv, fg);
}

const char* build_flags_mlp_bf16x3() { return bf16_build_x3()->build_flags; }
const char* build_flags_mlp_bf16_plain() { return bf16_build_plain()->build_flags; }

int launch_mlp_fwd_bf16x3(const ucnerf_mlp_params* p, hipStream_t st) {
    UCNERF_REQUIRE(p, "mlp_fwd: null params");
    UCNERF_REQUIRE(p->cfg.operand == 0 || p->cfg.operand == 1, "mlp_fwd: cfg.operand %d (0 = bf16 terms, 1 = fp16 terms)", p->cfg.operand);
    return launch_bf16(BF16_X3, p, nullptr, st);
}
int launch_mlp_fwd_bf16_plain(const ucnerf_mlp_params* p, hipStream_t st) {
    UCNERF_REQUIRE(p, "mlp_fwd: null params");
    UCNERF_REQUIRE(p->cfg.operand == 0 || p->cfg.operand == 1, "mlp_fwd: cfg.operand %d (0 = bf16 terms, 1 = fp16 terms)", p->cfg.operand);
    return launch_bf16(BF16_PLAIN, p, nullptr, st);
}
int launch_mlp_fwd_bf16x3_save(const ucnerf_mlp_params* p, const MlpSaved* save, hipStream_t st) {
    UCNERF_REQUIRE(p && p->cfg.operand == 0, "mlp_fwd_train: the training forward keeps its activations for a backward that splits them into bf16 terms "
                   "(cfg.operand 0); fp16 terms serve the inference forward");
    return launch_bf16(BF16_X3, p, save, st);
}

int check_cl_sources(const ucnerf_render_params* p, const char* who);      // gather_cl.hip
int launch_mlp_fwd_bf16x3_gather(const ucnerf_render_params* rp, const float* dirs, float* raw, hipStream_t st,
                                 const ucnerf_composite_params* tail_c, const ucnerf_sample_pdf_params* tail_s, float* tail_dir_out) {
    UCNERF_REQUIRE(rp->cfg.operand == 0 || rp->cfg.operand == 1, "render (gather fused): cfg.operand %d (0 = bf16 terms, 1 = fp16 terms)", rp->cfg.operand);
    const long long M = (long long)rp->n * rp->S;
    UCNERF_REQUIRE(M < (1ll << 31), "render (gather fused): %lld samples in one pass (limit 2^31 - 1)", M);
    if (int rc = check_cl_sources(rp, "render (gather fused)")) return rc;
    ucnerf_mlp_params m;
    memset(&m, 0, sizeof(m));
    m.cfg = rp->cfg; m.m = (int)M; m.S = rp->S; m.max_blocks = rp->max_blocks; m.dirs = dirs; m.wstream = rp->wstream; m.raw = raw;
    FusedGather f;
    memset(&f, 0, sizeof(f));
    f.S = rp->S; f.V = rp->cfg.n_src; f.H = rp->H; f.W = rp->W;
    for (int k = 0; k < 3; ++k) {
        f.vol_d[k] = rp->vol_d[k]; f.vol_h[k] = rp->vol_h[k]; f.vol_w[k] = rp->vol_w[k];
        f.vol[k] = reinterpret_cast<const char*>(rp->cl.vol[k]);
    }
    f.s16 = rp->cl.bf16 ? 1 : 0;
    f.feat = reinterpret_cast<const char*>(rp->cl.img_feat); f.col = reinterpret_cast<const char*>(rp->cl.imgs);
    f.col_px = rp->cl.bf16 ? 8u : 4u * (unsigned)rp->cl.rgb_stride;
    f.conf = rp->conf; f.rays_o = rp->rays_o; f.rays_d = rp->rays_d; f.z = rp->z; f.near_far = rp->near_far;
    f.near = rp->near; f.far = rp->far;
    memcpy(f.w2c_ref, rp->w2c_ref, sizeof(f.w2c_ref));
    memcpy(f.K_ref, rp->K_ref, sizeof(f.K_ref));
    f.w2cs = rp->w2cs; f.Ks = rp->intrinsics;
    f.pts_in = rp->pts_in; f.ndc_in[0] = rp->ndc1_in; f.ndc_in[1] = rp->ndc2_in; f.ndc_in[2] = rp->ndc3_in; f.ndc_enc = rp->ndc_in;
    if (rp->gen_rays) {          // ABI v4: the launch generates rays and stratified depths itself (validated by ucnerf_render_fused_fwd)
        const ucnerf_ray_gen_params* gr = rp->gen_rays;
        const ucnerf_sample_stratified_params* gs = rp->gen_depths;
        f.gen_xs = gr->xs; f.gen_ys = gr->ys; f.gen_noise = gs->perturb > 0.f ? gs->noise : nullptr;
        f.gen_K[0] = gr->K[0]; f.gen_K[1] = gr->K[2]; f.gen_K[2] = gr->K[4]; f.gen_K[3] = gr->K[5];
        memcpy(f.gen_R, gr->c2w, sizeof(f.gen_R));
        memcpy(f.gen_Q, gr->w2c_dir, sizeof(f.gen_Q));
        f.gen_perturb = gs->perturb; f.gen_lindisp = gs->lindisp;
        f.gen_rays_d = gr->rays_d; f.gen_z = gs->z; f.gen_angle = gr->angle;      // (`dirs` is not read: every lane derives its ray's feature itself)
    }
    const ExactDiv by_S((unsigned)rp->S);
    f.div_m = by_S.m; f.div_sh = by_S.sh;
    if (tail_c) {
        const int cus = device_cus();
        if (cus <= 0) return fail(UCNERF_EHIP, "mlp_fwd: no device");
        f.tail_rpb = cdiv(rp->n, cus); f.tail_tpr = cdiv(rp->S, 32); f.tail_resample = tail_s ? 1 : 0;
        f.tail_spb = f.tail_rpb * rp->S;
        if (tail_dir_out) { f.tail_dir_Q = rp->w2c_dir_dev; f.tail_dir_out = tail_dir_out; }      // (render.hip: the features are made in the blocks' prologues)
        f.tail_c = *tail_c;
        if (tail_s) f.tail_s = *tail_s;
    }
    return launch_bf16(BF16_X3, &m, nullptr, st, &f);
}

// ------------------------------------------------------------------------------------------------ host: packing the stream
// ONE launch for the whole stream (round 5: the evaluation loop re-packs in every rendering() call, the drop-in in every no_grad call -- two launches
// were 5 us of GPU time and two launches' host time per 1024-pixel chunk): blocks [0, nb16) convert the 16-bit half-steps, the rest copy the fp32
// constants.  `src`: the flat parameter vector (pack_all_flat_kernel) or the table of a module's tensors (pack_all_tab_kernel).
template <class Kernel, class Src>
static int launch_pack(Kernel* Bf16Build::*kernel, const char* who, const char* what, const ucnerf_mlp_config* cfg, const Src& src, const int32_t* idx,
                       float* out, hipStream_t st) {
    UCNERF_REQUIRE(cfg->operand == 0 || cfg->operand == 1, "%s: cfg.operand %d (0 = bf16 terms, 1 = fp16 terms)", who, cfg->operand);
    const Bf16Build* const b = pick_build(BF16_X3, cfg->operand);
    Bf16Layout B;
    UCNERF_REQUIRE(bf16_layout(cfg->n_src, &B), "mlp_pack: n_src %d outside 1..8", cfg->n_src);
    UCNERF_REQUIRE((split_guard().mode == GUARD_DETECT) == b->guard && (split_guard().mode == GUARD_NONE || split_guard().word),
                   "mlp_pack: range detection is compiled into the guarded fp16 packers only (ucnerf_mlp_pack*_guarded with cfg.operand 1), with a status word");
    const int64_t n16 = (int64_t)B.slots * (SLOT_BYTES / 2);
    const int nb16 = cdiv(n16, 256), nbc = cdiv(CONST_FLOATS, 256);
    hipLaunchKernelGGL(b->*kernel, dim3(nb16 + nbc), dim3(256), 0, st, src, idx, reinterpret_cast<unsigned short*>(out), n16,
                       reinterpret_cast<float*>(reinterpret_cast<char*>(out) + B.const_off_bytes), CONST_FLOATS, nb16, split_guard().word);
    return check_launch(what);
}

int launch_pack_bf16(const ucnerf_mlp_config* cfg, const float* flat, const int32_t* idx, float* out, hipStream_t st) {
    return launch_pack(&Bf16Build::pack_flat, "mlp_pack", "mlp_pack (bf16x3)", cfg, flat, idx, out, st);
}

int launch_pack_bf16_tab(const ucnerf_mlp_config* cfg, const ParamTable& t, const int32_t* idx, float* out, hipStream_t st) {
    return launch_pack(&Bf16Build::pack_tab, "mlp_pack_tensors", "mlp_pack_tensors (bf16x3)", cfg, t, idx, out, st);
}

}  // namespace ucnerf
