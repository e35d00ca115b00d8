// f2, the link between two cascade stages: the previous stage's depth map -> the next stage's per-pixel hypothesis volume
// depth_values [D, h + 2 pad, w + 2 pad]  (network/mvs_models.py:536-573 get_*depth_range_samples, :693-762 CascadeMVSNet.forward).
// The reference up-samples the depth to full resolution, builds a FULL-resolution [D,H,W] volume there (15.7 MB at stage 1 of a 256 x 320
// image) and interpolates it back down; here one thread owns one output column (y, x): it rebuilds the at most 2 x 2 full-resolution
// pixels its down-sampling taps touch -- each a 2 x 2 bilinear sample of the depth map, which stays in L2 -- and writes its D values.
// Nothing of full resolution is stored: the traffic is the output (<= 2.6 MB per stage), so what the launch costs is mostly its latency.
// No LDS, no matrix cores; a wave's store is 256 contiguous bytes of one depth plane.
//
// Backward (ucnerf_depth_hypotheses_bwd, map mode, into cur_depth): THREE launches through a scratch buffer of 2 h w + H W floats, each a gather --
//   A  one thread per inner output column: G0 = sum_d g_d and G1 = sum_d g_d * d / (D - 1), the pad border's columns folded onto the edge column
//      they repeat;
//   B  one thread per full-resolution pixel: the forward's own c and the two clamp decisions, then the sum over the output columns whose
//      down-sampling taps include the pixel;
//   C  one thread per cur_depth pixel: the sum over the full-resolution pixels whose up-sampling taps include it.
// The other option, one launch with a thread per cur_depth pixel, rebuilds every full-resolution pixel's column sums once per tap of every
// pixel that touches it (stage 2: ~12 x 12 full-resolution pixels x ~3 x 3 columns x 32 depths per thread on 5120 threads, three wave-fulls of
// work that cannot spread); the phases read g_out exactly once, spread over as many threads as there are columns, and the scratch (<= 1 MB at
// 256 x 320) stays in L2.  All three are latency-bound.  No float atomics: along an axis the destinations whose taps include source i are
// contiguous (src is monotone in dst), so a thread walks a conservative candidate range and lets dh_tap decide membership; the order of every
// sum is fixed and two launches give the same bits.
#include "common.h"

namespace ucnerf {

constexpr int DH_BLOCK = 256;     // threads = consecutive pixels of the (padded) output plane: stores coalesce whatever the row width
constexpr int DH_DEPTHS = 8;      // depths per thread (blockIdx.y picks the chunk): stage 1 has only 5120 columns but 48 depths

// torch's align_corners=False rule for one axis (area_pixel_compute_source_index + the lambda of upsample_bilinear2d):
// src = max(scale * (dst + 0.5) - 0.5, 0) with scale = n_in / n_out in float; taps floor(src) and the next one, clamped to the edge
struct DhTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ DhTap dh_tap(int dst, int n_in, int n_out) {
    const float scale = (float)n_in / (float)n_out;
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    DhTap t;
    t.i0 = min((int)src, n_in - 1);                  // (src >= 0: truncation is floor; the clamp only guards the address)
    t.i1 = min(t.i0 + 1, n_in - 1);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

__global__ void __launch_bounds__(DH_BLOCK) depth_hypotheses_kernel(ucnerf_depth_hypotheses_params p) {
    const int Hp = p.h + 2 * p.pad, Wp = p.w + 2 * p.pad;
    const unsigned plane = (unsigned)Hp * (unsigned)Wp;                     // (host checks plane < 2^31)
    const unsigned t = blockIdx.x * DH_BLOCK + threadIdx.x;
    if (t >= plane) return;
    const int d_begin = blockIdx.y * DH_DEPTHS, d_end = min(d_begin + DH_DEPTHS, p.D);
    float* out = p.out + (size_t)d_begin * plane + t;
    const float steps = (float)(p.D - 1);

    if (p.row) {                                                             // stage 1: one band for every pixel (mvs_models.py:559-567)
        const float mn = p.row[0], mx = p.row[p.D_in - 1];
        const float interval = (mx - mn) / steps;
        for (int d = d_begin; d < d_end; ++d, out += plane) *out = mn + (float)d * interval;
        return;
    }

    const float near = p.near_far[0], far = p.near_far[1];
    const float half = ((float)p.D / 2.f) * (p.k * (p.interval ? p.interval[0] : far - near));      // ndepth / 2 * depth_inteval_pixel (:540-541)
    // the pad border replicates the edge column (DepthNet's F.pad(..., "replicate"), :598)
    const int y = min(max((int)(t / (unsigned)Wp) - p.pad, 0), p.h - 1);
    const int x = min(max((int)(t % (unsigned)Wp) - p.pad, 0), p.w - 1);
    const DhTap ty = dh_tap(y, p.H, p.h), tx = dh_tap(x, p.W, p.w);          // down-sampling taps in the full-resolution grid
    const int Y[2] = {ty.i0, ty.i1}, X[2] = {tx.i0, tx.i1};
    DhTap uy[2], ux[2];                                                      // up-sampling taps of those rows / columns in the depth map
#pragma unroll
    for (int a = 0; a < 2; ++a) { uy[a] = dh_tap(Y[a], p.h0, p.H); ux[a] = dh_tap(X[a], p.w0, p.W); }
    float mn[2][2], interval[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float* r0 = p.cur_depth + (size_t)uy[a].i0 * p.w0;
            const float* r1 = p.cur_depth + (size_t)uy[a].i1 * p.w0;
            const float c = uy[a].l0 * (ux[b].l0 * r0[ux[b].i0] + ux[b].l1 * r0[ux[b].i1])
                          + uy[a].l1 * (ux[b].l0 * r1[ux[b].i0] + ux[b].l1 * r1[ux[b].i1]);
            // :540-541, torch.clamp: a NaN c stays NaN (fmaxf / fminf would hand back near and far: the full band where the depth is unknown)
            const float below = c - half, above = c + half;
            const float lo = below < near ? near : below, hi = above > far ? far : above;
            mn[a][b] = lo;
            interval[a][b] = (hi - lo) / steps;                                      // :544
        }
    auto plane_value = [&](int d) {
        const float fd = (float)d;
        const float s00 = mn[0][0] + fd * interval[0][0], s01 = mn[0][1] + fd * interval[0][1];      // :546-549
        const float s10 = mn[1][0] + fd * interval[1][0], s11 = mn[1][1] + fd * interval[1][1];
        return ty.l0 * (tx.l0 * s00 + tx.l1 * s01) + ty.l1 * (tx.l0 * s10 + tx.l1 * s11);
    };
    // the reference's trilinear interpolation keeps the depth axis' size: its taps there are d and min(d + 1, D - 1) with the weights 1 and 0.
    // The zero-weight tap changes no finite value and turns an infinite next plane into NaN (0 * inf), as torch does
    float v = plane_value(d_begin);
    for (int d = d_begin; d < d_end; ++d, out += plane) {
        const float next = plane_value(min(d + 1, p.D - 1));
        *out = v + 0.f * next;
        v = next;
    }
}

// ---- backward.  Candidate destinations of one axis (n_in -> n_out) whose taps may include source i: src(dst) in (i - 1, i + 1), i.e.
// dst in ((i - 0.5) n_out / n_in - 0.5, (i + 1.5) n_out / n_in - 0.5), widened by one on each side against the rounding of this estimate
// (the clamps of dh_tap only move src INTO [0, n_in - 1], never across an integer outside this range); dh_weight then decides exactly.
__device__ __forceinline__ void dh_candidates(int i, int n_in, int n_out, int& lo, int& hi) {
    const float inv = (float)n_out / (float)n_in;
    lo = max((int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1, 0);
    hi = min((int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1, n_out - 1);
}
// the weight destination dst gives source i (both taps count where they are the same pixel); `member` false: i is not among its taps
__device__ __forceinline__ float dh_weight(int dst, int i, int n_in, int n_out, bool& member) {
    const DhTap t = dh_tap(dst, n_in, n_out);
    member = t.i0 == i || t.i1 == i;
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

// A: column sums.  scratch[0 .. hw) = G0, scratch[hw .. 2 hw) = G1 of inner column (y, x); border cells fold onto the edge column they copy
__global__ void __launch_bounds__(DH_BLOCK) depth_hypotheses_bwd_columns_kernel(ucnerf_depth_hypotheses_bwd_params bp) {
    const ucnerf_depth_hypotheses_params& p = bp.fwd;
    const unsigned hw = (unsigned)p.h * (unsigned)p.w;
    const unsigned t = blockIdx.x * DH_BLOCK + threadIdx.x;
    if (t >= hw) return;
    const int y = (int)(t / (unsigned)p.w), x = (int)(t % (unsigned)p.w);
    const int Wp = p.w + 2 * p.pad;
    const size_t plane = (size_t)(p.h + 2 * p.pad) * (size_t)Wp;
    // padded rows / columns that show this column's value: its own, plus the border beyond it when it lies on the edge
    const int r0 = y == 0 ? 0 : y + p.pad, r1 = y == p.h - 1 ? y + 2 * p.pad : y + p.pad;
    const int c0 = x == 0 ? 0 : x + p.pad, c1 = x == p.w - 1 ? x + 2 * p.pad : x + p.pad;
    const float steps = (float)(p.D - 1);
    float G0 = 0.f, S1 = 0.f;
    for (int d = 0; d < p.D; ++d) {
        const float* g = bp.g_out + (size_t)d * plane;
        float s = 0.f;
        for (int r = r0; r <= r1; ++r)
            for (int c = c0; c <= c1; ++c) s += g[(size_t)r * Wp + c];
        G0 += s;
        S1 += s * (float)d;
    }
    bp.scratch[t] = G0;
    bp.scratch[hw + t] = S1 / steps;
}

// B: full-resolution pixel (Y, X).  scratch[2 hw + Y W + X] = sum over the columns (y, x) whose taps include it of
// ly * lx * ((G0 - G1) * pass_lo + G1 * pass_hi); c is formed by the forward's expression, so the two decisions are the forward's
__global__ void __launch_bounds__(DH_BLOCK) depth_hypotheses_bwd_full_kernel(ucnerf_depth_hypotheses_bwd_params bp) {
    const ucnerf_depth_hypotheses_params& p = bp.fwd;
    const unsigned HW = (unsigned)p.H * (unsigned)p.W, hw = (unsigned)p.h * (unsigned)p.w;
    const unsigned t = blockIdx.x * DH_BLOCK + threadIdx.x;
    if (t >= HW) return;
    const int Y = (int)(t / (unsigned)p.W), X = (int)(t % (unsigned)p.W);
    const float near = p.near_far[0], far = p.near_far[1];
    const float half = ((float)p.D / 2.f) * (p.k * (p.interval ? p.interval[0] : far - near));
    const DhTap uy = dh_tap(Y, p.h0, p.H), ux = dh_tap(X, p.w0, p.W);
    const float* r0 = p.cur_depth + (size_t)uy.i0 * p.w0;
    const float* r1 = p.cur_depth + (size_t)uy.i1 * p.w0;
    const float c = uy.l0 * (ux.l0 * r0[ux.i0] + ux.l1 * r0[ux.i1]) + uy.l1 * (ux.l0 * r1[ux.i0] + ux.l1 * r1[ux.i1]);
    const float pass_lo = c - half >= near ? 1.f : 0.f, pass_hi = c + half <= far ? 1.f : 0.f;      // ties pass (torch's clamp backward)
    int ylo, yhi, xlo, xhi;
    dh_candidates(Y, p.H, p.h, ylo, yhi);
    dh_candidates(X, p.W, p.w, xlo, xhi);
    const float* G0 = bp.scratch;
    const float* G1 = bp.scratch + hw;
    float sum = 0.f;
    for (int y = ylo; y <= yhi; ++y) {
        bool my;
        const float wy = dh_weight(y, Y, p.H, p.h, my);
        if (!my) continue;
        for (int x = xlo; x <= xhi; ++x) {
            bool mx;
            const float wx = dh_weight(x, X, p.W, p.w, mx);
            if (!mx) continue;
            const unsigned col = (unsigned)y * (unsigned)p.w + (unsigned)x;
            const float g0 = G0[col], g1 = G1[col];
            sum += (wy * wx) * ((g0 - g1) * pass_lo + g1 * pass_hi);
        }
    }
    bp.scratch[2 * (size_t)hw + t] = sum;
}

// C: cur_depth pixel (i, j) = sum over the full-resolution pixels whose up-sampling taps include it, with the up-sampling weights
__global__ void __launch_bounds__(DH_BLOCK) depth_hypotheses_bwd_cur_kernel(ucnerf_depth_hypotheses_bwd_params bp) {
    const ucnerf_depth_hypotheses_params& p = bp.fwd;
    const unsigned n0 = (unsigned)p.h0 * (unsigned)p.w0;
    const unsigned t = blockIdx.x * DH_BLOCK + threadIdx.x;
    if (t >= n0) return;
    const int i = (int)(t / (unsigned)p.w0), j = (int)(t % (unsigned)p.w0);
    const float* full = bp.scratch + 2 * (size_t)p.h * (size_t)p.w;
    int Ylo, Yhi, Xlo, Xhi;
    dh_candidates(i, p.h0, p.H, Ylo, Yhi);
    dh_candidates(j, p.w0, p.W, Xlo, Xhi);
    float sum = 0.f;
    for (int Y = Ylo; Y <= Yhi; ++Y) {
        bool my;
        const float wy = dh_weight(Y, i, p.h0, p.H, my);
        if (!my) continue;
        for (int X = Xlo; X <= Xhi; ++X) {
            bool mx;
            const float wx = dh_weight(X, j, p.w0, p.W, mx);
            if (!mx) continue;
            sum += (wy * wx) * full[(size_t)Y * p.W + X];
        }
    }
    bp.g_cur_depth[t] = sum;
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_depth_hypotheses(const ucnerf_depth_hypotheses_params* p, void* stream) {
    UCNERF_REQUIRE(p, "depth_hypotheses: null params");
    UCNERF_REQUIRE(p->D >= 0 && p->h >= 0 && p->w >= 0 && p->pad >= 0 && p->H >= 0 && p->W >= 0 && p->h0 >= 0 && p->w0 >= 0 && p->D_in >= 0,
                   "depth_hypotheses: negative size D=%d h=%d w=%d pad=%d H=%d W=%d h0=%d w0=%d D_in=%d", p->D, p->h, p->w, p->pad, p->H, p->W, p->h0, p->w0, p->D_in);
    UCNERF_REQUIRE(p->D >= 2 && p->D <= 65535 * DH_DEPTHS, "depth_hypotheses: D = %d outside 2..%d (the interval is (max - min) / (D - 1))", p->D, 65535 * DH_DEPTHS);
    const long long plane = (long long)(p->h + 2ll * p->pad) * (p->w + 2ll * p->pad);
    if (plane == 0) return UCNERF_OK;                                        // an empty volume: success, nothing launched, no pointer read
    UCNERF_REQUIRE(p->out, "depth_hypotheses: null output");
    UCNERF_REQUIRE((p->cur_depth != nullptr) != (p->row != nullptr), "depth_hypotheses: exactly one of cur_depth (map mode) and row (row mode) must be given");
    if (p->cur_depth) {
        UCNERF_REQUIRE(p->h <= p->H && p->w <= p->W && p->h0 <= p->H && p->w0 <= p->W,
                       "depth_hypotheses: the intermediate resolution %d x %d must cover the output %d x %d and the depth map %d x %d", p->H, p->W, p->h, p->w, p->h0, p->w0);
    }
    UCNERF_REQUIRE(plane < (1ll << 31), "depth_hypotheses: output plane of %lld pixels (32-bit pixel index)", plane);
    if (p->cur_depth) {
        UCNERF_REQUIRE(p->h >= 1 && p->w >= 1 && p->h0 >= 1 && p->w0 >= 1, "depth_hypotheses: an empty map cannot fill a non-empty output (h=%d w=%d h0=%d w0=%d)", p->h, p->w, p->h0, p->w0);
        UCNERF_REQUIRE(p->near_far, "depth_hypotheses: null near_far");
    } else {
        UCNERF_REQUIRE(p->D_in >= 1, "depth_hypotheses: empty hypothesis row");
    }
    hipLaunchKernelGGL(depth_hypotheses_kernel, dim3(cdiv(plane, DH_BLOCK), cdiv(p->D, DH_DEPTHS)), dim3(DH_BLOCK), 0, (hipStream_t)stream, *p);
    return check_launch("depth_hypotheses");
}

// the size checks the backward shares with the forward's map mode; 0 when they hold
static int dh_bwd_sizes(const ucnerf_depth_hypotheses_params* p, const char* who) {
    UCNERF_REQUIRE(p->D >= 0 && p->h >= 0 && p->w >= 0 && p->pad >= 0 && p->H >= 0 && p->W >= 0 && p->h0 >= 0 && p->w0 >= 0 && p->D_in >= 0,
                   "%s: negative size D=%d h=%d w=%d pad=%d H=%d W=%d h0=%d w0=%d D_in=%d", who, p->D, p->h, p->w, p->pad, p->H, p->W, p->h0, p->w0, p->D_in);
    UCNERF_REQUIRE(p->D >= 2 && p->D <= 65535 * DH_DEPTHS, "%s: D = %d outside 2..%d (the interval is (max - min) / (D - 1))", who, p->D, 65535 * DH_DEPTHS);
    UCNERF_REQUIRE(p->h <= p->H && p->w <= p->W && p->h0 <= p->H && p->w0 <= p->W,
                   "%s: the intermediate resolution %d x %d must cover the output %d x %d and the depth map %d x %d", who, p->H, p->W, p->h, p->w, p->h0, p->w0);
    const long long plane = (long long)(p->h + 2ll * p->pad) * (p->w + 2ll * p->pad);
    UCNERF_REQUIRE(plane < (1ll << 31), "%s: output plane of %lld pixels (32-bit pixel index)", who, plane);
    UCNERF_REQUIRE((long long)p->H * p->W < (1ll << 31), "%s: intermediate resolution of %lld pixels (32-bit pixel index)", who, (long long)p->H * p->W);
    return UCNERF_OK;
}

int64_t ucnerf_depth_hypotheses_bwd_scratch_floats(const ucnerf_depth_hypotheses_params* p) {
    if (!p || dh_bwd_sizes(p, "depth_hypotheses_bwd_scratch_floats") != UCNERF_OK) return -1;
    return 2ll * p->h * p->w + (long long)p->H * p->W;
}

int ucnerf_depth_hypotheses_bwd(const ucnerf_depth_hypotheses_bwd_params* bp, void* stream) {
    UCNERF_REQUIRE(bp, "depth_hypotheses_bwd: null params");
    const ucnerf_depth_hypotheses_params* p = &bp->fwd;
    if (const int rc = dh_bwd_sizes(p, "depth_hypotheses_bwd")) return rc;
    const long long n0 = (long long)p->h0 * p->w0, hw = (long long)p->h * p->w, HW = (long long)p->H * p->W;
    if (n0 == 0) return UCNERF_OK;                                           // an empty gradient: success, nothing launched, no pointer read
    UCNERF_REQUIRE(bp->g_cur_depth, "depth_hypotheses_bwd: null g_cur_depth");
    UCNERF_REQUIRE(p->cur_depth && !p->row, "depth_hypotheses_bwd: map mode only (cur_depth given, row NULL): row mode has no tensor to differentiate");
    UCNERF_REQUIRE(p->near_far, "depth_hypotheses_bwd: null near_far");
    if ((long long)(p->h + 2ll * p->pad) * (p->w + 2ll * p->pad) == 0) {    // an empty g_out: nothing depends on cur_depth
        const hipError_t e = hipMemsetAsync(bp->g_cur_depth, 0, (size_t)n0 * sizeof(float), (hipStream_t)stream);
        return e == hipSuccess ? UCNERF_OK : fail(UCNERF_EHIP, "depth_hypotheses_bwd: %s", hipGetErrorString(e));
    }
    UCNERF_REQUIRE(p->h >= 1 && p->w >= 1, "depth_hypotheses_bwd: an empty map cannot fill a non-empty output (h=%d w=%d)", p->h, p->w);
    UCNERF_REQUIRE(bp->g_out && bp->scratch, "depth_hypotheses_bwd: null g_out / scratch");
    hipLaunchKernelGGL(depth_hypotheses_bwd_columns_kernel, dim3(cdiv(hw, DH_BLOCK)), dim3(DH_BLOCK), 0, (hipStream_t)stream, *bp);
    hipLaunchKernelGGL(depth_hypotheses_bwd_full_kernel, dim3(cdiv(HW, DH_BLOCK)), dim3(DH_BLOCK), 0, (hipStream_t)stream, *bp);
    hipLaunchKernelGGL(depth_hypotheses_bwd_cur_kernel, dim3(cdiv(n0, DH_BLOCK)), dim3(DH_BLOCK), 0, (hipStream_t)stream, *bp);
    return check_launch("depth_hypotheses_bwd");
}

}  // extern "C"
