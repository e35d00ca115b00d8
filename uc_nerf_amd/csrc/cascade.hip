// f2, the link between two cascade stages: the previous stage's depth map -> the next stage's per-pixel hypothesis volume
// depth_values [D, h + 2 pad, w + 2 pad]  (network/mvs_models.py:536-573 get_*depth_range_samples, :693-762 CascadeMVSNet.forward).
// The reference up-samples the depth to full resolution, builds a FULL-resolution [D,H,W] volume there (15.7 MB at stage 1 of a 256 x 320
// image) and interpolates it back down; here one thread owns one output column (y, x): it rebuilds the at most 2 x 2 full-resolution
// pixels its down-sampling taps touch -- each a 2 x 2 bilinear sample of the depth map, which stays in L2 -- and writes its D values.
// Nothing of full resolution is stored: the traffic is the output (<= 2.6 MB per stage), so what the launch costs is mostly its latency.
// No LDS, no matrix cores; a wave's store is 256 contiguous bytes of one depth plane.
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
            const float lo = fmaxf(c - half, near), hi = fminf(c + half, far);      // :540-541
            mn[a][b] = lo;
            interval[a][b] = (hi - lo) / steps;                                      // :544
        }
    for (int d = d_begin; d < d_end; ++d, out += plane) {
        const float fd = (float)d;
        const float s00 = mn[0][0] + fd * interval[0][0], s01 = mn[0][1] + fd * interval[0][1];      // :546-549
        const float s10 = mn[1][0] + fd * interval[1][0], s11 = mn[1][1] + fd * interval[1][1];
        *out = ty.l0 * (tx.l0 * s00 + tx.l1 * s01) + ty.l1 * (tx.l0 * s10 + tx.l1 * s11);
    }
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

}  // extern "C"
