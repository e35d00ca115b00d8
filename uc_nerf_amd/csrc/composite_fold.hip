// K7 gradient fold: the chain-rule terms of the compositing's extra maps -- var (unbiased variance of the weights), disp and the composited
// uncertainty wu = sum_i w_i u_i -- added to the upstream gradients of depth, acc and weights, so that ucnerf_composite_bwd /
// ucnerf_composite_merged_bwd carry a loss on those maps to the network unchanged (include/ucnerf_hip.h: ucnerf_composite_fold_grads).
//
// One 64-lane wave per ray, lane l owns the E consecutive samples [l*E, (l+1)*E) as in composite_ray: the row sum of the weights is the
// forward's acc, bit for bit.  HBM-bound: up to 12 B in + 8 B out per sample; every output element is stored exactly once.
#include <cfloat>

#include "common.h"
#include "composite_device.h"

namespace ucnerf {

template <int E>
__global__ void __launch_bounds__(256) composite_fold_kernel(ucnerf_composite_fold_params p) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= p.n) return;
    const size_t row = (size_t)ray * p.S;
    float w[E];
    float sa = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        w[e] = i < p.S ? p.weights[row + i] : 0.f;
        if (i < p.S) sa += w[e];
    }
    float gv = 0.f, mean = 0.f;
    if (p.g_var) {                              // d var / d w_i = 2 (w_i - mean) / (S - 1)
        gv = p.g_var[ray];
        mean = wave_sum(sa) / (float)p.S;
    }
    const float gu = p.g_wu ? p.g_wu[ray] : 0.f;
    const float den = (float)(p.S - 1);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < p.S) {
            float g = p.g_weights ? p.g_weights[row + i] : 0.f;
            if (p.g_var) g += gv * ((2.f * (w[e] - mean)) / den);
            if (p.g_wu) g += gu * p.u[row + i];
            p.g_weights_out[row + i] = g;
            if (p.g_u) p.g_u[row + i] = gu * w[e];
        }
    }
    if (lane == 0) {
        float gd = p.g_depth ? p.g_depth[ray] : 0.f, ga = p.g_acc ? p.g_acc[ray] : 0.f;
        if (p.g_disp) {                         // disp = 1 / max(1e-10, depth / acc): no gradient where the clamp is active or the ratio not finite
            const float acc = p.acc[ray];
            const float q = p.depth[ray] / acc;
            if (q > 1e-10f && q <= FLT_MAX) {
                const float gdisp = p.g_disp[ray];
                const float d = 1.f / q;
                const float t = (d * d) / acc;
                gd += gdisp * (-t);
                ga += gdisp * (t * q);
            }
        }
        p.g_depth_out[ray] = gd;
        p.g_acc_out[ray] = ga;
    }
}

struct Span { const void* ptr; size_t bytes; };
static bool overlap(const Span& a, const Span& b) {
    if (!a.ptr || !b.ptr || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.ptr, b0 = (uintptr_t)b.ptr;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_composite_fold_grads(const ucnerf_composite_fold_params* p, void* stream) {
    UCNERF_REQUIRE(p, "composite_fold_grads: null params");
    UCNERF_COUNT(p->n);
    UCNERF_REQUIRE(p->S >= 1 && p->S <= 1024, "composite_fold_grads: S = %d outside 1..1024", p->S);
    UCNERF_REQUIRE(p->weights && p->depth && p->acc && p->g_depth_out && p->g_acc_out && p->g_weights_out, "composite_fold_grads: null pointer");
    UCNERF_REQUIRE(!p->g_var || p->S >= 2, "composite_fold_grads: g_var needs S >= 2 (the unbiased variance of one weight is undefined)");
    UCNERF_REQUIRE(!p->g_wu || p->u, "composite_fold_grads: g_wu (gradient of sum of w*u) needs the per-sample uncertainty u");
    const size_t ray_bytes = (size_t)p->n * sizeof(float), row_bytes = ray_bytes * (size_t)p->S;
    const Span in[] = {{p->weights, row_bytes}, {p->depth, ray_bytes}, {p->acc, ray_bytes}, {p->u, row_bytes}, {p->g_var, ray_bytes}, {p->g_disp, ray_bytes},
                       {p->g_wu, ray_bytes}, {p->g_depth, ray_bytes}, {p->g_acc, ray_bytes}, {p->g_weights, row_bytes}};
    const Span out[] = {{p->g_depth_out, ray_bytes}, {p->g_acc_out, ray_bytes}, {p->g_weights_out, row_bytes}, {p->g_u, row_bytes}};
    for (int o = 0; o < 4; ++o) {
        for (const Span& i : in) UCNERF_REQUIRE(!overlap(out[o], i), "composite_fold_grads: an output overlaps an input (outputs may not alias inputs)");
        for (int o2 = o + 1; o2 < 4; ++o2) UCNERF_REQUIRE(!overlap(out[o], out[o2]), "composite_fold_grads: two outputs overlap");
    }
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(cdiv(p->n, 4)), block(256);
    const int E = composite_lane_samples(p->S);          // the lane split of ucnerf_composite_fwd at this S: the same row sum, bit for bit
    if (E <= 1) hipLaunchKernelGGL(composite_fold_kernel<1>, grid, block, 0, st, *p);
    else if (E <= 2) hipLaunchKernelGGL(composite_fold_kernel<2>, grid, block, 0, st, *p);
    else if (E <= 3) hipLaunchKernelGGL(composite_fold_kernel<3>, grid, block, 0, st, *p);
    else if (E <= 4) hipLaunchKernelGGL(composite_fold_kernel<4>, grid, block, 0, st, *p);
    else if (E <= 8) hipLaunchKernelGGL(composite_fold_kernel<8>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(composite_fold_kernel<16>, grid, block, 0, st, *p);
    return check_launch("composite_fold_grads");
}

}  // extern "C"
