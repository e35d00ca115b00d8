// K7: alpha compositing along rays (network/renderer.py:25-36,109-140 and the nerf-pytorch variant
// utils/run_nerf_helpers.py:343-390 of the reference), forward and backward.
//
// One 64-lane wave per ray.  Lane l owns E consecutive samples [l*E, (l+1)*E): it multiplies its own
// transmittance factors sequentially, the wave combines the 64 lane products with a shuffle scan
// (inclusive product scan, shifted by one lane), and the ray sums are shuffle reductions.  HBM-bound:
// 20 B in + (4..8) B out per sample.
#include "common.h"
#include "composite_device.h"

namespace ucnerf {

template <int E, int VARIANT>
__global__ void __launch_bounds__(256) composite_fwd_kernel(ucnerf_composite_params p) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= p.n) return;
    composite_ray<E, VARIANT>(p, ray, lane, nullptr);
}

// The same ray from the rows of a sorted merge, read where they are (ucnerf_composite_merged_fwd): the wave first inverts its ray's rank row through
// LDS -- inv[rank[j]] = j for j in cat(a, b) order, S ints per wave -- then composite_ray fetches merged position i from row inv[i] of a or b.
template <int E>
__global__ void __launch_bounds__(256) composite_merged_fwd_kernel(ucnerf_composite_merged_params m) {
    extern __shared__ int inv_all[];            // [4 waves][S]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ray = blockIdx.x * 4 + wave;
    const int S = m.na + m.nb;
    int* inv = inv_all + wave * S;
    if (ray < m.n) {
        const int* rank = m.rank + (size_t)ray * S;
        for (int j = lane; j < S; j += 64) {
            const unsigned r = (unsigned)rank[j];
            if (r < (unsigned)S) inv[r] = j;      // (a rank outside the row is dropped: nothing outside this wave's S ints is written)
        }
    }
    __syncthreads();
    if (ray >= m.n) return;
    ucnerf_composite_params p;
    p.n = m.n; p.S = S; p.variant = 0; p.white_bkgd = m.white_bkgd;
    p.raw = nullptr; p.z = m.z; p.rays_d = nullptr; p.noise = nullptr;
    p.rgb_map = m.rgb_map; p.depth_map = m.depth_map; p.acc_map = m.acc_map; p.disp_map = m.disp_map;
    p.weights = m.weights; p.var = m.var; p.u = m.u; p.wu = m.wu;
    const MergedRows rows{reinterpret_cast<const float4*>(m.raw_a), reinterpret_cast<const float4*>(m.raw_b), m.na, m.nb, inv};
    composite_ray<E, 0>(p, ray, lane, nullptr, rows);
}

// Backward of the live variant (composite_bwd_ray of composite_device.h) over the dense array fwd.raw, gradients into g_raw.
template <int E>
__global__ void __launch_bounds__(256) composite_bwd_kernel(ucnerf_composite_bwd_params bp) {
    const ucnerf_composite_params& p = bp.fwd;
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= p.n) return;
    const CompositeUpstream up{bp.g_rgb, bp.g_depth, bp.g_acc, bp.g_weights};
    composite_bwd_ray<E>(p, up, ray, lane, DenseRows(), DenseGradRows{reinterpret_cast<float4*>(bp.g_raw)});
}

// The same backward over the rows of a sorted merge, read and written where they are (ucnerf_composite_merged_bwd): the wave inverts its ray's rank
// row through LDS as composite_merged_fwd_kernel does, loads merged position i from row inv[i] of a or b and stores its gradient to row inv[i] of
// g_raw_a or g_raw_b.  rank is a permutation: every gradient row is written exactly once -- no atomics, no zero fill.
template <int E>
__global__ void __launch_bounds__(256) composite_merged_bwd_kernel(ucnerf_composite_merged_bwd_params m) {
    extern __shared__ int inv_all[];            // [4 waves][S]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ray = blockIdx.x * 4 + wave;
    const int S = m.na + m.nb;
    int* inv = inv_all + wave * S;
    if (ray < m.n) {
        const int* rank = m.rank + (size_t)ray * S;
        for (int j = lane; j < S; j += 64) {
            const unsigned r = (unsigned)rank[j];
            if (r < (unsigned)S) inv[r] = j;      // (a rank outside the row is dropped: nothing outside this wave's S ints is written)
        }
    }
    __syncthreads();
    if (ray >= m.n) return;
    ucnerf_composite_params p;
    p.n = m.n; p.S = S; p.variant = 0; p.white_bkgd = m.white_bkgd;
    p.raw = nullptr; p.z = m.z; p.rays_d = nullptr; p.noise = nullptr;
    p.rgb_map = nullptr; p.depth_map = nullptr; p.acc_map = nullptr; p.disp_map = nullptr;
    p.weights = nullptr; p.var = nullptr; p.u = nullptr; p.wu = nullptr;
    const CompositeUpstream up{m.g_rgb, m.g_depth, m.g_acc, m.g_weights};
    const MergedRows rows{reinterpret_cast<const float4*>(m.raw_a), reinterpret_cast<const float4*>(m.raw_b), m.na, m.nb, inv};
    const MergedGradRows sink{reinterpret_cast<float4*>(m.g_raw_a), reinterpret_cast<float4*>(m.g_raw_b), m.na, m.nb, inv};
    composite_bwd_ray<E>(p, up, ray, lane, rows, sink);
}

template <int E>
static void launch_fwd(const ucnerf_composite_params& p, hipStream_t st) {
    dim3 grid(cdiv(p.n, 4)), block(256);
    if (p.variant == 0) hipLaunchKernelGGL((composite_fwd_kernel<E, 0>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((composite_fwd_kernel<E, 1>), grid, block, 0, st, p);
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_composite_fwd(const ucnerf_composite_params* p, void* stream) {
    UCNERF_REQUIRE(p, "composite_fwd: null params");
    UCNERF_COUNT(p->n);
    UCNERF_REQUIRE(p->raw && p->z && p->rgb_map && p->depth_map, "composite_fwd: null pointer");
    UCNERF_REQUIRE(p->S >= 1 && p->S <= 1024, "composite_fwd: S = %d outside 1..1024", p->S);
    UCNERF_REQUIRE(p->variant == 0 || (p->variant == 1 && p->rays_d), "composite_fwd: variant %d (variant 1 needs rays_d)", p->variant);
    UCNERF_REQUIRE(!p->var || (p->variant == 0 && p->S >= 2), "composite_fwd: var needs the live variant and S >= 2");
    UCNERF_REQUIRE(((uintptr_t)p->raw & 15) == 0, "composite_fwd: raw must be 16-byte aligned");
    UCNERF_REQUIRE(!p->wu || p->u, "composite_fwd: wu (sum of w*u) needs the per-sample uncertainty u");
    UCNERF_COUNT(p->n);
    hipStream_t st = (hipStream_t)stream;
    const int E = composite_lane_samples(p->S);      // (shared with the launch fused with the re-sampling: same lane split, same weights)
    if (E <= 1) launch_fwd<1>(*p, st);
    else if (E <= 2) launch_fwd<2>(*p, st);
    else if (E <= 3) launch_fwd<3>(*p, st);
    else if (E <= 4) launch_fwd<4>(*p, st);
    else if (E <= 8) launch_fwd<8>(*p, st);
    else launch_fwd<16>(*p, st);
    return check_launch("composite_fwd");
}

int ucnerf_composite_merged_fwd(const ucnerf_composite_merged_params* p, void* stream) {
    UCNERF_REQUIRE(p, "composite_merged_fwd: null params");
    UCNERF_COUNT(p->n);
    UCNERF_REQUIRE(p->na >= 0 && p->nb >= 0, "composite_merged_fwd: negative row count (na = %d, nb = %d)", p->na, p->nb);
    const long long S = (long long)p->na + p->nb;
    UCNERF_REQUIRE(S >= 1 && S <= 1024, "composite_merged_fwd: na + nb = %lld outside 1..1024", S);
    UCNERF_REQUIRE((p->raw_a || p->na == 0) && (p->raw_b || p->nb == 0) && p->rank && p->z && p->rgb_map && p->depth_map, "composite_merged_fwd: null pointer");
    UCNERF_REQUIRE(!p->var || S >= 2, "composite_merged_fwd: var needs na + nb >= 2");
    UCNERF_REQUIRE((((uintptr_t)p->raw_a | (uintptr_t)p->raw_b) & 15) == 0, "composite_merged_fwd: raw_a and raw_b must be 16-byte aligned");
    UCNERF_REQUIRE(((uintptr_t)p->rank & 3) == 0, "composite_merged_fwd: rank must be 4-byte aligned");
    UCNERF_REQUIRE(!p->wu || p->u, "composite_merged_fwd: wu (sum of w*u) needs the per-sample uncertainty u");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(cdiv(p->n, 4)), block(256);
    const size_t lds = 4 * (size_t)S * sizeof(int);      // one inverse per wave: at most 16 KB
    const int E = composite_lane_samples((int)S);        // the lane split of ucnerf_composite_fwd at this S: same weights, bit for bit
    if (E <= 1) hipLaunchKernelGGL(composite_merged_fwd_kernel<1>, grid, block, lds, st, *p);
    else if (E <= 2) hipLaunchKernelGGL(composite_merged_fwd_kernel<2>, grid, block, lds, st, *p);
    else if (E <= 3) hipLaunchKernelGGL(composite_merged_fwd_kernel<3>, grid, block, lds, st, *p);
    else if (E <= 4) hipLaunchKernelGGL(composite_merged_fwd_kernel<4>, grid, block, lds, st, *p);
    else if (E <= 8) hipLaunchKernelGGL(composite_merged_fwd_kernel<8>, grid, block, lds, st, *p);
    else hipLaunchKernelGGL(composite_merged_fwd_kernel<16>, grid, block, lds, st, *p);
    return check_launch("composite_merged_fwd");
}

int ucnerf_composite_bwd(const ucnerf_composite_bwd_params* bp, void* stream) {
    UCNERF_REQUIRE(bp, "composite_bwd: null params");
    UCNERF_COUNT(bp->fwd.n);
    UCNERF_REQUIRE(bp->fwd.raw && bp->fwd.z && bp->g_raw, "composite_bwd: null pointer");
    const ucnerf_composite_params& p = bp->fwd;
    UCNERF_REQUIRE(p.variant == 0, "composite_bwd: only the live variant (network/renderer.py) has a backward");
    UCNERF_REQUIRE(p.S >= 1 && p.S <= 1024, "composite_bwd: S = %d outside 1..1024", p.S);
    UCNERF_REQUIRE(((uintptr_t)p.raw & 15) == 0 && ((uintptr_t)bp->g_raw & 15) == 0, "composite_bwd: raw/g_raw must be 16-byte aligned");
    UCNERF_COUNT(p.n);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(cdiv(p.n, 4)), block(256);
    const int E = cdiv(p.S, 64);
    if (E <= 1) hipLaunchKernelGGL(composite_bwd_kernel<1>, grid, block, 0, st, *bp);
    else if (E <= 2) hipLaunchKernelGGL(composite_bwd_kernel<2>, grid, block, 0, st, *bp);
    else if (E <= 3) hipLaunchKernelGGL(composite_bwd_kernel<3>, grid, block, 0, st, *bp);
    else if (E <= 4) hipLaunchKernelGGL(composite_bwd_kernel<4>, grid, block, 0, st, *bp);
    else if (E <= 8) hipLaunchKernelGGL(composite_bwd_kernel<8>, grid, block, 0, st, *bp);
    else hipLaunchKernelGGL(composite_bwd_kernel<16>, grid, block, 0, st, *bp);
    return check_launch("composite_bwd");
}

int ucnerf_composite_merged_bwd(const ucnerf_composite_merged_bwd_params* p, void* stream) {
    UCNERF_REQUIRE(p, "composite_merged_bwd: null params");
    UCNERF_COUNT(p->n);
    UCNERF_REQUIRE(p->na >= 0 && p->nb >= 0, "composite_merged_bwd: negative row count (na = %d, nb = %d)", p->na, p->nb);
    const long long S = (long long)p->na + p->nb;
    UCNERF_REQUIRE(S >= 1 && S <= 1024, "composite_merged_bwd: na + nb = %lld outside 1..1024", S);
    UCNERF_REQUIRE(((p->raw_a && p->g_raw_a) || p->na == 0) && ((p->raw_b && p->g_raw_b) || p->nb == 0) && p->rank && p->z,
                   "composite_merged_bwd: null pointer");
    UCNERF_REQUIRE((((uintptr_t)p->raw_a | (uintptr_t)p->raw_b | (uintptr_t)p->g_raw_a | (uintptr_t)p->g_raw_b) & 15) == 0,
                   "composite_merged_bwd: raw_a, raw_b, g_raw_a and g_raw_b must be 16-byte aligned");
    UCNERF_REQUIRE(((uintptr_t)p->rank & 3) == 0, "composite_merged_bwd: rank must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(cdiv(p->n, 4)), block(256);
    const size_t lds = 4 * (size_t)S * sizeof(int);      // one inverse per wave: at most 16 KB
    const int E = cdiv(S, 64);                           // the lane split of ucnerf_composite_bwd at this S: same gradients, bit for bit
    if (E <= 1) hipLaunchKernelGGL(composite_merged_bwd_kernel<1>, grid, block, lds, st, *p);
    else if (E <= 2) hipLaunchKernelGGL(composite_merged_bwd_kernel<2>, grid, block, lds, st, *p);
    else if (E <= 3) hipLaunchKernelGGL(composite_merged_bwd_kernel<3>, grid, block, lds, st, *p);
    else if (E <= 4) hipLaunchKernelGGL(composite_merged_bwd_kernel<4>, grid, block, lds, st, *p);
    else if (E <= 8) hipLaunchKernelGGL(composite_merged_bwd_kernel<8>, grid, block, lds, st, *p);
    else hipLaunchKernelGGL(composite_merged_bwd_kernel<16>, grid, block, lds, st, *p);
    return check_launch("composite_merged_bwd");
}

}  // extern "C"
