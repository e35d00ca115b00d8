// e2, the middle of the validation loop on the device (train.py:274-288 of the reference): a rendered chunk is written straight into the image
// planes the metrics of metrics.hip read -- rgb clamped to [0, 1] and transposed to [3, H W], depth as it is --, the depth range is folded into a
// two-word cell in the same pass, and visualize_depth (utils/utils.py:58-77: numpy normalisation, cv2.applyColorMap, ToTensor) becomes one launch
// that reads the cell.  Plain HIP C++, wave64.  Every kernel moves a few bytes per pixel: what matters is that a wave's plane stores are
// consecutive addresses, that a workgroup issues ONE atomicMin and ONE atomicMax, and that the float32 arithmetic is numpy's, rounding for rounding.
//
// Arithmetic.  The build compiles with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt (uc_nerf_amd/build.py): `a / b` below is an
// IEEE division, never a multiplication by a reciprocal, and 255 * ((x - mi) / d) stays a division followed by a multiplication -- two roundings.
// On the lattice x = j, mi = 0, d = 255 that pair of roundings returns j for every j = 0 .. 255, as numpy's does; a quotient one unit in the last
// place low -- what a division that is not correctly rounded may give -- truncates to j - 1 at nearly every j (tests/test_image_cases_host.py).
//
// The range cell.  Two uint32 words: the smallest and the largest ORDER KEY seen (the key of metrics.hip: negatives with all bits flipped, the
// others with the sign bit set, so that unsigned order is float order and -0.0 sits right below +0.0).  An empty cell is (0xffffffff, 0); both
// decode to NaN, so a colour map made from an empty cell is index 0 everywhere rather than something that looks like a depth.  No entry point
// synchronises the stream or reads anything back.
#include "common.h"

#include <cfloat>

namespace ucnerf {

constexpr int IM_BLOCK = 256;
constexpr int IM_WAVES = IM_BLOCK / 64;
constexpr int IM_ITEMS = 4;                               // pixels per thread
constexpr int IM_GROUP = IM_BLOCK * IM_ITEMS;             // pixels per workgroup: 1024 (tests/image_cases.py: GROUP_PIXELS)
constexpr unsigned KEY_NONE_MIN = 0xffffffffu, KEY_NONE_MAX = 0u;

__device__ __forceinline__ unsigned im_order_key(float f) {
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float im_key_value(unsigned k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

// np.nan_to_num on float32: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX, everything else (denormals, -0.0) unchanged
__device__ __forceinline__ float nan_to_num(float x) {
    if (x != x) return 0.f;
    if (x == INFINITY) return FLT_MAX;
    if (x == -INFINITY) return -FLT_MAX;
    return x;
}

// torch.clamp(x, 0, 1): min(max(x, 0), 1) by comparison -- a NaN fails both and stays, -0.0 is not below 0 and stays (fmaxf / fminf promise neither)
__device__ __forceinline__ float clamp01(float x) {
    const float lo = x < 0.f ? 0.f : x;
    return 1.f < lo ? 1.f : lo;
}

// all IM_BLOCK threads call it; one atomicMin and one atomicMax per workgroup (none from a workgroup that saw no element)
__device__ __forceinline__ void fold_range(unsigned kmin, unsigned kmax, unsigned* cell) {
    __shared__ unsigned lmin[IM_WAVES], lmax[IM_WAVES];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned a = __shfl_down(kmin, d), b = __shfl_down(kmax, d);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if ((threadIdx.x & 63) == 0) { lmin[threadIdx.x >> 6] = kmin; lmax[threadIdx.x >> 6] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < IM_WAVES; ++w) { kmin = lmin[w] < kmin ? lmin[w] : kmin; kmax = lmax[w] > kmax ? lmax[w] : kmax; }
        if (kmin <= kmax) {                                // (an empty fold holds 0xffffffff above 0)
            atomicMin(cell, kmin);
            atomicMax(cell + 1, kmax);
        }
    }
}

__global__ void minmax_reset_kernel(unsigned* cell) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { cell[0] = KEY_NONE_MIN; cell[1] = KEY_NONE_MAX; }
}

__global__ void minmax_read_kernel(const unsigned* cell, float* out) {
    if (threadIdx.x < 2 && blockIdx.x == 0) out[threadIdx.x] = im_key_value(cell[threadIdx.x]);
}

// Block b owns chunk pixels b * 1024 .. + 1023; thread t takes b * 1024 + k * 256 + t, k = 0 .. 3: a wave's 64 stores to a plane are 256
// consecutive bytes.  (The chunk's rgb rows are 12 bytes: a wave's three loads cover the same 768 consecutive bytes.)
__global__ void __launch_bounds__(IM_BLOCK) image_put_kernel(ucnerf_image_put_params p) {
    const long long plane = p.pixels;
    unsigned kmin = KEY_NONE_MIN, kmax = KEY_NONE_MAX;
#pragma unroll
    for (int k = 0; k < IM_ITEMS; ++k) {
        const long long i = (long long)blockIdx.x * IM_GROUP + k * IM_BLOCK + threadIdx.x;
        if (i >= p.n) continue;                             // (host: first_pixel + n <= pixels, so every store below is inside its plane)
        const long long at = (long long)p.first_pixel + i;
        const float r = p.rgb[3 * i], g = p.rgb[3 * i + 1], b = p.rgb[3 * i + 2], d = p.depth[i];
        p.rgb_chw[at] = clamp01(r);
        p.rgb_chw[plane + at] = clamp01(g);
        p.rgb_chw[2 * plane + at] = clamp01(b);
        p.depth_hw[at] = d;
        const unsigned key = im_order_key(nan_to_num(d));
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
    }
    if (p.minmax) fold_range(kmin, kmax, p.minmax);          // (uniform)
}

__global__ void __launch_bounds__(IM_BLOCK) depth_minmax_kernel(ucnerf_depth_minmax_params p) {
    unsigned kmin = KEY_NONE_MIN, kmax = KEY_NONE_MAX;
#pragma unroll
    for (int k = 0; k < IM_ITEMS; ++k) {
        const long long i = (long long)blockIdx.x * IM_GROUP + k * IM_BLOCK + threadIdx.x;
        if (i >= p.count) continue;
        const unsigned key = im_order_key(nan_to_num(p.depth[i]));
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
    }
    fold_range(kmin, kmax, p.minmax);
}

// visualize_depth's arithmetic (utils/utils.py:65-76).  The 768 quotients table / 255 are formed once per workgroup into LDS (the same
// correctly rounded division ToTensor does per pixel); a pixel's three colours are then three LDS reads and three plane stores.
__global__ void __launch_bounds__(IM_BLOCK) depth_colormap_kernel(ucnerf_depth_colormap_params p, float mi_host, float d_host) {
    __shared__ float lut[256 * 3];
    if (p.color) {
        for (int e = threadIdx.x; e < 256 * 3; e += IM_BLOCK) lut[e] = (float)p.table[e] / 255.0f;
        __syncthreads();
    }
    float mi, d;
    if (p.minmax) {
        mi = im_key_value(p.minmax[0]);
        const float ma = im_key_value(p.minmax[1]);
        d = (ma - mi) + 1e-8f;                               // np.float32 scalars with a weak Python float: all in float32
    } else {
        mi = mi_host;
        d = d_host;
    }
    const long long plane = p.count;
#pragma unroll
    for (int k = 0; k < IM_ITEMS; ++k) {
        const long long i = (long long)blockIdx.x * IM_GROUP + k * IM_BLOCK + threadIdx.x;
        if (i >= p.count) continue;
        const float x = nan_to_num(p.depth[i]);
        const float t = (x - mi) / d;                        // first rounding: an IEEE division
        const float v = 255.0f * t;                          // second rounding: not fused with it
        // uint8(v) truncates toward zero where numpy defines it; the rest is this library's: NaN -> 0, below 0 -> 0, above 255 -> 255
        const int idx = v != v ? 0 : (v < 0.f ? 0 : (v > 255.f ? 255 : (int)v));
        if (p.index) p.index[i] = (uint8_t)idx;
        if (p.color) {
            p.color[i] = lut[3 * idx];
            p.color[plane + i] = lut[3 * idx + 1];
            p.color[2 * plane + i] = lut[3 * idx + 2];
        }
    }
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int32_t ucnerf_image_group_pixels(void) { return IM_GROUP; }

int ucnerf_minmax_reset(uint32_t* minmax, void* stream) {
    UCNERF_REQUIRE(minmax, "minmax_reset: null cell");
    UCNERF_REQUIRE(((uintptr_t)minmax & 3) == 0, "minmax_reset: the cell must be 4-byte aligned");
    hipLaunchKernelGGL(minmax_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, minmax);
    return check_launch("minmax_reset");
}

int ucnerf_minmax_read(const uint32_t* minmax, float* out, void* stream) {
    UCNERF_REQUIRE(minmax && out, "minmax_read: null cell or out");
    UCNERF_REQUIRE((((uintptr_t)minmax | (uintptr_t)out) & 3) == 0, "minmax_read: the cell and out must be 4-byte aligned");
    hipLaunchKernelGGL(minmax_read_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, minmax, out);
    return check_launch("minmax_read");
}

int ucnerf_image_put(const ucnerf_image_put_params* p, void* stream) {
    UCNERF_REQUIRE(p, "image_put: null params");
    UCNERF_REQUIRE(p->n >= 0 && p->first_pixel >= 0 && p->pixels >= 0, "image_put: n=%d first_pixel=%d pixels=%d (negative)", p->n, p->first_pixel, p->pixels);
    UCNERF_REQUIRE((long long)p->first_pixel + p->n <= (long long)p->pixels, "image_put: pixels %d .. %lld overrun the image of %d pixels", p->first_pixel,
                   (long long)p->first_pixel + p->n - 1, p->pixels);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->rgb && p->depth && p->rgb_chw && p->depth_hw, "image_put: null rgb, depth, rgb_chw or depth_hw");
    UCNERF_REQUIRE((((uintptr_t)p->rgb | (uintptr_t)p->depth | (uintptr_t)p->rgb_chw | (uintptr_t)p->depth_hw | (uintptr_t)p->minmax) & 3) == 0,
                   "image_put: every array must be 4-byte aligned");
    hipLaunchKernelGGL(image_put_kernel, dim3(cdiv(p->n, IM_GROUP)), dim3(IM_BLOCK), 0, (hipStream_t)stream, *p);
    return check_launch("image_put");
}

int ucnerf_depth_minmax(const ucnerf_depth_minmax_params* p, void* stream) {
    UCNERF_REQUIRE(p, "depth_minmax: null params");
    UCNERF_COUNT(p->count);
    UCNERF_REQUIRE(p->depth && p->minmax, "depth_minmax: null depth or cell");
    UCNERF_REQUIRE((((uintptr_t)p->depth | (uintptr_t)p->minmax) & 3) == 0, "depth_minmax: every array must be 4-byte aligned");
    hipLaunchKernelGGL(depth_minmax_kernel, dim3(cdiv(p->count, IM_GROUP)), dim3(IM_BLOCK), 0, (hipStream_t)stream, *p);
    return check_launch("depth_minmax");
}

int ucnerf_depth_colormap(const ucnerf_depth_colormap_params* p, void* stream) {
    UCNERF_REQUIRE(p, "depth_colormap: null params");
    UCNERF_COUNT(p->count);
    UCNERF_REQUIRE(p->depth, "depth_colormap: null depth");
    UCNERF_REQUIRE(p->index || p->color, "depth_colormap: null index and color (nothing to write)");
    UCNERF_REQUIRE(!p->color || p->table, "depth_colormap: a colour image needs the 256 x 3 table");
    UCNERF_REQUIRE((((uintptr_t)p->depth | (uintptr_t)p->color | (uintptr_t)p->minmax) & 3) == 0, "depth_colormap: depth, color and the cell must be 4-byte aligned");
    float mi = 0.f, d = 0.f;
    if (!p->minmax) {
        // a caller's pair of Python floats: x - mi rounds mi to float32 first, the denominator is formed in double and rounded once (utils/utils.py:70-72)
        mi = (float)p->range_host[0];
        d = (float)(p->range_host[1] - p->range_host[0] + 1e-8);
    }
    hipLaunchKernelGGL(depth_colormap_kernel, dim3(cdiv(p->count, IM_GROUP)), dim3(IM_BLOCK), 0, (hipStream_t)stream, *p, mi, d);
    return check_launch("depth_colormap");
}

}  // extern "C"
