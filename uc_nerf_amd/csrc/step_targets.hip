// t1, the training step's three target gathers (train.py:166-176) in ONE launch: sparse_depths[:, r, c] and sparse_weights[:, r, c] over the
// rays from n_rays on, dpt[:, r, c] over the first patch_num * patch_size^2 rays, (r, c) = the columns of pixel_coordinates.  In torch this is
// slicing plus index kernels (about eight launches), and a coordinate outside the image is a device-side assert that ends the process.  Here a
// coordinate outside [-H, H) x [-W, W) -- or a float that is no whole number -- gives NaN in its own element and one bit of a sticky status
// word; nothing else is touched and nothing is read back.
//
// One thread per output element (a depth ray's thread stores its two values), plain vector loads and stores, no LDS, no atomic but the
// status word's atomicOr (issued only by a thread whose coordinate is outside).  Every address is formed from an index that passed the range
// test: see st_index(), the only place an offset is computed.
//
// Bound: launch latency.  A step moves (2 (n_total - n_rays) + patch_num * patch_size^2) floats, a few thousand; the kernel is over before its
// launch overhead is.  It is not tuned, and is not meant to be.
#include "common.h"

namespace ucnerf {

constexpr int ST_BLOCK = 256;
constexpr int ST_MAX_SIDE = 1 << 24;       // every row / column index is exact in float32; H W fits in int64 with room to spare
constexpr int ST_MAX_N = 1 << 29;           // n_depth + n_patch <= 2 n_total stays inside int32

__device__ __forceinline__ float st_nan() { return __uint_as_float(0x7fc00000u); }

// coordinate `col` of row `which` (0: image rows, 1: image columns) of pixel_coordinates [2, n_total] as a wrapped index into `size`, or -1:
// torch's advanced indexing takes [-size, size) and adds size to a negative index
__device__ __forceinline__ int st_coord(const ucnerf_step_targets_params& p, int which, int col, int size) {
    const long long at = (long long)which * p.n_total + col;               // (col < n_total <= 2^29)
    long long v;
    if (p.coord_is_float) {
        const float f = static_cast<const float*>(p.pixel_coordinates)[at];
        if (!(f >= -(float)size && f < (float)size) || f != truncf(f)) return -1;      // (NaN fails the first test; |f| < 2^24: the cast is exact)
        v = (long long)f;
    } else {
        v = static_cast<const int64_t*>(p.pixel_coordinates)[at];
        if (v < -(long long)size || v >= (long long)size) return -1;
    }
    return (int)(v < 0 ? v + size : v);
}

// the offset of pixel_coordinates' column `col` inside an [H, W] map, or -1: the ONLY offset this file forms, from two indices inside 0 .. H-1 / 0 .. W-1
__device__ __forceinline__ long long st_index(const ucnerf_step_targets_params& p, int col) {
    const int r = st_coord(p, 0, col, p.H), c = st_coord(p, 1, col, p.W);
    return r < 0 || c < 0 ? -1 : (long long)r * p.W + c;
}

__global__ void __launch_bounds__(ST_BLOCK) step_targets_kernel(ucnerf_step_targets_params p, int n_depth, int n_patch) {
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;                     // (n_depth + n_patch <= 2^30: n_total <= 2^29 on the host)
    if (i < n_depth) {
        const long long at = st_index(p, p.n_rays + i);                    // (n_rays + i < n_total)
        p.target_depths[i] = at < 0 ? st_nan() : p.sparse_depths[at];
        p.target_weights[i] = at < 0 ? st_nan() : p.sparse_weights[at];
        if (at < 0 && p.status) atomicOr(p.status, 1u);
    } else if (i - n_depth < n_patch) {
        const int j = i - n_depth;                                         // (j < patch_num * patch_size^2 <= n_total)
        const long long at = st_index(p, j);
        p.patch_dpt[j] = at < 0 ? st_nan() : p.dpt[at];
        if (at < 0 && p.status) atomicOr(p.status, 2u);
    }
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_step_targets(const ucnerf_step_targets_params* p, void* stream) {
    UCNERF_REQUIRE(p, "step_targets: null params");
    UCNERF_REQUIRE(p->H >= 0 && p->W >= 0 && p->n_total >= 0 && p->n_rays >= 0 && p->patch_num >= 0 && p->patch_size >= 0,
                   "step_targets: H=%d W=%d n_total=%d n_rays=%d patch_num=%d patch_size=%d (negative)", p->H, p->W, p->n_total, p->n_rays, p->patch_num,
                   p->patch_size);
    UCNERF_REQUIRE(p->H <= ST_MAX_SIDE && p->W <= ST_MAX_SIDE && p->n_total <= ST_MAX_N, "step_targets: H=%d or W=%d above 2^24, or n_total=%d above 2^29",
                   p->H, p->W, p->n_total);
    UCNERF_REQUIRE(p->n_rays <= p->n_total, "step_targets: n_rays = %d above n_total = %d", p->n_rays, p->n_total);
    const long long ps2 = (long long)p->patch_size * p->patch_size;       // (< 2^62; the product with patch_num is formed only once ps2 <= n_total)
    const long long n_patch = p->patch_num == 0 || ps2 > p->n_total ? 0 : p->patch_num * ps2;
    UCNERF_REQUIRE(p->patch_num == 0 || (ps2 <= p->n_total && n_patch <= p->n_total),
                   "step_targets: %d patches of %d x %d pixels are more than the n_total = %d rays", p->patch_num, p->patch_size, p->patch_size, p->n_total);
    UCNERF_REQUIRE(p->coord_is_float == 0 || p->coord_is_float == 1, "step_targets: coord_is_float = %d (0: int64, 1: float32)", p->coord_is_float);
    const int n_depth = p->n_total - p->n_rays;
    if (n_depth + n_patch == 0) return UCNERF_OK;                          // both outputs empty: nothing to launch
    UCNERF_REQUIRE(p->H >= 1 && p->W >= 1, "step_targets: a %d x %d map has no pixel to gather", p->H, p->W);
    UCNERF_REQUIRE(p->pixel_coordinates, "step_targets: null pixel_coordinates");
    UCNERF_REQUIRE(((uintptr_t)p->pixel_coordinates & (p->coord_is_float ? 3 : 7)) == 0, "step_targets: pixel_coordinates is misaligned for its element type");
    UCNERF_REQUIRE(n_depth == 0 || (p->sparse_depths && p->sparse_weights && p->target_depths && p->target_weights),
                   "step_targets: null sparse_depths, sparse_weights, target_depths or target_weights");
    UCNERF_REQUIRE(n_patch == 0 || (p->dpt && p->patch_dpt), "step_targets: null dpt or patch_dpt");
    hipLaunchKernelGGL(step_targets_kernel, dim3(cdiv(n_depth + n_patch, ST_BLOCK)), dim3(ST_BLOCK), 0, (hipStream_t)stream, *p, n_depth, (int)n_patch);
    return check_launch("step_targets");
}

}  // extern "C"
