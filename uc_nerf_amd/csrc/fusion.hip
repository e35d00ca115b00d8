// e1, multi-view depth fusion: the geometric consistency filter over N per-view depth maps (ONE launch) and the compaction of the surviving
// pixels to a coloured world-space point cloud (a counted, fixed-order scan: count -> exclusive scan -> scatter).  Plain HIP C++, wave64, plain
// vector loads and stores, NO atomics: bit-identical from launch to launch.  Nothing is read back.
//
// Arithmetic (the build compiles with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt: every fmaf below is written out, every
// `a / b` is an IEEE division, sqrtf is correctly rounded).  Pixel convention of raygen_device.h: integer pixel (x, y), zero skew.
//   M . (a, b, c):     row i = fmaf(M[i][2], c, fmaf(M[i][1], b, M[i][0] * a)) + M[i][3]                                   (fu_apply)
//   back(K, x, y, d):  ((x - K02) / K00 * d, (y - K12) / K11 * d, d)                                                       (fu_back)
//   proj(K, Q):        (K00 * Q.x / Q.z + K02, K11 * Q.y / Q.z + K12): product, division, sum                              (fu_proj)
// Per reference pixel and source, in source-slot order (include/ucnerf_hip.h has every rule for invalid inputs):
//   X = c2w_r . back(K_r, x, y, d);  Q = w2c_s . X;  (u, v) = proj(K_s, Q);  d_s = bilinear(depth_s, u, v), a zero-weight tap not read;
//   Q' = w2c_r . (c2w_s . back(K_s, u, v, d_s));  d' = Q'.z;  (x', y') = proj(K_r, Q');
//   consistent iff sqrtf(fmaf(ey, ey, ex * ex)) < pix_thresh and fabsf(d' - d) / d < rel_thresh;  fused = (d + sum d') / (float)(count + 1).
// w2cs == NULL: the rigid inverse of novel.hip, [R^T | -R^T t] with the translation -fmaf(R[2][r], t[2], fmaf(R[1][r], t[1], R[0][r] * t[0])).
//
// Consistency kernel: a workgroup is 256 consecutive pixels of ONE view r (grid = N x ceil(H W / 256)); its threads first write r's camera and
// the cameras of r's S sources to LDS (28 floats each: fx cx fy cy, three rows of c2w, three rows of w2c), so the per-view matrices are formed
// once per workgroup and read as LDS broadcasts; the per-pixel state stays in registers.  The reference row is read coalesced; the sources'
// taps are a data-dependent gather and are not tiled.  Latency- / gather-bound: 4 taps x S sources per pixel.
//
// Compaction: FU_ITEMS = 1024 pixels a workgroup (4 consecutive mask bytes a thread).  pc_count writes the workgroup's number of masked pixels;
// pc_scan (ONE workgroup) turns the counts into exclusive offsets in place, FU_BLOCK counts a pass with a running carry, and writes the total;
// pc_scatter ranks its masked pixels in thread order (= pixel order) from its offset and stores rows below cap.
#include "common.h"

#include <cmath>

namespace ucnerf {

constexpr int FU_BLOCK = 256;
constexpr int FU_MAX_SRC = 32;
constexpr int FU_CAM = 28;                                 // fx cx fy cy | c2w rows 0..2 | w2c rows 0..2
constexpr int FU_PER = 4;                                  // mask bytes per thread of the compaction
constexpr int FU_ITEMS = FU_BLOCK * FU_PER;

__device__ __forceinline__ void fu_apply(const float* M, float a, float b, float c, float* x, float* y, float* z) {
    float r0 = M[0] * a, r1 = M[4] * a, r2 = M[8] * a;
    r0 = fmaf(M[1], b, r0); r1 = fmaf(M[5], b, r1); r2 = fmaf(M[9], b, r2);
    r0 = fmaf(M[2], c, r0); r1 = fmaf(M[6], c, r1); r2 = fmaf(M[10], c, r2);
    *x = r0 + M[3]; *y = r1 + M[7]; *z = r2 + M[11];
}

// cam = fx cx fy cy
__device__ __forceinline__ void fu_back(const float* cam, float x, float y, float d, float* a, float* b, float* c) {
    *a = (x - cam[1]) / cam[0] * d;
    *b = (y - cam[3]) / cam[2] * d;
    *c = d;
}

__device__ __forceinline__ void fu_proj(const float* cam, float qx, float qy, float qz, float* u, float* v) {
    *u = cam[0] * qx / qz + cam[1];
    *v = cam[2] * qy / qz + cam[3];
}

__device__ __forceinline__ bool fu_pos_finite(float v) { return v > 0.0f && v < INFINITY; }      // (false for a NaN)

// Element e of view `view`'s 28-float camera record.
__device__ __forceinline__ float fu_cam_entry(const ucnerf_depth_consistency_params& p, int view, int e) {
    if (e < 4) {
        const float* K = p.intrinsics + (long long)view * 9;
        return e == 0 ? K[0] : (e == 1 ? K[2] : (e == 2 ? K[4] : K[5]));
    }
    if (e < 16) return p.c2ws[(long long)view * 16 + (e - 4)];
    e -= 16;
    if (p.w2cs) return p.w2cs[(long long)view * 16 + e];
    const float* c = p.c2ws + (long long)view * 16;
    const int r = e >> 2, col = e & 3;
    if (col < 3) return c[col * 4 + r];
    float acc = c[r] * c[3];
    acc = fmaf(c[4 + r], c[7], acc);
    acc = fmaf(c[8 + r], c[11], acc);
    return -acc;
}

__global__ void __launch_bounds__(FU_BLOCK) depth_consistency_kernel(ucnerf_depth_consistency_params p, int blocks_per_view) {
    __shared__ float cams[(FU_MAX_SRC + 1) * FU_CAM];      // record 0: the reference view; 1 + j: source slot j
    __shared__ int sid[FU_MAX_SRC];
    const int r = blockIdx.x / blocks_per_view;
    const int HW = p.H * p.W;
    const int q = (blockIdx.x - r * blocks_per_view) * FU_BLOCK + threadIdx.x;
    for (int j = threadIdx.x; j < p.S; j += FU_BLOCK) {
        const int s = p.src_ids[(long long)r * p.S + j];
        sid[j] = (s < 0 || s == r || s >= p.N) ? -1 : s;
    }
    for (int i = threadIdx.x; i < (p.S + 1) * FU_CAM; i += FU_BLOCK) {
        const int j = i / FU_CAM, e = i - j * FU_CAM;
        int view = r;
        if (j > 0) {
            const int s = p.src_ids[(long long)r * p.S + (j - 1)];
            view = (s < 0 || s == r || s >= p.N) ? -1 : s;
        }
        cams[i] = view < 0 ? 0.0f : fu_cam_entry(p, view, e);
    }
    __syncthreads();
    if (q >= HW) return;
    const long long at = (long long)r * HW + q;
    const int yi = q / p.W, xi = q - yi * p.W;
    const float x = (float)xi, y = (float)yi;
    const float d = p.depth[at];
    bool valid = fu_pos_finite(d);
    if (p.conf) {
        const float c = p.conf[at];
        valid = valid && c >= p.conf_thresh && fabsf(c) < INFINITY;                 // (a NaN fails the first comparison, an infinity the second)
    }
    if (!valid) {
        p.count[at] = 0;
        p.mask[at] = 0;
        p.fused[at] = 0.0f;
        return;
    }
    const float* ref = cams;
    float a, b, c, X, Y, Z;
    fu_back(ref, x, y, d, &a, &b, &c);
    fu_apply(ref + 4, a, b, c, &X, &Y, &Z);
    const float umax = (float)(p.W - 1), vmax = (float)(p.H - 1);
    int count = 0;
    float sum = d;
    for (int j = 0; j < p.S; ++j) {
        const int s = sid[j];
        if (s < 0) continue;                                                         // (uniform over the workgroup)
        const float* src = cams + (j + 1) * FU_CAM;
        float qx, qy, qz;
        fu_apply(src + 16, X, Y, Z, &qx, &qy, &qz);
        if (!fu_pos_finite(qz)) continue;
        float u, v;
        fu_proj(src, qx, qy, qz, &u, &v);
        if (!(u >= 0.0f && u <= umax && v >= 0.0f && v <= vmax)) continue;
        const float fx0 = floorf(u), fy0 = floorf(v);
        const float wa = u - fx0, wb = v - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;                                       // 0 .. W-1, 0 .. H-1
        const float w00 = (1.0f - wa) * (1.0f - wb), w01 = wa * (1.0f - wb), w10 = (1.0f - wa) * wb, w11 = wa * wb;
        const float* ds = p.depth + (long long)s * HW + (long long)y0 * p.W + x0;
        // a tap is read only under a non-zero weight: wa != 0 implies x0 <= W - 2, wb != 0 implies y0 <= H - 2
        const float t00 = w00 != 0.0f ? ds[0] : 1.0f;
        const float t01 = w01 != 0.0f ? ds[1] : 1.0f;
        const float t10 = w10 != 0.0f ? ds[p.W] : 1.0f;
        const float t11 = w11 != 0.0f ? ds[p.W + 1] : 1.0f;
        if (!(fu_pos_finite(t00) && fu_pos_finite(t01) && fu_pos_finite(t10) && fu_pos_finite(t11))) continue;
        float dsrc = 0.0f;
        if (w00 != 0.0f) dsrc = fmaf(w00, t00, dsrc);
        if (w01 != 0.0f) dsrc = fmaf(w01, t01, dsrc);
        if (w10 != 0.0f) dsrc = fmaf(w10, t10, dsrc);
        if (w11 != 0.0f) dsrc = fmaf(w11, t11, dsrc);
        float sa, sb, sc, wx, wy, wz, rx, ry, rz;
        fu_back(src, u, v, dsrc, &sa, &sb, &sc);
        fu_apply(src + 4, sa, sb, sc, &wx, &wy, &wz);
        fu_apply(ref + 16, wx, wy, wz, &rx, &ry, &rz);
        if (!fu_pos_finite(rz)) continue;
        float xr, yr;
        fu_proj(ref, rx, ry, rz, &xr, &yr);
        const float ex = xr - x, ey = yr - y;
        const float e = sqrtf(fmaf(ey, ey, ex * ex));
        const float rel = fabsf(rz - d) / d;
        if (e < p.pix_thresh && rel < p.rel_thresh) {
            count += 1;
            sum = sum + rz;
        }
    }
    p.count[at] = (uint8_t)count;
    p.mask[at] = count >= p.min_views ? 1 : 0;
    p.fused[at] = sum / (float)(count + 1);
}

// ---------------------------------------------------------------------------------------------------------------- compaction
// Inclusive sum of `v` over the workgroup's threads in thread order; `total` = the workgroup's sum.  All FU_BLOCK threads; two barriers.
__device__ __forceinline__ int fu_block_scan(int v, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    __syncthreads();                                        // (the previous use of wave_sums is over)
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < FU_BLOCK / 64; ++w) {
        const int s = wave_sums[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return incl + before;
}

__device__ __forceinline__ int fu_mask4(const uint8_t* mask, long long i0, long long n, bool m[FU_PER]) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < FU_PER; ++k) {
        m[k] = i0 + k < n && mask[i0 + k] != 0;
        c += m[k] ? 1 : 0;
    }
    return c;
}

__global__ void __launch_bounds__(FU_BLOCK) pc_count_kernel(const uint8_t* mask, long long n, int* counts) {
    __shared__ int wave_sums[FU_BLOCK / 64];
    bool m[FU_PER];
    const long long i0 = (long long)blockIdx.x * FU_ITEMS + (long long)threadIdx.x * FU_PER;
    const int c = fu_mask4(mask, i0, n, m);
    int total;
    fu_block_scan(c, wave_sums, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(FU_BLOCK) pc_scan_kernel(int* counts, int n_blocks, long long* total_out) {
    __shared__ int wave_sums[FU_BLOCK / 64];
    long long carry = 0;                                    // (the same in every thread)
    for (int base = 0; base < n_blocks; base += FU_BLOCK) {
        const int i = base + threadIdx.x;
        const int c = i < n_blocks ? counts[i] : 0;
        int total;
        const int incl = fu_block_scan(c, wave_sums, &total);
        if (i < n_blocks) counts[i] = (int)(carry + (incl - c));                      // exclusive; below n < 2^31
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(FU_BLOCK) pc_scatter_kernel(ucnerf_points_compact_params p, long long n) {
    __shared__ int wave_sums[FU_BLOCK / 64];
    bool m[FU_PER];
    const long long i0 = (long long)blockIdx.x * FU_ITEMS + (long long)threadIdx.x * FU_PER;
    const int c = fu_mask4(p.mask, i0, n, m);
    int total;
    const int incl = fu_block_scan(c, wave_sums, &total);
    long long k = (long long)p.workspace[blockIdx.x] + (incl - c);
    const int HW = p.H * p.W;
#pragma unroll
    for (int j = 0; j < FU_PER; ++j) {
        if (!m[j]) continue;
        if (k < p.cap) {
            const long long i = i0 + j;
            const int view = (int)(i / HW);
            const int q = (int)(i - (long long)view * HW);
            const int yi = q / p.W, xi = q - yi * p.W;
            const float* K = p.intrinsics + (long long)view * 9;
            const float cam[4] = {K[0], K[2], K[4], K[5]};
            float a, b, cc, X, Y, Z;
            fu_back(cam, (float)xi, (float)yi, p.fused[i], &a, &b, &cc);
            fu_apply(p.c2ws + (long long)view * 16, a, b, cc, &X, &Y, &Z);
            p.points[3 * k] = X;
            p.points[3 * k + 1] = Y;
            p.points[3 * k + 2] = Z;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float v = p.rgb[((long long)view * 3 + ch) * HW + q];
                v = v != v ? 0.0f : fminf(fmaxf(v, 0.0f), 1.0f);
                p.colors[3 * k + ch] = (uint8_t)(v * 255.0f + 0.5f);
            }
        }
        ++k;
    }
}

static int fu_sizes(const char* what, int N, int H, int W, long long* n) {
    UCNERF_REQUIRE(N >= 0 && H >= 0 && W >= 0, "%s: N=%d H=%d W=%d (negative)", what, N, H, W);
    UCNERF_REQUIRE(H <= (1 << 24) && W <= (1 << 24), "%s: a %d x %d map (each side at most 2^24)", what, H, W);
    *n = (long long)N * H * W;
    UCNERF_REQUIRE(*n < (1ll << 31), "%s: N H W = %lld pixels, expected below 2^31", what, *n);
    return UCNERF_OK;
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_depth_consistency(const ucnerf_depth_consistency_params* p, void* stream) {
    UCNERF_REQUIRE(p, "depth_consistency: null params");
    long long n;
    if (int rc = fu_sizes("depth_consistency", p->N, p->H, p->W, &n)) return rc;
    UCNERF_REQUIRE(p->S >= 0, "depth_consistency: S = %d (negative)", p->S);
    UCNERF_REQUIRE(p->S <= FU_MAX_SRC, "depth_consistency: S = %d sources above %d", p->S, FU_MAX_SRC);
    if (n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->depth && p->intrinsics && p->c2ws, "depth_consistency: null input (depth, intrinsics or c2ws)");
    UCNERF_REQUIRE(p->src_ids || p->S == 0, "depth_consistency: null src_ids with S = %d", p->S);
    UCNERF_REQUIRE(p->count && p->mask && p->fused, "depth_consistency: null output (count, mask or fused)");
    UCNERF_REQUIRE((((uintptr_t)p->depth | (uintptr_t)p->intrinsics | (uintptr_t)p->c2ws | (uintptr_t)p->w2cs | (uintptr_t)p->src_ids | (uintptr_t)p->conf |
                     (uintptr_t)p->fused) & 3) == 0, "depth_consistency: the float and int32 arrays must be 4-byte aligned");
    const int bpv = cdiv((long long)p->H * p->W, FU_BLOCK);
    UCNERF_REQUIRE((long long)p->N * bpv < (1ll << 31), "depth_consistency: %lld workgroups", (long long)p->N * bpv);
    hipLaunchKernelGGL(depth_consistency_kernel, dim3(p->N * bpv), dim3(FU_BLOCK), 0, (hipStream_t)stream, *p, bpv);
    return check_launch("depth_consistency");
}

int64_t ucnerf_points_compact_workspace_bytes(int64_t n_pixels) {
    if (n_pixels < 0) { fail(UCNERF_EINVAL, "points_compact_workspace_bytes: negative count %lld", (long long)n_pixels); return -1; }
    return 4 * ((n_pixels + FU_ITEMS - 1) / FU_ITEMS);
}

int ucnerf_points_compact(const ucnerf_points_compact_params* p, void* stream) {
    UCNERF_REQUIRE(p, "points_compact: null params");
    long long n;
    if (int rc = fu_sizes("points_compact", p->N, p->H, p->W, &n)) return rc;
    UCNERF_REQUIRE(p->cap >= 0, "points_compact: cap = %lld (negative)", (long long)p->cap);
    UCNERF_REQUIRE(p->total && ((uintptr_t)p->total & 7) == 0, "points_compact: total must be a non-null, 8-byte aligned int64");
    if (n == 0) {
        hipError_t e = hipMemsetAsync(p->total, 0, 8, (hipStream_t)stream);
        return e == hipSuccess ? UCNERF_OK : fail(UCNERF_EHIP, "points_compact: %s", hipGetErrorString(e));
    }
    UCNERF_REQUIRE(p->fused && p->mask && p->rgb && p->intrinsics && p->c2ws, "points_compact: null input (fused, mask, rgb, intrinsics or c2ws)");
    UCNERF_REQUIRE(p->workspace && ((uintptr_t)p->workspace & 3) == 0, "points_compact: workspace must be non-null and 4-byte aligned");
    UCNERF_REQUIRE((p->points && p->colors) || p->cap == 0, "points_compact: null points or colors with cap = %lld", (long long)p->cap);
    UCNERF_REQUIRE((((uintptr_t)p->fused | (uintptr_t)p->rgb | (uintptr_t)p->intrinsics | (uintptr_t)p->c2ws | (uintptr_t)p->points) & 3) == 0,
                   "points_compact: the float arrays must be 4-byte aligned");
    const int blocks = cdiv(n, FU_ITEMS);
    hipLaunchKernelGGL(pc_count_kernel, dim3(blocks), dim3(FU_BLOCK), 0, (hipStream_t)stream, p->mask, n, p->workspace);
    hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(FU_BLOCK), 0, (hipStream_t)stream, p->workspace, blocks, (long long*)p->total);
    hipLaunchKernelGGL(pc_scatter_kernel, dim3(blocks), dim3(FU_BLOCK), 0, (hipStream_t)stream, *p, n);
    return check_launch("points_compact");
}

}  // extern "C"
