// d3, the input side of a FREE camera pose: the batch `ucnerf_sample_assemble` (sample.hip) gives for a dataset frame, for a pose that is no frame
// of the dataset: ONE launch per novel frame.  The target's matrices are formed here in closed form from the pose, the V - 1 source views are
// picked on the device (formats.get_nearest_pose_ids, 'dist' criterion) and never visit the host, their images are normalised with sample.hip's
// own expression and their matrices copied bit for bit.  Plain HIP C++, wave64, plain vector loads and stores, no atomics, no global scratch,
// nothing read back.
//
// Arithmetic (the build compiles with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt: every fmaf below is written out, every
// `a / b` is an IEEE division).  With the pose [R | t] (row-major [3,4]) and K = intrinsic (zero skew ASSUMED: K[0][1], K[1][0] and the last row
// are read only where the general product reads them, the closed-form inverse reads fx, fy, cx, cy alone):
//   w2c[r][c]        = R[c][r];   w2c[r][3] = -fmaf(R[2][r], t[2], fmaf(R[1][r], t[1], R[0][r] * t[0]))        (rigid inverse [R^T | -R^T t])
//   K_s              = K with rows 0 and 1 divided by 2^(2 - s) (exact)
//   affine[s][r][c]  = fmaf(K_s[r][2], w2c[2][c], fmaf(K_s[r][1], w2c[1][c], K_s[r][0] * w2c[0][c])),  r < 3;  row 3 = 0 0 0 1
//   affine_inv[s]    = c2w . diag(K_s^-1, 1):  [r][0] = R[r][0] / fx_s,  [r][1] = R[r][1] / fy_s,
//                      [r][2] = fmaf(-R[r][1], cy_s / fy_s, fmaf(-R[r][0], cx_s / fx_s, R[r][2])),  [r][3] = t[r];  row 3 = 0 0 0 1
//   proj_mats[v]     = (affine[f_v][2] @ affine_inv[0][2])[:3] in sample.hip's order: fmaf over k = 0 .. 3 ascending from a first product
// None of these is an LU inverse: a rotation block that is not orthonormal gives what the formulas give.
//
// Selection.  d_k = |c2w[cand[k]][:3,3] - t|^2 in float32: dx * dx, then fmaf(dy, dy, .), then fmaf(dz, dz, .).  The V - 1 smallest in ascending
// order, equal distances by the lower position k, a NaN distance after every number (by position).  Every workgroup that needs the ids computes
// them itself (as ucnerf_bn_apply's workgroups fold the slices themselves): its threads write the n_cand <= 4096 distances to LDS, a strided
// share each, and after one barrier every thread makes the same single pass over them, the V - 1 best kept sorted in registers.  A cand entry
// outside 0 .. N-1 (the list is on the device: the host cannot check it) is clamped into that range, so nothing outside the resident arrays is read.
//
// The grid is V x ceil(ceil(H W / 4) / 256) image workgroups (those of slot 0 store zeros: a free pose has no ground truth) and one for the
// matrices.  Latency-bound by construction: at 256 x 320 it reads (V - 1) x 245 KB and writes V x 0.98 MB per image tensor.
#include "common.h"

#include <cmath>

namespace ucnerf {

constexpr int NV_BLOCK = 256;
constexpr int NV_PIX = 4;                                  // pixels per thread of the image part
constexpr int NV_MAX_CAND = 4096;
constexpr int NV_MAX_SRC = 8;                              // V - 1 <= 8
constexpr int NV_PER_VIEW = 16 + 16 + 9 + 48 + 48 + 12 + 2 + 1;

__device__ __forceinline__ int nv_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The frame ids of the V - 1 nearest candidates, ascending, into ids[0 .. V-2] (every thread of the workgroup gets the same ones).
__device__ __forceinline__ void nv_select(const ucnerf_novel_assemble_params& p, float* dist, int ids[NV_MAX_SRC]) {
    const float* t = p.poses + (long long)p.pose_index * 12;
    const float tx = t[3], ty = t[7], tz = t[11];
    for (int k = threadIdx.x; k < p.n_cand; k += NV_BLOCK) {
        const float* c = p.c2w + (long long)nv_clampi(p.cand[k], p.N - 1) * 16;
        const float dx = c[3] - tx, dy = c[7] - ty, dz = c[11] - tz;
        float d = dx * dx;
        d = fmaf(dy, dy, d);
        d = fmaf(dz, dz, d);
        dist[k] = d;
    }
    __syncthreads();
    float bd[NV_MAX_SRC];
    int bk[NV_MAX_SRC];
#pragma unroll
    for (int s = 0; s < NV_MAX_SRC; ++s) { bd[s] = 0.0f; bk[s] = -1; }
    const int n_src = p.V - 1;
    for (int k = 0; k < p.n_cand; ++k) {
        float cd = dist[k];
        int ck = k;
        bool shift = false;                                  // once k is placed, what it displaced moves down whatever it compares to
#pragma unroll
        for (int s = 0; s < NV_MAX_SRC; ++s) {
            if (s < n_src) {
                // strictly before the slot's entry: an empty slot, or a number below a larger number or a NaN (equal, or NaN against NaN: k stays behind)
                const bool take = shift || bk[s] < 0 || (!std::isnan(cd) && (std::isnan(bd[s]) || cd < bd[s]));
                if (take) {
                    const float od = bd[s];
                    const int ok = bk[s];
                    bd[s] = cd; bk[s] = ck;
                    cd = od; ck = ok;
                    shift = true;
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NV_MAX_SRC; ++s) ids[s] = (s < n_src && bk[s] >= 0) ? nv_clampi(p.cand[bk[s]], p.N - 1) : 0;
}

// The image part: sample.hip's sa_images on frame f (the same expressions: ToTensor's division, Normalize's sub then div, unpreprocess's).
__device__ __forceinline__ void nv_images(const ucnerf_novel_assemble_params& p, int v, int f, int g, bool vec) {
    const int HW = p.H * p.W;
    const int q0 = g * NV_PIX;
    if (q0 >= HW) return;
    const int left = HW - q0;                                // pixels of this thread: 4, or 1 .. 3 at the end of an image
    float y[3][NV_PIX], z[3][NV_PIX];
    if (v == 0) {
#pragma unroll
        for (int k = 0; k < NV_PIX; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c][k] = z[c][k] = 0.0f;
    } else {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.frames + (long long)f * p.frame_stride) + 3 * g;
        uint32_t w[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) w[j] = (12 * g + 4 * j < 3 * HW) ? src[j] : 0u;   // (a dword is read only where one of its bytes is a pixel's)
#pragma unroll
        for (int k = 0; k < NV_PIX; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = 3 * k + c;
                const float u = (float)((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
                const float x = u / 255.0f;                      // ToTensor
                y[c][k] = (x - p.mean[c]) / p.std[c];            // Normalize: sub_ then div_
                z[c][k] = (y[c][k] - p.unpre_mean[c]) / p.unpre_std[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long at = ((long long)v * 3 + c) * HW + q0;
        if (vec && left >= NV_PIX) {
            *reinterpret_cast<float4*>(p.images + at) = make_float4(y[c][0], y[c][1], y[c][2], y[c][3]);
            if (p.images_unpre) *reinterpret_cast<float4*>(p.images_unpre + at) = make_float4(z[c][0], z[c][1], z[c][2], z[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < NV_PIX; ++k) {
                if (k < left) {
                    p.images[at + k] = y[c][k];
                    if (p.images_unpre) p.images_unpre[at + k] = z[c][k];
                }
            }
        }
    }
}

// The target's matrices, one entry at a time from the pose (row-major [3,4]) and K (row-major [3,3]); see the head of the file for the orders.
__device__ __forceinline__ float nv_c2w(const float* pose, int r, int c) { return r < 3 ? pose[r * 4 + c] : (c == 3 ? 1.0f : 0.0f); }

__device__ __forceinline__ float nv_w2c(const float* pose, int r, int c) {
    if (r == 3) return c == 3 ? 1.0f : 0.0f;
    if (c < 3) return pose[c * 4 + r];
    float acc = pose[r] * pose[3];
    acc = fmaf(pose[4 + r], pose[7], acc);
    acc = fmaf(pose[8 + r], pose[11], acc);
    return -acc;
}

__device__ __forceinline__ float nv_stage_k(const float* K, int s, int r, int c) {
    return r < 2 ? K[r * 3 + c] / (float)(1 << (2 - s)) : K[r * 3 + c];
}

__device__ __forceinline__ float nv_affine(const float* pose, const float* K, int s, int r, int c) {
    if (r == 3) return c == 3 ? 1.0f : 0.0f;
    float acc = nv_stage_k(K, s, r, 0) * nv_w2c(pose, 0, c);
    acc = fmaf(nv_stage_k(K, s, r, 1), nv_w2c(pose, 1, c), acc);
    acc = fmaf(nv_stage_k(K, s, r, 2), nv_w2c(pose, 2, c), acc);
    return acc;
}

__device__ __forceinline__ float nv_affine_inv(const float* pose, const float* K, int s, int r, int c) {
    if (r == 3) return c == 3 ? 1.0f : 0.0f;
    if (c == 3) return pose[r * 4 + 3];
    const float fx = nv_stage_k(K, s, 0, 0), fy = nv_stage_k(K, s, 1, 1);
    if (c == 0) return pose[r * 4] / fx;
    if (c == 1) return pose[r * 4 + 1] / fy;
    const float ix = nv_stage_k(K, s, 0, 2) / fx, iy = nv_stage_k(K, s, 1, 2) / fy;
    float acc = fmaf(-pose[r * 4], ix, pose[r * 4 + 2]);
    acc = fmaf(-pose[r * 4 + 1], iy, acc);
    return acc;
}

__device__ __forceinline__ void nv_matrices(const ucnerf_novel_assemble_params& p, const int ids[NV_MAX_SRC]) {
    const float* pose = p.poses + (long long)p.pose_index * 12;
    const float* K = p.intrinsic_in ? p.intrinsic_in : p.intrinsic;        // (NULL: frame 0's resident intrinsic)
    for (int i = threadIdx.x; i < p.V * NV_PER_VIEW; i += NV_BLOCK) {
        const int v = i / NV_PER_VIEW;
        int e = i - v * NV_PER_VIEW;
        int f = 0;
#pragma unroll
        for (int s = 0; s < NV_MAX_SRC; ++s)
            if (s == v - 1) f = ids[s];
        if (e < 16) { p.c2ws[v * 16 + e] = v ? p.c2w[f * 16 + e] : nv_c2w(pose, e >> 2, e & 3); continue; }
        e -= 16;
        if (e < 16) { p.w2cs[v * 16 + e] = v ? p.w2c[f * 16 + e] : nv_w2c(pose, e >> 2, e & 3); continue; }
        e -= 16;
        if (e < 9) { p.intrinsics[v * 9 + e] = v ? p.intrinsic[f * 9 + e] : K[e]; continue; }
        e -= 9;
        if (e < 48) { p.affine_mat[v * 48 + e] = v ? p.affine[f * 48 + e] : nv_affine(pose, K, e >> 4, (e >> 2) & 3, e & 3); continue; }
        e -= 48;
        if (e < 48) { p.affine_mat_inv[v * 48 + e] = v ? p.affine_inv[f * 48 + e] : nv_affine_inv(pose, K, e >> 4, (e >> 2) & 3, e & 3); continue; }
        e -= 48;
        if (e < 12) {
            const int r = e >> 2, c = e & 3;
            float acc;
            if (v == 0) {
                acc = r == c ? 1.0f : 0.0f;
            } else {
                const float* a = p.affine + f * 48 + 32 + r * 4;        // row r of the finest stage's matrix
                acc = a[0] * nv_affine_inv(pose, K, 2, 0, c);           // column c of the target's finest-stage inverse
                acc = fmaf(a[1], nv_affine_inv(pose, K, 2, 1, c), acc);
                acc = fmaf(a[2], nv_affine_inv(pose, K, 2, 2, c), acc);
                acc = fmaf(a[3], nv_affine_inv(pose, K, 2, 3, c), acc);
            }
            p.proj_mats[v * 12 + e] = acc;
            continue;
        }
        e -= 12;
        if (e < 2) { p.near_fars[v * 2 + e] = p.near_far[e]; continue; }
        p.view_ids_out[v] = v ? (long long)f : -1ll;
    }
}

__global__ void __launch_bounds__(NV_BLOCK) novel_assemble_kernel(ucnerf_novel_assemble_params p, int img_per_view, int vec) {
    __shared__ float dist[NV_MAX_CAND];
    const int b = blockIdx.x;
    const int v = b / img_per_view;                          // == V for the matrices' workgroup
    int ids[NV_MAX_SRC];
    if (v == 0) {                                            // slot 0: zeros, no ids needed (uniform over the workgroup: no barrier is skipped by part of it)
        nv_images(p, 0, 0, b * NV_BLOCK + threadIdx.x, vec != 0);
        return;
    }
    nv_select(p, dist, ids);
    if (v >= p.V) { nv_matrices(p, ids); return; }
    int f = 0;
#pragma unroll
    for (int s = 0; s < NV_MAX_SRC; ++s)
        if (s == v - 1) f = ids[s];
    nv_images(p, v, f, (b - v * img_per_view) * NV_BLOCK + threadIdx.x, vec != 0);
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_novel_assemble(const ucnerf_novel_assemble_params* p, void* stream) {
    UCNERF_REQUIRE(p, "novel_assemble: null params");
    UCNERF_REQUIRE(p->N >= 0 && p->H >= 0 && p->W >= 0 && p->V >= 0 && p->frame_stride >= 0 && p->P >= 0 && p->n_cand >= 0,
                   "novel_assemble: N=%d H=%d W=%d V=%d frame_stride=%d P=%d n_cand=%d (negative)", p->N, p->H, p->W, p->V, p->frame_stride, p->P, p->n_cand);
    UCNERF_REQUIRE(p->V >= 2 && p->V <= 9, "novel_assemble: V = %d outside 2..9", p->V);
    UCNERF_REQUIRE(p->P >= 1, "novel_assemble: P = %d poses (at least one)", p->P);
    UCNERF_REQUIRE(p->pose_index >= 0 && p->pose_index < p->P, "novel_assemble: pose_index = %d outside 0..%d", p->pose_index, p->P - 1);
    UCNERF_REQUIRE(p->n_cand >= p->V, "novel_assemble: n_cand = %d candidates below V = %d", p->n_cand, p->V);
    UCNERF_REQUIRE(p->n_cand <= NV_MAX_CAND, "novel_assemble: n_cand = %d candidates above %d", p->n_cand, NV_MAX_CAND);
    UCNERF_REQUIRE(p->N >= 1 && p->N <= (1 << 20), "novel_assemble: N = %d frames outside 1..2^20", p->N);
    UCNERF_REQUIRE(p->H >= 1 && p->W >= 1 && (long long)p->H * p->W <= (1 << 24), "novel_assemble: a %d x %d image (1 .. 2^24 pixels)", p->H, p->W);
    const long long HW = (long long)p->H * p->W;
    UCNERF_REQUIRE((p->frame_stride & 3) == 0 && p->frame_stride >= 3 * HW, "novel_assemble: frame_stride = %d must be a multiple of 4 and at least 3 H W = %lld",
                   p->frame_stride, 3 * HW);
    UCNERF_REQUIRE(p->frames && p->c2w && p->w2c && p->intrinsic && p->affine && p->affine_inv,
                   "novel_assemble: null resident array (frames, c2w, w2c, intrinsic, affine or affine_inv)");
    UCNERF_REQUIRE(p->poses && p->cand, "novel_assemble: null poses or cand");
    UCNERF_REQUIRE(p->images && p->c2ws && p->w2cs && p->intrinsics && p->affine_mat && p->affine_mat_inv && p->proj_mats && p->near_fars && p->view_ids_out,
                   "novel_assemble: null output (images, c2ws, w2cs, intrinsics, affine_mat, affine_mat_inv, proj_mats, near_fars or view_ids_out)");
    UCNERF_REQUIRE(((uintptr_t)p->frames & 3) == 0, "novel_assemble: frames must be 4-byte aligned (its bytes are read as dwords)");
    UCNERF_REQUIRE((((uintptr_t)p->poses | (uintptr_t)p->cand | (uintptr_t)p->intrinsic_in) & 3) == 0, "novel_assemble: poses, cand and intrinsic_in must be 4-byte aligned");
    UCNERF_REQUIRE((((uintptr_t)p->images | (uintptr_t)p->images_unpre) & 3) == 0 && ((uintptr_t)p->view_ids_out & 7) == 0,
                   "novel_assemble: images / images_unpre must be 4-byte aligned, view_ids_out 8-byte aligned");
    const int vec = (HW & 3) == 0 && (((uintptr_t)p->images | (uintptr_t)p->images_unpre) & 15) == 0;
    const int img_per_view = cdiv(cdiv(HW, NV_PIX), NV_BLOCK);
    hipLaunchKernelGGL(novel_assemble_kernel, dim3(p->V * img_per_view + 1), dim3(NV_BLOCK), 0, (hipStream_t)stream, *p, img_per_view, vec);
    return check_launch("novel_assemble");
}

}  // extern "C"
