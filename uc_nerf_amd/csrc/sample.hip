// d1, one sample of the reference's dataset (data/scared.py:387-522, plus train.py:61-70's unpreprocess) out of a scene that is resident on the
// device: ONE launch per sample.  Everything constant per frame was computed on the host at load (uc_nerf_amd/data/scene.py); what is left is to
// pick V frames and normalise them, read the target's two pyramid levels through index maps, build the keypoint rows in the order of a
// permutation, and gather / pair the matrices.  Plain HIP C++, wave64, plain vector stores, no atomics, nothing read back.
//
// Arithmetic.  The build compiles with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt (uc_nerf_amd/build.py): every `a / b` below
// is an IEEE division, never a multiplication by a reciprocal, and (x - m) / s stays a subtraction followed by a division.  The bytes 0 .. 255 go
// through float(u) / 255.0f (ToTensor), - mean, / std (Normalize) and, when asked for, - unpre_mean, / unpre_std: up to five roundings, the ones
// torch makes on the host.  proj_mats is the one product formed here: fmaf over k = 0 .. 3 in ascending order from a first product.
//
// The grid is four runs of workgroups, each run one kind of work (a workgroup's kind is uniform):
//   images     V x ceil(ceil(H W / 4) / 256) workgroups.  A thread owns four consecutive pixels of one view: 12 bytes = three whole dwords in
//              (a wave reads 768 consecutive bytes), one float4 out per plane (a wave writes 1 KB consecutive per plane).  The last thread of an
//              image whose H W is no multiple of 4 reads only the dwords that hold its pixels and stores them one by one; so does every
//              thread when a plane is not 16-byte aligned.
//   pyramids   one thread per output position of level 1 and level 2, both maps.
//   rays_depth one thread per output float (n_rows x 9).
//   matrices   one workgroup: 152 floats per view.
// Latency-bound by design: at 256 x 320, V = 5 it moves 1.2 MB in and about 5 to 10 MB out.
#include "common.h"

#include <cmath>

namespace ucnerf {

constexpr int SA_BLOCK = 256;
constexpr int SA_PIX = 4;                                  // pixels per thread of the image part
constexpr int SA_PER_VIEW = 16 + 16 + 9 + 48 + 48 + 12 + 2 + 1;

struct SampleGrid { int img_per_view, img, pyr, rays; };  // workgroups of each run (matrices: one more)

__device__ __forceinline__ int sa_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ void sa_images(const ucnerf_sample_assemble_params& p, int v, int g, bool vec) {
    const int HW = p.H * p.W;
    const int q0 = g * SA_PIX;
    if (q0 >= HW) return;
    const int left = HW - q0;                                // pixels of this thread: 4, or 1 .. 3 at the end of an image
    const int f = p.view_ids[v];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p.frames + (long long)f * p.frame_stride) + 3 * g;
    uint32_t w[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = (12 * g + 4 * j < 3 * HW) ? src[j] : 0u;   // (a dword is read only where one of its bytes is a pixel's)
    float y[3][SA_PIX], z[3][SA_PIX];
#pragma unroll
    for (int k = 0; k < SA_PIX; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int b = 3 * k + c;
            const float u = (float)((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
            const float x = u / 255.0f;                      // ToTensor
            y[c][k] = (x - p.mean[c]) / p.std[c];            // Normalize: sub_ then div_
            z[c][k] = (y[c][k] - p.unpre_mean[c]) / p.unpre_std[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long at = ((long long)v * 3 + c) * HW + q0;
        if (vec && left >= SA_PIX) {
            *reinterpret_cast<float4*>(p.images + at) = make_float4(y[c][0], y[c][1], y[c][2], y[c][3]);
            if (p.images_unpre) *reinterpret_cast<float4*>(p.images_unpre + at) = make_float4(z[c][0], z[c][1], z[c][2], z[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < SA_PIX; ++k) {
                if (k < left) {
                    p.images[at + k] = y[c][k];
                    if (p.images_unpre) p.images_unpre[at + k] = z[c][k];
                }
            }
        }
    }
}

__device__ __forceinline__ void sa_pyramids(const ucnerf_sample_assemble_params& p, int i) {
    const int n1 = p.h1 * p.w1, n2 = p.h2 * p.w2;
    if (i >= n1 + n2) return;
    const bool first = i < n1;
    const int e = first ? i : i - n1, wd = first ? p.w1 : p.w2;
    const int y = e / wd, x = e - y * wd;
    // (the maps are the caller's: an index outside the image is clamped into it, so that nothing outside the resident arrays is ever read)
    const int r = sa_clampi((first ? p.row1 : p.row2)[y], p.H - 1), c = sa_clampi((first ? p.col1 : p.col2)[x], p.W - 1);
    const long long at = ((long long)p.view_ids[0] * p.H + r) * p.W + c;
    (first ? p.sd1 : p.sd2)[e] = p.depth_img[at];
    (first ? p.wt1 : p.wt2)[e] = p.weight_img[at];
}

__device__ __forceinline__ void sa_rays(const ucnerf_sample_assemble_params& p, int i) {
    if (i >= p.n_rows * 9) return;
    const int row = i / 9, j = i - row * 9;
    const int k = p.perm[row];
    float v = NAN;                                           // a perm entry outside the segment reads nothing
    if (k >= 0 && k < p.n_kp) {
        const int at = p.kp_first + k;
        v = j < 3 ? p.kp_depth[at] : (j < 6 ? p.kp_weight[at] : (j == 8 ? 1.0f : (float)p.kp_coord[2 * at + (j - 6)]));
    }
    p.rays_depth[i] = v;
}

__device__ __forceinline__ void sa_matrices(const ucnerf_sample_assemble_params& p) {
    const int tgt = p.view_ids[0];
    for (int i = threadIdx.x; i < p.V * SA_PER_VIEW; i += SA_BLOCK) {
        const int v = i / SA_PER_VIEW;
        int e = i - v * SA_PER_VIEW;
        const int f = p.view_ids[v];
        if (e < 16) { p.c2ws[v * 16 + e] = p.c2w[f * 16 + e]; continue; }
        e -= 16;
        if (e < 16) { p.w2cs[v * 16 + e] = p.w2c[f * 16 + e]; continue; }
        e -= 16;
        if (e < 9) { p.intrinsics[v * 9 + e] = p.intrinsic[f * 9 + e]; continue; }
        e -= 9;
        if (e < 48) { p.affine_mat[v * 48 + e] = p.affine[f * 48 + e]; continue; }
        e -= 48;
        if (e < 48) { p.affine_mat_inv[v * 48 + e] = p.affine_inv[f * 48 + e]; continue; }
        e -= 48;
        if (e < 12) {
            const int r = e >> 2, c = e & 3;
            float acc;
            if (v == 0) {
                acc = r == c ? 1.0f : 0.0f;
            } else {
                const float* a = p.affine + f * 48 + 32 + r * 4;        // row r of the finest stage's matrix
                const float* b = p.ref_proj_inv + tgt * 16 + c;         // column c
                acc = a[0] * b[0];
                acc = fmaf(a[1], b[4], acc);
                acc = fmaf(a[2], b[8], acc);
                acc = fmaf(a[3], b[12], acc);
            }
            p.proj_mats[v * 12 + e] = acc;
            continue;
        }
        e -= 12;
        if (e < 2) { p.near_fars[v * 2 + e] = p.near_far[e]; continue; }
        p.view_ids_out[v] = (long long)f;
    }
}

__global__ void __launch_bounds__(SA_BLOCK) sample_assemble_kernel(ucnerf_sample_assemble_params p, SampleGrid gr, int vec) {
    int b = blockIdx.x;
    if (b < gr.img) {
        const int v = b / gr.img_per_view;
        sa_images(p, v, (b - v * gr.img_per_view) * SA_BLOCK + threadIdx.x, vec != 0);
        return;
    }
    b -= gr.img;
    if (b < gr.pyr) { sa_pyramids(p, b * SA_BLOCK + threadIdx.x); return; }
    b -= gr.pyr;
    if (b < gr.rays) { sa_rays(p, b * SA_BLOCK + threadIdx.x); return; }
    sa_matrices(p);
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_sample_assemble(const ucnerf_sample_assemble_params* p, void* stream) {
    UCNERF_REQUIRE(p, "sample_assemble: null params");
    UCNERF_REQUIRE(p->N >= 0 && p->H >= 0 && p->W >= 0 && p->V >= 0 && p->h1 >= 0 && p->w1 >= 0 && p->h2 >= 0 && p->w2 >= 0 && p->frame_stride >= 0 &&
                   p->kp_total >= 0 && p->kp_first >= 0 && p->n_kp >= 0 && p->n_rows >= 0,
                   "sample_assemble: N=%d H=%d W=%d V=%d levels %dx%d %dx%d frame_stride=%d kp_total=%d kp_first=%d n_kp=%d n_rows=%d (negative)", p->N, p->H,
                   p->W, p->V, p->h1, p->w1, p->h2, p->w2, p->frame_stride, p->kp_total, p->kp_first, p->n_kp, p->n_rows);
    UCNERF_REQUIRE(p->V >= 1 && p->V <= 9, "sample_assemble: V = %d outside 1..9", p->V);
    UCNERF_REQUIRE(p->N >= 1 && p->N <= (1 << 20), "sample_assemble: N = %d frames outside 1..2^20", p->N);
    UCNERF_REQUIRE(p->H >= 1 && p->W >= 1 && (long long)p->H * p->W <= (1 << 24), "sample_assemble: a %d x %d image (1 .. 2^24 pixels)", p->H, p->W);
    const long long HW = (long long)p->H * p->W;
    UCNERF_REQUIRE(p->h1 <= p->H && p->w1 <= p->W && p->h2 <= p->H && p->w2 <= p->W, "sample_assemble: a pyramid level (%d x %d, %d x %d) larger than the %d x %d image",
                   p->h1, p->w1, p->h2, p->w2, p->H, p->W);
    UCNERF_REQUIRE((p->frame_stride & 3) == 0 && p->frame_stride >= 3 * HW, "sample_assemble: frame_stride = %d must be a multiple of 4 and at least 3 H W = %lld",
                   p->frame_stride, 3 * HW);
    for (int v = 0; v < p->V; ++v)
        UCNERF_REQUIRE(p->view_ids[v] >= 0 && p->view_ids[v] < p->N, "sample_assemble: view_ids[%d] = %d outside 0..%d", v, p->view_ids[v], p->N - 1);
    UCNERF_REQUIRE(p->n_rows <= 1024 && p->n_rows <= p->n_kp, "sample_assemble: n_rows = %d above 1024 or above n_kp = %d", p->n_rows, p->n_kp);
    UCNERF_REQUIRE((long long)p->kp_first + p->n_kp <= p->kp_total, "sample_assemble: keypoints %d .. + %d overrun the %d of the scene", p->kp_first, p->n_kp, p->kp_total);
    UCNERF_REQUIRE(p->frames && p->depth_img && p->weight_img && p->c2w && p->w2c && p->intrinsic && p->affine && p->affine_inv && p->ref_proj_inv,
                   "sample_assemble: null resident array (frames, depth_img, weight_img, c2w, w2c, intrinsic, affine, affine_inv or ref_proj_inv)");
    UCNERF_REQUIRE((p->h1 * p->w1 == 0 || (p->row1 && p->col1 && p->sd1 && p->wt1)) && (p->h2 * p->w2 == 0 || (p->row2 && p->col2 && p->sd2 && p->wt2)),
                   "sample_assemble: null index map or pyramid output");
    UCNERF_REQUIRE(p->n_rows == 0 || (p->kp_depth && p->kp_weight && p->kp_coord && p->perm && p->rays_depth), "sample_assemble: null kp_depth, kp_weight, kp_coord, perm or rays_depth");
    UCNERF_REQUIRE(p->images && p->c2ws && p->w2cs && p->intrinsics && p->affine_mat && p->affine_mat_inv && p->proj_mats && p->near_fars && p->view_ids_out,
                   "sample_assemble: null output (images, c2ws, w2cs, intrinsics, affine_mat, affine_mat_inv, proj_mats, near_fars or view_ids_out)");
    UCNERF_REQUIRE(((uintptr_t)p->frames & 3) == 0, "sample_assemble: frames must be 4-byte aligned (its bytes are read as dwords)");
    UCNERF_REQUIRE((((uintptr_t)p->images | (uintptr_t)p->images_unpre) & 3) == 0 && ((uintptr_t)p->view_ids_out & 7) == 0,
                   "sample_assemble: images / images_unpre must be 4-byte aligned, view_ids_out 8-byte aligned");
    const int vec = (HW & 3) == 0 && (((uintptr_t)p->images | (uintptr_t)p->images_unpre) & 15) == 0;
    SampleGrid gr;
    gr.img_per_view = cdiv(cdiv(HW, SA_PIX), SA_BLOCK);
    gr.img = p->V * gr.img_per_view;
    gr.pyr = cdiv((long long)p->h1 * p->w1 + (long long)p->h2 * p->w2, SA_BLOCK);
    gr.rays = cdiv((long long)p->n_rows * 9, SA_BLOCK);
    hipLaunchKernelGGL(sample_assemble_kernel, dim3(gr.img + gr.pyr + gr.rays + 1), dim3(SA_BLOCK), 0, (hipStream_t)stream, *p, gr, vec);
    return check_launch("sample_assemble");
}

}  // extern "C"
