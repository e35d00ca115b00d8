// The weight gradient of the 3-D convolutions of csrc/conv3d.hip (include/ucnerf_hip.h, "ucnerf_conv3d_wgrad"): float32, NCDHW, K = 3.  Exact
// float32 products and sums on v_mfma_f32_16x16x4_f32; no atomics, every element of the workspace and of the result is written by one lane with a
// plain vector store, every sum has one fixed order: two calls give the same bits.
//
// Both forms are one computation over a SMALL grid (sd, sh, sw) and a BIG one:  out[a][b][t] = sum over (img, s) of
// A[img,a,s] * B[img,b, stride * s - pad + t], t = (td, th, tw) the 27 taps, a tap outside the big grid contributing +0.
//   forward form     A = grad_y [n,cout,OD,OH,OW], B = x [n,cin,D,H,W], stride and pad the layer's: out = grad_weight [cout,cin,27]
//   transposed form  A = x [n,cin,D,H,W], B = grad_y [n,cout,2D,2H,2W], stride 2, pad 1:        out = grad_weight [cin,cout,27]
//
// As a GEMM the voxels v = img * S + s are the REDUCTION dimension (1 280 .. 655 360 of them at the network's shapes) and the output is small
// (Ca x 27 Cb), so the voxel range is cut into chunks (split-K): block (chunk, a tile, b group) multiplies 16 channels of A with 16 channels x 27
// taps of B over its chunk and stores the partial to the workspace; a second launch folds the partials in ascending chunk order.
//
// The forward's trick of loading the MFMA operands straight from global memory needs 16 consecutive voxels per lane group; here the lanes of an
// operand run over CHANNELS (A[row = lane & 15][k = lane >> 4]), which are a whole volume apart.  So both operands go through LDS: 32 voxels
// at a time, every thread owns ONE voxel of the 32 (its 27-bit tap mask and base offsets are made once) and writes that voxel's column of
// As[16][32] and of the im2col image Bs[16 b][27 t][32]: the global loads run along consecutive voxels (coalesced; stride 2 reads every other
// float), an element of B is read 27 times from L1 / L2 and once from HBM.  Rows are 36 floats apart: 36 l and 27 * 36 l (mod 64 banks) are
// distinct multiples of 4 for l = 0 .. 15, so the MFMA's reads (lane l & 15 a channel, lane >> 4 one of 4 voxels) hit 64 different banks.
// Wave w owns the taps t = w, w + 4, ...: 7 (6 for wave 3) independent accumulator chains.
//
// SUMMATION ORDER (fixed, part of the interface; the header states it in full).  Within a chunk one fmaf chain from +0 over ascending voxel v
// (the MFMA adds four voxels per instruction, the lowest first); over the chunks (((+0 + P_0) + P_1) + ...) ascending.
#include "common.h"
#include "mfma_split.h"

#include <cstdint>

namespace ucnerf {
namespace {

constexpr int WG_THREADS = 256, WG_SUB = 32, WG_ROW = 36, WG_TAPS = 27;
constexpr int WG_TARGET_BLOCKS = 512;                    // two blocks of 63 KiB LDS per CU on 256 CUs
constexpr int WG_TILES_PER_WAVE = 7;                     // ceil(27 / 4)
constexpr int WG_MAX_C = 1 << 16;

struct WgGeom {
    int Ca, Cb, SD, SH, SW, BD, BH, BW, stride, pad;
    int V, L, chunks;                                    // voxels n S, chunk length (a multiple of 32), number of chunks
};

__device__ __forceinline__ unsigned wg_axis_bits(int base, int size) {
    unsigned m = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) m |= (unsigned)(base + d >= 0 && base + d < size) << d;
    return m;
}

__global__ void __launch_bounds__(WG_THREADS) conv3d_wgrad_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ ws, WgGeom g) {
    __shared__ float As[16 * WG_ROW];
    __shared__ float Bs[16 * WG_TAPS * WG_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, kq = lane >> 4;
    const int vi = tid & (WG_SUB - 1), grp = tid >> 5;                   // this thread's voxel of the 32, and which of 8 channels it stages
    const int a0 = blockIdx.y * 16, b0 = blockIdx.z * 16;
    const int begin = blockIdx.x * g.L, end = min(begin + g.L, g.V);     // (blockIdx.x < chunks: begin < V)
    const int S = g.SD * g.SH * g.SW;
    const long long BDHW = (long long)g.BD * g.BH * g.BW;
    f32x4 acc[WG_TILES_PER_WAVE];
#pragma unroll
    for (int i = 0; i < WG_TILES_PER_WAVE; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int sub = begin; sub < end; sub += WG_SUB) {
        const int v = sub + vi;
        unsigned mask = 0;
        long long aoff = 0, boff = 0;
        const bool live = v < end;
        if (live) {
            const int img = v / S, s = v - img * S;
            const int sw = s % g.SW, sh = (s / g.SW) % g.SH, sd = s / (g.SW * g.SH);
            const int bd = sd * g.stride - g.pad, bh = sh * g.stride - g.pad, bw = sw * g.stride - g.pad;
            const unsigned md = wg_axis_bits(bd, g.BD), mh = wg_axis_bits(bh, g.BH), mw = wg_axis_bits(bw, g.BW);
#pragma unroll
            for (int dd = 0; dd < 3; ++dd)
#pragma unroll
                for (int dh = 0; dh < 3; ++dh)
                    if ((md >> dd & 1) && (mh >> dh & 1)) mask |= mw << (9 * dd + 3 * dh);
            aoff = (long long)img * g.Ca * S + s;
            boff = (long long)img * g.Cb * BDHW + ((long long)bd * g.BH + bh) * g.BW + bw;   // (may lie before the image: read only where a bit is set)
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int a = grp + 8 * i;
            As[a * WG_ROW + vi] = (live && a0 + a < g.Ca) ? A[aoff + (long long)(a0 + a) * S] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < 2 * WG_TAPS; ++it) {
            const int t = it >> 1, b = (it & 1) * 8 + grp;
            const int td = t / 9, th = (t / 3) % 3, tw = t % 3;
            const bool on = (mask >> t & 1) && b0 + b < g.Cb;
            Bs[(b * WG_TAPS + t) * WG_ROW + vi] = on ? B[boff + (long long)(b0 + b) * BDHW + ((long long)td * g.BH + th) * g.BW + tw] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WG_SUB / 4; ++j) {
            const float a = As[l15 * WG_ROW + 4 * j + kq];
#pragma unroll
            for (int i = 0; i < WG_TILES_PER_WAVE; ++i) {
                const int t = wave + 4 * i;
                if (t < WG_TAPS) acc[i] = mfma_16x16x4(a, Bs[(l15 * WG_TAPS + t) * WG_ROW + 4 * j + kq], acc[i]);    // (t: uniform over the wave)
            }
        }
        __syncthreads();
    }
    // register r of tile i: row a0 + 4 (lane >> 4) + r, column b0 + (lane & 15), tap wave + 4 i.  workspace [chunk][a][t][b]
#pragma unroll
    for (int i = 0; i < WG_TILES_PER_WAVE; ++i) {
        const int t = wave + 4 * i, b = b0 + l15;
        if (t >= WG_TAPS || b >= g.Cb) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * kq + r;
            if (a < g.Ca) ws[(((size_t)blockIdx.x * g.Ca + a) * WG_TAPS + t) * g.Cb + b] = acc[i][r];
        }
    }
}

// one thread per element, in the workspace's order [a][t][b]; out is [a][b][t]
__global__ void __launch_bounds__(256) conv3d_wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ out, int Ca, int Cb, int chunks) {
    const int total = Ca * WG_TAPS * Cb;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int b = e % Cb, t = (e / Cb) % WG_TAPS, a = e / (Cb * WG_TAPS);
    float sum = 0.f;
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {                    // eight loads in flight, added in ascending order
        float p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = ws[(size_t)(c + u) * total + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += p[u];
    }
    for (; c < chunks; ++c) sum += ws[(size_t)c * total + e];
    out[((size_t)a * Cb + b) * WG_TAPS + t] = sum;
}

// the checks every caller shares and the geometry; `n` may be 0 (then g->V == 0 and nothing is launched)
int wg_geometry(const char* who, int n, int cin, int cout, int D, int H, int W, int K, int stride, int pad, int transposed, WgGeom* g) {
    UCNERF_REQUIRE(n >= 0, "%s: negative count %d", who, n);
    UCNERF_REQUIRE(cin >= 1 && cout >= 1 && cin <= WG_MAX_C && cout <= WG_MAX_C, "%s: cin=%d cout=%d (1 .. %d)", who, cin, cout, WG_MAX_C);
    UCNERF_REQUIRE(D >= 1 && H >= 1 && W >= 1, "%s: D=%d H=%d W=%d (all at least 1)", who, D, H, W);
    UCNERF_REQUIRE(transposed == 0 || transposed == 1, "%s: transposed=%d (0 or 1)", who, transposed);
    UCNERF_REQUIRE(K == 3, "%s: K=%d (the weight gradient is built for K = 3 only)", who, K);
    if (transposed) {
        UCNERF_REQUIRE(stride == 2 && pad == 1, "%s: the transposed form is K=3 stride=2 pad=1 output_padding=1 only, got stride=%d pad=%d", who, stride, pad);
        UCNERF_REQUIRE(D < (1 << 29) && H < (1 << 29) && W < (1 << 29), "%s: D H W too large", who);
        g->Ca = cin; g->Cb = cout;
        g->SD = D; g->SH = H; g->SW = W;
        g->BD = 2 * D; g->BH = 2 * H; g->BW = 2 * W;
    } else {
        UCNERF_REQUIRE((stride == 1 || stride == 2) && pad >= 0 && pad <= 64, "%s: stride=%d pad=%d (stride 1 or 2, pad 0 .. 64)", who, stride, pad);
        UCNERF_REQUIRE(D + 2 * pad >= 3 && H + 2 * pad >= 3 && W + 2 * pad >= 3, "%s: a %d x %d x %d input with pad %d is smaller than the kernel 3", who, D, H, W, pad);
        g->Ca = cout; g->Cb = cin;
        g->SD = (D + 2 * pad - 3) / stride + 1; g->SH = (H + 2 * pad - 3) / stride + 1; g->SW = (W + 2 * pad - 3) / stride + 1;
        g->BD = D; g->BH = H; g->BW = W;
    }
    g->stride = stride; g->pad = pad;
    const long long S = (long long)g->SD * g->SH * g->SW, big = (long long)g->BD * g->BH * g->BW, V = (long long)n * S;
    UCNERF_REQUIRE(S < (1ll << 31) && (long long)g->Ca * S < (1ll << 31) && (long long)g->Cb * big < (1ll << 31) && V < (1ll << 31) - 1024,
                   "%s: a tensor of %lld or %lld floats per image or %lld voxels is too large (32-bit index)", who, (long long)g->Ca * S, (long long)g->Cb * big, V);
    UCNERF_REQUIRE((long long)g->Ca * g->Cb * WG_TAPS < (1ll << 31), "%s: cin cout 27 = %lld is too large (32-bit index)", who, (long long)g->Ca * g->Cb * WG_TAPS);
    g->V = (int)V;
    const long long tiles = (long long)cdiv(g->Ca, 16) * cdiv(g->Cb, 16);
    long long c0 = (WG_TARGET_BLOCKS + tiles - 1) / tiles, most = (V + WG_SUB - 1) / WG_SUB;
    if (c0 > most) c0 = most;
    if (c0 < 1) c0 = 1;
    g->L = (int)((V + WG_SUB * c0 - 1) / (WG_SUB * c0)) * WG_SUB;
    if (g->L < WG_SUB) g->L = WG_SUB;
    g->chunks = V == 0 ? 0 : (int)((V + g->L - 1) / g->L);
    return UCNERF_OK;
}

}  // namespace
}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int64_t ucnerf_conv3d_wgrad_workspace_floats(int32_t n, int32_t cin, int32_t cout, int32_t D, int32_t H, int32_t W, int32_t K, int32_t stride, int32_t pad,
                                             int32_t transposed) {
    WgGeom g;
    if (int rc = wg_geometry("conv3d_wgrad_workspace_floats", n, cin, cout, D, H, W, K, stride, pad, transposed, &g)) return rc;
    return (int64_t)g.chunks * g.Ca * g.Cb * WG_TAPS;
}

int ucnerf_conv3d_wgrad(const ucnerf_conv3d_wgrad_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv3d_wgrad: null params");
    WgGeom g;
    if (int rc = wg_geometry("conv3d_wgrad", p->n, p->cin, p->cout, p->D, p->H, p->W, p->K, p->stride, p->pad, p->transposed, &g)) return rc;
    const int64_t want = (int64_t)g.chunks * g.Ca * g.Cb * WG_TAPS;
    UCNERF_REQUIRE(p->workspace_floats == want, "conv3d_wgrad: the workspace holds %lld floats, this call writes %lld (ucnerf_conv3d_wgrad_workspace_floats)",
                   (long long)p->workspace_floats, (long long)want);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->x && p->grad_y && p->workspace && p->grad_weight, "conv3d_wgrad: null x, grad_y, workspace or grad_weight");
    const float* A = p->transposed ? p->x : p->grad_y;
    const float* B = p->transposed ? p->grad_y : p->x;
    hipLaunchKernelGGL(conv3d_wgrad_kernel, dim3((unsigned)g.chunks, (unsigned)cdiv(g.Ca, 16), (unsigned)cdiv(g.Cb, 16)), dim3(WG_THREADS), 0, (hipStream_t)stream, A, B,
                       p->workspace, g);
    if (int rc = check_launch("conv3d_wgrad")) return rc;
    const int total = g.Ca * g.Cb * WG_TAPS;
    hipLaunchKernelGGL(conv3d_wgrad_fold_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, p->workspace, p->grad_weight, g.Ca, g.Cb, g.chunks);
    return check_launch("conv3d_wgrad fold");
}

}  // extern "C"
