// The backward of FeatureNet's 2-D convolutions (include/ucnerf_hip.h, "Training FeatureNet on the device"): the weight gradient
// ucnerf_conv2d_wgrad, the input gradient of the stride-2 layers ucnerf_conv2d_dgrad_s2 and the bias gradient ucnerf_conv2d_bias_grad.
// float32, NCHW.  No atomics, every element of every result is written by one lane with a plain vector store, every sum has one fixed order:
// two calls give the same bits.
//
// WEIGHT GRADIENT.  As a GEMM: rows = cout (A = grad_y), columns = the flat (ci, ky, kx) of the weight itself (B = the taps of x), and the
// output pixels v = (img OH + oy) OW + ox are the REDUCTION dimension.  They are cut into chunks of whole output rows (split-K); block (chunk,
// 32 output channels, a group of CG input channels) multiplies over its chunk and stores its partial to the workspace, a second launch folds the
// partials in ascending chunk order.
// A chunk is walked in rounds: RR whole output rows of one image (or, where a row has more than 128 pixels, a segment of at most 128 pixels of
// one row).  A round's input footprint is a halo window: (RR - 1) stride + K rows by stride (pixels - 1) + K columns per channel.  It is staged
// in LDS ONCE, zeros where it leaves the image, and all K^2 taps are formed from LDS offsets: column c = (ci, ky, kx) of pixel (r, j) is
// Xs[ci][r stride + ky][j stride + kx].  A 3-channel layer is 27 columns (two 16-column tiles), not 9 tiles of 3-in-16.  grad_y's round is
// staged as As[32][pixels], rows 132 floats apart: 132 l (mod 64 banks) are the multiples of 4, so the MFMA's reads (lane & 15 a channel,
// lane >> 4 one of 4 pixels) hit 64 different banks.  Wave w owns the column tiles w, w + 4, ..., for both 16-row tiles.
//
// SUMMATION ORDER (fixed, part of the interface; the header states it in full).  Within a chunk one fmaf chain from +0 over ascending v (the MFMA
// adds four pixels per instruction, the lowest first; a row's pixel count is padded to a multiple of 4 with products +0 * +0, which change no
// bit of a chain that starts at +0); over the chunks (((+0 + P_0) + P_1) + ...) ascending.
//
// INPUT GRADIENT, stride 2.  One thread per input pixel and input channel, blocks by parity class (the taps ky = py, py + 2, ... that reach
// the pixel), the weight read through uniform addresses; the blocked order of the forward kernel (runs of 32, each an fmaf chain from +0,
// run sums added ascending) in plain fmaf.  grad_y is re-read by the cin blocks from L2; the layer's two instances are 1 % of its step.
#include "common.h"
#include "mfma_split.h"

#include <cstdint>

namespace ucnerf {
namespace {

constexpr int W2_THREADS = 256, W2_SLOTS = 128, W2_AROW = 132, W2_XS_FLOATS = 11264, W2_COLS = 256, W2_BM = 32;
constexpr int W2_TARGET_BLOCKS = 512;                    // two blocks of 60 KiB LDS per CU on 256 CUs
constexpr int W2_TPW = 4;                                // column tiles per wave: 16 tiles of 16 columns
constexpr int W2_MAX_C = 1 << 16;

struct W2Geom {
    int n, cin, cout, H, W, K, stride, pad, OH, OW;
    int SW, RR, CG, WP, WR;                              // segment slots, rows per round, channels per group, window pitch and rows
    int G, RC, chunks;                                   // global rows n OH, rows per chunk, number of chunks
};

__global__ void __launch_bounds__(W2_THREADS) conv2d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ ws, W2Geom g) {
    __shared__ float As[W2_BM * W2_AROW];
    __shared__ float Xs[W2_XS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, kq = lane >> 4;
    const int K = g.K, KK = K * K, stride = g.stride;
    const int co0 = blockIdx.y * W2_BM, cg0 = blockIdx.z * g.CG;
    const int CGc = min(g.CG, g.cin - cg0), cols = CGc * KK;             // this block's channels and columns
    const int ntiles = (cols + 15) >> 4;
    const int row_begin = blockIdx.x * g.RC, row_end = min(row_begin + g.RC, g.G);
    const int chan = g.WR * g.WP;                                        // floats of one channel's window
    // the LDS offset of this lane's column in each of the wave's tiles (a column past the block's: 0, multiplied and never stored)
    int coloff[W2_TPW];
#pragma unroll
    for (int i = 0; i < W2_TPW; ++i) {
        const int c = (wave + 4 * i) * 16 + l15;
        const int ci = c / KK, t = c - ci * KK, ky = t / K, kx = t - ky * K;
        coloff[i] = c < cols ? ci * chan + ky * g.WP + kx : 0;
    }
    f32x4 acc[2][W2_TPW];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < W2_TPW; ++i) acc[m][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool two = co0 + 16 < g.cout;                                  // (uniform) the second 16-row tile holds a channel
    const size_t plane_y = (size_t)g.OH * g.OW, plane_x = (size_t)g.H * g.W;
    for (int row = row_begin; row < row_end;) {
        const int img = row / g.OH, oy0 = row - img * g.OH;
        const int rr = min(min(g.RR, row_end - row), g.OH - oy0);        // rows of this round: one image, one chunk
        for (int seg0 = 0; seg0 < g.OW; seg0 += g.SW) {
            const int valid = min(g.SW, g.OW - seg0), sw = (valid + 3) & ~3;     // pixels of a row in this round, and padded to fours
            const int wr = (rr - 1) * stride + K, wp = stride * (sw - 1) + K;    // the window that is read
            // ---- grad_y: As[co][r sw + j], zero past cout and past the row
            {
                const int s = tid & (W2_SLOTS - 1), r = s / sw, j = s - r * sw;
                const bool on = r < rr && j < valid;
                const float* src = gy + ((size_t)img * g.cout * g.OH + (oy0 + r)) * g.OW + seg0 + j;
#pragma unroll 4
                for (int c = tid >> 7; c < W2_BM; c += 2)
                    As[c * W2_AROW + s] = (on && co0 + c < g.cout) ? src[(size_t)(co0 + c) * plane_y] : 0.f;
            }
            // ---- x: the halo window, Xs[ci][window row][window column], zero outside the image
            {
                const int iy0 = oy0 * stride - g.pad, ix0 = seg0 * stride - g.pad;
                const float* src = x + ((size_t)img * g.cin + cg0) * plane_x;
                for (int q = wave; q < CGc * wr; q += 4) {                       // (uniform over the wave)
                    const int ci = q / wr, r = q - ci * wr, iy = iy0 + r;
                    const bool row_in = iy >= 0 && iy < g.H;
                    for (int j = lane; j < wp; j += 64) {
                        const int ix = ix0 + j;
                        Xs[ci * chan + r * g.WP + j] = (row_in && ix >= 0 && ix < g.W) ? src[(size_t)ci * plane_x + (size_t)iy * g.W + ix] : 0.f;
                    }
                }
            }
            __syncthreads();
            // ---- the product: pixels ascending, four per instruction
            for (int r = 0; r < rr; ++r) {
                const float* a_at = As + l15 * W2_AROW + r * sw + kq;
                const float* b_at = Xs + r * stride * g.WP + kq * stride;
                for (int j = 0; j < sw; j += 4) {
                    const bool in = j + kq < valid;                              // a slot past the row's end: +0 * +0
                    const float a0 = a_at[j], a1 = two ? a_at[16 * W2_AROW + j] : 0.f;
#pragma unroll
                    for (int i = 0; i < W2_TPW; ++i) {
                        if (wave + 4 * i < ntiles) {                             // (uniform over the wave)
                            const float b = in ? b_at[coloff[i] + j * stride] : 0.f;
                            acc[0][i] = mfma_16x16x4(a0, b, acc[0][i]);
                            if (two) acc[1][i] = mfma_16x16x4(a1, b, acc[1][i]);
                        }
                    }
                }
            }
            __syncthreads();
        }
        row += rr;
    }
    // register r of tile (m, i): channel co0 + 16 m + 4 (lane >> 4) + r, column 16 (wave + 4 i) + (lane & 15).  workspace [chunk][cout][cin K K]
    const int ktot = g.cin * KK;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < W2_TPW; ++i) {
            const int c = (wave + 4 * i) * 16 + l15;
            if (c >= cols) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + 16 * m + 4 * kq + r;
                if (co < g.cout) ws[((size_t)blockIdx.x * g.cout + co) * ktot + (size_t)cg0 * KK + c] = acc[m][i][r];
            }
        }
}

// one thread per element of grad_weight
__global__ void __launch_bounds__(256) conv2d_wgrad_fold_kernel(const float* __restrict__ ws, float* __restrict__ out, int total, int chunks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
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
    out[e] = sum;
}

// the checks every caller shares and the geometry; `n` may be 0 (then chunks == 0 and nothing is launched)
int w2_geometry(const char* who, int n, int cin, int cout, int H, int W, int K, int stride, int pad, W2Geom* g) {
    UCNERF_REQUIRE(n >= 0, "%s: negative count %d", who, n);
    UCNERF_REQUIRE(cin >= 1 && cout >= 1 && cin <= W2_MAX_C && cout <= W2_MAX_C, "%s: cin=%d cout=%d (1 .. %d)", who, cin, cout, W2_MAX_C);
    UCNERF_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d (both at least 1)", who, H, W);
    UCNERF_REQUIRE(K == 1 || K == 3 || K == 5, "%s: K=%d (1, 3 or 5)", who, K);
    UCNERF_REQUIRE(pad == (K - 1) / 2, "%s: pad=%d (the layers' own (K - 1) / 2 = %d)", who, pad, (K - 1) / 2);
    UCNERF_REQUIRE(stride == 1 || (stride == 2 && K > 1), "%s: stride=%d with K=%d (stride 1, or 2 with K 3 or 5)", who, stride, K);
    const int OH = (H + 2 * pad - K) / stride + 1, OW = (W + 2 * pad - K) / stride + 1;
    const long long G = (long long)n * OH;
    UCNERF_REQUIRE((long long)n * cin * H * W < (1ll << 31) && (long long)n * cout * OH * OW < (1ll << 31) && G < (1ll << 31) - 1024,
                   "%s: x of %lld or grad_y of %lld floats is too large (32-bit index)", who, (long long)n * cin * H * W, (long long)n * cout * OH * OW);
    UCNERF_REQUIRE((long long)cin * cout * K * K < (1ll << 31), "%s: cin cout K K = %lld is too large (32-bit index)", who, (long long)cin * cout * K * K);
    g->n = n; g->cin = cin; g->cout = cout; g->H = H; g->W = W; g->K = K; g->stride = stride; g->pad = pad; g->OH = OH; g->OW = OW;
    const int OW4 = (OW + 3) & ~3;
    g->SW = OW4 < W2_SLOTS ? OW4 : W2_SLOTS;
    g->WP = stride * (g->SW - 1) + K;
    const int cg_most = cin < W2_COLS / (K * K) ? cin : W2_COLS / (K * K);
    g->RR = 1;
    if (OW4 <= W2_SLOTS)
        for (int r = W2_SLOTS / OW4; r > 1; --r)
            if ((long long)cg_most * ((r - 1) * stride + K) * g->WP <= W2_XS_FLOATS) { g->RR = r; break; }
    g->WR = (g->RR - 1) * stride + K;
    const int fit = W2_XS_FLOATS / (g->WR * g->WP);      // (at least 8: a window of one channel is at most 5 x 259 floats)
    g->CG = cg_most < fit ? cg_most : fit;
    const long long tiles = (long long)cdiv(cout, W2_BM) * cdiv(cin, g->CG);
    UCNERF_REQUIRE(cdiv(cout, W2_BM) <= 65535 && cdiv(cin, g->CG) <= 65535, "%s: cin=%d cout=%d above the grid limit", who, cin, cout);
    long long c0 = (W2_TARGET_BLOCKS + tiles - 1) / tiles, most = (G + g->RR - 1) / g->RR;
    if (c0 > most) c0 = most;
    if (c0 < 1) c0 = 1;
    g->G = (int)G;
    g->RC = (int)((G + g->RR * c0 - 1) / (g->RR * c0)) * g->RR;
    if (g->RC < g->RR) g->RC = g->RR;
    g->chunks = G == 0 ? 0 : (int)((G + g->RC - 1) / g->RC);
    return UCNERF_OK;
}

// ------------------------------------------------------------------------------------------------ the stride-2 input gradient
constexpr int DG_THREADS = 256, DG_RUN = 32;

// grid (tiles of 256 class pixels, 4 n, cin): block y = 4 img + 2 ry + rx, (ry, rx) the parities of iy and ix
__global__ void __launch_bounds__(DG_THREADS) conv2d_dgrad_s2_kernel(const float* __restrict__ gy, const float* __restrict__ w, float* __restrict__ gx,
                                                                     int cin, int cout, int H, int W, int K) {
    const int OH = H >> 1, OW = W >> 1, pad = (K - 1) >> 1;
    const int q = blockIdx.x * DG_THREADS + threadIdx.x;                 // the pixel of the class: (q / OW, q % OW)
    if (q >= OH * OW) return;
    const int img = blockIdx.y >> 2, ry = (blockIdx.y >> 1) & 1, rx = blockIdx.y & 1, ci = blockIdx.z;
    const int qy = q / OW, qx = q - qy * OW, iy = 2 * qy + ry, ix = 2 * qx + rx;
    const int py = (ry + pad) & 1, px = (rx + pad) & 1;                  // the class's first tap: ky = py + 2 jy reaches iy
    const int nky = (K - py + 1) >> 1, nkx = (K - px + 1) >> 1;
    const int by = (iy + pad - py) >> 1, bx = (ix + pad - px) >> 1;      // the source of tap (jy, jx): (by - jy, bx - jx)
    const float* __restrict__ src = gy + (size_t)img * cout * OH * OW;
    float total = 0.f, run = 0.f;
    int in_run = 0;
    for (int co = 0; co < cout; ++co) {
        const float* __restrict__ wk = w + ((size_t)co * cin + ci) * K * K;
        for (int jy = 0; jy < nky; ++jy) {
            const int oy = by - jy;
            const bool row_in = oy >= 0 && oy < OH;
            for (int jx = 0; jx < nkx; ++jx) {
                const int ox = bx - jx;
                const float v = (row_in && ox >= 0 && ox < OW) ? src[((size_t)co * OH + oy) * OW + ox] : 0.f;
                run = fmaf(v, wk[(py + 2 * jy) * K + px + 2 * jx], run);
                if (++in_run == DG_RUN) {                                // (uniform)
                    total += run;
                    run = 0.f;
                    in_run = 0;
                }
            }
        }
    }
    if (in_run) total += run;
    gx[(((size_t)img * cin + ci) * H + iy) * W + ix] = total;
}

// ------------------------------------------------------------------------------------------------ the bias gradient
constexpr int BG_THREADS = 1024;

// one block per channel; thread t adds, image after image, the pixels s = t, t + 1024, ... ascending in float64 from 0, then the threads' sums
// fold pairwise: for d = 512, 256, .. 1 thread t < d adds thread t + d's
__global__ void __launch_bounds__(BG_THREADS) conv2d_bias_grad_kernel(const float* __restrict__ gy, float* __restrict__ gb, int n, int cout, int S) {
    __shared__ double part[BG_THREADS];
    const int co = blockIdx.x, t = threadIdx.x;
    double sum = 0.0;
    for (int img = 0; img < n; ++img) {
        const float* __restrict__ src = gy + ((size_t)img * cout + co) * S;
        for (int s = t; s < S; s += BG_THREADS) sum += (double)src[s];
    }
    part[t] = sum;
    __syncthreads();
    for (int d = BG_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) part[t] += part[t + d];
        __syncthreads();
    }
    if (t == 0) gb[co] = (float)part[0];
}

}  // namespace
}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int64_t ucnerf_conv2d_wgrad_workspace_floats(int32_t n, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t K, int32_t stride, int32_t pad) {
    W2Geom g;
    if (int rc = w2_geometry("conv2d_wgrad_workspace_floats", n, cin, cout, H, W, K, stride, pad, &g)) return rc;
    return (int64_t)g.chunks * cout * cin * K * K;
}

int ucnerf_conv2d_wgrad(const ucnerf_conv2d_wgrad_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv2d_wgrad: null params");
    W2Geom g;
    if (int rc = w2_geometry("conv2d_wgrad", p->n, p->cin, p->cout, p->H, p->W, p->K, p->stride, p->pad, &g)) return rc;
    const int total = p->cout * p->cin * p->K * p->K;
    const int64_t want = (int64_t)g.chunks * total;
    UCNERF_REQUIRE(p->workspace_floats == want, "conv2d_wgrad: the workspace holds %lld floats, this call writes %lld (ucnerf_conv2d_wgrad_workspace_floats)",
                   (long long)p->workspace_floats, (long long)want);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->x && p->grad_y && p->workspace && p->grad_weight, "conv2d_wgrad: null x, grad_y, workspace or grad_weight");
    hipLaunchKernelGGL(conv2d_wgrad_kernel, dim3((unsigned)g.chunks, (unsigned)cdiv(g.cout, W2_BM), (unsigned)cdiv(g.cin, g.CG)), dim3(W2_THREADS), 0, (hipStream_t)stream,
                       p->x, p->grad_y, p->workspace, g);
    if (int rc = check_launch("conv2d_wgrad")) return rc;
    hipLaunchKernelGGL(conv2d_wgrad_fold_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, p->workspace, p->grad_weight, total, g.chunks);
    return check_launch("conv2d_wgrad fold");
}

int ucnerf_conv2d_dgrad_s2(const ucnerf_conv2d_dgrad_s2_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv2d_dgrad_s2: null params");
    UCNERF_REQUIRE(p->n >= 0, "conv2d_dgrad_s2: negative count %d", p->n);
    UCNERF_REQUIRE(p->cin >= 1 && p->cout >= 1 && p->cin <= 65535, "conv2d_dgrad_s2: cin=%d cout=%d (at least 1, cin at most 65535)", p->cin, p->cout);
    UCNERF_REQUIRE(p->H >= 1 && p->W >= 1, "conv2d_dgrad_s2: H=%d W=%d (both at least 1)", p->H, p->W);
    UCNERF_REQUIRE(p->K == 3 || p->K == 5, "conv2d_dgrad_s2: K=%d (3 or 5, pad (K - 1) / 2, stride 2)", p->K);
    UCNERF_REQUIRE(p->H % 2 == 0 && p->W % 2 == 0, "conv2d_dgrad_s2: H=%d W=%d must be even (an odd size needs output_padding 0, which is not built)", p->H, p->W);
    UCNERF_REQUIRE((long long)p->n * p->cin * p->H * p->W < (1ll << 31) && (long long)p->n * p->cout * (p->H / 2) * (p->W / 2) < (1ll << 31) && p->n <= 16383
                       && (long long)p->cin * p->cout * p->K * p->K < (1ll << 31),
                   "conv2d_dgrad_s2: n=%d, grad_x of %lld floats or the weight is too large (32-bit index, n at most 16383)", p->n, (long long)p->n * p->cin * p->H * p->W);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->grad_y && p->weight && p->grad_x, "conv2d_dgrad_s2: null grad_y, weight or grad_x");
    const int cls = (p->H / 2) * (p->W / 2);
    hipLaunchKernelGGL(conv2d_dgrad_s2_kernel, dim3((unsigned)cdiv(cls, DG_THREADS), (unsigned)(4 * p->n), (unsigned)p->cin), dim3(DG_THREADS), 0, (hipStream_t)stream,
                       p->grad_y, p->weight, p->grad_x, p->cin, p->cout, p->H, p->W, p->K);
    return check_launch("conv2d_dgrad_s2");
}

int ucnerf_conv2d_bias_grad(const ucnerf_conv2d_bias_grad_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv2d_bias_grad: null params");
    UCNERF_REQUIRE(p->n >= 0, "conv2d_bias_grad: negative count %d", p->n);
    UCNERF_REQUIRE(p->cout >= 1 && p->OH >= 1 && p->OW >= 1, "conv2d_bias_grad: cout=%d OH=%d OW=%d (all at least 1)", p->cout, p->OH, p->OW);
    UCNERF_REQUIRE((long long)p->n * p->cout * p->OH * p->OW < (1ll << 31), "conv2d_bias_grad: grad_y of %lld floats is too large (32-bit index)",
                   (long long)p->n * p->cout * p->OH * p->OW);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->grad_y && p->grad_bias, "conv2d_bias_grad: null grad_y or grad_bias");
    hipLaunchKernelGGL(conv2d_bias_grad_kernel, dim3((unsigned)p->cout), dim3(BG_THREADS), 0, (hipStream_t)stream, p->grad_y, p->grad_bias, p->n, p->cout, p->OH * p->OW);
    return check_launch("conv2d_bias_grad");
}

}  // extern "C"
