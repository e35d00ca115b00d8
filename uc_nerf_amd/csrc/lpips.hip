// e1, LPIPS (the `lpips` package, net='alex') on the device: the AlexNet feature stack -- a forward convolution with bias and ReLU as an implicit
// GEMM on v_mfma_f32_32x32x2_f32, a 3 x 3 / 2 max pool -- and the distance of one feature level.  Inference only, float32 throughout, the
// weights are the caller's.  No atomics anywhere: every output element is written by one lane, every sum has one fixed order, so two calls
// on the same input give the same bits, whatever the batch an image is part of.
//
// The convolution as a GEMM.  y[co][q] = sum_k w[co][k] x[k][q], k = (cin * K + ky) * K + kx (the flat index of a [Cout,Cin,K,K] weight's row),
// q = (image * OH + oy) * OW + ox over the whole batch.  A block of 4 waves owns 64 output channels x 64 pixels; wave (mh, nh) the 32 x 32
// tile (channels 32 mh .., pixels 32 nh ..): A = weights (row = channel), B = inputs (column = pixel), so an accumulator register holds 32
// consecutive pixels of one channel and is stored as one 128-byte segment.  k is walked in chunks of 32: the chunk's 32 x 64 weights (from
// the packed image, contiguous) and 32 x 64 input taps (gathered; a tap outside the image, a pixel past the batch, a k past Cin K K: +0) are
// loaded into registers while the previous chunk is multiplied, then stored to LDS.
//
// ACCUMULATION ORDER (fixed, part of the interface).  Within chunk j: S_j = fma chain over k = 32 j .. 32 j + 31 ascending from +0 (the MFMA
// is bit for bit an fmaf chain, two k per instruction, the lower first).  Over the chunks: T = (((0 + S_0) + S_1) + ...) in float32, ascending.
// y = T + bias, then max(y, 0) with relu.  The chunk sums bound the length of any one rounding chain to 32 + K_total / 32 (blocked summation)
// instead of K_total; a zero tap adds an exact +0 at either level.
#include "common.h"
#include "mfma_split.h"

namespace ucnerf {

constexpr int CV_BM = 64, CV_BN = 64, CV_KC = 32, CV_THREADS = 256;
constexpr int CV_ROW = 96;            // LDS row stride in floats: rows k and k + 1 (the two lane halves of one operand read) 32 banks apart
constexpr int CV_ROWS_PER_THREAD = CV_KC / (CV_THREADS / 64);
constexpr int CV_MAX_K = 11;
constexpr int LP_BLOCK = 1024, LP_WAVES = LP_BLOCK / 64;
constexpr int ALEX_MIN_SIDE = 31;

static inline int conv_kpad(long long ktot) { return (int)((ktot + CV_KC - 1) / CV_KC * CV_KC); }
static inline long long conv_packed_floats(int cin, int cout, int K) {
    const long long kp = conv_kpad((long long)cin * K * K);
    return (long long)cdiv(cout, CV_BM) * kp * CV_BM + kp;
}

// Packed image: [cout tile][k < Kpad][64 channels] weights (zero past Cout and past Cin K K), then Kpad int32 tap codes
// (cin << 8 | ky << 4 | kx; -1 past Cin K K): the order the kernel walks, no division in its loop.
__global__ void __launch_bounds__(256) conv_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int cin, int cout, int K, int kpad, long long nw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int ktot = cin * K * K;
    if (i < nw) {
        const int c = (int)(i % CV_BM), k = (int)((i / CV_BM) % kpad), mt = (int)(i / ((long long)CV_BM * kpad));
        const int co = mt * CV_BM + c;
        packed[i] = co < cout && k < ktot ? w[(size_t)co * ktot + k] : 0.f;
    } else if (i < nw + kpad) {
        const int k = (int)(i - nw);
        const int ci = k / (K * K), r = k % (K * K);
        reinterpret_cast<int*>(packed)[i] = k < ktot ? (ci << 8) | ((r / K) << 4) | (r % K) : -1;
    }
}

__global__ void __launch_bounds__(CV_THREADS) conv2d_kernel(ucnerf_conv2d_params p, int OH, int OW, int kpad, int npix) {
    __shared__ float sA[CV_KC * CV_ROW], sB[CV_KC * CV_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ohw = OH * OW, H = p.H, W = p.W;
    // ---- the fill: this thread's column (a channel of A, a pixel of B) and its 8 rows wave, wave + 4, ...
    const int q = blockIdx.x * CV_BN + lane;
    const bool q_in = q < npix;
    const int img = q_in ? q / ohw : 0, rem = q_in ? q % ohw : 0;
    const int iy0 = (rem / OW) * p.stride - p.pad, ix0 = (rem % OW) * p.stride - p.pad;
    const float* __restrict__ xin = p.x + (size_t)img * p.cin * H * W;
    const float* __restrict__ wsrc = p.packed + (size_t)blockIdx.y * kpad * CV_BM + lane;
    const int* __restrict__ ktab = reinterpret_cast<const int*>(p.packed + (size_t)gridDim.y * kpad * CV_BM);
    float ra[CV_ROWS_PER_THREAD], rb[CV_ROWS_PER_THREAD];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < CV_ROWS_PER_THREAD; ++j) {
            const int k = chunk * CV_KC + wave + 4 * j;                  // (< kpad: wave-uniform)
            ra[j] = wsrc[(size_t)k * CV_BM];
            const int e = ktab[k];
            float v = 0.f;
            if (e >= 0 && q_in) {
                const int ci = e >> 8, iy = iy0 + ((e >> 4) & 15), ix = ix0 + (e & 15);
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                    v = xin[((size_t)ci * H + iy) * W + ix];
                    if (p.shift) v = (v - p.shift[ci]) / p.scale[ci];     // the scaling layer, applied to what is inside the image only
                }
            }
            rb[j] = v;
        }
    };
    // ---- the product: wave (mh, nh)
    const int mh = wave & 1, nh = wave >> 1, l31 = lane & 31, half = lane >> 5;
    const float* a_at = sA + half * CV_ROW + mh * 32 + l31;
    const float* b_at = sB + half * CV_ROW + nh * 32 + l31;
    f32x16 total;
#pragma unroll
    for (int r = 0; r < 16; ++r) total[r] = 0.f;
    const int chunks = kpad / CV_KC;
    fetch(0);
    for (int c = 0; c < chunks; ++c) {
        __syncthreads();                                                 // the previous chunk has been read
#pragma unroll
        for (int j = 0; j < CV_ROWS_PER_THREAD; ++j) {
            sA[(wave + 4 * j) * CV_ROW + lane] = ra[j];
            sB[(wave + 4 * j) * CV_ROW + lane] = rb[j];
        }
        __syncthreads();
        if (c + 1 < chunks) fetch(c + 1);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int t = 0; t < CV_KC / 2; ++t) acc = mfma_32x32x2(a_at[2 * t * CV_ROW], b_at[2 * t * CV_ROW], acc);
        total += acc;
    }
    // ---- bias, ReLU, store: register r is channel row(r) of 32 consecutive pixels
    const int qs = blockIdx.x * CV_BN + nh * 32 + l31;
    if (qs >= npix) return;
    const int simg = qs / ohw, srem = qs % ohw;
    float* __restrict__ yout = p.y + (size_t)simg * p.cout * ohw + srem;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = blockIdx.y * CV_BM + mh * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (co < p.cout) {
            float v = total[r] + p.bias[co];
            if (p.relu) v = v > 0.f ? v : (v != v ? v : 0.f);           // torch.relu: a NaN stays
            yout[(size_t)co * ohw] = v;
        }
    }
}

// 3 x 3 window, stride 2, no pad, floor mode; one thread per output.  The first tap starts the maximum, so any float works (-inf
// included); a NaN in the window is the result, as in torch.
__global__ void __launch_bounds__(256) maxpool_kernel(ucnerf_maxpool2d_params p, int OH, int OW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const long long plane = i / ((long long)OW * OH);
    const float* __restrict__ x = p.x + (size_t)plane * p.H * p.W + (size_t)(2 * oy) * p.W + 2 * ox;
    float m = x[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float v = x[dy * p.W + dx];
            m = (v > m || v != v) ? v : m;
        }
    p.y[i] = m;
}

// One feature level of the distance, one block per image pair.  A pixel is owned by G lanes of one wave (G a power of two, chosen from h w
// alone: 1 for the large maps, up to 64 for a 1 x 1 map, so that a small map still fills the block); lane g of them takes the channels
// g, g + G, ... in ascending order.  A wave holds 64 / G consecutive pixels in its low lane bits, so a load is contiguous along the row.
// Per pixel two passes over the channels (the second comes from L2): the two norms, then d; each is the lanes' float32 partial sums folded by
// an xor butterfly (every lane gets the same bits, the order is fixed).  The sum over the pixels is carried in fp64 -- lane, wave (shuffle
// tree), the 16 waves in order -- and rounded once with the mean.
__device__ __forceinline__ float group_sum(float v, int first) {          // over the lanes that differ in the bits first, 2 first, ..., 32
    for (int s = first; s < 64; s <<= 1) v += __shfl_xor(v, s);
    return v;
}
__global__ void __launch_bounds__(LP_BLOCK) lpips_layer_kernel(ucnerf_lpips_layer_params p, int G) {
    __shared__ double ld[LP_WAVES];
    const int img = blockIdx.x, hw = p.h * p.w, C = p.C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, P = 64 / G, g = lane / P, pl = lane % P;
    const float* __restrict__ f0 = p.f0 + (size_t)img * C * hw;
    const float* __restrict__ f1 = p.f1 + (size_t)img * C * hw;
    double acc = 0.0;
    for (int q0 = wave * P; q0 < hw; q0 += LP_WAVES * P) {              // (uniform over the wave: the butterflies run with all 64 lanes)
        const int q = q0 + pl;
        const bool in = q < hw;
        float s0 = 0.f, s1 = 0.f;
        if (in)
            for (int c = g; c < C; c += G) {
                const float a = f0[(size_t)c * hw + q], b = f1[(size_t)c * hw + q];
                s0 += a * a;
                s1 += b * b;
            }
        s0 = group_sum(s0, P);
        s1 = group_sum(s1, P);
        const float r0 = sqrtf(s0) + 1e-10f, r1 = sqrtf(s1) + 1e-10f;
        float d = 0.f;
        if (in)
            for (int c = g; c < C; c += G) {
                const float u = f0[(size_t)c * hw + q] / r0 - f1[(size_t)c * hw + q] / r1;      // (an all-zero pixel: 0 / 1e-10 = 0)
                d += p.lin[c] * (u * u);
            }
        d = group_sum(d, P);
        if (g == 0 && in) acc += (double)d;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_down(acc, s);
    if (lane == 0) ld[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = ld[0];
#pragma unroll
        for (int w = 1; w < LP_WAVES; ++w) s += ld[w];
        const float mean = (float)(s / (double)hw);
        p.out[img] = p.accumulate ? p.out[img] + mean : mean;
    }
}
// lanes per pixel: the smallest power of two that brings h w G to 4096 (four pixels' worth of work per thread of the block), at most 64
static inline int layer_group(long long hw) {
    int G = 1;
    while (G < 64 && hw * G < 4096) G <<= 1;
    return G;
}

struct AlexDims { int o1h, o1w, p1h, p1w, p2h, p2w; };
static inline AlexDims alex_dims(int H, int W) {
    AlexDims d;
    d.o1h = (H + 4 - 11) / 4 + 1; d.o1w = (W + 4 - 11) / 4 + 1;
    d.p1h = (d.o1h - 3) / 2 + 1; d.p1w = (d.o1w - 3) / 2 + 1;
    d.p2h = (d.p1h - 3) / 2 + 1; d.p2w = (d.p1w - 3) / 2 + 1;
    return d;
}
constexpr int ALEX_C[5] = {64, 192, 384, 256, 256};
// workspace, in floats, for 2 n images: [f1][pool1][f2][pool2][f3][f4][f5]
struct AlexLayout { long long f[5], pool[2], total; };
static inline AlexLayout alex_layout(long long n, const AlexDims& d) {
    const long long m = 2 * n, s1 = (long long)d.o1h * d.o1w, s2 = (long long)d.p1h * d.p1w, s3 = (long long)d.p2h * d.p2w;
    AlexLayout L;
    long long at = 0;
    L.f[0] = at; at += m * 64 * s1;
    L.pool[0] = at; at += m * 64 * s2;
    L.f[1] = at; at += m * 192 * s2;
    L.pool[1] = at; at += m * 192 * s3;
    L.f[2] = at; at += m * 384 * s3;
    L.f[3] = at; at += m * 256 * s3;
    L.f[4] = at; at += m * 256 * s3;
    L.total = at;
    return L;
}

static int conv_check(const ucnerf_conv2d_params* p, const char* who) {
    UCNERF_REQUIRE(p->n >= 0, "%s: negative count %d", who, p->n);
    UCNERF_REQUIRE(p->cin >= 1 && p->cout >= 1 && p->H >= 1 && p->W >= 1, "%s: cin=%d cout=%d H=%d W=%d (all at least 1)", who, p->cin, p->cout, p->H, p->W);
    UCNERF_REQUIRE(p->K >= 1 && p->K <= CV_MAX_K, "%s: kernel size %d outside 1 .. %d", who, p->K, CV_MAX_K);
    UCNERF_REQUIRE(p->stride >= 1 && p->pad >= 0 && p->pad < (1 << 20), "%s: stride=%d pad=%d", who, p->stride, p->pad);
    UCNERF_REQUIRE(p->H + 2 * p->pad >= p->K && p->W + 2 * p->pad >= p->K, "%s: a %d x %d input with pad %d is smaller than the %d x %d kernel", who, p->H, p->W, p->pad, p->K, p->K);
    UCNERF_REQUIRE((long long)p->cin * p->K * p->K < (1ll << 22) && (long long)p->cin * p->H * p->W < (1ll << 31), "%s: cin K K = %lld or cin H W = %lld too large", who,
                   (long long)p->cin * p->K * p->K, (long long)p->cin * p->H * p->W);
    return UCNERF_OK;
}
static int conv_launch(const ucnerf_conv2d_params* p, hipStream_t st, const char* who) {
    if (int rc = conv_check(p, who)) return rc;
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->x && p->packed && p->bias && p->y, "%s: null x, packed, bias or y", who);
    UCNERF_REQUIRE((p->shift == nullptr) == (p->scale == nullptr), "%s: shift and scale must both be given or both NULL", who);
    const int OH = (p->H + 2 * p->pad - p->K) / p->stride + 1, OW = (p->W + 2 * p->pad - p->K) / p->stride + 1;
    const long long npix = (long long)p->n * OH * OW;
    UCNERF_REQUIRE(npix < (1ll << 31) - CV_BN, "%s: n OH OW = %lld output pixels (32-bit index)", who, npix);
    const int mt = cdiv(p->cout, CV_BM);
    UCNERF_REQUIRE(mt <= 65535, "%s: cout = %d above the grid limit", who, p->cout);
    hipLaunchKernelGGL(conv2d_kernel, dim3(cdiv(npix, CV_BN), mt), dim3(CV_THREADS), 0, st, *p, OH, OW, conv_kpad((long long)p->cin * p->K * p->K), (int)npix);
    return UCNERF_OK;
}
static int pool_launch(const ucnerf_maxpool2d_params* p, hipStream_t st, const char* who) {
    UCNERF_REQUIRE(p->planes >= 0, "%s: negative count %lld", who, (long long)p->planes);
    UCNERF_REQUIRE(p->H >= 3 && p->W >= 3, "%s: a %d x %d map is smaller than the 3 x 3 window", who, p->H, p->W);
    if (p->planes == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->x && p->y, "%s: null x or y", who);
    const int OH = (p->H - 3) / 2 + 1, OW = (p->W - 3) / 2 + 1;
    const long long total = (long long)p->planes * OH * OW;
    UCNERF_REQUIRE(total < (1ll << 38), "%s: %lld outputs (grid limit)", who, total);
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *p, OH, OW, total);
    return UCNERF_OK;
}
static int layer_launch(const ucnerf_lpips_layer_params* p, hipStream_t st, const char* who) {
    UCNERF_REQUIRE(p->n >= 0, "%s: negative count %d", who, p->n);
    UCNERF_REQUIRE(p->C >= 1 && p->h >= 1 && p->w >= 1 && (long long)p->C * p->h * p->w < (1ll << 31), "%s: C=%d h=%d w=%d", who, p->C, p->h, p->w);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->f0 && p->f1 && p->lin && p->out, "%s: null f0, f1, lin or out", who);
    hipLaunchKernelGGL(lpips_layer_kernel, dim3(p->n), dim3(LP_BLOCK), 0, st, *p, layer_group((long long)p->h * p->w));
    return UCNERF_OK;
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int64_t ucnerf_conv2d_packed_floats(int32_t cin, int32_t cout, int32_t K) {
    if (cin < 1 || cout < 1 || K < 1 || K > CV_MAX_K || (long long)cin * K * K >= (1ll << 22)) return fail(UCNERF_EINVAL, "conv2d_packed_floats: cin=%d cout=%d K=%d", cin, cout, K);
    return conv_packed_floats(cin, cout, K);
}

int ucnerf_conv2d_pack(const ucnerf_conv2d_pack_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv2d_pack: null params");
    UCNERF_REQUIRE(p->cin >= 1 && p->cout >= 1 && p->K >= 1 && p->K <= CV_MAX_K && (long long)p->cin * p->K * p->K < (1ll << 22), "conv2d_pack: cin=%d cout=%d K=%d (K at most %d)", p->cin, p->cout, p->K, CV_MAX_K);
    UCNERF_REQUIRE(p->weight && p->packed, "conv2d_pack: null weight or packed");
    const int kpad = conv_kpad((long long)p->cin * p->K * p->K);
    const long long nw = (long long)cdiv(p->cout, CV_BM) * kpad * CV_BM;
    hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)((nw + kpad + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->weight, p->packed, p->cin, p->cout, p->K, kpad, nw);
    return check_launch("conv2d_pack");
}

int ucnerf_conv2d_bias_relu(const ucnerf_conv2d_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv2d_bias_relu: null params");
    if (int rc = conv_launch(p, (hipStream_t)stream, "conv2d_bias_relu")) return rc;
    return p->n == 0 ? UCNERF_OK : check_launch("conv2d_bias_relu");
}

int ucnerf_maxpool2d(const ucnerf_maxpool2d_params* p, void* stream) {
    UCNERF_REQUIRE(p, "maxpool2d: null params");
    if (int rc = pool_launch(p, (hipStream_t)stream, "maxpool2d")) return rc;
    return p->planes == 0 ? UCNERF_OK : check_launch("maxpool2d");
}

int ucnerf_lpips_layer(const ucnerf_lpips_layer_params* p, void* stream) {
    UCNERF_REQUIRE(p, "lpips_layer: null params");
    if (int rc = layer_launch(p, (hipStream_t)stream, "lpips_layer")) return rc;
    return p->n == 0 ? UCNERF_OK : check_launch("lpips_layer");
}

int64_t ucnerf_lpips_workspace_floats(int32_t n, int32_t H, int32_t W) {
    if (n < 0) return fail(UCNERF_EINVAL, "lpips_workspace_floats: negative count %d", n);
    if (H < ALEX_MIN_SIDE || W < ALEX_MIN_SIDE) return fail(UCNERF_EINVAL, "lpips_workspace_floats: a %d x %d image is below the minimum side %d", H, W, ALEX_MIN_SIDE);
    return alex_layout(n, alex_dims(H, W)).total;
}

int ucnerf_lpips_alex(const ucnerf_lpips_alex_params* p, void* stream) {
    UCNERF_REQUIRE(p, "lpips_alex: null params");
    UCNERF_REQUIRE(p->n >= 0, "lpips_alex: negative count %d", p->n);
    UCNERF_REQUIRE(p->H >= ALEX_MIN_SIDE && p->W >= ALEX_MIN_SIDE, "lpips_alex: a %d x %d image is below the minimum side %d (the second pool needs a 3 x 3 map)", p->H, p->W, ALEX_MIN_SIDE);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->n <= (1 << 20), "lpips_alex: n = %d pairs above 2^20 (grid limit): call in chunks", p->n);
    UCNERF_REQUIRE(p->a && p->b && p->shift && p->scale && p->workspace && p->out, "lpips_alex: null a, b, shift, scale, workspace or out");
    for (int l = 0; l < 5; ++l) UCNERF_REQUIRE(p->packed[l] && p->bias[l] && p->lin[l], "lpips_alex: null packed, bias or lin of level %d", l);
    hipStream_t st = (hipStream_t)stream;
    const AlexDims d = alex_dims(p->H, p->W);
    const AlexLayout L = alex_layout(p->n, d);
    const int n = p->n, m = 2 * n;
    float* ws = p->workspace;
    int rc;
    // conv1 with the scaling layer in its operand load: once per image set, into the two halves of level 0
    for (int side = 0; side < 2; ++side) {
        ucnerf_conv2d_params c = {n, 3, p->H, p->W, 64, 11, 4, 2, 1, 0, side ? p->b : p->a, p->packed[0], p->bias[0], p->shift, p->scale,
                                  ws + L.f[0] + (long long)side * n * 64 * d.o1h * d.o1w};
        if ((rc = conv_launch(&c, st, "lpips_alex conv1"))) return rc;
    }
    ucnerf_maxpool2d_params q1 = {(int64_t)m * 64, d.o1h, d.o1w, ws + L.f[0], ws + L.pool[0]};
    if ((rc = pool_launch(&q1, st, "lpips_alex pool1"))) return rc;
    ucnerf_conv2d_params c2 = {m, 64, d.p1h, d.p1w, 192, 5, 1, 2, 1, 0, ws + L.pool[0], p->packed[1], p->bias[1], nullptr, nullptr, ws + L.f[1]};
    if ((rc = conv_launch(&c2, st, "lpips_alex conv2"))) return rc;
    ucnerf_maxpool2d_params q2 = {(int64_t)m * 192, d.p1h, d.p1w, ws + L.f[1], ws + L.pool[1]};
    if ((rc = pool_launch(&q2, st, "lpips_alex pool2"))) return rc;
    const float* in = ws + L.pool[1];
    for (int l = 2; l < 5; ++l) {
        ucnerf_conv2d_params c = {m, ALEX_C[l - 1], d.p2h, d.p2w, ALEX_C[l], 3, 1, 1, 1, 0, in, p->packed[l], p->bias[l], nullptr, nullptr, ws + L.f[l]};
        if ((rc = conv_launch(&c, st, "lpips_alex conv3-5"))) return rc;
        in = ws + L.f[l];
    }
    // the five levels in ascending order: out = d0, then out += d1 ... (one stream: each launch sees the previous one's value)
    const int lh[5] = {d.o1h, d.p1h, d.p2h, d.p2h, d.p2h}, lw[5] = {d.o1w, d.p1w, d.p2w, d.p2w, d.p2w};
    for (int l = 0; l < 5; ++l) {
        const long long half = (long long)n * ALEX_C[l] * lh[l] * lw[l];
        ucnerf_lpips_layer_params y = {n, ALEX_C[l], lh[l], lw[l], l > 0, 0, ws + L.f[l], ws + L.f[l] + half, p->lin[l], p->out};
        if ((rc = layer_launch(&y, st, "lpips_alex layer"))) return rc;
    }
    return check_launch("lpips_alex");
}

}  // extern "C"
