// e2, the 3-D convolutions of CasMVSNet's cost regularisation (network/mvs_models.py: Conv3d, Deconv3d, CostRegNet): forward only, float32, NCDHW
// in and out, y = act(conv(x) + bias[co]) (+ skip), act = ReLU or the identity, skip added AFTER the activation.  Exact float32 products and sums
// on v_mfma_f32_16x16x4_f32; no atomics, every output element is written by one lane and every sum has one fixed order, so two calls give the
// same bits and an image's result does not depend on the batch it is in.
//
// The convolution as a GEMM, without LDS.  y[co][q] = sum_k w[co][k] x[k][q] over the output voxels q.  The 16x16x4 MFMA takes ONE float of A and
// of B per lane (lane l: A[row l & 15][k = l >> 4], B[k = l >> 4][column l & 15]), so a lane loads exactly the operands it multiplies: its weight
// from the packed image (64 consecutive floats per wave and step) and its input tap straight from x (16 consecutive voxels for each of 4 taps).
// A wave owns MT x NT tiles of 16 channels x 16 voxels (cout <= 16: 1 x 4, a 16-row tile over 64 voxels; above: 2 x 2, a 32-row tile over 32
// voxels), a block 4 waves' worth of consecutive voxels, blockIdx.y the channel tile.  The MT NT accumulators are independent chains (the
// instruction's dependent latency is 40 cycles at a 32-cycle issue).  Channels are padded to the tile: cout = 8 multiplies 16 rows (2 x), never more.
//
// A tap is (ci, dd, dh, dw): the input voxel base + (dd, dh, dw) of channel ci, base = voxel * stride - pad.  Whether base + d lies inside the
// volume is one bit of a 27-bit word per voxel (bit 9 dd + 3 dh + dw), made once before the loop; a tap outside contributes +0, as does a k past
// the end (its code names bit 31, which is never set).
//
// The transposed form (K 3, stride 2, pad 1, output_padding 1: the output is 2 D x 2 H x 2 W) never multiplies the zeros of the upsampling.
// out[o] = sum x[i] w[k] over o = 2 i - 1 + k: an even o takes k = 1 alone (i = o / 2), an odd o takes k = 0 (i = (o + 1) / 2) and k = 2
// (i = (o - 1) / 2).  The output voxels are split into 8 parity classes (od & 1, oh & 1, ow & 1) = blockIdx.z; a block's voxels share a class and
// walk its 1, 2, 4 or 8 live taps only; class c has its own packed image (k = ci * taps + t, t over the live (kd, kh, kw) ascending).  Within a
// class the voxel q = the input-sized index (j d, j h, j w), o = 2 j + parity, and a live tap reads j + d with d = 1 for k = 0 and d = 0 otherwise.
//
// ACCUMULATION ORDER (fixed, part of the interface).  k = (ci * taps + t), t = (kd K + kh) K + kw for the forward form (the flat index of a
// [cout,cin,K,K,K] weight's row), the live taps in that same order for a class of the transposed form.  Within the j-th run of 32 consecutive k:
// S_j = the fma chain over ascending k from +0 (the MFMA is an fmaf chain, four k per instruction, the lowest first).  Over the runs:
// T = (((+0 + S_0) + S_1) + ...) ascending.  y = T + bias; with relu, y > 0 ? y : +0 (a NaN stays); then y + skip.  The cout = 1 layer (`prob`)
// runs the same order as a VALU kernel, one thread per voxel (a 16-row tile would multiply 15 rows of zeros).
#include "common.h"
#include "mfma_split.h"

namespace ucnerf {

constexpr int C3_KC = 32, C3_THREADS = 256, C3_WAVES = C3_THREADS / 64;
constexpr int C3_PAD_BIT = 31;                       // the validity bit a k past the end names
constexpr int C3_MAX_CIN = 1 << 16;

// Packed image: per class (one for the forward form, 8 for the transposed) [channel tile][k < kpad][rows] weights (zero past cout and past the
// class's cin * taps), then kpad int32 tap codes ci << 11 | bit << 6 | dd << 4 | dh << 2 | dw.
struct C3Layout {
    long long woff[8], toff[8], total;
    int kpad[8], taps[8], classes, rows;
};
static inline int c3_rows(int cout) { return cout <= 16 ? 16 : 32; }
static inline C3Layout c3_layout(int cin, int cout, int K, int transposed) {
    C3Layout L;
    L.classes = transposed ? 8 : 1;
    L.rows = c3_rows(cout);
    const long long mt = cdiv(cout, L.rows);
    long long at = 0;
    for (int c = 0; c < 8; ++c) {
        if (c >= L.classes) { L.woff[c] = L.toff[c] = 0; L.kpad[c] = L.taps[c] = 0; continue; }
        L.taps[c] = transposed ? (1 + (c >> 2 & 1)) * (1 + (c >> 1 & 1)) * (1 + (c & 1)) : K * K * K;
        L.kpad[c] = (int)(((long long)cin * L.taps[c] + C3_KC - 1) / C3_KC * C3_KC);
        L.woff[c] = at; at += mt * L.kpad[c] * L.rows;
        L.toff[c] = at; at += L.kpad[c];
    }
    L.total = at;
    return L;
}

__global__ void __launch_bounds__(256) conv3d_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int cin, int cout, int K, int transposed, C3Layout L) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.total) return;
    int c = 0;
    for (int j = 1; j < 8; ++j)
        if (j < L.classes && i >= L.woff[j]) c = j;
    const int pd = c >> 2 & 1, ph = c >> 1 & 1, pw = c & 1, taps = L.taps[c], kpad = L.kpad[c], ktot = cin * taps;
    const bool table = i >= L.toff[c];
    const long long r = i - (table ? L.toff[c] : L.woff[c]);
    const int k = table ? (int)r : (int)((r / L.rows) % kpad);
    const int ci = k / taps, t = k % taps;
    int kd, kh, kw, dd, dh, dw;
    if (transposed) {                                                    // live taps: parity 0 -> k = 1 (d = 0); parity 1 -> k = 0 (d = 1), k = 2 (d = 0)
        const int nh = 1 + ph, nw = 1 + pw, td = t / (nh * nw), th = (t / nw) % nh, tw = t % nw;
        kd = pd ? 2 * td : 1; kh = ph ? 2 * th : 1; kw = pw ? 2 * tw : 1;
        dd = pd ? 1 - td : 0; dh = ph ? 1 - th : 0; dw = pw ? 1 - tw : 0;
    } else {
        kd = dd = t / (K * K); kh = dh = (t / K) % K; kw = dw = t % K;
    }
    if (table) {
        reinterpret_cast<int*>(packed)[i] = k < ktot ? (ci << 11) | ((9 * dd + 3 * dh + dw) << 6) | (dd << 4) | (dh << 2) | dw : C3_PAD_BIT << 6;
    } else {
        const int co = (int)(r / ((long long)L.rows * kpad)) * L.rows + (int)(r % L.rows);
        const int K3 = K * K * K, tap = (kd * K + kh) * K + kw;
        float v = 0.f;
        if (co < cout && k < ktot) v = transposed ? w[((size_t)ci * cout + co) * K3 + tap] : w[((size_t)co * cin + ci) * K3 + tap];
        packed[i] = v;
    }
}

// what the kernels need beside the parameters: the voxel grid a block index runs over (the output's for the forward form, the input's for a
// class of the transposed one), how a grid voxel maps to the output (o = ostep * j + parity) and to the input base (j * istride - ipad)
struct C3Geom {
    int OD, OH, OW, QD, QH, QW, npix, ostep, istride, ipad;
    C3Layout lay;
};

__device__ __forceinline__ unsigned axis_bits(int base, int size, int K) {
    unsigned m = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) m |= (unsigned)(d < K && base + d >= 0 && base + d < size) << d;
    return m;
}

template <int MT, int NT>
__global__ void __launch_bounds__(C3_THREADS) conv3d_kernel(ucnerf_conv3d_params p, C3Geom g) {
    constexpr int ROWS = 16 * MT, WPIX = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, kq = lane >> 4;
    const int cls = blockIdx.z, pd = cls >> 2 & 1, ph = cls >> 1 & 1, pw = cls & 1;
    const int D = p.D, H = p.H, W = p.W, DHW = D * H * W, kpad = g.lay.kpad[cls];
    const int Kext = p.transposed ? 2 : p.K;
    const float* __restrict__ wsrc = p.packed + g.lay.woff[cls] + (size_t)blockIdx.y * kpad * ROWS + l15;
    const int* __restrict__ ktab = reinterpret_cast<const int*>(p.packed + g.lay.toff[cls]);
    const float* __restrict__ x = p.x;
    const int q0 = (blockIdx.x * C3_WAVES + wave) * WPIX + l15;
    long long xoff[NT];
    unsigned mask[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const int q = q0 + 16 * s;
        xoff[s] = 0;
        mask[s] = 0;
        if (q < g.npix) {
            const int jw = q % g.QW, jh = (q / g.QW) % g.QH, jd = (q / (g.QW * g.QH)) % g.QD, img = q / (g.QW * g.QH * g.QD);
            const int bd = jd * g.istride - g.ipad, bh = jh * g.istride - g.ipad, bw = jw * g.istride - g.ipad;
            const unsigned md = axis_bits(bd, D, Kext), mh = axis_bits(bh, H, Kext), mw = axis_bits(bw, W, Kext);
            unsigned m = 0;
#pragma unroll
            for (int dd = 0; dd < 3; ++dd)
#pragma unroll
                for (int dh = 0; dh < 3; ++dh)
                    if ((md >> dd & 1) && (mh >> dh & 1)) m |= mw << (9 * dd + 3 * dh);
            mask[s] = m;
            xoff[s] = (long long)img * p.cin * DHW + ((long long)bd * H + bh) * W + bw;      // (may lie before the image: read only where a bit is set)
        }
    }
    f32x4 total[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int s = 0; s < NT; ++s) total[m][s] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < kpad; c += C3_KC) {
        f32x4 acc[MT][NT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int s = 0; s < NT; ++s) acc[m][s] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < C3_KC / 4; ++t) {
            const int k = c + 4 * t + kq;                                // (< kpad)
            float a[MT], b[NT];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = wsrc[(size_t)k * ROWS + 16 * m];
            const int e = ktab[k];
            const int bit = (e >> 6) & 31;
            const int delta = (e >> 11) * DHW + (((e >> 4) & 3) * H + ((e >> 2) & 3)) * W + (e & 3);
#pragma unroll
            for (int s = 0; s < NT; ++s) b[s] = (mask[s] >> bit & 1) ? x[xoff[s] + delta] : 0.f;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int s = 0; s < NT; ++s) acc[m][s] = mfma_16x16x4(a[m], b[s], acc[m][s]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int s = 0; s < NT; ++s) total[m][s] += acc[m][s];
    }
    // ---- bias, activation, skip, store: register r of tile (m, s) is channel 16 m + 4 (lane >> 4) + r of voxel s 16 + (lane & 15)
    const long long ohw = (long long)g.OH * g.OW, odhw = ohw * g.OD;
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const int q = q0 + 16 * s;
        if (q >= g.npix) continue;
        const int jw = q % g.QW, jh = (q / g.QW) % g.QH, jd = (q / (g.QW * g.QH)) % g.QD, img = q / (g.QW * g.QH * g.QD);
        const long long at = (long long)img * p.cout * odhw + (long long)(jd * g.ostep + pd) * ohw + (long long)(jh * g.ostep + ph) * g.OW + (jw * g.ostep + pw);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = blockIdx.y * ROWS + 16 * m + 4 * kq + r;
                if (co < p.cout) {
                    float v = total[m][s][r] + p.bias[co];
                    if (p.relu) v = v > 0.f ? v : (v != v ? v : 0.f);       // torch.relu: a NaN stays
                    const long long idx = at + (long long)co * odhw;
                    if (p.skip) v += p.skip[idx];
                    p.y[idx] = v;
                }
            }
    }
}

// cout == 1, forward form: one thread per output voxel, the packed image's row 0 and tap codes, the same runs of 32.
__global__ void __launch_bounds__(C3_THREADS) conv3d_single_kernel(ucnerf_conv3d_params p, C3Geom g) {
    const int q = blockIdx.x * C3_THREADS + threadIdx.x;
    if (q >= g.npix) return;
    const int D = p.D, H = p.H, W = p.W, DHW = D * H * W, kpad = g.lay.kpad[0], ktot = p.cin * g.lay.taps[0];
    const float* __restrict__ wsrc = p.packed + g.lay.woff[0];
    const int* __restrict__ ktab = reinterpret_cast<const int*>(p.packed + g.lay.toff[0]);
    const int jw = q % g.QW, jh = (q / g.QW) % g.QH, jd = (q / (g.QW * g.QH)) % g.QD, img = q / (g.QW * g.QH * g.QD);
    const int bd = jd * g.istride - g.ipad, bh = jh * g.istride - g.ipad, bw = jw * g.istride - g.ipad;
    const unsigned md = axis_bits(bd, D, p.K), mh = axis_bits(bh, H, p.K), mw = axis_bits(bw, W, p.K);
    unsigned mask = 0;
#pragma unroll
    for (int dd = 0; dd < 3; ++dd)
#pragma unroll
        for (int dh = 0; dh < 3; ++dh)
            if ((md >> dd & 1) && (mh >> dh & 1)) mask |= mw << (9 * dd + 3 * dh);
    const float* __restrict__ x = p.x + (long long)img * p.cin * DHW + ((long long)bd * H + bh) * W + bw;
    float total = 0.f;
    for (int c = 0; c < kpad; c += C3_KC) {
        float acc = 0.f;
        const int end = min(C3_KC, ktot - c);                            // (uniform; the padded k would add fma(0, 0, acc))
        for (int t = 0; t < end; ++t) {
            const int e = ktab[c + t];                                   // (uniform: scalar loads)
            const int delta = (e >> 11) * DHW + (((e >> 4) & 3) * H + ((e >> 2) & 3)) * W + (e & 3);
            const float v = (mask >> ((e >> 6) & 31) & 1) ? x[delta] : 0.f;
            acc = __builtin_fmaf(wsrc[(size_t)(c + t) * 16], v, acc);
        }
        total += acc;
    }
    float v = total + p.bias[0];
    if (p.relu) v = v > 0.f ? v : (v != v ? v : 0.f);
    const long long idx = (long long)img * g.OD * g.OH * g.OW + ((long long)jd * g.OH + jh) * g.OW + jw;
    if (p.skip) v += p.skip[idx];
    p.y[idx] = v;
}

static int c3_shape_check(int cin, int cout, int K, int stride, int pad, int transposed, const char* who) {
    UCNERF_REQUIRE(cin >= 1 && cout >= 1 && cin <= C3_MAX_CIN && cout <= (1 << 20), "%s: cin=%d cout=%d (cin 1 .. %d, cout 1 .. 2^20)", who, cin, cout, C3_MAX_CIN);
    UCNERF_REQUIRE(transposed == 0 || transposed == 1, "%s: transposed=%d (0 or 1)", who, transposed);
    if (transposed)
        UCNERF_REQUIRE(K == 3 && stride == 2 && pad == 1, "%s: the transposed form is K=3 stride=2 pad=1 output_padding=1 only, got K=%d stride=%d pad=%d", who, K, stride, pad);
    else
        UCNERF_REQUIRE((K == 1 || K == 3) && (stride == 1 || stride == 2) && pad >= 0 && pad <= 64, "%s: K=%d stride=%d pad=%d (K 1 or 3, stride 1 or 2, pad 0 .. 64)", who, K, stride, pad);
    return UCNERF_OK;
}

static int c3_launch(const ucnerf_conv3d_params* p, hipStream_t st, const char* who) {
    UCNERF_REQUIRE(p->n >= 0, "%s: negative count %d", who, p->n);
    if (int rc = c3_shape_check(p->cin, p->cout, p->K, p->stride, p->pad, p->transposed, who)) return rc;
    UCNERF_REQUIRE(p->D >= 1 && p->H >= 1 && p->W >= 1, "%s: D=%d H=%d W=%d (all at least 1)", who, p->D, p->H, p->W);
    const C3Layout L = c3_layout(p->cin, p->cout, p->K, p->transposed);
    UCNERF_REQUIRE(p->packed_floats == L.total, "%s: the packed weight holds %lld floats, cin=%d cout=%d K=%d transposed=%d packs to %lld", who,
                   (long long)p->packed_floats, p->cin, p->cout, p->K, p->transposed, L.total);
    C3Geom g;
    g.lay = L;
    if (p->transposed) {
        g.OD = 2 * p->D; g.OH = 2 * p->H; g.OW = 2 * p->W;
        g.QD = p->D; g.QH = p->H; g.QW = p->W;
        g.ostep = 2; g.istride = 1; g.ipad = 0;
    } else {
        UCNERF_REQUIRE(p->D + 2 * p->pad >= p->K && p->H + 2 * p->pad >= p->K && p->W + 2 * p->pad >= p->K, "%s: a %d x %d x %d input with pad %d is smaller than the kernel %d", who,
                       p->D, p->H, p->W, p->pad, p->K);
        g.OD = (p->D + 2 * p->pad - p->K) / p->stride + 1; g.OH = (p->H + 2 * p->pad - p->K) / p->stride + 1; g.OW = (p->W + 2 * p->pad - p->K) / p->stride + 1;
        g.QD = g.OD; g.QH = g.OH; g.QW = g.OW;
        g.ostep = 1; g.istride = p->stride; g.ipad = p->pad;
    }
    const long long in_img = (long long)p->cin * p->D * p->H * p->W, out_img = (long long)p->cout * g.OD * g.OH * g.OW;
    const long long npix = (long long)p->n * g.QD * g.QH * g.QW;
    UCNERF_REQUIRE(in_img < (1ll << 31) && out_img < (1ll << 31) && npix < (1ll << 31) - 1024, "%s: cin D H W = %lld, cout OD OH OW = %lld or n voxels = %lld too large (32-bit index)", who,
                   in_img, out_img, npix);
    if (p->n == 0) return UCNERF_OK;
    UCNERF_REQUIRE(p->x && p->packed && p->bias && p->y, "%s: null x, packed, bias or y", who);
    g.npix = (int)npix;
    const int mt = cdiv(p->cout, L.rows);
    UCNERF_REQUIRE(mt <= 65535, "%s: cout = %d above the grid limit", who, p->cout);
    if (p->cout == 1 && !p->transposed)
        hipLaunchKernelGGL(conv3d_single_kernel, dim3(cdiv(npix, C3_THREADS)), dim3(C3_THREADS), 0, st, *p, g);
    else if (L.rows == 16)
        hipLaunchKernelGGL((conv3d_kernel<1, 4>), dim3(cdiv(npix, C3_WAVES * 64), mt, L.classes), dim3(C3_THREADS), 0, st, *p, g);
    else
        hipLaunchKernelGGL((conv3d_kernel<2, 2>), dim3(cdiv(npix, C3_WAVES * 32), mt, L.classes), dim3(C3_THREADS), 0, st, *p, g);
    return UCNERF_OK;
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int64_t ucnerf_conv3d_packed_floats(int32_t cin, int32_t cout, int32_t K, int32_t transposed) {
    if (int rc = c3_shape_check(cin, cout, K, transposed ? 2 : 1, transposed ? 1 : 0, transposed, "conv3d_packed_floats")) return rc;
    return c3_layout(cin, cout, K, transposed).total;
}

int ucnerf_conv3d_pack(const ucnerf_conv3d_pack_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv3d_pack: null params");
    if (int rc = c3_shape_check(p->cin, p->cout, p->K, p->transposed ? 2 : 1, p->transposed ? 1 : 0, p->transposed, "conv3d_pack")) return rc;
    UCNERF_REQUIRE(p->weight && p->packed, "conv3d_pack: null weight or packed");
    const C3Layout L = c3_layout(p->cin, p->cout, p->K, p->transposed);
    hipLaunchKernelGGL(conv3d_pack_kernel, dim3((unsigned)((L.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->weight, p->packed, p->cin, p->cout, p->K, p->transposed, L);
    return check_launch("conv3d_pack");
}

int ucnerf_conv3d(const ucnerf_conv3d_params* p, void* stream) {
    UCNERF_REQUIRE(p, "conv3d: null params");
    if (int rc = c3_launch(p, (hipStream_t)stream, "conv3d")) return rc;
    return p->n == 0 ? UCNERF_OK : check_launch("conv3d");
}

}  // extern "C"
