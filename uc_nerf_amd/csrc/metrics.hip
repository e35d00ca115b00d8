// e1, the evaluation metrics of utils/evaluation.py on the device: median-scaled depth errors (depth_evaluation / compute_errors, :8-74) and the
// per-image mean squared error, PSNR and SSIM of rgb_evaluation (:76-101).  The images stay where the render pass wrote them; a host reads one
// small vector per call.  Plain HIP C++, wave64; no LDS tricks, no matrix cores: at 10 views of 256 x 320 every kernel here moves a few MB.
//
// Reproducibility.  Everything that is counted is an integer (LDS and global uint32 atomics: order-independent).  Every float sum goes
// thread -> wave (shuffle tree) -> block (4 waves in order) -> one partial per block in a slab -> a second launch that adds the partials in a
// fixed order.  No float atomics, so two calls give the same bits (the grid of every kernel depends on the shapes alone).
//
// Hand-offs between blocks happen ONLY at kernel boundaries (a launch reads what an earlier launch on the same stream wrote): there is no
// "last block" counter and no in-kernel publish / acquire to get wrong.  The price is a handful of one-block launches of a few microseconds.
#include "common.h"

namespace ucnerf {

constexpr int EV_BLOCK = 256;
constexpr int EV_WAVES = EV_BLOCK / 64;
constexpr int EV_MAX_PARTS = 64;      // blocks per image of the slab reductions: the second launch folds them with ONE wave
constexpr int SEL = 4;                // selections in flight: gt rank (N-1)/2, gt rank N/2, pred rank (N-1)/2, pred rank N/2
constexpr int SEL_PASSES = 4;         // 8-bit digits, most significant first
constexpr int SEL_BINS = 256;
constexpr int HIST_MAX_BLOCKS = 256;      // one per CU: a block flushes up to 1024 bins with global atomics, so few and long-lived blocks
constexpr int SSIM_TILE = 16;         // windows (outputs) per tile side; the staged input tile is (16 + 6)^2
constexpr int SSIM_WIN = 7;
constexpr int SSIM_IN = SSIM_TILE + SSIM_WIN - 1;

// Workspace layout, in 32-bit words (all offsets even: the fp64 slab comes first and the base is 8-byte aligned)
//   depth:  [hist: SEL_PASSES x SEL x 256 u32][state: 16 u32][slab: n x parts x 8 words]
//   image:  [ssim slab: n x 3 x tiles doubles][mse slab: n x parts x 2 floats]
constexpr long long WS_HIST = 0, WS_HIST_WORDS = (long long)SEL_PASSES * SEL * SEL_BINS, WS_STATE = WS_HIST + WS_HIST_WORDS, WS_STATE_WORDS = 16;
constexpr long long WS_DEPTH_SLAB = WS_STATE + WS_STATE_WORDS;
// state words: [0..3] key prefix of each selection, [4..7] rank still to find inside the prefix, [8] 1 = no valid pixel
enum { ST_PREFIX = 0, ST_RANK = 4, ST_EMPTY = 8 };

static inline int parts_per_image(long long elems) { return (int)((elems + EV_BLOCK - 1) / EV_BLOCK < EV_MAX_PARTS ? (elems + EV_BLOCK - 1) / EV_BLOCK : EV_MAX_PARTS); }
static inline long long ssim_tiles(int H, int W) { return H >= SSIM_WIN && W >= SSIM_WIN ? (long long)cdiv(H - 6, SSIM_TILE) * cdiv(W - 6, SSIM_TILE) : 0; }

// ---------------------------------------------------------------------------------------------- block sums in a fixed order
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);      // lane 0 holds the sum; the tree is the same on every run
    return v;
}
// all EV_BLOCK threads call it; thread 0 gets the sum (the others an unspecified value).  `lds` holds EV_WAVES values; ends behind a barrier,
// so that the next call may reuse `lds`
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = lds[0];
#pragma unroll
    for (int w = 1; w < EV_WAVES; ++w) s += lds[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ float block_max(float v, float* lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_down(v, d));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = lds[0];
#pragma unroll
    for (int w = 1; w < EV_WAVES; ++w) s = fmaxf(s, lds[w]);
    __syncthreads();
    return s;
}

// ---------------------------------------------------------------------------------------------- median by radix selection
// float32 -> uint32 key with the same order: negatives have all bits flipped, the others the sign bit (-0.0 sorts right below +0.0)
__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

__device__ __forceinline__ bool depth_valid(const ucnerf_depth_eval_params& p, unsigned i, float g) {
    return g > p.min_depth && g < p.max_depth && (p.mask == nullptr || p.mask[i] != 0);      // evaluation.py:38, :44-45 (NaN: never valid)
}

// Pass `pass` counts, for each selection, the digit (key >> shift) & 255 of the valid pixels whose higher digits equal the selection's prefix
__global__ void __launch_bounds__(EV_BLOCK) select_hist_kernel(ucnerf_depth_eval_params p, unsigned total, int pass) {
    __shared__ unsigned h[SEL][SEL_BINS];
    unsigned* ws = reinterpret_cast<unsigned*>(p.workspace);
    const unsigned* state = ws + WS_STATE;
    unsigned* hist = ws + WS_HIST + (long long)pass * SEL * SEL_BINS;
    for (int b = threadIdx.x; b < SEL * SEL_BINS; b += EV_BLOCK) (&h[0][0])[b] = 0;
    __syncthreads();
    if (pass > 0 && state[ST_EMPTY]) return;                           // (uniform: nothing to select from)
    const int shift = 24 - 8 * pass;
    unsigned prefix[SEL];
#pragma unroll
    for (int s = 0; s < SEL; ++s) prefix[s] = pass > 0 ? state[ST_PREFIX + s] : 0u;
    for (unsigned i = blockIdx.x * EV_BLOCK + threadIdx.x; i < total; i += gridDim.x * EV_BLOCK) {      // (total < 2^31, grid * block = 2^16: no wrap)
        const float g = p.gt[i];
        if (!depth_valid(p, i, g)) continue;
        const unsigned key[2] = {order_key(g), order_key(p.pred[i])};
#pragma unroll
        for (int s = 0; s < SEL; ++s) {
            const unsigned k = key[s >> 1];
            // the digits above this pass's: pass 0 has none (and a shift by 32 is not defined)
            if (pass == 0 || ((k ^ prefix[s]) >> (shift + 8)) == 0) atomicAdd(&h[s][(k >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SEL * SEL_BINS; b += EV_BLOCK) {
        const unsigned c = (&h[0][0])[b];
        if (c) atomicAdd(hist + b, c);
    }
}

// One block: thread s walks selection s's 256 counts to the digit that holds its rank.  After the last pass the prefixes ARE the keys of the
// wanted order statistics: the medians and their quotient go to out[0..3].
__global__ void __launch_bounds__(64) select_pick_kernel(ucnerf_depth_eval_params p, int pass) {
    __shared__ unsigned done[SEL];
    unsigned* ws = reinterpret_cast<unsigned*>(p.workspace);
    unsigned* state = ws + WS_STATE;
    const unsigned* hist = ws + WS_HIST + (long long)pass * SEL * SEL_BINS;
    const int s = threadIdx.x;
    bool empty = false;
    if (s < SEL) {
        const unsigned* hs = hist + s * SEL_BINS;
        unsigned rank, prefix;
        if (pass == 0) {
            unsigned N = 0;
            for (int b = 0; b < SEL_BINS; ++b) N += hs[b];             // the number of valid pixels (the same for all four selections)
            empty = N == 0;
            rank = (s & 1) ? N / 2 : (N - (N != 0)) / 2;               // ranks (N-1)/2 and N/2: equal for an odd count
            prefix = 0;
            if (s == 0) state[ST_EMPTY] = empty;
        } else {
            empty = state[ST_EMPTY] != 0;
            rank = state[ST_RANK + s];
            prefix = state[ST_PREFIX + s];
        }
        if (!empty) {
            unsigned below = 0;
            int digit = SEL_BINS - 1;                                   // (the rank always falls inside the counted pixels; the last bin otherwise)
            for (int b = 0; b < SEL_BINS; ++b) {
                const unsigned c = hs[b];
                if (rank < below + c) { digit = b; break; }
                below += c;
            }
            rank -= below;
            prefix |= (unsigned)digit << (24 - 8 * pass);
        }
        state[ST_RANK + s] = rank;
        state[ST_PREFIX + s] = prefix;
        done[s] = prefix;
    }
    if (pass != SEL_PASSES - 1) return;
    __syncthreads();
    if (s == 0) {
        float med[2];
        for (int a = 0; a < 2; ++a) {
            const float lo = key_value(done[2 * a]), hi = key_value(done[2 * a + 1]);
            med[a] = done[2 * a] == done[2 * a + 1] ? lo : (lo + hi) / 2.f;      // numpy: the mean of the two middle values, fl(fl(a + b) / 2)
        }
        const float nan = __uint_as_float(0x7fc00000u);
        p.out[0] = empty ? nan : med[0] / med[1];                       // evaluation.py:56-57
        reinterpret_cast<int*>(p.out)[1] = empty;
        p.out[2] = empty ? nan : med[0];
        p.out[3] = empty ? nan : med[1];
    }
}

// raw mode (compute_errors alone): the header of `out` without a selection
__global__ void depth_raw_header_kernel(ucnerf_depth_eval_params p) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        p.out[0] = 1.f;
        reinterpret_cast<int*>(p.out)[1] = 0;
        p.out[2] = p.out[3] = __uint_as_float(0x7fc00000u);
    }
}

// ---------------------------------------------------------------------------------------------- depth errors
// grid (parts, n): block (b, i) walks image i's pixels b * 256 + t, + parts * 256, ...; its partial: 4 float sums and 4 counts
__global__ void __launch_bounds__(EV_BLOCK) depth_errors_kernel(ucnerf_depth_eval_params p, unsigned plane, int with_header) {
    __shared__ float lf[EV_WAVES];
    __shared__ int li[EV_WAVES];
    const float ratio = with_header ? p.out[0] : 1.f;                  // (written by an earlier launch; raw mode: 1)
    const unsigned base = blockIdx.y * plane;
    float s_sq = 0.f, s_log = 0.f, s_abs = 0.f, s_sqrel = 0.f;
    int c_n = 0, c1 = 0, c2 = 0, c3 = 0;
    for (unsigned j = blockIdx.x * EV_BLOCK + threadIdx.x; j < plane; j += gridDim.x * EV_BLOCK) {
        const unsigned i = base + j;
        const float g = p.gt[i];
        float q = p.pred[i];
        if (!p.raw) {
            if (!depth_valid(p, i, g)) continue;
            q = q * ratio;                                              // :63
            q = q < p.min_depth ? p.min_depth : q;                      // :64-65
            q = q > p.max_depth ? p.max_depth : q;
        }
        const float a = g / q, b = q / g, t = fmaxf(a, b);              // :11
        const bool nan_t = a != a || b != b;                            // (np.maximum propagates a NaN, fmaxf drops it: a NaN fails every `<`)
        c_n += 1;
        c1 += !nan_t && t < 1.25f;
        c2 += !nan_t && t < 1.5625f;
        c3 += !nan_t && t < 1.953125f;
        const float d = g - q, d2 = d * d, l = logf(g) - logf(q);
        s_sq += d2;                                                      // :16
        s_log += l * l;                                                  // :19
        s_abs += fabsf(d) / g;                                           // :22
        s_sqrel += d2 / g;                                               // :24
    }
    const float f0 = block_sum(s_sq, lf), f1 = block_sum(s_log, lf), f2 = block_sum(s_abs, lf), f3 = block_sum(s_sqrel, lf);
    const int i0 = block_sum(c_n, li), i1 = block_sum(c1, li), i2 = block_sum(c2, li), i3 = block_sum(c3, li);
    if (threadIdx.x == 0) {
        float* part = p.workspace + WS_DEPTH_SLAB + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8;
        part[0] = f0; part[1] = f1; part[2] = f2; part[3] = f3;
        int* ip = reinterpret_cast<int*>(part + 4);
        ip[0] = i0; ip[1] = i1; ip[2] = i2; ip[3] = i3;
    }
}

// grid n, one wave: lane l holds partial l (parts <= 64), the shuffle tree adds them in the same order every time
__global__ void __launch_bounds__(64) depth_finish_kernel(ucnerf_depth_eval_params p, int parts) {
    const int lane = threadIdx.x, img = blockIdx.x;
    const float* part = p.workspace + WS_DEPTH_SLAB + ((long long)img * parts + lane) * 8;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    int c[4] = {0, 0, 0, 0};
    if (lane < parts) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { f[k] = part[k]; c[k] = reinterpret_cast<const int*>(part + 4)[k]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[k] = wave_sum(f[k]); c[k] = wave_sum(c[k]); }
    if (lane != 0) return;
    float* o = p.out + 4 + 12 * (long long)img;
    int* oi = reinterpret_cast<int*>(o);
    const float cnt = (float)c[0];
    oi[0] = c[0]; oi[1] = c[1]; oi[2] = c[2]; oi[3] = c[3];
    o[4] = f[2] / cnt;                                                   // abs_rel
    o[5] = f[3] / cnt;                                                   // sq_rel
    o[6] = sqrtf(f[0] / cnt);                                            // rmse
    o[7] = sqrtf(f[1] / cnt);                                            // rmse_log
    o[8] = (float)c[1] / cnt; o[9] = (float)c[2] / cnt; o[10] = (float)c[3] / cnt;
    oi[11] = c[0] == 0;                                                  // (0 / 0 above: NaN in all seven)
}

// ---------------------------------------------------------------------------------------------- image error
// grid (parts, n): sum of (gt - pred)^2 and max of gt over image i's 3 H W values
__global__ void __launch_bounds__(EV_BLOCK) image_mse_kernel(ucnerf_image_eval_params p, unsigned elems, long long slab) {
    __shared__ float lf[EV_WAVES];
    const unsigned base = blockIdx.y * elems;
    float s = 0.f, m = -INFINITY;
    for (unsigned j = blockIdx.x * EV_BLOCK + threadIdx.x; j < elems; j += gridDim.x * EV_BLOCK) {
        const float g = p.gt[base + j], d = g - p.pred[base + j];
        s += d * d;
        m = fmaxf(m, g);
    }
    s = block_sum(s, lf);
    m = block_max(m, lf);
    if (threadIdx.x == 0) {
        float* part = p.workspace + slab + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        part[0] = s; part[1] = m;
    }
}

// SSIM.  One block per (tile of 16 x 16 windows, channel, image).  The (16 + 6)^2 input pixels of x and y are staged in LDS as float32; the window
// sums of x, y, xx, yy, xy are formed separably -- 7 taps along the row into LDS, then 7 taps down the column -- by DIRECT summation (no sliding
// add-and-subtract, which would carry its rounding from window to window) and in fp64.  Form of the cancellation in uxx - ux ux: a product of
// two float32 values is exact in fp64 (48 bits), a sum of 49 of them carries at most 12 roundings of 2^-53, so the difference loses
// log2(uxx / v) of 53 bits: for 8-bit images (v >= 1e-6 unless the window is constant, where the difference is exactly 0 because all 49
// terms are equal ... up to those 12 roundings, 1e-15 against C2 = 9e-4) nothing a float32 result can show.  S and its sums stay in fp64 up to
// the one rounding of the per-image mean.
__global__ void __launch_bounds__(EV_BLOCK) ssim_tile_kernel(ucnerf_image_eval_params p, int tiles_x, int tiles) {
    __shared__ float tx[SSIM_IN][SSIM_IN + 1], ty[SSIM_IN][SSIM_IN + 1];
    __shared__ double hs[5][SSIM_IN][SSIM_TILE];
    __shared__ double ld[EV_WAVES];
    const int H = p.H, W = p.W;
    const int tile = blockIdx.x, ch = blockIdx.y, img = blockIdx.z;
    const int r0 = (tile / tiles_x) * SSIM_TILE, c0 = (tile % tiles_x) * SSIM_TILE;      // first window (= first input pixel) of the tile
    const size_t plane = ((size_t)img * 3 + ch) * (size_t)H * W;
    for (int e = threadIdx.x; e < SSIM_IN * SSIM_IN; e += EV_BLOCK) {
        const int r = e / SSIM_IN, c = e % SSIM_IN;
        const bool in = r0 + r < H && c0 + c < W;                      // (past the image: zeros, read only by windows that are not counted)
        const size_t at = plane + (size_t)(r0 + r) * W + (c0 + c);
        tx[r][c] = in ? p.gt[at] : 0.f;
        ty[r][c] = in ? p.pred[at] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SSIM_IN * SSIM_TILE; e += EV_BLOCK) {
        const int r = e / SSIM_TILE, c = e % SSIM_TILE;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int d = 0; d < SSIM_WIN; ++d) {
            const double x = tx[r][c + d], y = ty[r][c + d];
            sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
        }
        hs[0][r][c] = sx; hs[1][r][c] = sy; hs[2][r][c] = sxx; hs[3][r][c] = syy; hs[4][r][c] = sxy;
    }
    __syncthreads();
    const int r = threadIdx.x / SSIM_TILE, c = threadIdx.x % SSIM_TILE;
    double S = 0;
    if (r0 + r < H - 6 && c0 + c < W - 6) {
        double q[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double a = 0;
#pragma unroll
            for (int d = 0; d < SSIM_WIN; ++d) a += hs[k][r + d][c];
            q[k] = a / 49.0;
        }
        const double cov_norm = 49.0 / 48.0, C1 = 1e-4, C2 = 9e-4;      // (K1 data_range)^2, (K2 data_range)^2
        const double ux = q[0], uy = q[1];
        const double vx = cov_norm * (q[2] - ux * ux), vy = cov_norm * (q[3] - uy * uy), vxy = cov_norm * (q[4] - ux * uy);
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
    }
    S = block_sum(S, ld);
    if (threadIdx.x == 0) reinterpret_cast<double*>(p.workspace)[((size_t)img * 3 + ch) * tiles + tile] = S;
}

// grid n, one block: the three channels' tile partials in a fixed order, the mse partials with one wave; out[i] = (mse, psnr, ssim, gt_max)
__global__ void __launch_bounds__(EV_BLOCK) image_finish_kernel(ucnerf_image_eval_params p, int parts, int tiles, long long slab) {
    __shared__ double ld[EV_WAVES];
    __shared__ float lf[EV_WAVES];
    const int img = blockIdx.x, t = threadIdx.x;
    const double* sp = reinterpret_cast<const double*>(p.workspace) + (size_t)img * 3 * tiles;
    const double windows = (double)(p.H - 6) * (double)(p.W - 6);
    double ssim = 0;
    for (int ch = 0; ch < 3; ++ch) {
        double a = 0;
        for (int k = t; k < tiles; k += EV_BLOCK) a += sp[(size_t)ch * tiles + k];
        a = block_sum(a, ld);
        ssim += a / windows;                                             // (thread 0's value is the one used)
    }
    const float* part = p.workspace + slab + (long long)img * parts * 2;
    const float s = block_sum(t < parts ? part[2 * t] : 0.f, lf);
    const float m = block_max(t < parts ? part[2 * t + 1] : -INFINITY, lf);
    if (t != 0) return;
    float* o = p.out + 4 * (long long)img;
    const float mse = s / (float)(3ll * p.H * p.W);
    o[0] = mse;
    o[1] = (float)(-10.0 * log10((double)mse));                          // evaluation.py:83, one rounding
    o[2] = p.no_ssim ? __uint_as_float(0x7fc00000u) : (float)(ssim / 3.0);
    o[3] = m;
}

}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int64_t ucnerf_eval_workspace_floats(int32_t n, int32_t H, int32_t W) {
    if (n <= 0 || H <= 0 || W <= 0) return fail(UCNERF_EINVAL, "eval_workspace_floats: n=%d H=%d W=%d", n, H, W);
    const long long plane = (long long)H * W;
    if ((long long)n * plane * 3 >= (1ll << 31)) return fail(UCNERF_EINVAL, "eval_workspace_floats: 3 n H W = %lld does not fit 31 bits", 3ll * n * plane);
    const long long depth = WS_DEPTH_SLAB + (long long)n * parts_per_image(plane) * 8;
    const long long image = 2 * (long long)n * 3 * ssim_tiles(H, W) + (long long)n * parts_per_image(3 * plane) * 2;
    return (depth > image ? depth : image) + 2;
}

int ucnerf_depth_eval(const ucnerf_depth_eval_params* p, void* stream) {
    UCNERF_REQUIRE(p, "depth_eval: null params");
    UCNERF_REQUIRE(p->n > 0 && p->H > 0 && p->W > 0, "depth_eval: n=%d H=%d W=%d (negative or empty)", p->n, p->H, p->W);
    const long long plane = (long long)p->H * p->W, total = plane * p->n;
    UCNERF_REQUIRE(total < (1ll << 31), "depth_eval: n H W = %lld pixels (32-bit pixel index)", total);
    UCNERF_REQUIRE(p->n <= 65535, "depth_eval: n = %d images above 65535 (grid limit)", p->n);
    UCNERF_REQUIRE(p->gt && p->pred && p->workspace && p->out, "depth_eval: null gt, pred, workspace or out");
    UCNERF_REQUIRE(((uintptr_t)p->workspace & 7) == 0 && ((uintptr_t)p->out & 3) == 0, "depth_eval: workspace must be 8-byte aligned");
    UCNERF_REQUIRE(p->raw || p->min_depth <= p->max_depth, "depth_eval: min_depth %g above max_depth %g", p->min_depth, p->max_depth);
    hipStream_t st = (hipStream_t)stream;
    const int parts = parts_per_image(plane);
    if (!p->raw) {
        if (hipMemsetAsync(p->workspace + WS_HIST, 0, (WS_HIST_WORDS + WS_STATE_WORDS) * sizeof(float), st) != hipSuccess)
            return fail(UCNERF_EHIP, "depth_eval: clearing the histograms failed");
        const int blocks = cdiv(total, EV_BLOCK) < HIST_MAX_BLOCKS ? cdiv(total, EV_BLOCK) : HIST_MAX_BLOCKS;
        for (int pass = 0; pass < SEL_PASSES; ++pass) {
            hipLaunchKernelGGL(select_hist_kernel, dim3(blocks), dim3(EV_BLOCK), 0, st, *p, (unsigned)total, pass);
            hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(64), 0, st, *p, pass);
        }
    } else {
        hipLaunchKernelGGL(depth_raw_header_kernel, dim3(1), dim3(64), 0, st, *p);
    }
    hipLaunchKernelGGL(depth_errors_kernel, dim3(parts, p->n), dim3(EV_BLOCK), 0, st, *p, (unsigned)plane, p->raw ? 0 : 1);
    hipLaunchKernelGGL(depth_finish_kernel, dim3(p->n), dim3(64), 0, st, *p, parts);
    return check_launch("depth_eval");
}

int ucnerf_image_eval(const ucnerf_image_eval_params* p, void* stream) {
    UCNERF_REQUIRE(p, "image_eval: null params");
    UCNERF_REQUIRE(p->n > 0 && p->H > 0 && p->W > 0, "image_eval: n=%d H=%d W=%d (negative or empty)", p->n, p->H, p->W);
    UCNERF_REQUIRE(p->no_ssim || (p->H >= SSIM_WIN && p->W >= SSIM_WIN), "image_eval: a %d x %d image is smaller than the 7 x 7 SSIM window", p->H, p->W);
    const long long elems = 3ll * p->H * p->W, total = elems * p->n;
    UCNERF_REQUIRE(total < (1ll << 31), "image_eval: 3 n H W = %lld values (32-bit index)", total);
    UCNERF_REQUIRE(p->n <= 65535, "image_eval: n = %d images above 65535 (grid limit)", p->n);
    UCNERF_REQUIRE(p->gt && p->pred && p->workspace && p->out, "image_eval: null gt, pred, workspace or out");
    UCNERF_REQUIRE(((uintptr_t)p->workspace & 7) == 0, "image_eval: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int parts = parts_per_image(elems), tiles_x = p->no_ssim ? 0 : cdiv(p->W - 6, SSIM_TILE);
    const long long tiles = p->no_ssim ? 0 : ssim_tiles(p->H, p->W), slab = 2 * (long long)p->n * 3 * tiles;
    UCNERF_REQUIRE(tiles < (1ll << 31), "image_eval: %lld SSIM tiles", tiles);
    hipLaunchKernelGGL(image_mse_kernel, dim3(parts, p->n), dim3(EV_BLOCK), 0, st, *p, (unsigned)elems, slab);
    if (tiles > 0) hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)tiles, 3, p->n), dim3(EV_BLOCK), 0, st, *p, tiles_x, (int)tiles);
    hipLaunchKernelGGL(image_finish_kernel, dim3(p->n), dim3(EV_BLOCK), 0, st, *p, parts, (int)tiles, slab);
    return check_launch("image_eval");
}

}  // extern "C"
