// What the two batch-norm translation units share (bn.hip: one set of statistics per call; bn_groups.hip: one per group of images): the walk over
// a channel's values, Chan's merge, every reduction and the streaming epilogues as device functions, and the host-side shape checks.  A kernel
// of either file is one of these bodies on a slab [n,C,S]; the grouped kernels only move the base pointers to their group's slab first, so the
// arithmetic of a group IS the ungrouped arithmetic: the same expressions in the same order (the build compiles with -ffp-contract=off and
// correctly rounded division and square root, so equal expressions give equal bits).
//
// A channel's N = n S values are numbered i = img * S + offset.  Everything walks them in QUADS of four consecutive i; where S is a multiple of
// four and the arrays are 16-byte aligned a quad is one 16-byte access, otherwise four scalar ones -- the values and the order of every sum are
// the same either way.  Every intermediate of the statistics is float64: a float32 slice mean at |mean| >> sigma would put its own rounding,
// squared and multiplied by the count, into M2.
#pragma once
#include "common.h"

#include <cstdint>

namespace ucnerf {
namespace {

constexpr int BN_STATS_THREADS = 1024;                   // 16 waves: one block per CU keeps 64 KiB of loads in flight
constexpr int BN_CHUNK_QUADS = 4;                        // a thread's chunk: 4 quads = 16 values held in registers
constexpr int BN_MIN_SLICE = BN_STATS_THREADS * 4;       // one round of the block
constexpr int BN_MAX_PARTIALS = 32;                      // what an apply block folds serially
constexpr int BN_APPLY_THREADS = 256;
constexpr int BN_APPLY_QUADS = 4;
constexpr int BN_APPLY_CHUNK = BN_APPLY_THREADS * BN_APPLY_QUADS * 4;     // 4096 values per block
constexpr int64_t BN_MAX_COUNT = (1ll << 31) - (1ll << 20);               // N: 32-bit walk with room for the last round's overshoot
constexpr int BN_MAX_GROUPS = 64;                        // G of the grouped entry points: one thread of an apply block per group

struct Triple { double n, mean, m2; };

struct Walk {                      // where the values of one channel lie
    int64_t C, S;                  // address of value i of channel c: ((i / S) * C + c) * S + i % S
    unsigned N, S32;
    int vec;                       // 1: S % 4 == 0 and every array 16-byte aligned
};

struct ApplyArgs {
    const float *y, *skip, *gamma, *beta;
    float *out, *saved_mean, *saved_var, *running_mean, *running_var;
    long long* num_batches_tracked;
    const double* ws;
    float eps, momentum;
    int P, relu;
};

// ---- backward: the same slices and quads as the forward pair, a float64 workspace [C, P, 2].
// gm = g where the forward's ReLU let the value through (z = bn_affine(y, mu, s, beta), the mask is !(z <= 0): torch's threshold rule), else 0.
struct BwdArgs {
    const float *g, *y, *mean, *var, *gamma, *beta;
    float eps;
    int relu, P;
};

#ifdef __HIPCC__
// Chan's pairwise update, a then b.  One division; b empty leaves a as it is (an empty a comes out as b: r = 1, na r = 0).
__device__ __forceinline__ Triple chan(const Triple a, const Triple b) {
    if (b.n == 0.0) return a;
    const double n = a.n + b.n, r = b.n / n, d = b.mean - a.mean;
    Triple o;
    o.n = n;
    o.mean = a.mean + d * r;
    o.m2 = (a.m2 + b.m2) + (d * d) * (a.n * r);
    return o;
}

__device__ __forceinline__ size_t bn_addr(const Walk& w, int c, unsigned i) {
    const unsigned img = i / w.S32;
    return ((size_t)img * (size_t)w.C + (size_t)c) * (size_t)w.S + (size_t)(i - img * w.S32);
}

// the quad at i (a multiple of four), values at or past `end` read as 0 and are never used
__device__ __forceinline__ void bn_load_quad(const float* p,const Walk& w, int c, unsigned i, unsigned end, float v[4]) {
    if (w.vec) {                                           // (i + 3 < end wherever i < end: S, hence N and every slice start, is a multiple of 4)
        const float4 q = *reinterpret_cast<const float4*>(p + bn_addr(w, c, i));
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i + e < end ? p[bn_addr(w, c, i + e)] : 0.f;
    }
}

// Slice j of channel c of the slab at y -> its triple, held by thread 0 on return.  Every thread of the 1024 calls it (one barrier).
__device__ __forceinline__ Triple bn_slice_triple(const float* __restrict__ y, const Walk& w, unsigned L, int j, int c, int t) {
    const unsigned begin = (unsigned)j * L;
    const unsigned end = min(begin + L, w.N);              // (j < P: begin < N)
    Triple run = {0.0, 0.0, 0.0};
    // thread t, chunk k: the quads (k * 4 + u) * 1024 + t, u = 0 .. 3, of the slice
    for (unsigned q0 = 0; begin + q0 * 4u < end; q0 += BN_CHUNK_QUADS * BN_STATS_THREADS) {
        float v[BN_CHUNK_QUADS][4];
        unsigned at[BN_CHUNK_QUADS];
#pragma unroll
        for (int u = 0; u < BN_CHUNK_QUADS; ++u) {
            at[u] = begin + (q0 + (unsigned)u * BN_STATS_THREADS + (unsigned)t) * 4u;
            if (at[u] < end) bn_load_quad(y, w, c, at[u], end, v[u]);
        }
        double sum = 0.0;
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < BN_CHUNK_QUADS; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (at[u] < end && at[u] + e < end) { sum += (double)v[u][e]; ++cnt; }
        if (cnt == 0) continue;
        Triple ch;
        ch.n = (double)cnt;
        ch.mean = sum / ch.n;
        ch.m2 = 0.0;
#pragma unroll
        for (int u = 0; u < BN_CHUNK_QUADS; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (at[u] < end && at[u] + e < end) { const double d = (double)v[u][e] - ch.mean; ch.m2 += d * d; }
        run = chan(run, ch);
    }
    // lanes: six steps, lane l takes lane l + d for d = 1, 2, .. 32 (the total is lane 0's); waves: thread 0, ascending
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Triple o;
        o.n = __shfl_down(run.n, d);
        o.mean = __shfl_down(run.mean, d);
        o.m2 = __shfl_down(run.m2, d);
        if ((t & 63) + d < 64) run = chan(run, o);
    }
    __shared__ Triple waves[BN_STATS_THREADS / 64];
    if ((t & 63) == 0) waves[t >> 6] = run;
    __syncthreads();
    if (t == 0)
        for (int wv = 1; wv < BN_STATS_THREADS / 64; ++wv) run = chan(run, waves[wv]);
    return run;
}

// merge(.. merge(triple 0, triple 1) .., triple P - 1) of the P triples at tr (LDS or global: the same operations either way)
__device__ __forceinline__ Triple bn_fold_triples(const double* tr, int P) {
    Triple all = {tr[0], tr[1], tr[2]};
    for (int j = 1; j < P; ++j) all = chan(all, Triple{tr[j * 3 + 0], tr[j * 3 + 1], tr[j * 3 + 2]});
    return all;
}

// The scale and the pre-activation value as the forward's apply forms them; the backward kernels recompute both through these same
// expressions (IEEE square root and division: plain sqrtf and / under the build's -fhip-fp32-correctly-rounded-divide-sqrt.  __fsqrt_rn is NOT
// that here: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define it as the native v_sqrt_f32, one float32 spacing off for some arguments).
__device__ __forceinline__ float bn_scale(float gamma, float var, float eps) { return gamma / sqrtf(var + eps); }
__device__ __forceinline__ float bn_affine(float v, float mu, float s, float beta) { return fmaf(v - mu, s, beta); }

// One apply block on the slab a.y / a.skip / a.out with the triples at a.ws [C,P,3]: folds its channel's triples (every thread, the same
// operations), streams its 4096 values.  OWNER: the block with blockIdx.x == 0 also writes the channel's saved and running statistics (the
// ungrouped kernel; the grouped one leaves that to its own fold over the groups).  -> the channel's statistics in `all`.
template <bool OWNER>
__device__ __forceinline__ void bn_apply_block(const ApplyArgs& a, const Walk& w) {
    const int c = blockIdx.y, t = threadIdx.x;
    __shared__ double tr[BN_MAX_PARTIALS][3];
    if (t < a.P * 3) tr[t / 3][t % 3] = a.ws[(size_t)c * (size_t)a.P * 3 + t];
    __syncthreads();
    const Triple all = bn_fold_triples(&tr[0][0], a.P);
    const float mu = (float)all.mean, var = (float)(all.m2 / all.n);
    const float s = bn_scale(a.gamma[c], var, a.eps), beta = a.beta[c];
    if (OWNER && blockIdx.x == 0 && t == 0) {
        const float m = a.momentum, unbiased = (float)(all.m2 / (all.n - 1.0));
        a.saved_mean[c] = mu;
        a.saved_var[c] = var;
        a.running_mean[c] = (1.f - m) * a.running_mean[c] + m * mu;
        a.running_var[c] = (1.f - m) * a.running_var[c] + m * unbiased;
        if (c == 0) *a.num_batches_tracked = *a.num_batches_tracked + 1;
    }
    const unsigned base = blockIdx.x * (unsigned)BN_APPLY_CHUNK;
#pragma unroll
    for (int k = 0; k < BN_APPLY_QUADS; ++k) {
        const unsigned i = base + ((unsigned)k * BN_APPLY_THREADS + (unsigned)t) * 4u;
        if (i >= w.N) break;
        float v[4], sk[4] = {0.f, 0.f, 0.f, 0.f};
        bn_load_quad(a.y, w, c, i, w.N, v);
        if (a.skip) bn_load_quad(a.skip, w, c, i, w.N, sk);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float r = bn_affine(v[e], mu, s, beta);
            if (a.relu) r = r < 0.f ? 0.f : r;             // (a NaN stays)
            v[e] = a.skip ? r + sk[e] : r;
        }
        if (w.vec) {
            *reinterpret_cast<float4*>(a.out + bn_addr(w, c, i)) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < w.N) a.out[bn_addr(w, c, i + e)] = v[e];
        }
    }
}

__device__ __forceinline__ float bn_masked(const BwdArgs& a, float g, float y, float mu, float s, float beta) {
    return (!a.relu || !(bn_affine(y, mu, s, beta) <= 0.f)) ? g : 0.f;
}

// Slice j of channel c of the slabs a.g / a.y -> (sum gm, sum gm (y - mu)) in sa, sb, held by thread 0 on return.  Every thread of the 1024
// calls it (one barrier).
__device__ __forceinline__ void bn_bwd_slice_sums(const BwdArgs& a, const Walk& w, unsigned L, int j, int c, int t, double& sa, double& sb) {
    const unsigned begin = (unsigned)j * L;
    const unsigned end = min(begin + L, w.N);
    const float mu = a.mean[c], beta = a.beta[c], s = bn_scale(a.gamma[c], a.var[c], a.eps);
    sa = 0.0;
    sb = 0.0;
    for (unsigned q0 = 0; begin + q0 * 4u < end; q0 += BN_CHUNK_QUADS * BN_STATS_THREADS) {
        float gv[BN_CHUNK_QUADS][4], yv[BN_CHUNK_QUADS][4];
        unsigned at[BN_CHUNK_QUADS];
#pragma unroll
        for (int u = 0; u < BN_CHUNK_QUADS; ++u) {
            at[u] = begin + (q0 + (unsigned)u * BN_STATS_THREADS + (unsigned)t) * 4u;
            if (at[u] < end) { bn_load_quad(a.g, w, c, at[u], end, gv[u]); bn_load_quad(a.y, w, c, at[u], end, yv[u]); }
        }
#pragma unroll
        for (int u = 0; u < BN_CHUNK_QUADS; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (at[u] < end && at[u] + e < end) {
                    const double gm = (double)bn_masked(a, gv[u][e], yv[u][e], mu, s, beta);
                    sa += gm;
                    sb += gm * ((double)yv[u][e] - (double)mu);
                }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double oa = __shfl_down(sa, d), ob = __shfl_down(sb, d);
        if ((t & 63) + d < 64) { sa += oa; sb += ob; }
    }
    __shared__ double waves[BN_STATS_THREADS / 64][2];
    if ((t & 63) == 0) { waves[t >> 6][0] = sa; waves[t >> 6][1] = sb; }
    __syncthreads();
    if (t == 0)
        for (int wv = 1; wv < BN_STATS_THREADS / 64; ++wv) { sa += waves[wv][0]; sb += waves[wv][1]; }
}

// ((A_0 + A_1) + ...), B likewise, over the P pairs at pr (LDS or global: the same operations either way)
__device__ __forceinline__ void bn_fold_pairs(const double* pr, int P, double& A, double& B) {
    A = pr[0];
    B = pr[1];
    for (int j = 1; j < P; ++j) { A += pr[j * 2 + 0]; B += pr[j * 2 + 1]; }
}

__device__ __forceinline__ double bn_rstd(float var, float eps) { return 1.0 / sqrt((double)var + (double)eps); }

// One backward apply block on the slabs a.g / a.y / dy with the pairs at ws [C,P,2] and the statistics a.mean / a.var [C].  OWNER: the block
// with blockIdx.x == 0 also writes the channel's parameter gradients (the ungrouped kernel).
template <bool OWNER>
__device__ __forceinline__ void bn_bwd_apply_block(const BwdArgs& a, const Walk& w, const double* __restrict__ ws, float* dy, float* __restrict__ dgamma,
                                                   float* __restrict__ dbeta) {
    const int c = blockIdx.y, t = threadIdx.x;
    __shared__ double pr[BN_MAX_PARTIALS][2];
    if (t < a.P * 2) pr[t / 2][t % 2] = ws[(size_t)c * (size_t)a.P * 2 + t];
    __syncthreads();
    double A, B;
    bn_fold_pairs(&pr[0][0], a.P, A, B);                                                         // every thread, the same operations
    const float mu = a.mean[c], beta = a.beta[c], var = a.var[c], s = bn_scale(a.gamma[c], var, a.eps);
    const double r = bn_rstd(var, a.eps), N = (double)w.N;
    const double k1 = A / N, k2 = r * r * B / N, sg = (double)a.gamma[c] * r;
    if (OWNER && blockIdx.x == 0 && t == 0) {
        dbeta[c] = (float)A;
        dgamma[c] = (float)(B * r);
    }
    const unsigned base = blockIdx.x * (unsigned)BN_APPLY_CHUNK;
#pragma unroll
    for (int k = 0; k < BN_APPLY_QUADS; ++k) {
        const unsigned i = base + ((unsigned)k * BN_APPLY_THREADS + (unsigned)t) * 4u;
        if (i >= w.N) break;
        float gv[4], yv[4];
        bn_load_quad(a.g, w, c, i, w.N, gv);
        bn_load_quad(a.y, w, c, i, w.N, yv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double gm = (double)bn_masked(a, gv[e], yv[e], mu, s, beta);
            gv[e] = (float)(sg * ((gm - k1) - ((double)yv[e] - (double)mu) * k2));
        }
        if (w.vec) {
            *reinterpret_cast<float4*>(dy + bn_addr(w, c, i)) = make_float4(gv[0], gv[1], gv[2], gv[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < w.N) dy[bn_addr(w, c, i + e)] = gv[e];
        }
    }
}
#endif  // __HIPCC__

// ---- host: the checks both files make before any device call
inline int bn_shape(const char* who, int64_t n, int64_t C, int64_t S, int64_t* N) {
    UCNERF_REQUIRE(n >= 1 && C >= 1 && S >= 1, "%s: n=%lld C=%lld S=%lld (all at least 1)", who, (long long)n, (long long)C, (long long)S);
    UCNERF_REQUIRE(n <= BN_MAX_COUNT && S <= BN_MAX_COUNT && n * S <= BN_MAX_COUNT, "%s: n S = %lld x %lld values per channel, at most %lld", who,
                   (long long)n, (long long)S, (long long)BN_MAX_COUNT);
    UCNERF_REQUIRE(C <= 65535 && n * S <= (1ll << 62) / C, "%s: C=%lld (at most 65535) or n C S overflows", who, (long long)C);
    *N = n * S;
    UCNERF_REQUIRE(*N >= 2, "%s: %lld value per channel, the batch statistics need at least 2", who, (long long)*N);
    return UCNERF_OK;
}

inline int64_t bn_partials(int64_t N) { const int64_t p = (N + BN_MIN_SLICE - 1) / BN_MIN_SLICE; return p < BN_MAX_PARTIALS ? p : BN_MAX_PARTIALS; }
inline int64_t bn_slice(int64_t N, int64_t P) { return ((N + P - 1) / P + 3) / 4 * 4; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline Walk bn_walk(int64_t C, int64_t S, int64_t N, bool vec) {
    Walk w;
    w.C = C; w.S = S; w.N = (unsigned)N; w.S32 = (unsigned)S;
    w.vec = vec;
    return w;
}

}  // namespace
}  // namespace ucnerf
