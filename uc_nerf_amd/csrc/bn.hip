// Train-mode batch-norm for the MVS CNNs (include/ucnerf_hip.h, "batch-statistic batch-norm" and "grouped batch-statistic batch-norm"): the
// statistics of the batch itself, the normalise / ReLU / skip epilogue, the running-statistic update, and the backward of all that.  y is
// [G,n,C,S]: group q is the images q n .. q n + n - 1 and is normalised with its OWN statistics.  ONE code path: the ungrouped entry points are
// G = 1 of the grouped ones (their structs copied behind G = 1), and what a group computes never depends on G.  Two launches forward, two
// backward, nothing read back, no atomics.
//
//   stats        grid (P, C, G), 1024 threads: block (j, c, q) reduces slice j of channel c of group q to one float64 triple (count, mean, M2).
//   apply        grid (ceil(N / 4096), C, G), 256 threads: block (x, c, q) folds the P triples of (q, c) itself (the same operations in the
//                same order in every block, so all of them hold the same mu and sigma^2), then streams 4096 values of group q.  Block (0, c, q)
//                writes saved_mean / saved_var [q, c] from that fold.  Block (0, c, 0) moves the running statistics G times, q ascending, as G
//                successive calls would: with its own fold for q = 0 and, only where G > 1, thread q's fold of group q's triples for the rest.
//   bwd reduce   grid (P, C, G), 1024 threads: block (j, c, q) -> the float64 pair (sum gm, sum gm (y - mu)) of its slice.
//   bwd apply    grid (ceil(N / 4096), C, G), 256 threads: folds the pairs of (q, c), streams grad_y.  Block (0, c, 0) writes the parameter
//                gradients: float64 sums over the groups, q ascending (its own fold, then thread q's where G > 1), rounded once.
//
// Within a group a channel's N = n S values are numbered i = img * S + offset.  Everything walks them in QUADS of four consecutive i; where S is
// a multiple of four and the arrays are 16-byte aligned a quad is one 16-byte access, otherwise four scalar ones -- the values and the order of
// every sum are the same either way.  Every intermediate of the statistics is float64: a float32 slice mean at |mean| >> sigma would put its own
// rounding, squared and multiplied by the count, into M2.  The build compiles with -ffp-contract=off and correctly rounded division and square
// root, so equal expressions give equal bits.
#include "common.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

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
constexpr int BN_MAX_GROUPS = 64;                        // G: one thread of an apply block per group

struct Triple { double n, mean, m2; };

struct Walk {                      // where the values of one channel of one group lie
    int64_t C, S;                  // address of value i of channel c: ((i / S) * C + c) * S + i % S in the group's slab
    size_t slab;                   // floats per group: n C S
    unsigned N, S32;
    int vec;                       // 1: S % 4 == 0 and every array 16-byte aligned (then every group base is: a slab is a multiple of four floats)
    int G;
};

struct ApplyArgs {
    const float *y, *skip, *gamma, *beta;
    float *out, *saved_mean, *saved_var, *running_mean, *running_var;
    long long* num_batches_tracked;
    const double* ws;              // [G,C,P,3]
    float eps, momentum;
    int P, relu;
};

// gm = g where the forward's ReLU let the value through (z = bn_affine(y, mu, s, beta), the mask is !(z <= 0): torch's threshold rule), else 0.
struct BwdArgs {
    const float *g, *y, *mean, *var, *gamma, *beta;        // mean, var [G,C]
    float eps;
    int relu, P;
};

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

__device__ __forceinline__ float bn_masked(const BwdArgs& a, float g, float y, float mu, float s, float beta) {
    return (!a.relu || !(bn_affine(y, mu, s, beta) <= 0.f)) ? g : 0.f;
}

// ((A_0 + A_1) + ...), B likewise, over the P pairs at pr (LDS or global: the same operations either way)
__device__ __forceinline__ void bn_fold_pairs(const double* pr, int P, double& A, double& B) {
    A = pr[0];
    B = pr[1];
    for (int j = 1; j < P; ++j) { A += pr[j * 2 + 0]; B += pr[j * 2 + 1]; }
}

__device__ __forceinline__ double bn_rstd(float var, float eps) { return 1.0 / sqrt((double)var + (double)eps); }

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

__global__ __launch_bounds__(BN_STATS_THREADS) void bn_stats_kernel(const float* __restrict__ y, Walk w, unsigned L, int P, double* __restrict__ ws) {
    const int j = blockIdx.x, c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    const Triple run = bn_slice_triple(y + (size_t)q * w.slab, w, L, j, c, t);
    if (t == 0) {
        double* o = ws + (((size_t)q * (size_t)w.C + (size_t)c) * (size_t)P + (size_t)j) * 3;
        o[0] = run.n; o[1] = run.mean; o[2] = run.m2;
    }
}

__global__ __launch_bounds__(BN_APPLY_THREADS) void bn_apply_kernel(ApplyArgs a, Walk w) {
    const int c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    const size_t C = (size_t)w.C, P = (size_t)a.P, slab = (size_t)q * w.slab;
    // G > 1 is marked unlikely at every branch so that its code lies out of line and G = 1 falls straight through: an owner block of a small layer is bound by
    // latency, and every jump over code that does not run is an instruction fetch it waits for
    const bool many = w.G > 1;
    __shared__ double tr[BN_MAX_PARTIALS][3];
    if (t < a.P * 3) tr[t / 3][t % 3] = a.ws[((size_t)q * C + (size_t)c) * P * 3 + t];
    __syncthreads();
    const Triple all = bn_fold_triples(&tr[0][0], a.P);    // every thread, the same operations
    const float mu = (float)all.mean, var = (float)(all.m2 / all.n);
    const float s = bn_scale(a.gamma[c], var, a.eps), beta = a.beta[c];
    if (blockIdx.x == 0) {                                 // the statistics (the triples are the stats launch's: nothing of this launch is read)
        if (t == 0) {
            a.saved_mean[(size_t)q * C + c] = mu;
            a.saved_var[(size_t)q * C + c] = var;
        }
        if (q == 0) {
            __shared__ float mean_of[BN_MAX_GROUPS], unbiased_of[BN_MAX_GROUPS];
            if (__builtin_expect(many, 0)) {     // the other groups' statistics: thread k folds group k's triples as that group's blocks do
                if (t >= 1 && t < w.G) {
                    const Triple other = bn_fold_triples(a.ws + ((size_t)t * C + (size_t)c) * P * 3, a.P);
                    mean_of[t] = (float)other.mean;
                    unbiased_of[t] = (float)(other.m2 / (other.n - 1.0));
                }
                __syncthreads();
            }
            if (t == 0) {
                const float m = a.momentum;
                float rm = (1.f - m) * a.running_mean[c] + m * mu;
                float rv = (1.f - m) * a.running_var[c] + m * (float)(all.m2 / (all.n - 1.0));
                if (__builtin_expect(many, 0))
                    for (int k = 1; k < w.G; ++k) {
                        rm = (1.f - m) * rm + m * mean_of[k];
                        rv = (1.f - m) * rv + m * unbiased_of[k];
                    }
                a.running_mean[c] = rm;
                a.running_var[c] = rv;
                if (c == 0) *a.num_batches_tracked = *a.num_batches_tracked + w.G;
            }
        }
    }
    const float* y = a.y + slab;
    const float* skip = a.skip ? a.skip + slab : nullptr;
    float* out = a.out + slab;
    const unsigned base = blockIdx.x * (unsigned)BN_APPLY_CHUNK;
#pragma unroll
    for (int k = 0; k < BN_APPLY_QUADS; ++k) {
        const unsigned i = base + ((unsigned)k * BN_APPLY_THREADS + (unsigned)t) * 4u;
        if (i >= w.N) break;
        float v[4], sk[4] = {0.f, 0.f, 0.f, 0.f};
        bn_load_quad(y, w, c, i, w.N, v);
        if (skip) bn_load_quad(skip, w, c, i, w.N, sk);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float r = bn_affine(v[e], mu, s, beta);
            if (a.relu) r = r < 0.f ? 0.f : r;             // (a NaN stays)
            v[e] = skip ? r + sk[e] : r;
        }
        if (w.vec) {
            *reinterpret_cast<float4*>(out + bn_addr(w, c, i)) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < w.N) out[bn_addr(w, c, i + e)] = v[e];
        }
    }
}

// ---- backward: the same slices and quads as the forward pair, a float64 workspace [G,C,P,2]
__device__ __forceinline__ BwdArgs bn_group_args(const BwdArgs& a, const Walk& w, int q) {
    BwdArgs mine = a;                                      // group q's slabs and its statistics [C]
    mine.g = a.g + (size_t)q * w.slab;
    mine.y = a.y + (size_t)q * w.slab;
    mine.mean = a.mean + (size_t)q * (size_t)w.C;
    mine.var = a.var + (size_t)q * (size_t)w.C;
    return mine;
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

__global__ __launch_bounds__(BN_STATS_THREADS) void bn_bwd_reduce_kernel(BwdArgs a, Walk w, unsigned L, double* __restrict__ ws) {
    const int j = blockIdx.x, c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    double sa, sb;
    bn_bwd_slice_sums(bn_group_args(a, w, q), w, L, j, c, t, sa, sb);
    if (t == 0) {
        double* o = ws + (((size_t)q * (size_t)w.C + (size_t)c) * (size_t)a.P + (size_t)j) * 2;
        o[0] = sa; o[1] = sb;
    }
}

__global__ __launch_bounds__(BN_APPLY_THREADS) void bn_bwd_apply_kernel(BwdArgs all, Walk w, const double* __restrict__ ws, float* dy, float* __restrict__ dgamma,
                                                                        float* __restrict__ dbeta) {
    const int c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    const size_t C = (size_t)w.C, P = (size_t)all.P;
    const bool many = w.G > 1;                            // (marked unlikely at every branch, as in bn_apply_kernel)
    const BwdArgs a = bn_group_args(all, w, q);
    dy += (size_t)q * w.slab;
    __shared__ double pr[BN_MAX_PARTIALS][2];
    if (t < a.P * 2) pr[t / 2][t % 2] = ws[((size_t)q * C + (size_t)c) * P * 2 + t];
    __syncthreads();
    double A, B;
    bn_fold_pairs(&pr[0][0], a.P, A, B);                                                         // every thread, the same operations
    const float mu = a.mean[c], beta = a.beta[c], var = a.var[c], s = bn_scale(a.gamma[c], var, a.eps);
    const double r = bn_rstd(var, a.eps), N = (double)w.N;
    const double k1 = A / N, k2 = r * r * B / N, sg = (double)a.gamma[c] * r;
    if (blockIdx.x == 0 && q == 0) {                       // the channel's parameter gradients: float64 sums over the groups, q ascending, rounded once
        __shared__ double bias_of[BN_MAX_GROUPS], weight_of[BN_MAX_GROUPS];
        if (__builtin_expect(many, 0)) {     // the other groups' terms: thread k folds group k's pairs as that group's blocks do
            if (t >= 1 && t < w.G) {
                double Ak, Bk;
                bn_fold_pairs(ws + ((size_t)t * C + (size_t)c) * P * 2, a.P, Ak, Bk);
                bias_of[t] = Ak;
                weight_of[t] = Bk * bn_rstd(all.var[(size_t)t * C + c], a.eps);
            }
            __syncthreads();
        }
        if (t == 0) {
            double Asum = A, Brsum = B * r;
            if (__builtin_expect(many, 0))
                for (int k = 1; k < w.G; ++k) { Asum += bias_of[k]; Brsum += weight_of[k]; }
            dbeta[c] = (float)Asum;
            dgamma[c] = (float)Brsum;
        }
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

// ---- host: every check before any device call, once for both families of entry points (`who` names the one that was called)
int64_t bn_partials(int64_t N) { const int64_t p = (N + BN_MIN_SLICE - 1) / BN_MIN_SLICE; return p < BN_MAX_PARTIALS ? p : BN_MAX_PARTIALS; }
int64_t bn_slice(int64_t N, int64_t P) { return ((N + P - 1) / P + 3) / 4 * 4; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// G, then the slab's shape, then the products over the groups -> N = n S and P
template <class Params>
int bn_shape(const char* who, const Params& p, int64_t* N, int64_t* P) {
    const int64_t G = p.G, n = p.n, C = p.C, S = p.S;
    UCNERF_REQUIRE(G >= 1 && G <= BN_MAX_GROUPS, "%s: G=%lld (from 1 to %d groups)", who, (long long)G, BN_MAX_GROUPS);
    UCNERF_REQUIRE(n >= 1 && C >= 1 && S >= 1, "%s: n=%lld C=%lld S=%lld (all at least 1)", who, (long long)n, (long long)C, (long long)S);
    UCNERF_REQUIRE(n <= BN_MAX_COUNT && S <= BN_MAX_COUNT && n * S <= BN_MAX_COUNT, "%s: n S = %lld x %lld values per channel, at most %lld", who,
                   (long long)n, (long long)S, (long long)BN_MAX_COUNT);
    UCNERF_REQUIRE(C <= 65535 && n * S <= (1ll << 62) / C, "%s: C=%lld (at most 65535) or n C S overflows", who, (long long)C);
    *N = n * S;
    UCNERF_REQUIRE(*N >= 2, "%s: %lld value per channel, the batch statistics need at least 2", who, (long long)*N);
    UCNERF_REQUIRE(G * *N <= BN_MAX_COUNT, "%s: G n S = %lld x %lld values per channel over all groups, at most %lld", who, (long long)G, (long long)*N,
                   (long long)BN_MAX_COUNT);
    UCNERF_REQUIRE(*N * C <= (1ll << 62) / G, "%s: G n C S overflows", who);
    *P = bn_partials(*N);
    return UCNERF_OK;                                      // (G C P <= 64 x 65535 x 32: no overflow)
}

template <class Params>
Walk bn_walk(const Params& p, int64_t N, bool vec) {
    Walk w;
    w.C = p.C; w.S = p.S; w.slab = (size_t)p.n * (size_t)p.C * (size_t)p.S; w.N = (unsigned)N; w.S32 = (unsigned)p.S;
    w.vec = p.S % 4 == 0 && vec;
    w.G = (int)p.G;
    return w;
}

int bn_stats(const char* who, const ucnerf_bn_stats_groups_params& p, void* stream) {
    int64_t N, P;
    if (int rc = bn_shape(who, p, &N, &P)) return rc;
    UCNERF_REQUIRE(p.y && p.workspace, "%s: null y or workspace", who);
    UCNERF_REQUIRE(p.workspace_triples >= p.G * p.C * P, "%s: the workspace holds %lld triples, G C P = %lld x %lld x %lld are written", who,
                   (long long)p.workspace_triples, (long long)p.G, (long long)p.C, (long long)P);
    UCNERF_REQUIRE(((uintptr_t)p.workspace & 7) == 0, "%s: the workspace is not 8-byte aligned", who);
    const Walk w = bn_walk(p, N, aligned16(p.y));
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)P, (unsigned)p.C, (unsigned)p.G), dim3(BN_STATS_THREADS), 0, (hipStream_t)stream, p.y, w,
                       (unsigned)bn_slice(N, P), (int)P, p.workspace);
    return check_launch(who);
}

int bn_apply(const char* who, const ucnerf_bn_apply_groups_params& p, void* stream) {
    int64_t N, P;
    if (int rc = bn_shape(who, p, &N, &P)) return rc;
    UCNERF_REQUIRE(p.y && p.out && p.workspace && p.weight && p.bias, "%s: null y, out, workspace, weight or bias", who);
    UCNERF_REQUIRE(p.saved_mean && p.saved_var && p.running_mean && p.running_var && p.num_batches_tracked,
                   "%s: null saved_mean, saved_var, running_mean, running_var or num_batches_tracked", who);
    UCNERF_REQUIRE(p.eps > 0.f, "%s: eps=%g (must be positive)", who, (double)p.eps);                      // (a NaN fails both)
    UCNERF_REQUIRE(p.momentum > 0.f && p.momentum <= 1.f, "%s: momentum=%g (must lie in (0, 1])", who, (double)p.momentum);
    UCNERF_REQUIRE(p.workspace_triples >= p.G * p.C * P, "%s: the workspace holds %lld triples, G C P = %lld x %lld x %lld are read", who,
                   (long long)p.workspace_triples, (long long)p.G, (long long)p.C, (long long)P);
    UCNERF_REQUIRE(((uintptr_t)p.workspace & 7) == 0 && ((uintptr_t)p.num_batches_tracked & 7) == 0, "%s: workspace or num_batches_tracked not 8-byte aligned", who);
    const Walk w = bn_walk(p, N, aligned16(p.y) && aligned16(p.out) && (!p.skip || aligned16(p.skip)));
    ApplyArgs a;
    a.y = p.y; a.skip = p.skip; a.gamma = p.weight; a.beta = p.bias; a.out = p.out;
    a.saved_mean = p.saved_mean; a.saved_var = p.saved_var; a.running_mean = p.running_mean; a.running_var = p.running_var;
    a.num_batches_tracked = reinterpret_cast<long long*>(p.num_batches_tracked);
    a.ws = p.workspace; a.eps = p.eps; a.momentum = p.momentum; a.P = (int)P; a.relu = p.relu != 0;
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((N + BN_APPLY_CHUNK - 1) / BN_APPLY_CHUNK), (unsigned)p.C, (unsigned)p.G), dim3(BN_APPLY_THREADS), 0,
                       (hipStream_t)stream, a, w);
    return check_launch(who);
}

// what the two backward launches check alike (their structs share every field up to the workspace) -> N, P and the kernels' arguments
template <class Params>
int bn_bwd_args(const char* who, const Params& p, int64_t* N, BwdArgs* a) {
    int64_t P;
    if (int rc = bn_shape(who, p, N, &P)) return rc;
    UCNERF_REQUIRE(p.g && p.y && p.saved_mean && p.saved_var && p.weight && p.bias && p.workspace, "%s: null g, y, saved_mean, saved_var, weight, bias or workspace", who);
    UCNERF_REQUIRE(p.eps > 0.f, "%s: eps=%g (must be positive)", who, (double)p.eps);
    UCNERF_REQUIRE(p.workspace_pairs >= p.G * p.C * P, "%s: the workspace holds %lld pairs, G C P = %lld x %lld x %lld are used", who, (long long)p.workspace_pairs,
                   (long long)p.G, (long long)p.C, (long long)P);
    UCNERF_REQUIRE(((uintptr_t)p.workspace & 7) == 0, "%s: the workspace is not 8-byte aligned", who);
    a->g = p.g; a->y = p.y; a->mean = p.saved_mean; a->var = p.saved_var; a->gamma = p.weight; a->beta = p.bias; a->eps = p.eps; a->relu = p.relu != 0; a->P = (int)P;
    return UCNERF_OK;
}

int bn_bwd_reduce(const char* who, const ucnerf_bn_bwd_reduce_groups_params& p, void* stream) {
    int64_t N;
    BwdArgs a;
    if (int rc = bn_bwd_args(who, p, &N, &a)) return rc;
    const Walk w = bn_walk(p, N, aligned16(p.g) && aligned16(p.y));
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((unsigned)a.P, (unsigned)p.C, (unsigned)p.G), dim3(BN_STATS_THREADS), 0, (hipStream_t)stream, a, w,
                       (unsigned)bn_slice(N, a.P), p.workspace);
    return check_launch(who);
}

int bn_bwd_apply(const char* who, const ucnerf_bn_bwd_apply_groups_params& p, void* stream) {
    int64_t N;
    BwdArgs a;
    if (int rc = bn_bwd_args(who, p, &N, &a)) return rc;
    UCNERF_REQUIRE(p.grad_y && p.grad_weight && p.grad_bias, "%s: null grad_y, grad_weight or grad_bias", who);
    const Walk w = bn_walk(p, N, aligned16(p.g) && aligned16(p.y) && aligned16(p.grad_y));
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((N + BN_APPLY_CHUNK - 1) / BN_APPLY_CHUNK), (unsigned)p.C, (unsigned)p.G), dim3(BN_APPLY_THREADS), 0,
                       (hipStream_t)stream, a, w, p.workspace, p.grad_y, p.grad_weight, p.grad_bias);
    return check_launch(who);
}

// An ungrouped struct behind G = 1: the grouped struct is G followed by exactly the ungrouped fields.  The copy runs over the members from n on
// and relies on that correspondence field by field; the assertion below sees only offset and size, the fields themselves are compared in
// tests/test_feature_views_host.py (the ctypes mirrors' _fields_ and ucnerf_sizeof) -- a reorder in the header has to keep both structs alike.
template <class Grouped, class Plain>
Grouped one_group(const Plain& p) {
    static_assert(offsetof(Grouped, n) == sizeof(int64_t) && sizeof(Grouped) == sizeof(int64_t) + sizeof(Plain), "the grouped struct is G, then the ungrouped fields");
    Grouped g;
    g.G = 1;
    std::memcpy(&g.n, &p, sizeof(Plain));
    return g;
}

}  // namespace
}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int64_t ucnerf_bn_partials(int64_t n, int64_t S) {
    if (n < 1 || S < 1 || n > BN_MAX_COUNT || S > BN_MAX_COUNT || n * S > BN_MAX_COUNT || n * S < 2) return -1;
    return bn_partials(n * S);
}

int ucnerf_bn_stats(const ucnerf_bn_stats_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_stats: null params");
    return bn_stats("bn_stats", one_group<ucnerf_bn_stats_groups_params>(*p), stream);
}

int ucnerf_bn_apply(const ucnerf_bn_apply_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_apply: null params");
    return bn_apply("bn_apply", one_group<ucnerf_bn_apply_groups_params>(*p), stream);
}

int ucnerf_bn_bwd_reduce(const ucnerf_bn_bwd_reduce_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_reduce: null params");
    return bn_bwd_reduce("bn_bwd_reduce", one_group<ucnerf_bn_bwd_reduce_groups_params>(*p), stream);
}

int ucnerf_bn_bwd_apply(const ucnerf_bn_bwd_apply_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_apply: null params");
    return bn_bwd_apply("bn_bwd_apply", one_group<ucnerf_bn_bwd_apply_groups_params>(*p), stream);
}

int ucnerf_bn_stats_groups(const ucnerf_bn_stats_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_stats_groups: null params");
    return bn_stats("bn_stats_groups", *p, stream);
}

int ucnerf_bn_apply_groups(const ucnerf_bn_apply_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_apply_groups: null params");
    return bn_apply("bn_apply_groups", *p, stream);
}

int ucnerf_bn_bwd_reduce_groups(const ucnerf_bn_bwd_reduce_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_reduce_groups: null params");
    return bn_bwd_reduce("bn_bwd_reduce_groups", *p, stream);
}

int ucnerf_bn_bwd_apply_groups(const ucnerf_bn_bwd_apply_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_apply_groups: null params");
    return bn_bwd_apply("bn_bwd_apply_groups", *p, stream);
}

}  // extern "C"
