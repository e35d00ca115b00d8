// Batch-norm with the statistics kept PER GROUP OF IMAGES (include/ucnerf_hip.h, "grouped batch-statistic batch-norm"): y [G,n,C,S], group q the
// images q n .. q n + n - 1, every group normalised with its own batch statistics -- what G calls of bn.hip's entry points on the G slabs [n,C,S]
// compute, bit for bit, in one launch each.  FeatureNet over all the views of a sample in one pass is the user: the reference's batch-norm sees
// one view at a time.
//
//   ucnerf_bn_stats_groups        grid (P, C, G), 1024 threads: block (j, c, q) reduces slice j of channel c of group q.
//   ucnerf_bn_apply_groups        grid (ceil(N / 4096), C, G), 256 threads: block (x, c, q) folds the P triples of (q, c) and streams 4096 values
//                                 of group q.  Block (0, c, 0) also owns channel c's statistics: thread q < G folds group q's triples (the same
//                                 operations as every block of that group) and writes saved_mean / saved_var [q, c]; then thread 0 moves the
//                                 running statistics G times, q ascending, as G successive calls would.
//   ucnerf_bn_bwd_reduce_groups   grid (P, C, G), 1024 threads.
//   ucnerf_bn_bwd_apply_groups    grid (ceil(N / 4096), C, G), 256 threads; block (0, c, 0) sums the groups' parameter gradients in float64.
//
// A block's arithmetic is bn_device.h's, on base pointers moved to its group's slab: nothing of the per-group order is restated here.
#include "bn_device.h"

namespace ucnerf {
namespace {

struct Groups {
    int G;
    size_t slab;                   // floats per group: n C S
};

__global__ __launch_bounds__(BN_STATS_THREADS) void bn_stats_groups_kernel(const float* __restrict__ y, Walk w, unsigned L, int P, Groups gr, double* __restrict__ ws) {
    const int j = blockIdx.x, c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    const Triple run = bn_slice_triple(y + (size_t)q * gr.slab, w, L, j, c, t);
    if (t == 0) {
        double* o = ws + (((size_t)q * (size_t)w.C + (size_t)c) * (size_t)P + (size_t)j) * 3;
        o[0] = run.n; o[1] = run.mean; o[2] = run.m2;
    }
}

__global__ __launch_bounds__(BN_APPLY_THREADS) void bn_apply_groups_kernel(ApplyArgs a, Walk w, Groups gr) {
    const int c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    const size_t C = (size_t)w.C, P = (size_t)a.P;
    ApplyArgs mine = a;                                    // group q's slab and its triples [C,P,3]
    mine.y = a.y + (size_t)q * gr.slab;
    mine.skip = a.skip ? a.skip + (size_t)q * gr.slab : nullptr;
    mine.out = a.out + (size_t)q * gr.slab;
    mine.ws = a.ws + (size_t)q * C * P * 3;
    if (blockIdx.x == 0 && q == 0) {                       // the channel's statistics, all groups (the triples are the stats launch's: nothing of this launch is read)
        __shared__ float mean_of[BN_MAX_GROUPS], unbiased_of[BN_MAX_GROUPS];
        if (t < gr.G) {
            const Triple all = bn_fold_triples(a.ws + ((size_t)t * C + (size_t)c) * P * 3, a.P);
            const float mu = (float)all.mean, var = (float)(all.m2 / all.n);
            a.saved_mean[(size_t)t * C + c] = mu;
            a.saved_var[(size_t)t * C + c] = var;
            mean_of[t] = mu;
            unbiased_of[t] = (float)(all.m2 / (all.n - 1.0));
        }
        __syncthreads();
        if (t == 0) {
            const float m = a.momentum;
            float rm = a.running_mean[c], rv = a.running_var[c];
            for (int k = 0; k < gr.G; ++k) {
                rm = (1.f - m) * rm + m * mean_of[k];
                rv = (1.f - m) * rv + m * unbiased_of[k];
            }
            a.running_mean[c] = rm;
            a.running_var[c] = rv;
            if (c == 0) *a.num_batches_tracked = *a.num_batches_tracked + gr.G;
        }
    }
    bn_apply_block<false>(mine, w);
}

__device__ __forceinline__ BwdArgs bn_group_args(const BwdArgs& a, const Walk& w, const Groups& gr, int q) {
    BwdArgs mine = a;                                      // group q's slabs and its statistics [C]
    mine.g = a.g + (size_t)q * gr.slab;
    mine.y = a.y + (size_t)q * gr.slab;
    mine.mean = a.mean + (size_t)q * (size_t)w.C;
    mine.var = a.var + (size_t)q * (size_t)w.C;
    return mine;
}

__global__ __launch_bounds__(BN_STATS_THREADS) void bn_bwd_reduce_groups_kernel(BwdArgs a, Walk w, unsigned L, Groups gr, double* __restrict__ ws) {
    const int j = blockIdx.x, c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    const BwdArgs mine = bn_group_args(a, w, gr, q);
    double sa, sb;
    bn_bwd_slice_sums(mine, w, L, j, c, t, sa, sb);
    if (t == 0) {
        double* o = ws + (((size_t)q * (size_t)w.C + (size_t)c) * (size_t)a.P + (size_t)j) * 2;
        o[0] = sa; o[1] = sb;
    }
}

__global__ __launch_bounds__(BN_APPLY_THREADS) void bn_bwd_apply_groups_kernel(BwdArgs a, Walk w, Groups gr, const double* __restrict__ ws, float* dy,
                                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.y, q = blockIdx.z, t = threadIdx.x;
    const size_t C = (size_t)w.C, P = (size_t)a.P;
    if (blockIdx.x == 0 && q == 0) {                       // the channel's parameter gradients: float64 sums over the groups, q ascending, rounded once
        __shared__ double bias_of[BN_MAX_GROUPS], weight_of[BN_MAX_GROUPS];
        if (t < gr.G) {
            double A, B;
            bn_fold_pairs(ws + ((size_t)t * C + (size_t)c) * P * 2, a.P, A, B);
            bias_of[t] = A;
            weight_of[t] = B * bn_rstd(a.var[(size_t)t * C + c], a.eps);
        }
        __syncthreads();
        if (t == 0) {
            double A = bias_of[0], Br = weight_of[0];
            for (int k = 1; k < gr.G; ++k) { A += bias_of[k]; Br += weight_of[k]; }
            dbeta[c] = (float)A;
            dgamma[c] = (float)Br;
        }
    }
    const BwdArgs mine = bn_group_args(a, w, gr, q);
    bn_bwd_apply_block<false>(mine, w, ws + (size_t)q * C * P * 2, dy + (size_t)q * gr.slab, nullptr, nullptr);
}

// G, then the slab's shape as the ungrouped entries check it, then the products over the groups
int bn_groups_shape(const char* who, int64_t G, int64_t n, int64_t C, int64_t S, int64_t* N, int64_t* P) {
    UCNERF_REQUIRE(G >= 1 && G <= BN_MAX_GROUPS, "%s: G=%lld (from 1 to %d groups)", who, (long long)G, BN_MAX_GROUPS);
    if (int rc = bn_shape(who, n, C, S, N)) return rc;
    UCNERF_REQUIRE(G * *N <= BN_MAX_COUNT, "%s: G n S = %lld x %lld values per channel over all groups, at most %lld", who, (long long)G, (long long)*N,
                   (long long)BN_MAX_COUNT);
    UCNERF_REQUIRE(*N * C <= (1ll << 62) / G, "%s: G n C S overflows", who);
    *P = bn_partials(*N);
    return UCNERF_OK;                                      // (G C P <= 64 x 65535 x 32: no overflow)
}

Groups bn_groups(int64_t G, int64_t n, int64_t C, int64_t S) {
    Groups gr;
    gr.G = (int)G;
    gr.slab = (size_t)n * (size_t)C * (size_t)S;
    return gr;
}

int bn_bwd_groups_common(const char* who, int64_t G, int64_t n, int64_t C, int64_t S, int64_t pairs, float eps, const void* g, const void* y, const void* mean,
                         const void* var, const void* gamma, const void* beta, const void* ws, int64_t* N, int64_t* P) {
    if (int rc = bn_groups_shape(who, G, n, C, S, N, P)) return rc;
    UCNERF_REQUIRE(g && y && mean && var && gamma && beta && ws, "%s: null g, y, saved_mean, saved_var, weight, bias or workspace", who);
    UCNERF_REQUIRE(eps > 0.f, "%s: eps=%g (must be positive)", who, (double)eps);
    UCNERF_REQUIRE(pairs >= G * C * *P, "%s: the workspace holds %lld pairs, G C P = %lld x %lld x %lld are used", who, (long long)pairs, (long long)G, (long long)C,
                   (long long)*P);
    UCNERF_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: the workspace is not 8-byte aligned", who);
    return UCNERF_OK;
}

BwdArgs bn_bwd_args(const float* g, const float* y, const float* mean, const float* var, const float* gamma, const float* beta, float eps, int relu, int64_t P) {
    BwdArgs a;
    a.g = g; a.y = y; a.mean = mean; a.var = var; a.gamma = gamma; a.beta = beta; a.eps = eps; a.relu = relu != 0; a.P = (int)P;
    return a;
}

}  // namespace
}  // namespace ucnerf

using namespace ucnerf;

extern "C" {

int ucnerf_bn_stats_groups(const ucnerf_bn_stats_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_stats_groups: null params");
    int64_t N, P;
    if (int rc = bn_groups_shape("bn_stats_groups", p->G, p->n, p->C, p->S, &N, &P)) return rc;
    UCNERF_REQUIRE(p->y && p->workspace, "bn_stats_groups: null y or workspace");
    UCNERF_REQUIRE(p->workspace_triples >= p->G * p->C * P, "bn_stats_groups: the workspace holds %lld triples, G C P = %lld x %lld x %lld are written",
                   (long long)p->workspace_triples, (long long)p->G, (long long)p->C, (long long)P);
    UCNERF_REQUIRE(((uintptr_t)p->workspace & 7) == 0, "bn_stats_groups: the workspace is not 8-byte aligned");
    // (a group starts at q n C S floats: with S % 4 == 0 every group base is as aligned as the array's)
    const Walk w = bn_walk(p->C, p->S, N, p->S % 4 == 0 && aligned16(p->y));
    hipLaunchKernelGGL(bn_stats_groups_kernel, dim3((unsigned)P, (unsigned)p->C, (unsigned)p->G), dim3(BN_STATS_THREADS), 0, (hipStream_t)stream, p->y, w,
                       (unsigned)bn_slice(N, P), (int)P, bn_groups(p->G, p->n, p->C, p->S), p->workspace);
    return check_launch("bn_stats_groups");
}

int ucnerf_bn_apply_groups(const ucnerf_bn_apply_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_apply_groups: null params");
    int64_t N, P;
    if (int rc = bn_groups_shape("bn_apply_groups", p->G, p->n, p->C, p->S, &N, &P)) return rc;
    UCNERF_REQUIRE(p->y && p->out && p->workspace && p->weight && p->bias, "bn_apply_groups: null y, out, workspace, weight or bias");
    UCNERF_REQUIRE(p->saved_mean && p->saved_var && p->running_mean && p->running_var && p->num_batches_tracked,
                   "bn_apply_groups: null saved_mean, saved_var, running_mean, running_var or num_batches_tracked");
    UCNERF_REQUIRE(p->eps > 0.f, "bn_apply_groups: eps=%g (must be positive)", (double)p->eps);             // (a NaN fails both)
    UCNERF_REQUIRE(p->momentum > 0.f && p->momentum <= 1.f, "bn_apply_groups: momentum=%g (must lie in (0, 1])", (double)p->momentum);
    UCNERF_REQUIRE(p->workspace_triples >= p->G * p->C * P, "bn_apply_groups: the workspace holds %lld triples, G C P = %lld x %lld x %lld are read",
                   (long long)p->workspace_triples, (long long)p->G, (long long)p->C, (long long)P);
    UCNERF_REQUIRE(((uintptr_t)p->workspace & 7) == 0 && ((uintptr_t)p->num_batches_tracked & 7) == 0,
                   "bn_apply_groups: workspace or num_batches_tracked not 8-byte aligned");
    const Walk w = bn_walk(p->C, p->S, N, p->S % 4 == 0 && aligned16(p->y) && aligned16(p->out) && (!p->skip || aligned16(p->skip)));
    ApplyArgs a;
    a.y = p->y; a.skip = p->skip; a.gamma = p->weight; a.beta = p->bias; a.out = p->out;
    a.saved_mean = p->saved_mean; a.saved_var = p->saved_var; a.running_mean = p->running_mean; a.running_var = p->running_var;
    a.num_batches_tracked = reinterpret_cast<long long*>(p->num_batches_tracked);
    a.ws = p->workspace; a.eps = p->eps; a.momentum = p->momentum; a.P = (int)P; a.relu = p->relu != 0;
    hipLaunchKernelGGL(bn_apply_groups_kernel, dim3((unsigned)((N + BN_APPLY_CHUNK - 1) / BN_APPLY_CHUNK), (unsigned)p->C, (unsigned)p->G), dim3(BN_APPLY_THREADS), 0,
                       (hipStream_t)stream, a, w, bn_groups(p->G, p->n, p->C, p->S));
    return check_launch("bn_apply_groups");
}

int ucnerf_bn_bwd_reduce_groups(const ucnerf_bn_bwd_reduce_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_reduce_groups: null params");
    int64_t N, P;
    if (int rc = bn_bwd_groups_common("bn_bwd_reduce_groups", p->G, p->n, p->C, p->S, p->workspace_pairs, p->eps, p->g, p->y, p->saved_mean, p->saved_var, p->weight,
                                      p->bias, p->workspace, &N, &P))
        return rc;
    const Walk w = bn_walk(p->C, p->S, N, p->S % 4 == 0 && aligned16(p->g) && aligned16(p->y));
    const BwdArgs a = bn_bwd_args(p->g, p->y, p->saved_mean, p->saved_var, p->weight, p->bias, p->eps, p->relu, P);
    hipLaunchKernelGGL(bn_bwd_reduce_groups_kernel, dim3((unsigned)P, (unsigned)p->C, (unsigned)p->G), dim3(BN_STATS_THREADS), 0, (hipStream_t)stream, a, w,
                       (unsigned)bn_slice(N, P), bn_groups(p->G, p->n, p->C, p->S), p->workspace);
    return check_launch("bn_bwd_reduce_groups");
}

int ucnerf_bn_bwd_apply_groups(const ucnerf_bn_bwd_apply_groups_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_apply_groups: null params");
    int64_t N, P;
    if (int rc = bn_bwd_groups_common("bn_bwd_apply_groups", p->G, p->n, p->C, p->S, p->workspace_pairs, p->eps, p->g, p->y, p->saved_mean, p->saved_var, p->weight,
                                      p->bias, p->workspace, &N, &P))
        return rc;
    UCNERF_REQUIRE(p->grad_y && p->grad_weight && p->grad_bias, "bn_bwd_apply_groups: null grad_y, grad_weight or grad_bias");
    const Walk w = bn_walk(p->C, p->S, N, p->S % 4 == 0 && aligned16(p->g) && aligned16(p->y) && aligned16(p->grad_y));
    const BwdArgs a = bn_bwd_args(p->g, p->y, p->saved_mean, p->saved_var, p->weight, p->bias, p->eps, p->relu, P);
    hipLaunchKernelGGL(bn_bwd_apply_groups_kernel, dim3((unsigned)((N + BN_APPLY_CHUNK - 1) / BN_APPLY_CHUNK), (unsigned)p->C, (unsigned)p->G), dim3(BN_APPLY_THREADS), 0,
                       (hipStream_t)stream, a, w, bn_groups(p->G, p->n, p->C, p->S), p->workspace, p->grad_y, p->grad_weight, p->grad_bias);
    return check_launch("bn_bwd_apply_groups");
}

}  // extern "C"
