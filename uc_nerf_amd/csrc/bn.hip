// Train-mode batch-norm for the MVS CNNs under train() + no_grad (include/ucnerf_hip.h, "batch-statistic batch-norm"): the statistics of the
// batch itself, the normalise / ReLU / skip epilogue and the running-statistic update.  Two launches, nothing read back, no atomics.
//
//   ucnerf_bn_stats   grid (P, C), 1024 threads: block (j, c) reduces slice j of channel c to one float64 triple (count, mean, M2).
//   ucnerf_bn_apply   grid (ceil(N / 4096), C), 256 threads: every block folds its channel's P triples itself (the same operations in the
//                     same order in every block, so all of them hold the same mu and sigma^2), then streams 4096 values.
//
// A channel's N = n S values are numbered i = img * S + offset.  Both kernels walk them in QUADS of four consecutive i; where S is a multiple of
// four and the arrays are 16-byte aligned a quad is one 16-byte access, otherwise four scalar ones -- the values and the order of every sum are
// the same either way.  Every intermediate of the statistics is float64: a float32 slice mean at |mean| >> sigma would put its own rounding,
// squared and multiplied by the count, into M2.
#include "bn_device.h"

namespace ucnerf {
namespace {

__global__ __launch_bounds__(BN_STATS_THREADS) void bn_stats_kernel(const float* __restrict__ y, Walk w, unsigned L, int P, double* __restrict__ ws) {
    const int j = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    const Triple run = bn_slice_triple(y, w, L, j, c, t);
    if (t == 0) {
        double* o = ws + ((size_t)c * (size_t)P + (size_t)j) * 3;
        o[0] = run.n; o[1] = run.mean; o[2] = run.m2;
    }
}

__global__ __launch_bounds__(BN_APPLY_THREADS) void bn_apply_kernel(ApplyArgs a, Walk w) { bn_apply_block<true>(a, w); }

// ---- backward (ucnerf_bn_bwd_reduce, ucnerf_bn_bwd_apply): the same slices and quads as the forward pair, a float64 workspace [C, P, 2]
__global__ __launch_bounds__(BN_STATS_THREADS) void bn_bwd_reduce_kernel(BwdArgs a, Walk w, unsigned L, double* __restrict__ ws) {
    const int j = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    double sa, sb;
    bn_bwd_slice_sums(a, w, L, j, c, t, sa, sb);
    if (t == 0) {
        double* o = ws + ((size_t)c * (size_t)a.P + (size_t)j) * 2;
        o[0] = sa; o[1] = sb;
    }
}

__global__ __launch_bounds__(BN_APPLY_THREADS) void bn_bwd_apply_kernel(BwdArgs a, Walk w, const double* __restrict__ ws, float* dy, float* __restrict__ dgamma,
                                                                        float* __restrict__ dbeta) {
    bn_bwd_apply_block<true>(a, w, ws, dy, dgamma, dbeta);
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
    int64_t N;
    if (int rc = bn_shape("bn_stats", p->n, p->C, p->S, &N)) return rc;
    UCNERF_REQUIRE(p->y && p->workspace, "bn_stats: null y or workspace");
    const int64_t P = bn_partials(N);
    UCNERF_REQUIRE(p->workspace_triples >= p->C * P, "bn_stats: the workspace holds %lld triples, C P = %lld x %lld are written", (long long)p->workspace_triples,
                   (long long)p->C, (long long)P);
    UCNERF_REQUIRE(((uintptr_t)p->workspace & 7) == 0, "bn_stats: the workspace is not 8-byte aligned");
    Walk w;
    w.C = p->C; w.S = p->S; w.N = (unsigned)N; w.S32 = (unsigned)p->S;
    w.vec = p->S % 4 == 0 && aligned16(p->y);
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)P, (unsigned)p->C), dim3(BN_STATS_THREADS), 0, (hipStream_t)stream, p->y, w, (unsigned)bn_slice(N, P), (int)P,
                       p->workspace);
    return check_launch("bn_stats");
}

int ucnerf_bn_apply(const ucnerf_bn_apply_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_apply: null params");
    int64_t N;
    if (int rc = bn_shape("bn_apply", p->n, p->C, p->S, &N)) return rc;
    UCNERF_REQUIRE(p->y && p->out && p->workspace && p->weight && p->bias, "bn_apply: null y, out, workspace, weight or bias");
    UCNERF_REQUIRE(p->saved_mean && p->saved_var && p->running_mean && p->running_var && p->num_batches_tracked,
                   "bn_apply: null saved_mean, saved_var, running_mean, running_var or num_batches_tracked");
    UCNERF_REQUIRE(p->eps > 0.f, "bn_apply: eps=%g (must be positive)", (double)p->eps);                    // (a NaN fails both)
    UCNERF_REQUIRE(p->momentum > 0.f && p->momentum <= 1.f, "bn_apply: momentum=%g (must lie in (0, 1])", (double)p->momentum);
    const int64_t P = bn_partials(N);
    UCNERF_REQUIRE(p->workspace_triples >= p->C * P, "bn_apply: the workspace holds %lld triples, C P = %lld x %lld are read", (long long)p->workspace_triples,
                   (long long)p->C, (long long)P);
    UCNERF_REQUIRE(((uintptr_t)p->workspace & 7) == 0 && ((uintptr_t)p->num_batches_tracked & 7) == 0, "bn_apply: workspace or num_batches_tracked not 8-byte aligned");
    Walk w;
    w.C = p->C; w.S = p->S; w.N = (unsigned)N; w.S32 = (unsigned)p->S;
    w.vec = p->S % 4 == 0 && aligned16(p->y) && aligned16(p->out) && (!p->skip || aligned16(p->skip));
    ApplyArgs a;
    a.y = p->y; a.skip = p->skip; a.gamma = p->weight; a.beta = p->bias; a.out = p->out;
    a.saved_mean = p->saved_mean; a.saved_var = p->saved_var; a.running_mean = p->running_mean; a.running_var = p->running_var;
    a.num_batches_tracked = reinterpret_cast<long long*>(p->num_batches_tracked);
    a.ws = p->workspace; a.eps = p->eps; a.momentum = p->momentum; a.P = (int)P; a.relu = p->relu != 0;
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((N + BN_APPLY_CHUNK - 1) / BN_APPLY_CHUNK), (unsigned)p->C), dim3(BN_APPLY_THREADS), 0, (hipStream_t)stream, a, w);
    return check_launch("bn_apply");
}

static int bn_bwd_common(const char* who, int64_t n, int64_t C, int64_t S, int64_t pairs, float eps, const void* g, const void* y, const void* mean, const void* var,
                         const void* gamma, const void* beta, const void* ws, int64_t* N, int64_t* P) {
    if (int rc = bn_shape(who, n, C, S, N)) return rc;
    UCNERF_REQUIRE(g && y && mean && var && gamma && beta && ws, "%s: null g, y, saved_mean, saved_var, weight, bias or workspace", who);
    UCNERF_REQUIRE(eps > 0.f, "%s: eps=%g (must be positive)", who, (double)eps);
    *P = bn_partials(*N);
    UCNERF_REQUIRE(pairs >= C * *P, "%s: the workspace holds %lld pairs, C P = %lld x %lld are used", who, (long long)pairs, (long long)C, (long long)*P);
    UCNERF_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: the workspace is not 8-byte aligned", who);
    return UCNERF_OK;
}

int ucnerf_bn_bwd_reduce(const ucnerf_bn_bwd_reduce_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_reduce: null params");
    int64_t N, P;
    if (int rc = bn_bwd_common("bn_bwd_reduce", p->n, p->C, p->S, p->workspace_pairs, p->eps, p->g, p->y, p->saved_mean, p->saved_var, p->weight, p->bias, p->workspace, &N, &P))
        return rc;
    Walk w;
    w.C = p->C; w.S = p->S; w.N = (unsigned)N; w.S32 = (unsigned)p->S;
    w.vec = p->S % 4 == 0 && aligned16(p->g) && aligned16(p->y);
    BwdArgs a;
    a.g = p->g; a.y = p->y; a.mean = p->saved_mean; a.var = p->saved_var; a.gamma = p->weight; a.beta = p->bias; a.eps = p->eps; a.relu = p->relu != 0; a.P = (int)P;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((unsigned)P, (unsigned)p->C), dim3(BN_STATS_THREADS), 0, (hipStream_t)stream, a, w, (unsigned)bn_slice(N, P), p->workspace);
    return check_launch("bn_bwd_reduce");
}

int ucnerf_bn_bwd_apply(const ucnerf_bn_bwd_apply_params* p, void* stream) {
    UCNERF_REQUIRE(p, "bn_bwd_apply: null params");
    int64_t N, P;
    if (int rc = bn_bwd_common("bn_bwd_apply", p->n, p->C, p->S, p->workspace_pairs, p->eps, p->g, p->y, p->saved_mean, p->saved_var, p->weight, p->bias, p->workspace, &N, &P))
        return rc;
    UCNERF_REQUIRE(p->grad_y && p->grad_weight && p->grad_bias, "bn_bwd_apply: null grad_y, grad_weight or grad_bias");
    Walk w;
    w.C = p->C; w.S = p->S; w.N = (unsigned)N; w.S32 = (unsigned)p->S;
    w.vec = p->S % 4 == 0 && aligned16(p->g) && aligned16(p->y) && aligned16(p->grad_y);
    BwdArgs a;
    a.g = p->g; a.y = p->y; a.mean = p->saved_mean; a.var = p->saved_var; a.gamma = p->weight; a.beta = p->bias; a.eps = p->eps; a.relu = p->relu != 0; a.P = (int)P;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((N + BN_APPLY_CHUNK - 1) / BN_APPLY_CHUNK), (unsigned)p->C), dim3(BN_APPLY_THREADS), 0, (hipStream_t)stream, a, w,
                       p->workspace, p->grad_y, p->grad_weight, p->grad_bias);
    return check_launch("bn_bwd_apply");
}

}  // extern "C"
