// f3, the cascade depth loss of network/mvs_models.py:512-529 (cas_mvsnet_loss) with every count kept on the device: the reference indexes with
// boolean masks (est[mask], gt[mask], w[w > 0]), which compacts and therefore reads element counts back to the host -- three stream drains a
// step, and a step no graph can capture.  The pairing those compactions imply -- k-th valid depth with k-th positive weight, both in row-major
// order -- is kept: an order-preserving rank, formed with ballots and integer prefix sums.  Plain HIP C++, wave64, no float atomics.
//
// One workgroup does all (up to three) stages in turn.  A stage per workgroup would leave `total` to a second launch or to a hand-off between
// workgroups; this file has neither -- nothing here waits for another workgroup, so nothing here can hang -- and the sticky status word has
// exactly one writer.  The price is that the two small stages (1/16 and 1/4 of the largest) run in front of the large one instead of beside it.
//
// Reproducibility: counts and ranks are integers; the float sum goes lane (its tiles in order) -> wave (shuffle tree) -> 16 waves (pairwise
// tree by one thread).  Tile ownership depends on n alone, so two calls on the same inputs give the same bits.
#include "common.h"

namespace ucnerf {

constexpr int CL_BLOCK = 1024;
constexpr int CL_WAVES = CL_BLOCK / 64;
constexpr int CL_MAX_N = 1 << 30;          // begin + tile * 64 + lane stays inside int32 with room to spare
constexpr int CL_BWD_BLOCK = 256;

__device__ __forceinline__ float cl_nan() { return __uint_as_float(0x7fc00000u); }

// entry s of a three-element array of a by-value params struct, selected without indexing the kernel arguments with a run-time value
template <typename T>
__device__ __forceinline__ T cl_pick(const T (&a)[3], int s) { return s == 0 ? a[0] : s == 1 ? a[1] : a[2]; }
__device__ __forceinline__ int cl_cdiv(int a, int b) { return (a + b - 1) / b; }

__global__ void __launch_bounds__(CL_BLOCK) cas_loss_fwd_kernel(ucnerf_cas_loss_params p) {
    __shared__ int s_valid[CL_WAVES], s_pos[CL_WAVES];
    __shared__ float s_sum[CL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;              // the lanes in front of this one
    float total = 0.f;                                                    // (thread 0's is the one stored)
    long long ws_off = 0;
    for (int s = 0; s < p.n_stages; ++s) {
        const int n = cl_pick(p.n, s);
        const float* est = cl_pick(p.est, s);
        const float* gt = cl_pick(p.gt, s);
        const float* w = cl_pick(p.w, s);
        float* wpair = cl_pick(p.wpair, s);
        float* wc = p.with_weight ? p.workspace + ws_off : nullptr;      // [n]: the positive weights in row-major order
        ws_off += n;
        const int per_wave = cl_cdiv(cl_cdiv(n, 64), CL_WAVES) * 64;   // elements of a wave's run (a multiple of the tile)
        const int begin = wave * per_wave < n ? wave * per_wave : n;     // (n <= 2^30, per_wave <= n / 16 + 64: no overflow)
        const int end = n - begin < per_wave ? n : begin + per_wave;

        // ---- pass 1: valid elements and positive weights of this wave's run
        int c_valid = 0, c_pos = 0;
        for (int t = begin; t < end; t += 64) {
            const int i = t + lane;
            const bool in = i < end;
            c_valid += __popcll(__ballot(in && gt[i] > 0.f));            // (&&: nothing past `end` is read; NaN > 0 is false)
            if (p.with_weight) c_pos += __popcll(__ballot(in && w[i] > 0.f));
        }
        if (lane == 0) { s_valid[wave] = c_valid; s_pos[wave] = c_pos; }
        __syncthreads();
        int off_valid = 0, off_pos = 0, count = 0, n_pos = 0;
#pragma unroll
        for (int v = 0; v < CL_WAVES; ++v) {
            const int a = s_valid[v], b = s_pos[v];
            if (v < wave) { off_valid += a; off_pos += b; }
            count += a; n_pos += b;
        }
        const bool mismatch = p.with_weight && count != n_pos;           // (the same in every thread)

        // ---- pass 2: positive weight number k of the stage -> wc[k]   (k < n_pos <= n: inside the stage's part of the workspace)
        if (p.with_weight && !mismatch) {
            int run = off_pos;
            for (int t = begin; t < end; t += 64) {
                const int i = t + lane;
                const float v = i < end ? w[i] : 0.f;
                const bool pos = v > 0.f;
                const unsigned long long m = __ballot(pos);
                if (pos) wc[run + __popcll(m & below)] = v;
                run += __popcll(m);
            }
        }
        __syncthreads();                                                  // the workgroup's own global stores, visible to the workgroup

        // ---- pass 3: valid element number k takes wc[k]
        float acc = 0.f;
        int run = off_valid;
        for (int t = begin; t < end; t += 64) {
            const int i = t + lane;
            const bool in = i < end;
            const float g = in ? gt[i] : 0.f;
            const bool valid = g > 0.f;
            const unsigned long long m = __ballot(valid);
            float wv = 0.f;
            if (valid) {
                wv = !p.with_weight ? 1.f : mismatch ? cl_nan() : wc[run + __popcll(m & below)];      // (rank < count == n_pos)
                const float d = est[i] - g, z = fabsf(d);
                const float term = z < 1.f ? 0.5f * z * z : z - 0.5f;    // smooth-L1, beta 1 (a NaN difference: NaN)
                acc += term * wv;
            }
            if (in && wpair) wpair[i] = wv;
            run += __popcll(m);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d);
        if (lane == 0) s_sum[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float r[CL_WAVES];
#pragma unroll
            for (int v = 0; v < CL_WAVES; ++v) r[v] = s_sum[v];
#pragma unroll
            for (int width = CL_WAVES / 2; width >= 1; width >>= 1) {
#pragma unroll
                for (int v = 0; v < width; ++v) r[v] = r[2 * v] + r[2 * v + 1];
            }
            const float loss = mismatch ? cl_nan() : r[0] / (float)count;      // (count == 0: 0 / 0 = NaN, torch's mean of nothing)
            p.stage_loss[s] = loss;
            p.count[s] = count;
            total = total + cl_pick(p.stage_w, s) * loss;
            if (mismatch && p.status) *p.status = *p.status | (1 << s);       // (one writer: this thread)
        }
        // (the next stage writes s_valid / s_pos behind the two barriers above and s_sum behind two more of its own: no LDS reuse hazard)
    }
    if (threadIdx.x == 0) *p.total = total;
}

// grid (blocks over the largest stage, stages)
__global__ void __launch_bounds__(CL_BWD_BLOCK) cas_loss_bwd_kernel(ucnerf_cas_loss_bwd_params p) {
    const int s = blockIdx.y;
    const int n = cl_pick(p.n, s);
    const int i = blockIdx.x * CL_BWD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float g = cl_pick(p.gt, s)[i];
    float out = 0.f;
    if (g > 0.f) {
        float up = p.g_total[0] * cl_pick(p.stage_w, s);
        if (p.g_stage) up = up + p.g_stage[s];
        const float per = up / (float)p.count[s];                         // mean backward: a division
        const float d = cl_pick(p.est, s)[i] - g;
        const float slope = d < -1.f ? -1.f : d > 1.f ? 1.f : d;         // (a NaN difference stays NaN)
        out = per * cl_pick(p.wpair, s)[i] * slope;
    }
    cl_pick(p.g_est, s)[i] = out;
}

}  // namespace ucnerf

using namespace ucnerf;

static int cas_loss_sizes(const char* what, int32_t n_stages, const int32_t* n) {
    UCNERF_REQUIRE(n_stages >= 1 && n_stages <= 3, "%s: n_stages = %d outside 1..3", what, n_stages);
    for (int s = 0; s < n_stages; ++s)
        UCNERF_REQUIRE(n[s] >= 1 && n[s] <= CL_MAX_N, "%s: stage %d has n = %d elements, outside 1..%d", what, s, n[s], CL_MAX_N);
    return UCNERF_OK;
}

extern "C" {

int64_t ucnerf_cas_loss_workspace_floats(int32_t n_stages, const int32_t* n_host) {
    if (!n_host) return fail(UCNERF_EINVAL, "cas_loss_workspace_floats: null sizes");
    if (const int rc = cas_loss_sizes("cas_loss_workspace_floats", n_stages, n_host)) return rc;
    int64_t sum = 0;
    for (int s = 0; s < n_stages; ++s) sum += n_host[s];
    return sum;
}

int ucnerf_cas_loss_fwd(const ucnerf_cas_loss_params* p, void* stream) {
    UCNERF_REQUIRE(p, "cas_loss_fwd: null params");
    if (const int rc = cas_loss_sizes("cas_loss_fwd", p->n_stages, p->n)) return rc;
    UCNERF_REQUIRE(p->total && p->stage_loss && p->count, "cas_loss_fwd: null total, stage_loss or count");
    UCNERF_REQUIRE(!p->with_weight || p->workspace, "cas_loss_fwd: null workspace (with_weight)");
    int n_wpair = 0;
    for (int s = 0; s < p->n_stages; ++s) {
        UCNERF_REQUIRE(p->est[s] && p->gt[s], "cas_loss_fwd: null est or gt of stage %d", s);
        UCNERF_REQUIRE(!p->with_weight || p->w[s], "cas_loss_fwd: null w of stage %d (with_weight)", s);
        n_wpair += p->wpair[s] != nullptr;
    }
    UCNERF_REQUIRE(n_wpair == 0 || n_wpair == p->n_stages, "cas_loss_fwd: wpair given for %d of %d stages (all or none)", n_wpair, p->n_stages);
    hipLaunchKernelGGL(cas_loss_fwd_kernel, dim3(1), dim3(CL_BLOCK), 0, (hipStream_t)stream, *p);
    return check_launch("cas_loss_fwd");
}

int ucnerf_cas_loss_bwd(const ucnerf_cas_loss_bwd_params* p, void* stream) {
    UCNERF_REQUIRE(p, "cas_loss_bwd: null params");
    if (const int rc = cas_loss_sizes("cas_loss_bwd", p->n_stages, p->n)) return rc;
    UCNERF_REQUIRE(p->count && p->g_total, "cas_loss_bwd: null count or g_total");
    int n_max = 0;
    for (int s = 0; s < p->n_stages; ++s) {
        UCNERF_REQUIRE(p->est[s] && p->gt[s] && p->wpair[s] && p->g_est[s], "cas_loss_bwd: null est, gt, wpair or g_est of stage %d", s);
        n_max = p->n[s] > n_max ? p->n[s] : n_max;
    }
    hipLaunchKernelGGL(cas_loss_bwd_kernel, dim3(cdiv(n_max, CL_BWD_BLOCK), p->n_stages), dim3(CL_BWD_BLOCK), 0, (hipStream_t)stream, *p);
    return check_launch("cas_loss_bwd");
}

}  // extern "C"
