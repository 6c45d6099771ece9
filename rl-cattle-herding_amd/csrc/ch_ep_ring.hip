// ch_ep_ring.hip -- the device side of the SB3 training log (include/cattleherd.h ch_ep_ring_*, ch_explained_variance):
// the episode ring behind rollout/ep_rew_mean and rollout/ep_len_mean, and train/explained_variance; and the same for a
// population of P members on one env batch (ch_ep_ring_pop_*, ch_explained_variance_pop): the member
// is a grid dimension of kernels that run the solo kernels' bodies, and the rings' fitness table.
//
// Reference: OnPolicyAlgorithm._update_info_buffer appends Monitor's info["episode"] of every env that ended an episode
// to a deque(maxlen=stats_window_size), in env order, after each step of collect_rollouts; PPO.train logs
// explained_variance(values.flatten(), returns.flatten()).  (SB3 is not installed here: restated, "parity unpinned".)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ch_episode_dev.h"
#include "ch_internal.h"

namespace ch {

// ---- the episode ring ------------------------------------------------------------------------------------------
// One workgroup per ring.  C, the number of envs that ended in the step, decides who writes (only the last W of the
// step), so the envs are walked twice: count_ended, then ranked_walk in ascending env order; the slot is ring_slot's
// (ch_episode_dev.h for all three).  `wsum`: the kernel's LDS array of kEpisodeWaves + 1 long long.
__device__ __forceinline__ void ep_ring_record_body(const EpRingArgs& a, long long* wsum) {
    const long long total = *a.total;   // (rewritten by thread 0 at the very end, behind the barriers below)
    const long long C = count_ended(a.E, a.reset, wsum);
    if (C == 0) return;   // (uniform: most steps end no episode)
    const long long first = C > a.W ? C - a.W : 0;   // ranks below it would be overwritten within this step
    ranked_walk(a.E, a.reset, wsum, [&](long long e, long long r) {
        if (r >= first) {
            const long long slot = ring_slot(total, r, a.W);
            a.ep_return[slot] = a.stats[2 * e];
            a.ep_length[slot] = (int)a.stats[2 * e + 1];
            a.ep_env[slot] = (int)e;
        }
    });
    if (threadIdx.x == 0) *a.total = total + C;
}

__global__ __launch_bounds__(kEpisodeThreads) void k_ep_ring_record(EpRingArgs a) {
    __shared__ long long wsum[kEpisodeWaves + 1];
    ep_ring_record_body(a, wsum);
}

hipError_t launch_ep_ring_record(const EpRingArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_ep_ring_record, dim3(1), dim3(kEpisodeThreads), 0, st, a);
    return hipGetLastError();
}

// ---- explained variance ----------------------------------------------------------------------------------------
// y = returns, d = returns - values, both widened exactly to float64.  Three launches, one per all-to-all seam (no
// atomics): the sums of y and d per workgroup; their means (every workgroup adds the partials in index order) and the
// squared deviations per workgroup; the final sums and the two outputs.  Within a workgroup thread t adds its
// elements in order and a fixed LDS tree adds the threads (k_metrics_reduce's scheme): the same input, the same bits.
constexpr int kEvThreads = 256;
constexpr int kEvMaxGrid = 256;
constexpr long long kEvPerGroup = 4096;   // elements per workgroup before the grid stops growing

int ev_grid(long long n) { return (int)std::min<long long>(kEvMaxGrid, (n + kEvPerGroup - 1) / kEvPerGroup); }
long long ev_scratch_doubles(long long n) { return 4LL * ev_grid(n); }

namespace {

// the workgroup's two sums in thread 0 (sy[0], sd[0]): a fixed halving tree over NT threads
template <int NT = kEvThreads>
__device__ __forceinline__ void ev_tree(double* sy, double* sd, double y, double d) {
    const int t = threadIdx.x;
    sy[t] = y; sd[t] = d;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (t < w) { sy[t] += sy[t + w]; sd[t] += sd[t + w]; }
        __syncthreads();
    }
}

// workgroup g = blockIdx.x of G = gridDim.x owns the elements [g * per, min(n, (g + 1) * per)); scratch: this input's
// 4G doubles
__device__ __forceinline__ void ev_pass_body(const float* __restrict__ values, const float* __restrict__ returns,
                                             long long n, long long per, double* scratch, int second) {
    __shared__ double sy[kEvThreads], sd[kEvThreads];
    __shared__ double mean[2];
    const int t = threadIdx.x, G = gridDim.x;
    if (second) {
        if (t == 0) {
            double y = 0.0, d = 0.0;
            for (int g = 0; g < G; ++g) { y += scratch[2 * g]; d += scratch[2 * g + 1]; }
            mean[0] = y / (double)n; mean[1] = d / (double)n;
        }
        __syncthreads();
    }
    const double my = second ? mean[0] : 0.0, md = second ? mean[1] : 0.0;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    double y = 0.0, d = 0.0;
    for (long long i = lo + t; i < hi; i += kEvThreads) {
        const double r = (double)returns[i], dv = r - (double)values[i];
        if (second) { y += (r - my) * (r - my); d += (dv - md) * (dv - md); }
        else { y += r; d += dv; }
    }
    ev_tree(sy, sd, y, d);
    if (t == 0) {
        double* out = scratch + (second ? 2 * G : 0) + 2 * blockIdx.x;
        out[0] = sy[0]; out[1] = sd[0];
    }
}

// one thread: the G second-pass partials in index order, the two outputs
__device__ __forceinline__ void ev_final_body(const double* scratch, int G, long long n, double* out) {
    double y = 0.0, d = 0.0;
    for (int g = 0; g < G; ++g) { y += scratch[2 * G + 2 * g]; d += scratch[2 * G + 2 * g + 1]; }
    const double var_y = y / (double)n, var_d = d / (double)n;
    out[0] = var_y == 0.0 ? __longlong_as_double(0x7ff8000000000000LL) : 1.0 - var_d / var_y;
    out[1] = var_y;
}

__global__ __launch_bounds__(kEvThreads) void k_ev_pass(const float* __restrict__ values, const float* __restrict__ returns,
                                                        long long n, long long per, double* scratch, int second) {
    ev_pass_body(values, returns, n, per, scratch, second);
}

__global__ void k_ev_final(const double* scratch, int G, long long n, double* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ev_final_body(scratch, G, n, out);
}

// The population's (ch_explained_variance_pop): grid (G, P) and (1, P), the member in blockIdx.y; its two inputs come
// from the device pointer tables, its scratch is row p of [P][4G] and its outputs row p of [P][2].  The same bodies on
// the same G and per: the solo call's bits.
__global__ __launch_bounds__(kEvThreads) void k_ev_pass_pop(const float* const* __restrict__ values,
                                                            const float* const* __restrict__ returns, long long n,
                                                            long long per, double* scratch, int second) {
    const int p = blockIdx.y;
    ev_pass_body(values[p], returns[p], n, per, scratch + 4LL * gridDim.x * p, second);
}

__global__ void k_ev_final_pop(const double* scratch, int G, long long n, double* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int p = blockIdx.y;
    ev_final_body(scratch + 4LL * G * p, G, n, out + 2 * p);
}

// ---- the population's fitness table (ch_ep_ring_pop_summary) -------------------------------------------------------
// Workgroup p, kSummaryThreads threads: the ring's content in chronological order is position i = 0 .. count - 1,
// episode total - count + i, slot (total - count + i) % W.  Thread t adds positions t, t + 64, ... in that order,
// starting from 0.0 (a thread without a position keeps 0.0); ev_tree<64> adds the threads.  out[p] = {count, the sum of
// the returns / count, the sum of the lengths / count, total}; NaN means for an empty ring.
constexpr int kSummaryThreads = 64;
__global__ __launch_bounds__(kSummaryThreads) void k_ep_ring_pop_summary(int W, const double* __restrict__ ep_return,
                                                                         const int* __restrict__ ep_length,
                                                                         const long long* __restrict__ total_all, double* out) {
    __shared__ double sr[kSummaryThreads], sl[kSummaryThreads];
    const long long p = blockIdx.x, total = total_all[p];
    const long long count = total < W ? total : W;
    double r = 0.0, l = 0.0;
    for (long long i = threadIdx.x; i < count; i += kSummaryThreads) {
        const long long slot = p * W + (total - count + i) % W;
        r += ep_return[slot];
        l += (double)ep_length[slot];
    }
    ev_tree<kSummaryThreads>(sr, sl, r, l);
    if (threadIdx.x == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        out[4 * p] = (double)count;
        out[4 * p + 1] = count ? sr[0] / (double)count : nan;
        out[4 * p + 2] = count ? sl[0] / (double)count : nan;
        out[4 * p + 3] = (double)total;
    }
}

}  // namespace

hipError_t launch_explained_variance(const float* values, const float* returns, long long n, double* out, double* scratch,
                                     hipStream_t st) {
    const int G = ev_grid(n);
    const long long per = (n + G - 1) / G;
    for (int second = 0; second < 2; ++second) {
        hipLaunchKernelGGL(k_ev_pass, dim3(G), dim3(kEvThreads), 0, st, values, returns, n, per, scratch, second);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ev_final, dim3(1), dim3(64), 0, st, scratch, G, n, out);
    return hipGetLastError();
}

// The population's rings (ch_ep_ring_pop_record): workgroup p is the solo recorder on member p's E envs -- rows
// [pE, (p + 1)E) of the step's reset_happened and episode_stats -- and on row p of the [P][W] arrays and of total, so
// ep_env holds member-local indices.  `a` is the whole population's: E envs per member, the arrays' first rows.  The
// return on C == 0 is the workgroup's own (uniform in it, before ranked_walk's barriers); the workgroups share nothing.
__global__ __launch_bounds__(kEpisodeThreads) void k_ep_ring_record_pop(EpRingArgs a) {
    __shared__ long long wsum[kEpisodeWaves + 1];
    const long long p = blockIdx.x;
    a.reset += p * a.E; a.stats += 2 * p * a.E;
    a.ep_return += p * a.W; a.ep_length += p * a.W; a.ep_env += p * a.W;
    a.total += p;
    ep_ring_record_body(a, wsum);
}

hipError_t launch_ep_ring_record_pop(const EpRingArgs& a, int members, hipStream_t st) {
    hipLaunchKernelGGL(k_ep_ring_record_pop, dim3((unsigned)members), dim3(kEpisodeThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_explained_variance_pop(const float* const* values, const float* const* returns, int members, long long n,
                                         double* out, double* scratch, hipStream_t st) {
    const int G = ev_grid(n);
    const long long per = (n + G - 1) / G;
    for (int second = 0; second < 2; ++second) {
        hipLaunchKernelGGL(k_ev_pass_pop, dim3(G, (unsigned)members), dim3(kEvThreads), 0, st, values, returns, n, per, scratch, second);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ev_final_pop, dim3(1, (unsigned)members), dim3(64), 0, st, scratch, G, n, out);
    return hipGetLastError();
}

hipError_t launch_ep_ring_pop_summary(const EpRingArgs& a, int members, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_ep_ring_pop_summary, dim3((unsigned)members), dim3(kSummaryThreads), 0, st, a.W, a.ep_return,
                       a.ep_length, a.total, out);
    return hipGetLastError();
}

}  // namespace ch
