// ch_marl_ep_ring.hip -- the device side of the RLlib training log's env-runner half (include/cattleherd.h
// ch_marl_ep_ring_*): the ring of the last W episodes of a MARL handle, with per-agent returns and lengths, and the
// sampling counters behind env_runners/episode_return_mean, episode_len_mean, agent_episode_returns_mean/* and
// num_env_steps_sampled / num_agent_steps_sampled/*.
//
// Reference: RLlib's MetricsLogger over RLlibMultiAgentWrapper envs (rllib_envs/marl_wrapper.py:77-119), a window of
// metrics_num_episodes_for_smoothing episodes.  (RLlib is not installed here: restated, "parity unpinned".)  The
// episode rule is ch_marl_eval_record's (ch_marl_eval.hip): an agent adds its reward and one step only where it was
// live at the step's start, an env's episode ends where reset_happened is set, a truncation ends nothing.  The append
// rule is ch_ep_ring_record's (ch_ep_ring.hip): the C envs that ended in the step in ascending env order, rank r into
// slot (total + r) % W, only the last W of a step written, plain stores, one writer per slot.
#include <hip/hip_runtime.h>

#include "ch_internal.h"

namespace ch {

constexpr int kMarlRingThreads = 1024;
constexpr int kMarlRingWaves = kMarlRingThreads / 64;
constexpr int kMarlAccThreads = 256;

// The first of the recorder's two launches, one thread per env over as many workgroups as that takes: the env's live
// agents' rewards into its accumulators (agents in index order: every float64 sum has one thread and one fixed order),
// and the live agent-steps per agent index -- a pure count, added with one integer atomic per wave and agent (ballot +
// popcount), as ch_marl_eval_record counts `remaining`: integer adds commute, so the result does not depend on the
// order the waves arrive in.  Workgroup 0 adds the step's E env steps.
__global__ __launch_bounds__(kMarlAccThreads) void k_marl_ep_ring_acc(MarlRingArgs a) {
    const long long e = (long long)blockIdx.x * kMarlAccThreads + threadIdx.x;
    const bool in = e < a.E;
    const int N = a.N;
    if (in) {
        const long long r0 = e * N;
        for (int i = 0; i < N; ++i) {
            if (a.live[r0 + i]) {   // (the reward of an agent that is not live is never loaded)
                a.acc_return[r0 + i] += (double)a.reward[r0 + i];
                a.acc_length[r0 + i] += 1;
            }
        }
        a.acc_steps[e] += 1;
    }
    for (int i = 0; i < N; ++i) {   // (N is uniform: every lane of the wave reaches each ballot)
        const unsigned long long m = __ballot(in && a.live[e * N + i] != 0);
        if ((threadIdx.x & 63) == 0 && m)
            atomicAdd(reinterpret_cast<unsigned long long*>(a.agent_steps + i), (unsigned long long)__popcll(m));
    }
    if (e == 0) *a.env_steps += a.E;
}

// The second launch, one workgroup: ch_ep_ring_record's append.  C, the number of envs that ended in the step, decides
// who writes (only the last W of the step), so the envs' reset flags are walked twice: a counting pass, then -- only
// when C > 0 -- the ranking pass of k_ep_ring_record, each chunk of 1024 envs ranked by wave ballots and a scan of the
// 16 wave totals.  An ended env files the accumulators the first launch left, where its rank is among the last W,
// and zeroes them.  `total` is read at the start and rewritten by thread 0 at the end.
__global__ __launch_bounds__(kMarlRingThreads) void k_marl_ep_ring_append(MarlRingArgs a) {
    __shared__ long long wsum[kMarlRingWaves + 1];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int N = a.N;
    const long long total = *a.total;
    long long ended = 0;       // (the same in every lane of the wave)
    for (long long c0 = 0; c0 < a.E; c0 += kMarlRingThreads) {
        const long long e = c0 + t;
        ended += __popcll(__ballot(e < a.E && a.reset[e] != 0));
    }
    if (lane == 0) wsum[w] = ended;
    __syncthreads();
    long long C = 0;
    for (int k = 0; k < kMarlRingWaves; ++k) C += wsum[k];
    __syncthreads();
    if (C == 0) return;   // (uniform: most steps end no episode)
    const long long first = C > a.W ? C - a.W : 0;   // ranks below it would be overwritten within this step
    long long base = 0;
    for (long long c0 = 0; c0 < a.E; c0 += kMarlRingThreads) {
        const long long e = c0 + t;
        const bool f = e < a.E && a.reset[e] != 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        if (t == 0) {
            long long s = 0;
            for (int k = 0; k < kMarlRingWaves; ++k) { const long long v = wsum[k]; wsum[k] = s; s += v; }
            wsum[kMarlRingWaves] = s;
        }
        __syncthreads();
        if (f) {
            const long long r0 = e * N;
            const long long r = base + wsum[w] + __popcll(m & ((1ull << lane) - 1ull));
            if (r >= first) {
                const long long slot = (total + r) % a.W;   // 0 <= slot < W
                double sum = 0.0;
                for (int i = 0; i < N; ++i) {
                    const double v = a.acc_return[r0 + i];
                    a.agent_return[slot * N + i] = v;
                    a.agent_length[slot * N + i] = a.acc_length[r0 + i];
                    sum += v;
                }
                a.ep_return[slot] = sum;
                a.ep_length[slot] = a.acc_steps[e];
                a.ep_env[slot] = (int)e;
            }
            for (int i = 0; i < N; ++i) {
                a.acc_return[r0 + i] = 0.0;
                a.acc_length[r0 + i] = 0;
            }
            a.acc_steps[e] = 0;
        }
        base += wsum[kMarlRingWaves];
        __syncthreads();
    }
    if (t == 0) *a.total = total + C;
}

// total, the counters and the accumulators to zero (the slots are not cleared)
__global__ __launch_bounds__(256) void k_marl_ep_ring_begin(MarlRingArgs a) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) {
        *a.total = 0;
        *a.env_steps = 0;
    }
    if (e < a.N) a.agent_steps[e] = 0;
    if (e >= a.E) return;
    a.acc_steps[e] = 0;
    for (int i = 0; i < a.N; ++i) {
        a.acc_return[e * a.N + i] = 0.0;
        a.acc_length[e * a.N + i] = 0;
    }
}

hipError_t launch_marl_ep_ring_begin(const MarlRingArgs& a, hipStream_t st) {
    const long long n = a.E > a.N ? a.E : a.N;
    hipLaunchKernelGGL(k_marl_ep_ring_begin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_marl_ep_ring_record(const MarlRingArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_marl_ep_ring_acc, dim3((unsigned)((a.E + kMarlAccThreads - 1) / kMarlAccThreads)),
                       dim3(kMarlAccThreads), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_marl_ep_ring_append, dim3(1), dim3(kMarlRingThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace ch
