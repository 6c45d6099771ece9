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

#include "ch_episode_dev.h"
#include "ch_internal.h"

namespace ch {

constexpr int kMarlAccThreads = 256;

// The first of the recorder's two launches, one thread per env over as many workgroups as that takes: the env's live
// agents' rewards into its accumulators (ch_episode_dev.h episode_accumulate), and the live agent-steps per agent index
// -- a pure count, added with one integer atomic per wave and agent (ballot + popcount): integer adds commute, so the
// result does not depend on the order the waves arrive in.  Workgroup 0 adds the step's E env steps.
__global__ __launch_bounds__(kMarlAccThreads) void k_marl_ep_ring_acc(MarlRingArgs a) {
    const long long e = (long long)blockIdx.x * kMarlAccThreads + threadIdx.x;
    const bool in = e < a.E;
    const int N = a.N;
    if (in) episode_accumulate(e, N, a.live, a.reward, a.acc_return, a.acc_length, a.acc_steps);
    for (int i = 0; i < N; ++i) {   // (N is uniform: every lane of the wave reaches each ballot)
        const unsigned long long m = __ballot(in && a.live[e * N + i] != 0);
        if ((threadIdx.x & 63) == 0 && m)
            atomicAdd(reinterpret_cast<unsigned long long*>(a.agent_steps + i), (unsigned long long)__popcll(m));
    }
    if (e == 0) *a.env_steps += a.E;
}

// The second launch, one workgroup: ch_ep_ring_record's append (count_ended, ranked_walk and ring_slot of
// ch_episode_dev.h).  An ended env files the accumulators the first launch left, where its rank is among the last W,
// and zeroes them.  `total` is read at the start and rewritten by thread 0 at the end.
__global__ __launch_bounds__(kEpisodeThreads) void k_marl_ep_ring_append(MarlRingArgs a) {
    __shared__ long long wsum[kEpisodeWaves + 1];
    const int N = a.N;
    const long long total = *a.total;
    const long long C = count_ended(a.E, a.reset, wsum);
    if (C == 0) return;   // (uniform: most steps end no episode)
    const long long first = C > a.W ? C - a.W : 0;   // ranks below it would be overwritten within this step
    ranked_walk(a.E, a.reset, wsum, [&](long long e, long long r) {
        if (r >= first) {
            const long long slot = ring_slot(total, r, a.W);
            a.ep_return[slot] = episode_file(e, N, a.acc_return, a.acc_length, slot, a.agent_return, a.agent_length);
            a.ep_length[slot] = a.acc_steps[e];
            a.ep_env[slot] = (int)e;
        }
        episode_zero(e, N, a.acc_return, a.acc_length);
        a.acc_steps[e] = 0;
    });
    if (threadIdx.x == 0) *a.total = total + C;
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
    episode_zero(e, a.N, a.acc_return, a.acc_length);
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
    hipLaunchKernelGGL(k_marl_ep_ring_append, dim3(1), dim3(kEpisodeThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace ch
