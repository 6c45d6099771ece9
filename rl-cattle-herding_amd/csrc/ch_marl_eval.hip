// ch_marl_eval.hip — the on-device policy evaluation of the DTDE (RLlib) driver (include/cattleherd.h ch_marl_eval_*):
// the per-agent episode table and the deterministic action of the shared policy.
//
// Reference: the DTDEModelPlayback.py workflow and RLlib's evaluation_* metrics over RLlibMultiAgentWrapper envs
// (rllib_envs/marl_wrapper.py:77-119).  RLlib is not in this image: its semantics are restated, "parity unpinned" to
// its source, as ch_marl_rollout's are (ch_aux.hip).  An episode is the wrapper's: agents that terminate drop out of
// self.agents, "__all__" is set -- the env ends and auto-resets -- once every agent has terminated.  Divergence, the
// one ch_marl_rollout documents: RLlib's per-agent episodes end on terminated OR truncated; under the wrapper's
// "__all__" rule a truncation does not end an episode, and none ends here on one.
// The quota rule and `remaining` are the CTDE table's (ch_eval.hip): quota[e] = (n + e) / E, slot = the env's count.
// What the CTDE table takes from the step's episode_stats is kept here per agent: `live` (marked before the step: the
// wrapper's self.agents, k_marl_store's mask), and the accumulators acc_return / acc_length / acc_steps the recorder
// advances after it (ch_episode_dev.h: one thread per env, its N <= 12 agents in index order).
#include <hip/hip_runtime.h>

#include "ch_episode_dev.h"
#include "ch_internal.h"

namespace ch {

constexpr int kMarlEvalThreads = 256;

__global__ __launch_bounds__(kMarlEvalThreads) void k_marl_eval_begin(MarlEvalArgs a, long long n_eval) {
    const long long e = (long long)blockIdx.x * kMarlEvalThreads + threadIdx.x;
    if (e == 0) *a.remaining = n_eval;
    if (e >= a.E) return;
    a.quota[e] = eval_quota(e, n_eval, a.E);
    a.count[e] = 0;
    a.acc_steps[e] = 0;
    episode_zero(e, a.N, a.acc_return, a.acc_length);
}

__device__ __forceinline__ bool marl_eval_live(const MarlEvalArgs& a, long long e, int i) {
    return agent_live(a.env_n, a.env_active, e, i);
}

__device__ __forceinline__ void marl_eval_mark_env(const MarlEvalArgs& a, long long e) {
    if (e >= a.E) return;
    for (int i = 0; i < a.N; ++i) a.live[e * a.N + i] = marl_eval_live(a, e, i) ? 1 : 0;
}

// one thread per env: the step's rewards of the agents marked live into the accumulators, then, where the env ended,
// the episode into slot count[e] (below the capacity whatever the quota array holds) and the accumulators back to 0
// (ch_episode_dev.h for each piece, and for how `remaining` drops).
__device__ __forceinline__ void marl_eval_record_env(const MarlEvalArgs& a, long long e) {
    bool rec = false;
    if (e < a.E) {
        const int steps = episode_accumulate(e, a.N, a.live, a.reward, a.acc_return, a.acc_length, a.acc_steps);
        if (a.reset[e] != 0) {
            const int c = a.count[e];
            if (c < a.quota[e] && c < a.C) {
                rec = true;
                const long long s = e * a.C + c;
                a.ep_return[s] = episode_file(e, a.N, a.acc_return, a.acc_length, s, a.agent_return, a.agent_length);
                a.ep_length[s] = steps;
                a.ep_end_step[s] = a.step_index;
                a.count[e] = c + 1;
            }
            episode_zero(e, a.N, a.acc_return, a.acc_length);
            a.acc_steps[e] = 0;
        }
    }
    drop_remaining(a.remaining, rec);   // (every lane of the wave gets here)
}

__global__ __launch_bounds__(kMarlEvalThreads) void k_marl_eval_mark(MarlEvalArgs a) {
    marl_eval_mark_env(a, (long long)blockIdx.x * kMarlEvalThreads + threadIdx.x);
}

__global__ __launch_bounds__(kMarlEvalThreads) void k_marl_eval_record(MarlEvalArgs a) {
    marl_eval_record_env(a, (long long)blockIdx.x * kMarlEvalThreads + threadIdx.x);
}

// RLlib explore=False on a DiagGaussian: the mean half of the policy output, unsquashed to the Box(-1, 1) by a clip (a
// NaN stays a NaN, as in np.clip); 0 for the agents that are not live (the env ignores them).  One thread per env action
// float; it takes the agent's liveness from the env ints themselves, not from `live`, which another thread of this
// launch writes.  The threads of the first E floats also keep the table, each for its own env: with RECORD
// (ch_marl_evaluate_policy between two checks of `remaining`) first the recorder of the step before -- its outputs
// stay in place until the next step runs, after this kernel -- on the old `live`, then the mark that overwrites it.
template <bool RECORD>
__global__ __launch_bounds__(kMarlEvalThreads) void k_marl_eval_actions(const float* pol, int pol_ld, long long n,
                                                                      float* env_actions, MarlEvalArgs a) {
    const long long j = (long long)blockIdx.x * kMarlEvalThreads + threadIdx.x;
    if ((long long)blockIdx.x * kMarlEvalThreads < a.E) {   // (a whole workgroup takes the branch)
        if constexpr (RECORD) marl_eval_record_env(a, j);
        marl_eval_mark_env(a, j);
    }
    if (j >= n) return;
    const long long row = j >> 2;   // agent row e * N + i
    const long long e = row / a.N;
    float v = 0.0f;
    if (marl_eval_live(a, e, (int)(row - e * a.N))) {
        v = pol[row * pol_ld + (j & 3)];
        v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    }
    env_actions[j] = v;
}

static unsigned marl_eval_grid(long long n) { return (unsigned)((n + kMarlEvalThreads - 1) / kMarlEvalThreads); }

hipError_t launch_marl_eval_begin(const MarlEvalArgs& a, long long n_eval, hipStream_t st) {
    hipLaunchKernelGGL(k_marl_eval_begin, dim3(marl_eval_grid(a.E)), dim3(kMarlEvalThreads), 0, st, a, n_eval);
    return hipGetLastError();
}

hipError_t launch_marl_eval_mark(const MarlEvalArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_marl_eval_mark, dim3(marl_eval_grid(a.E)), dim3(kMarlEvalThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_marl_eval_record(const MarlEvalArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_marl_eval_record, dim3(marl_eval_grid(a.E)), dim3(kMarlEvalThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_marl_eval_actions(const float* pol, int pol_ld, float* env_actions, const MarlEvalArgs& a,
                                    bool record_prev, hipStream_t st) {
    const long long n = a.E * a.N * 4;   // >= E: the table's threads are in the grid
    if (record_prev)
        hipLaunchKernelGGL(k_marl_eval_actions<true>, dim3(marl_eval_grid(n)), dim3(kMarlEvalThreads), 0, st, pol, pol_ld,
                           n, env_actions, a);
    else
        hipLaunchKernelGGL(k_marl_eval_actions<false>, dim3(marl_eval_grid(n)), dim3(kMarlEvalThreads), 0, st, pol, pol_ld,
                           n, env_actions, a);
    return hipGetLastError();
}

}  // namespace ch
