// ch_eval.hip — the on-device evaluate_policy (include/cattleherd.h ch_eval_*): the episode table and the
// deterministic action.
//
// Reference: stable_baselines3 evaluate_policy (SB3 is not in this image: restated from its source, "parity
// unpinned"), as CTDECattleHerder.py:139-148 (EvalCallback) and :185 run it.  Its bookkeeping per env.step of a VecEnv:
//   episode_count_targets[i] = (n_eval_episodes + i) // n_envs;
//   for every env i with episode_counts[i] < episode_count_targets[i]: if the env's episode ended in the step, append
//   Monitor's info["episode"] "r" and "l" to the lists and count it; loop while (episode_counts < targets).any().
// The lists are a table [E][C] here (slot = the env's count), `remaining` is what the while condition sums, and the
// recorder runs after each ch_step on the step's reset_happened / episode_stats.
#include <hip/hip_runtime.h>

#include "ch_episode_dev.h"
#include "ch_internal.h"

namespace ch {

constexpr int kEvalThreads = 256;

__global__ __launch_bounds__(kEvalThreads) void k_eval_begin(EvalArgs a, long long n_eval) {
    const long long e = (long long)blockIdx.x * kEvalThreads + threadIdx.x;
    if (e == 0) *a.remaining = n_eval;
    if (e >= a.E) return;
    a.quota[e] = eval_quota(e, n_eval, a.E);
    a.count[e] = 0;
}

// one thread per env (coalesced reads of the step's outputs).  The slot is below the capacity whatever the quota array
// holds; `remaining` drops as ch_episode_dev.h drop_remaining says.
__device__ __forceinline__ void eval_record_env(const EvalArgs& a, long long e) {
    bool rec = false;
    if (e < a.E && a.reset[e] != 0) {
        const int c = a.count[e];
        if (c < a.quota[e] && c < a.C) {
            rec = true;
            const long long s = e * a.C + c;
            a.ep_return[s] = a.stats[2 * e];
            a.ep_length[s] = (int)a.stats[2 * e + 1];
            a.ep_flags[s] = (uint8_t)((a.term[e] ? 1 : 0) | (a.trunc[e] ? 2 : 0));
            a.ep_end_step[s] = a.step_index;
            a.count[e] = c + 1;
        }
    }
    drop_remaining(a.remaining, rec);   // (every lane of the wave gets here)
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_record(EvalArgs a) {
    eval_record_env(a, (long long)blockIdx.x * kEvalThreads + threadIdx.x);
}

// SB3 predict(deterministic=True): the action mean clipped to the Box [-1, 1] (np.clip: a NaN stays a NaN); the env
// reads the first num_drones rows of the (12, 4) action.  One thread per env action float.  RECORD (ch_evaluate_policy
// between two checks of `remaining`): the threads of the first E floats first run the recorder of the step before --
// its outputs stay in place until the next step runs, after this kernel -- which saves that step's recorder launch.
template <bool RECORD>
__global__ __launch_bounds__(kEvalThreads) void k_eval_actions(const float* mean, int mean_ld, int act_w, long long n,
                                                             float* env_actions, EvalArgs a) {
    const long long i = (long long)blockIdx.x * kEvalThreads + threadIdx.x;
    if constexpr (RECORD) {
        if ((long long)blockIdx.x * kEvalThreads < a.E) eval_record_env(a, i);   // (a whole workgroup takes the branch)
    }
    if (i >= n) return;
    const long long e = i / act_w;
    const float v = mean[e * mean_ld + (i - e * act_w)];
    env_actions[i] = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}

static unsigned eval_grid(long long n) { return (unsigned)((n + kEvalThreads - 1) / kEvalThreads); }

hipError_t launch_eval_begin(const EvalArgs& a, long long n_eval, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_begin, dim3(eval_grid(a.E)), dim3(kEvalThreads), 0, st, a, n_eval);
    return hipGetLastError();
}

hipError_t launch_eval_record(const EvalArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_record, dim3(eval_grid(a.E)), dim3(kEvalThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_eval_actions(const float* mean, int mean_ld, int act_w, long long E, float* env_actions,
                               const EvalArgs* record_prev, hipStream_t st) {
    const long long n = E * act_w;   // >= E: the recorder's threads are in the grid
    if (record_prev)
        hipLaunchKernelGGL(k_eval_actions<true>, dim3(eval_grid(n)), dim3(kEvalThreads), 0, st, mean, mean_ld, act_w, n,
                           env_actions, *record_prev);
    else
        hipLaunchKernelGGL(k_eval_actions<false>, dim3(eval_grid(n)), dim3(kEvalThreads), 0, st, mean, mean_ld, act_w, n,
                           env_actions, EvalArgs{});
    return hipGetLastError();
}

}  // namespace ch
