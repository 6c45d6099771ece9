// ch_episode_dev.h -- the device-side episode bookkeeping the per-step recorders share, each rule written and explained
// once: the ordered compaction of the envs that ended in a step (ch_aux.hip k_stage_ended, ch_ep_ring.hip,
// ch_marl_ep_ring.hip), the rings' slot rule, the per-agent episode accumulators and the live-agent predicate of the MARL
// table and ring (ch_marl_eval.hip, ch_marl_ep_ring.hip, ch_aux.hip k_marl_store) and the evaluation tables' quota and
// `remaining` (ch_eval.hip, ch_marl_eval.hip).  (ch_eval_log.hip keeps its own arithmetic: see its header.)
#pragma once
#include "ch_internal.h"

namespace ch {

// ---- the ordered compaction: one workgroup of kEpisodeThreads walks the E envs in chunks of kEpisodeThreads; `wsum` is
// the kernel's own LDS array of kEpisodeWaves + 1 long long (the helpers declare no __shared__ of their own)
constexpr int kEpisodeThreads = 1024;
constexpr int kEpisodeWaves = kEpisodeThreads / 64;

// C, the number of envs with reset[e] != 0, the same in every thread: each wave's count over its lanes' envs (the
// ballot's popcount is the same in every lane of the wave), then the waves in index order.  The first barrier publishes
// the wave counts; the second keeps a later writer of wsum (ranked_walk) behind every thread's reads.
__device__ __forceinline__ long long count_ended(long long E, const uint8_t* reset, long long* wsum) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    long long mine = 0;
    for (long long c0 = 0; c0 < E; c0 += kEpisodeThreads) {
        const long long e = c0 + t;
        mine += __popcll(__ballot(e < E && reset[e] != 0));
    }
    if (lane == 0) wsum[w] = mine;
    __syncthreads();
    long long C = 0;
    for (int k = 0; k < kEpisodeWaves; ++k) C += wsum[k];
    __syncthreads();
    return C;
}

// f(e, r) for every env e with reset[e] != 0, r its rank among them in ascending env order; returns their number.
// Per chunk: every wave ballots its ended envs and lane 0 posts the count; (barrier) thread 0 turns the wave counts
// into their exclusive scan and the chunk's total; (barrier) a lane's rank is the ranks of the chunks before (`base`),
// plus the waves before its own, plus the set lanes below it; (barrier, before the next chunk's counts overwrite the
// scan).  Every thread of the workgroup must call it (barriers), and f must not touch wsum.
template <class F>
__device__ __forceinline__ long long ranked_walk(long long E, const uint8_t* reset, long long* wsum, F f) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    long long base = 0;
    for (long long c0 = 0; c0 < E; c0 += kEpisodeThreads) {
        const long long e = c0 + t;
        const bool ended = e < E && reset[e] != 0;
        const unsigned long long m = __ballot(ended);
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        if (t == 0) {
            long long s = 0;
            for (int k = 0; k < kEpisodeWaves; ++k) { const long long v = wsum[k]; wsum[k] = s; s += v; }
            wsum[kEpisodeWaves] = s;
        }
        __syncthreads();
        if (ended) f(e, base + wsum[w] + __popcll(m & ((1ull << lane) - 1ull)));
        base += wsum[kEpisodeWaves];
        __syncthreads();
    }
    return base;
}

// The rings' append rule: a step's C ended envs are episodes total .. total + C - 1 in ascending env order, and
// episode total + r goes to slot (total + r) % W.  Only the ranks r >= first = max(0, C - W) are written -- the others
// would be overwritten within the step -- so every slot has exactly one writer: plain stores.  0 <= slot < W.
__device__ __forceinline__ long long ring_slot(long long total, long long r, int W) { return (total + r) % W; }

// ---- the per-agent episode accumulators (MARL): acc_return / acc_length [E][N] and acc_steps [E] hold the open episode
// of every env.  One thread owns an env and loops its N agents in index order, so every float64 sum has one fixed order
// and the same inputs give the same bits.
// one step of env e: the reward of every agent marked live at the step's start and one step into its accumulators (the
// reward of an agent that is not live is never loaded), and one env step; returns the episode's env steps so far
__device__ __forceinline__ int episode_accumulate(long long e, int N, const uint8_t* live, const float* reward,
                                                  double* acc_return, int* acc_length, int* acc_steps) {
    const long long r0 = e * N;
    for (int i = 0; i < N; ++i) {
        if (live[r0 + i]) {
            acc_return[r0 + i] += (double)reward[r0 + i];
            acc_length[r0 + i] += 1;
        }
    }
    const int steps = acc_steps[e] + 1;
    acc_steps[e] = steps;
    return steps;
}

// env e's episode into row `dst` of agent_return / agent_length ([rows][N]); returns the episode's return, the agents'
// returns added in index order
__device__ __forceinline__ double episode_file(long long e, int N, const double* acc_return, const int* acc_length,
                                               long long dst, double* agent_return, int* agent_length) {
    const long long r0 = e * N;
    double sum = 0.0;
    for (int i = 0; i < N; ++i) {
        const double r = acc_return[r0 + i];
        agent_return[dst * N + i] = r;
        agent_length[dst * N + i] = acc_length[r0 + i];
        sum += r;
    }
    return sum;
}

// env e's per-agent accumulators back to zero (acc_steps[e] is the caller's)
__device__ __forceinline__ void episode_zero(long long e, int N, double* acc_return, int* acc_length) {
    for (int i = 0; i < N; ++i) {
        acc_return[e * N + i] = 0.0;
        acc_length[e * N + i] = 0;
    }
}

// the wrapper's self.agents at the start of a step (rllib_envs/marl_wrapper.py): agent i < NUM_DRONES and not dropped
// out; env_n / env_active are the handle's envi rows 0 and 7
__device__ __forceinline__ bool agent_live(const int* env_n, const int* env_active, long long e, int i) {
    return i < env_n[e] && ((env_active[e] >> i) & 1);
}

// ---- the evaluation tables.  SB3 evaluate_policy's episode_count_targets[e] = (n_eval_episodes + e) // n_envs.  (e
// before n_eval: with this parameter order the begin kernels compile to the instructions they had with the rule inline)
__device__ __forceinline__ int eval_quota(long long e, long long n_eval, long long E) { return (int)((n_eval + e) / E); }

// `remaining` drops by the wave's number of recorded episodes in one integer atomic per wave (ballot + popcount):
// integer adds commute, so the result does not depend on the order the waves arrive in.  Every lane of the wave must
// get here.
__device__ __forceinline__ void drop_remaining(long long* remaining, bool rec) {
    const unsigned long long m = __ballot(rec);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long*>(remaining), 0ull - (unsigned long long)__popcll(m));
}

}  // namespace ch
