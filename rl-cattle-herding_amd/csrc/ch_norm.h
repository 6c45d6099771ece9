// ch_norm.h — what ch_norm.hip (the kernels of the device-side VecNormalize) and ch_api_norm.cpp (its C ABI,
// include/cattleherd.h ch_norm_*) share: the launch arguments and the scratch layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ch {

// ---- geometry -------------------------------------------------------------------------------------------------
constexpr int kNormThreads = 256;      // every obs kernel's workgroup
constexpr int kNormTile = 64;          // columns per workgroup
constexpr int kNormBlockRows = 64;     // rows a workgroup holds in registers at a time (one sub-block)
constexpr int kNormMaxChunks = 256;    // row chunks per matrix at most: what the merge walks per column
constexpr int kNormApplyRows = 256;    // rows per workgroup of k_norm_apply
constexpr int kRewardThreads = 1024;   // the reward kernel's workgroup
constexpr int kRewardPer = 4;          // envs per thread: one workgroup takes kRewardThreads * kRewardPer envs

// rows per chunk of k_norm_moments (a multiple of kNormBlockRows) and the chunks that makes
inline long long norm_chunk_rows(long long rows) {
    const long long blocks = (rows + kNormBlockRows - 1) / kNormBlockRows;
    return kNormBlockRows * ((blocks + kNormMaxChunks - 1) / kNormMaxChunks);
}
inline int norm_chunks(long long rows) {
    const long long cr = norm_chunk_rows(rows);
    return (int)((rows + cr - 1) / cr);
}
inline int reward_chunks(long long n) { return (int)((n + kRewardThreads * kRewardPer - 1) / (kRewardThreads * kRewardPer)); }

// The scratch, in doubles.  The obs update: part_mean [chunks][dim], part_m2 [chunks][dim] (moments of x - pivot, the
// pivot of column c being x[0][c]), part_n [chunks], count_old [1].  The reward kernel beyond one workgroup:
// {n, mean, M2} per chunk (of ret - pivot, the pivot being the running ret_mean).
inline long long norm_obs_scratch(long long rows, long long dim) {
    const long long c = norm_chunks(rows);
    return 2 * c * dim + c + 1;
}
inline long long norm_reward_scratch(long long n) { return 3LL * reward_chunks(n); }

struct NormObsArgs {
    const float* x;            // [rows][dim]
    float* y;                  // apply: [rows][dim] (may be x)
    const uint8_t* row_mask;   // apply: optional [rows]
    long long rows, chunk_rows;
    int dim, chunks;
    double *mean, *var, *count;   // the running statistics [dim], [dim], [1]
    double* scratch;
    double clip, eps;
    int passthrough;           // apply: y = x (norm_obs off)
};

struct NormRewardArgs {
    long long n;
    const float* reward;       // [n]
    const uint8_t *terminated, *truncated;   // [n]
    float* reward_out;         // [n]
    double* ret;               // [n]
    double* stats;             // ret_mean, ret_var, ret_count
    double* scratch;
    double gamma, clip, eps;
    int training, norm_reward, chunks;
};

struct NormBeginArgs {
    int dim;
    long long n;
    double *mean, *var, *count, *stats, *ret;
};

hipError_t launch_norm_begin(const NormBeginArgs& a, hipStream_t st);
hipError_t launch_norm_obs_update(const NormObsArgs& a, hipStream_t st);   // k_norm_moments, k_norm_merge
hipError_t launch_norm_obs_apply(const NormObsArgs& a, hipStream_t st);    // k_norm_apply
hipError_t launch_norm_reward(const NormRewardArgs& a, hipStream_t st);

}  // namespace ch
