// ch_ppo.h -- the native PPO minibatch update (ch_ppo.hip) as its host file (ch_api_ppo.cpp) sees it: the flat
// parameter order, the scratch layout and the three launches of one minibatch step.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ch {

constexpr int kPpoTile = 16;        // minibatch rows per workgroup of the forward / backward kernel
constexpr int kPpoMaxHidden = 256;  // widest hidden layer
constexpr int kPpoMaxAct = 64;      // widest action
constexpr int kPpoMaxSeg = 13;      // parameter tensors: 2 nets x 3 layers x (weight, bias) + log_std

// one MLP of the actor-critic: n_hidden tanh layers, then the linear head (action_net / value_net)
struct PpoMlp {
    int layers;          // n_hidden + 1
    int dims[4];         // obs_dim, hidden widths, head width
    float* w[3];         // nn.Linear layout [dims[i + 1]][dims[i]]
    float* b[3];
    long long goff_w[3]; // offsets of the layer's weight / bias in the flat parameter order
    long long goff_b[3];
};

struct PpoNet {
    PpoMlp net[2];       // 0 the policy MLP + action_net, 1 the value MLP + value_net
    float* log_std;
    long long goff_log_std;
    long long n_params;
    int obs_dim, act_dim;
};

struct PpoHp {
    double lr, beta1, beta2, eps, clip_range, ent_coef, vf_coef, max_grad_norm;
    int normalize_advantage;
};

struct PpoData {
    const float* obs;
    const float* actions;
    const float* old_log_prob;
    const float* advantages;
    const float* returns;
    long long rows;
};

// Scratch (floats) for minibatches of up to `batch` rows, rows padded to whole tiles (bp):
//   per net: act[l] [bp][dims[l + 1]] hidden activations (l < n_hidden), dz[l] [bp][dims[l + 1]] (every layer)
//   tile_stat [tiles][2]   sums of the surrogate minimum and of the squared value error
//   tile_dls  [tiles][act] log_std gradient partials
//   misc      [4]          mean entropy
//   partial   [workgroups] sum-of-squares partials of the gradient, one per workgroup that produced a piece of it
//   grad      [n_params]   the flat gradient (ch_ppo_train)
struct PpoScratch {
    long long act[2][2], dz[2][3], tile_stat, tile_dls, misc, partial, grad, total;
    int tiles, bp;
};
void ppo_scratch_layout(const PpoNet& n, long long batch, PpoScratch& s);

// the three launches of one minibatch step.  ppo_launch_grad: forward, loss and backward per (row tile, net), then the
// weight-gradient grid; `bump_step` makes the latter increment *step_dev (the Adam step this gradient is for).
// ppo_launch_sumsq: the sum-of-squares partials of a given flat gradient (ch_ppo_adam), increments *step_dev.
// ppo_launch_adam: every workgroup sums the partials in order, forms the clip coefficient and updates its slice;
// workgroup 0 writes stats4 when it is not NULL.  ppo_launch_stats: stats4 alone (ch_ppo_grad).
hipError_t ppo_launch_grad(const PpoNet& n, const PpoHp& hp, const PpoData& d, const long long* idx, long long batch,
                           float* grad, float* scratch, const PpoScratch& s, long long* step_dev, int* n_partials,
                           hipStream_t st);
hipError_t ppo_launch_sumsq(const PpoNet& n, const float* grad, float* scratch, const PpoScratch& s, long long* step_dev,
                            int* n_partials, hipStream_t st);
hipError_t ppo_launch_adam(const PpoNet& n, const PpoHp& hp, const float* grad, float* m, float* v,
                           const long long* step_dev, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                           float* stats4, hipStream_t st);
hipError_t ppo_launch_stats(const PpoNet& n, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                            float* stats4, hipStream_t st);

}  // namespace ch
