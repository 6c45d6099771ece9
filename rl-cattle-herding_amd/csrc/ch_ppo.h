// ch_ppo.h -- the native PPO minibatch update (ch_ppo.hip) as its host file (ch_api_ppo.cpp) sees it: the flat
// parameter order, the scratch layout and the three launches of one minibatch step.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ch {

constexpr int kPpoTile = 16;        // minibatch rows per workgroup of the forward / backward kernel
constexpr int kPpoMaxHidden = 256;  // widest hidden layer
constexpr int kPpoMaxAct = 64;      // widest policy head (SB3: act_dim; RLlib: 2 * act_dim, the mean then log_std)
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

// The loss / head flavour the three kernels are compiled for.
//   kPpoSb3    SB3 PPO.train: the head is the mean, log_std a free parameter; per-minibatch advantage normalisation,
//              MSE value loss, clip_grad_norm_.
//   kPpoRllib  RLlib's PPO learner for the shared DTDE policy: the head is [mean, raw log_std] (log_std = the raw
//              value clamped to +-log_std_clip), no free log_std; the KL penalty with its coefficient read from the
//              device, the clipped value loss, advantages taken as given, the global-norm clip optional.
enum PpoFlavour { kPpoSb3 = 0, kPpoRllib = 1 };

// statistics per minibatch step.  kPpoSb3: policy loss, value loss, mean entropy, gradient norm; kPpoRllib: policy
// loss, clipped value loss, mean entropy, mean KL, gradient norm.
constexpr int ppo_n_stats(PpoFlavour f) { return f == kPpoRllib ? 5 : 4; }

struct PpoNet {
    PpoMlp net[2];       // 0 the policy MLP + action_net (RLlib: actor encoder + pi), 1 the value MLP + value_net
    float* log_std;      // kPpoSb3 only
    long long goff_log_std;
    long long n_params;
    int obs_dim, act_dim;
    int flavour;
};

struct PpoHp {
    double lr, beta1, beta2, eps, clip_range, ent_coef, vf_coef, max_grad_norm;   // max_grad_norm <= 0 (kPpoRllib): no clip
    int normalize_advantage;
    // kPpoRllib
    double vf_clip, log_std_clip;
    const float* kl_coeff_dev;
};

struct PpoData {
    const float* obs;
    const float* actions;
    const float* old_log_prob;
    const float* advantages;
    const float* returns;
    long long rows;
    const float* old_dist;   // kPpoRllib: [rows][2 * act_dim], the mean then the clamped log_std of the sampling policy
};

// Scratch (floats) for minibatches of up to `batch` rows, rows padded to whole tiles (bp):
//   per net: act[l] [bp][dims[l + 1]] hidden activations (l < n_hidden), dz[l] [bp][dims[l + 1]] (every layer)
//   tile_stat [tiles][2]   sums of the surrogate minimum and of the squared value error; with log_stats then
//             [tiles][2] the sums of SB3's diagnostics (ratio - 1) - log_ratio (evaluated in float64, rounded
//             once) and |ratio - 1| > clip_range, behind the current minibatch's tiles (kPpoRllib: [tiles][4],
//             with the sums of the rows' entropies and KL divergences)
//   tile_dls  [tiles][act] log_std gradient partials (kPpoSb3)
//   misc      [4]          mean entropy (kPpoSb3); kPpoRllib keeps the training log's region here (written only with
//             log_stats): [4] vf_loss_coeff, entropy_coeff, the KL coefficient; [tiles] the tiles' sums of unclipped
//             squared value errors, then [bp][2] each row's (value, value target), behind the current minibatch's tiles
//   partial   [workgroups] sum-of-squares partials of the gradient, one per workgroup that produced a piece of it
//   grad      [n_params]   the flat gradient (ch_ppo_train)
struct PpoScratch {
    long long act[2][2], dz[2][3], tile_stat, tile_dls, misc, partial, grad, total;
    int tiles, bp;
};
void ppo_scratch_layout(const PpoNet& n, long long batch, PpoScratch& s);

// the three launches of one minibatch step.  ppo_launch_grad: forward, loss and backward per (row tile, net), then the
// weight-gradient grid; `bump_step` makes the latter increment *step_dev (the Adam step this gradient is for);
// log_stats (kPpoSb3): the forward-backward kernel's variant that also leaves the tiles' sums of SB3's two diagnostics.
// ppo_launch_sumsq: the sum-of-squares partials of a given flat gradient (ch_ppo_adam), increments *step_dev.
// ppo_launch_adam: every workgroup sums the partials in order, forms the clip coefficient and updates its slice;
// workgroup 0 writes the step's statistics (ppo_n_stats of them) to `stats` when it is not NULL; log_stats (kPpoSb3):
// CH_PPO_LOG_STATS of them, with approx_kl and clip_fraction (ch_ppo_train_log).  log_stats with kPpoRllib
// (ch_marl_ppo_train_log): both launches take the kPpoRllibLog kernels, which leave CH_MARL_PPO_LOG_STATS statistics,
// with vf_loss_unclipped, total_loss and vf_explained_var.  ppo_launch_stats: the statistics alone (ch_ppo_grad,
// ch_marl_ppo_grad).
hipError_t ppo_launch_grad(const PpoNet& n, const PpoHp& hp, const PpoData& d, const long long* idx, long long batch,
                           float* grad, float* scratch, const PpoScratch& s, long long* step_dev, int* n_partials,
                           hipStream_t st, bool log_stats = false);
hipError_t ppo_launch_sumsq(const PpoNet& n, const float* grad, float* scratch, const PpoScratch& s, long long* step_dev,
                            int* n_partials, hipStream_t st);
hipError_t ppo_launch_adam(const PpoNet& n, const PpoHp& hp, const float* grad, float* m, float* v,
                           const long long* step_dev, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                           float* stats, hipStream_t st, bool log_stats = false);

// ch_ppo_train_opt's options (kPpoSb3): SB3's target_kl and clip_range_vf, <= 0 for None.
struct PpoOpt {
    double target_kl, clip_range_vf;
    const float* old_values;   // [rows], read when clip_range_vf > 0
    int32_t* stop_dev;         // the stop word, read and set when target_kl > 0
};
// One minibatch step of ch_ppo_train_opt: the three launches of ppo_launch_grad + ppo_launch_adam with log_stats, as
// their option variants (ch_ppo.hip: k_ppo_fb_opt, k_ppo_dw_opt, k_ppo_adam_opt) over the gradient region of
// `scratch`.  stats7: this step's row of CH_PPO_OPT_STATS.  With the stop word set the launches return at entry (the
// Adam launch leaves the row NaN with state -1); a minibatch whose approx_kl exceeds 1.5 * target_kl writes its
// statistics, sets the word and updates nothing, *step_dev included.
hipError_t ppo_launch_step_opt(const PpoNet& n, const PpoHp& hp, const PpoData& d, const PpoOpt& opt, const long long* idx,
                               long long batch, float* m, float* v, long long* step_dev, float* scratch,
                               const PpoScratch& s, float* stats7, hipStream_t st);
hipError_t ppo_launch_stats(const PpoNet& n, float* scratch, const PpoScratch& s, int n_partials, long long batch,
                            float* stats, hipStream_t st);

}  // namespace ch
