// ch_ppo.h -- the native PPO minibatch update (ch_ppo.hip) as its host file (ch_api_ppo.cpp) sees it: the kernel
// flavours, the step plan (which kernels an ABI entry launches), the flat parameter order, the scratch layout and the
// launches of one minibatch step.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cattleherd.h"   // the statistics rows' widths

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

// ---- the kernel flavours: the kernels' template parameter `int F` --------------------------------------------------
// Two bases, the head and the loss (PpoNet::flavour is one of them; all three kernels have both):
//   kPpoSb3       SB3 PPO.train: the head is the mean, log_std a free parameter; per-minibatch advantage
//                 normalisation, MSE value loss, clip_grad_norm_.
//   kPpoRllib     RLlib's PPO learner for the shared DTDE policy: the head is [mean, raw log_std] (log_std = the raw
//                 value clamped to +-log_std_clip), no free log_std; the KL penalty with its coefficient read from the
//                 device, the clipped value loss, advantages taken as given, the global-norm clip optional.
// Four more, each its base plus one thing, as kernels of their own so that the base's code carries none of it:
//   kFbSb3Log     kPpoSb3 + log partials: the tiles' sums of SB3's approx_kl and clip_fraction terms, evaluated in
//                 float64 (k_ppo_fb only; k_ppo_adam<kPpoSb3> turns them into two statistics under `update` bit 1).
//   kPpoRllibLog  kPpoRllib + log partials: the critic workgroups leave the loss's coefficients, each tile's sum of
//                 unclipped squared value errors and each row's (value, target) in the scratch region `misc`
//                 (k_ppo_fb), which k_ppo_adam turns into vf_loss_unclipped, total_loss and vf_explained_var.
//   kFbSb3Opt     kFbSb3Log + stop word: the early return behind ch_ppo_train_opt's KL gate (k_ppo_fb_opt only).
//   kFbSb3OptVf   kFbSb3Opt + value clip: SB3's clip_range_vf against the rollout's value predictions.
// (ch_ppo.hip's header: which kernel is instantiated for which flavour.)
enum PpoFlavour { kPpoSb3 = 0, kPpoRllib = 1, kFbSb3Log = 2, kPpoRllibLog = 3, kFbSb3Opt = 4, kFbSb3OptVf = 5 };
constexpr bool ppo_rllib(int F) { return F == kPpoRllib || F == kPpoRllibLog; }
constexpr bool fb_opt(int F) { return F == kFbSb3Opt || F == kFbSb3OptVf; }

// ---- the kernel table's rows (ch_ppo.hip kPpoTable: one per instantiation) and the step plan ----------------------
enum PpoKernel {
    kPpoNone = 0, kPpoFb0, kPpoFb1, kPpoFb2, kPpoFb3, kPpoFbOpt4, kPpoFbOpt5, kPpoDw0, kPpoDw1, kPpoDwOpt, kPpoSumsq,
    kPpoAdam0, kPpoAdam1, kPpoAdam3, kPpoAdamOpt, kPpoKernels
};
const char* ppo_kernel_name(int row);   // NULL past the table

// What one minibatch step of an ABI entry launches.  Statistics per step, `n_stats` of them -- kPpoSb3: policy loss,
// value loss, mean entropy, gradient norm (4); kPpoRllib: policy loss, clipped value loss, mean entropy, mean KL,
// gradient norm (5); with log_stats / options the rows of CH_PPO_LOG_STATS, CH_MARL_PPO_LOG_STATS, CH_PPO_OPT_STATS.
struct PpoPlan {
    int fb, dw, adam;   // PpoKernel rows of the forward-backward, weight-gradient and Adam launches
    int update;         // AdamArgs::update: 1 Adam, 3 Adam with the log's statistics (0, the statistics alone: ppo_launch_stats)
    int n_stats;        // width of a statistics row
    bool opts;          // the three kernels take the option structs (FbOpt, GateArgs) behind their arguments
};

// The plan of (base flavour, log_stats, the call has options, KL gate armed, value clip on): pure, the only place that
// knows which instantiation serves what.  `opts` is ch_ppo_train_opt, whose kernels and CH_PPO_OPT_STATS row do not
// depend on whether an option is on: the gate only decides if the stop word is handed on (ppo_stop), the value clip
// picks the forward-backward kernel.  What does not exist -- options with kPpoRllib, gate or clip without options, a
// flavour that is no base -- gives the empty plan (fb == kPpoNone).
inline PpoPlan ppo_plan(int flavour, bool log_stats, bool opts, bool gate, bool vclip) {
    const bool rllib = flavour == kPpoRllib;
    if ((flavour != kPpoSb3 && !rllib) || (opts && rllib) || ((gate || vclip) && !opts)) return {};
    if (opts) return {vclip ? kPpoFbOpt5 : kPpoFbOpt4, kPpoDwOpt, kPpoAdamOpt, 3, CH_PPO_OPT_STATS, true};
    if (rllib) return log_stats ? PpoPlan{kPpoFb3, kPpoDw1, kPpoAdam3, 3, CH_MARL_PPO_LOG_STATS, false}
                                : PpoPlan{kPpoFb1, kPpoDw1, kPpoAdam1, 1, 5, false};
    return log_stats ? PpoPlan{kPpoFb2, kPpoDw0, kPpoAdam0, 3, CH_PPO_LOG_STATS, false}
                     : PpoPlan{kPpoFb0, kPpoDw0, kPpoAdam0, 1, 4, false};
}

// ch__ppo_last_step: the rows of the minibatch step launched last in this process -- host side only.  ch_*_adam leaves
// {kPpoNone, kPpoSumsq, its Adam row}.
struct PpoLastStep { int fb, dw, adam, update, adam_grid; };
extern PpoLastStep g_ppo_last_step;

struct PpoNet {
    PpoMlp net[2];       // 0 the policy MLP + action_net (RLlib: actor encoder + pi), 1 the value MLP + value_net
    float* log_std;      // kPpoSb3 only
    long long goff_log_std;
    long long n_params;
    int obs_dim, act_dim;
    int flavour;         // kPpoSb3 or kPpoRllib
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

// ch_ppo_train_opt's options (kPpoSb3): SB3's target_kl and clip_range_vf, <= 0 for None.
struct PpoOpt {
    double target_kl, clip_range_vf;
    const float* old_values;   // [rows], read when clip_range_vf > 0
    int32_t* stop_dev;         // the stop word, read and set when target_kl > 0
};
// the stop word as the kernels get it: NULL (no gate) unless target_kl > 0, a value clip alone included
inline int32_t* ppo_stop(const PpoOpt& o) { return o.target_kl > 0.0 ? o.stop_dev : nullptr; }

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
// a call's layout as a minibatch of `batch` rows (at most the layout's) uses it: the regions stay, the tiles are its own
inline PpoScratch ppo_scratch_for(PpoScratch s, long long batch) {
    s.tiles = (int)((batch + kPpoTile - 1) / kPpoTile); s.bp = s.tiles * kPpoTile;
    return s;
}

// The launches of one minibatch step, by the call's plan `p`; `opt` is read when p.opts (ch_ppo_train_opt: with the
// stop word set the three launches return at entry, the Adam launch leaving the row NaN with state -1; a minibatch
// whose approx_kl exceeds 1.5 * target_kl writes its statistics, sets the word and updates nothing, *step_dev included).
// ppo_launch_grad: p.fb -- forward, loss and backward per (row tile, net) -- then p.dw, the weight-gradient grid, which
// increments *step_dev (the Adam step this gradient is for) unless it is NULL.
// ppo_launch_sumsq: the sum-of-squares partials of a given flat gradient (ch_ppo_adam), increments *step_dev.
// ppo_launch_adam: p.adam with p.update -- every workgroup sums the partials in order, forms the clip coefficient and
// updates its slice; workgroup 0 writes the step's p.n_stats statistics to `stats` when it is not NULL.
// ppo_launch_stats: the same launch without hyper-parameters -- update 0 and one workgroup, the statistics alone
// (ch_ppo_grad, ch_marl_ppo_grad).
hipError_t ppo_launch_grad(const PpoPlan& p, const PpoNet& n, const PpoHp& hp, const PpoData& d, const PpoOpt* opt,
                           const long long* idx, long long batch, float* grad, float* scratch, const PpoScratch& s,
                           long long* step_dev, int* n_partials, hipStream_t st);
hipError_t ppo_launch_sumsq(const PpoNet& n, const float* grad, float* scratch, const PpoScratch& s, long long* step_dev,
                            int* n_partials, hipStream_t st);
hipError_t ppo_launch_adam(const PpoPlan& p, const PpoNet& n, const PpoHp* hp, const PpoOpt* opt, const float* grad,
                           float* m, float* v, const long long* step_dev, float* scratch, const PpoScratch& s,
                           int n_partials, long long batch, float* stats, hipStream_t st);
inline hipError_t ppo_launch_stats(const PpoPlan& p, const PpoNet& n, float* scratch, const PpoScratch& s, int n_partials,
                                   long long batch, float* stats, hipStream_t st) {
    return ppo_launch_adam(p, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, scratch, s, n_partials, batch, stats, st);
}

// ---- the population update (ch_ppo_train_pop): P members of one architecture in the same three launches ------------
// The population kernels (ch_ppo.hip kPpoPopTable: one row per instantiation) run ch_ppo_train_opt's bodies on the
// member that a grid coordinate names -- blockIdx.z of k_ppo_fb_pop, blockIdx.y of k_ppo_dw_pop and k_ppo_adam_pop --
// with that member's arguments read from a device table instead of the kernel-argument segment.  kPpoTable and
// g_ppo_last_step know nothing of them.
enum PpoPopKernel { kPpoPopFb4 = 0, kPpoPopFb5, kPpoPopDw, kPpoPopAdam, kPpoPopKernels };
const char* ppo_pop_kernel_name(int row);   // NULL outside the table

// the rows of one population step, by (value clip on): pure, like ppo_plan.  The statistics rows are CH_PPO_OPT_STATS
// wide and the Adam launch's update bits are ppo_plan's for options (3).
struct PpoPopPlan { int fb, dw, adam; };
inline PpoPopPlan ppo_pop_plan(bool vclip) { return {vclip ? kPpoPopFb5 : kPpoPopFb4, kPpoPopDw, kPpoPopAdam}; }

// one member as ch_ppo_train_opt would take it
struct PpoMember {
    PpoNet n; PpoHp hp; PpoData d; PpoOpt o;
    const long long* idx;
    float* m; float* v; long long* step_dev;
    float* stats;     // the call's first row
    float* scratch;
};
// The three argument tables: arrays, indexed by member, of what k_ppo_{fb,dw,adam}_opt take as kernel arguments (the
// entries' sizes: ppo_pop_entry_sizes).  A table is written on the host (ppo_pop_fill) and read on the device.
struct PpoPopTables { void* fb; void* dw; void* adam; };
struct PpoPopSizes { size_t fb, dw, adam; };
PpoPopSizes ppo_pop_entry_sizes();
struct PpoPopGeom { int tiles, dw_grid, adam_grid; };   // the same for every member: it follows from the architecture
// Member `i`'s entries for minibatches of `batch` rows that start at mb.idx[0] and write mb.stats' first row, built by
// the code that builds ch_ppo_train_opt's kernel arguments; a step adds its offsets (ppo_pop_launch).
void ppo_pop_fill(const PpoPopTables& host, int i, const PpoMember& mb, long long batch, const PpoScratch& s, PpoPopGeom* g);
// one minibatch step of `members` members: rows [idx_off, idx_off + batch) of each member's idx, statistics at
// stats + stats_off floats
hipError_t ppo_pop_launch(const PpoPopPlan& p, const PpoPopTables& dev, const PpoPopGeom& g, int members,
                          long long idx_off, long long stats_off, hipStream_t st);

}  // namespace ch
