/*
 * cattleherd.h — C ABI of the MI355X-native batched cattle-herding environment (libcattleherd.so).
 *
 * The reference (BenCooper305/RL-Cattle-Herding, gym_pybullet_drones/) has no native FFI: its
 * hot path is a Python gym.Env whose step() drives PyBullet.  This ABI replaces that env object
 * for a whole batch of environments at once; each entry point names the reference interface it
 * stands in for (paths relative to gym_pybullet_drones/).  INTEGRATION.md shows the ctypes
 * binding and the Gymnasium / SB3 / RLlib adapters layered on top.
 *
 * Conventions
 *   - Every call returns an int status: CH_OK (0) or a negative CH_ERR_*; ch_last_error() gives the
 *     message.  No exception crosses the ABI.  NaN/Inf in the simulation propagate exactly like the
 *     reference (e.g. the CTDE reward is NaN for 2 drones — see DESIGN.md "Quirks").
 *   - Buffers passed to ch_reset/ch_step are DEVICE pointers owned by the caller (e.g. torch
 *     tensors' data_ptr()); state is owned by the handle and lives in HBM.
 *   - One handle <-> one device.  Work is enqueued on the given hipStream_t (NULL = default stream)
 *     and is asynchronous until the caller synchronises.  One host thread per handle.
 *   - Layouts (E = n_envs, N = num_drones from the config, R = obs rows, K = reward columns):
 *       actions       float32 [E][N][4]          (VEL action, BaseRLAviary.py:185-222)
 *       obs           float32 [E][R][86]         R = 12 (CTDE, BaseRLAviary.py:272-342) or N (MARL,
 *                                                BaseMARLAviary.py:253-303)
 *       reward        float32 [E][K]             K = 1 (CTDE) or N (MARL, per agent)
 *       terminated    uint8   [E][K]
 *       truncated     uint8   [E][K]
 *       agent_active  uint8   [E][N]             MARL wrapper's live agents (marl_wrapper.py:112-113)
 */
#ifndef CATTLEHERD_H
#define CATTLEHERD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CH_ABI_VERSION 6

enum {
    CH_OK = 0,
    CH_ERR_INVALID = -1,     /* bad argument / configuration (reference: print+exit / ValueError) */
    CH_ERR_DEVICE = -2,      /* HIP runtime error */
    CH_ERR_NOMEM = -3,
    CH_ERR_UNSUPPORTED = -4  /* configuration the reference itself cannot run (e.g. 1 drone) */
};

enum { CH_MODE_CTDE = 0, CH_MODE_MARL = 1 };
enum { CH_PREC_F64 = 0, CH_PREC_F32 = 1 };
/* Physics enum, in the reference's order (utils/enums.py:13-21; dispatch BaseAviary.py:420-450) */
enum {
    CH_PHYS_PYB = 0,          /* _physics + p.stepSimulation (default) */
    CH_PHYS_DYN = 1,          /* explicit _dynamics + _integrateQ (BaseAviary.py:1043-1118); cattle stay put */
    CH_PHYS_PYB_GND = 2,      /* + _groundEffect (943-980) */
    CH_PHYS_PYB_DRAG = 3,     /* + _drag (982-1011) */
    CH_PHYS_PYB_DW = 4,       /* + _downwash (1013-1041) */
    CH_PHYS_PYB_GND_DRAG_DW = 5,
    CH_PHYS_DYN_RK4 = 6       /* option, not in the reference: DYN's equations of motion integrated by classic
                                 RK4 per substep (q renormalised); cattle stay put as under DYN */
};

/* Flags for ch_step_io.flags */
#define CH_STEP_AUTORESET      0x1u  /* reset finished envs in the same launch (SB3 VecEnv semantics) */
#define CH_STEP_RANDOM_ACTIONS 0x2u  /* draw U[-1,1) actions on device (Philox4x32-10, key = seed,
                                        counter = (step, drone, env)); written to actions_out if set */

/* Environment configuration.  Mirrors the constructor of CattleAviary (sb3_envs/CattleAviary.py:14-28)
 * / MARLCattleAviary (rllib_envs/MARLCattleAviary.py:14-28) plus the knobs the reference hard-codes. */
typedef struct ch_config {
    int32_t abi_version;      /* = CH_ABI_VERSION */
    int32_t mode;             /* CH_MODE_CTDE (sb3_envs) or CH_MODE_MARL (rllib_envs) */
    int32_t num_drones;       /* constructor num_drones: action rows (BaseRLAviary.py:80), <= 12 */
    int32_t num_cattle;       /* num_cattle, <= 64 (reference spawns at most 16, BaseAviary.py:611) */
    int32_t min_drones;       /* NUM_DRONES drawn per reset in [min, max] (BaseAviary.py:307);      */
    int32_t max_drones;       /*   -1 = num_drones (pinned)                                          */
    int32_t curriculum_level; /* starting level; -1 = reference default (CTDE 7, MARL 0)             */
    int32_t ctrl_freq;        /* 60 (CattleAviary.py:23) */
    int32_t pyb_freq;         /* 240 (CattleAviary.py:22) */
    int32_t compat;           /* 1 = reproduce reference quirks bit-for-bit (DESIGN.md "Quirks") */
    int32_t precision;        /* CH_PREC_F64 (reference arithmetic) or CH_PREC_F32 */
    int32_t torque_world;     /* link_lag = 0 only: 1 = applyExternalTorque(LINK_FRAME) acts in world frame.  With
                                 link_lag = 1 the z torque turns with the cached link frame whatever this says: the
                                 recorded real-PyBullet trace rejects a world-frame z torque there (2e-5 vs 2e-13
                                 m/s by step 4) */
    int32_t gyro;             /* 1 = gyroscopic term (btMultiBody default) */
    int32_t marl_wrapper;     /* MARL only: 1 = RLlibMultiAgentWrapper.step semantics (marl_wrapper.py:77-119:
                                 per-agent recomputation, finished agents drop out, episode ends when all
                                 agents terminated); 0 = bare MARLCattleAviary.step dicts
                                 (rllib_envs/BaseAviary.py:425-431) */
    double damping;           /* btMultiBody default linear/angular damping 0.04 */
    uint64_t seed;            /* Philox key for resets and random actions */
    int64_t env_id_offset;    /* global index of env 0 (multi-GPU sharding) */
    const double* spawn_table;/* host [spawn_scenarios][spawn_cows][2]; NULL = built-in table
                                 (config/cattle_positions.yaml, 100 x 16; extended for > 16 cows) */
    int32_t spawn_scenarios;
    int32_t spawn_cows;
    int32_t physics;          /* CH_PHYS_* (CattleAviary ctor `physics`, CattleAviary.py:21) */
    int32_t eval_metrics;     /* 1 (default) = keep update_evaluation_metrics' per-drone episode distance on
                                 the device every step (BaseAviary.py:1406-1435), read with ch_get_eval */
    int32_t link_lag;         /* 1 (default) = _physics' applyExternalForce/Torque(LINK_FRAME) (BaseAviary.py:907-939)
                                 rotate by the link transform Bullet cached at the previous substep (the
                                 attitude one substep old, state components qlag): what the recorded real-PyBullet
                                 trace shows; 0 = the current attitude (rounds 1-4 model) */
} ch_config;

typedef struct ch_handle ch_handle;

/* Fill *cfg with the reference defaults for `mode` (CattleAviary / MARLCattleAviary constructors). */
int ch_default_config(ch_config* cfg, int32_t mode, int32_t num_drones, int32_t num_cattle);

/* Replaces: CattleAviary.__init__ (sb3_envs/CattleAviary.py:14-105) — one env — with n_envs envs on
 * `device`.  Allocates the SoA state in HBM and uploads the spawn table. */
int ch_create(const ch_config* cfg, int64_t n_envs, int32_t device, ch_handle** out);

/* Replaces: BaseAviary.close (sb3_envs/BaseAviary.py:498-503). */
int ch_destroy(ch_handle* h);

/* Message of the last failing call on `h` (or of the last failing ch_create when h == NULL). */
const char* ch_last_error(const ch_handle* h);

/* Shapes: obs rows R and reward columns K. */
int ch_shape(const ch_handle* h, int64_t* n_envs, int32_t* obs_rows, int32_t* obs_cols, int32_t* reward_cols);

/* Replaces: BaseAviary.reset (sb3_envs/BaseAviary.py:280-331; rllib_envs/BaseAviary.py:280-318).
 * Resets the envs whose mask byte is non-zero (mask = NULL: all) and writes their initial
 * observation into obs (device, [E][R][86]); other envs' obs rows are left untouched.
 * A reset env's open episode is abandoned, as SB3's Monitor.reset drops its reward list: the running return and
 * length behind ch_step_io.episode_stats start again from zero, and the abandoned steps are counted in neither
 * CH_METRIC_EPISODES, CH_METRIC_RETURN_SUM nor CH_METRIC_LENGTH_SUM (CH_METRIC_STEPS and the other per-step sums keep
 * them).  The call has no agent_active output: a reset env's live agents are the first NUM_DRONES (ch_get_state).
 * A full reset (mask = NULL) first reads and clears the handle's sticky device error word: it synchronises `stream`
 * (so it blocks the host and cannot be captured into a HIP graph), and a device error an earlier step recorded and no
 * ch_sync / ch_metrics / ch_get_state has reported yet is returned as CH_ERR_DEVICE after the reset has been done
 * (the state is then the fresh reset's). */
int ch_reset(ch_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* ch_reset with the reset's random draws supplied by the caller instead of the device's Philox stream:
 * num_drones host int32[E] (NUM_DRONES of each reset env, BaseAviary.py:307) and/or cow_vel host
 * double[E][M][2] (the cattle spawn velocities 0.2 (cos a, sin a), BaseAviary.py:631-632); either may be
 * NULL.  With cattleherd/seeded.py replaying the reference's own seeded `random` / NumPy draws this
 * reproduces the reference's reset state bit for bit.  Synchronises `stream`. */
int ch_reset_with(ch_handle* h, const uint8_t* mask_dev, const int32_t* num_drones, const double* cow_vel,
                  float* obs_dev, void* stream);

typedef struct ch_step_io {
    const float* actions;      /* device [E][N][4]; ignored with CH_STEP_RANDOM_ACTIONS */
    float* actions_out;        /* optional: where device-drawn random actions are stored */
    float* obs;                /* device [E][R][86] (required) */
    float* reward;             /* device [E][K] (required) */
    uint8_t* terminated;       /* device [E][K] (required) */
    uint8_t* truncated;        /* device [E][K] (required) */
    float* terminal_obs;       /* optional device [E][R][86]: pre-reset obs of envs that auto-reset; leave NULL
                                  when not needed: the 16-env x 4-drone geometry then rebuilds reset envs
                                  without a workgroup sync (same outputs) */
    uint8_t* agent_active;     /* optional device [E][N]: MARL live-agent mask after this step */
    uint8_t* reset_happened;   /* optional device [E]: 1 where the env auto-reset in this call */
    uint32_t flags;            /* CH_STEP_* */
    uint32_t _pad;
    double* episode_stats;     /* optional device [E][2]: where an episode ends in this call, its return (the sum of
                                  the float64 rewards the reference returns) and length in steps -- SB3 Monitor's
                                  info["episode"] "r" and "l" (CTDECattleHerder.py:91-99); other rows untouched */
} ch_step_io;

/* Replaces: BaseAviary.step (sb3_envs/BaseAviary.py:335-465) for every env at once — VEL action →
 * DSLPIDControl → motor model → pyb_freq/ctrl_freq physics substeps → flocking every 2nd step →
 * observation → reward / terminated / truncated; with CH_STEP_AUTORESET, SB3 VecEnv auto-reset.
 * MARL mode additionally applies RLlibMultiAgentWrapper.step's per-agent recomputation
 * (rllib_envs/marl_wrapper.py:77-119). */
int ch_step(ch_handle* h, const ch_step_io* io, void* stream);

/* n_steps consecutive ch_step calls with the same io, in as few launches as the geometry allows: the steps run in one
 * launch in which every workgroup steps its envs back to back (k_step2_multi) -- the BASELINE
 * geometries under PYB without terminal observations; elsewhere one launch per step.  A buffer whose constant
 * observation bytes are not known to be in place (first use, after ch_set_state / invalidation) gets one plain
 * ch_step first.  The kernel reads its parameters from a device copy that is re-uploaded (stream-ordered) when they
 * change (from host memory, staged by the runtime at the call): use one stream per handle.  Under stream capture
 * (a HIP graph) the call records n_steps plain ch_step launches instead.  The outputs in io are those of the last step; state, auto-resets, metrics and the device-drawn
 * random actions (CH_STEP_RANDOM_ACTIONS: each step draws its own) equal n_steps ch_step calls bit for bit.  For
 * random-action rollouts and data generation; a policy that reads each step's observation calls ch_step.
 * Replaces: n_steps iterations of the reference's env.step loop (BaseAviary.step, sb3_envs/BaseAviary.py:335-465). */
int ch_step_n(ch_handle* h, const ch_step_io* io, int32_t n_steps, void* stream);

/* Host delivery of one step's outputs (the batched SB3 VecEnv and RLlib dict surfaces).
 * Replaces: what SubprocVecEnv.step_wait gathers from its worker processes -- obs (E, R, 86), rewards,
 * dones, and for the envs that ended info["terminal_observation"] and Monitor's info["episode"]
 * (CTDECattleHerder.py:91-99) -- and the arrays RLlibMultiAgentWrapper.step builds its per-agent dicts from
 * (marl_wrapper.py:97-119).  After ch_step on `stream`: copies the step's outputs from io's device buffers
 * into caller-owned host buffers (pinned host memory for full speed), then synchronises `stream`.
 *   - The observation copy moves only the first num_drones rows of every block: a CTDE (12, 86) block's rows
 *     >= num_drones are always zero, so the caller zero-fills `obs` once and they stay zero.
 *   - The envs that auto-reset in the step (io->reset_happened) are compacted on the device, in ascending env
 *     order: their count, indices, terminal observations (io->terminal_obs, whole blocks) and episode statistics
 *     (io->episode_stats: return, length).  Before the count is known the call copies a first part sized from the
 *     recent counts (twice the larger of the last count and its running mean, plus 8): one synchronisation when at
 *     most that many envs ended, two otherwise. */
typedef struct ch_host_out {
    float* obs;                /* host [E][R][86] (required) */
    float* reward;             /* host [E][K] (required) */
    uint8_t* terminated;       /* host [E][K] (required) */
    uint8_t* truncated;        /* host [E][K] (required) */
    uint8_t* reset_happened;   /* optional host [E] (needs io->reset_happened) */
    uint8_t* agent_active;     /* optional host [E][N] (needs io->agent_active) */
    int64_t ended_count;       /* out: envs that auto-reset in the step (needs io->reset_happened) */
    int64_t* ended_env;        /* optional host [E]: their indices, ascending */
    float* ended_obs;          /* optional host [E][R][86]: their terminal observations (needs io->terminal_obs) */
    double* ended_stats;       /* optional host [E][2]: their episode return and length (needs io->episode_stats) */
} ch_host_out;
int ch_outputs_to_host(ch_handle* h, const ch_step_io* io, ch_host_out* out, void* stream);

/* Full SoA state, for checkpoint/resume and parity state-injection.  Layout of the two host
 * buffers (counts from ch_state_size):
 *   doubles: drone[26][E][N] (px py pz qx qy qz qw vx vy vz wx wy wz pid_last_rpy[3]
 *            pid_int_pos[3] pid_int_rpy[3] qlag[4] = the cached link frame, link_lag), cattle[4][E][M] (x y vx vy),
 *            env[2][E] (prev_cent clock),
 *            phys[7][E][N] (last_clipped_action[4] = drag input, DYN body rates rpy_rates[3])
 *   int32:   env[10][E] (n, step_counter, step_counter_A, has_prev, level, tally, spawn_index,
 *            active_mask, episode, step_index = ch_step calls so far = the Philox action counter) */
int ch_state_size(const ch_handle* h, int64_t* n_doubles, int64_t* n_ints);
int ch_get_state(ch_handle* h, double* host_doubles, int32_t* host_ints, void* stream);
int ch_set_state(ch_handle* h, const double* host_doubles, const int32_t* host_ints, void* stream);

/* End-of-rollout metrics (host double[CH_METRIC_COUNT]) accumulated on device since the last call
 * with reset_after != 0: see CH_METRIC_* below.  Rank-local; bench.py all-reduces them over RCCL. */
enum {
    CH_METRIC_STEPS = 0, CH_METRIC_EPISODES, CH_METRIC_RETURN_SUM, CH_METRIC_LENGTH_SUM,
    CH_METRIC_TERMINATED, CH_METRIC_TRUNCATED, CH_METRIC_NAN_REWARDS, CH_METRIC_EFFECTIVENESS_SUM,
    CH_METRIC_COUNT
};
int ch_metrics(ch_handle* h, double* host_out, int32_t reset_after, void* stream);

/* The same sums written to a DEVICE buffer double[CH_METRIC_COUNT] on `stream`, without a host sync:
 * the input of the end-of-rollout RCCL all-reduce (bench.py).  Replaces the same reference code. */
int ch_metrics_device(ch_handle* h, double* dev_out, int32_t reset_after, void* stream);

/* Wait for `stream` and report the handle's sticky device error word: CH_ERR_DEVICE if a step kernel
 * recorded a failure (e.g. an LDS hand-off that timed out), CH_OK otherwise.  ch_metrics and
 * ch_get_state report it too.  (The reference's analogue: an exception out of env.step,
 * marl_wrapper.py:87-95.) */
int ch_sync(ch_handle* h, void* stream);

/* update_evaluation_metrics' per-drone episode distance (sb3_envs/BaseAviary.py:1415-1426, the
 * `episode_drone_distances` the evaluator logs; both components of the reference's 2-vector are equal):
 * host double[E][N], zero for drones beyond NUM_DRONES; reset with the episode.  Needs
 * cfg->eval_metrics (CH_ERR_UNSUPPORTED otherwise).  Synchronises `stream`. */
int ch_get_eval(ch_handle* h, double* host_out, void* stream);

/* Number of built-in spawn scenarios / cows, and a copy of the table (host double[S][C][2]):
 * config/cattle_positions.yaml, 100 scenarios x 16 cows (BaseAviary.py:88-94). */
int ch_builtin_spawn_table(double* out, int32_t* scenarios, int32_t* cows);

/* The table ch_create uses when cfg->spawn_table is NULL: the built-in 16 cows per scenario, extended
 * deterministically for cows > 16 (out: host double[100][max(cows,16)][2]; out may be NULL to query). */
int ch_spawn_table(int32_t cows, double* out, int32_t* scenarios, int32_t* out_cows);

/* ---- On-device policy ---------------------------------------------------------
 * A dense MLP evaluated on the matrix cores in f32 (exact f32 products, f32 sums), weights in
 * device memory in torch nn.Linear layout.  The SB3 actor of the reference's CTDE driver is
 * dims {1032, 128, 128, 48}, tanh hidden, output clipped to [-1, 1]; its critic {1032, 128, 128, 1};
 * the RLlib per-agent model {86, 256, 256, 8}. */
#define CH_ACT_NONE 0
#define CH_ACT_TANH 1
#define CH_ACT_RELU 2
typedef struct ch_mlp {
    int32_t n_layers;          /* 1..4 */
    int32_t dims[5];           /* dims[0] inputs; dims[i + 1] outputs of layer i (<= 256) */
    const float* weight[4];    /* device [dims[i+1]][dims[i]] row-major (nn.Linear.weight) */
    const float* bias[4];      /* device [dims[i+1]] or NULL */
    int32_t hidden_act;        /* CH_ACT_* applied after every layer but the last */
    int32_t clip;              /* non-zero: clip the output to [lo, hi] */
    float lo, hi;
    const float* packed;       /* NULL, or the same weights in the MFMA operand layout written by ch_mlp_pack
                                  (read instead of `weight`; re-pack after every weight update) */
    int32_t split_out[4];      /* block-diagonal layer i (i >= 1; 0 = dense): outputs [0, split_out) read only */
    int32_t split_in[4];       /* inputs [0, split_in), outputs [split_out, N) only [split_in, K) -- the weights
                                  outside the two blocks are zero and are not multiplied (e.g. SB3's actor and
                                  critic packed as one net).  Used when split_in % 128 == 0 and split_out % 32 == 0,
                                  else the layer runs dense (same result). */
} ch_mlp;

/* The operand layout of the forward kernel: per layer [16-column tile][32-wide K pair][half][lane][4], so that
 * each wave's weight load is one contiguous 1 KB block.  ch_mlp_packed_size: floats of device memory the
 * layout of `net` takes; ch_mlp_pack: writes it (from net->weight) into dst on `stream`.  No reference
 * counterpart: the reference's torch forward reads nn.Linear weights (CTDECattleHerder.py:203). */
int64_t ch_mlp_packed_size(const ch_mlp* net);
int ch_mlp_pack(const ch_mlp* net, float* dst, void* stream);

/* Replaces: stable_baselines3 ActorCriticPolicy.predict(obs, deterministic=True) for a Box action
 * space (mlp_extractor.policy_net -> action_net -> np.clip to the space, CTDECattleHerder.py:203,
 * 106-127) and predict_values (value_net), and the RLlib model forward of DTDECattleHerder.py.
 * y[rows][dims[L]] = MLP(x[rows][dims[0]]); x and y are device buffers. */
int ch_mlp_forward(const ch_mlp* net, const float* x, int64_t rows, float* y, void* stream);

/* ch_mlp_forward for the rows whose byte in row_mask (device uint8 [rows]) is non-zero; the other rows of y
 * are left untouched, and 16-row tiles with no selected row cost next to nothing.  Replaces the SB3 rollout's
 * predict_values(terminal_observation) for the envs that just reset (OnPolicyAlgorithm.collect_rollouts'
 * TimeLimit.truncated bootstrap, CTDECattleHerder.py:107-150), evaluated only where it is used. */
int ch_mlp_forward_masked(const ch_mlp* net, const float* x, int64_t rows, const uint8_t* row_mask, float* y,
                          void* stream);

/* ch_mlp_forward on a handle's observation buffer: one row per env for CTDE (x = obs [E][R][86]
 * flattened, dims[0] = R*86) or per agent for MARL (x = obs [E][N][86], dims[0] = 86, E*N rows).
 * Input features past an env's NUM_DRONES rows (CTDE) or of agents past NUM_DRONES (MARL) are zero
 * in the observation and are not multiplied. */
int ch_policy_forward(ch_handle* h, const ch_mlp* net, const float* obs, float* y, void* stream);

/* ---- On-device PPO rollout buffer ---------------------------------------------
 * Replaces: stable_baselines3 OnPolicyAlgorithm.collect_rollouts' RolloutBuffer and
 * RolloutBuffer.compute_returns_and_advantage for the CTDE driver's PPO (CTDECattleHerder.py:107-150:
 * n_steps, gamma 0.99, gae_lambda 0.95, DiagGaussian actions with log_std).  CTDE handles only (one row
 * per env).  All buffers are caller-owned device float32 arrays, rows = n_envs:
 *   obs [T][rows][12*86], actions [T][rows][act_dim] (unclipped samples), rewards, episode_starts, values,
 *   log_probs, advantages, returns [T][rows]; last_episode_starts [rows] (SB3's _last_episode_starts,
 *   1 after a reset). */
typedef struct ch_rollout {
    int32_t n_steps;           /* T */
    int32_t act_dim;           /* policy action width (the reference's 12 x 4 = 48) */
    float* obs;
    float* actions;
    float* rewards;
    float* episode_starts;
    float* values;
    float* log_probs;
    float* advantages;
    float* returns;
    float* last_episode_starts;
} ch_rollout;

/* Step t, before env.step: copy obs [rows][12*86] into the buffer, sample actions = mean + exp(log_std) eps
 * (eps ~ N(0,1) from Philox keyed by seed, counter (t, action, env)), store them with their summed Normal
 * log-probability, value [rows] and the episode starts; write the actions clipped to [-1, 1] into
 * env_actions [rows][num_drones][4] (the first num_drones*4 of act_dim, as the env reads a (12, 4) action). */
int ch_rollout_store(ch_handle* h, const ch_rollout* rb, int32_t t, const float* obs, const float* mean,
                     const float* value, const float* log_std, uint64_t seed, float* env_actions, void* stream);

/* Step t, after env.step: rewards[t] = reward, plus gamma * terminal_value where the env was truncated and
 * not terminated (SB3's TimeLimit.truncated bootstrap; terminal_value may be NULL); the next step's
 * episode starts = terminated | truncated. */
int ch_rollout_post(ch_handle* h, const ch_rollout* rb, int32_t t, const float* reward, const uint8_t* terminated,
                    const uint8_t* truncated, const float* terminal_value, float gamma, void* stream);

/* compute_returns_and_advantage: GAE(gamma, gae_lambda) backwards over the T steps in float32 with
 * last_value [rows] = V(obs after the last step). */
int ch_rollout_gae(ch_handle* h, const ch_rollout* rb, const float* last_value, float gamma, float gae_lambda,
                   void* stream);

/* The whole collection in one call (the native loop behind cattleherd.rollout.DeviceRolloutBuffer.collect):
 * for t < n_steps, on `stream`: actor and critic forwards on step->obs (ch_policy_forward), ch_rollout_store,
 * ch_step with auto-reset and terminal observations, the critic on the terminal observations of the envs that
 * reset (ch_mlp_forward_masked; skipped with bootstrap_truncated = 0), ch_rollout_post; then the critic on the
 * last observations and ch_rollout_gae.
 * critic == NULL: `actor` is a fused actor-critic whose output is act_dim + 1 wide (the action mean, then the
 * value; e.g. SB3's two MLPs packed as one: layer 1 stacked, layers 2-3 block-diagonal, which leaves every output
 * bit-identical to the separate nets): one forward per step reads the observation once.  `mean` and
 * `terminal_value` are then [rows][act_dim + 1] (both heads); `value` is not used.
 * Device scratch (caller-owned): */
typedef struct ch_rollout_io {
    const ch_step_io* step;    /* the env's step buffers; obs, reward, terminated, truncated, terminal_obs and
                                  reset_happened are required (actions are env_actions below) */
    float* mean;               /* [rows][act_dim] ([rows][act_dim + 1] with a fused actor-critic) */
    float* value;              /* [rows] */
    float* terminal_value;     /* [rows] ([rows][act_dim + 1] with a fused actor-critic) */
    float* env_actions;        /* [rows][num_drones][4] */
} ch_rollout_io;
int ch_rollout_collect(ch_handle* h, const ch_rollout* rb, const ch_rollout_io* io, const ch_mlp* actor,
                       const ch_mlp* critic, const float* log_std, uint64_t seed, float gamma, float gae_lambda,
                       int32_t bootstrap_truncated, void* stream);

/* ---- Population collection: P members' policies collect on one env batch ------------------------------------------
 * Replaces: P calls of ch_rollout_collect, one per member of a population (seeds, hyper-parameter variants) on P handles
 * of E envs; the reference has no counterpart for running them together.  The envs of a batch are independent and
 * ch_config.env_id_offset makes env e of a shard global env offset + e, so the members share one handle of P * E envs,
 * member p owning envs [pE, (p + 1)E): the env step is one launch for everybody, and each of the policy launches carries
 * every member, the member being a grid dimension.
 * CONTRACT: after ch_rollout_collect_pop member p's buffers are bit for bit what ch_rollout_collect writes for a handle
 * of E envs created with the same config and env_id_offset = this handle's + pE, run from the same env state with
 * member p's actor, critic, log_std, seed, gamma, gae_lambda and the same bootstrap_truncated; the env state of the
 * slice is that handle's too.  The Philox counter of a sample is (t, action, member-local row) under the member's seed;
 * last_episode_starts is per member.  Nothing is shared between members but the env step.
 * `io` is the whole handle's scratch as for ch_rollout_collect (mean [P*E][act_dim], value, terminal_value [P*E],
 * env_actions [P*E][num_drones][4], the step buffers); member p uses rows [pE, (p + 1)E) of each.  The step writes the
 * handle's own observation buffer and every step's observation is copied into the members' buffers (the members'
 * buffers are separate allocations).  The deferred truncation bootstrap has a queue slice and a counter per member and
 * is flushed with the period of a solo handle of E envs.  ch__set_rollout_path's bits are not read. */
typedef struct ch_rollout_member {
    ch_rollout   rb;           /* this member's own buffers, rows = n_envs / n_members */
    const ch_mlp *actor, *critic;   /* separate nets (no fused actor-critic) */
    const float* log_std;      /* [act_dim] */
    uint64_t     seed;
    float        gamma, gae_lambda;
} ch_rollout_member;
typedef struct ch_rollout_pop ch_rollout_pop;   /* opaque: the kernels' argument tables */

/* Replaces: nothing in the reference (see above).  The object that holds the argument tables of up to max_members
 * members on `device`: one block of entries per launch kind (step forward, flush, last value), in two slots of pinned
 * host staging and device memory, so that a call may fill its staging while the copy an earlier, still queued call
 * issued reads the other slot's; a slot is reused only after the event behind its copy.  One object serves one stream
 * at a time.  CH_ERR_INVALID for max_members outside 1..65535 or a NULL out, CH_ERR_DEVICE / CH_ERR_NOMEM when the
 * allocation fails. */
int ch_rollout_pop_create(int32_t max_members, int32_t device, ch_rollout_pop** out);
/* Waits for the copies it issued, then frees the tables.  The caller has let the launches that read them finish. */
int ch_rollout_pop_destroy(ch_rollout_pop* pop);

/* The collection (see above), stream-ordered on `stream`, no host synchronisation beyond the wait for a staging slot two
 * calls old.  The tables are uploaded once per call; the step index is a kernel argument.
 * Checked on the host before anything is launched (CH_ERR_INVALID unless noted; ch_last_error says which): NULL
 * arguments; 1 <= n_members <= the object's max_members; the handle's envs divide evenly among the members; a MARL
 * handle (CH_ERR_UNSUPPORTED); a NULL critic; members that differ from member 0 in architecture (dims, activation, clip,
 * splits), n_steps or act_dim; nets the forward kernel does not take as one two-segment launch (CH_ERR_UNSUPPORTED:
 * there is no fallback path here); obs buffers that are not 16-byte aligned; two writable buffer arrays that are the
 * same pointer. */
int ch_rollout_collect_pop(ch_handle* h, ch_rollout_pop* pop, const ch_rollout_member* members, int32_t n_members,
                           const ch_rollout_io* io, int32_t bootstrap_truncated, void* stream);

/* ---- Device-side SB3 training log: the episode ring (rollout/ep_rew_mean, rollout/ep_len_mean) ---------------
 * Replaces: OnPolicyAlgorithm._update_info_buffer, which appends Monitor's info["episode"] of every env that ended an
 * episode to ep_info_buffer = deque(maxlen=stats_window_size), step by step and in env order inside collect_rollouts;
 * the logger's rollout/ep_rew_mean and rollout/ep_len_mean are the means over that deque.  Here the deque is a ring of
 * `window` slots in device memory, appended to by one small kernel after each step, with no host synchronisation.
 * CTDE handles only (CH_ERR_UNSUPPORTED for a MARL handle).  All arrays are caller-owned device memory.
 * (SB3 is not installed here: restated from its source, "parity unpinned".) */
typedef struct ch_ep_ring {
    int32_t  window;      /* W >= 1: SB3's stats_window_size (100) */
    int32_t  _pad;
    double*  ep_return;   /* device [W]: io->episode_stats[e][0], as it is (no rounding on the device) */
    int32_t* ep_length;   /* device [W]: io->episode_stats[e][1] */
    int32_t* ep_env;      /* device [W]: the env it came from */
    int64_t* total;       /* device [1]: episodes appended since begin; episode k lives in slot k % W */
} ch_ep_ring;

/* total = 0 (the slots are not cleared: the ring holds episodes max(0, total - W) .. total - 1). */
int ch_ep_ring_begin(ch_handle* h, const ch_ep_ring* ring, void* stream);

/* After a ch_step with CH_STEP_AUTORESET on the same stream (io->reset_happened and io->episode_stats are required,
 * CH_ERR_INVALID otherwise; nothing else of the io and nothing of the handle but n_envs is read): the C envs with
 * reset_happened[e] != 0 are appended in ascending env order, the order _update_info_buffer walks `infos` -- the
 * env of rank r among them is episode total + r and goes to slot (total + r) % W; when C > W only the last W of the
 * step (r >= C - W) are written, so that every slot has one writer; then total += C.  One workgroup: a counting
 * pass and a ranking pass (wave ballots and a scan of the wave totals) over the envs in chunks of 1024; plain stores,
 * no atomics.  n_envs up to 262144 and beyond. */
int ch_ep_ring_record(ch_handle* h, const ch_ep_ring* ring, const ch_step_io* io, void* stream);

/* ch_rollout_collect with the episode ring: with ring != NULL, ch_ep_ring_record runs once per step, right after the
 * launch that holds step t's env step (ch_step, or the step fused with the next step's actor forward) and before
 * anything that can overwrite reset_happened or episode_stats, on every path of the collection; io->step->episode_stats
 * is then required (CH_ERR_INVALID).  ring == NULL is ch_rollout_collect exactly.  The rollout buffer's contents do
 * not depend on the ring.  The call does not begin the ring: one ring spans the collections of a training run. */
int ch_rollout_collect_log(ch_handle* h, const ch_rollout* rb, const ch_rollout_io* io, const ch_mlp* actor,
                           const ch_mlp* critic, const float* log_std, uint64_t seed, float gamma, float gae_lambda,
                           int32_t bootstrap_truncated, const ch_ep_ring* ring, void* stream);

/* ---- A population's training log: per-member episode rings and a fitness table on the device -----------------------
 * Replaces: P ep_info_buffer deques, one per member of a population that collects with ch_rollout_collect_pop; the
 * reference has no counterpart for running the members together.  Member p of n_members owns envs [pE, (p + 1)E) of the
 * handle, E = n_envs / n_members, and row p of every array.  CTDE handles only (CH_ERR_UNSUPPORTED for a MARL handle).
 * All arrays are caller-owned device memory; one window for every member. */
typedef struct ch_ep_ring_pop {
    int32_t  window;      /* W >= 1, the same for every member */
    int32_t  n_members;   /* P >= 1; the handle's n_envs must be a multiple of it, E = n_envs / P */
    double*  ep_return;   /* device [P][W] */
    int32_t* ep_length;   /* device [P][W] */
    int32_t* ep_env;      /* device [P][W]: the MEMBER-LOCAL env index, e - pE */
    int64_t* total;       /* device [P]: member p's episodes appended since begin; its episode k lives in slot k % W */
} ch_ep_ring_pop;

/* total[p] = 0 for every member (the slots are not cleared). */
int ch_ep_ring_pop_begin(ch_handle* h, const ch_ep_ring_pop* ring, void* stream);

/* After a ch_step with CH_STEP_AUTORESET on the same stream.  CONTRACT: row p of the four arrays is afterwards bit for
 * bit what ch_ep_ring_record writes to a solo ring of window W on a handle of E envs whose reset_happened and
 * episode_stats are rows [pE, (p + 1)E) of this io's: member p's C_p ended envs in ascending env order, rank r to slot
 * (total[p] + r) % W, only ranks r >= C_p - W written, then total[p] += C_p; a member with C_p == 0 writes nothing, not
 * even total[p].  One launch whatever P is: workgroup p is the solo recorder on the member's slice (the same counting
 * and ranking passes in chunks of 1024 envs; plain stores, no atomics, nothing shared between workgroups).
 * CH_ERR_INVALID (ch_last_error says which): a NULL ring, io or handle, window < 1, n_members < 1, a missing ring array,
 * n_envs % n_members != 0, an io without reset_happened or episode_stats. */
int ch_ep_ring_pop_record(ch_handle* h, const ch_ep_ring_pop* ring, const ch_step_io* io, void* stream);

/* ch_rollout_collect_pop with the members' episode rings: with ring != NULL, ch_ep_ring_pop_record's launch runs once
 * per step, right after the step's ch_step and before anything that can overwrite reset_happened or episode_stats
 * (where ch_rollout_collect_log records); io->step->episode_stats is then required and ring->n_members must equal
 * n_members (CH_ERR_INVALID; checked with everything else before the first launch).  ring == NULL is
 * ch_rollout_collect_pop exactly.  The members' buffers and the env state do not depend on the ring.  The call does not
 * begin the ring: one ring spans the collections of a training run. */
int ch_rollout_collect_pop_log(ch_handle* h, ch_rollout_pop* pop, const ch_rollout_member* members, int32_t n_members,
                               const ch_rollout_io* io, int32_t bootstrap_truncated, const ch_ep_ring_pop* ring,
                               void* stream);

/* The fitness table a population is compared on: out_dev[p] = {count = min(total[p], W), mean return, mean length,
 * total[p] as a double}, CH_EP_RING_POP_SUMMARY doubles per member.  Handle-free (errors through ch_last_error(NULL));
 * one launch, grid (P), stream-ordered, no host synchronisation.  The means are float64 over the ring's content in
 * chronological order, oldest first -- position i = 0 .. count - 1 is episode total - count + i, slot
 * (total - count + i) % W -- in this FIXED ORDER: one 64-thread workgroup per member; thread t starts from 0.0 and adds
 * positions t, t + 64, t + 128, ... in that order; the 64 thread sums are added by a halving tree (for w = 32, 16, ..,
 * 1: s[t] += s[t + w] for t < w); the mean is s[0] / count.  count == 0 gives NaN means.
 * DIFFERENCE: the returns are not rounded to 6 decimals here; Monitor's rounding stays on the host path (train_log.py
 * summary_of), so a mean return can differ from rollout/ep_rew_mean in the 7th decimal.
 * CH_ERR_INVALID: a NULL ring or out_dev, window < 1, n_members < 1, a missing ring array. */
#define CH_EP_RING_POP_SUMMARY 4
int ch_ep_ring_pop_summary(const ch_ep_ring_pop* ring, double* out_dev, void* stream);

/* ---- Device-side VecNormalize: running observation / return statistics for the CTDE PPO path -----------------
 * Replaces: stable_baselines3 VecNormalize(venv, training, norm_obs, norm_reward, clip_obs, clip_reward, gamma,
 * epsilon) around the reference's VecEnv, and its two RunningMeanStd (obs_rms over the observation features, ret_rms
 * over the envs' discounted returns): update(x[n]) merges the batch mean, population variance and n into the running
 * (mean, var, count) by update_from_moments; the initial state is mean 0, var 1, count 1e-4.  All statistics are
 * float64.  (SB3 is not installed here: restated from its source, "parity unpinned".)  Not restated: norm_obs_keys /
 * dict observations, SB3's pickled file, MARL handles (RLlib normalises with connectors).
 * The struct lives in host memory and is read at each call; every array is caller-owned DEVICE memory.  The five
 * statistic arrays are meant to be views of one block (mean, var, count, ret_stats, ret), so that a checkpoint is one
 * copy each way.  All work is enqueued on `stream`, with no host synchronisation; one stream per normaliser.
 * Determinism: no floating-point atomics; every sum has a fixed order, so the same state and input give the same bits.
 * Failures of the handle-free entry points are reported by ch_last_error(NULL). */
typedef struct ch_norm {
    int32_t dim;               /* observation features (a CTDE handle's obs_rows * 86) */
    int32_t training;          /* non-zero: the statistics move (VecNormalize.training) */
    int32_t norm_obs;          /* non-zero: observations are normalised; 0: ch_norm_obs_apply copies */
    int32_t norm_reward;       /* non-zero: rewards are normalised; 0: ch_norm_reward copies them (ret_rms still moves) */
    double clip_obs;           /* >= 0 (10) */
    double clip_reward;        /* >= 0 (10) */
    double epsilon;            /* >= 0 (1e-8) */
    double gamma;              /* the return's discount (0.99) */
    int64_t n_envs;            /* E: rows of ret */
    double* mean;              /* device [dim]  obs_rms.mean */
    double* var;               /* device [dim]  obs_rms.var */
    double* count;             /* device [1]    obs_rms.count */
    double* ret_stats;         /* device [3]    ret_rms.mean, .var, .count */
    double* ret;               /* device [E]    VecNormalize.returns */
    double* scratch;           /* device [scratch_doubles]: the reductions' partials (contents not kept) */
    int64_t scratch_doubles;   /* >= ch_norm_scratch_size(rows, dim) of every matrix passed, and of (E, dim) */
    float* obs_n;              /* ch_rollout_collect_norm only (NULL otherwise): device [E][dim], the normalised observation */
    float* terminal_obs_n;     /*   device [E][dim]: the normalised terminal observations of the envs that reset */
    float* reward_n;           /*   device [E]: the normalised reward */
} ch_norm;

/* Doubles of scratch ch_norm_obs_update takes for a [rows][dim] matrix (and ch_norm_reward for `rows` envs); -1 for
 * rows or dim outside [1, 2^24].  Host only. */
int64_t ch_norm_scratch_size(int64_t rows, int32_t dim);

/* Replaces: RunningMeanStd.__init__ for both statistics and VecNormalize's returns = zeros: mean 0, var 1, count 1e-4,
 * ret 0, on `stream`. */
int ch_norm_begin(const ch_norm* norm, void* stream);

/* Replaces: obs_rms.update(x) for a device float32 [rows][dim] matrix (no handle: any matrix will do).  A no-op
 * unless training and norm_obs.  Two launches: the batch moments per (column tile, row chunk) workgroup -- float4 loads
 * along dim where dim % 4 == 0 and x is 16-byte aligned, a scalar path otherwise; two-pass variance over 64 rows held
 * in registers, Chan's merge above, all of x - x[0][column] -- and the merge of the chunks in index order with the
 * running update, the only writer of mean / var / count (a launch of its own: no workgroup reads the running statistics
 * while another writes them). */
int ch_norm_obs_update(const ch_norm* norm, const float* x, int64_t rows, void* stream);

/* Replaces: VecNormalize.normalize_obs: y = float32(clip((float64(x) - mean) / sqrt(var + epsilon), -clip_obs,
 * clip_obs)), IEEE float64 division and square root, no contraction: numpy's bits for the same statistics.  y may be
 * x.  row_mask (optional device uint8 [rows]): only the rows with a non-zero byte are written (the terminal
 * observations of the envs that reset, as ch_mlp_forward_masked).  With norm_obs off: y = x. */
int ch_norm_obs_apply(const ch_norm* norm, const float* x, int64_t rows, const uint8_t* row_mask, float* y, void* stream);

/* Replaces, for one env step: VecNormalize.step_wait's reward half -- when training, ret = ret * gamma + reward and
 * ret_rms.update(ret) (with norm_reward off too); reward_out = float32(clip(float64(reward) / sqrt(ret_rms.var +
 * epsilon), -clip_reward, clip_reward)) with the updated variance (norm_reward off: reward_out = reward); then
 * ret = 0 where terminated | truncated.  reward / terminated / truncated: device [n_envs], n_envs = norm->n_envs.
 * The raw reward is read only (reward_out must be another buffer): episode_stats and the episode ring keep reporting
 * unnormalised returns, as SB3's Monitor sits under VecNormalize.  One launch of one workgroup up to 4096 envs; beyond
 * that three (chunk moments, merge and update, elementwise). */
int ch_norm_reward(const ch_norm* norm, const float* reward, const uint8_t* terminated, const uint8_t* truncated,
                   int64_t n_envs, float* reward_out, void* stream);

/* ch_rollout_collect_log under a normaliser (the native loop behind DeviceRolloutBuffer.collect(normalizer=...)):
 * first obs_n = normalised step->obs under the statistics as they stand; then for t < n_steps the actor and critic
 * forwards on obs_n, ch_rollout_store of obs_n (the buffer keeps normalised observations, as SB3's), ch_step with
 * auto-reset and terminal observations, the optional ring record (raw returns), ch_norm_obs_update and
 * ch_norm_obs_apply of the new observation into obs_n, the masked apply of the terminal observations (with the
 * statistics already updated; they do not enter the update) and the masked critic on them, ch_norm_reward, and
 * ch_rollout_post with the normalised reward; then the critic on obs_n and ch_rollout_gae.
 * The forwards are the DENSE ch_mlp_forward, not ch_policy_forward: that one skips the input features past an env's
 * NUM_DRONES because they are zero in the raw observation; normalised they are (0 - mean) / sqrt(var + epsilon), which
 * is not zero wherever envs differ in NUM_DRONES.  A policy trained here must be evaluated the same way.
 * The step fused with the next actor forward and the deferred bootstrap are not used.  norm == NULL is refused
 * (CH_ERR_INVALID), as are a fused actor-critic (critic == NULL) and a MARL handle (CH_ERR_UNSUPPORTED), and
 * norm->dim != obs_rows * 86 or norm->n_envs != n_envs (CH_ERR_INVALID).  obs_n, terminal_obs_n, reward_n required. */
int ch_rollout_collect_norm(ch_handle* h, const ch_rollout* rb, const ch_rollout_io* io, const ch_mlp* actor,
                            const ch_mlp* critic, const float* log_std, uint64_t seed, float gamma, float gae_lambda,
                            int32_t bootstrap_truncated, const ch_ep_ring* ring, const ch_norm* norm, void* stream);

/* ---- On-device rollout collection for the DTDE (RLlib) driver ----------------------------------------------
 * Replaces: RLlib PPO's sampling of RLlibMultiAgentWrapper envs with one shared policy over every agent
 * (DTDECattleHerder.py:62-97: policies = {"shared_policy"}, gamma 0.99, train_batch_size 4096; the wrapper's
 * agent drop-out and "__all__", marl_wrapper.py:77-119) and its GAE postprocessing.  MARL handles only.  Rows are
 * agents: rows = n_envs * num_drones, row e * num_drones + i = agent_i of env e.  Per step t < n_steps:
 *   the policy (output [rows][2 * act_dim]: RLlib's DiagGaussian inputs, the mean then log_std) and the value net
 *   on the agents' observations (obs[t] = [rows][86]); for every agent live at the step's start (the wrapper's
 *   self.agents: agent i < NUM_DRONES, not dropped out) a Gaussian sample a = mean + exp(log_std) eps (Philox keyed
 *   by seed, counter (t, action, row), Box-Muller), stored unclipped with its summed Normal log-probability, the
 *   value and agent_mask = 1; the env gets the samples clipped to [-1, 1] (RLlib's unsquash for Box(-1, 1)) and 0
 *   for the other agents (ignored by the env); ch_step with auto-reset; the step's reward / terminated / truncated
 *   per agent (0 where agent_mask is 0).
 * Then last_values = V(obs after the last step) and GAE(gamma, gae_lambda) per agent backwards in float32: an
 * agent's trajectory ends where it terminates (bootstrap 0; the env resets only once every agent has terminated, so
 * a live agent that did not terminate is live at the next step of the same episode); rows with agent_mask 0 get
 * advantage and return 0; truncation does not end a trajectory (the wrapper keeps truncated agents acting).
 * Divergence note: RLlib's per-agent episodes treat terminated OR truncated as done and bootstrap V(obs) at a
 * truncation; this restatement follows the wrapper's "__all__" rule instead and bootstraps straight through the
 * time limit (marl_wrapper.py:104-117).  Parity unpinned either way: RLlib is not installed here.
 * RLlib is not installed here: these semantics are restated from its PPO defaults ("parity unpinned" to its
 * source).  All arrays are caller-owned device memory. */
typedef struct ch_marl_rollout {
    int32_t n_steps;           /* T */
    int32_t act_dim;           /* 4 (the VEL action of one agent) */
    float* obs;                /* [T][rows][86] */
    float* actions;            /* [T][rows][act_dim] unclipped samples (0 where not live) */
    float* log_probs;          /* [T][rows] */
    float* values;             /* [T][rows] */
    float* rewards;            /* [T][rows] */
    uint8_t* agent_mask;       /* [T][rows]: the agent was live at the start of step t */
    uint8_t* terminated;       /* [T][rows] */
    uint8_t* truncated;        /* [T][rows] */
    float* advantages;         /* [T][rows] */
    float* returns;            /* [T][rows] (advantages + values) */
    float* last_values;        /* [rows] */
} ch_marl_rollout;
typedef struct ch_marl_rollout_io {
    const ch_step_io* step;    /* the env's step buffers: obs, reward, terminated, truncated (actions are env_actions) */
    float* policy_out;         /* scratch [rows][2 * act_dim] */
    float* value_out;          /* scratch [rows] */
    float* env_actions;        /* scratch [n_envs][num_drones][4] */
} ch_marl_rollout_io;
int ch_marl_rollout_collect(ch_handle* h, const ch_marl_rollout* rb, const ch_marl_rollout_io* io, const ch_mlp* policy,
                            const ch_mlp* value, uint64_t seed, float gamma, float gae_lambda, void* stream);

/* ---- Device-side RLlib training log: the episode ring of a MARL handle (env_runners/...) ----------------------
 * Replaces: what RLlib's env runners report of RLlibMultiAgentWrapper envs while the DTDE driver trains
 * (DTDECattleHerder.py:62-97) -- env_runners/episode_return_mean / _min / _max, episode_len_mean,
 * agent_episode_returns_mean/<agent>, module_episode_returns_mean/shared_policy over the last
 * metrics_num_episodes_for_smoothing (100) episodes, and num_env_steps_sampled, num_agent_steps_sampled/<agent>.
 * Here the window is a ring of `window` slots in device memory and the open episodes' sums sit beside it, advanced by
 * one small kernel after each step, with no host synchronisation.  MARL handles with marl_wrapper = 1 only
 * (CH_ERR_UNSUPPORTED otherwise).  All arrays are caller-owned device memory; N = the handle's num_drones.
 * (RLlib is not installed here: restated from its source, "parity unpinned".)
 * The episode rule is ch_marl_eval_record's (marl_wrapper.py:77-119): an agent adds (double)reward and one step only
 * where it was live at the start of the step (the reward of an agent that is not live is never read); an env's
 * episode ends where reset_happened[e] is set; a truncation ends nothing. */
typedef struct ch_marl_ep_ring {
    int32_t  window;        /* W >= 1: RLlib's metrics_num_episodes_for_smoothing (100) */
    int32_t  _pad;
    double*  ep_return;     /* device [W]: the sum over the agents, in agent order, of agent_return */
    double*  agent_return;  /* device [W][N] */
    int32_t* ep_length;     /* device [W]: env steps of the episode */
    int32_t* agent_length;  /* device [W][N]: the steps the agent was live in */
    int32_t* ep_env;        /* device [W]: the env it came from */
    int64_t* total;         /* device [1]: episodes appended since begin; episode k lives in slot k % W */
    double*  acc_return;    /* device [E][N]: the open episodes' running state */
    int32_t* acc_length;    /* device [E][N] */
    int32_t* acc_steps;     /* device [E] */
    int64_t* env_steps;     /* device [1]: env steps recorded since begin (E per recorded step) */
    int64_t* agent_steps;   /* device [N]: live agent-steps since begin, per agent index */
} ch_marl_ep_ring;

/* total, the counters and the accumulators = 0 (the slots are not cleared: the ring holds episodes
 * max(0, total - W) .. total - 1).  An episode that is open at begin counts from zero. */
int ch_marl_ep_ring_begin(ch_handle* h, const ch_marl_ep_ring* ring, void* stream);

/* After a ch_step with CH_STEP_AUTORESET on the same stream.  live: device uint8 [E][N], the agents live at the start
 * of that step (ch_marl_eval_mark's, or a rollout buffer's agent_mask[t]).  io->reward and io->reset_happened are
 * required (CH_ERR_INVALID otherwise; nothing else of the io is read).  Every env's live agents add their rewards to
 * the accumulators; then the C envs with reset_happened[e] != 0 are appended in ascending env order -- rank r among
 * them is episode total + r and goes to slot (total + r) % W; when C > W only the last W of the step (r >= C - W)
 * are written, so that every slot has one writer -- their accumulators go back to 0, and total += C.  Two launches:
 * one thread per env accumulates (the live agent-steps, a pure count, with one integer atomic per wave and agent, as
 * ch_marl_eval_record counts `remaining`); then one workgroup counts the ended envs and (C > 0) ranks them (wave
 * ballots and a scan of the wave totals) over the envs in chunks of 1024.  Plain stores, no atomic on a float, every
 * float64 sum by one thread in agent order: the same inputs give the same bits. */
int ch_marl_ep_ring_record(ch_handle* h, const ch_marl_ep_ring* ring, const uint8_t* live, const ch_step_io* io,
                           void* stream);

/* ch_marl_rollout_collect with the episode ring: with ring != NULL, ch_marl_ep_ring_record runs once per step, right
 * after step t's ch_step, with live = rb->agent_mask[t] (written by step t's store kernel, before the step) and the
 * step's own reward / reset_happened, which nothing overwrites before step t + 1's ch_step: the forwards write the
 * scratch outputs, and the store kernel of step t + 1, which posts step t, writes the buffer only.
 * io->step->reset_happened is then required (CH_ERR_INVALID).  ring == NULL is ch_marl_rollout_collect exactly.  The
 * rollout buffer's contents and the env state do not depend on the ring.  The call does not begin the ring: one ring
 * spans the collections of a training run, and episodes span collection boundaries.  No host synchronisation. */
int ch_marl_rollout_collect_log(ch_handle* h, const ch_marl_rollout* rb, const ch_marl_rollout_io* io,
                                const ch_mlp* policy, const ch_mlp* value, uint64_t seed, float gamma, float gae_lambda,
                                const ch_marl_ep_ring* ring, void* stream);

/* ---- On-device policy evaluation ---------------------------------------------------------
 * Replaces: stable_baselines3 evaluate_policy(model, env, n_eval_episodes, deterministic=True), as the CTDE driver
 * runs it after training and EvalCallback runs it during training (CTDECattleHerder.py:139-148, 185): every env
 * steps with the deterministic action until it has contributed its share of the n episodes; each counted episode's
 * return and length (Monitor's info["episode"]) go into a list whose mean +- std is the model-selection signal.
 * Here the list is a device table with `capacity` slots per env, filled by a recorder kernel after each step, so
 * the evaluation runs without the host reading any per-step output.  CTDE handles only.  All arrays are
 * caller-owned device memory.  (SB3 is not installed here: restated from its source, "parity unpinned".) */
typedef struct ch_eval_table {
    int32_t  capacity;      /* C: episode slots per env */
    int32_t  _pad;
    int32_t* quota;         /* device [E]: episodes env e still has to contribute in total (SB3's episode_count_targets) */
    int32_t* count;         /* device [E]: episodes recorded for env e (never exceeds quota) */
    double*  ep_return;     /* device [E][C]: io->episode_stats[e][0] of the recorded episode */
    int32_t* ep_length;     /* device [E][C]: io->episode_stats[e][1] */
    uint8_t* ep_flags;      /* device [E][C]: bit 0 terminated, bit 1 truncated (the step's outputs for env e) */
    int32_t* ep_end_step;   /* device [E][C]: the evaluation step index at which it ended */
    int64_t* remaining;     /* device [1]: sum over e of quota[e] - count[e] */
} ch_eval_table;

/* Start an evaluation of n_eval_episodes episodes: quota[e] = (n_eval_episodes + e) / E (evaluate_policy's
 * episode_count_targets: the integer division leaves the later envs with one episode more), count = 0,
 * remaining = n_eval_episodes.  The slots are not cleared: slot [e][k] is valid for k < count[e].
 * CH_ERR_INVALID if n_eval_episodes < 1 or ceil(n_eval_episodes / E) > capacity; CH_ERR_UNSUPPORTED for a MARL
 * handle. */
int ch_eval_begin(ch_handle* h, const ch_eval_table* table, int32_t n_eval_episodes, void* stream);

/* After a ch_step with CH_STEP_AUTORESET on the same stream (io->reset_happened and io->episode_stats are required,
 * CH_ERR_INVALID otherwise): every env that ended an episode in that step (reset_happened[e] != 0) and is below its
 * quota writes slot count[e] (return, length, the step's terminated / truncated, step_index), counts it and lowers
 * `remaining`.  Episodes of an env at its quota are ignored, as evaluate_policy ignores them: the env keeps stepping.
 * 0 <= step_index < 2^31. */
int ch_eval_record(ch_handle* h, const ch_eval_table* table, const ch_step_io* io, int64_t step_index, void* stream);

/* The evaluation loop in one call.  Per step t = 0, 1, ... on `stream`: ch_policy_forward(actor) on io->step->obs
 * into io->mean; env_actions[e][i][c] = clamp(mean[e][4 i + c], -1, 1) for i < num_drones (predict's clip to the
 * action Box and the env's read of the first num_drones rows; applied whether or not actor->clip is set, so a
 * training actor evaluates unchanged; the actor's output must be at least 4 * num_drones wide); ch_step with
 * auto-reset; ch_eval_record with step index first_step_index + t (run inside the next step's action kernel, while
 * the step's outputs are still in place, and as a launch of its own before each read of `remaining`: three launches
 * per step between reads).
 * Every check_every steps (>= 1) and at max_steps (>= 1) `remaining` is copied to the host and the stream is
 * synchronised -- nowhere else -- and the loop stops when it is 0.  Reaching max_steps with episodes outstanding is
 * not an error: the call returns CH_OK with *remaining > 0.  *steps_run: the steps taken.  The steps after the last
 * quota filled (at most check_every - 1) leave the table untouched -- recording is gated by the quotas -- and only
 * advance the env state.  The call neither resets the envs nor begins the table (ch_reset, ch_eval_begin): a second
 * call with first_step_index = the steps run so far continues an evaluation.
 * A HIP error ends the loop at once (CH_ERR_DEVICE); the sticky device error word is read at every check and
 * reported as ch_sync reports it. */
typedef struct ch_eval_io {
    const ch_step_io* step;   /* env step buffers: obs, reward, terminated, truncated, reset_happened, episode_stats */
    float* mean;              /* scratch [E][actor->dims[last]] */
    float* env_actions;       /* scratch [E][num_drones][4] */
} ch_eval_io;
int ch_evaluate_policy(ch_handle* h, const ch_mlp* actor, const ch_eval_table* table, const ch_eval_io* io,
                       int64_t max_steps, int32_t check_every, int64_t first_step_index,
                       int64_t* steps_run, int64_t* remaining, void* stream);

/* ---- On-device policy evaluation for the DTDE (RLlib) driver -------------------------------------------------
 * Replaces: the reference's DTDEModelPlayback.py workflow and RLlib's evaluation_* metrics (episode_return_mean,
 * episode_len_mean, per-agent returns) for the shared policy over RLlibMultiAgentWrapper envs: every env steps with
 * the deterministic action (explore=False on a DiagGaussian: the mean half, unsquashed to the Box(-1, 1) by a clip)
 * until it has contributed its share of the n episodes (the CTDE table's quota rule), and each counted episode's
 * per-agent returns and lengths go into a device table.  An episode is what the wrapper makes of it
 * (marl_wrapper.py:77-119): agents that terminate drop out, the env ends (and auto-resets) once every agent has
 * terminated, and a truncation ends nothing.  MARL handles with marl_wrapper = 1 only (CH_ERR_UNSUPPORTED for a CTDE
 * handle and for the bare-dict semantics); both precisions.  All arrays are caller-owned device memory.
 * RLlib is not installed here: these semantics are restated from its defaults ("parity unpinned" to its source).
 * Divergence note (the one ch_marl_rollout_collect documents): RLlib's per-agent episodes treat terminated OR
 * truncated as done; this restatement follows the wrapper's "__all__" rule, under which a truncation does not end
 * an episode. */
typedef struct ch_marl_eval_table {
    int32_t  capacity;      /* C: episode slots per env */
    int32_t  _pad;
    int32_t* quota;         /* device [E]: episodes env e contributes: (n + e) / E, the CTDE table's rule */
    int32_t* count;         /* device [E]: episodes recorded for env e (never exceeds quota) */
    double*  ep_return;     /* device [E][C]: the sum over agents, in agent order, of agent_return */
    double*  agent_return;  /* device [E][C][N]: each agent's summed float32 rewards over the steps it was live at the
                               start of (added in float64 in step order); 0 for agents that never took part */
    int32_t* ep_length;     /* device [E][C]: env steps of the episode */
    int32_t* agent_length;  /* device [E][C][N]: steps the agent was live at the start of (>= 1 exactly for
                               i < the episode's NUM_DRONES) */
    int32_t* ep_end_step;   /* device [E][C]: the evaluation step index at which it ended */
    int64_t* remaining;     /* device [1]: sum over e of quota[e] - count[e] */
    /* the running state of the current episodes */
    double*  acc_return;    /* device [E][N] */
    int32_t* acc_length;    /* device [E][N] */
    int32_t* acc_steps;     /* device [E] */
    uint8_t* live;          /* device [E][N]: the agent is live at the start of the step about to run / that just ran */
} ch_marl_eval_table;

/* Start an evaluation of n_eval_episodes episodes: quota[e] = (n_eval_episodes + e) / E, count = 0, every acc_* = 0,
 * remaining = n_eval_episodes (`live` is ch_marl_eval_mark's).  The slots are not cleared: slot [e][k] is valid for
 * k < count[e].  CH_ERR_INVALID if n_eval_episodes < 1 or ceil(n_eval_episodes / E) > capacity. */
int ch_marl_eval_begin(ch_handle* h, const ch_marl_eval_table* table, int32_t n_eval_episodes, void* stream);

/* Before a step: live[e][i] = i < NUM_DRONES(e) && bit i of active_mask(e), read from the handle's env ints -- the
 * wrapper's self.agents, exactly ch_marl_rollout's agent_mask. */
int ch_marl_eval_mark(ch_handle* h, const ch_marl_eval_table* table, void* stream);

/* After a ch_step with CH_STEP_AUTORESET on the same stream (io->reward and io->reset_happened are required,
 * CH_ERR_INVALID otherwise), one thread per env, agents in index order: for every agent with `live` set
 * acc_return += (double)reward[e][i] and acc_length += 1 (the reward of an agent that is not live is never read into
 * a sum); acc_steps += 1.  Where reset_happened[e] is set: if count < quota and count < capacity the episode goes
 * into slot count[e] (agent_return / agent_length = the accumulators, ep_return = their sum in agent order from 0,
 * ep_length = acc_steps, step_index), the env counts it and `remaining` drops (one integer atomic per wave); in every
 * ended env, filed or ignored, the accumulators return to 0.  0 <= step_index < 2^31. */
int ch_marl_eval_record(ch_handle* h, const ch_marl_eval_table* table, const ch_step_io* io, int64_t step_index,
                        void* stream);

/* The evaluation loop in one call: ch_evaluate_policy's for a MARL handle.  Per step t on `stream`:
 * ch_policy_forward(policy) on the agents' observations into io->policy_out ([E * N][width], width >= 4; 8 = mean
 * then log_std is the trained model's); one action kernel that runs the recorder of step t - 1 (between two reads of
 * `remaining`), marks `live` and writes env_actions[e][i][c] = clamp(policy_out[e * N + i][c], -1, 1), c < 4, for
 * live agents and 0 for the others; ch_step with auto-reset.  Every check_every steps and at max_steps a stand-alone
 * recorder runs, `remaining` and the device error word are copied to the host and the stream is synchronised --
 * nowhere else.  Return codes, *steps_run, *remaining, "reaching max_steps is not an error" and continuation with
 * first_step_index are ch_evaluate_policy's. */
typedef struct ch_marl_eval_io {
    const ch_step_io* step;   /* env step buffers: obs, reward, terminated, truncated, reset_happened */
    float* policy_out;        /* scratch [E * N][policy->dims[last]] */
    float* env_actions;       /* scratch [E][N][4] */
} ch_marl_eval_io;
int ch_marl_evaluate_policy(ch_handle* h, const ch_mlp* policy, const ch_marl_eval_table* table,
                            const ch_marl_eval_io* io, int64_t max_steps, int32_t check_every, int64_t first_step_index,
                            int64_t* steps_run, int64_t* remaining, void* stream);

/* ---- Native PPO minibatch update ---------------------------------------------------------------------------
 * Replaces: stable_baselines3 PPO.train for the CTDE driver's PPO("MlpPolicy", ...) (CTDECattleHerder.py:107-150),
 * one minibatch step at a time: ActorCriticPolicy.evaluate_actions (separate tanh MLPs obs -> pi -> action_net and
 * obs -> vf -> value_net, DiagGaussian with a free log_std), per-minibatch advantage normalisation (torch's unbiased
 * std, skipped for a one-row minibatch), the clipped surrogate, vf_coef * MSE value loss, the entropy bonus,
 * backward, clip_grad_norm_ and torch Adam (bias correction, no weight decay, no amsgrad).  Float32 on the matrix
 * cores, weights read and written in place in nn.Linear layout.  Handle-free; errors through ch_last_error(NULL).
 * Supported: 1 or 2 hidden layers per MLP, hidden widths multiples of 16 up to 256, act_dim 1..64, obs_dim >= 1;
 * anything else is CH_ERR_UNSUPPORTED on entry.  Every sum runs in a fixed order: the same state gives the same
 * bits.  All pointers are device pointers unless a call says "host only". */
typedef struct ch_ppo_net {
    int32_t obs_dim, act_dim;
    int32_t n_pi, n_vf;        /* hidden layers of the policy / value MLP: 1 or 2 */
    int32_t pi[2], vf[2];      /* their widths */
    float* pi_weight[3];       /* mlp_extractor.policy_net's Linear layers, then action_net at [n_pi] */
    float* pi_bias[3];
    float* vf_weight[3];       /* mlp_extractor.value_net's Linear layers, then value_net at [n_vf] */
    float* vf_bias[3];
    float* log_std;            /* [act_dim] */
} ch_ppo_net;

typedef struct ch_ppo_hparams {
    double learning_rate, beta1, beta2, eps;    /* Adam (SB3: 3e-4, 0.9, 0.999, 1e-5) */
    double clip_range, ent_coef, vf_coef, max_grad_norm;
    int32_t normalize_advantage;
    int32_t _pad;
} ch_ppo_hparams;

/* The flattened rollout buffer (RolloutBuffer.get's arrays): obs [rows][obs_dim], actions [rows][act_dim],
 * old_log_prob, advantages, returns [rows]. */
typedef struct ch_ppo_data {
    const float* obs;
    const float* actions;
    const float* old_log_prob;
    const float* advantages;
    const float* returns;
    int64_t rows;
} ch_ppo_data;

/* Host only.  Replaces: sum(p.numel() for p in policy.parameters()).  The number of parameters, which is the length
 * of the flat gradient and of Adam's m and v; -1 for an unsupported net.  The flat order is that of
 * cattleherd.ppo.SB3ActorCritic.parameters(): policy MLP (weight, bias per layer), value MLP, action_net, value_net,
 * log_std.  The net's pointers are not read.
 * With -1 (here and from ch_ppo_scratch_size) the reason is what ch_last_error(NULL) returns next. */
int64_t ch_ppo_param_count(const ch_ppo_net* net);

/* Host only.  No reference counterpart (torch autograd keeps its own buffers): floats of device scratch the calls
 * below need for minibatches of up to batch_size rows; -1 for an unsupported net or batch_size < 1, with the reason
 * as for ch_ppo_param_count. */
int64_t ch_ppo_scratch_size(const ch_ppo_net* net, int64_t batch_size);

/* Replaces: PPO.train's loss.backward() for one minibatch (evaluate_actions, the three loss terms, autograd).
 * idx: int64 [batch], rows of `data`; PRECONDITION 0 <= idx[i] < data->rows (not checked on the device).
 * grad_flat [param_count] receives the gradient (unclipped); stats4 = policy loss, value loss (the MSE, without
 * vf_coef), mean entropy, gradient L2 norm.  Nothing is updated.  scratch: 16-byte aligned. */
int ch_ppo_grad(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                int64_t batch, float* grad_flat, float* stats4, float* scratch, void* stream);

/* Replaces: torch.nn.utils.clip_grad_norm_(policy.parameters(), max_grad_norm) and policy.optimizer.step() (Adam)
 * from a given flat gradient: coefficient min(1, max_grad_norm / (norm + 1e-6)), then Adam on the net's weights in
 * place with m, v [param_count] and the step count *step_dev (int64, incremented on the device). */
int ch_ppo_adam(const ch_ppo_net* net, const ch_ppo_hparams* hp, const float* grad_flat, float* m, float* v,
                int64_t* step_dev, float* scratch, void* stream);

/* Replaces: one epoch of PPO.train's loop over RolloutBuffer.get(batch_size): ceil(n_idx / batch_size) consecutive
 * minibatch steps (gradient, clip, Adam) over idx (int64 [n_idx], a permutation drawn by the caller; the same
 * precondition as ch_ppo_grad), the last one partial if batch_size does not divide n_idx.  Stream-ordered, no host
 * synchronisation.  stats: NULL or [steps][4] as in ch_ppo_grad. */
int ch_ppo_train(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                 int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev, float* stats, float* scratch,
                 void* stream);

/* ch_ppo_train with SB3's two per-minibatch diagnostics (PPO.train's approx_kl_divs and clip_fractions), from the
 * values the loss already holds: log_ratio = log_prob - old_log_prob, ratio = exp(log_ratio),
 *   approx_kl = mean((ratio - 1) - log_ratio), clip_fraction = mean(|ratio - 1| > clip_range),
 * summed per 16-row tile in row order and over the tiles in index order (rows past the minibatch add 0): the same
 * state gives the same bits.  clip_fraction tests the loss's own float32 ratio.  approx_kl's row term cancels (it is
 * ~log_ratio^2 / 2), so it alone is evaluated in float64 -- the log-probability summed again from the same float32
 * mean, then expm1(log_ratio) - log_ratio -- and rounded once to float32.
 * stats is required: [steps][CH_PPO_LOG_STATS], columns 0-3 what ch_ppo_train writes into [steps][4] from the same
 * state, then approx_kl, clip_fraction.  The weights, m, v and the step count are what ch_ppo_train leaves. */
#define CH_PPO_LOG_STATS 6   /* policy loss, value loss, mean entropy, grad norm, approx_kl, clip_fraction */
int ch_ppo_train_log(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                     int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev, float* stats,
                     float* scratch, void* stream);

/* Replaces: the rest of PPO.train's loop body that ch_ppo_train_log leaves out -- PPO(..., target_kl=, clip_range_vf=):
 *   values_pred = old_values + clamp(values - old_values, -clip_range_vf, clip_range_vf)   (clip_range_vf set)
 *   if approx_kl > 1.5 * target_kl: continue_training = False; break                     (target_kl set)
 * One call is one epoch, as ch_ppo_train_log; `opts` carries the two options and what they read.
 * Value clipping: the clipped prediction enters the squared error (column 1 is then the clipped value loss), and a
 * row with |values - old_values| > clip_range_vf gives the value head no gradient; a row exactly at the bound keeps
 * it (torch.clamp's backward).
 * The gate runs on the device, with no host synchronisation: the minibatch's approx_kl is column 4's float32 value,
 * and every workgroup that needs the decision forms it from the same per-tile sums in the same order.  A minibatch
 * that trips writes its statistics row, sets *stop_dev and changes nothing else: no weight, m, v, and *step_dev does
 * not advance (SB3 breaks before the optimizer step).  With *stop_dev non-zero -- later minibatches of the call, and
 * later calls handed the same word, the following epochs -- every launch returns at entry: weights, m, v, *step_dev
 * and *stop_dev stay bit-for-bit as they were.
 * stats is required: [steps][CH_PPO_OPT_STATS]; column 6, `state`: 1 the optimizer step was applied, 0 this
 * minibatch tripped the gate (columns 0-5 valid, ch_ppo_train_log's), -1 not run because the gate had tripped
 * (columns 0-5 NaN).  SB3's lists hold the rows with state >= 0; n_updates grows by the epochs with such a row.
 * With both options off (<= 0) the weights, m, v, the step count and columns 0-5 are bit-identical to
 * ch_ppo_train_log from the same state.  ch_ppo_scratch_size sizes the scratch; the flat gradient of the last
 * minibatch that ran is its last region, param_count floats rounded up to a multiple of 4.
 * CH_ERR_INVALID (nothing is launched) for NULL opts, clip_range_vf > 0 with NULL old_values, target_kl > 0 with NULL
 * stop_dev.
 * DIFFERENCE: SB3 compares np.mean of a float32 tensor's numpy array with the Python float 1.5 * target_kl; whether
 * that comparison runs in float32 or float64 depends on the numpy version's promotion rules.  The device compares in
 * float64: (double)approx_kl > 1.5 * target_kl, approx_kl being the float32 statistic.  A NaN approx_kl does not trip,
 * as in SB3. */
typedef struct ch_ppo_opts {
    double target_kl;        /* <= 0: no gate (SB3 None) */
    double clip_range_vf;    /* <= 0: no value clipping (SB3 None) */
    const float* old_values; /* [data->rows], RolloutBuffer.values; required when clip_range_vf > 0 */
    int32_t* stop_dev;       /* required when target_kl > 0: 0 = running, non-zero = stopped; the caller zeroes it
                                before a train() and passes the same word to every epoch's call */
} ch_ppo_opts;
#define CH_PPO_OPT_STATS 7   /* CH_PPO_LOG_STATS columns, then `state` */
int ch_ppo_train_opt(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const ch_ppo_opts* opts,
                     const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev,
                     float* stats, float* scratch, void* stream);

/* ---- Population update: P independent learners of one architecture in one set of launches ----------------------
 * Replaces: P independent PPO.train epochs (seeds, hyper-parameter variants), one ch_ppo_train_opt call each; the
 * reference has no counterpart for running them together.  A minibatch step of one learner is three dependent launches
 * that fill a small part of the device; here each of the three launches carries every member, the member being a grid
 * dimension.  A member is everything ch_ppo_train_opt takes: its own weights, Adam state, rollout data, permutation,
 * hyper-parameters, options with its own stop word, statistics table and scratch.
 * CONTRACT: after ch_ppo_train_pop every member's weights, m, v, *step_dev, stop word, statistics table and the flat
 * gradient left in its scratch are bit-for-bit what ch_ppo_train_opt(&net, &hp, &data, &opts, idx, n_idx, batch_size,
 * m, v, step_dev, stats, scratch, stream) leaves for that member from the same state: the kernels run the same code
 * on the same arguments, and nothing is shared between members.  The KL gate is per member: one that trips, or whose
 * stop word is already set, stops exactly as it does alone while the others carry on.
 * Members may not alias each other's writable memory (weights, m, v, step_dev, stats, scratch, stop word); what is
 * only read (the data, idx) may be shared. */
typedef struct ch_ppo_member {
    ch_ppo_net net; ch_ppo_hparams hp; ch_ppo_data data; ch_ppo_opts opts;
    const int64_t* idx;          /* [n_idx], this member's permutation */
    float* m; float* v; int64_t* step_dev;
    float* stats;                /* [steps][CH_PPO_OPT_STATS], required */
    float* scratch;              /* ch_ppo_scratch_size(net, batch) floats, 16-byte aligned, the member's own */
} ch_ppo_member;
typedef struct ch_ppo_pop ch_ppo_pop;   /* opaque: the kernels' argument tables */

/* Replaces: nothing in the reference (see above).  The object that holds the argument tables of up to max_members
 * members on `device`: pinned host staging and the device tables, two slots of each, so that a call may fill its
 * staging while the copy an earlier, still queued call issued reads the other slot's; a slot is reused only after the
 * event behind its copy.  One object is used from one stream at a time.  CH_ERR_INVALID for max_members < 1 or a NULL
 * out, CH_ERR_DEVICE / CH_ERR_NOMEM when the allocation fails. */
int ch_ppo_pop_create(int32_t max_members, int32_t device, ch_ppo_pop** out);
/* Waits for the copies it issued, then frees the tables.  The caller has let the launches that read them finish. */
int ch_ppo_pop_destroy(ch_ppo_pop* pop);

/* Replaces: one epoch of PPO.train's minibatch loop for each of n_members independent learners (see above):
 * ceil(n_idx / batch_size) population steps of three launches each on `stream`, stream-ordered, no host
 * synchronisation beyond the wait for a staging slot two calls old.  The tables are uploaded once per call; a step
 * passes its offset into idx and its statistics row as kernel arguments, and a last, partial minibatch has a table of
 * its own.
 * Checked on the host before anything is launched: 1 <= n_members <= the object's max_members; every member as
 * ch_ppo_train_opt checks it, stats required (CH_ERR_INVALID); the members agree on obs_dim, act_dim, the layer counts
 * and widths, on data.rows and on whether clip_range_vf is set (CH_ERR_UNSUPPORTED).  They may differ in everything
 * else: every hyper-parameter, clip_range_vf's value, target_kl set or not, which pointers are 16-byte aligned. */
int ch_ppo_train_pop(ch_ppo_pop* pop, const ch_ppo_member* members, int32_t n_members, int64_t n_idx,
                     int64_t batch_size, void* stream);

/* Replaces: stable_baselines3.common.utils.explained_variance(rollout_buffer.values.flatten(),
 * rollout_buffer.returns.flatten()), PPO.train's train/explained_variance.  Handle-free; errors through
 * ch_last_error(NULL).  out_dev[0] = 1 - var(returns - values) / var(returns) with population variances (np.var), NaN
 * when var(returns) == 0; out_dev[1] = var(returns).  Float64 and two-pass: the means first, then the squared
 * deviations; workgroup partials are combined in index order (no atomics: the same input gives the same bits).
 * DIFFERENCE: SB3 computes this in float32 numpy; here the float32 inputs are widened exactly and every sum is
 * float64.  values, returns: device [n], n >= 1; out_dev: device double [2]; scratch: device,
 * ch_explained_variance_scratch(n) doubles (host only; -1 for n < 1). */
int64_t ch_explained_variance_scratch(int64_t n);
int ch_explained_variance(const float* values, const float* returns, int64_t n, double* out_dev, double* scratch,
                          void* stream);

/* Replaces: n_members calls of ch_explained_variance, one per member of a population, by one set of three launches
 * with the member as a grid dimension.  values_dev, returns_dev: DEVICE arrays of n_members device pointers, each to
 * [n] floats (the members' buffers are separate allocations); out_dev: device double [n_members][2]; scratch: device,
 * ch_explained_variance_pop_scratch(n, n_members) doubles ([n_members][4G]; host only, -1 for n < 1 or n_members < 1).
 * CONTRACT: out_dev[p] is bit for bit what ch_explained_variance(values[p], returns[p], n, ...) gives: the same grid
 * for n, the same elements per workgroup, the same per-thread and tree order (the kernels share their bodies).
 * Handle-free; CH_ERR_INVALID for a NULL argument, n_members outside 1..65535 or n < 1. */
int64_t ch_explained_variance_pop_scratch(int64_t n, int32_t n_members);
int ch_explained_variance_pop(const float* const* values_dev, const float* const* returns_dev, int32_t n_members,
                              int64_t n, double* out_dev, double* scratch, void* stream);

/* ---- Native PPO minibatch update for the DTDE (RLlib) driver's shared policy ---------------------------------
 * Replaces: the minibatch step of RLlib 2.x's new-API-stack PPO learner (PPOTorchLearner.compute_loss_for_module,
 * the optimizer step) for the DTDE driver's shared policy (DTDECattleHerder.py:62-97), with RLlib's defaults.  The
 * module: actor encoder (tanh MLP) -> pi, whose 2 * act_dim outputs are the DiagGaussian's mean then raw log_std,
 * log_std = clamp(raw, -log_std_clip, log_std_clip) with torch.clamp's gradient (k_marl_store applies the same
 * clamp when sampling); a critic encoder of its own (vf_share_layers False) -> vf.  Loss of a minibatch of B rows:
 *   mean(-min(A ratio, A clamp(ratio, 1 - clip_param, 1 + clip_param)) + vf_loss_coeff clamp((V - R)^2, 0,
 *   vf_clip_param) - entropy_coeff H) + kl_coeff mean(KL(sampling policy || current)),
 * advantages taken as given (the caller standardises them once per training iteration), kl_coeff read from device
 * memory at each step; then an optional global-norm clip and torch Adam.  The kernels are ch_ppo.hip's, compiled
 * for this loss and head.  RLlib is not installed here: restated from its source and defaults ("parity unpinned").
 * Supported: 1 or 2 hidden layers per encoder, widths multiples of 16 up to 256, act_dim 1..32, obs_dim >= 1;
 * anything else is CH_ERR_UNSUPPORTED on entry.  Handle-free; errors through ch_last_error(NULL).  The same state
 * gives the same bits.  All pointers are device pointers unless a call says "host only". */
typedef struct ch_marl_ppo_net {
    int32_t obs_dim, act_dim;
    int32_t n_actor, n_critic;     /* hidden layers of the actor / critic encoder: 1 or 2 */
    int32_t actor[2], critic[2];   /* their widths */
    float* actor_weight[3];        /* encoder.actor_encoder's Linear layers, then pi [2 * act_dim][.] at [n_actor] */
    float* actor_bias[3];
    float* critic_weight[3];       /* encoder.critic_encoder's Linear layers, then vf at [n_critic] */
    float* critic_bias[3];
} ch_marl_ppo_net;

typedef struct ch_marl_ppo_hparams {
    double learning_rate, beta1, beta2, eps;    /* Adam (RLlib: 5e-5, 0.9, 0.999, 1e-8) */
    double clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff;   /* (RLlib: 0.3, 10, 1, 0) */
    double log_std_clip;                        /* (RLlib: 20) */
    double grad_clip;                           /* global-norm clip; <= 0: none (RLlib's default) */
    const float* kl_coeff_dev;                  /* one float on the device, read by each step (RLlib starts at 0.2) */
} ch_marl_ppo_hparams;

/* The live agents' rows of a DTDE rollout: obs [rows][obs_dim], actions [rows][act_dim], old_log_prob [rows],
 * old_dist_inputs [rows][2 * act_dim] (the sampling policy's mean, then its clamped log_std), advantages [rows]
 * (already standardised), value_targets [rows]. */
typedef struct ch_marl_ppo_data {
    const float* obs;
    const float* actions;
    const float* old_log_prob;
    const float* old_dist_inputs;
    const float* advantages;
    const float* value_targets;
    int64_t rows;
} ch_marl_ppo_data;

/* Host only.  Replaces: sum(p.numel() for p in module.parameters()).  The length of the flat gradient and of
 * Adam's m and v; -1 for an unsupported net.  The flat order is that of cattleherd.marl_ppo.RLlibActorCritic
 * .parameters(): actor encoder (weight, bias per layer), critic encoder, pi, vf.  The net's pointers are not read.
 * With -1 (here and from ch_marl_ppo_scratch_size) the reason is what ch_last_error(NULL) returns next. */
int64_t ch_marl_ppo_param_count(const ch_marl_ppo_net* net);

/* Host only.  No reference counterpart (torch autograd keeps its own buffers): floats of device scratch the calls
 * below need for minibatches of up to batch_size rows; -1 for an unsupported net or batch_size < 1.  The size covers
 * ch_marl_ppo_train_log as well: it includes that call's region of 33 floats per 16-row tile (a tile's sum, and each
 * row's value and target), whichever call the scratch is for. */
int64_t ch_marl_ppo_scratch_size(const ch_marl_ppo_net* net, int64_t batch_size);

/* Replaces: the learner's compute_losses + backward for one minibatch.  idx: int64 [batch], rows of `data`;
 * PRECONDITION 0 <= idx[i] < data->rows (not checked on the device).  grad_flat [param_count] receives the gradient
 * (unclipped); stats5 = policy loss (-mean surrogate), value loss (mean clipped squared error, without
 * vf_loss_coeff), mean entropy, mean KL, gradient L2 norm.  Nothing is updated.  scratch: 16-byte aligned. */
int ch_marl_ppo_grad(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                     const int64_t* idx, int64_t batch, float* grad_flat, float* stats5, float* scratch, void* stream);

/* Replaces: the learner's gradient clipping (grad_clip_by "global_norm": coefficient min(1, grad_clip / (norm +
 * 1e-6)); exactly 1 when grad_clip <= 0) and its Adam step from a given flat gradient, on the net's weights in place
 * with m, v [param_count] and the step count *step_dev (int64, incremented on the device). */
int ch_marl_ppo_adam(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const float* grad_flat, float* m,
                     float* v, int64_t* step_dev, float* scratch, void* stream);

/* Replaces: one epoch of the learner's minibatch loop: ceil(n_idx / batch_size) consecutive minibatch steps
 * (gradient, clip, Adam) over idx (int64 [n_idx], drawn by the caller from the live rows; the same precondition as
 * ch_marl_ppo_grad), the last one partial if batch_size does not divide n_idx (RLlib's cyclic iterator would wrap
 * around instead).  Stream-ordered, no host synchronisation.  stats: NULL or [steps][5] as in ch_marl_ppo_grad. */
int ch_marl_ppo_train(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                      const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev,
                      float* stats, float* scratch, void* stream);

/* ch_marl_ppo_train with the rest of RLlib's learner record (learners/shared_policy/...) per minibatch step.  stats is
 * required: [steps][CH_MARL_PPO_LOG_STATS], columns 0-4 what ch_marl_ppo_train writes into [steps][5] from the same
 * state, then
 *   vf_loss_unclipped  = mean((v - target)^2) before the clamp (float32: the loss's own squared errors, summed per
 *                        16-row tile in row order and over the tiles in index order),
 *   total_loss         = policy_loss + vf_loss_coeff * vf_loss - entropy_coeff * entropy + kl_coeff * kl, the sum
 *                        formed in float64 from columns 0-3 and the coefficient on the device, rounded once,
 *   vf_explained_var   = RLlib's explained_variance(value_targets, values) over the minibatch:
 *                        max(-1, 1 - var(y - v) / (var(y) + 1e-6)) with torch's unbiased variances; NaN for a one-row
 *                        minibatch (0 / 0), and a NaN stays a NaN under the max.
 * DIFFERENCE: RLlib computes the variances in float32; the differences cancel, so here both are two-pass float64
 * reductions (the means, then the squared deviations) over the exactly widened float32 y and v -- the v the loss
 * used -- in a fixed order (thread t of one workgroup adds rows t, t + 256, ..., a fixed tree adds the threads), and
 * the result is rounded once.  (Restated from RLlib's source: parity unpinned.)
 * The weights, m, v, the step count and columns 0-4 are what ch_marl_ppo_train leaves, bit for bit.  The forward-
 * backward and Adam kernels are instantiations of their own: ch_marl_ppo_train launches what it launched before. */
#define CH_MARL_PPO_LOG_STATS 8   /* policy loss, vf loss, entropy, kl, grad norm, vf_loss_unclipped, total_loss, vf_explained_var */
int ch_marl_ppo_train_log(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                          const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev,
                          float* stats, float* scratch, void* stream);

/* ---- Device-side evaluator log: the per-step rows of update_evaluation_metrics ---------------------------------
 * Replaces: the reference's logging while is_evaluating is set -- BaseAviary.update_evaluation_metrics (sb3_envs/
 * BaseAviary.py:1406-1437) and the time-out evaluation_episode_trigger of _computeTruncated (CattleAviary.py:545-548)
 * -- for a chosen subset of a batch's envs, as a device table: one row per logged env and step, written by a small
 * kernel after the step, with no host synchronisation and no copy of the state (HerdBatch.get_state is the only other
 * route to these values).  cattleherd.eval_log turns the table into the reference's evaluation_data.pkl schema.
 *
 * THE ONE RESTRICTION: the recorder reads the handle's state, which must be the post-step, pre-reset state.  It
 * therefore follows a ch_step WITHOUT CH_STEP_AUTORESET; the caller (or ch_eval_log_run) then resets the finished envs
 * with a masked ch_reset.  With the flag set in the io, ch_eval_log_record returns CH_ERR_INVALID.
 * CTDE handles only (MARL: CH_ERR_UNSUPPORTED), both precisions (an f32 handle's state is widened exactly: the log is
 * always float64; positions are the f64 copies ch_get_state returns).  The handle needs cfg.eval_metrics
 * (CH_ERR_UNSUPPORTED otherwise, as ch_get_eval).  N = cfg.num_drones, M = cfg.num_cattle below.
 * The env indices of sel_env must be distinct: each logged env's rows are owned by one wave and written with plain
 * stores, so a duplicate index leaves rows / dropped and the rows of that env undefined. */
typedef struct ch_eval_log {
    int32_t n_sel;            /* S: logged envs */
    int32_t capacity;         /* T: rows per logged env */
    const int32_t* sel_env;   /* device [S]: env indices, distinct, 0 <= . < E (validated on entry by the caller-facing
                                 Python; the kernel skips an out-of-range index and sets the handle's error word) */
    int32_t* rows;            /* device [S]: rows written so far (<= T) */
    int32_t* dropped;         /* device [S]: steps not logged because the env's rows were full */
    /* per row [S][T] */
    double*  time;            /* step_counter at the step's start / ctrl_freq (update_evaluation_metrics' ep_time) */
    double*  effectiveness;   /* evaluate_herding_effectiveness after the step, in percent */
    int32_t* num_drones;      /* NUM_DRONES of the episode */
    int32_t* episode;         /* the env's episode counter (env int `episode`) */
    uint8_t* flags;           /* bit 0 terminated, bit 1 truncated (the step's outputs), bit 2 time-out trigger:
                                 ep_time > EPISODE_LEN_SEC and none of _computeTruncated's conditions 1-4 holds
                                 (CattleAviary.py:513-548) -- where evaluation_episode_trigger fires.  EPISODE_LEN_SEC
                                 is the handle's (its configured curriculum level's), the value the step's own
                                 truncation compares with */
    double*  drone_xy;        /* [S][T][N][2] after the step; 0 for i >= NUM_DRONES */
    double*  drone_vxy;       /* [S][T][N][2] */
    double*  drone_dist;      /* [S][T][N]   the evald accumulator after the step */
    double*  cattle_xy;       /* [S][T][M][2] after the step */
    double*  cattle_vxy;      /* [S][T][M][2] at the step's START (what the reference's read-back returns) */
    /* carry, written by ch_eval_log_mark */
    double*  start_cattle_vxy;/* device [S][M][2] */
    int32_t* start_counter;   /* device [S] */
} ch_eval_log;
/* (drone_xy, drone_vxy, cattle_xy, cattle_vxy and start_cattle_vxy are stored as pairs: 16-byte aligned.) */

/* rows = dropped = 0 for every logged env.  Stream-ordered. */
int ch_eval_log_begin(ch_handle* h, const ch_eval_log* log, void* stream);
/* Before a step: the carry (the cattle velocities and step_counter at the step's start) of every logged env. */
int ch_eval_log_mark(ch_handle* h, const ch_eval_log* log, void* stream);
/* After a step without CH_STEP_AUTORESET (io: that step's io; terminated and truncated are read): one row per logged
 * env.  An env whose rows are full increments `dropped` and writes nothing; no row index ever reaches `capacity`,
 * whatever the arrays hold. */
int ch_eval_log_record(ch_handle* h, const ch_eval_log* log, const ch_step_io* io, void* stream);

typedef struct ch_eval_log_io {
    const ch_step_io* step;  /* obs, reward, terminated, truncated; flags must not hold CH_STEP_AUTORESET */
    float* mean;             /* scratch [E][actor->dims[last]] */
    float* env_actions;      /* scratch [E][num_drones][4] */
    uint8_t* done_mask;      /* scratch [E] */
} ch_eval_log_io;
/* Replaces: the playback loop `action = model.predict(obs, deterministic=True); env.step(action); env.reset() when
 * the episode ended` with is_evaluating set, for every env of the batch, n_steps times: ch_policy_forward, the
 * deterministic action (the clamp ch_evaluate_policy documents), mark, ch_step without auto-reset, record -- which
 * here also writes done_mask[e] = terminated | truncated for EVERY env -- and ch_reset(done_mask) into step->obs.
 * No host synchronisation and no host read; a HIP error ends the loop with CH_ERR_DEVICE and nothing further is
 * launched.  The sticky device error word is not read here: the caller's ch_sync reports it. */
int ch_eval_log_run(ch_handle* h, const ch_mlp* actor, const ch_eval_log* log, const ch_eval_log_io* io,
                    int64_t n_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATTLEHERD_H */
