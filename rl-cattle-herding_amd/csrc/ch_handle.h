// ch_handle.h — the handle behind the C ABI, private to its host files: ch_api.cpp (config, create / destroy, reset,
// step, state, metrics, host output), ch_api_policy.cpp (policy forwards, PPO and MARL rollout collection),
// ch_api_eval.cpp (the on-device evaluate_policy and the DTDE driver's evaluation), ch_api_eval_log.cpp (the device-side
// evaluator log), ch_api_train_log.cpp (the SB3 and the RLlib training log) and ch_api_norm.cpp (the device-side
// VecNormalize and the collection under it).
//
// What the env step launches is the handle's StepPlan (ch_step_plan.h): ch_create asks the planner once, for the
// handle's shape on its device; ch__set_kernel, ch__set_geometry and ch__set_phase_mask change the overrides and ask
// again.  ch_step, ch_step_n and the fused rollout step read the plan and launch its rows; none of them decides anything.
#pragma once
#include <string>
#include <vector>

#include "ch_internal.h"
#include "ch_step_plan.h"

// ch_rollout_collect's state (ch_api_policy.cpp)
struct ch_rollout_state {
    // the deferred-bootstrap queue (allocated on first use, grown when a call needs more): terminal observations,
    // their rewards rows, the count, the values; and the bytes each buffer holds
    float* tv_obs = nullptr;
    long long* tv_row = nullptr;
    int* tv_count = nullptr;
    float* tv_val = nullptr;
    size_t tv_obs_bytes = 0, tv_row_bytes = 0, tv_count_bytes = 0, tv_val_bytes = 0;
    // the collection's path (diagnostics / tests, ch__set_rollout_path): bit 0 copy every step's observation into
    // the buffer instead of stepping into its slots, bit 1 the stand-alone store kernel instead of the forward epilogues,
    // bit 2 the actor forward fused into the step kernel (k_step2_actor, where the geometry takes it), bit 3 never fused
    int path = 0;
    long long fused_steps = 0;   // fused steps launched by ch_rollout_collect (ch__rollout_fused_steps)
};

// ch_outputs_to_host's device staging of the envs that auto-reset (allocated on first use): count, indices,
// episode statistics, terminal observation blocks; and the pinned host copy of the count
struct ch_staging {
    long long* count = nullptr;
    long long* env = nullptr;
    double* stats = nullptr;
    float* obs = nullptr;
    long long* count_host = nullptr;
    // how many ended envs ch_outputs_to_host copies before it knows the count: twice the larger of the last count and
    // its running mean, plus 8 (a step where more end costs one more copy and stream sync)
    double ended_mean = 8.0;
    int64_t ended_last = 8;
};

struct ch_handle {
    ch_config cfg{};
    int64_t E = 0;
    int device = 0;
    int NC = 0, M = 0, rows = 0, K = 0, team = 0;
    int start_level = 0;
    double episode_len = 0;
    size_t rsize = 8;
    void* drone = nullptr;
    // Euler angles of each drone's stored quaternion, written by the v2 step at the end of every
    // step (it needs them for the observation anyway) and read by the next one instead of
    // recomputing atan2/asin/atan2; any other writer of the state clears rpy_valid.
    void* rpy = nullptr;
    uint8_t* stale = nullptr;   // device [2][E]: StepParams::stale (Euler cache stale, obs bytes unknown, per env)
    unsigned long long* obs_tag = nullptr;   // device [E]: StepParams::obs_tag (the buffer holding env e's constant obs bytes)
    void* cattle = nullptr;
    void* phys = nullptr;   // [kPhysComps][E][NC]: last_clipped_action, DYN rpy_rates
    void* envr = nullptr;
    // f32 mode only: the f64 copies of the positions and prev_cent_dists the step integrates and measures
    // centroids on (StepParams::pos64 / cpos64 / prev64); the f32 arrays above keep their rounded values
    double* pos64 = nullptr;    // [3][E][NC]
    double* cpos64 = nullptr;   // [2][E][M]
    double* prev64 = nullptr;   // [E]
    int* envi = nullptr;
    double* metrics = nullptr;
    double* spawn = nullptr;
    int n_scen = 0, n_cows = 0;
    double* debug = nullptr;
    // The obs buffer whose constant-zero bytes (rows >= NUM_DRONES, the action-buffer block, padding)
    // are known to hold zeros: the last one a full-block writer (v1 step, full ch_reset, v2 step with
    // obs_full) wrote.  The v2 step then stores only the entries that change.
    const float* obs_zero_ptr = nullptr;
    // the step's kernels and geometry (ch_step_plan.h): the plan, what it was planned for (the shape is cfg and E; the
    // device's CU count and LDS budget) and the diagnostics' overrides
    ch::StepPlan plan{};
    ch::StepOverrides ov;
    int cus = 0;
    size_t lds_budget = 0;
    long long* tstamp = nullptr;
    int P = 0;                   // cow pairs per env, and their list (v2 step)
    uint16_t* pairs = nullptr;
    int* errw = nullptr;        // device error word (CH_DEVERR_* bits), sticky
    double* evald = nullptr;    // [E][NC] evaluation distances (cfg.eval_metrics)
    int* rdn = nullptr;         // ch_reset_with: device copies of the injected draws
    double* rdv = nullptr;
    double* mdev = nullptr;     // device [CH_METRIC_COUNT + 1]: reduced metrics + error word
    double* mhost = nullptr;    // pinned host copy of mdev
    long long multi_steps = 0;   // steps ch_step_n ran inside k_step2_multi (ch__multi_steps)
    void* d_params = nullptr;    // k_step2_multi's parameters (device copy, ch_step_n)
    std::vector<unsigned char> params_host;   // what d_params holds (uploaded again only when the parameters change)
    ch_rollout_state ro;
    ch_staging st;
    // ch_evaluate_policy's and ch_marl_evaluate_policy's pinned host copy of {the table's remaining, the device error word} (allocated on first use)
    long long* eval_host = nullptr;
    // the device error word was reported to the caller (device_status) since it was last cleared
    bool err_seen = false;
    std::string err;
};

// the message ch_last_error(NULL) returns: failures without a handle, from either host file (defined in ch_api.cpp)
extern thread_local std::string g_create_err;

inline int fail(ch_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}

// the sticky device error word as a status, after the stream has drained (ch_api.cpp; what ch_sync returns)
int device_status(ch_handle* h, int word);

#define HIP_TRY(h, expr)                                                                           \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail((h), CH_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

// the episode ring's checks (ch_api_train_log.cpp; ch_ep_ring_record and ch_rollout_collect_log share them): a whole
// ring, a CTDE handle, and -- with `io` -- a step io that carries reset_happened and episode_stats; fills `a`
int ep_ring_args(ch_handle* h, const ch_ep_ring* ring, const ch_step_io* io, ch::EpRingArgs& a, const char* who);

// a population's rings' checks (ch_api_train_log.cpp; ch_ep_ring_pop_* and ch_rollout_collect_pop_log share them): whole
// rings with window >= 1 and n_members >= 1, and -- `h_needed` -- a CTDE handle whose envs divide among the members and,
// with `io`, a step io that carries reset_happened and episode_stats; fills `a` for launch_ep_ring_record_pop
int ep_ring_pop_args(ch_handle* h, const ch_ep_ring_pop* ring, const ch_step_io* io, ch::EpRingArgs& a, const char* who,
                     bool h_needed);

// the MARL episode ring's checks (ch_api_train_log.cpp; ch_marl_ep_ring_record and ch_marl_rollout_collect_log
// share them): a whole ring, a MARL handle under the wrapper's semantics, and -- with `io` -- a step io that carries
// reward and reset_happened; fills `a` but for `live`
int marl_ring_args(ch_handle* h, const ch_marl_ep_ring* ring, const ch_step_io* io, ch::MarlRingArgs& a, const char* who);

// ch_rollout_collect's fused step (ch_api.cpp; launch_step_v2_actor): the step of `io` with the actor forward `fa` on
// the observations it writes (fa.x == io->obs) and the sampling epilogue `ro`.  launch = false: hipSuccess iff the
// handle's plan and the net fit the fused kernel (nothing launched).
hipError_t step_actor(ch_handle* h, const ch_step_io* io, hipStream_t st, const ch::MlpArgs& fa, const ch::RolloutArgs& ro,
                      bool launch);
