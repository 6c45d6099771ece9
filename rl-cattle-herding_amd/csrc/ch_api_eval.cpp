// ch_api_eval.cpp — the evaluation part of the C ABI (see include/cattleherd.h), for CTDE and for MARL (DTDE) handles:
// the device episode tables (ch_eval_begin, ch_eval_record; ch_marl_eval_begin, ch_marl_eval_mark, ch_marl_eval_record;
// kernels in ch_eval.hip and ch_marl_eval.hip) and the one native evaluation loop around ch_policy_forward and ch_step
// behind ch_evaluate_policy and ch_marl_evaluate_policy.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ch_handle.h"

using namespace ch;

// ---- the checks the two drivers share (who: the entry point's name, first in every message) -------------------------
// the recorders stamp an episode with the index of the step that ended it, an int
static int step_index_arg(ch_handle* h, int64_t step_index, int& out, const char* who) {
    if (step_index < 0 || step_index > INT32_MAX)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": step_index outside [0, 2^31)");
    out = (int)step_index;
    return CH_OK;
}

// n episodes over E envs: the last env's quota must fit the table's slots per env
static int begin_args(ch_handle* h, int32_t n_eval_episodes, int capacity, const char* who) {
    if (n_eval_episodes < 1) return fail(h, CH_ERR_INVALID, std::string(who) + ": n_eval_episodes must be >= 1");
    const int64_t per_env = (n_eval_episodes + h->E - 1) / h->E;   // the last env's quota
    if (per_env > capacity)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": " + std::to_string(n_eval_episodes) + " episodes over " +
                                           std::to_string(h->E) + " envs need " + std::to_string(per_env) +
                                           " slots per env, the table's capacity is " + std::to_string(capacity));
    return CH_OK;
}

// the loop's bounds: they do not depend on the handle, so the loops check them first
static int loop_bounds(ch_handle* h, int64_t max_steps, int32_t check_every, const char* who) {
    if (max_steps < 1)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": max_steps must be >= 1 (the loop is always bounded)");
    if (check_every < 1) return fail(h, CH_ERR_INVALID, std::string(who) + ": check_every must be >= 1");
    return CH_OK;
}

// what the loops check after the table: the pointers (`present`) and the range of the step indices
static int loop_args(ch_handle* h, bool present, int64_t max_steps, int64_t first_step_index, const char* who) {
    if (!present) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL argument");
    if (first_step_index < 0 || first_step_index > INT32_MAX - max_steps)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": first_step_index + max_steps outside [0, 2^31)");
    return CH_OK;
}

// ---- the tables' kernel arguments -----------------------------------------------------------------------------------
// a CTDE handle and a whole table
static int table_args(ch_handle* h, const ch_eval_table* tb, EvalArgs& a, const char* who) {
    if (!tb) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL table");
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
    if (h->cfg.mode != CH_MODE_CTDE)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the episode table is for CTDE handles");
    if (tb->capacity < 1 || !tb->quota || !tb->count || !tb->ep_return || !tb->ep_length || !tb->ep_flags ||
        !tb->ep_end_step || !tb->remaining)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": capacity >= 1 and every table array are required");
    std::memset(&a, 0, sizeof(a));
    a.E = h->E; a.C = tb->capacity;
    a.quota = tb->quota; a.count = tb->count; a.ep_return = tb->ep_return; a.ep_length = tb->ep_length;
    a.ep_flags = tb->ep_flags; a.ep_end_step = tb->ep_end_step;
    a.remaining = reinterpret_cast<long long*>(tb->remaining);
    return CH_OK;
}

// a MARL handle under the wrapper's semantics and a whole table
static int table_args(ch_handle* h, const ch_marl_eval_table* tb, MarlEvalArgs& a, const char* who) {
    if (!tb) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL table");
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
    if (h->cfg.mode != CH_MODE_MARL)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the per-agent episode table is for MARL handles");
    if (!h->cfg.marl_wrapper)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the per-agent episode table needs marl_wrapper = 1 "
                                                              "(agents drop out, the env ends when all have terminated)");
    if (tb->capacity < 1 || !tb->quota || !tb->count || !tb->ep_return || !tb->agent_return || !tb->ep_length ||
        !tb->agent_length || !tb->ep_end_step || !tb->remaining || !tb->acc_return || !tb->acc_length || !tb->acc_steps ||
        !tb->live)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": capacity >= 1 and every table array are required");
    std::memset(&a, 0, sizeof(a));
    a.E = h->E; a.N = h->NC; a.C = tb->capacity;
    a.quota = tb->quota; a.count = tb->count; a.ep_return = tb->ep_return; a.agent_return = tb->agent_return;
    a.ep_length = tb->ep_length; a.agent_length = tb->agent_length; a.ep_end_step = tb->ep_end_step;
    a.remaining = reinterpret_cast<long long*>(tb->remaining);
    a.acc_return = tb->acc_return; a.acc_length = tb->acc_length; a.acc_steps = tb->acc_steps; a.live = tb->live;
    a.env_n = h->envi; a.env_active = h->envi + 7 * h->E;
    return CH_OK;
}

// the recorders' inputs: the outputs of the step that just ran
static int record_args(ch_handle* h, const ch_step_io* io, int64_t step_index, EvalArgs& a, const char* who) {
    if (!io || !io->reset_happened || !io->episode_stats || !io->terminated || !io->truncated)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry reset_happened, episode_stats, "
                                                          "terminated and truncated");
    a.reset = io->reset_happened; a.stats = io->episode_stats; a.term = io->terminated; a.trunc = io->truncated;
    return step_index_arg(h, step_index, a.step_index, who);
}

static int record_args(ch_handle* h, const ch_step_io* io, int64_t step_index, MarlEvalArgs& a, const char* who) {
    if (!io || !io->reward || !io->reset_happened)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry reward and reset_happened");
    a.reward = io->reward; a.reset = io->reset_happened;
    return step_index_arg(h, step_index, a.step_index, who);
}

// ---- the evaluation loop --------------------------------------------------------------------------------------------
// SB3 evaluate_policy (and the DTDE driver's evaluation), one step of every env per turn: predict(obs,
// deterministic=True) -> env.step -> the episode lists.  `actions(recorded)` launches the driver's action kernel on
// `policy_out` -- with the recorder of the step before in it unless that step is `recorded` -- and `record()` the
// recorder alone; both return a status and read the table's kernel arguments, whose step_index is `*step_index`.
// The recorder of a step runs in the next step's action kernel (the step's outputs are still in place there: the
// forward in between writes only policy_out), and as a launch of its own only before `remaining` is read: per step that
// leaves the forward, the action kernel and the step.
template <class Actions, class Record>
static int evaluate_loop(ch_handle* h, const ch_mlp* policy, float* policy_out, const ch_step_io* step,
                         float* env_actions, int64_t max_steps, int32_t check_every, int64_t first_step_index,
                         int* step_index, const long long* remaining_dev, int64_t* steps_run, int64_t* remaining,
                         void* stream, Actions actions, Record record) {
    ch_step_io s = *step;
    s.actions = env_actions; s.actions_out = nullptr; s.terminal_obs = nullptr;
    s.flags = (s.flags & ~CH_STEP_RANDOM_ACTIONS) | CH_STEP_AUTORESET;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (!h->eval_host) HIP_TRY(h, hipHostMalloc(&h->eval_host, 2 * sizeof(long long), hipHostMallocDefault));
    long long* host = h->eval_host;   // [0] remaining, [1] the device error word (an int in its low half)
    *steps_run = 0;
    *remaining = -1;   // not read yet
    bool recorded = true;   // the last step's rewards and episodes are in the table (*step_index: that step)
    for (int64_t t = 0; t < max_steps;) {
        if (int rc = ch_policy_forward(h, policy, s.obs, policy_out, stream)) return rc;
        if (int rc = actions(recorded)) return rc;
        if (int rc = ch_step(h, &s, stream)) return rc;
        *step_index = (int)(first_step_index + t);
        recorded = false;
        *steps_run = ++t;
        if (t % check_every == 0 || t == max_steps) {
            if (int rc = record()) return rc;
            recorded = true;
            host[1] = 0;
            HIP_TRY(h, hipMemcpyAsync(&host[0], remaining_dev, sizeof(long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipMemcpyAsync(&host[1], h->errw, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            *remaining = host[0];
            int word = 0;
            std::memcpy(&word, &host[1], sizeof(int));
            if (word) return device_status(h, word);
            if (host[0] == 0) break;
        }
    }
    return CH_OK;
}

extern "C" {

int ch_eval_begin(ch_handle* h, const ch_eval_table* table, int32_t n_eval_episodes, void* stream) {
    EvalArgs a;
    if (int rc = table_args(h, table, a, "ch_eval_begin")) return rc;
    if (int rc = begin_args(h, n_eval_episodes, table->capacity, "ch_eval_begin")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_eval_begin(a, n_eval_episodes, (hipStream_t)stream));
    return CH_OK;
}

int ch_eval_record(ch_handle* h, const ch_eval_table* table, const ch_step_io* io, int64_t step_index, void* stream) {
    EvalArgs a;
    if (int rc = table_args(h, table, a, "ch_eval_record")) return rc;
    if (int rc = record_args(h, io, step_index, a, "ch_eval_record")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_eval_record(a, (hipStream_t)stream));
    return CH_OK;
}

int ch_evaluate_policy(ch_handle* h, const ch_mlp* actor, const ch_eval_table* table, const ch_eval_io* io,
                       int64_t max_steps, int32_t check_every, int64_t first_step_index,
                       int64_t* steps_run, int64_t* remaining, void* stream) {
    const char* who = "ch_evaluate_policy";
    if (int rc = loop_bounds(h, max_steps, check_every, who)) return rc;
    EvalArgs a;
    if (int rc = table_args(h, table, a, who)) return rc;
    if (int rc = loop_args(h, actor && io && io->step && io->mean && io->env_actions && steps_run && remaining, max_steps,
                           first_step_index, who))
        return rc;
    if (int rc = record_args(h, io->step, first_step_index, a, who)) return rc;
    if (actor->n_layers < 1 || actor->n_layers > 4)
        return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: n_layers must be 1..4");
    // the env reads a (num_drones, 4) action per env: the first num_drones * 4 outputs of the actor (SB3: Box((NUM_DRONES,
    // 4)) or the reference's (12, 4))
    const int out_w = actor->dims[actor->n_layers], act_w = h->NC * 4;
    if (out_w < act_w)
        return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: the actor's output (" + std::to_string(out_w) +
                                           " wide) must be at least num_drones * 4 = " + std::to_string(act_w) + " wide");
    hipStream_t st = (hipStream_t)stream;
    return evaluate_loop(
        h, actor, io->mean, io->step, io->env_actions, max_steps, check_every, first_step_index, &a.step_index,
        a.remaining, steps_run, remaining, stream,
        [&](bool recorded) {
            HIP_TRY(h, launch_eval_actions(io->mean, out_w, act_w, h->E, io->env_actions, recorded ? nullptr : &a, st));
            return (int)CH_OK;
        },
        [&] { HIP_TRY(h, launch_eval_record(a, st)); return (int)CH_OK; });
}

int ch_marl_eval_begin(ch_handle* h, const ch_marl_eval_table* table, int32_t n_eval_episodes, void* stream) {
    MarlEvalArgs a;
    if (int rc = table_args(h, table, a, "ch_marl_eval_begin")) return rc;
    if (int rc = begin_args(h, n_eval_episodes, table->capacity, "ch_marl_eval_begin")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_marl_eval_begin(a, n_eval_episodes, (hipStream_t)stream));
    return CH_OK;
}

int ch_marl_eval_mark(ch_handle* h, const ch_marl_eval_table* table, void* stream) {
    MarlEvalArgs a;
    if (int rc = table_args(h, table, a, "ch_marl_eval_mark")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_marl_eval_mark(a, (hipStream_t)stream));
    return CH_OK;
}

int ch_marl_eval_record(ch_handle* h, const ch_marl_eval_table* table, const ch_step_io* io, int64_t step_index,
                        void* stream) {
    MarlEvalArgs a;
    if (int rc = table_args(h, table, a, "ch_marl_eval_record")) return rc;
    if (int rc = record_args(h, io, step_index, a, "ch_marl_eval_record")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_marl_eval_record(a, (hipStream_t)stream));
    return CH_OK;
}

int ch_marl_evaluate_policy(ch_handle* h, const ch_mlp* policy, const ch_marl_eval_table* table,
                            const ch_marl_eval_io* io, int64_t max_steps, int32_t check_every, int64_t first_step_index,
                            int64_t* steps_run, int64_t* remaining, void* stream) {
    const char* who = "ch_marl_evaluate_policy";
    if (int rc = loop_bounds(h, max_steps, check_every, who)) return rc;
    MarlEvalArgs a;
    if (int rc = table_args(h, table, a, who)) return rc;
    if (int rc = loop_args(h, policy && io && io->step && io->policy_out && io->env_actions && steps_run && remaining,
                           max_steps, first_step_index, who))
        return rc;
    if (int rc = record_args(h, io->step, first_step_index, a, who)) return rc;
    if (policy->n_layers < 1 || policy->n_layers > 4)
        return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: n_layers must be 1..4");
    // the env reads one VEL action of 4 floats per agent: the first 4 outputs of the agent's row (the DiagGaussian's
    // mean half when the policy outputs mean then log_std)
    const int out_w = policy->dims[policy->n_layers];
    if (out_w < 4)
        return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: the policy's output (" + std::to_string(out_w) +
                                           " wide) must be at least 4 wide (one VEL action per agent)");
    hipStream_t st = (hipStream_t)stream;
    return evaluate_loop(
        h, policy, io->policy_out, io->step, io->env_actions, max_steps, check_every, first_step_index, &a.step_index,
        a.remaining, steps_run, remaining, stream,
        [&](bool recorded) {
            HIP_TRY(h, launch_marl_eval_actions(io->policy_out, out_w, io->env_actions, a, !recorded, st));
            return (int)CH_OK;
        },
        [&] { HIP_TRY(h, launch_marl_eval_record(a, st)); return (int)CH_OK; });
}

}  // extern "C"
