// ch_api_marl_eval.cpp — the DTDE driver's evaluation part of the C ABI (see include/cattleherd.h): the per-agent
// episode table (ch_marl_eval_begin, ch_marl_eval_mark, ch_marl_eval_record; kernels in ch_marl_eval.hip) and the native
// evaluation loop around ch_policy_forward and ch_step, ch_evaluate_policy's (ch_api_eval.cpp) for a MARL handle.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ch_handle.h"

using namespace ch;

// the checks every entry point shares: a MARL handle under the wrapper's semantics and a whole table
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

// the recorder's inputs: the outputs of the step that just ran
static int record_args(ch_handle* h, const ch_step_io* io, int64_t step_index, MarlEvalArgs& a, const char* who) {
    if (!io || !io->reward || !io->reset_happened)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry reward and reset_happened");
    if (step_index < 0 || step_index > INT32_MAX)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": step_index outside [0, 2^31)");
    a.reward = io->reward; a.reset = io->reset_happened;
    a.step_index = (int)step_index;
    return CH_OK;
}

extern "C" {

int ch_marl_eval_begin(ch_handle* h, const ch_marl_eval_table* table, int32_t n_eval_episodes, void* stream) {
    MarlEvalArgs a;
    if (int rc = table_args(h, table, a, "ch_marl_eval_begin")) return rc;
    if (n_eval_episodes < 1) return fail(h, CH_ERR_INVALID, "ch_marl_eval_begin: n_eval_episodes must be >= 1");
    const int64_t per_env = (n_eval_episodes + h->E - 1) / h->E;   // the last env's quota
    if (per_env > table->capacity)
        return fail(h, CH_ERR_INVALID, "ch_marl_eval_begin: " + std::to_string(n_eval_episodes) + " episodes over " +
                                           std::to_string(h->E) + " envs need " + std::to_string(per_env) +
                                           " slots per env, the table's capacity is " + std::to_string(table->capacity));
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
    // the loop's bounds first: they do not depend on the handle
    if (max_steps < 1)
        return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: max_steps must be >= 1 (the loop is always bounded)");
    if (check_every < 1) return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: check_every must be >= 1");
    MarlEvalArgs a;
    if (int rc = table_args(h, table, a, "ch_marl_evaluate_policy")) return rc;
    if (!policy || !io || !io->step || !io->policy_out || !io->env_actions || !steps_run || !remaining)
        return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: NULL argument");
    if (first_step_index < 0 || first_step_index > INT32_MAX - max_steps)
        return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: first_step_index + max_steps outside [0, 2^31)");
    if (int rc = record_args(h, io->step, first_step_index, a, "ch_marl_evaluate_policy")) return rc;
    if (policy->n_layers < 1 || policy->n_layers > 4)
        return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: n_layers must be 1..4");
    // the env reads one VEL action of 4 floats per agent: the first 4 outputs of the agent's row (the DiagGaussian's
    // mean half when the policy outputs mean then log_std)
    const int out_w = policy->dims[policy->n_layers];
    if (out_w < 4)
        return fail(h, CH_ERR_INVALID, "ch_marl_evaluate_policy: the policy's output (" + std::to_string(out_w) +
                                           " wide) must be at least 4 wide (one VEL action per agent)");
    ch_step_io s = *io->step;
    s.actions = io->env_actions; s.actions_out = nullptr; s.terminal_obs = nullptr;
    s.flags = (s.flags & ~CH_STEP_RANDOM_ACTIONS) | CH_STEP_AUTORESET;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (!h->eval_host) HIP_TRY(h, hipHostMalloc(&h->eval_host, 2 * sizeof(long long), hipHostMallocDefault));
    long long* host = h->eval_host;   // [0] remaining, [1] the device error word (an int in its low half)
    *steps_run = 0;
    *remaining = -1;   // not read yet
    // As in ch_evaluate_policy, the recorder of a step runs in the next step's action kernel (the step's outputs are
    // still in place there: the forward in between writes only io->policy_out), and as a launch of its own only before
    // `remaining` is read: per step that leaves the forward, the action kernel and the step.
    bool recorded = true;   // the last step's rewards and episodes are in the table (a.step_index: that step)
    for (int64_t t = 0; t < max_steps;) {
        if (int rc = ch_policy_forward(h, policy, s.obs, io->policy_out, stream)) return rc;
        HIP_TRY(h, launch_marl_eval_actions(io->policy_out, out_w, io->env_actions, a, !recorded, st));
        if (int rc = ch_step(h, &s, stream)) return rc;
        a.step_index = (int)(first_step_index + t);
        recorded = false;
        *steps_run = ++t;
        if (t % check_every == 0 || t == max_steps) {
            HIP_TRY(h, launch_marl_eval_record(a, st));
            recorded = true;
            host[1] = 0;
            HIP_TRY(h, hipMemcpyAsync(&host[0], a.remaining, sizeof(long long), hipMemcpyDeviceToHost, st));
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

}  // extern "C"
