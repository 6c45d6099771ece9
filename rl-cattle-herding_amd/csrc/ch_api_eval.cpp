// ch_api_eval.cpp — the evaluation part of the C ABI (see include/cattleherd.h): the device episode table (ch_eval_begin,
// ch_eval_record; kernels in ch_eval.hip) and the native evaluate_policy loop around ch_policy_forward and ch_step.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ch_handle.h"

using namespace ch;

// the checks every entry point shares: a CTDE handle and a whole table
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

// the recorder's inputs: the outputs of the step that just ran
static int record_args(ch_handle* h, const ch_step_io* io, int64_t step_index, EvalArgs& a, const char* who) {
    if (!io || !io->reset_happened || !io->episode_stats || !io->terminated || !io->truncated)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry reset_happened, episode_stats, "
                                                          "terminated and truncated");
    if (step_index < 0 || step_index > INT32_MAX)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": step_index outside [0, 2^31)");
    a.reset = io->reset_happened; a.stats = io->episode_stats; a.term = io->terminated; a.trunc = io->truncated;
    a.step_index = (int)step_index;
    return CH_OK;
}

extern "C" {

int ch_eval_begin(ch_handle* h, const ch_eval_table* table, int32_t n_eval_episodes, void* stream) {
    EvalArgs a;
    if (int rc = table_args(h, table, a, "ch_eval_begin")) return rc;
    if (n_eval_episodes < 1) return fail(h, CH_ERR_INVALID, "ch_eval_begin: n_eval_episodes must be >= 1");
    const int64_t per_env = (n_eval_episodes + h->E - 1) / h->E;   // the last env's quota
    if (per_env > table->capacity)
        return fail(h, CH_ERR_INVALID, "ch_eval_begin: " + std::to_string(n_eval_episodes) + " episodes over " +
                                           std::to_string(h->E) + " envs need " + std::to_string(per_env) +
                                           " slots per env, the table's capacity is " + std::to_string(table->capacity));
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
    // the loop's bounds first: they do not depend on the handle
    if (max_steps < 1) return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: max_steps must be >= 1 (the loop is always bounded)");
    if (check_every < 1) return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: check_every must be >= 1");
    EvalArgs a;
    if (int rc = table_args(h, table, a, "ch_evaluate_policy")) return rc;
    if (!actor || !io || !io->step || !io->mean || !io->env_actions || !steps_run || !remaining)
        return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: NULL argument");
    if (first_step_index < 0 || first_step_index > INT32_MAX - max_steps)
        return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: first_step_index + max_steps outside [0, 2^31)");
    if (int rc = record_args(h, io->step, first_step_index, a, "ch_evaluate_policy")) return rc;
    if (actor->n_layers < 1 || actor->n_layers > 4)
        return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: n_layers must be 1..4");
    // the env reads a (num_drones, 4) action per env: the first num_drones * 4 outputs of the actor (SB3: Box((NUM_DRONES,
    // 4)) or the reference's (12, 4))
    const int out_w = actor->dims[actor->n_layers], act_w = h->NC * 4;
    if (out_w < act_w)
        return fail(h, CH_ERR_INVALID, "ch_evaluate_policy: the actor's output (" + std::to_string(out_w) +
                                           " wide) must be at least num_drones * 4 = " + std::to_string(act_w) + " wide");
    ch_step_io s = *io->step;
    s.actions = io->env_actions; s.actions_out = nullptr; s.terminal_obs = nullptr;
    s.flags = (s.flags & ~CH_STEP_RANDOM_ACTIONS) | CH_STEP_AUTORESET;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (!h->eval_host) HIP_TRY(h, hipHostMalloc(&h->eval_host, 2 * sizeof(long long), hipHostMallocDefault));
    long long* host = h->eval_host;   // [0] remaining, [1] the device error word (an int in its low half)
    *steps_run = 0;
    *remaining = -1;   // not read yet
    // The recorder of a step runs in the next step's action kernel (the step's outputs are still in place there: the
    // forward in between writes only io->mean), and as a launch of its own only before `remaining` is read: per step
    // that leaves the forward, the action kernel and the step.
    bool recorded = true;   // the last step's episodes are in the table (a.step_index: that step)
    for (int64_t t = 0; t < max_steps;) {
        // SB3 evaluate_policy, one step of every env: predict(obs, deterministic=True) -> env.step -> the episode lists
        if (int rc = ch_policy_forward(h, actor, s.obs, io->mean, stream)) return rc;
        HIP_TRY(h, launch_eval_actions(io->mean, out_w, act_w, h->E, io->env_actions, recorded ? nullptr : &a, st));
        if (int rc = ch_step(h, &s, stream)) return rc;
        a.step_index = (int)(first_step_index + t);
        recorded = false;
        *steps_run = ++t;
        if (t % check_every == 0 || t == max_steps) {
            HIP_TRY(h, launch_eval_record(a, st));
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
