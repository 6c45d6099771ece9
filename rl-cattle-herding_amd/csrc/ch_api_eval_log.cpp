// ch_api_eval_log.cpp — the evaluator-log part of the C ABI (see include/cattleherd.h): the device table of
// update_evaluation_metrics' per-step rows (ch_eval_log_begin, ch_eval_log_mark, ch_eval_log_record; kernels in
// ch_eval_log.hip) and the playback loop around ch_policy_forward, ch_step and ch_reset that fills it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ch_handle.h"

using namespace ch;

// the checks every entry point shares: a CTDE handle with the distance accumulator, and a whole table
static int log_args(ch_handle* h, const ch_eval_log* lg, EvalLogArgs& a, const char* who) {
    if (!lg) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL log");
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
    if (h->cfg.mode != CH_MODE_CTDE)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the evaluator log is for CTDE handles");
    if (!h->evald)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the handle was created with eval_metrics = 0");
    if (lg->n_sel < 1 || lg->capacity < 1 || !lg->sel_env || !lg->rows || !lg->dropped || !lg->time ||
        !lg->effectiveness || !lg->num_drones || !lg->episode || !lg->flags || !lg->drone_xy || !lg->drone_vxy ||
        !lg->drone_dist || !lg->cattle_xy || !lg->cattle_vxy || !lg->start_cattle_vxy || !lg->start_counter)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": n_sel >= 1, capacity >= 1 and every log array are required");
    if ((reinterpret_cast<uintptr_t>(lg->drone_xy) | reinterpret_cast<uintptr_t>(lg->drone_vxy) |
         reinterpret_cast<uintptr_t>(lg->cattle_xy) | reinterpret_cast<uintptr_t>(lg->cattle_vxy) |
         reinterpret_cast<uintptr_t>(lg->start_cattle_vxy)) & 15)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the xy / vxy arrays must be 16-byte aligned");
    std::memset(&a, 0, sizeof(a));
    a.E = h->E; a.NC = h->NC; a.M = h->M; a.S = lg->n_sel; a.T = lg->capacity;
    a.ctrl_freq = h->cfg.ctrl_freq; a.episode_len = h->episode_len;
    a.drone = h->drone; a.cattle = h->cattle; a.pos64 = h->pos64; a.cpos64 = h->cpos64;
    a.envi = h->envi; a.evald = h->evald; a.err = h->errw;
    a.sel = lg->sel_env; a.rows = lg->rows; a.dropped = lg->dropped; a.time = lg->time; a.eff = lg->effectiveness;
    a.num_drones = lg->num_drones; a.episode = lg->episode; a.flags = lg->flags;
    a.drone_xy = lg->drone_xy; a.drone_vxy = lg->drone_vxy; a.drone_dist = lg->drone_dist;
    a.cattle_xy = lg->cattle_xy; a.cattle_vxy = lg->cattle_vxy;
    a.start_vxy = lg->start_cattle_vxy; a.start_counter = lg->start_counter;
    return CH_OK;
}

// the recorder's inputs: the outputs of the step that just ran, which must not have reset the envs it ended
static int record_args(ch_handle* h, const ch_step_io* io, EvalLogArgs& a, const char* who) {
    if (!io || !io->terminated || !io->truncated)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry terminated and truncated");
    if (io->flags & CH_STEP_AUTORESET)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io holds CH_STEP_AUTORESET: the recorder reads the "
                                           "post-step, pre-reset state, so the step before it must not auto-reset "
                                           "(reset the finished envs with a masked ch_reset afterwards)");
    a.term = io->terminated; a.trunc = io->truncated;
    return CH_OK;
}

static bool is_f32(const ch_handle* h) { return h->rsize != sizeof(double); }

extern "C" {

int ch_eval_log_begin(ch_handle* h, const ch_eval_log* log, void* stream) {
    EvalLogArgs a;
    if (int rc = log_args(h, log, a, "ch_eval_log_begin")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_eval_log_begin(a, (hipStream_t)stream));
    return CH_OK;
}

int ch_eval_log_mark(ch_handle* h, const ch_eval_log* log, void* stream) {
    EvalLogArgs a;
    if (int rc = log_args(h, log, a, "ch_eval_log_mark")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_eval_log_mark(a, is_f32(h), (hipStream_t)stream));
    return CH_OK;
}

int ch_eval_log_record(ch_handle* h, const ch_eval_log* log, const ch_step_io* io, void* stream) {
    EvalLogArgs a;
    if (int rc = log_args(h, log, a, "ch_eval_log_record")) return rc;
    if (int rc = record_args(h, io, a, "ch_eval_log_record")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_eval_log_record(a, is_f32(h), (hipStream_t)stream));
    return CH_OK;
}

int ch_eval_log_run(ch_handle* h, const ch_mlp* actor, const ch_eval_log* log, const ch_eval_log_io* io,
                    int64_t n_steps, void* stream) {
    if (n_steps < 1) return fail(h, CH_ERR_INVALID, "ch_eval_log_run: n_steps must be >= 1");
    EvalLogArgs a;
    if (int rc = log_args(h, log, a, "ch_eval_log_run")) return rc;
    if (!actor || !io || !io->step || !io->mean || !io->env_actions || !io->done_mask)
        return fail(h, CH_ERR_INVALID, "ch_eval_log_run: NULL argument");
    if (int rc = record_args(h, io->step, a, "ch_eval_log_run")) return rc;
    if (actor->n_layers < 1 || actor->n_layers > 4)
        return fail(h, CH_ERR_INVALID, "ch_eval_log_run: n_layers must be 1..4");
    // the env reads a (num_drones, 4) action per env: the first num_drones * 4 outputs of the actor, as ch_evaluate_policy
    const int out_w = actor->dims[actor->n_layers], act_w = h->NC * 4;
    if (out_w < act_w)
        return fail(h, CH_ERR_INVALID, "ch_eval_log_run: the actor's output (" + std::to_string(out_w) +
                                           " wide) must be at least num_drones * 4 = " + std::to_string(act_w) + " wide");
    ch_step_io s = *io->step;
    s.actions = io->env_actions; s.actions_out = nullptr; s.terminal_obs = nullptr;
    s.flags &= ~(uint32_t)CH_STEP_RANDOM_ACTIONS;
    a.done_mask = io->done_mask;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const bool f32 = is_f32(h);
    // every call returns on its first failure: nothing further is launched
    for (int64_t t = 0; t < n_steps; ++t) {
        if (int rc = ch_policy_forward(h, actor, s.obs, io->mean, stream)) return rc;
        HIP_TRY(h, launch_eval_actions(io->mean, out_w, act_w, h->E, io->env_actions, nullptr, st));
        HIP_TRY(h, launch_eval_log_mark(a, f32, st));
        if (int rc = ch_step(h, &s, stream)) return rc;
        HIP_TRY(h, launch_eval_log_record(a, f32, st));   // + done_mask of every env
        if (int rc = ch_reset(h, io->done_mask, s.obs, stream)) return rc;   // masked: asynchronous
    }
    return CH_OK;
}

}  // extern "C"
