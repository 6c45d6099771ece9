// ch_api_norm.cpp — the device-side VecNormalize's part of the C ABI (see include/cattleherd.h ch_norm_*): the running
// observation and return statistics (kernels in ch_norm.hip) and ch_rollout_collect_norm, the CTDE collection with a
// normaliser.  The collection is a loop over public entry points only (ch_mlp_forward, ch_rollout_store, ch_step,
// ch_ep_ring_record's launch, ch_norm_*, ch_mlp_forward_masked, ch_rollout_post, ch_rollout_gae): the same launches
// cattleherd.rollout.DeviceRolloutBuffer.collect_steps(normalizer=...) makes from Python, so the two agree bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "ch_handle.h"
#include "ch_norm.h"

using namespace ch;

// the normaliser's own checks (no handle: failures go to ch_last_error(NULL))
static int norm_ok(const ch_norm* n, const char* who) {
    if (!n) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL normaliser");
    if (n->dim < 1 || n->dim > (1 << 24)) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": dim must be in [1, 2^24]");
    if (n->n_envs < 1) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": n_envs < 1");
    if (!n->mean || !n->var || !n->count || !n->ret_stats || !n->ret || !n->scratch)
        return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": every statistic array and the scratch are required");
    if (!(n->clip_obs >= 0.0) || !(n->clip_reward >= 0.0))
        return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": clip_obs and clip_reward must be >= 0");
    if (!(n->epsilon >= 0.0)) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": epsilon must be >= 0");
    return CH_OK;
}

static int obs_args(const ch_norm* n, const float* x, int64_t rows, NormObsArgs& a, const char* who) {
    if (int rc = norm_ok(n, who)) return rc;
    if (!x) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL matrix");
    if (rows < 1 || rows > (1LL << 24)) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": rows must be in [1, 2^24]");
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.rows = rows; a.dim = n->dim;
    a.mean = n->mean; a.var = n->var; a.count = n->count; a.scratch = n->scratch;
    a.clip = n->clip_obs; a.eps = n->epsilon;
    return CH_OK;
}

static int launched(const char* who, hipError_t e) {
    return e == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, std::string(who) + " launch: " + hipGetErrorString(e));
}

extern "C" {

int64_t ch_norm_scratch_size(int64_t rows, int32_t dim) {
    if (rows < 1 || rows > (1LL << 24) || dim < 1 || dim > (1 << 24)) {
        fail(nullptr, CH_ERR_INVALID, "ch_norm_scratch_size: rows and dim must be in [1, 2^24]");
        return -1;
    }
    return std::max(norm_obs_scratch(rows, dim), norm_reward_scratch(rows));
}

int ch_norm_begin(const ch_norm* norm, void* stream) {
    if (int rc = norm_ok(norm, "ch_norm_begin")) return rc;
    NormBeginArgs a{norm->dim, norm->n_envs, norm->mean, norm->var, norm->count, norm->ret_stats, norm->ret};
    return launched("ch_norm_begin", launch_norm_begin(a, (hipStream_t)stream));
}

int ch_norm_obs_update(const ch_norm* norm, const float* x, int64_t rows, void* stream) {
    NormObsArgs a;
    if (int rc = obs_args(norm, x, rows, a, "ch_norm_obs_update")) return rc;
    if (norm->scratch_doubles < norm_obs_scratch(rows, norm->dim))
        return fail(nullptr, CH_ERR_INVALID, "ch_norm_obs_update: the scratch is smaller than ch_norm_scratch_size(rows, dim)");
    if (!norm->training || !norm->norm_obs) return CH_OK;   // VecNormalize: the statistics move only while training
    a.y = const_cast<float*>(x);   // (not written: the alignment test of the float4 path looks at both)
    a.chunk_rows = norm_chunk_rows(rows); a.chunks = norm_chunks(rows);
    return launched("ch_norm_obs_update", launch_norm_obs_update(a, (hipStream_t)stream));
}

int ch_norm_obs_apply(const ch_norm* norm, const float* x, int64_t rows, const uint8_t* row_mask, float* y, void* stream) {
    NormObsArgs a;
    if (int rc = obs_args(norm, x, rows, a, "ch_norm_obs_apply")) return rc;
    if (!y) return fail(nullptr, CH_ERR_INVALID, "ch_norm_obs_apply: NULL output");
    a.y = y; a.row_mask = row_mask; a.passthrough = !norm->norm_obs;
    if (a.passthrough && x == y) return CH_OK;
    return launched("ch_norm_obs_apply", launch_norm_obs_apply(a, (hipStream_t)stream));
}

int ch_norm_reward(const ch_norm* norm, const float* reward, const uint8_t* terminated, const uint8_t* truncated,
                   int64_t n_envs, float* reward_out, void* stream) {
    if (int rc = norm_ok(norm, "ch_norm_reward")) return rc;
    if (!reward || !terminated || !truncated || !reward_out) return fail(nullptr, CH_ERR_INVALID, "ch_norm_reward: NULL array");
    if (n_envs != norm->n_envs) return fail(nullptr, CH_ERR_INVALID, "ch_norm_reward: n_envs is not the normaliser's");
    if (n_envs > (1LL << 24)) return fail(nullptr, CH_ERR_UNSUPPORTED, "ch_norm_reward: more than 2^24 envs");
    if (reward == reward_out) return fail(nullptr, CH_ERR_INVALID, "ch_norm_reward: the raw reward stays where it is (reward_out must be another buffer)");
    if (norm->scratch_doubles < norm_reward_scratch(n_envs))
        return fail(nullptr, CH_ERR_INVALID, "ch_norm_reward: the scratch is smaller than ch_norm_scratch_size(n_envs, dim)");
    NormRewardArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = n_envs; a.reward = reward; a.terminated = terminated; a.truncated = truncated; a.reward_out = reward_out;
    a.ret = norm->ret; a.stats = norm->ret_stats; a.scratch = norm->scratch;
    a.gamma = norm->gamma; a.clip = norm->clip_reward; a.eps = norm->epsilon;
    a.training = norm->training != 0; a.norm_reward = norm->norm_reward != 0; a.chunks = reward_chunks(n_envs);
    return launched("ch_norm_reward", launch_norm_reward(a, (hipStream_t)stream));
}

int ch_rollout_collect_norm(ch_handle* h, const ch_rollout* rb, const ch_rollout_io* io, const ch_mlp* actor,
                            const ch_mlp* critic, const float* log_std, uint64_t seed, float gamma, float gae_lambda,
                            int32_t bootstrap_truncated, const ch_ep_ring* ring, const ch_norm* norm, void* stream) {
    const char* who = "ch_rollout_collect_norm";
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
    if (h->cfg.mode != CH_MODE_CTDE)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the normalised collection is for CTDE handles");
    if (!norm) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL normaliser (ch_rollout_collect is the collection without one)");
    // the normaliser's own failures are reported on the handle too
    if (int rc = norm_ok(norm, who)) return fail(h, rc, ch_last_error(nullptr));
    if (norm->dim != h->rows * 86)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the normaliser's dim must be obs_rows * 86 = " + std::to_string(h->rows * 86));
    if (norm->n_envs != h->E) return fail(h, CH_ERR_INVALID, std::string(who) + ": the normaliser's n_envs is not the handle's");
    if (!norm->obs_n || !norm->terminal_obs_n || !norm->reward_n)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the normaliser's obs_n, terminal_obs_n and reward_n buffers are required");
    if (!rb) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL rollout buffer");
    if (!io || !io->step || !io->mean || !io->value || !io->env_actions || !log_std || !actor)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL argument");
    if (!critic)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": a fused actor-critic is not taken here (pass the actor and the critic)");
    const ch_step_io* sio = io->step;
    if (!sio->obs || !sio->reward || !sio->terminated || !sio->truncated || !sio->terminal_obs || !sio->reset_happened ||
        (bootstrap_truncated && !io->terminal_value))
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the step buffers (obs, reward, terminated, truncated, "
                                                         "terminal_obs, reset_happened) and terminal_value are required");
    if (actor->dims[0] != norm->dim || critic->dims[0] != norm->dim)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": dims[0] of the actor and the critic must be " + std::to_string(norm->dim));
    if (actor->dims[actor->n_layers < 1 || actor->n_layers > 4 ? 0 : actor->n_layers] != rb->act_dim ||
        critic->dims[critic->n_layers < 1 || critic->n_layers > 4 ? 0 : critic->n_layers] != 1)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": actor output must be act_dim wide, critic output 1");
    int rc;
    EpRingArgs er;
    if (ring && (rc = ep_ring_args(h, ring, sio, er, who))) return rc;
    const int64_t E = h->E;
    hipStream_t st = (hipStream_t)stream;
    ch_step_io s = *sio;   // the collections' step: the sampled env actions in, auto-reset on, no random actions
    s.actions = io->env_actions; s.actions_out = nullptr;
    s.flags = (s.flags & ~CH_STEP_RANDOM_ACTIONS) | CH_STEP_AUTORESET;
    // a failure of a handle-free call (forwards, normaliser) is reported on the handle
    auto on_handle = [&](int code) { return code ? fail(h, code, ch_last_error(nullptr)) : CH_OK; };
    HIP_TRY(h, hipSetDevice(h->device));
    // the observation the env holds, under the statistics as they stand (what reset_obs or the previous collection's
    // last step left in obs_n, formed again: the same bits)
    if ((rc = on_handle(ch_norm_obs_apply(norm, sio->obs, E, nullptr, norm->obs_n, stream)))) return rc;
    for (int32_t t = 0; t < rb->n_steps; ++t) {
        // dense forwards: a normalised feature past an env's NUM_DRONES is (0 - mean) / std, not zero
        if ((rc = on_handle(ch_mlp_forward(actor, norm->obs_n, E, io->mean, stream)))) return rc;
        if ((rc = on_handle(ch_mlp_forward(critic, norm->obs_n, E, io->value, stream)))) return rc;
        if ((rc = ch_rollout_store(h, rb, t, norm->obs_n, io->mean, io->value, log_std, seed, io->env_actions, stream))) return rc;
        if ((rc = ch_step(h, &s, stream))) return rc;
        if (ring) HIP_TRY(h, launch_ep_ring_record(er, st));   // the raw returns: Monitor sits under VecNormalize
        if ((rc = on_handle(ch_norm_obs_update(norm, sio->obs, E, stream)))) return rc;
        if ((rc = on_handle(ch_norm_obs_apply(norm, sio->obs, E, nullptr, norm->obs_n, stream)))) return rc;
        if (bootstrap_truncated) {
            if ((rc = on_handle(ch_norm_obs_apply(norm, sio->terminal_obs, E, sio->reset_happened, norm->terminal_obs_n, stream)))) return rc;
            if ((rc = on_handle(ch_mlp_forward_masked(critic, norm->terminal_obs_n, E, sio->reset_happened, io->terminal_value, stream)))) return rc;
        }
        if ((rc = on_handle(ch_norm_reward(norm, sio->reward, sio->terminated, sio->truncated, E, norm->reward_n, stream)))) return rc;
        if ((rc = ch_rollout_post(h, rb, t, norm->reward_n, sio->terminated, sio->truncated,
                                  bootstrap_truncated ? io->terminal_value : nullptr, gamma, stream))) return rc;
    }
    if ((rc = on_handle(ch_mlp_forward(critic, norm->obs_n, E, io->value, stream)))) return rc;
    return ch_rollout_gae(h, rb, io->value, gamma, gae_lambda, stream);
}

}  // extern "C"
