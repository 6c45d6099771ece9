// ch_api_policy.cpp — the policy half of the C ABI (see include/cattleherd.h): MLP packing and forwards on device
// buffers (ch_policy.hip), the on-device PPO rollout buffer and its collection loop, the population's collection
// (ch_rollout_collect_pop, ch_rollout_collect_pop_log), the per-agent MARL rollout (ch_aux.hip).  It reaches the env through ch_step and step_actor (ch_api.cpp) and a few fields of the handle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "ch_handle.h"

using namespace ch;

static int launch_or_fail(ch_handle* h, const char* who, hipError_t e) {
    if (e != hipSuccess) return fail(h, CH_ERR_DEVICE, std::string(who) + " launch: " + hipGetErrorString(e));
    return CH_OK;
}

static int mlp_args(const ch_mlp* net, const float* x, int64_t rows, float* y, MlpArgs& a, std::string& err) {
    if (!net || !x || !y) { err = "NULL argument"; return CH_ERR_INVALID; }
    if (net->n_layers < 1 || net->n_layers > 4) { err = "n_layers must be 1..4"; return CH_ERR_INVALID; }
    if (rows < 0) { err = "rows < 0"; return CH_ERR_INVALID; }
    std::memset(&a, 0, sizeof(a));
    a.layers = net->n_layers;
    for (int i = 0; i <= net->n_layers; ++i) {
        a.dims[i] = net->dims[i];
        if (net->dims[i] < 1 || (i > 0 && net->dims[i] > 256)) { err = "layer widths must be 1..256"; return CH_ERR_UNSUPPORTED; }
    }
    for (int i = 0; i < net->n_layers; ++i) {
        if (!net->weight[i]) { err = "NULL weight"; return CH_ERR_INVALID; }
        a.w[i] = net->weight[i]; a.b[i] = net->bias[i];
    }
    if (net->hidden_act < CH_ACT_NONE || net->hidden_act > CH_ACT_RELU) { err = "unknown activation"; return CH_ERR_INVALID; }
    a.hidden_act = net->hidden_act; a.clip = net->clip != 0; a.lo = net->lo; a.hi = net->hi;
    a.x = x; a.rows = rows; a.y = y; a.rows_per_env = 1;
    a.kcap = net->dims[0];
    // float4 weight loads need 16-B aligned rows of a multiple of 8 floats (k_mlp2 reads 8 per lane), inputs 4
    for (int i = 0; i < net->n_layers; ++i)
        if (net->dims[i] % 8 == 0 && (reinterpret_cast<uintptr_t>(net->weight[i]) & 15) == 0) a.vec_w |= 1 << i;
    if (net->dims[0] % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) a.vec_w |= 1 << 7;
    // block-diagonal layers the kernel can skip by whole K-pair groups (ch_mlp.split_*); others run dense
    for (int i = 1; i < net->n_layers; ++i) {
        const int so = net->split_out[i], si = net->split_in[i];
        if (so > 0 && so < net->dims[i + 1] && so % 32 == 0 && si > 0 && si < net->dims[i] && si % 128 == 0) {
            a.split_out[i] = so; a.split_in[i] = si;
        }
    }
    if (net->packed) {
        if (reinterpret_cast<uintptr_t>(net->packed) & 15) { err = "packed weights must be 16-byte aligned"; return CH_ERR_INVALID; }
        a.packed = net->packed;
        mlp_packed_floats(a.layers, a.dims, a.pk_off, a.pk_pairs);
    }
    return CH_OK;
}

// the forward of `net` on a handle's observation buffer: one row per env (CTDE) or agent (MARL), live widths from
// NUM_DRONES (envi row 0)
static int policy_args(ch_handle* h, const ch_mlp* net, const float* obs, float* y, MlpArgs& a, const char* who) {
    const bool marl = h->cfg.mode == CH_MODE_MARL;
    const int64_t rows = marl ? h->E * h->NC : h->E;
    const int want = marl ? 86 : h->rows * 86;
    if (net && net->dims[0] != want)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": dims[0] must be " + std::to_string(want) + " for this handle");
    std::string err;
    const int rc = mlp_args(net, obs, rows, y, a, err);
    if (rc) return fail(h, rc, std::string(who) + ": " + err);
    a.env_n = h->envi;   // envi row 0: NUM_DRONES of the episode each env is in
    a.rows_per_env = marl ? h->NC : 1;
    a.k_unit = 86;
    a.kcap = std::min(a.dims[0], marl ? 86 : h->NC * 86);   // NUM_DRONES <= the constructor's drones
    return CH_OK;
}

// the step both collections run: the caller's io with the sampled env actions in, auto-reset on, no random actions
static ch_step_io collect_step_io(const ch_step_io* sio, const float* env_actions) {
    ch_step_io s = *sio;
    s.actions = env_actions; s.actions_out = nullptr;
    s.flags = (s.flags & ~CH_STEP_RANDOM_ACTIONS) | CH_STEP_AUTORESET;
    return s;
}

static int rollout_args(ch_handle* h, const ch_rollout* rb, RolloutArgs& a, const char* who) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
    if (!rb) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL rollout buffer");
    if (h->cfg.mode != CH_MODE_CTDE)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the SB3 rollout buffer is for CTDE handles");
    // the env reads a (num_drones, 4) action per env (ch_step: float4 [e * num_drones + k]), so the policy must
    // produce at least num_drones * 4 outputs (SB3: Box((NUM_DRONES, 4)) or the reference's (12, 4))
    if (rb->n_steps < 1 || rb->act_dim < h->NC * 4 || rb->act_dim > 256)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": n_steps >= 1 and num_drones * 4 = " +
                                           std::to_string(h->NC * 4) + " <= act_dim <= 256 required");
    std::memset(&a, 0, sizeof(a));
    a.T = rb->n_steps; a.rows = h->E; a.obs_dim = h->rows * 86; a.act_dim = rb->act_dim;
    a.env_act_dim = h->NC * 4;
    a.mean_ld = rb->act_dim; a.value_ld = 1; a.tv_ld = 1; a.post_prev = 0;
    a.obs = rb->obs; a.actions = rb->actions; a.rewards = rb->rewards; a.episode_starts = rb->episode_starts;
    a.values = rb->values; a.log_probs = rb->log_probs; a.advantages = rb->advantages; a.returns = rb->returns;
    a.last_episode_starts = rb->last_episode_starts;
    return CH_OK;
}

// a device buffer of at least `want` bytes (contents not kept): freed and allocated again when it is smaller
static int grow(ch_handle* h, void** p, size_t* have, size_t want) {
    if (*have >= want) return CH_OK;
    if (*p) HIP_TRY(h, hipFree(*p));
    *p = nullptr;
    *have = 0;
    HIP_TRY(h, hipMalloc(p, want));
    *have = want;
    return CH_OK;
}

extern "C" {

// diagnostics: k_mlp2 writes wave 0's phase clocks of every workgroup to dev[blockIdx][16] (NULL: off); the fused
// step + actor kernel (k_step2_actor) writes its forward's clocks and wall-clock slots 13-15 to rows [grid, 2 grid),
// so a buffer for a collection on the fused path holds 2 x 16 x (E / 16) entries (tools/fused_probe.py trace)
int ch__set_mlp_tstamp(long long* dev) {
    g_mlp_tstamp = dev;
    return CH_OK;
}

/* Internal (tests / diagnostics): the forward kernel the last ch_mlp_forward / ch_policy_forward / collection launch
 * ran (launch_mlp_multi's record; host side): out = {kernel, row tiles per workgroup, grid, dynamic LDS bytes}.
 * kernel: the row of the kernel table (ch_mlp_plan.h kMlpTable, MlpKernel; ch__mlp_kernel gives a row's name and
 * columns), 0 = nothing launched (no rows). */
int ch__mlp_last_launch(int32_t out[4]) {
    if (!out) return CH_ERR_INVALID;
    out[0] = g_mlp_last_launch.kernel; out[1] = g_mlp_last_launch.rt;
    out[2] = g_mlp_last_launch.grid; out[3] = g_mlp_last_launch.lds;
    return CH_OK;
}

/* Internal (tests / diagnostics): launches of each forward kernel since the library was loaded, indexed by
 * ch__mlp_last_launch's kernel number (11 counters) -- a collection launches several; a test takes the difference. */
int ch__mlp_launch_counts(int64_t out[11]) {
    if (!out) return CH_ERR_INVALID;
    for (int i = 0; i < kMlpKernels; ++i) out[i] = g_mlp_launches[i];
    return CH_OK;
}

/* Internal (tests / diagnostics): row `kernel` of the kernel table: its name (NULL past the table) and, if `out` is
 * given, {family (2 k_mlp2, 1 k_mlp, 0 none), NW, TW, SHARE, RT, packed weights only, the most first-layer K pairs it
 * stages, takes raw weights with ragged hidden widths}. */
const char* ch__mlp_kernel(int32_t kernel, int32_t out[8]) {
    if (kernel < 0 || kernel >= kMlpKernels) return nullptr;
    const MlpKernelInfo& k = kMlpTable[kernel];
    const int32_t v[8] = {k.family, k.nw, k.tw, k.share, k.rt, k.packed_only, k.max_pair0, k.raw_ragged};
    if (out) std::copy(v, v + 8, out);
    return k.name;
}

/* Internal (tests / diagnostics): what launch_mlp_multi would launch for up to three nets -- mlp_plan on the host, no
 * device touched.  rows[s]: segment s's row count; kcap (optional) its live input width, 0 = dims[0]; cus: the CU
 * count to plan for; then the four switches the library otherwise reads from the environment (CH_MLP_V1,
 * CH_MLP2_NW4, CH_MLP_WIDE4, CH_MLP_RT).  out = {v2, rt, lda, ldh, lds bytes, live segments n, kernel[3], grid[3]}
 * (kernel and grid per live segment; v2: one launch of kernel[0] over the summed grid). */
int ch__mlp_plan(const ch_mlp* const* nets, const int64_t* rows, const int32_t* kcap, int32_t nseg, int32_t cus,
                 int32_t v1, int32_t nw4, int32_t wide4, int32_t rt, int32_t out[12]) {
    if (!nets || !rows || !out || nseg < 1 || nseg > 3 || cus < 1) return fail(nullptr, CH_ERR_INVALID, "ch__mlp_plan: bad argument");
    MlpArgs segs[3];
    float one = 0.0f;
    for (int s = 0; s < nseg; ++s) {
        std::string err;
        const int rc = mlp_args(nets[s], &one, rows[s], &one, segs[s], err);
        if (rc) return fail(nullptr, rc, "ch__mlp_plan: " + err);
        if (kcap && kcap[s] > 0) segs[s].kcap = std::min(kcap[s], segs[s].dims[0]);
    }
    const MlpPlan p = mlp_plan(segs, nseg, cus, MlpSwitches{v1 != 0, nw4 != 0, wide4 != 0, rt});
    const int32_t v[12] = {p.v2, p.rt, p.lda, p.ldh, p.lds, p.n, p.kernel[0], p.kernel[1], p.kernel[2],
                           p.grid[0], p.grid[1], p.grid[2]};
    std::copy(v, v + 12, out);
    return CH_OK;
}

/* Internal (tests / diagnostics): ch_rollout_collect's path, bit 0 copy each step's observation into the buffer
 * (CH_ROLLOUT_COPY=1), bit 1 the stand-alone store kernel instead of the forward epilogues (CH_ROLLOUT_STORE_KERNEL=1),
 * bit 2 the actor forward fused into the step (CH_FUSED_ACTOR=1), bit 3 never fused. */
int ch__set_rollout_path(ch_handle* h, int32_t bits) {
    if (!h || bits < 0 || bits > 15) return CH_ERR_INVALID;
    h->ro.path = bits;
    return CH_OK;
}

/* Internal: the handle's current rollout path bits (ch__set_rollout_path), or -1 for a null handle. */
int ch__get_rollout_path(const ch_handle* h) { return h ? h->ro.path : -1; }

/* Internal (tests): steps ch_rollout_collect has launched as the fused step + actor kernel on this handle. */
int64_t ch__rollout_fused_steps(const ch_handle* h) { return h ? (int64_t)h->ro.fused_steps : -1; }

int64_t ch_mlp_packed_size(const ch_mlp* net) {
    if (!net || net->n_layers < 1 || net->n_layers > 4) return -1;
    for (int i = 0; i <= net->n_layers; ++i)
        if (net->dims[i] < 1 || (i > 0 && net->dims[i] > 256)) return -1;
    return mlp_packed_floats(net->n_layers, net->dims, nullptr, nullptr);
}

int ch_mlp_pack(const ch_mlp* net, float* dst, void* stream) {
    MlpArgs a;
    std::string err;
    float one = 0.0f;
    const int rc = mlp_args(net, &one, 0, &one, a, err);
    if (rc) return fail(nullptr, rc, "ch_mlp_pack: " + err);
    if (!dst || (reinterpret_cast<uintptr_t>(dst) & 15)) return fail(nullptr, CH_ERR_INVALID, "ch_mlp_pack: dst NULL or not 16-byte aligned");
    return launch_or_fail(nullptr, "ch_mlp_pack", launch_mlp_pack(a, dst, (hipStream_t)stream));
}

int ch_mlp_forward(const ch_mlp* net, const float* x, int64_t rows, float* y, void* stream) {
    MlpArgs a;
    std::string err;
    const int rc = mlp_args(net, x, rows, y, a, err);
    if (rc) return fail(nullptr, rc, "ch_mlp_forward: " + err);
    return launch_or_fail(nullptr, "ch_mlp_forward", launch_mlp(a, (hipStream_t)stream));
}

int ch_mlp_forward_masked(const ch_mlp* net, const float* x, int64_t rows, const uint8_t* row_mask, float* y,
                          void* stream) {
    MlpArgs a;
    std::string err;
    const int rc = mlp_args(net, x, rows, y, a, err);
    if (rc) return fail(nullptr, rc, "ch_mlp_forward_masked: " + err);
    if (!row_mask) return fail(nullptr, CH_ERR_INVALID, "ch_mlp_forward_masked: NULL row mask");
    a.row_mask = row_mask;
    return launch_or_fail(nullptr, "ch_mlp_forward_masked", launch_mlp(a, (hipStream_t)stream));
}

int ch_policy_forward(ch_handle* h, const ch_mlp* net, const float* obs, float* y, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_policy_forward: NULL handle");
    MlpArgs a;
    const int rc = policy_args(h, net, obs, y, a, "ch_policy_forward");
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_or_fail(h, "ch_policy_forward", launch_mlp(a, (hipStream_t)stream));
}

int ch_rollout_store(ch_handle* h, const ch_rollout* rb, int32_t t, const float* obs, const float* mean,
                     const float* value, const float* log_std, uint64_t seed, float* env_actions, void* stream) {
    RolloutArgs a;
    int rc = rollout_args(h, rb, a, "ch_rollout_store");
    if (rc) return rc;
    if (t < 0 || t >= rb->n_steps) return fail(h, CH_ERR_INVALID, "ch_rollout_store: t outside [0, n_steps)");
    if (!obs || !mean || !value || !log_std || !env_actions || !rb->obs || !rb->actions || !rb->values ||
        !rb->log_probs || !rb->episode_starts || !rb->last_episode_starts)
        return fail(h, CH_ERR_INVALID, "ch_rollout_store: NULL buffer");
    if ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(rb->obs)) & 15)
        return fail(h, CH_ERR_INVALID, "ch_rollout_store: obs buffers must be 16-byte aligned");
    a.t = t; a.obs_now = obs; a.mean = mean; a.value = value; a.log_std = log_std; a.seed = seed;
    a.env_actions = env_actions; a.copy_obs = 1;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_rollout(a, 0, (hipStream_t)stream));
    return CH_OK;
}

int ch_rollout_post(ch_handle* h, const ch_rollout* rb, int32_t t, const float* reward, const uint8_t* terminated,
                    const uint8_t* truncated, const float* terminal_value, float gamma, void* stream) {
    RolloutArgs a;
    int rc = rollout_args(h, rb, a, "ch_rollout_post");
    if (rc) return rc;
    if (t < 0 || t >= rb->n_steps) return fail(h, CH_ERR_INVALID, "ch_rollout_post: t outside [0, n_steps)");
    if (!reward || !terminated || !truncated || !rb->rewards || !rb->last_episode_starts)
        return fail(h, CH_ERR_INVALID, "ch_rollout_post: NULL buffer");
    a.t = t; a.reward = reward; a.terminated = terminated; a.truncated = truncated; a.terminal_value = terminal_value;
    a.gamma = gamma;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_rollout(a, 1, (hipStream_t)stream));
    return CH_OK;
}

int ch_rollout_gae(ch_handle* h, const ch_rollout* rb, const float* last_value, float gamma, float gae_lambda,
                   void* stream) {
    RolloutArgs a;
    int rc = rollout_args(h, rb, a, "ch_rollout_gae");
    if (rc) return rc;
    if (!last_value || !rb->rewards || !rb->values || !rb->episode_starts || !rb->advantages || !rb->returns)
        return fail(h, CH_ERR_INVALID, "ch_rollout_gae: NULL buffer");
    a.value = last_value; a.gamma = gamma;
    a.gamma_lambda = (float)((double)gamma * (double)gae_lambda);   // SB3: float32(self.gamma * self.gae_lambda)
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_rollout(a, 2, (hipStream_t)stream));
    return CH_OK;
}

// ch_rollout_collect and ch_rollout_collect_log (`ring`: NULL, or the episode ring each step's ended episodes go to)
static int rollout_collect(ch_handle* h, const ch_rollout* rb, const ch_rollout_io* io, const ch_mlp* actor,
                           const ch_mlp* critic, const float* log_std, uint64_t seed, float gamma, float gae_lambda,
                           int32_t bootstrap_truncated, const ch_ep_ring* ring, void* stream) {
    RolloutArgs ra;
    int rc = rollout_args(h, rb, ra, "ch_rollout_collect");
    if (rc) return rc;
    if (!io || !io->step || !io->mean || !io->env_actions || !log_std || !actor || (critic && !io->value))
        return fail(h, CH_ERR_INVALID, "ch_rollout_collect: NULL argument");
    const ch_step_io* sio = io->step;
    if (!sio->obs || !sio->reward || !sio->terminated || !sio->truncated || !sio->terminal_obs || !sio->reset_happened ||
        (bootstrap_truncated && !io->terminal_value))
        return fail(h, CH_ERR_INVALID, "ch_rollout_collect: the step buffers (obs, reward, terminated, truncated, "
                                       "terminal_obs, reset_happened) and terminal_value are required");
    EpRingArgs er;   // the recorder's arguments: the ring and this io's reset_happened / episode_stats
    if (ring && (rc = ep_ring_args(h, ring, sio, er, "ch_rollout_collect_log"))) return rc;
    if (!rb->obs || !rb->actions || !rb->rewards || !rb->episode_starts || !rb->values || !rb->log_probs ||
        !rb->advantages || !rb->returns || !rb->last_episode_starts)
        return fail(h, CH_ERR_INVALID, "ch_rollout_collect: NULL rollout buffer array");
    if ((reinterpret_cast<uintptr_t>(sio->obs) | reinterpret_cast<uintptr_t>(rb->obs)) & 15)
        return fail(h, CH_ERR_INVALID, "ch_rollout_collect: obs buffers must be 16-byte aligned");
    // critic == NULL: `actor` is a fused actor-critic (both heads in one net, output act_dim + 1 wide: the action
    // mean, then the value); one forward per step reads the observation once.  io->mean is then its
    // [rows][act_dim + 1] output and io->terminal_value a [rows][act_dim + 1] one for the terminal observations.
    const bool fused = critic == nullptr;
    const int out_w = fused ? rb->act_dim + 1 : rb->act_dim;
    if (actor->dims[actor->n_layers] != out_w || (!fused && critic->dims[critic->n_layers] != 1))
        return fail(h, CH_ERR_INVALID, fused ? "ch_rollout_collect: a fused actor-critic's output must be act_dim + 1 wide"
                                             : "ch_rollout_collect: actor output must be act_dim wide, critic output 1");
    hipStream_t st = (hipStream_t)stream;
    const int32_t T = rb->n_steps;
    ch_step_io s = collect_step_io(sio, io->env_actions);
    const ch_mlp* vnet = fused ? actor : critic;
    float* value = fused ? io->mean + rb->act_dim : io->value;
    const float* tval = fused ? io->terminal_value + rb->act_dim : io->terminal_value;
    RolloutArgs a = ra;
    a.mean_ld = out_w; a.value_ld = fused ? out_w : 1; a.tv_ld = fused ? out_w : 1;
    // each step's post (reward + gamma V(terminal obs), next episode start) runs in the next step's store, the
    // last one in the GAE kernel: the step outputs and terminal values it reads are still that step's then
    a.post_prev = 1;
    a.reward = sio->reward; a.terminated = sio->terminated; a.truncated = sio->truncated;
    a.terminal_value = bootstrap_truncated ? tval : nullptr; a.gamma = gamma;
    a.obs_now = sio->obs; a.mean = io->mean; a.value = value; a.log_std = log_std; a.seed = seed;
    a.env_actions = io->env_actions;
    // The step writes its observations straight into the buffer's next slot (obs[t + 1]; the last step into the
    // env's own obs buffer): the obs of step t > 0 is already in place when it is stored, and only obs[0] is copied
    // (a v2 step into a buffer other than the one it wrote last writes every block in full, ch_step's obs_zero_ptr).
    // The actor and critic on obs[t] go out as one launch (launch_mlp_multi; their workgroups share the CUs,
    // so each forward's latencies hide behind the other's matrix work).  The truncation bootstrap is deferred: the
    // post of step t queues the terminal observations of the envs that were truncated and not terminated, and
    // every kTvEvery steps one forward over the queue gives their values, added to those rewards rows (the queue
    // holds at most kTvEvery * E rows).  Per step that leaves two launches with separate nets (forwards with the
    // store in their epilogues, step) and three with a fused net or CH_ROLLOUT_STORE_KERNEL=1 (forward, store, step).
    // (the period: 16 steps, fewer when the queue would pass 1 GiB -- one flush is a whole forward's latency, ~20 us
    // at configs[2]'s size, whatever the queue holds)
    const int kTvEvery = (int)std::min<long long>(16, std::max<long long>(1, (1LL << 30) / ((long long)h->E * ra.obs_dim * 4)));
    const bool copy_each = (h->ro.path & 1) != 0;
    const size_t slot = (size_t)h->E * (size_t)ra.obs_dim;
    auto obs_at = [&](int32_t t) { return (t == 0 || t == T || copy_each) ? sio->obs : rb->obs + (size_t)t * slot; };
    const int nnet = fused ? 1 : 2;
    MlpArgs segs[2], ftv;   // the actor (or the fused net) and the critic; V over the queue
    if ((rc = policy_args(h, actor, sio->obs, io->mean, segs[0], "ch_rollout_collect (actor)"))) return rc;
    if (!fused && (rc = policy_args(h, critic, sio->obs, io->value, segs[1], "ch_rollout_collect (critic)"))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const long long cap = (long long)h->E * kTvEvery;
    RolloutArgs ap = a;   // k_rollout_apply over the queue
    if (bootstrap_truncated) {
        ch_rollout_state& q = h->ro;
        if ((rc = grow(h, (void**)&q.tv_obs, &q.tv_obs_bytes, sizeof(float) * (size_t)cap * ra.obs_dim)) ||
            (rc = grow(h, (void**)&q.tv_row, &q.tv_row_bytes, sizeof(long long) * (size_t)cap)) ||
            (rc = grow(h, (void**)&q.tv_val, &q.tv_val_bytes, sizeof(float) * (size_t)cap * out_w)) ||
            (rc = grow(h, (void**)&q.tv_count, &q.tv_count_bytes, sizeof(int))))
            return rc;
        HIP_TRY(h, hipMemsetAsync(q.tv_count, 0, sizeof(int), st));
        // V(terminal obs) over the queue: whole (12, 86) blocks, zero past the constructor's drones
        std::string err;
        if ((rc = mlp_args(vnet, q.tv_obs, cap, q.tv_val, ftv, err))) return fail(h, rc, "ch_rollout_collect: " + err);
        ftv.rows_dev = q.tv_count;
        ftv.kcap = std::min(ftv.dims[0], h->NC * 86);
        a.defer = 1; a.term_obs = sio->terminal_obs; a.tv_obs = q.tv_obs; a.tv_count = q.tv_count; a.tv_row = q.tv_row;
        a.terminal_value = nullptr;
        ap = a;
        ap.rows = cap;
        ap.terminal_value = q.tv_val + (fused ? rb->act_dim : 0);
        ap.tv_ld = fused ? out_w : 1;   // the value net's output width
        ap.v_col = fused ? rb->act_dim : 0;
    }
    // the flush: V over the queue with the reward update in the forward's epilogue (kRoleTvApply), or (a net k_mlp2
    // does not take) the forward into tv_val and k_rollout_apply; then the queue is emptied
    const bool tv_epi = bootstrap_truncated && mlp_multi_fits(&ftv, 1) && !(h->ro.path & 2);
    auto flush = [&]() -> hipError_t {
        hipError_t e;
        if (tv_epi) {
            const int role = kRoleTvApply;
            e = launch_mlp_multi(&ftv, 1, st, &role, &ap);
        } else {
            e = launch_mlp_multi(&ftv, 1, st);
            if (e == hipSuccess) e = launch_rollout(ap, 3, st);
        }
        if (e == hipSuccess) e = hipMemsetAsync(h->ro.tv_count, 0, sizeof(int), st);
        return e;
    };
    // What the paths differ in.  epi: two separate nets k_mlp2 takes, and no store kernel asked for (path bit 1) --
    // the store is folded into the forwards' epilogues (the actor's samples its actions, log-probabilities and env
    // actions; the critic's writes the values, the previous step's post and the episode starts, and at t = 0 copies
    // obs[0]); otherwise the plain forwards are followed by k_rollout_store.  fuse (path bit 2: CH_FUSED_ACTOR=1 or
    // ch__set_rollout_path; bit 3 forbids it): the actor forward of step t + 1 runs in the step kernel of step t, in
    // the workgroup that wrote those observations (k_step2_actor), and the critic goes out alone: the same work in the
    // same stream order.
    const bool epi = !fused && !(h->ro.path & 2) && mlp_multi_fits(segs, 2);
    const bool fuse = epi && (h->ro.path & 4) && !(h->ro.path & 8) && step_actor(h, &s, st, segs[0], a, false) == hipSuccess;
    const int roles[2] = {kRoleSample, kRoleValue};
    RolloutArgs ro = a;
    for (int32_t t = 0; t < T; ++t) {
        // SB3 collect_rollouts, one step of every env: policy(obs) -> sample, log-prob, value -> env.step ->
        // bootstrap truncated rewards with V(terminal obs) -> buffer (OnPolicyAlgorithm.collect_rollouts)
        segs[0].x = segs[1].x = obs_at(t);
        ro.t = t;
        ro.copy_obs = t == 0 || copy_each;
        if (!epi) {
            HIP_TRY(h, launch_mlp_multi(segs, nnet, st));
            HIP_TRY(h, launch_rollout(ro, 0, st));   // (with the post of step t - 1)
        } else if (fuse && t > 0) {
            HIP_TRY(h, launch_mlp_multi(&segs[1], 1, st, &roles[1], &ro));   // the critic; step t - 1 ran the actor
        } else {
            HIP_TRY(h, launch_mlp_multi(segs, 2, st, roles, &ro));
        }
        if (bootstrap_truncated && t > 0 && t % kTvEvery == 0) HIP_TRY(h, flush());
        s.obs = (t + 1 < T && !copy_each) ? rb->obs + (size_t)(t + 1) * slot : sio->obs;
        if (fuse && t + 1 < T) {
            MlpArgs fa = segs[0];
            fa.x = obs_at(t + 1);   // = s.obs
            RolloutArgs rn = ro;
            rn.t = t + 1;
            const hipError_t e = step_actor(h, &s, st, fa, rn, true);
            if (e != hipSuccess) return fail(h, CH_ERR_DEVICE, std::string("ch_rollout_collect fused step: ") + hipGetErrorString(e));
        } else if ((rc = ch_step(h, &s, stream))) {
            return rc;
        }
        // The episode ring: step t's reset_happened / episode_stats are written by the launch above on every path
        // (the fused one runs step t's env step, then step t + 1's actor forward) and by nothing else before step
        // t + 1's env step: the forwards, the store, the flush and the post write the buffer, the queue and the
        // scratch outputs only.  So the recorder goes right here.
        if (ring) HIP_TRY(h, launch_ep_ring_record(er, st));
    }
    // The tail: the last step's post (and queue) with the last flush, V(obs after the last step) = GAE's last_value,
    // GAE.  The epilogue path posts before that forward, the others after it and only when bootstrapping -- without
    // the bootstrap their GAE kernel runs the last post itself.
    RolloutArgs pa = a;
    pa.t = T;
    pa.post_only = 1;
    auto last_post = [&]() -> int {
        HIP_TRY(h, launch_rollout(pa, 0, st));
        if (bootstrap_truncated) HIP_TRY(h, flush());
        return CH_OK;
    };
    if (epi && (rc = last_post())) return rc;
    MlpArgs fv = segs[nnet - 1];
    fv.x = obs_at(T);
    HIP_TRY(h, launch_mlp_multi(&fv, 1, st));
    if (!epi && bootstrap_truncated && (rc = last_post())) return rc;
    a.post_prev = !epi && !bootstrap_truncated;
    a.gamma_lambda = (float)((double)gamma * (double)gae_lambda);   // SB3: float32(self.gamma * self.gae_lambda)
    HIP_TRY(h, launch_rollout(a, 2, st));
    return CH_OK;
}

int ch_rollout_collect(ch_handle* h, const ch_rollout* rb, const ch_rollout_io* io, const ch_mlp* actor,
                       const ch_mlp* critic, const float* log_std, uint64_t seed, float gamma, float gae_lambda,
                       int32_t bootstrap_truncated, void* stream) {
    return rollout_collect(h, rb, io, actor, critic, log_std, seed, gamma, gae_lambda, bootstrap_truncated, nullptr, stream);
}

int ch_rollout_collect_log(ch_handle* h, const ch_rollout* rb, const ch_rollout_io* io, const ch_mlp* actor,
                           const ch_mlp* critic, const float* log_std, uint64_t seed, float gamma, float gae_lambda,
                           int32_t bootstrap_truncated, const ch_ep_ring* ring, void* stream) {
    return rollout_collect(h, rb, io, actor, critic, log_std, seed, gamma, gae_lambda, bootstrap_truncated, ring, stream);
}

}  // extern "C"

// ---- the population collection (ch_rollout_collect_pop) -------------------------------------------
namespace {
constexpr int kRoPopSlots = 2;   // staging and tables a call may fill while an earlier call's copy is still queued
enum { kRoPopStep = 0, kRoPopFlush, kRoPopLast, kRoPopKinds };   // one block of max_members entries per launch kind
}  // namespace

// The argument tables (see include/cattleherd.h).  A slot is one pinned host block and one device block of the same
// layout, [launch kind][max_members] PopMlp entries, and the event recorded behind the slot's latest copy.
struct ch_rollout_pop {
    int max_members = 0, device = 0;
    size_t bytes = 0;                 // of a slot
    size_t off[kRoPopKinds] = {};     // the blocks' places in it
    struct Slot { char* host = nullptr; char* dev = nullptr; hipEvent_t copied = nullptr; bool queued = false; } slot[kRoPopSlots];
    unsigned calls = 0;
};

namespace {

int ro_pop_free(ch_rollout_pop* pop) {
    hipError_t bad = hipSuccess;
    for (auto& s : pop->slot) {
        if (s.copied) {
            if (s.queued) (void)hipEventSynchronize(s.copied);
            if (hipError_t e = hipEventDestroy(s.copied)) bad = e;
        }
        if (s.dev) if (hipError_t e = hipFree(s.dev)) bad = e;
        if (s.host) if (hipError_t e = hipHostFree(s.host)) bad = e;
    }
    delete pop;
    return bad == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, std::string("ch_rollout_pop_destroy: ") + hipGetErrorString(bad));
}

// the device current while the object is made or freed, the caller's again afterwards
struct RoPopDevice {
    int prev = -1;
    hipError_t err;
    explicit RoPopDevice(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) err = hipSetDevice(device); else if (err == hipSuccess) prev = -1;
    }
    ~RoPopDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// ch_rollout_collect's flush period for a handle of E envs: 16 steps, fewer when the queue would pass 1 GiB
int ro_tv_every(long long E, int obs_dim) {
    return (int)std::min<long long>(16, std::max<long long>(1, (1LL << 30) / (E * obs_dim * 4)));
}

// Member p's slice of the handle-wide scratch of a population of P members on n_envs envs: its env count, its first
// env, and where its rows start in obs / terminal_obs, mean, the one-column arrays (value, terminal_value, reward,
// terminated, truncated), env_actions (elements) and in the deferred-bootstrap queue (rows; a member's share is the
// whole queue of a solo handle of E envs)
struct RoPopSlice { int64_t E, env, obs, mean, row, env_actions, queue; };
RoPopSlice ro_pop_slice(int64_t n_envs, int P, int p, int obs_dim, int num_drones, int act_dim) {
    RoPopSlice s;
    s.E = n_envs / P;
    s.env = s.E * p;
    s.obs = s.env * obs_dim;
    s.mean = s.env * act_dim;
    s.row = s.env;
    s.env_actions = s.env * num_drones * 4;
    s.queue = s.env * ro_tv_every(s.E, obs_dim);
    return s;
}

bool same_mlp_arch(const ch_mlp* a, const ch_mlp* b) {
    if (a->n_layers != b->n_layers || a->hidden_act != b->hidden_act || (a->clip != 0) != (b->clip != 0)) return false;
    if (a->clip && (a->lo != b->lo || a->hi != b->hi)) return false;
    if (a->n_layers < 1 || a->n_layers > 4) return true;   // (mlp_args refuses it by name)
    for (int i = 0; i <= a->n_layers; ++i)
        if (a->dims[i] != b->dims[i]) return false;
    for (int i = 0; i < a->n_layers; ++i)
        if (a->split_out[i] != b->split_out[i] || a->split_in[i] != b->split_in[i]) return false;
    return true;
}

bool same_mlp_plan(const MlpPlan& a, const MlpPlan& b) {
    return a.v2 == b.v2 && a.n == b.n && a.kernel[0] == b.kernel[0] && a.rt == b.rt && a.lda == b.lda && a.ldh == b.ldh &&
           a.lds == b.lds && a.start[1] == b.start[1] && a.start[2] == b.start[2];
}

}  // namespace

extern "C" {

int ch_rollout_pop_create(int32_t max_members, int32_t device, ch_rollout_pop** out) {
    const std::string w = "ch_rollout_pop_create: ";
    if (!out) return fail(nullptr, CH_ERR_INVALID, w + "NULL argument");
    *out = nullptr;
    if (max_members < 1 || max_members > 65535) return fail(nullptr, CH_ERR_INVALID, w + "max_members must be 1..65535");   // (a grid dimension)
    RoPopDevice scope(device);
    if (scope.err != hipSuccess) return fail(nullptr, CH_ERR_DEVICE, w + "device: " + hipGetErrorString(scope.err));
    ch_rollout_pop* pop = new ch_rollout_pop;
    pop->max_members = max_members; pop->device = device;
    for (int k = 0; k < kRoPopKinds; ++k) {
        pop->off[k] = pop->bytes;
        pop->bytes += (sizeof(PopMlp) * (size_t)max_members + 255) / 256 * 256;
    }
    for (auto& s : pop->slot) {
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&s.host), pop->bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s.dev), pop->bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)ro_pop_free(pop);
            return fail(nullptr, e == hipErrorOutOfMemory ? CH_ERR_NOMEM : CH_ERR_DEVICE, w + hipGetErrorString(e));
        }
    }
    *out = pop;
    return CH_OK;
}

int ch_rollout_pop_destroy(ch_rollout_pop* pop) {
    if (!pop) return fail(nullptr, CH_ERR_INVALID, "ch_rollout_pop_destroy: NULL argument");
    RoPopDevice scope(pop->device);
    return ro_pop_free(pop);
}

/* Internal (tests): where member p's slice starts in each handle-wide scratch array of a collection of n_members
 * members on n_envs envs of `obs_rows` observation rows and `num_drones` drones (host only): out = {envs per member,
 * obs / terminal_obs floats, mean floats, value / terminal_value / reward floats, env_actions floats, terminated /
 * truncated bytes, queue rows}.  The arithmetic ch_rollout_collect_pop uses. */
int ch__rollout_pop_slice(int64_t n_envs, int32_t n_members, int32_t p, int32_t obs_rows, int32_t num_drones,
                          int32_t act_dim, int64_t out[7]) {
    if (!out || n_envs < 1 || n_members < 1 || n_envs % n_members || p < 0 || p >= n_members || obs_rows < 1 ||
        num_drones < 1 || act_dim < 1)
        return fail(nullptr, CH_ERR_INVALID, "ch__rollout_pop_slice: bad argument");
    const RoPopSlice sl = ro_pop_slice(n_envs, n_members, p, obs_rows * 86, num_drones, act_dim);
    const int64_t v[7] = {sl.E, sl.obs, sl.mean, sl.row, sl.env_actions, sl.row, sl.queue};
    std::copy(v, v + 7, out);
    return CH_OK;
}

}  // extern "C"

// ch_rollout_collect_pop and ch_rollout_collect_pop_log (`ring`: NULL, or the members' episode rings each step's ended
// episodes go to)
static int rollout_collect_pop(ch_handle* h, ch_rollout_pop* pop, const ch_rollout_member* members, int32_t n_members,
                               const ch_rollout_io* io, int32_t bootstrap_truncated, const ch_ep_ring_pop* ring,
                               void* stream) {
    const std::string w = "ch_rollout_collect_pop: ";
    if (!h) return fail(nullptr, CH_ERR_INVALID, w + "NULL handle");
    if (!pop || !members || !io || !io->step) return fail(h, CH_ERR_INVALID, w + "NULL argument");
    if (n_members < 1 || n_members > pop->max_members)
        return fail(h, CH_ERR_INVALID, w + "n_members must be 1..max_members (" + std::to_string(pop->max_members) + ")");
    if (h->cfg.mode != CH_MODE_CTDE) return fail(h, CH_ERR_UNSUPPORTED, w + "the SB3 rollout buffer is for CTDE handles");
    if (h->E % n_members) return fail(h, CH_ERR_INVALID, w + "the handle's envs must divide evenly among the members");
    if (pop->device != h->device) return fail(h, CH_ERR_INVALID, w + "the tables are on another device than the handle");
    const ch_step_io* sio = io->step;
    if (!io->mean || !io->value || !io->env_actions || !sio->obs || !sio->reward || !sio->terminated || !sio->truncated ||
        !sio->terminal_obs || !sio->reset_happened || (bootstrap_truncated && !io->terminal_value))
        return fail(h, CH_ERR_INVALID, w + "NULL argument: mean, value, env_actions, the step buffers (obs, reward, terminated, "
                                           "truncated, terminal_obs, reset_happened) and terminal_value are required");
    EpRingArgs er;   // the recorder's arguments: the rings and this io's reset_happened / episode_stats
    if (ring) {
        if (int rc = ep_ring_pop_args(h, ring, sio, er, "ch_rollout_collect_pop_log", true)) return rc;
        if (ring->n_members != n_members)
            return fail(h, CH_ERR_INVALID, "ch_rollout_collect_pop_log: the ring's n_members (" + std::to_string(ring->n_members) +
                                               ") is not the call's (" + std::to_string(n_members) + ")");
    }
    const int P = n_members;
    const int64_t E = h->E / P;
    const ch_rollout_member& m0 = members[0];
    const int obs_dim = h->rows * 86;
    // every member as ch_rollout_collect checks it, then what the members must agree on; nothing is launched before
    std::set<const void*> writable;
    for (int p = 0; p < P; ++p) {
        const ch_rollout_member& c = members[p];
        const ch_rollout& rb = c.rb;
        const std::string wp = w + "member " + std::to_string(p) + ": ";
        if (!c.actor || !c.log_std) return fail(h, CH_ERR_INVALID, wp + "NULL argument (actor, log_std)");
        if (!c.critic) return fail(h, CH_ERR_INVALID, wp + "NULL critic (a fused actor-critic is not supported here)");
        float* const arrays[9] = {rb.obs, rb.actions, rb.rewards, rb.episode_starts, rb.values, rb.log_probs, rb.advantages,
                                  rb.returns, rb.last_episode_starts};
        for (float* a : arrays)
            if (!a) return fail(h, CH_ERR_INVALID, wp + "NULL rollout buffer array");
        if (rb.n_steps < 1 || rb.act_dim < h->NC * 4 || rb.act_dim > 256)
            return fail(h, CH_ERR_INVALID, wp + "n_steps >= 1 and num_drones * 4 = " + std::to_string(h->NC * 4) +
                                               " <= act_dim <= 256 required");
        if (rb.n_steps != m0.rb.n_steps || rb.act_dim != m0.rb.act_dim)
            return fail(h, CH_ERR_INVALID, wp + "n_steps and act_dim must be member 0's");
        if (!same_mlp_arch(c.actor, m0.actor) || !same_mlp_arch(c.critic, m0.critic))
            return fail(h, CH_ERR_INVALID, wp + "architecture (dims, activation, clip, splits) differs from member 0's");
        for (float* a : arrays)
            if (!writable.insert(a).second) return fail(h, CH_ERR_INVALID, wp + "a writable buffer is shared with another array or member");
    }
    const RoPopSlice s1 = ro_pop_slice(h->E, P, P > 1 ? 1 : 0, obs_dim, h->NC, m0.rb.act_dim);
    if ((reinterpret_cast<uintptr_t>(sio->obs) | reinterpret_cast<uintptr_t>(sio->terminal_obs) | (uintptr_t)(s1.obs * 4)) & 15)
        return fail(h, CH_ERR_INVALID, w + "obs buffers must be 16-byte aligned");
    for (int p = 0; p < P; ++p)
        if (reinterpret_cast<uintptr_t>(members[p].rb.obs) & 15)
            return fail(h, CH_ERR_INVALID, w + "member " + std::to_string(p) + ": obs buffers must be 16-byte aligned");
    const int32_t T = m0.rb.n_steps, act_dim = m0.rb.act_dim;
    // the flush period of a solo handle of E envs, so that every f32 operation comes in the solo call's order
    const int kTvEvery = ro_tv_every(E, obs_dim);
    const long long cap = (long long)E * kTvEvery;
    // the members' arguments: segs (actor, critic) on the member's rows of the handle's obs, the critic over its queue
    // slice, and its RolloutArgs (the solo epilogue path's, copy_obs on every step); the queue's pointers come later
    struct Member { MlpArgs segs[2], ftv; RolloutArgs a, ap; };
    std::vector<Member> mb((size_t)P);
    HIP_TRY(h, hipSetDevice(h->device));   // (the plans ask the device for its CU count)
    MlpPlan plan[kRoPopKinds] = {};
    for (int p = 0; p < P; ++p) {
        const ch_rollout_member& c = members[p];
        const std::string wp = "ch_rollout_collect_pop: member " + std::to_string(p);
        const RoPopSlice sl = ro_pop_slice(h->E, P, p, obs_dim, h->NC, act_dim);
        Member& m = mb[(size_t)p];
        int rc;
        if ((rc = policy_args(h, c.actor, sio->obs + sl.obs, io->mean + sl.mean, m.segs[0], (wp + " (actor)").c_str()))) return rc;
        if ((rc = policy_args(h, c.critic, sio->obs + sl.obs, io->value + sl.row, m.segs[1], (wp + " (critic)").c_str()))) return rc;
        if (c.actor->dims[c.actor->n_layers] != act_dim || c.critic->dims[c.critic->n_layers] != 1)
            return fail(h, CH_ERR_INVALID, wp + ": actor output must be act_dim wide, critic output 1");
        for (MlpArgs& sg : m.segs) { sg.rows = E; sg.env_n = h->envi + sl.env; }
        std::string err;
        float one = 0.0f;   // (the queue is allocated after the checks: a placeholder until then)
        if ((rc = mlp_args(c.critic, &one, cap, &one, m.ftv, err))) return fail(h, rc, wp + ": " + err);
        m.ftv.kcap = std::min(m.ftv.dims[0], h->NC * 86);
        MlpPlan mine[kRoPopKinds];
        const bool fits = mlp_pop_plan(m.segs, 2, mine[kRoPopStep]) && mlp_pop_plan(&m.segs[1], 1, mine[kRoPopLast]) &&
                          (!bootstrap_truncated || mlp_pop_plan(&m.ftv, 1, mine[kRoPopFlush]));
        if (!fits) return fail(h, CH_ERR_UNSUPPORTED, wp + ": the nets are not a k_mlp2 launch (no k_mlp / store-kernel path here)");
        for (int k = 0; k < kRoPopKinds; ++k) {
            if (k == kRoPopFlush && !bootstrap_truncated) continue;
            if (p == 0) plan[k] = mine[k];
            else if (!same_mlp_plan(plan[k], mine[k]))
                return fail(h, CH_ERR_UNSUPPORTED, wp + ": its forward plan (packed or raw weights, alignment) differs from member 0's");
        }
        RolloutArgs& a = m.a;
        std::memset(&a, 0, sizeof(a));
        a.T = T; a.rows = E; a.obs_dim = obs_dim; a.act_dim = act_dim; a.env_act_dim = h->NC * 4;
        a.mean_ld = act_dim; a.value_ld = 1; a.tv_ld = 1; a.post_prev = 1; a.copy_obs = 1;
        a.obs = c.rb.obs; a.actions = c.rb.actions; a.rewards = c.rb.rewards; a.episode_starts = c.rb.episode_starts;
        a.values = c.rb.values; a.log_probs = c.rb.log_probs; a.advantages = c.rb.advantages; a.returns = c.rb.returns;
        a.last_episode_starts = c.rb.last_episode_starts;
        a.reward = sio->reward + sl.row; a.terminated = sio->terminated + sl.row; a.truncated = sio->truncated + sl.row;
        a.gamma = c.gamma;
        a.gamma_lambda = (float)((double)c.gamma * (double)c.gae_lambda);   // SB3: float32(self.gamma * self.gae_lambda)
        a.obs_now = sio->obs + sl.obs; a.mean = io->mean + sl.mean; a.value = io->value + sl.row;
        a.log_std = c.log_std; a.seed = c.seed; a.env_actions = io->env_actions + sl.env_actions;
    }
    hipStream_t st = (hipStream_t)stream;
    ch_rollout_state& q = h->ro;
    if (bootstrap_truncated) {
        int rc;
        if ((rc = grow(h, (void**)&q.tv_obs, &q.tv_obs_bytes, sizeof(float) * (size_t)cap * P * obs_dim)) ||
            (rc = grow(h, (void**)&q.tv_row, &q.tv_row_bytes, sizeof(long long) * (size_t)cap * P)) ||
            (rc = grow(h, (void**)&q.tv_val, &q.tv_val_bytes, sizeof(float) * (size_t)cap * P)) ||
            (rc = grow(h, (void**)&q.tv_count, &q.tv_count_bytes, sizeof(int) * (size_t)P)))
            return rc;
        HIP_TRY(h, hipMemsetAsync(q.tv_count, 0, sizeof(int) * (size_t)P, st));
        for (int p = 0; p < P; ++p) {
            const RoPopSlice sl = ro_pop_slice(h->E, P, p, obs_dim, h->NC, act_dim);
            Member& m = mb[(size_t)p];
            // V(terminal obs) over the member's queue slice: whole (12, 86) blocks, zero past the constructor's drones
            m.ftv.x = q.tv_obs + (size_t)sl.queue * obs_dim;
            m.ftv.y = q.tv_val + sl.queue;
            m.ftv.rows_dev = q.tv_count + p;
            m.ftv.vec_w &= ~(1 << 7);   // (the placeholder's alignment)
            if (reinterpret_cast<uintptr_t>(m.ftv.x) % 16 == 0 && m.ftv.dims[0] % 4 == 0) m.ftv.vec_w |= 1 << 7;
            RolloutArgs& a = m.a;
            a.defer = 1; a.term_obs = sio->terminal_obs + sl.obs; a.tv_obs = q.tv_obs + (size_t)sl.queue * obs_dim;
            a.tv_count = q.tv_count + p; a.tv_row = q.tv_row + sl.queue;
            m.ap = a;
            m.ap.rows = cap;
            m.ap.terminal_value = q.tv_val + sl.queue;
        }
    }
    // the staging slot: not before the copy that read it last is done (two calls ago; the device block behind it is
    // read by that call's launches, which this call's copy follows in the stream)
    ch_rollout_pop::Slot& slot = pop->slot[pop->calls++ % kRoPopSlots];
    if (slot.queued) {
        HIP_TRY(h, hipEventSynchronize(slot.copied));
        slot.queued = false;
    }
    const int roles[2] = {kRoleSample, kRoleValue}, tv_role = kRoleTvApply;
    for (int p = 0; p < P; ++p) {
        Member& m = mb[(size_t)p];
        PopMlp* host[kRoPopKinds];
        for (int k = 0; k < kRoPopKinds; ++k) host[k] = reinterpret_cast<PopMlp*>(slot.host + pop->off[k]) + p;
        mlp_pop_fill(*host[kRoPopStep], plan[kRoPopStep], m.segs, roles, &m.a);
        if (bootstrap_truncated) mlp_pop_fill(*host[kRoPopFlush], plan[kRoPopFlush], &m.ftv, &tv_role, &m.ap);
        else std::memset(host[kRoPopFlush], 0, sizeof(PopMlp));
        mlp_pop_fill(*host[kRoPopLast], plan[kRoPopLast], &m.segs[1], nullptr, nullptr);
    }
    HIP_TRY(h, hipMemcpyAsync(slot.dev, slot.host, pop->bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipEventRecord(slot.copied, st));
    slot.queued = true;
    const PopMlp* dev[kRoPopKinds];
    for (int k = 0; k < kRoPopKinds; ++k) dev[k] = reinterpret_cast<const PopMlp*>(slot.dev + pop->off[k]);
    auto flush = [&]() -> hipError_t {
        hipError_t e = launch_mlp_pop(plan[kRoPopFlush], dev[kRoPopFlush], P, 0, st);
        if (e == hipSuccess) e = hipMemsetAsync(q.tv_count, 0, sizeof(int) * (size_t)P, st);
        return e;
    };
    // per step: every member's actor and critic on its rows of the handle's obs with the store in their epilogues
    // (step t - 1's post and the copy of obs[t] into the member's buffer in the critic's), the flush where a solo
    // handle of E envs has it, one env step of the whole handle into its own obs buffer
    ch_step_io s = collect_step_io(sio, io->env_actions);
    for (int32_t t = 0; t < T; ++t) {
        HIP_TRY(h, launch_mlp_pop(plan[kRoPopStep], dev[kRoPopStep], P, t, st));
        if (bootstrap_truncated && t > 0 && t % kTvEvery == 0) HIP_TRY(h, flush());
        if (int rc = ch_step(h, &s, stream)) return rc;
        // the episode rings, where ch_rollout_collect_log records: step t's reset_happened / episode_stats are the
        // launch above's, and nothing before step t + 1's env step writes them (the forwards, the flush and the post
        // write the members' buffers, the queue and the scratch outputs only)
        if (ring) HIP_TRY(h, launch_ep_ring_record_pop(er, P, st));
    }
    // the tail, as the solo epilogue path: the last step's post, the last flush, V(obs after the last step), GAE
    HIP_TRY(h, launch_rollout_pop(dev[kRoPopStep], P, E, 0, T, st));
    if (bootstrap_truncated) HIP_TRY(h, flush());
    HIP_TRY(h, launch_mlp_pop(plan[kRoPopLast], dev[kRoPopLast], P, 0, st));
    HIP_TRY(h, launch_rollout_pop(dev[kRoPopStep], P, E, 2, T, st));
    return CH_OK;
}

extern "C" {

int ch_rollout_collect_pop(ch_handle* h, ch_rollout_pop* pop, const ch_rollout_member* members, int32_t n_members,
                           const ch_rollout_io* io, int32_t bootstrap_truncated, void* stream) {
    return rollout_collect_pop(h, pop, members, n_members, io, bootstrap_truncated, nullptr, stream);
}

int ch_rollout_collect_pop_log(ch_handle* h, ch_rollout_pop* pop, const ch_rollout_member* members, int32_t n_members,
                               const ch_rollout_io* io, int32_t bootstrap_truncated, const ch_ep_ring_pop* ring,
                               void* stream) {
    return rollout_collect_pop(h, pop, members, n_members, io, bootstrap_truncated, ring, stream);
}

}  // extern "C"

extern "C" {

// ch_marl_rollout_collect and ch_marl_rollout_collect_log (`ring`: NULL, or the episode ring every step is recorded in)
static int marl_rollout_collect(ch_handle* h, const ch_marl_rollout* rb, const ch_marl_rollout_io* io, const ch_mlp* policy,
                                const ch_mlp* value, uint64_t seed, float gamma, float gae_lambda,
                                const ch_marl_ep_ring* ring, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_marl_rollout_collect: NULL handle");
    if (h->cfg.mode != CH_MODE_MARL)
        return fail(h, CH_ERR_UNSUPPORTED, "ch_marl_rollout_collect: the per-agent rollout is for MARL handles");
    if (!rb || !io || !io->step || !policy || !value || !io->policy_out || !io->value_out || !io->env_actions)
        return fail(h, CH_ERR_INVALID, "ch_marl_rollout_collect: NULL argument");
    if (rb->n_steps < 1 || rb->act_dim != 4)
        return fail(h, CH_ERR_INVALID, "ch_marl_rollout_collect: n_steps >= 1 and act_dim = 4 (one VEL action per agent)");
    if (!rb->obs || !rb->actions || !rb->log_probs || !rb->values || !rb->rewards || !rb->agent_mask || !rb->terminated ||
        !rb->truncated || !rb->advantages || !rb->returns || !rb->last_values)
        return fail(h, CH_ERR_INVALID, "ch_marl_rollout_collect: NULL rollout buffer array");
    const ch_step_io* sio = io->step;
    if (!sio->obs || !sio->reward || !sio->terminated || !sio->truncated)
        return fail(h, CH_ERR_INVALID, "ch_marl_rollout_collect: the step buffers obs, reward, terminated, truncated are required");
    if ((reinterpret_cast<uintptr_t>(sio->obs) | reinterpret_cast<uintptr_t>(rb->obs)) & 15)
        return fail(h, CH_ERR_INVALID, "ch_marl_rollout_collect: obs buffers must be 16-byte aligned");
    if (policy->dims[policy->n_layers] != 2 * rb->act_dim || value->dims[value->n_layers] != 1)
        return fail(h, CH_ERR_INVALID, "ch_marl_rollout_collect: the policy must output 2 * act_dim (mean, log_std), the value net 1");
    int rc;
    MarlRingArgs er;   // the recorder's arguments: the ring and this io's reward / reset_happened
    if (ring && (rc = marl_ring_args(h, ring, sio, er, "ch_marl_rollout_collect_log"))) return rc;
    MlpArgs fp, fv;
    if ((rc = policy_args(h, policy, sio->obs, io->policy_out, fp, "ch_marl_rollout_collect (policy)"))) return rc;
    if ((rc = policy_args(h, value, sio->obs, io->value_out, fv, "ch_marl_rollout_collect (value)"))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    MarlArgs a;
    std::memset(&a, 0, sizeof(a));
    a.T = rb->n_steps; a.A = rb->act_dim; a.N = h->NC; a.E = h->E; a.rows = h->E * h->NC;
    a.env_n = h->envi; a.env_active = h->envi + 7 * h->E;
    a.pol = io->policy_out; a.val = io->value_out; a.seed = seed; a.post_prev = 1;
    a.reward = sio->reward; a.term = sio->terminated; a.trunc = sio->truncated;
    a.gamma = gamma; a.gamma_lambda = (float)((double)gamma * (double)gae_lambda);
    a.obs = rb->obs; a.actions = rb->actions; a.log_probs = rb->log_probs; a.values = rb->values; a.rewards = rb->rewards;
    a.advantages = rb->advantages; a.returns = rb->returns; a.last_values = rb->last_values; a.env_actions = io->env_actions;
    a.mask = rb->agent_mask; a.terminated = rb->terminated; a.truncated = rb->truncated;
    // the step writes its observations straight into the buffer's next slot (a step into a buffer other than the one
    // it wrote last writes every block in full); the last step into the env's own buffer.  No terminal observations:
    // an agent's trajectory ends only where it terminates (no bootstrap), so the reset path needs no copy.
    // With an odd number of agent rows a slot is 8 bytes off the 16-byte alignment the step and the forwards need:
    // every step then writes the env's own buffer and the store kernel copies it into the slot (as it does at t = 0).
    ch_step_io s = collect_step_io(sio, io->env_actions);
    s.terminal_obs = nullptr;
    const size_t slot = (size_t)a.rows * 86;
    const bool in_place = (slot * sizeof(float)) % 16 == 0;
    MlpArgs segs[2];
    for (int32_t t = 0; t < rb->n_steps; ++t) {
        const bool own = t == 0 || !in_place;
        const float* x = own ? sio->obs : rb->obs + (size_t)t * slot;
        segs[0] = fp; segs[1] = fv;
        segs[0].x = segs[1].x = x;
        HIP_TRY(h, launch_mlp_multi(segs, 2, st));
        a.t = t;
        a.obs_now = own ? sio->obs : nullptr;
        HIP_TRY(h, launch_marl_rollout(a, 0, st));
        s.obs = (in_place && t + 1 < rb->n_steps) ? rb->obs + (size_t)(t + 1) * slot : sio->obs;
        if ((rc = ch_step(h, &s, stream))) return rc;
        // The episode ring: step t's reward / reset_happened are written by the step above and by nothing else before
        // step t + 1's ch_step -- the forwards write the scratch outputs, and the store kernel of step t + 1 (which
        // posts step t: post_prev) and the GAE kernel read the step's outputs and write the buffer only.  agent_mask[t]
        // was written by step t's store kernel, before the step.  So the recorder goes right here.
        if (ring) {
            er.live = rb->agent_mask + (size_t)t * a.rows;
            HIP_TRY(h, launch_marl_ep_ring_record(er, st));
        }
    }
    // V(obs after the last step) -> last_values, the last step's post, GAE
    fv.x = sio->obs;
    HIP_TRY(h, launch_mlp_multi(&fv, 1, st));
    HIP_TRY(h, launch_marl_rollout(a, 1, st));
    return CH_OK;
}

int ch_marl_rollout_collect(ch_handle* h, const ch_marl_rollout* rb, const ch_marl_rollout_io* io, const ch_mlp* policy,
                            const ch_mlp* value, uint64_t seed, float gamma, float gae_lambda, void* stream) {
    return marl_rollout_collect(h, rb, io, policy, value, seed, gamma, gae_lambda, nullptr, stream);
}

int ch_marl_rollout_collect_log(ch_handle* h, const ch_marl_rollout* rb, const ch_marl_rollout_io* io,
                                const ch_mlp* policy, const ch_mlp* value, uint64_t seed, float gamma, float gae_lambda,
                                const ch_marl_ep_ring* ring, void* stream) {
    return marl_rollout_collect(h, rb, io, policy, value, seed, gamma, gae_lambda, ring, stream);
}

}  // extern "C"
