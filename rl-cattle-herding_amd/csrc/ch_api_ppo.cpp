// ch_api_ppo.cpp — the PPO update's part of the C ABI (see include/cattleherd.h): argument checks, the flat
// parameter order and the launches of ch_ppo.hip.  Handle-free: failures go to ch_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "ch_handle.h"
#include "ch_ppo.h"

using namespace ch;

namespace {

// what the two ABI structs (ch_ppo_net, ch_marl_ppo_net) say of the two MLPs
struct NetDesc {
    int obs_dim, act_dim, head;   // head: the policy head's width
    int nh[2];
    const int32_t* widths[2];
    float* const* w[2];
    float* const* b[2];
    float* log_std;               // kPpoSb3
};

// dims, the flat order of the model's parameters() (policy MLP, value MLP, policy head, value head, then SB3's
// log_std) and, with `ptrs`, the pointers; CH_OK or the error with its message in `err`
int build_net(const NetDesc& D, int flavour, bool ptrs, PpoNet& n, std::string& err) {
    n = PpoNet{};
    n.flavour = flavour;
    const NetDesc* net = &D;
    const int* nh = D.nh;
    const int32_t* const* widths = D.widths;
    if (net->obs_dim < 1) { err = "obs_dim must be >= 1"; return CH_ERR_UNSUPPORTED; }
    if (net->act_dim < 1 || D.head > kPpoMaxAct) {
        err = flavour == kPpoSb3 ? "act_dim must be 1..64" : "act_dim must be 1..32";
        return CH_ERR_UNSUPPORTED;
    }
    for (int ni = 0; ni < 2; ++ni) {
        if (nh[ni] < 1 || nh[ni] > 2) { err = "each MLP must have 1 or 2 hidden layers"; return CH_ERR_UNSUPPORTED; }
        for (int i = 0; i < nh[ni]; ++i)
            if (widths[ni][i] < 16 || widths[ni][i] > kPpoMaxHidden || widths[ni][i] % 16) {
                err = "hidden widths must be multiples of 16, at most 256";
                return CH_ERR_UNSUPPORTED;
            }
    }
    n.obs_dim = net->obs_dim; n.act_dim = net->act_dim;
    long long off = 0;
    for (int ni = 0; ni < 2; ++ni) {
        PpoMlp& m = n.net[ni];
        m.layers = nh[ni] + 1;
        m.dims[0] = net->obs_dim;
        for (int i = 0; i < nh[ni]; ++i) m.dims[i + 1] = widths[ni][i];
        m.dims[m.layers] = ni == 0 ? D.head : 1;
        for (int li = 0; li < nh[ni]; ++li) {
            m.goff_w[li] = off; off += (long long)m.dims[li + 1] * m.dims[li];
            m.goff_b[li] = off; off += m.dims[li + 1];
        }
    }
    for (int ni = 0; ni < 2; ++ni) {
        PpoMlp& m = n.net[ni];
        const int li = m.layers - 1;
        m.goff_w[li] = off; off += (long long)m.dims[li + 1] * m.dims[li];
        m.goff_b[li] = off; off += m.dims[li + 1];
    }
    n.goff_log_std = off;
    if (flavour == kPpoSb3) off += net->act_dim;
    n.n_params = off;
    if (!ptrs) return CH_OK;
    for (int ni = 0; ni < 2; ++ni)
        for (int li = 0; li < n.net[ni].layers; ++li) {
            if (!D.w[ni][li] || !D.b[ni][li]) { err = "NULL weight or bias"; return CH_ERR_INVALID; }
            n.net[ni].w[li] = D.w[ni][li]; n.net[ni].b[li] = D.b[ni][li];
        }
    if (flavour == kPpoSb3) {
        if (!net->log_std) { err = "NULL log_std"; return CH_ERR_INVALID; }
        n.log_std = net->log_std;
    }
    return CH_OK;
}

int ppo_net(const ch_ppo_net* net, bool ptrs, PpoNet& n, std::string& err) {
    const NetDesc D = {net->obs_dim, net->act_dim, net->act_dim, {net->n_pi, net->n_vf}, {net->pi, net->vf},
                       {net->pi_weight, net->vf_weight}, {net->pi_bias, net->vf_bias}, net->log_std};
    return build_net(D, kPpoSb3, ptrs, n, err);
}

// the RLlib module: actor encoder + pi (head [mean, log_std]: 2 * act_dim wide), critic encoder + vf
int marl_net(const ch_marl_ppo_net* net, bool ptrs, PpoNet& n, std::string& err) {
    const int head = net->act_dim > kPpoMaxAct / 2 ? kPpoMaxAct + 1 : 2 * net->act_dim;
    const NetDesc D = {net->obs_dim, net->act_dim, head, {net->n_actor, net->n_critic}, {net->actor, net->critic},
                       {net->actor_weight, net->critic_weight}, {net->actor_bias, net->critic_bias}, nullptr};
    return build_net(D, kPpoRllib, ptrs, n, err);
}

PpoHp ppo_hp(const ch_ppo_hparams* hp) {
    PpoHp h = {};
    h.lr = hp->learning_rate; h.beta1 = hp->beta1; h.beta2 = hp->beta2; h.eps = hp->eps;
    h.clip_range = hp->clip_range; h.ent_coef = hp->ent_coef; h.vf_coef = hp->vf_coef;
    h.max_grad_norm = hp->max_grad_norm; h.normalize_advantage = hp->normalize_advantage != 0;
    return h;
}

PpoHp marl_hp(const ch_marl_ppo_hparams* hp) {
    PpoHp h = {};
    h.lr = hp->learning_rate; h.beta1 = hp->beta1; h.beta2 = hp->beta2; h.eps = hp->eps;
    h.clip_range = hp->clip_param; h.ent_coef = hp->entropy_coeff; h.vf_coef = hp->vf_loss_coeff;
    h.max_grad_norm = hp->grad_clip > 0.0 ? hp->grad_clip : 0.0;
    h.vf_clip = hp->vf_clip_param; h.log_std_clip = hp->log_std_clip; h.kl_coeff_dev = hp->kl_coeff_dev;
    return h;
}

int marl_data(const ch_marl_ppo_data* data, PpoData& d, std::string& err) {
    if (!data->obs || !data->actions || !data->old_log_prob || !data->old_dist_inputs || !data->advantages ||
        !data->value_targets) {
        err = "NULL data array";
        return CH_ERR_INVALID;
    }
    if (data->rows < 1) { err = "rows < 1"; return CH_ERR_INVALID; }
    d = PpoData{data->obs, data->actions, data->old_log_prob, data->advantages, data->value_targets, data->rows,
                data->old_dist_inputs};
    return CH_OK;
}

int ppo_data(const ch_ppo_data* data, PpoData& d, std::string& err) {
    if (!data->obs || !data->actions || !data->old_log_prob || !data->advantages || !data->returns) {
        err = "NULL data array";
        return CH_ERR_INVALID;
    }
    if (data->rows < 1) { err = "rows < 1"; return CH_ERR_INVALID; }
    d.obs = data->obs; d.actions = data->actions; d.old_log_prob = data->old_log_prob;
    d.advantages = data->advantages; d.returns = data->returns; d.rows = data->rows; d.old_dist = nullptr;
    return CH_OK;
}

constexpr int64_t kMaxBatch = 1 << 24;   // (row counts stay well inside int arithmetic)

int launch_fail(const char* who, hipError_t e) {
    return fail(nullptr, CH_ERR_DEVICE, std::string(who) + ": launch: " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int64_t ch_ppo_param_count(const ch_ppo_net* net) {
    PpoNet n;
    std::string err;
    if (!net || ppo_net(net, false, n, err)) return -1;
    return n.n_params;
}

int64_t ch_ppo_scratch_size(const ch_ppo_net* net, int64_t batch_size) {
    PpoNet n;
    std::string err;
    if (!net || batch_size < 1 || batch_size > kMaxBatch || ppo_net(net, false, n, err)) return -1;
    PpoScratch s;
    ppo_scratch_layout(n, batch_size, s);
    return s.total;
}

int ch_ppo_grad(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                int64_t batch, float* grad_flat, float* stats4, float* scratch, void* stream) {
    const std::string who = "ch_ppo_grad: ";
    if (!net || !hp || !data || !idx || !grad_flat || !stats4 || !scratch) return fail(nullptr, CH_ERR_INVALID, who + "NULL argument");
    PpoNet n;
    PpoData d;
    std::string err;
    int rc;
    if ((rc = ppo_net(net, true, n, err)) || (rc = ppo_data(data, d, err))) return fail(nullptr, rc, who + err);
    if (batch < 1 || batch > kMaxBatch) return fail(nullptr, CH_ERR_INVALID, who + "batch must be 1..2^24");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(nullptr, CH_ERR_INVALID, who + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, batch, s);
    const PpoHp h = ppo_hp(hp);
    hipStream_t st = (hipStream_t)stream;
    int np = 0;
    hipError_t e = ppo_launch_grad(n, h, d, reinterpret_cast<const long long*>(idx), batch, grad_flat, scratch, s, nullptr, &np, st);
    if (e == hipSuccess) e = ppo_launch_stats(n, scratch, s, np, batch, stats4, st);
    return e == hipSuccess ? CH_OK : launch_fail("ch_ppo_grad", e);
}

int ch_ppo_adam(const ch_ppo_net* net, const ch_ppo_hparams* hp, const float* grad_flat, float* m, float* v,
                int64_t* step_dev, float* scratch, void* stream) {
    const std::string who = "ch_ppo_adam: ";
    if (!net || !hp || !grad_flat || !m || !v || !step_dev || !scratch) return fail(nullptr, CH_ERR_INVALID, who + "NULL argument");
    PpoNet n;
    std::string err;
    int rc;
    if ((rc = ppo_net(net, true, n, err))) return fail(nullptr, rc, who + err);
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(nullptr, CH_ERR_INVALID, who + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, 1, s);   // (only the partials are used: any scratch sized for this net holds them)
    const PpoHp h = ppo_hp(hp);
    hipStream_t st = (hipStream_t)stream;
    int np = 0;
    hipError_t e = ppo_launch_sumsq(n, grad_flat, scratch, s, reinterpret_cast<long long*>(step_dev), &np, st);
    if (e == hipSuccess)
        e = ppo_launch_adam(n, h, grad_flat, m, v, reinterpret_cast<const long long*>(step_dev), scratch, s, np, 1, nullptr, st);
    return e == hipSuccess ? CH_OK : launch_fail("ch_ppo_adam", e);
}

int ch_ppo_train(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                 int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev, float* stats, float* scratch,
                 void* stream) {
    const std::string who = "ch_ppo_train: ";
    if (!net || !hp || !data || !idx || !m || !v || !step_dev || !scratch) return fail(nullptr, CH_ERR_INVALID, who + "NULL argument");
    PpoNet n;
    PpoData d;
    std::string err;
    int rc;
    if ((rc = ppo_net(net, true, n, err)) || (rc = ppo_data(data, d, err))) return fail(nullptr, rc, who + err);
    if (n_idx < 1 || batch_size < 1 || batch_size > kMaxBatch) return fail(nullptr, CH_ERR_INVALID, who + "n_idx >= 1 and batch_size 1..2^24 required");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(nullptr, CH_ERR_INVALID, who + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, std::min(batch_size, n_idx), s);   // one layout for every step, the partial last one included
    const PpoHp h = ppo_hp(hp);
    hipStream_t st = (hipStream_t)stream;
    float* grad = scratch + s.grad;
    long long* step = reinterpret_cast<long long*>(step_dev);
    int64_t k = 0;
    for (int64_t j = 0; j < n_idx; j += batch_size, ++k) {
        const int64_t batch = std::min(batch_size, n_idx - j);
        PpoScratch sj = s;
        sj.tiles = (int)((batch + kPpoTile - 1) / kPpoTile);
        sj.bp = sj.tiles * kPpoTile;
        int np = 0;
        hipError_t e = ppo_launch_grad(n, h, d, reinterpret_cast<const long long*>(idx) + j, batch, grad, scratch, sj, step, &np, st);
        if (e == hipSuccess) e = ppo_launch_adam(n, h, grad, m, v, step, scratch, sj, np, batch, stats ? stats + 4 * k : nullptr, st);
        if (e != hipSuccess) return launch_fail("ch_ppo_train", e);
    }
    return CH_OK;
}

int64_t ch_marl_ppo_param_count(const ch_marl_ppo_net* net) {
    PpoNet n;
    std::string err;
    // (-1 is the answer; the reason goes to ch_last_error(NULL) as for the calls below)
    if (!net) { fail(nullptr, CH_ERR_INVALID, "ch_marl_ppo_param_count: NULL argument"); return -1; }
    if (int rc = marl_net(net, false, n, err)) { fail(nullptr, rc, "ch_marl_ppo_param_count: " + err); return -1; }
    return n.n_params;
}

int64_t ch_marl_ppo_scratch_size(const ch_marl_ppo_net* net, int64_t batch_size) {
    PpoNet n;
    std::string err;
    const std::string who = "ch_marl_ppo_scratch_size: ";
    if (!net) { fail(nullptr, CH_ERR_INVALID, who + "NULL argument"); return -1; }
    if (batch_size < 1 || batch_size > kMaxBatch) { fail(nullptr, CH_ERR_INVALID, who + "batch_size must be 1..2^24"); return -1; }
    if (int rc = marl_net(net, false, n, err)) { fail(nullptr, rc, who + err); return -1; }
    PpoScratch s;
    ppo_scratch_layout(n, batch_size, s);
    return s.total;
}

int ch_marl_ppo_grad(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                     const int64_t* idx, int64_t batch, float* grad_flat, float* stats5, float* scratch, void* stream) {
    const std::string who = "ch_marl_ppo_grad: ";
    if (!net || !hp || !data || !idx || !grad_flat || !stats5 || !scratch) return fail(nullptr, CH_ERR_INVALID, who + "NULL argument");
    PpoNet n;
    PpoData d;
    std::string err;
    int rc;
    if ((rc = marl_net(net, true, n, err)) || (rc = marl_data(data, d, err))) return fail(nullptr, rc, who + err);
    if (!hp->kl_coeff_dev) return fail(nullptr, CH_ERR_INVALID, who + "NULL kl_coeff_dev");
    if (batch < 1 || batch > kMaxBatch) return fail(nullptr, CH_ERR_INVALID, who + "batch must be 1..2^24");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(nullptr, CH_ERR_INVALID, who + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, batch, s);
    const PpoHp h = marl_hp(hp);
    hipStream_t st = (hipStream_t)stream;
    int np = 0;
    hipError_t e = ppo_launch_grad(n, h, d, reinterpret_cast<const long long*>(idx), batch, grad_flat, scratch, s, nullptr, &np, st);
    if (e == hipSuccess) e = ppo_launch_stats(n, scratch, s, np, batch, stats5, st);
    return e == hipSuccess ? CH_OK : launch_fail("ch_marl_ppo_grad", e);
}

int ch_marl_ppo_adam(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const float* grad_flat, float* m, float* v,
                     int64_t* step_dev, float* scratch, void* stream) {
    const std::string who = "ch_marl_ppo_adam: ";
    if (!net || !hp || !grad_flat || !m || !v || !step_dev || !scratch) return fail(nullptr, CH_ERR_INVALID, who + "NULL argument");
    PpoNet n;
    std::string err;
    int rc;
    if ((rc = marl_net(net, true, n, err))) return fail(nullptr, rc, who + err);
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(nullptr, CH_ERR_INVALID, who + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, 1, s);   // (only the partials are used: any scratch sized for this net holds them)
    const PpoHp h = marl_hp(hp);
    hipStream_t st = (hipStream_t)stream;
    int np = 0;
    hipError_t e = ppo_launch_sumsq(n, grad_flat, scratch, s, reinterpret_cast<long long*>(step_dev), &np, st);
    if (e == hipSuccess)
        e = ppo_launch_adam(n, h, grad_flat, m, v, reinterpret_cast<const long long*>(step_dev), scratch, s, np, 1, nullptr, st);
    return e == hipSuccess ? CH_OK : launch_fail("ch_marl_ppo_adam", e);
}

int ch_marl_ppo_train(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                      const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev,
                      float* stats, float* scratch, void* stream) {
    const std::string who = "ch_marl_ppo_train: ";
    if (!net || !hp || !data || !idx || !m || !v || !step_dev || !scratch) return fail(nullptr, CH_ERR_INVALID, who + "NULL argument");
    PpoNet n;
    PpoData d;
    std::string err;
    int rc;
    if ((rc = marl_net(net, true, n, err)) || (rc = marl_data(data, d, err))) return fail(nullptr, rc, who + err);
    if (!hp->kl_coeff_dev) return fail(nullptr, CH_ERR_INVALID, who + "NULL kl_coeff_dev");
    if (n_idx < 1 || batch_size < 1 || batch_size > kMaxBatch) return fail(nullptr, CH_ERR_INVALID, who + "n_idx >= 1 and batch_size 1..2^24 required");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(nullptr, CH_ERR_INVALID, who + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, std::min(batch_size, n_idx), s);   // one layout for every step, the partial last one included
    const PpoHp h = marl_hp(hp);
    hipStream_t st = (hipStream_t)stream;
    float* grad = scratch + s.grad;
    long long* step = reinterpret_cast<long long*>(step_dev);
    int64_t k = 0;
    for (int64_t j = 0; j < n_idx; j += batch_size, ++k) {
        const int64_t batch = std::min(batch_size, n_idx - j);
        PpoScratch sj = s;
        sj.tiles = (int)((batch + kPpoTile - 1) / kPpoTile);
        sj.bp = sj.tiles * kPpoTile;
        int np = 0;
        hipError_t e = ppo_launch_grad(n, h, d, reinterpret_cast<const long long*>(idx) + j, batch, grad, scratch, sj, step, &np, st);
        if (e == hipSuccess) e = ppo_launch_adam(n, h, grad, m, v, step, scratch, sj, np, batch, stats ? stats + 5 * k : nullptr, st);
        if (e != hipSuccess) return launch_fail("ch_marl_ppo_train", e);
    }
    return CH_OK;
}

}  // extern "C"
