// ch_api_ppo.cpp — the PPO update's part of the C ABI (see include/cattleherd.h): argument checks, the flat
// parameter order and the launches of ch_ppo.hip.  Handle-free: failures go to ch_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "ch_handle.h"
#include "ch_ppo.h"

using namespace ch;

namespace {

// dims, the flat order of SB3ActorCritic.parameters() (policy MLP, value MLP, action_net, value_net, log_std) and,
// with `ptrs`, the pointers; CH_OK or the error with its message in `err`
int ppo_net(const ch_ppo_net* net, bool ptrs, PpoNet& n, std::string& err) {
    n = PpoNet{};
    if (net->obs_dim < 1) { err = "obs_dim must be >= 1"; return CH_ERR_UNSUPPORTED; }
    if (net->act_dim < 1 || net->act_dim > kPpoMaxAct) { err = "act_dim must be 1..64"; return CH_ERR_UNSUPPORTED; }
    const int nh[2] = {net->n_pi, net->n_vf};
    const int32_t* widths[2] = {net->pi, net->vf};
    float* const* w[2] = {net->pi_weight, net->vf_weight};
    float* const* b[2] = {net->pi_bias, net->vf_bias};
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
        m.dims[m.layers] = ni == 0 ? net->act_dim : 1;
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
    n.goff_log_std = off; off += net->act_dim;
    n.n_params = off;
    if (!ptrs) return CH_OK;
    for (int ni = 0; ni < 2; ++ni)
        for (int li = 0; li < n.net[ni].layers; ++li) {
            if (!w[ni][li] || !b[ni][li]) { err = "NULL weight or bias"; return CH_ERR_INVALID; }
            n.net[ni].w[li] = w[ni][li]; n.net[ni].b[li] = b[ni][li];
        }
    if (!net->log_std) { err = "NULL log_std"; return CH_ERR_INVALID; }
    n.log_std = net->log_std;
    return CH_OK;
}

PpoHp ppo_hp(const ch_ppo_hparams* hp) {
    PpoHp h;
    h.lr = hp->learning_rate; h.beta1 = hp->beta1; h.beta2 = hp->beta2; h.eps = hp->eps;
    h.clip_range = hp->clip_range; h.ent_coef = hp->ent_coef; h.vf_coef = hp->vf_coef;
    h.max_grad_norm = hp->max_grad_norm; h.normalize_advantage = hp->normalize_advantage != 0;
    return h;
}

int ppo_data(const ch_ppo_data* data, PpoData& d, std::string& err) {
    if (!data->obs || !data->actions || !data->old_log_prob || !data->advantages || !data->returns) {
        err = "NULL data array";
        return CH_ERR_INVALID;
    }
    if (data->rows < 1) { err = "rows < 1"; return CH_ERR_INVALID; }
    d.obs = data->obs; d.actions = data->actions; d.old_log_prob = data->old_log_prob;
    d.advantages = data->advantages; d.returns = data->returns; d.rows = data->rows;
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

}  // extern "C"
