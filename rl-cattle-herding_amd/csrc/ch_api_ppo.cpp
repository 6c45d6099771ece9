// ch_api_ppo.cpp — the PPO update's part of the C ABI (see include/cattleherd.h): argument checks, the flat
// parameter order and the launches of ch_ppo.hip.  Handle-free: failures go to ch_last_error(NULL).
// The two ABI faces (ch_ppo_*, ch_marl_ppo_*) are one implementation over a description of each flavour (Sb3, Rllib).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

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
int build_net(const NetDesc& D, PpoFlavour flavour, bool ptrs, PpoNet& n, std::string& err) {
    n = PpoNet{};
    n.flavour = flavour;
    if (D.obs_dim < 1) { err = "obs_dim must be >= 1"; return CH_ERR_UNSUPPORTED; }
    if (D.act_dim < 1 || D.head > kPpoMaxAct) {
        err = flavour == kPpoSb3 ? "act_dim must be 1..64" : "act_dim must be 1..32";
        return CH_ERR_UNSUPPORTED;
    }
    for (int ni = 0; ni < 2; ++ni) {
        if (D.nh[ni] < 1 || D.nh[ni] > 2) { err = "each MLP must have 1 or 2 hidden layers"; return CH_ERR_UNSUPPORTED; }
        for (int i = 0; i < D.nh[ni]; ++i)
            if (D.widths[ni][i] < 16 || D.widths[ni][i] > kPpoMaxHidden || D.widths[ni][i] % 16) {
                err = "hidden widths must be multiples of 16, at most 256";
                return CH_ERR_UNSUPPORTED;
            }
    }
    n.obs_dim = D.obs_dim; n.act_dim = D.act_dim;
    long long off = 0;
    for (int ni = 0; ni < 2; ++ni) {
        PpoMlp& m = n.net[ni];
        m.layers = D.nh[ni] + 1;
        m.dims[0] = D.obs_dim;
        for (int i = 0; i < D.nh[ni]; ++i) m.dims[i + 1] = D.widths[ni][i];
        m.dims[m.layers] = ni == 0 ? D.head : 1;
        for (int li = 0; li < D.nh[ni]; ++li) {
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
    if (flavour == kPpoSb3) off += D.act_dim;
    n.n_params = off;
    if (!ptrs) return CH_OK;
    for (int ni = 0; ni < 2; ++ni)
        for (int li = 0; li < n.net[ni].layers; ++li) {
            if (!D.w[ni][li] || !D.b[ni][li]) { err = "NULL weight or bias"; return CH_ERR_INVALID; }
            n.net[ni].w[li] = D.w[ni][li]; n.net[ni].b[li] = D.b[ni][li];
        }
    if (flavour == kPpoSb3) {
        if (!D.log_std) { err = "NULL log_std"; return CH_ERR_INVALID; }
        n.log_std = D.log_std;
    }
    return CH_OK;
}

// A flavour as the ABI shows it: its three structs, the prefix of its function names (for the messages), how the
// structs read as NetDesc / PpoHp / PpoData (field by field, in the order those declare), and what it asks of its
// hparams (NULL: nothing wrong).
struct Sb3 {
    using Net = ch_ppo_net; using Hparams = ch_ppo_hparams; using Data = ch_ppo_data;
    static constexpr PpoFlavour kFlavour = kPpoSb3;
    static constexpr const char* kPrefix = "ch_ppo_";
    static NetDesc net(const Net* n) {
        return {n->obs_dim, n->act_dim, n->act_dim, {n->n_pi, n->n_vf}, {n->pi, n->vf},
                {n->pi_weight, n->vf_weight}, {n->pi_bias, n->vf_bias}, n->log_std};
    }
    static PpoHp hp(const Hparams* hp) {
        return {hp->learning_rate, hp->beta1, hp->beta2, hp->eps, hp->clip_range, hp->ent_coef, hp->vf_coef,
                hp->max_grad_norm, hp->normalize_advantage != 0, 0.0, 0.0, nullptr};
    }
    static PpoData data(const Data* d) {
        return {d->obs, d->actions, d->old_log_prob, d->advantages, d->returns, d->rows, nullptr};
    }
    static const char* check_hp(const Hparams*) { return nullptr; }
};

// the RLlib module: actor encoder + pi (head [mean, log_std]: 2 * act_dim wide), critic encoder + vf
struct Rllib {
    using Net = ch_marl_ppo_net; using Hparams = ch_marl_ppo_hparams; using Data = ch_marl_ppo_data;
    static constexpr PpoFlavour kFlavour = kPpoRllib;
    static constexpr const char* kPrefix = "ch_marl_ppo_";
    static NetDesc net(const Net* n) {
        const int head = n->act_dim > kPpoMaxAct / 2 ? kPpoMaxAct + 1 : 2 * n->act_dim;
        return {n->obs_dim, n->act_dim, head, {n->n_actor, n->n_critic}, {n->actor, n->critic},
                {n->actor_weight, n->critic_weight}, {n->actor_bias, n->critic_bias}, nullptr};
    }
    static PpoHp hp(const Hparams* hp) {
        return {hp->learning_rate, hp->beta1, hp->beta2, hp->eps, hp->clip_param, hp->entropy_coeff, hp->vf_loss_coeff,
                hp->grad_clip > 0.0 ? hp->grad_clip : 0.0, 0, hp->vf_clip_param, hp->log_std_clip, hp->kl_coeff_dev};
    }
    static PpoData data(const Data* d) {
        return {d->obs, d->actions, d->old_log_prob, d->advantages, d->value_targets, d->rows, d->old_dist_inputs};
    }
    static const char* check_hp(const Hparams* hp) { return hp->kl_coeff_dev ? nullptr : "NULL kl_coeff_dev"; }
};

constexpr int64_t kMaxBatch = 1 << 24;   // (row counts stay well inside int arithmetic)

template <class F>
std::string who(const char* fn) { return std::string(F::kPrefix) + fn + ": "; }

bool misaligned(const float* scratch) { return reinterpret_cast<uintptr_t>(scratch) & 15; }

// The checks that follow a call's NULL-argument test, in their order: the net (`ptrs`: with its pointers), then the
// data and what the flavour asks of its hparams.  CH_OK or the error with its message in `err`.
template <class F>
int to_net(const typename F::Net* net, bool ptrs, PpoNet& n, std::string& err) {
    return build_net(F::net(net), F::kFlavour, ptrs, n, err);
}

template <class F>
int to_data(const typename F::Data* data, const typename F::Hparams* hp, PpoData& d, std::string& err) {
    d = F::data(data);
    if (!d.obs || !d.actions || !d.old_log_prob || !d.advantages || !d.returns || (F::kFlavour == kPpoRllib && !d.old_dist))
        err = "NULL data array";
    else if (d.rows < 1)
        err = "rows < 1";
    else if (const char* bad = F::check_hp(hp))
        err = bad;
    else
        return CH_OK;
    return CH_ERR_INVALID;
}

// (-1 is the answer of the two host-only calls; the reason goes to ch_last_error(NULL) as for the calls below)
template <class F>
int64_t param_count(const typename F::Net* net) {
    const std::string w = who<F>("param_count");
    PpoNet n;
    std::string err;
    if (!net) { fail(nullptr, CH_ERR_INVALID, w + "NULL argument"); return -1; }
    if (int rc = to_net<F>(net, false, n, err)) { fail(nullptr, rc, w + err); return -1; }
    return n.n_params;
}

template <class F>
int64_t scratch_size(const typename F::Net* net, int64_t batch_size) {
    const std::string w = who<F>("scratch_size");
    PpoNet n;
    std::string err;
    if (!net) { fail(nullptr, CH_ERR_INVALID, w + "NULL argument"); return -1; }
    if (batch_size < 1 || batch_size > kMaxBatch) { fail(nullptr, CH_ERR_INVALID, w + "batch_size must be 1..2^24"); return -1; }
    if (int rc = to_net<F>(net, false, n, err)) { fail(nullptr, rc, w + err); return -1; }
    PpoScratch s;
    ppo_scratch_layout(n, batch_size, s);
    return s.total;
}

template <class F>
int grad(const typename F::Net* net, const typename F::Hparams* hp, const typename F::Data* data, const int64_t* idx,
         int64_t batch, float* grad_flat, float* stats, float* scratch, void* stream) {
    const std::string w = who<F>("grad");
    if (!net || !hp || !data || !idx || !grad_flat || !stats || !scratch) return fail(nullptr, CH_ERR_INVALID, w + "NULL argument");
    PpoNet n;
    PpoData d;
    std::string err;
    int rc;
    if ((rc = to_net<F>(net, true, n, err)) || (rc = to_data<F>(data, hp, d, err))) return fail(nullptr, rc, w + err);
    if (batch < 1 || batch > kMaxBatch) return fail(nullptr, CH_ERR_INVALID, w + "batch must be 1..2^24");
    if (misaligned(scratch)) return fail(nullptr, CH_ERR_INVALID, w + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, batch, s);
    const PpoHp h = F::hp(hp);
    const PpoPlan p = ppo_plan(F::kFlavour, false, false, false, false);   // ch_*_train's rows
    hipStream_t st = (hipStream_t)stream;
    int np = 0;
    hipError_t e = ppo_launch_grad(p, n, h, d, nullptr, reinterpret_cast<const long long*>(idx), batch, grad_flat, scratch, s, nullptr, &np, st);
    if (e == hipSuccess) e = ppo_launch_stats(p, n, scratch, s, np, batch, stats, st);
    return e == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, w + "launch: " + hipGetErrorString(e));
}

template <class F>
int adam(const typename F::Net* net, const typename F::Hparams* hp, const float* grad_flat, float* m, float* v,
         int64_t* step_dev, float* scratch, void* stream) {
    const std::string w = who<F>("adam");
    if (!net || !hp || !grad_flat || !m || !v || !step_dev || !scratch) return fail(nullptr, CH_ERR_INVALID, w + "NULL argument");
    PpoNet n;
    std::string err;
    if (int rc = to_net<F>(net, true, n, err)) return fail(nullptr, rc, w + err);
    if (misaligned(scratch)) return fail(nullptr, CH_ERR_INVALID, w + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, 1, s);   // (only the partials are used: any scratch sized for this net holds them)
    const PpoHp h = F::hp(hp);
    hipStream_t st = (hipStream_t)stream;
    long long* step = reinterpret_cast<long long*>(step_dev);
    int np = 0;
    hipError_t e = ppo_launch_sumsq(n, grad_flat, scratch, s, step, &np, st);
    if (e == hipSuccess)   // (ch_*_train's Adam row)
        e = ppo_launch_adam(ppo_plan(F::kFlavour, false, false, false, false), n, &h, nullptr, grad_flat, m, v, step, scratch, s, np, 1, nullptr, st);
    return e == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, w + "launch: " + hipGetErrorString(e));
}

// The three training entries.  kTrainLog: `stats` is required and wider -- Sb3 (ch_ppo_train_log): CH_PPO_LOG_STATS,
// with approx_kl and clip_fraction; Rllib (ch_marl_ppo_train_log): CH_MARL_PPO_LOG_STATS, with vf_loss_unclipped,
// total_loss and vf_explained_var.  kTrainOpt (ch_ppo_train_opt, Sb3 only): kTrainLog through the option kernels, with
// `opts` and rows of CH_PPO_OPT_STATS.  ppo_plan has the kernels and the width of each.
enum TrainKind { kTrain, kTrainLog, kTrainOpt };

template <class F>
int train(TrainKind kind, const typename F::Net* net, const typename F::Hparams* hp, const typename F::Data* data,
          const ch_ppo_opts* opts, const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v,
          int64_t* step_dev, float* stats, float* scratch, void* stream) {
    const std::string w = who<F>(kind == kTrainOpt ? "train_opt" : kind == kTrainLog ? "train_log" : "train");
    if (!net || !hp || !data || !idx || !m || !v || !step_dev || !scratch || (kind != kTrain && !stats))
        return fail(nullptr, CH_ERR_INVALID, w + "NULL argument");
    PpoOpt o{};
    if (kind == kTrainOpt) {
        if (!opts) return fail(nullptr, CH_ERR_INVALID, w + "NULL opts");
        if (opts->clip_range_vf > 0.0 && !opts->old_values) return fail(nullptr, CH_ERR_INVALID, w + "clip_range_vf > 0 needs old_values");
        if (opts->target_kl > 0.0 && !opts->stop_dev) return fail(nullptr, CH_ERR_INVALID, w + "target_kl > 0 needs stop_dev");
        o = PpoOpt{opts->target_kl, opts->clip_range_vf, opts->old_values, opts->stop_dev};
    }
    const PpoPlan p = ppo_plan(F::kFlavour, kind == kTrainLog, kind == kTrainOpt, o.target_kl > 0.0, o.clip_range_vf > 0.0);
    if (p.fb == kPpoNone) return fail(nullptr, CH_ERR_UNSUPPORTED, w + "no such update for this flavour");
    PpoNet n;
    PpoData d;
    std::string err;
    int rc;
    if ((rc = to_net<F>(net, true, n, err)) || (rc = to_data<F>(data, hp, d, err))) return fail(nullptr, rc, w + err);
    if (n_idx < 1 || batch_size < 1 || batch_size > kMaxBatch) return fail(nullptr, CH_ERR_INVALID, w + "n_idx >= 1 and batch_size 1..2^24 required");
    if (misaligned(scratch)) return fail(nullptr, CH_ERR_INVALID, w + "scratch must be 16-byte aligned");
    PpoScratch s;
    ppo_scratch_layout(n, std::min(batch_size, n_idx), s);   // one layout for every step, the partial last one included
    const PpoHp h = F::hp(hp);
    hipStream_t st = (hipStream_t)stream;
    float* grad = scratch + s.grad;
    long long* step = reinterpret_cast<long long*>(step_dev);
    int64_t k = 0;
    for (int64_t j = 0; j < n_idx; j += batch_size, ++k) {
        const int64_t batch = std::min(batch_size, n_idx - j);
        const PpoScratch sj = ppo_scratch_for(s, batch);
        int np = 0;
        hipError_t e = ppo_launch_grad(p, n, h, d, &o, reinterpret_cast<const long long*>(idx) + j, batch, grad, scratch, sj, step, &np, st);
        if (e == hipSuccess)
            e = ppo_launch_adam(p, n, &h, &o, grad, m, v, step, scratch, sj, np, batch, stats ? stats + p.n_stats * k : nullptr, st);
        if (e != hipSuccess) return fail(nullptr, CH_ERR_DEVICE, w + "launch: " + hipGetErrorString(e));
    }
    return CH_OK;
}

bool same_arch(const PpoNet& a, const PpoNet& b) {
    if (a.obs_dim != b.obs_dim || a.act_dim != b.act_dim) return false;
    for (int ni = 0; ni < 2; ++ni) {
        if (a.net[ni].layers != b.net[ni].layers) return false;
        for (int i = 0; i <= a.net[ni].layers; ++i)
            if (a.net[ni].dims[i] != b.net[ni].dims[i]) return false;
    }
    return true;
}

constexpr int kPopSlots = 2;      // staging and tables a call may fill while an earlier call's copy is still queued
constexpr int kPopVariants = 2;   // a table for the full minibatches, one for a last, partial minibatch

}  // namespace

// The population's argument tables (see include/cattleherd.h).  A slot is one pinned host block and one device block
// of the same layout, [variant][fb | dw | adam][max_members], and the event recorded behind the slot's latest copy.
struct ch_ppo_pop {
    int max_members = 0, device = 0;
    size_t bytes = 0;                    // of a slot
    size_t off[kPopVariants][3] = {};    // the tables' places in it
    struct Slot { char* host = nullptr; char* dev = nullptr; hipEvent_t copied = nullptr; bool queued = false; } slot[kPopSlots];
    unsigned calls = 0;
    PpoPopTables tables(char* base, int variant) const {
        return {base + off[variant][0], base + off[variant][1], base + off[variant][2]};
    }
};

namespace {

int pop_free(ch_ppo_pop* pop) {
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
    return bad == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, std::string("ch_ppo_pop_destroy: ") + hipGetErrorString(bad));
}

// the device current while the object's calls run, the caller's again afterwards
struct DeviceScope {
    int prev = -1;
    hipError_t err;
    explicit DeviceScope(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) err = hipSetDevice(device); else if (err == hipSuccess) prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

extern "C" {

int ch_ppo_pop_create(int32_t max_members, int32_t device, ch_ppo_pop** out) {
    const std::string w = "ch_ppo_pop_create: ";
    if (!out) return fail(nullptr, CH_ERR_INVALID, w + "NULL argument");
    *out = nullptr;
    if (max_members < 1 || max_members > 65535) return fail(nullptr, CH_ERR_INVALID, w + "max_members must be 1..65535");   // (a grid dimension)
    DeviceScope scope(device);
    if (scope.err != hipSuccess) return fail(nullptr, CH_ERR_DEVICE, w + "device: " + hipGetErrorString(scope.err));
    ch_ppo_pop* pop = new ch_ppo_pop;
    pop->max_members = max_members; pop->device = device;
    const PpoPopSizes sz = ppo_pop_entry_sizes();
    const size_t each[3] = {sz.fb, sz.dw, sz.adam};
    for (int v = 0; v < kPopVariants; ++v)
        for (int t = 0; t < 3; ++t) {
            pop->off[v][t] = pop->bytes;
            pop->bytes += (each[t] * (size_t)max_members + 255) / 256 * 256;
        }
    for (auto& s : pop->slot) {
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&s.host), pop->bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s.dev), pop->bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)pop_free(pop);
            return fail(nullptr, e == hipErrorOutOfMemory ? CH_ERR_NOMEM : CH_ERR_DEVICE, w + hipGetErrorString(e));
        }
    }
    *out = pop;
    return CH_OK;
}

int ch_ppo_pop_destroy(ch_ppo_pop* pop) {
    if (!pop) return fail(nullptr, CH_ERR_INVALID, "ch_ppo_pop_destroy: NULL argument");
    DeviceScope scope(pop->device);
    return pop_free(pop);
}

int ch_ppo_train_pop(ch_ppo_pop* pop, const ch_ppo_member* members, int32_t n_members, int64_t n_idx, int64_t batch_size,
                     void* stream) {
    const std::string w = "ch_ppo_train_pop: ";
    if (!pop || !members) return fail(nullptr, CH_ERR_INVALID, w + "NULL argument");
    if (n_members < 1 || n_members > pop->max_members)
        return fail(nullptr, CH_ERR_INVALID, w + "n_members must be 1..max_members (" + std::to_string(pop->max_members) + ")");
    if (n_idx < 1 || batch_size < 1 || batch_size > kMaxBatch) return fail(nullptr, CH_ERR_INVALID, w + "n_idx >= 1 and batch_size 1..2^24 required");
    // every member as train<Sb3>(kTrainOpt) checks it, then what the members must agree on; nothing is launched before
    std::vector<PpoMember> mb((size_t)n_members);
    for (int i = 0; i < n_members; ++i) {
        const ch_ppo_member& c = members[i];
        const std::string wi = w + "member " + std::to_string(i) + ": ";
        if (!c.idx || !c.m || !c.v || !c.step_dev || !c.scratch || !c.stats) return fail(nullptr, CH_ERR_INVALID, wi + "NULL argument (idx, m, v, step_dev, stats and scratch are required)");
        if (c.opts.clip_range_vf > 0.0 && !c.opts.old_values) return fail(nullptr, CH_ERR_INVALID, wi + "clip_range_vf > 0 needs old_values");
        if (c.opts.target_kl > 0.0 && !c.opts.stop_dev) return fail(nullptr, CH_ERR_INVALID, wi + "target_kl > 0 needs stop_dev");
        PpoMember& m = mb[(size_t)i];
        std::string err;
        int rc;
        if ((rc = to_net<Sb3>(&c.net, true, m.n, err)) || (rc = to_data<Sb3>(&c.data, &c.hp, m.d, err))) return fail(nullptr, rc, wi + err);
        if (misaligned(c.scratch)) return fail(nullptr, CH_ERR_INVALID, wi + "scratch must be 16-byte aligned");
        m.hp = Sb3::hp(&c.hp);
        m.o = PpoOpt{c.opts.target_kl, c.opts.clip_range_vf, c.opts.old_values, c.opts.stop_dev};
        m.idx = reinterpret_cast<const long long*>(c.idx);
        m.m = c.m; m.v = c.v; m.step_dev = reinterpret_cast<long long*>(c.step_dev);
        m.stats = c.stats; m.scratch = c.scratch;
    }
    for (int i = 1; i < n_members; ++i) {
        const std::string wi = w + "member " + std::to_string(i) + ": ";
        if (!same_arch(mb[0].n, mb[(size_t)i].n)) return fail(nullptr, CH_ERR_UNSUPPORTED, wi + "architecture differs from member 0's");
        if (mb[0].d.rows != mb[(size_t)i].d.rows) return fail(nullptr, CH_ERR_UNSUPPORTED, wi + "data rows differ from member 0's");
        if ((mb[0].o.clip_range_vf > 0.0) != (mb[(size_t)i].o.clip_range_vf > 0.0))
            return fail(nullptr, CH_ERR_UNSUPPORTED, wi + "clip_range_vf must be set for every member or for none");
    }
    DeviceScope scope(pop->device);
    if (scope.err != hipSuccess) return fail(nullptr, CH_ERR_DEVICE, w + "device: " + hipGetErrorString(scope.err));
    hipStream_t st = (hipStream_t)stream;
    PpoScratch s;
    ppo_scratch_layout(mb[0].n, std::min(batch_size, n_idx), s);   // one layout for every member and step
    const int64_t full = std::min(batch_size, n_idx), last = n_idx % full;   // last: the partial minibatch's rows, or 0
    // the staging slot: not before the copy that read it last is done (two calls ago; the device block behind it is
    // read by that call's launches, which this call's copy follows in the stream)
    ch_ppo_pop::Slot& slot = pop->slot[pop->calls++ % kPopSlots];
    if (slot.queued) {
        if (hipError_t e = hipEventSynchronize(slot.copied)) return fail(nullptr, CH_ERR_DEVICE, w + "staging: " + hipGetErrorString(e));
        slot.queued = false;
    }
    PpoPopGeom geom[kPopVariants] = {};
    for (int v = 0; v < (last ? 2 : 1); ++v) {
        const int64_t batch = v ? last : full;
        const PpoPopTables host = pop->tables(slot.host, v);
        for (int i = 0; i < n_members; ++i) ppo_pop_fill(host, i, mb[(size_t)i], batch, ppo_scratch_for(s, batch), &geom[v]);
    }
    hipError_t e = hipMemcpyAsync(slot.dev, slot.host, pop->bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(slot.copied, st);
    if (e != hipSuccess) return fail(nullptr, CH_ERR_DEVICE, w + "tables: " + hipGetErrorString(e));
    slot.queued = true;
    const PpoPopPlan p = ppo_pop_plan(mb[0].o.clip_range_vf > 0.0);
    int64_t k = 0;
    for (int64_t j = 0; j < n_idx; j += batch_size, ++k) {
        const int v = n_idx - j < full ? 1 : 0;
        e = ppo_pop_launch(p, pop->tables(slot.dev, v), geom[v], n_members, j, CH_PPO_OPT_STATS * k, st);
        if (e != hipSuccess) return fail(nullptr, CH_ERR_DEVICE, w + "launch: " + hipGetErrorString(e));
    }
    return CH_OK;
}

int64_t ch_ppo_param_count(const ch_ppo_net* net) { return param_count<Sb3>(net); }
int64_t ch_ppo_scratch_size(const ch_ppo_net* net, int64_t batch_size) { return scratch_size<Sb3>(net, batch_size); }

int ch_ppo_grad(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                int64_t batch, float* grad_flat, float* stats4, float* scratch, void* stream) {
    return grad<Sb3>(net, hp, data, idx, batch, grad_flat, stats4, scratch, stream);
}

int ch_ppo_adam(const ch_ppo_net* net, const ch_ppo_hparams* hp, const float* grad_flat, float* m, float* v,
                int64_t* step_dev, float* scratch, void* stream) {
    return adam<Sb3>(net, hp, grad_flat, m, v, step_dev, scratch, stream);
}

int ch_ppo_train(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                 int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev, float* stats, float* scratch,
                 void* stream) {
    return train<Sb3>(kTrain, net, hp, data, nullptr, idx, n_idx, batch_size, m, v, step_dev, stats, scratch, stream);
}

int ch_ppo_train_log(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const int64_t* idx,
                     int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev, float* stats, float* scratch,
                     void* stream) {
    return train<Sb3>(kTrainLog, net, hp, data, nullptr, idx, n_idx, batch_size, m, v, step_dev, stats, scratch, stream);
}

int ch_ppo_train_opt(const ch_ppo_net* net, const ch_ppo_hparams* hp, const ch_ppo_data* data, const ch_ppo_opts* opts,
                     const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev,
                     float* stats, float* scratch, void* stream) {
    return train<Sb3>(kTrainOpt, net, hp, data, opts, idx, n_idx, batch_size, m, v, step_dev, stats, scratch, stream);
}

int64_t ch_marl_ppo_param_count(const ch_marl_ppo_net* net) { return param_count<Rllib>(net); }
int64_t ch_marl_ppo_scratch_size(const ch_marl_ppo_net* net, int64_t batch_size) { return scratch_size<Rllib>(net, batch_size); }

int ch_marl_ppo_grad(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                     const int64_t* idx, int64_t batch, float* grad_flat, float* stats5, float* scratch, void* stream) {
    return grad<Rllib>(net, hp, data, idx, batch, grad_flat, stats5, scratch, stream);
}

int ch_marl_ppo_adam(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const float* grad_flat, float* m, float* v,
                     int64_t* step_dev, float* scratch, void* stream) {
    return adam<Rllib>(net, hp, grad_flat, m, v, step_dev, scratch, stream);
}

int ch_marl_ppo_train(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                      const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev,
                      float* stats, float* scratch, void* stream) {
    return train<Rllib>(kTrain, net, hp, data, nullptr, idx, n_idx, batch_size, m, v, step_dev, stats, scratch, stream);
}

int ch_marl_ppo_train_log(const ch_marl_ppo_net* net, const ch_marl_ppo_hparams* hp, const ch_marl_ppo_data* data,
                          const int64_t* idx, int64_t n_idx, int64_t batch_size, float* m, float* v, int64_t* step_dev,
                          float* stats, float* scratch, void* stream) {
    return train<Rllib>(kTrainLog, net, hp, data, nullptr, idx, n_idx, batch_size, m, v, step_dev, stats, scratch, stream);
}

// Internal (tests / diagnostics), host only: ppo_plan (ch_ppo.h) for a base flavour (0 SB3, 1 RLlib) and the four
// switches -- the call has options, its KL gate is armed, its value clip is on -- as out = {fb, dw, adam rows of the
// kernel table, update bits, statistics-row width, kernels take the option structs}; CH_ERR_UNSUPPORTED for a
// combination that does not exist.
int ch__ppo_plan(int32_t flavour, int32_t log_stats, int32_t opts, int32_t gate, int32_t vclip, int32_t out[6]) {
    const PpoPlan p = ppo_plan(flavour, log_stats != 0, opts != 0, gate != 0, vclip != 0);
    if (!out || p.fb == kPpoNone) return fail(nullptr, out ? CH_ERR_UNSUPPORTED : CH_ERR_INVALID, "ch__ppo_plan: no such update");
    const int32_t v[6] = {p.fb, p.dw, p.adam, p.update, p.n_stats, p.opts};
    std::copy(v, v + 6, out);
    return CH_OK;
}

// Internal: row `kernel` of the update's kernel table (ch_ppo.hip kPpoTable), its name; NULL past the table.
const char* ch__ppo_kernel(int32_t kernel) { return ppo_kernel_name(kernel); }

// Internal, host only: ppo_pop_plan (ch_ppo.h) for (value clip on) as out = {fb, dw, adam rows of the population
// kernels' table}, and row `kernel` of that table (ch_ppo.hip kPpoPopTable), its name; NULL outside the table.
int ch__ppo_pop_plan(int32_t vclip, int32_t out[3]) {
    if (!out) return fail(nullptr, CH_ERR_INVALID, "ch__ppo_pop_plan: NULL argument");
    const PpoPopPlan p = ppo_pop_plan(vclip != 0);
    out[0] = p.fb; out[1] = p.dw; out[2] = p.adam;
    return CH_OK;
}
const char* ch__ppo_pop_kernel(int32_t kernel) { return ppo_pop_kernel_name(kernel); }

// Internal: the minibatch step launched last in this process (host record, no device work): out = {fb, dw, adam rows,
// the Adam launch's update bits, its grid}.  ch_*_adam leaves {0, k_ppo_sumsq's row, ...}.
int ch__ppo_last_step(int32_t out[5]) {
    if (!out) return CH_ERR_INVALID;
    const int32_t v[5] = {g_ppo_last_step.fb, g_ppo_last_step.dw, g_ppo_last_step.adam, g_ppo_last_step.update, g_ppo_last_step.adam_grid};
    std::copy(v, v + 5, out);
    return CH_OK;
}

}  // extern "C"
