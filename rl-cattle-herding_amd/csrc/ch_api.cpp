// ch_api.cpp — C ABI of libcattleherd.so (see include/cattleherd.h).
//
// Host side: validates the configuration the way the reference's constructors do, owns the SoA
// state in HBM, and launches the kernels in ch_kernels.hip.  No host<->device traffic on the
// ch_step path: actions, observations, rewards and flags stay in caller-owned device buffers.
// The policy forwards and the rollout collections are in ch_api_policy.cpp; both share ch_handle.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ch_handle.h"
#include "ch_spawn_table.inc"

using namespace ch;

// the message of a failure without a handle (ch_handle.h)
thread_local std::string g_create_err;

// episode_length per curriculum level (curriculum_learning.py:24-182)
static const double kEpisodeLen[8] = {40, 40, 40, 40, 80, 40, 80, 80};

// --------------------------------------------------------------------------------------------
// Spawn table.  Cows 0..15 of every scenario come from config/cattle_positions.yaml (the
// reference's only table, BaseAviary.py:88-94, 600-637).  For num_cattle > 16 (beyond what the
// reference can run, BaseAviary.py:611,719) extra cows are drawn around the scenario's herd
// centroid with the generator's rules (utils/cattle_spawn.py:5-12: min spacing 0.8, uniform
// offsets), the offset box widened by 1.25 sqrt(cows/16), rounded to 3 decimals, from a fixed-seed
// splitmix64 stream — deterministic and identical for every caller.
// --------------------------------------------------------------------------------------------
static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<double> make_spawn_table(int cows) {
    const int S = CH_SPAWN_SCENARIOS, C0 = CH_SPAWN_COWS;
    const int C = std::max(cows, C0);
    std::vector<double> t((size_t)S * C * 2);
    for (int s = 0; s < S; ++s) {
        double cx = 0, cy = 0;
        for (int j = 0; j < C0; ++j) {
            t[((size_t)s * C + j) * 2] = CH_SPAWN_TABLE[(s * C0 + j) * 2];
            t[((size_t)s * C + j) * 2 + 1] = CH_SPAWN_TABLE[(s * C0 + j) * 2 + 1];
            cx += CH_SPAWN_TABLE[(s * C0 + j) * 2];
            cy += CH_SPAWN_TABLE[(s * C0 + j) * 2 + 1];
        }
        cx /= C0; cy /= C0;
        uint64_t st = 0xC0FFEEull * (s + 1);
        double half = 2.5 * std::sqrt((double)C / C0), mind = 0.8;
        for (int j = C0; j < C; ++j) {
            for (int attempt = 0;; ++attempt) {
                if (attempt > 0 && attempt % 2000 == 0) mind *= 0.95;
                double ox = ((splitmix(st) >> 11) * (1.0 / 9007199254740992.0) * 2 - 1) * half;
                double oy = ((splitmix(st) >> 11) * (1.0 / 9007199254740992.0) * 2 - 1) * half;
                double x = std::round((cx + ox) * 1000.0) / 1000.0, y = std::round((cy + oy) * 1000.0) / 1000.0;
                bool ok = true;
                for (int k = 0; k < j && ok; ++k) {
                    double dx = x - t[((size_t)s * C + k) * 2], dy = y - t[((size_t)s * C + k) * 2 + 1];
                    ok = std::sqrt(dx * dx + dy * dy) >= mind;
                }
                if (ok) { t[((size_t)s * C + j) * 2] = x; t[((size_t)s * C + j) * 2 + 1] = y; break; }
            }
        }
    }
    return t;
}

// CattleSpacingRewardFunction (CattleAviary.py:572-592), r > r0 branch: C = f(r0) / exp(-lambda r0) is the
// same number on every call; evaluated once here with the reference's expression.
static double cattle_spacing_cc() {
    const double A = 1.2, B = 2.1, C = 3.3, K = 0.2, D = -1, R0 = 1.3, LAM = 0.8;
    volatile double r0 = R0;   // evaluate at run time with the host libm, as the reference (and the oracle) do
    double fr0 = A * std::exp(-((r0 - D) * (r0 - D)) / (2 * (C * C))) - B * std::exp(-(r0 * r0) / (2 * (K * K)));
    return fr0 / std::exp(-LAM * r0);
}

// GND_EFF_H_CLIP (BaseAviary.py:163-173): 0.25 r_prop sqrt(15 MAX_RPM^2 KF c_gnd / MAX_THRUST), cf2x.urdf:5
static double gnd_eff_h_clip() {
    const double G = 9.8, MASS = 0.027, KF = 3.16e-10, T2W = 2.25, C = 11.36859, PR = 2.31348e-2;
    const double max_rpm = std::sqrt((T2W * (G * MASS)) / (4 * KF));
    const double max_thrust = 4 * KF * (max_rpm * max_rpm);
    return 0.25 * PR * std::sqrt((15 * (max_rpm * max_rpm) * KF * C) / max_thrust);
}

template <class R>
static StepParams<R> params(ch_handle* h) {
    StepParams<R> p{};
    const ch_config& c = h->cfg;
    p.E = (int)h->E; p.NC = h->NC; p.M = h->M; p.mode = c.mode; p.rows = h->rows;
    p.min_drones = c.min_drones; p.max_drones = c.max_drones; p.ctrl_freq = c.ctrl_freq;
    p.substeps = c.pyb_freq / c.ctrl_freq; p.compat = c.compat; p.torque_world = c.torque_world; p.gyro = c.gyro;
    p.link_lag = c.link_lag;
    p.marl_wrapper = c.marl_wrapper;
    p.episode_len = h->episode_len; p.damping = c.damping;
    p.dt_ctrl = 1.0 / c.ctrl_freq; p.dt = 1.0 / c.pyb_freq;
    p.k0 = (uint32_t)c.seed; p.k1 = (uint32_t)(c.seed >> 32);
    p.env_off = c.env_id_offset;
    p.cs_cc = cattle_spacing_cc();
    p.drone = (R*)h->drone; p.rpy = (R*)h->rpy; p.stale = h->stale; p.obs_tag = h->obs_tag; p.cattle = (R*)h->cattle; p.envr = (R*)h->envr; p.envi = h->envi;
    p.pos64 = h->pos64; p.cpos64 = h->cpos64; p.prev64 = h->prev64;
    p.metrics = h->metrics; p.spawn = h->spawn; p.n_scen = h->n_scen; p.n_cows = h->n_cows;
    p.debug = h->debug;
    p.phase_mask = h->ov.phase_mask;
    p.G = h->plan.G; p.P = h->P; p.pairs = h->pairs; p.pw = h->plan.pw; p.sep = h->plan.sep;
    p.tstamp = h->tstamp;
    p.physics = c.physics; p.gnd_h_clip = gnd_eff_h_clip(); p.phys = (R*)h->phys;
    p.err = h->errw;
    p.evald = h->evald;
    return p;
}

// f(params<R>(h)) for the handle's precision
template <class F>
static auto with_params(ch_handle* h, F&& f) {
    return h->rsize == sizeof(double) ? f(params<double>(h)) : f(params<float>(h));
}

// Plans the handle's step under the overrides `ov` (ch_step_plan.h) and, when the planner takes them, stores both and
// sets the v2 step rows' once-per-device function attribute, outside any stream capture.  CH_ERR_INVALID /
// CH_ERR_UNSUPPORTED: the planner refused the overrides and the handle is as it was.
static int replan(ch_handle* h, const StepOverrides& ov) {
    const ch_config& c = h->cfg;
    const StepPlan pl = step_plan({c.mode, h->NC, h->M, c.precision, c.physics, h->E}, h->cus, h->lds_budget, ov);
    if (pl.error) return pl.error;
    h->plan = pl;
    h->ov = ov;
    hipError_t e = hipSuccess;
    if (pl.kernel == 2)
        e = with_params(h, [&](auto p) {
            hipError_t e2 = launch_step_v2(p, pl.step_row[0], pl.block, pl.lds, nullptr, false);
            if (e2 == hipSuccess && pl.step_row[1] != pl.step_row[0])
                e2 = launch_step_v2(p, pl.step_row[1], pl.block, pl.lds, nullptr, false);
            return e2;
        });
    return e == hipSuccess ? CH_OK : fail(h, CH_ERR_DEVICE, std::string("prepare_step(h): ") + hipGetErrorString(e));
}

extern "C" {

int ch_builtin_spawn_table(double* out, int32_t* scenarios, int32_t* cows) {
    if (scenarios) *scenarios = CH_SPAWN_SCENARIOS;
    if (cows) *cows = CH_SPAWN_COWS;
    if (out) std::memcpy(out, CH_SPAWN_TABLE, sizeof(CH_SPAWN_TABLE));
    return CH_OK;
}

int ch_spawn_table(int32_t cows, double* out, int32_t* scenarios, int32_t* out_cows) {
    std::vector<double> t = make_spawn_table(cows);
    int C = std::max(cows, (int)CH_SPAWN_COWS);
    if (scenarios) *scenarios = CH_SPAWN_SCENARIOS;
    if (out_cows) *out_cows = C;
    if (out) std::memcpy(out, t.data(), t.size() * sizeof(double));
    return CH_OK;
}

int ch_default_config(ch_config* c, int32_t mode, int32_t num_drones, int32_t num_cattle) {
    if (!c) return fail(nullptr, CH_ERR_INVALID, "ch_default_config: cfg is NULL");
    std::memset(c, 0, sizeof(*c));
    c->abi_version = CH_ABI_VERSION;
    c->mode = mode;
    c->num_drones = num_drones;
    c->num_cattle = num_cattle;
    c->min_drones = -1;
    c->max_drones = -1;
    c->curriculum_level = -1;
    c->ctrl_freq = 60;
    c->pyb_freq = 240;
    c->compat = 1;
    c->precision = CH_PREC_F64;
    c->torque_world = 1;
    c->gyro = 1;
    c->marl_wrapper = 1;
    c->damping = 0.04;
    c->seed = 0x5EEDull;
    c->env_id_offset = 0;
    c->spawn_table = nullptr;
    c->physics = CH_PHYS_PYB;
    c->eval_metrics = 1;
    c->link_lag = 1;
    return CH_OK;
}

const char* ch_last_error(const ch_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

constexpr size_t kParamsBytes = 1024;   // ch_step_n's device copy of StepParams

static void free_all(ch_handle* h) {
    void* ptrs[] = {h->drone, h->rpy, h->cattle, h->phys, h->envr, h->envi, h->metrics, h->spawn, h->pairs,
                    h->errw, h->mdev, h->stale, h->obs_tag, h->evald, h->rdn, h->rdv, h->pos64, h->cpos64, h->prev64,
                    h->d_params};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->mhost) (void)hipHostFree(h->mhost);
    const ch_rollout_state& ro = h->ro;   // the rollout's queue
    for (void* p : {(void*)ro.tv_obs, (void*)ro.tv_row, (void*)ro.tv_count, (void*)ro.tv_val})
        if (p) (void)hipFree(p);
    const ch_staging& sg = h->st;         // ch_outputs_to_host's staging
    for (void* p : {(void*)sg.count, (void*)sg.env, (void*)sg.stats, (void*)sg.obs})
        if (p) (void)hipFree(p);
    if (sg.count_host) (void)hipHostFree(sg.count_host);
    if (h->eval_host) (void)hipHostFree(h->eval_host);
}

}  // extern "C"

// the sticky device error word as a status (call after the stream has drained; ch_handle.h: ch_api_eval.cpp reports
// it too)
int device_status(ch_handle* h, int word) {
    if (!word) return CH_OK;
    h->err_seen = true;
    return fail(h, CH_ERR_DEVICE,
                "device error word " + std::to_string(word) +
                    ((word & CH_DEVERR_HANDOFF) ? ": a step kernel's LDS hand-off timed out (ch_step_sync.h lds_wait); "
                                                  "the results of that step are wrong"
                                                : "") +
                    ((word & CH_DEVERR_LOG_INDEX) ? ": an evaluator log's sel_env held an env index outside [0, E); "
                                                    "that entry was not logged"
                                                  : ""));
}

// ch_create in three parts: the configuration's checks (the reference constructors'), the device arrays with the state
// the constructors leave behind, and the step's plan.

// `level`, `mn`, `mx`: the curriculum level and the drone-count bounds with their defaults filled in
static int validate_config(const ch_config* c, int64_t n_envs, int& level, int& mn, int& mx) {
    if (c->abi_version != CH_ABI_VERSION) return fail(nullptr, CH_ERR_INVALID, "ch_create: abi_version mismatch");
    if (c->mode != CH_MODE_CTDE && c->mode != CH_MODE_MARL) return fail(nullptr, CH_ERR_INVALID, "ch_create: bad mode");
    if (c->physics < CH_PHYS_PYB || c->physics > CH_PHYS_DYN_RK4)
        return fail(nullptr, CH_ERR_INVALID, "ch_create: physics must be one of CH_PHYS_* (utils/enums.py:13-21)");
    if (n_envs <= 0 || n_envs > (1ll << 28)) return fail(nullptr, CH_ERR_INVALID, "ch_create: n_envs out of range");
    if (c->num_drones < 1 || c->num_drones > kNMax)
        return fail(nullptr, CH_ERR_INVALID, "ch_create: num_drones must be in [1, 12] (GLOBAL_MAX_NUM_DRONES)");
    if (c->num_cattle < 1 || c->num_cattle > kMMax)
        return fail(nullptr, CH_ERR_INVALID, "ch_create: num_cattle must be in [1, 64]");
    if (c->ctrl_freq <= 0 || c->pyb_freq <= 0 || c->pyb_freq % c->ctrl_freq != 0)
        return fail(nullptr, CH_ERR_INVALID, "[ERROR] in BaseAviary.__init__(), pyb_freq is not divisible by env_freq.");
    if (c->precision != CH_PREC_F64 && c->precision != CH_PREC_F32)
        return fail(nullptr, CH_ERR_INVALID, "ch_create: bad precision");
    level = c->curriculum_level < 0 ? (c->mode == CH_MODE_CTDE ? 7 : 0) : c->curriculum_level;
    if (level > 7) return fail(nullptr, CH_ERR_INVALID, "ch_create: curriculum_level must be in [0, 7]");
    mn = c->min_drones < 0 ? c->num_drones : c->min_drones;
    mx = c->max_drones < 0 ? c->num_drones : c->max_drones;
    if (mn < 1 || mx < mn || mx > c->num_drones)
        return fail(nullptr, CH_ERR_INVALID,
                    "ch_create: need 1 <= min_drones <= max_drones <= num_drones (the reference indexes "
                    "self.ctrl[k] sized by num_drones, BaseRLAviary.py:80)");
    if (c->compat && mn < 2)
        return fail(nullptr, CH_ERR_UNSUPPORTED,
                    "compat mode: the reference raises ValueError for a single drone (np.partition kth=1, "
                    "CattleAviary.py:234); use compat=0");
    if (c->spawn_table && (c->spawn_scenarios < 1 || c->spawn_cows < c->num_cattle))
        return fail(nullptr, CH_ERR_INVALID, "ch_create: spawn table smaller than num_cattle");
    return CH_OK;
}

#define CTRY(expr)                                                                                  \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            h->err = std::string(#expr) + ": " + hipGetErrorString(_e);                             \
            return _e;                                                                              \
        }                                                                                           \
    } while (0)

// the handle's device arrays, the spawn table and the cow-pair list; the failed call and its error in h->err
static hipError_t allocate_state(ch_handle* h) {
    const ch_config* c = &h->cfg;
    const int64_t E = h->E;
    CTRY(hipMalloc(&h->drone, h->rsize * kDroneComps * E * h->NC));
    CTRY(hipMalloc(&h->rpy, h->rsize * 3 * E * h->NC));
    CTRY(hipMalloc(&h->cattle, h->rsize * kCattleComps * E * h->M));
    CTRY(hipMalloc(&h->phys, h->rsize * kPhysComps * E * h->NC));
    CTRY(hipMemset(h->phys, 0, h->rsize * kPhysComps * E * h->NC));
    CTRY(hipMalloc(&h->envr, h->rsize * kEnvReal * E));
    if (h->rsize == sizeof(float)) {
        CTRY(hipMalloc(&h->pos64, sizeof(double) * 3 * E * h->NC));
        CTRY(hipMalloc(&h->cpos64, sizeof(double) * 2 * E * h->M));
        CTRY(hipMalloc(&h->prev64, sizeof(double) * E));
    }
    CTRY(hipMalloc(&h->envi, sizeof(int) * kEnvInt * E));
    CTRY(hipMalloc(&h->metrics, sizeof(double) * kMetricRows * E));
    CTRY(hipMalloc(&h->stale, 2 * (size_t)E));
    CTRY(hipMemset(h->stale, 1, 2 * (size_t)E));   // no Euler cache yet; obs bytes unknown
    CTRY(hipMalloc(&h->obs_tag, sizeof(unsigned long long) * (size_t)E));
    CTRY(hipMemset(h->obs_tag, 0, sizeof(unsigned long long) * (size_t)E));   // no buffer holds them
    if (c->eval_metrics) {
        CTRY(hipMalloc(&h->evald, sizeof(double) * E * h->NC));
        CTRY(hipMemset(h->evald, 0, sizeof(double) * E * h->NC));
    }
    CTRY(hipMalloc(&h->errw, sizeof(int)));
    CTRY(hipMemset(h->errw, 0, sizeof(int)));
    CTRY(hipMalloc(&h->mdev, sizeof(double) * (CH_METRIC_COUNT + 1)));
    CTRY(hipHostMalloc(&h->mhost, sizeof(double) * (CH_METRIC_COUNT + 1), hipHostMallocDefault));

    std::vector<double> table;
    if (c->spawn_table) {
        table.assign(c->spawn_table, c->spawn_table + (size_t)c->spawn_scenarios * c->spawn_cows * 2);
        h->n_scen = c->spawn_scenarios;
        h->n_cows = c->spawn_cows;
    } else {
        table = make_spawn_table(h->M);
        h->n_scen = CH_SPAWN_SCENARIOS;
        h->n_cows = std::max(h->M, (int)CH_SPAWN_COWS);
    }
    CTRY(hipMalloc(&h->spawn, table.size() * sizeof(double)));
    CTRY(hipMemcpy(h->spawn, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice));
    std::vector<uint16_t> pl((size_t)std::max(h->P, 1));
    for (int i = 0, r = 0; i < h->M; ++i)
        for (int j = i + 1; j < h->M; ++j) pl[r++] = (uint16_t)(i | (j << 8));
    CTRY(hipMalloc(&h->pairs, pl.size() * sizeof(uint16_t)));
    CTRY(hipMemcpy(h->pairs, pl.data(), pl.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return hipSuccess;
}

// initial state = what the constructors leave behind before the first reset():
// identity quaternions, zero PID state, spawn index advanced once by __init__'s _housekeeping.
static hipError_t initial_state(ch_handle* h) {
    const int64_t E = h->E;
    std::vector<double> dz((size_t)kDroneComps * E * h->NC, 0.0);
    for (int64_t i = 0; i < E * h->NC; ++i) {
        dz[(size_t)6 * E * h->NC + i] = 1.0;
        dz[(size_t)25 * E * h->NC + i] = 1.0;   // cached link frame: identity too
    }
    std::vector<int> ei((size_t)kEnvInt * E, 0);
    for (int64_t e = 0; e < E; ++e) {
        ei[4 * E + e] = h->start_level;
        ei[6 * E + e] = (int)((1 + h->cfg.env_id_offset + e) % h->n_scen);
    }
    std::vector<double> cz((size_t)kCattleComps * E * h->M, 0.0), rz((size_t)kEnvReal * E, 0.0);
    if (h->rsize == sizeof(double)) {
        CTRY(hipMemcpy(h->drone, dz.data(), dz.size() * 8, hipMemcpyHostToDevice));
        CTRY(hipMemcpy(h->cattle, cz.data(), cz.size() * 8, hipMemcpyHostToDevice));
        CTRY(hipMemcpy(h->envr, rz.data(), rz.size() * 8, hipMemcpyHostToDevice));
    } else {
        std::vector<float> f(dz.begin(), dz.end()), fc(cz.begin(), cz.end()), fr(rz.begin(), rz.end());
        CTRY(hipMemcpy(h->drone, f.data(), f.size() * 4, hipMemcpyHostToDevice));
        CTRY(hipMemcpy(h->cattle, fc.data(), fc.size() * 4, hipMemcpyHostToDevice));
        CTRY(hipMemcpy(h->envr, fr.data(), fr.size() * 4, hipMemcpyHostToDevice));
        CTRY(hipMemcpy(h->pos64, dz.data(), sizeof(double) * 3 * E * h->NC, hipMemcpyHostToDevice));
        CTRY(hipMemcpy(h->cpos64, cz.data(), sizeof(double) * 2 * E * h->M, hipMemcpyHostToDevice));
        CTRY(hipMemcpy(h->prev64, rz.data(), sizeof(double) * E, hipMemcpyHostToDevice));
    }
    CTRY(hipMemcpy(h->envi, ei.data(), ei.size() * sizeof(int), hipMemcpyHostToDevice));
    CTRY(hipMemset(h->metrics, 0, sizeof(double) * kMetricRows * E));
    return hipSuccess;
}

// what the planner plans for: the device's CU count and its LDS per CU, capped at what the step kernels opt in to
static hipError_t device_limits(ch_handle* h) {
    int cus = 256, lds_max = 64 * 1024;
    CTRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, h->device) != hipSuccess)
        lds_max = 64 * 1024;
    h->cus = cus;
    h->lds_budget = std::min<size_t>((size_t)lds_max, kStepLdsMax);
    return hipSuccess;
}
#undef CTRY

extern "C" {

int ch_create(const ch_config* c, int64_t n_envs, int32_t device, ch_handle** out) {
    if (!c || !out) return fail(nullptr, CH_ERR_INVALID, "ch_create: NULL argument");
    *out = nullptr;
    int level = 0, mn = 0, mx = 0;
    if (int rc = validate_config(c, n_envs, level, mn, mx)) return rc;
    int dev_count = 0;
    hipError_t ge = hipGetDeviceCount(&dev_count);
    if (ge != hipSuccess || dev_count == 0)
        return fail(nullptr, CH_ERR_DEVICE, std::string("ch_create: no HIP device: ") + hipGetErrorString(ge));
    if (device < 0 || device >= dev_count) return fail(nullptr, CH_ERR_INVALID, "ch_create: bad device index");

    ch_handle* h = new (std::nothrow) ch_handle();
    if (!h) return fail(nullptr, CH_ERR_NOMEM, "ch_create: out of host memory");
    h->cfg = *c;
    h->cfg.curriculum_level = level;
    h->cfg.min_drones = mn;
    h->cfg.max_drones = mx;
    h->E = n_envs;
    h->device = device;
    h->NC = c->num_drones;
    h->M = c->num_cattle;
    h->rows = c->mode == CH_MODE_CTDE ? 12 : c->num_drones;
    h->K = c->mode == CH_MODE_CTDE ? 1 : c->num_drones;
    int need = std::max(h->NC, h->M);
    h->team = need <= 16 ? 16 : (need <= 32 ? 32 : 64);
    h->start_level = level;
    h->episode_len = kEpisodeLen[level];
    h->rsize = c->precision == CH_PREC_F64 ? sizeof(double) : sizeof(float);
    h->P = h->M * (h->M - 1) / 2;
    {   // ch_rollout_collect's path: the environment's choice, ch__set_rollout_path overrides it per handle
        const char* v = getenv("CH_ROLLOUT_COPY");
        const char* k = getenv("CH_ROLLOUT_STORE_KERNEL");
        const char* f = getenv("CH_FUSED_ACTOR");
        h->ro.path = ((v && v[0] == '1') ? 1 : 0) | ((k && k[0] == '1') ? 2 : 0) | ((f && f[0] == '1') ? 4 : 0);
    }

    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) h->err = std::string("hipSetDevice(device): ") + hipGetErrorString(e);
    if (e == hipSuccess) e = allocate_state(h);
    if (e == hipSuccess) e = initial_state(h);
    if (e == hipSuccess) e = device_limits(h);
    int rc = e == hipSuccess ? CH_OK : e == hipErrorOutOfMemory ? CH_ERR_NOMEM : CH_ERR_DEVICE;
    if (rc == CH_OK) rc = replan(h, StepOverrides{});   // (the rules alone always plan)
    if (rc != CH_OK) {
        free_all(h);
        g_create_err = h->err;
        delete h;
        return rc;
    }
    *out = h;
    return CH_OK;
}

int ch_destroy(ch_handle* h) {
    if (!h) return CH_OK;
    (void)hipSetDevice(h->device);
    free_all(h);
    delete h;
    return CH_OK;
}

int ch_shape(const ch_handle* h, int64_t* n_envs, int32_t* obs_rows, int32_t* obs_cols, int32_t* reward_cols) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_shape: NULL handle");
    if (n_envs) *n_envs = h->E;
    if (obs_rows) *obs_rows = h->rows;
    if (obs_cols) *obs_cols = 86;
    if (reward_cols) *reward_cols = h->K;
    return CH_OK;
}

// A full reset rebuilds every env, so the results a failed hand-off spoiled are gone and the sticky device error word
// is cleared.  The word is read first (a stream sync: full resets are rare): if it was set and no ch_sync /
// ch_metrics / ch_get_state has reported it yet, the reset still happens but returns CH_ERR_DEVICE, so that the
// failure of the steps before it is never lost silently.
static int clear_error_word(ch_handle* h, hipStream_t st, const char* who) {
    int word = 0;
    HIP_TRY(h, hipStreamSynchronize(st));
    HIP_TRY(h, hipMemcpy(&word, h->errw, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemsetAsync(h->errw, 0, sizeof(int), st));
    const bool unseen = word && !h->err_seen;
    h->err_seen = false;
    if (unseen)
        return fail(h, CH_ERR_DEVICE, std::string(who) + ": the envs were reset, but the steps before it had set device "
                                          "error word " + std::to_string(word) + " (never reported: the results of "
                                          "those steps are wrong); the word is now cleared");
    return CH_OK;
}

}  // extern "C"

// ch_reset (`who`, no draws) and ch_reset_with (optional draws from host arrays)
static int reset_envs(ch_handle* h, const uint8_t* mask_dev, const int32_t* num_drones, const double* cow_vel,
                      float* obs_dev, void* stream, const std::string& who, bool injected) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, who + ": NULL handle");
    if (!obs_dev) return fail(h, CH_ERR_INVALID, who + ": obs is NULL");
    if (num_drones)
        for (int64_t e = 0; e < h->E; ++e)
            if (num_drones[e] < 1 || num_drones[e] > h->NC)
                return fail(h, CH_ERR_INVALID,
                            who + ": NUM_DRONES " + std::to_string(num_drones[e]) + " outside [1, num_drones] "
                            "(the reference indexes controllers sized by num_drones, BaseRLAviary.py:80)");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (num_drones) {
        if (!h->rdn) HIP_TRY(h, hipMalloc(&h->rdn, sizeof(int) * h->E));
        HIP_TRY(h, hipMemcpyAsync(h->rdn, num_drones, sizeof(int) * h->E, hipMemcpyHostToDevice, st));
    }
    if (cow_vel) {
        if (!h->rdv) HIP_TRY(h, hipMalloc(&h->rdv, sizeof(double) * h->E * h->M * 2));
        HIP_TRY(h, hipMemcpyAsync(h->rdv, cow_vel, sizeof(double) * h->E * h->M * 2, hipMemcpyHostToDevice, st));
    }
    const hipError_t e = with_params(h, [&](auto p) {
        p.reset_mask = mask_dev; p.obs = obs_dev;
        p.reset_n = num_drones ? h->rdn : nullptr; p.reset_vel = cow_vel ? h->rdv : nullptr;
        return launch_reset(p, h->team, st);
    });
    if (e != hipSuccess) return fail(h, CH_ERR_DEVICE, who + " launch: " + hipGetErrorString(e));
    if (injected) HIP_TRY(h, hipStreamSynchronize(st));   // the host arrays may be reused as soon as this returns
    if (!mask_dev) h->obs_zero_ptr = obs_dev;                    // every block written in full
    else if (h->obs_zero_ptr != obs_dev) h->obs_zero_ptr = nullptr;   // some blocks of obs_dev unknown
    return mask_dev ? CH_OK : clear_error_word(h, st, who.c_str());
}

extern "C" {

int ch_reset(ch_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream) {
    return reset_envs(h, mask_dev, nullptr, nullptr, obs_dev, stream, "ch_reset", false);
}

int ch_reset_with(ch_handle* h, const uint8_t* mask_dev, const int32_t* num_drones, const double* cow_vel,
                  float* obs_dev, void* stream) {
    return reset_envs(h, mask_dev, num_drones, cow_vel, obs_dev, stream, "ch_reset_with", true);
}

}  // extern "C"

template <class P>
static void fill_step(const ch_handle* h, const ch_step_io* io, P& p) {
    p.actions = io->actions; p.actions_out = io->actions_out; p.obs = io->obs; p.reward = io->reward;
    p.term = io->terminated; p.trunc = io->truncated; p.terminal_obs = io->terminal_obs;
    p.agent_active = io->agent_active; p.reset_happened = io->reset_happened; p.flags = io->flags;
    p.episode_stats = io->episode_stats;
    p.obs_full = io->obs != h->obs_zero_ptr;
}

// ch_rollout_collect's fused step (ch_handle.h)
hipError_t step_actor(ch_handle* h, const ch_step_io* io, hipStream_t st, const MlpArgs& fa, const RolloutArgs& ro,
                      bool launch) {
    const StepPlan& pl = h->plan;
    const int row = pl.actor_row[io->terminal_obs != nullptr];
    if (row == kStepNoRow) return hipErrorNotSupported;
    StepParams<double> p = params<double>(h);
    fill_step(h, io, p);
    const hipError_t e = launch_step_v2_actor(p, row, pl.block, pl.lds, st, fa, ro, launch);
    if (e == hipSuccess && launch) { h->obs_zero_ptr = io->obs; ++h->ro.fused_steps; }
    return e;
}

// what ch_step and ch_step_n ask of their io
static int validate_step_io(ch_handle* h, const ch_step_io* io, const char* who) {
    auto bad = [&](const char* what) { return fail(h, CH_ERR_INVALID, std::string(who) + ": " + what); };
    if (!io) return bad("io is NULL");
    if (!io->obs || !io->reward || !io->terminated || !io->truncated)
        return bad("obs, reward, terminated and truncated are required");
    if (!(io->flags & CH_STEP_RANDOM_ACTIONS) && !io->actions)
        return bad("actions is NULL (and CH_STEP_RANDOM_ACTIONS not set)");
    if (io->actions && (reinterpret_cast<uintptr_t>(io->actions) & 15)) return bad("actions must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(io->obs) & 15) ||
        (io->terminal_obs && (reinterpret_cast<uintptr_t>(io->terminal_obs) & 15)))
        return bad("obs buffers must be 16-byte aligned");
    return CH_OK;
}

// one step of a validated io on the handle's device (ch_step; ch_step_n's plain steps)
static int step_once(ch_handle* h, const ch_step_io* io, hipStream_t st) {
    const StepPlan& pl = h->plan;
    const hipError_t e = with_params(h, [&](auto p) {
        fill_step(h, io, p);
        return pl.kernel == 2 ? launch_step_v2(p, pl.step_row[io->terminal_obs != nullptr], pl.block, pl.lds, st)
                              : launch_step(p, h->team, st);
    });
    if (e != hipSuccess) return fail(h, CH_ERR_DEVICE, std::string("ch_step launch: ") + hipGetErrorString(e));
    h->obs_zero_ptr = (h->ov.phase_mask & 8) ? nullptr : io->obs;
    // Which buffer holds each env's constant-zero obs bytes is also tracked on the device, per env: the step kernels
    // record the address they wrote (StepParams::obs_tag) and write an env's block in full when the buffer they are
    // given is not that one (k_step2 and k_env compare p.obs_tag[e] with p.obs), so a HIP graph captured on one
    // buffer and replayed after steps into another stays exact.  A new tensor at a recycled address is the caller's
    // to flag (HerdBatch.step(obs_out=...) calls invalidate_obs when the tensor changes).
    return CH_OK;
}

extern "C" {

int ch_step(ch_handle* h, const ch_step_io* io, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_step: NULL handle");
    if (int rc = validate_step_io(h, io, "ch_step")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return step_once(h, io, (hipStream_t)stream);
}

int ch_step_n(ch_handle* h, const ch_step_io* io, int32_t n_steps, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_step_n: NULL handle");
    if (n_steps < 1) return fail(h, CH_ERR_INVALID, "ch_step_n: n_steps must be >= 1");
    int done = 0, rc = validate_step_io(h, io, "ch_step_n");
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const StepPlan& pl = h->plan;
    // under stream capture: n_steps plain launches (a captured multi-step launch would read the handle's parameter copy
    // as a later call left it, and the upload's host source would not outlive the call)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    // a buffer whose constant observation bytes are not known to be in place gets one plain step first (it writes
    // them); every step of the multi-step kernel then finds them there
    if (cap == hipStreamCaptureStatusNone && (io->obs != h->obs_zero_ptr || pl.kernel != 2 || h->ov.phase_mask)) {
        if ((rc = step_once(h, io, st)) != CH_OK) return rc;
        done = 1;
    }
    const int rest = n_steps - done;
    // the multi-step kernel where the plan has a row for it (and the io asks for no terminal observations); captured,
    // and at other geometries: one launch per step
    if (cap != hipStreamCaptureStatusNone || pl.multi_row == kStepNoRow || io->terminal_obs) {
        for (int k = 0; k < rest; ++k)
            if ((rc = step_once(h, io, st)) != CH_OK) return rc;
        return CH_OK;
    }
    if (rest == 0) return CH_OK;
    // the kernel reads its parameters from a device copy (k_step2_multi), uploaded when they differ from the last
    // upload (stream-ordered; a pageable source is staged by the runtime before the call returns)
    if (!h->d_params) HIP_TRY(h, hipMalloc(&h->d_params, kParamsBytes));
    const hipError_t e = with_params(h, [&](auto p) {
        fill_step(h, io, p);
        using P = decltype(p);
        static_assert(sizeof(P) <= kParamsBytes, "StepParams fits the device copy");
        if (h->params_host.size() != sizeof(P) || std::memcmp(h->params_host.data(), &p, sizeof(P)) != 0) {
            const hipError_t ce = hipMemcpyAsync(h->d_params, &p, sizeof(P), hipMemcpyHostToDevice, st);
            if (ce != hipSuccess) return ce;
            h->params_host.assign(reinterpret_cast<const unsigned char*>(&p),
                                  reinterpret_cast<const unsigned char*>(&p) + sizeof(P));
        }
        return launch_step_v2_multi(p, static_cast<const P*>(h->d_params), pl.multi_row, pl.multi_block, pl.multi_lds, st,
                                    rest);
    });
    if (e != hipSuccess) return fail(h, CH_ERR_DEVICE, std::string("ch_step_n launch: ") + hipGetErrorString(e));
    h->multi_steps += rest;
    h->obs_zero_ptr = io->obs;
    return CH_OK;
}

/* Internal (tests): steps ch_step_n has run inside its multi-step kernel on this handle. */
int64_t ch__multi_steps(const ch_handle* h) { return h ? (int64_t)h->multi_steps : -1; }

int ch_state_size(const ch_handle* h, int64_t* n_doubles, int64_t* n_ints) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_state_size: NULL handle");
    if (n_doubles)
        *n_doubles = (int64_t)kDroneComps * h->E * h->NC + (int64_t)kCattleComps * h->E * h->M + kEnvReal * h->E +
                     (int64_t)kPhysComps * h->E * h->NC;
    if (n_ints) *n_ints = (int64_t)kEnvInt * h->E;
    return CH_OK;
}

int ch_get_state(ch_handle* h, double* hd, int32_t* hi, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_get_state: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h, hipStreamSynchronize(st));
    const size_t nd = (size_t)kDroneComps * h->E * h->NC, nc = (size_t)kCattleComps * h->E * h->M,
                 nr = (size_t)kEnvReal * h->E, np_ = (size_t)kPhysComps * h->E * h->NC;
    if (hd) {
        if (h->rsize == sizeof(double)) {
            HIP_TRY(h, hipMemcpy(hd, h->drone, nd * 8, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(hd + nd, h->cattle, nc * 8, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(hd + nd + nc, h->envr, nr * 8, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(hd + nd + nc + nr, h->phys, np_ * 8, hipMemcpyDeviceToHost));
        } else {
            std::vector<float> f(nd + nc + nr + np_);
            HIP_TRY(h, hipMemcpy(f.data(), h->drone, nd * 4, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(f.data() + nd, h->cattle, nc * 4, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(f.data() + nd + nc, h->envr, nr * 4, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(f.data() + nd + nc + nr, h->phys, np_ * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < f.size(); ++i) hd[i] = f[i];
            // the positions and prev_cent_dists as the step holds them (f64)
            HIP_TRY(h, hipMemcpy(hd, h->pos64, sizeof(double) * 3 * h->E * h->NC, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(hd + nd, h->cpos64, sizeof(double) * 2 * h->E * h->M, hipMemcpyDeviceToHost));
            HIP_TRY(h, hipMemcpy(hd + nd + nc, h->prev64, sizeof(double) * h->E, hipMemcpyDeviceToHost));
        }
    }
    if (hi) HIP_TRY(h, hipMemcpy(hi, h->envi, sizeof(int) * kEnvInt * h->E, hipMemcpyDeviceToHost));
    int word = 0;
    HIP_TRY(h, hipMemcpy(&word, h->errw, sizeof(int), hipMemcpyDeviceToHost));
    return device_status(h, word);
}

int ch_set_state(ch_handle* h, const double* hd, const int32_t* hi, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_set_state: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h, hipStreamSynchronize(st));
    h->obs_zero_ptr = nullptr;   // NUM_DRONES may change: the next step writes every obs block in full
    // the same on the device, for steps replayed from a graph captured earlier
    HIP_TRY(h, hipMemset(h->stale, 1, 2 * (size_t)h->E));
    const size_t nd = (size_t)kDroneComps * h->E * h->NC, nc = (size_t)kCattleComps * h->E * h->M,
                 nr = (size_t)kEnvReal * h->E, np_ = (size_t)kPhysComps * h->E * h->NC;
    if (hd) {
        if (h->rsize == sizeof(double)) {
            HIP_TRY(h, hipMemcpy(h->drone, hd, nd * 8, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->cattle, hd + nd, nc * 8, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->envr, hd + nd + nc, nr * 8, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->phys, hd + nd + nc + nr, np_ * 8, hipMemcpyHostToDevice));
        } else {
            std::vector<float> f(hd, hd + nd + nc + nr + np_);
            HIP_TRY(h, hipMemcpy(h->drone, f.data(), nd * 4, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->cattle, f.data() + nd, nc * 4, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->envr, f.data() + nd + nc, nr * 4, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->phys, f.data() + nd + nc + nr, np_ * 4, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->pos64, hd, sizeof(double) * 3 * h->E * h->NC, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->cpos64, hd + nd, sizeof(double) * 2 * h->E * h->M, hipMemcpyHostToDevice));
            HIP_TRY(h, hipMemcpy(h->prev64, hd + nd + nc, sizeof(double) * h->E, hipMemcpyHostToDevice));
        }
    }
    if (hi) HIP_TRY(h, hipMemcpy(h->envi, hi, sizeof(int) * kEnvInt * h->E, hipMemcpyHostToDevice));
    return CH_OK;
}

/* Internal, not part of the public ABI: device buffer [E][N][16] receiving per-drone PID intermediates. */
int ch__set_debug(ch_handle* h, double* dev) {
    if (!h) return CH_ERR_INVALID;
    h->debug = dev;
    return CH_OK;
}

/* Internal diagnostics: step kernel version (1 = team-per-env ch_kernels.hip, 2 = role-split ch_step.hip). */
int ch__set_kernel(ch_handle* h, int32_t version) {
    if (!h || (version != 1 && version != 2)) return CH_ERR_INVALID;
    StepOverrides ov = h->ov;
    ov.kernel = version;
    return replan(h, ov);
}

/* Internal diagnostics: device buffer [grid][16] of per-workgroup timestamps written by the v2 kernel. */
int ch__set_tstamp(ch_handle* h, long long* dev) {
    if (!h) return CH_ERR_INVALID;
    h->tstamp = dev;
    return CH_OK;
}

/* Internal diagnostics: override the v2 geometry (envs per workgroup, block size) for sweeps. */
int ch__set_geometry(ch_handle* h, int32_t G, int32_t block) {
    if (!h) return CH_ERR_INVALID;
    StepOverrides ov = h->ov;
    ov.geometry = true; ov.G = G; ov.block = block;
    return replan(h, ov);
}

/* Internal diagnostics: v2 geometry (envs per workgroup, block size, dynamic LDS bytes). */
int ch__geometry(const ch_handle* h, int32_t* G, int32_t* block, int64_t* lds, int32_t* kernel) {
    if (!h) return CH_ERR_INVALID;
    if (G) *G = h->plan.G;
    if (block) *block = h->plan.block;
    if (lds) *lds = (int64_t)h->plan.lds;
    if (kernel) *kernel = h->plan.kernel;
    return CH_OK;
}

/* Internal (tests): the plan the handle holds, as ch__step_plan's out (ch_step_plan.cpp). */
int ch__step_plan_of(const ch_handle* h, int64_t out[13]) {
    if (!h || !out) return CH_ERR_INVALID;
    step_plan_out(h->plan, out);
    return CH_OK;
}

/* Internal: forget which obs buffer holds valid constant-zero bytes (the caller wrote into it); the
 * next ch_step writes every obs block in full. */
int ch__obs_invalidate(ch_handle* h, void* stream) {
    if (!h) return CH_ERR_INVALID;
    h->obs_zero_ptr = nullptr;
    // and on the device (stale row 1), for steps replayed from a graph captured before this call
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemsetAsync(h->stale + h->E, 1, (size_t)h->E, (hipStream_t)stream));
    return CH_OK;
}

/* Internal diagnostics: skip kernel phases (1 drones, 2 flock, 4 task, 8 obs) to attribute time; 128 / 256: cow waves
 * on the drone wave's SIMD take no chunks after / before the drone hand-off (v2 scheduling experiments). */
int ch__set_phase_mask(ch_handle* h, int32_t mask) {
    if (!h) return CH_ERR_INVALID;
    StepOverrides ov = h->ov;
    ov.phase_mask = mask;
    return replan(h, ov);
}

int ch_metrics(ch_handle* h, double* out, int32_t reset_after, void* stream) {
    if (!h || !out) return fail(h, CH_ERR_INVALID, "ch_metrics: NULL argument");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    // device reduction on the caller's stream, then one 72-byte copy into pinned memory
    HIP_TRY(h, launch_metrics_reduce(h->metrics, h->E, h->mdev, h->errw, h->mdev + CH_METRIC_COUNT, reset_after, st));
    HIP_TRY(h, hipMemcpyAsync(h->mhost, h->mdev, sizeof(double) * (CH_METRIC_COUNT + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    std::memcpy(out, h->mhost, sizeof(double) * CH_METRIC_COUNT);
    return device_status(h, (int)h->mhost[CH_METRIC_COUNT]);
}

/* Internal (tests): the per-env metric rows [kMetricRows][E] as the step kernels keep them (the public sums' inputs and
 * the two running rows of the open episode), copied to host memory after the stream's work. */
int ch__metric_rows(ch_handle* h, double* host_out, void* stream) {
    if (!h || !host_out) return fail(h, CH_ERR_INVALID, "ch__metric_rows: NULL argument");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h, hipMemcpyAsync(host_out, h->metrics, sizeof(double) * kMetricRows * h->E, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return CH_OK;
}

int ch_metrics_device(ch_handle* h, double* dev_out, int32_t reset_after, void* stream) {
    if (!h || !dev_out) return fail(h, CH_ERR_INVALID, "ch_metrics_device: NULL argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_metrics_reduce(h->metrics, h->E, dev_out, nullptr, nullptr, reset_after, (hipStream_t)stream));
    return CH_OK;
}

int ch_get_eval(ch_handle* h, double* host_out, void* stream) {
    if (!h || !host_out) return fail(h, CH_ERR_INVALID, "ch_get_eval: NULL argument");
    if (!h->evald) return fail(h, CH_ERR_UNSUPPORTED, "ch_get_eval: the handle was created with eval_metrics = 0");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(h, hipMemcpy(host_out, h->evald, sizeof(double) * h->E * h->NC, hipMemcpyDeviceToHost));
    return CH_OK;
}

int ch_outputs_to_host(ch_handle* h, const ch_step_io* io, ch_host_out* out, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_outputs_to_host: NULL handle");
    if (!io || !out || !io->obs || !io->reward || !io->terminated || !io->truncated || !out->obs || !out->reward ||
        !out->terminated || !out->truncated)
        return fail(h, CH_ERR_INVALID, "ch_outputs_to_host: obs, reward, terminated and truncated are required on both sides");
    if ((out->reset_happened || out->ended_env || out->ended_obs || out->ended_stats) && !io->reset_happened)
        return fail(h, CH_ERR_INVALID, "ch_outputs_to_host: the reset list needs io->reset_happened");
    if ((out->ended_obs && !io->terminal_obs) || (out->ended_stats && !io->episode_stats))
        return fail(h, CH_ERR_INVALID, "ch_outputs_to_host: ended_obs needs io->terminal_obs, ended_stats io->episode_stats");
    if (out->agent_active && !io->agent_active)
        return fail(h, CH_ERR_INVALID, "ch_outputs_to_host: agent_active needs io->agent_active");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t E = h->E;
    const size_t blk = (size_t)h->rows * 86, live = (size_t)h->NC * 86;   // floats per block / in its first NC rows
    if (io->reset_happened) {
        if (!h->st.count) {
            HIP_TRY(h, hipMalloc(&h->st.count, sizeof(long long)));
            HIP_TRY(h, hipMalloc(&h->st.env, sizeof(long long) * E));
            HIP_TRY(h, hipMalloc(&h->st.stats, sizeof(double) * 2 * E));
            HIP_TRY(h, hipMalloc(&h->st.obs, sizeof(float) * blk * E));
            HIP_TRY(h, hipHostMalloc(&h->st.count_host, sizeof(long long), hipHostMallocDefault));
        }
        HIP_TRY(h, launch_stage_ended(E, io->reset_happened, out->ended_obs ? io->terminal_obs : nullptr,
                                      out->ended_stats ? io->episode_stats : nullptr, (int)blk, h->st.count, h->st.env,
                                      h->st.stats, h->st.obs, st));
        HIP_TRY(h, hipMemcpyAsync(h->st.count_host, h->st.count, sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    // the first NC rows of every block (CTDE: rows >= NC are always zero; MARL: R = NC, one contiguous copy)
    if (live == blk)
        HIP_TRY(h, hipMemcpyAsync(out->obs, io->obs, sizeof(float) * blk * E, hipMemcpyDeviceToHost, st));
    else
        HIP_TRY(h, hipMemcpy2DAsync(out->obs, sizeof(float) * blk, io->obs, sizeof(float) * blk, sizeof(float) * live, E,
                                    hipMemcpyDeviceToHost, st));
    const size_t K = (size_t)h->K;
    HIP_TRY(h, hipMemcpyAsync(out->reward, io->reward, sizeof(float) * K * E, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(out->terminated, io->terminated, K * E, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(out->truncated, io->truncated, K * E, hipMemcpyDeviceToHost, st));
    if (out->reset_happened) HIP_TRY(h, hipMemcpyAsync(out->reset_happened, io->reset_happened, E, hipMemcpyDeviceToHost, st));
    if (out->agent_active)
        HIP_TRY(h, hipMemcpyAsync(out->agent_active, io->agent_active, (size_t)h->NC * E, hipMemcpyDeviceToHost, st));
    // the ended envs' lists: a speculative first part sized from the recent counts (the usual case: a few envs end per
    // step -- at C4 under random actions ~20, in a training rollout ~3), the rest after the count
    const int64_t cap = std::min<int64_t>(E, 2 * std::max<int64_t>(h->st.ended_last, (int64_t)h->st.ended_mean) + 8);
    auto copy_ended = [&](int64_t lo, int64_t hi) -> int {
        if (hi <= lo) return CH_OK;
        if (out->ended_env)
            HIP_TRY(h, hipMemcpyAsync(out->ended_env + lo, h->st.env + lo, sizeof(long long) * (hi - lo), hipMemcpyDeviceToHost, st));
        if (out->ended_stats)
            HIP_TRY(h, hipMemcpyAsync(out->ended_stats + 2 * lo, h->st.stats + 2 * lo, sizeof(double) * 2 * (hi - lo),
                                      hipMemcpyDeviceToHost, st));
        if (out->ended_obs)
            HIP_TRY(h, hipMemcpyAsync(out->ended_obs + blk * lo, h->st.obs + blk * lo, sizeof(float) * blk * (hi - lo),
                                      hipMemcpyDeviceToHost, st));
        return CH_OK;
    };
    int rc = CH_OK;
    if (io->reset_happened && (rc = copy_ended(0, cap))) return rc;
    HIP_TRY(h, hipStreamSynchronize(st));
    out->ended_count = io->reset_happened ? *h->st.count_host : 0;
    if (io->reset_happened) {
        h->st.ended_last = out->ended_count;
        h->st.ended_mean = 0.9 * h->st.ended_mean + 0.1 * (double)out->ended_count;
    }
    if (out->ended_count > cap) {
        if ((rc = copy_ended(cap, out->ended_count))) return rc;
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    return CH_OK;
}

int ch_sync(ch_handle* h, void* stream) {
    if (!h) return fail(nullptr, CH_ERR_INVALID, "ch_sync: NULL handle");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    int word = 0;
    HIP_TRY(h, hipMemcpy(&word, h->errw, sizeof(int), hipMemcpyDeviceToHost));
    return device_status(h, word);
}

}  // extern "C"
