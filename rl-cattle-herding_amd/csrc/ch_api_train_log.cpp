// ch_api_train_log.cpp — the training logs' part of the C ABI (see include/cattleherd.h).  SB3 (CTDE): the episode ring
// (ch_ep_ring_begin, ch_ep_ring_record; its wiring into the collection is ch_rollout_collect_log in ch_api_policy.cpp)
// and the handle-free ch_explained_variance; a population's rings, their fitness table and explained variances
// (ch_ep_ring_pop_*, ch_explained_variance_pop; the rings' wiring into the population collection is
// ch_rollout_collect_pop_log in ch_api_policy.cpp); kernels in ch_ep_ring.hip.  RLlib (MARL): the per-agent episode ring
// (ch_marl_ep_ring_begin, ch_marl_ep_ring_record; wired in by ch_marl_rollout_collect_log in ch_api_policy.cpp); kernels
// in ch_marl_ep_ring.hip.  ch_ppo_train_log and ch_marl_ppo_train_log live with the updates in ch_api_ppo.cpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ch_handle.h"

using namespace ch;

// what both rings check first: the ring (it can be judged without a handle: its window, and `whole`: every array is
// there), then the handle
static int ring_and_handle(ch_handle* h, int64_t window, bool whole, const char* who) {
    if (window < 1) return fail(h, CH_ERR_INVALID, std::string(who) + ": the ring's window must be >= 1");
    if (!whole) return fail(h, CH_ERR_INVALID, std::string(who) + ": every ring array is required");
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
    return CH_OK;
}

// the ring and the handle, then the handle's mode, then the step io
int ep_ring_args(ch_handle* h, const ch_ep_ring* ring, const ch_step_io* io, EpRingArgs& a, const char* who) {
    if (!ring) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL ring");
    if (int rc = ring_and_handle(h, ring->window, ring->ep_return && ring->ep_length && ring->ep_env && ring->total, who))
        return rc;
    if (h->cfg.mode != CH_MODE_CTDE)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the episode ring is for CTDE handles");
    std::memset(&a, 0, sizeof(a));
    a.E = h->E; a.W = ring->window;
    a.ep_return = ring->ep_return; a.ep_length = ring->ep_length; a.ep_env = ring->ep_env;
    a.total = reinterpret_cast<long long*>(ring->total);
    if (io) {
        if (!io->reset_happened || !io->episode_stats)
            return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry reset_happened and episode_stats");
        a.reset = io->reset_happened; a.stats = io->episode_stats;
    }
    return CH_OK;
}

// The population's rings.  What can be judged without a handle (ch_ep_ring_pop_summary stops there: `h_needed` false):
// the ring, its window, its member count, every array; then the handle, its mode, the envs' division among the
// members; then the step io.  `a` describes all the rings at once (ch_internal.h launch_ep_ring_record_pop).
int ep_ring_pop_args(ch_handle* h, const ch_ep_ring_pop* ring, const ch_step_io* io, EpRingArgs& a, const char* who,
                     bool h_needed) {
    if (!ring) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL ring");
    if (ring->window < 1) return fail(h, CH_ERR_INVALID, std::string(who) + ": the ring's window must be >= 1");
    if (ring->n_members < 1) return fail(h, CH_ERR_INVALID, std::string(who) + ": the ring's n_members must be >= 1");
    if (!ring->ep_return || !ring->ep_length || !ring->ep_env || !ring->total)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": every ring array is required");
    std::memset(&a, 0, sizeof(a));
    a.W = ring->window;
    a.ep_return = ring->ep_return; a.ep_length = ring->ep_length; a.ep_env = ring->ep_env;
    a.total = reinterpret_cast<long long*>(ring->total);
    if (!h_needed) return CH_OK;
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
    if (h->cfg.mode != CH_MODE_CTDE)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the episode ring is for CTDE handles");
    if (h->E % ring->n_members)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": the handle's envs must divide evenly among the ring's n_members");
    a.E = h->E / ring->n_members;
    if (io) {
        if (!io->reset_happened || !io->episode_stats)
            return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry reset_happened and episode_stats");
        a.reset = io->reset_happened; a.stats = io->episode_stats;
    }
    return CH_OK;
}

int marl_ring_args(ch_handle* h, const ch_marl_ep_ring* ring, const ch_step_io* io, MarlRingArgs& a, const char* who) {
    if (!ring) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL ring");
    if (int rc = ring_and_handle(h, ring->window,
                                 ring->ep_return && ring->agent_return && ring->ep_length && ring->agent_length &&
                                     ring->ep_env && ring->total && ring->acc_return && ring->acc_length &&
                                     ring->acc_steps && ring->env_steps && ring->agent_steps, who))
        return rc;
    if (h->cfg.mode != CH_MODE_MARL)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the per-agent episode ring is for MARL handles");
    if (!h->cfg.marl_wrapper)
        return fail(h, CH_ERR_UNSUPPORTED, std::string(who) + ": the per-agent episode ring needs marl_wrapper = 1 "
                                                              "(agents drop out, the env ends when all have terminated)");
    std::memset(&a, 0, sizeof(a));
    a.E = h->E; a.N = h->NC; a.W = ring->window;   // (NC <= kNMax: ch_create)
    a.ep_return = ring->ep_return; a.agent_return = ring->agent_return;
    a.ep_length = ring->ep_length; a.agent_length = ring->agent_length; a.ep_env = ring->ep_env;
    a.total = reinterpret_cast<long long*>(ring->total);
    a.acc_return = ring->acc_return; a.acc_length = ring->acc_length; a.acc_steps = ring->acc_steps;
    a.env_steps = reinterpret_cast<long long*>(ring->env_steps);
    a.agent_steps = reinterpret_cast<long long*>(ring->agent_steps);
    if (io) {
        if (!io->reward || !io->reset_happened)
            return fail(h, CH_ERR_INVALID, std::string(who) + ": the step io must carry reward and reset_happened");
        a.reward = io->reward; a.reset = io->reset_happened;
    }
    return CH_OK;
}

extern "C" {

int ch_ep_ring_begin(ch_handle* h, const ch_ep_ring* ring, void* stream) {
    EpRingArgs a;
    if (int rc = ep_ring_args(h, ring, nullptr, a, "ch_ep_ring_begin")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemsetAsync(a.total, 0, sizeof(long long), (hipStream_t)stream));
    return CH_OK;
}

int ch_ep_ring_record(ch_handle* h, const ch_ep_ring* ring, const ch_step_io* io, void* stream) {
    EpRingArgs a;
    if (!io) return fail(h, CH_ERR_INVALID, "ch_ep_ring_record: NULL step io");
    if (int rc = ep_ring_args(h, ring, io, a, "ch_ep_ring_record")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_ep_ring_record(a, (hipStream_t)stream));
    return CH_OK;
}

int ch_ep_ring_pop_begin(ch_handle* h, const ch_ep_ring_pop* ring, void* stream) {
    EpRingArgs a;
    if (int rc = ep_ring_pop_args(h, ring, nullptr, a, "ch_ep_ring_pop_begin", true)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemsetAsync(a.total, 0, sizeof(long long) * (size_t)ring->n_members, (hipStream_t)stream));
    return CH_OK;
}

int ch_ep_ring_pop_record(ch_handle* h, const ch_ep_ring_pop* ring, const ch_step_io* io, void* stream) {
    EpRingArgs a;
    if (!io) return fail(h, CH_ERR_INVALID, "ch_ep_ring_pop_record: NULL step io");
    if (int rc = ep_ring_pop_args(h, ring, io, a, "ch_ep_ring_pop_record", true)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_ep_ring_record_pop(a, ring->n_members, (hipStream_t)stream));
    return CH_OK;
}

int ch_ep_ring_pop_summary(const ch_ep_ring_pop* ring, double* out_dev, void* stream) {
    EpRingArgs a;
    if (int rc = ep_ring_pop_args(nullptr, ring, nullptr, a, "ch_ep_ring_pop_summary", false)) return rc;
    if (!out_dev) return fail(nullptr, CH_ERR_INVALID, "ch_ep_ring_pop_summary: NULL out_dev");
    const hipError_t e = launch_ep_ring_pop_summary(a, ring->n_members, out_dev, (hipStream_t)stream);
    return e == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, std::string("ch_ep_ring_pop_summary launch: ") + hipGetErrorString(e));
}

int ch_marl_ep_ring_begin(ch_handle* h, const ch_marl_ep_ring* ring, void* stream) {
    MarlRingArgs a;
    if (int rc = marl_ring_args(h, ring, nullptr, a, "ch_marl_ep_ring_begin")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_marl_ep_ring_begin(a, (hipStream_t)stream));
    return CH_OK;
}

int ch_marl_ep_ring_record(ch_handle* h, const ch_marl_ep_ring* ring, const uint8_t* live, const ch_step_io* io,
                           void* stream) {
    MarlRingArgs a;
    if (!io) return fail(h, CH_ERR_INVALID, "ch_marl_ep_ring_record: NULL step io");
    if (int rc = marl_ring_args(h, ring, io, a, "ch_marl_ep_ring_record")) return rc;
    if (!live) return fail(h, CH_ERR_INVALID, "ch_marl_ep_ring_record: NULL live");
    a.live = live;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_marl_ep_ring_record(a, (hipStream_t)stream));
    return CH_OK;
}

int64_t ch_explained_variance_scratch(int64_t n) {
    if (n < 1) { fail(nullptr, CH_ERR_INVALID, "ch_explained_variance_scratch: n < 1"); return -1; }
    return ev_scratch_doubles(n);
}

int ch_explained_variance(const float* values, const float* returns, int64_t n, double* out_dev, double* scratch,
                          void* stream) {
    if (!values || !returns || !out_dev || !scratch) return fail(nullptr, CH_ERR_INVALID, "ch_explained_variance: NULL argument");
    if (n < 1) return fail(nullptr, CH_ERR_INVALID, "ch_explained_variance: n < 1");
    const hipError_t e = launch_explained_variance(values, returns, n, out_dev, scratch, (hipStream_t)stream);
    return e == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, std::string("ch_explained_variance launch: ") + hipGetErrorString(e));
}

int64_t ch_explained_variance_pop_scratch(int64_t n, int32_t n_members) {
    if (n < 1 || n_members < 1) { fail(nullptr, CH_ERR_INVALID, "ch_explained_variance_pop_scratch: n < 1 or n_members < 1"); return -1; }
    return ev_scratch_doubles(n) * n_members;
}

int ch_explained_variance_pop(const float* const* values_dev, const float* const* returns_dev, int32_t n_members, int64_t n,
                              double* out_dev, double* scratch, void* stream) {
    const std::string w = "ch_explained_variance_pop: ";
    if (!values_dev || !returns_dev || !out_dev || !scratch) return fail(nullptr, CH_ERR_INVALID, w + "NULL argument");
    if (n_members < 1 || n_members > 65535) return fail(nullptr, CH_ERR_INVALID, w + "n_members must be 1..65535");   // (a grid dimension)
    if (n < 1) return fail(nullptr, CH_ERR_INVALID, w + "n < 1");
    const hipError_t e = launch_explained_variance_pop(values_dev, returns_dev, n_members, n, out_dev, scratch, (hipStream_t)stream);
    return e == hipSuccess ? CH_OK : fail(nullptr, CH_ERR_DEVICE, w + "launch: " + hipGetErrorString(e));
}

}  // extern "C"
