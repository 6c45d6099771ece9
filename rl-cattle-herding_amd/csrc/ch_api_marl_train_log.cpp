// ch_api_marl_train_log.cpp — the RLlib training log's part of the C ABI (see include/cattleherd.h): the MARL episode
// ring (ch_marl_ep_ring_begin, ch_marl_ep_ring_record; its wiring into the collection is ch_marl_rollout_collect_log in
// ch_api_policy.cpp).  Kernels in ch_marl_ep_ring.hip; ch_marl_ppo_train_log lives with ch_marl_ppo_train in
// ch_api_ppo.cpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ch_handle.h"

using namespace ch;

// the ring first (it can be judged without a handle), then the handle, then the step io
int marl_ring_args(ch_handle* h, const ch_marl_ep_ring* ring, const ch_step_io* io, MarlRingArgs& a, const char* who) {
    if (!ring) return fail(h, CH_ERR_INVALID, std::string(who) + ": NULL ring");
    if (ring->window < 1) return fail(h, CH_ERR_INVALID, std::string(who) + ": the ring's window must be >= 1");
    if (!ring->ep_return || !ring->agent_return || !ring->ep_length || !ring->agent_length || !ring->ep_env ||
        !ring->total || !ring->acc_return || !ring->acc_length || !ring->acc_steps || !ring->env_steps || !ring->agent_steps)
        return fail(h, CH_ERR_INVALID, std::string(who) + ": every ring array is required");
    if (!h) return fail(nullptr, CH_ERR_INVALID, std::string(who) + ": NULL handle");
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

}  // extern "C"
