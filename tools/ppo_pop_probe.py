"""Diagnostics: the population update against solo calls.  The update alone -- no collection -- at
the driver's shape, net 1032-128-128-48 and minibatches of 64, --rows rows of synthetic data per member (each member
its own model, data, permutation, Adam state, statistics and scratch).  One process runs one leg for one P:

  --leg solo   P ch_ppo_train_opt epochs, one member after another; the calls an older library has too, so the same
               leg runs on a parent library through CH_LIB_PATH -- leg (a), on both libraries
  --leg pop    one ch_ppo_train_pop epoch for the P members                                       -- leg (b)

A window is one epoch for all P members (rows / 64 population steps) between two device synchronisations; two
untimed windows, then --reps timed ones.  Prints one JSON line: every window's microseconds per population step,
their median, and member-steps per second at the median.  Launch each process under its own `timeout`, once, the legs
alternating."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-cattle-herding_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("solo", "pop"), required=True)
    ap.add_argument("--members", type=int, required=True)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from cattleherd import _lib, ppo
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n, P, B = a.rows, a.members, 64
    nb = (n + B - 1) // B
    members, keep = (_lib.ChPpoMember * P)(), []
    for i in range(P):
        model = ppo.SB3ActorCritic(obs_dim=1032, act_dim=48, device=dev, seed=i)
        g = torch.Generator(device=dev).manual_seed(100 + i)
        obs = torch.zeros(n, 1032, device=dev)
        obs[:, :344] = 0.5 * torch.randn(n, 344, device=dev, generator=g)
        with torch.no_grad():
            act = model.action_net(model.policy_net(obs)) + torch.exp(model.log_std) * torch.randn(n, 48, device=dev, generator=g)
            _, lp, _ = model.evaluate_actions(obs, act)
        data = (obs, act.contiguous(), (lp + 0.05 * torch.randn(n, device=dev, generator=g)).contiguous(),
                torch.randn(n, device=dev, generator=g), torch.randn(n, device=dev, generator=g))
        net = ppo.ppo_net(model)
        k = L.ch_ppo_param_count(ctypes.byref(net))
        state = [torch.zeros(k, device=dev), torch.zeros(k, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                 torch.zeros(nb, _lib.CH_PPO_OPT_STATS, device=dev),
                 torch.empty(L.ch_ppo_scratch_size(ctypes.byref(net), B), device=dev), torch.randperm(n, device=dev, generator=g)]
        mb = members[i]
        mb.net, mb.hp = net, _lib.ChPpoHparams(3e-4, 0.9, 0.999, 1e-5, 0.1, 0.1, 0.7, 0.5, 1, 0)
        mb.data, mb.opts = _lib.ChPpoData(*(t.data_ptr() for t in data), n), _lib.ChPpoOpts(0.0, 0.0, None, None)
        mb.m, mb.v, mb.step_dev, mb.stats, mb.scratch, mb.idx = (t.data_ptr() for t in state)
        keep.append((model, data, state))
    pop = ctypes.c_void_p()
    if a.leg == "pop":
        _lib.check(L.ch_ppo_pop_create(P, 0, ctypes.byref(pop)))

    def window():
        if a.leg == "pop":
            _lib.check(L.ch_ppo_train_pop(pop, members, P, n, B, None))
            return
        for mb in members:
            _lib.check(L.ch_ppo_train_opt(ctypes.byref(mb.net), ctypes.byref(mb.hp), ctypes.byref(mb.data), ctypes.byref(mb.opts),
                                          mb.idx, n, B, mb.m, mb.v, mb.step_dev, mb.stats, mb.scratch, None))

    us = []
    for r in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        window()
        torch.cuda.synchronize()
        if r >= 2:
            us.append((time.perf_counter() - t0) / nb * 1e6)
    med = float(np.median(us))
    steps = [int(s[2][2]) for s in keep]
    print(json.dumps({"leg": a.leg, "members": P, "library": os.path.relpath(_lib.LIB_PATH, ROOT),
                      "code_object": _lib.code_object_hash(), "rows": n, "steps_per_window": nb,
                      "us_per_population_step": [round(x, 3) for x in us], "median_us_per_population_step": round(med, 3),
                      "min": round(min(us), 3), "max": round(max(us), 3),
                      "member_steps_per_s": round(P * 1e6 / med, 1), "adam_steps_applied": [min(steps), max(steps)]}), flush=True)
    if a.leg == "pop":
        _lib.check(L.ch_ppo_pop_destroy(pop))


if __name__ == "__main__":
    main()
