"""Diagnostics: what the native PPO update's options cost per SGD step.  The update alone -- no
collection -- at the driver's shape, net 1032-128-128-48 and minibatches of 64, over a synthetic buffer of --rows rows
(old_log_prob = the model's own + N(0, 0.05^2), old values = the model's own + N(0, 0.25^2)).  One process runs one leg:

  --leg plain    PPOUpdate(backend="native"), no option: ch_ppo_train, the calls an older library has too, so the
                 same leg runs on a parent library through CH_LIB_PATH -- leg (a), the two alternating on one box
  --leg armed    target_kl = 1e6: ch_ppo_train_opt, the gate armed and never tripping           (b)
  --leg vfclip   clip_range_vf = 0.25                                                           (c)
  --leg stopped  target_kl = 1e-12: the first minibatch trips, every later step of the call returns at entry; the
                 figure is the call's time over the steps behind the trip                       (d)

--reps timed train() calls after one untimed, each ended by a device synchronise (a window).  Prints one JSON line
with every window's microseconds per step and their median.  Launch each process under its own `timeout`, once."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-cattle-herding_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("plain", "armed", "vfclip", "stopped"), required=True)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from cattleherd import _lib
    from cattleherd.ppo import PPOUpdate, SB3ActorCritic
    dev = torch.device("cuda", 0)
    model = SB3ActorCritic(obs_dim=1032, act_dim=48, device=dev, seed=0)
    g = torch.Generator(device=dev).manual_seed(1)
    n = a.rows
    obs = torch.zeros(n, 1032, device=dev)
    obs[:, :344] = 0.5 * torch.randn(n, 344, device=dev, generator=g)
    with torch.no_grad():
        mean = model.action_net(model.policy_net(obs))
        act = mean + torch.exp(model.log_std) * torch.randn(n, 48, device=dev, generator=g)
        values, lp, _ = model.evaluate_actions(obs, act)
    rb = types.SimpleNamespace(
        T=n // 64, batch=types.SimpleNamespace(n_envs=64), obs=obs.view(n // 64, 64, 1032), actions=act.view(n // 64, 64, 48),
        log_probs=(lp + 0.05 * torch.randn(n, device=dev, generator=g)).view(n // 64, 64),
        advantages=torch.randn(n, device=dev, generator=g).view(n // 64, 64),
        returns=torch.randn(n, device=dev, generator=g).view(n // 64, 64),
        values=(values + 0.25 * torch.randn(n, device=dev, generator=g)).view(n // 64, 64).contiguous())
    kw = {"plain": {}, "armed": {"target_kl": 1e6}, "vfclip": {"clip_range_vf": 0.25}, "stopped": {"target_kl": 1e-12}}[a.leg]
    upd = PPOUpdate(model, batch_size=64, n_epochs=a.epochs, backend="native", **kw)
    us = []
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = upd.train(rb)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if r:
            us.append((t1 - t0) / (steps - 1 if a.leg == "stopped" else steps) * 1e6)
    out = {"leg": a.leg, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "code_object": _lib.code_object_hash(),
           "rows": n, "n_epochs": a.epochs, "sgd_steps_launched": steps, "us_per_sgd_step": [round(x, 3) for x in us],
           "median_us_per_sgd_step": round(float(np.median(us)), 3), "min": round(min(us), 3), "max": round(max(us), 3)}
    if a.leg != "plain":
        out.update(stopped_early=upd.stopped_early, steps_applied=upd.steps_applied)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
