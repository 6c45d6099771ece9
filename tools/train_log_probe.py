"""Diagnostics: what the device-side SB3 training log costs.  One PPO training iteration of the CTDE
driver on the device -- the native collection (cattleherd.rollout) then the native update (PPOUpdate(backend="native"),
the driver's hyper-parameters, minibatches of 64) -- at 4096 envs, with and without the log:

  --log 0   collect() and PPOUpdate(log_stats=False): the calls an older library has too, so the same leg runs on a
            baseline library through CH_LIB_PATH (the update then shows what the two extra partials of k_ppo_fb cost).
  --log 1   collect(ring=EpisodeRing(batch)) and PPOUpdate(log_stats=True): ch_rollout_collect_log, ch_ppo_train_log,
            ch_explained_variance and the one read of the record.

  --config c2   configs[2]: (2 drones, 8 cattle), NaN-safe rewards, level 7 (the training leg of bench.py)
  --config c3   configs[3]: (4 drones, 16 cattle)

One process runs one leg: --reps timed iterations after one untimed, each half ended by a device synchronise.  Prints
one JSON line; run the legs alternating (profiles/train_log/).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-cattle-herding_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, choices=(0, 1), required=True)
    ap.add_argument("--config", choices=("c2", "c3"), default="c2")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.ppo import PPOUpdate, SB3ActorCritic
    from cattleherd.rollout import DeviceRolloutBuffer
    if a.config == "c2":
        b = HerdBatch(a.envs, 2, 8, mode="ctde", compat=False, curriculum_level=7)
    else:
        b = HerdBatch(a.envs, 4, 16, mode="ctde")
    b.reset()
    model = SB3ActorCritic(obs_dim=b.obs_rows * 86, act_dim=48, device=b.device, seed=0)
    actor, critic, log_std = model.device_nets()
    rb = DeviceRolloutBuffer(b, a.steps, act_dim=48)
    kw, upd_kw = {}, {}
    ring = None
    if a.log:
        from cattleherd.train_log import EpisodeRing
        ring = EpisodeRing(b).begin()
        kw, upd_kw = {"ring": ring}, {"log_stats": True}
    upd = PPOUpdate(model, batch_size=64, n_epochs=a.epochs, backend="native", **upd_kw)
    # time limits inside every collection: the ring has episodes to append
    b.set_state({"step_counter": 4800 - 4 * (np.arange(a.envs) % (8 * a.steps))})
    collect_us, sgd_us, record = [], [], {}
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        rb.collect(actor, critic, log_std, seed=1 + r, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        steps = upd.train(rb)
        if ring is not None:
            record = dict(ring.summary(), **upd.last_log)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r:
            collect_us.append((t1 - t0) / a.steps * 1e6)
            sgd_us.append((t2 - t1) / steps * 1e6)
    b.sync()
    out = {"log": a.log, "config": a.config, "library": os.path.relpath(_lib.LIB_PATH, ROOT),
           "code_object": _lib.code_object_hash(), "envs": a.envs, "n_steps": a.steps, "n_epochs": a.epochs,
           "sgd_steps": steps, "collect_us_per_step": [round(x, 2) for x in collect_us],
           "us_per_sgd_step": [round(x, 3) for x in sgd_us],
           "median_collect_us_per_step": round(float(np.median(collect_us)), 2),
           "median_collect_env_steps_per_s": round(a.envs / float(np.median(collect_us)) * 1e6, 1),
           "median_us_per_sgd_step": round(float(np.median(sgd_us)), 3)}
    if ring is not None:
        out.update(episodes=ring.count(), record={k: (round(v, 6) if isinstance(v, float) else v) for k, v in record.items()})
    print(json.dumps(out), flush=True)
    b.close()


if __name__ == "__main__":
    main()
