"""Diagnostics: what the device-side RLlib training log costs.  One DTDE training iteration on the
device at configs[4]'s size -- 4096 envs x (4 drones, 32 cattle), MARL, the RLlib default module: the native
collection (DeviceMarlRolloutBuffer.collect) then the native update (MarlPPOUpdate(backend="native"), minibatches of
128) -- with and without the log:

  --log 0   collect() and MarlPPOUpdate(log_stats=False): the calls an older library has too, so the same leg runs on a
            baseline library through CH_LIB_PATH.
  --log 1   collect(ring=MarlEpisodeRing(batch)) and MarlPPOUpdate(log_stats=True): ch_marl_rollout_collect_log,
            ch_marl_ppo_train_log and the one read of each record.

One process runs one leg: --reps timed iterations after one untimed, each half ended by a device synchronise.  Prints
one JSON line; run the legs alternating (profiles/marl_train_log/).
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
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--minibatch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.marl_ppo import MarlPPOUpdate, RLlibActorCritic
    from cattleherd.rollout import DeviceMarlRolloutBuffer
    b = HerdBatch(a.envs, 4, 32, mode="marl", compat=False)
    b.reset()
    model = RLlibActorCritic(device=b.device, seed=0)
    policy, value = model.device_nets()
    rb = DeviceMarlRolloutBuffer(b, a.steps)
    kw, upd_kw, ring = {}, {}, None
    if a.log:
        from cattleherd.train_log import MarlEpisodeRing, rllib_result
        ring = MarlEpisodeRing(b).begin()
        kw, upd_kw = {"ring": ring}, {"log_stats": True}
    upd = MarlPPOUpdate(model, num_epochs=a.epochs, minibatch_size=a.minibatch, backend="native", **upd_kw)
    collect_us, sgd_us, record = [], [], {}
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        rb.collect(policy, value, seed=1 + r, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        steps = upd.train(rb)
        if ring is not None:
            record = rllib_result(ring, upd)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r:
            collect_us.append((t1 - t0) / a.steps * 1e6)
            sgd_us.append((t2 - t1) / steps * 1e6)
    b.sync()
    out = {"log": a.log, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "code_object": _lib.code_object_hash(),
           "envs": a.envs, "n_steps": a.steps, "n_epochs": a.epochs, "minibatch": a.minibatch, "sgd_steps": steps,
           "collect_us_per_step": [round(x, 2) for x in collect_us], "us_per_sgd_step": [round(x, 3) for x in sgd_us],
           "median_collect_us_per_step": round(float(np.median(collect_us)), 2),
           "median_us_per_sgd_step": round(float(np.median(sgd_us)), 3)}
    if ring is not None:
        out.update(episodes=ring.count(), record=record)
    print(json.dumps(out), flush=True)
    b.close()


if __name__ == "__main__":
    main()
