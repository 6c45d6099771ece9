"""Diagnostics: env-steps/s of the on-device evaluation loop at 4096 envs x (4 drones, 16 cattle), f64, with the
v16-6 actor (tests/golden/policy_ctde_v16_6.npz), against the loop a user writes without it.

  --leg native   cattleherd.eval_policy's native loop (ch_evaluate_policy): forward, action kernel, step, recorder,
                 ``remaining`` read every --check-every steps.  The table is sized so that no quota fills inside a
                 window (4 slots per env; if it does, the rate is over the steps that ran).
  --leg loop     ``batch.step_policy(policy)`` each step and ``reset_happened.any()`` pulled to the host every
                 --check-every steps.  Needs nothing of the evaluation, so it also runs on an older library
                 (CH_LIB_PATH=<the parent commit's libcattleherd.so>).

One process runs one leg: --windows timed windows of --steps steps after a warm-up, each ended by a device
synchronise.  Prints one JSON line.  Run the legs alternating, several times each (profiles/eval/).
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
    ap.add_argument("--leg", choices=("native", "loop"), required=True)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--check-every", type=int, default=16)
    a = ap.parse_args()
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.policy import DevicePolicy
    d = np.load(os.path.join(ROOT, "tests", "golden", "policy_ctde_v16_6.npz"))
    sd = {k.replace("__", "."): torch.tensor(d[k]) for k in d.files if "__" in k}
    b = HerdBatch(a.envs, 4, 16, mode="ctde", precision="f64")
    b.reset()
    rates, ran = [], []
    if a.leg == "native":
        from cattleherd.eval_policy import DeviceEvalTable
        actor = DevicePolicy.sb3_actor(sd, clip=False, cache_packed=True)
        table = DeviceEvalTable(b, 4)

        def window(steps):
            table.begin(4 * a.envs)
            return table.run(actor, steps, a.check_every)[0]
    else:
        actor = DevicePolicy.sb3_actor(sd, cache_packed=True)

        def window(steps):
            for t in range(1, steps + 1):
                b.step_policy(actor)
                if t % a.check_every == 0 or t == steps:
                    bool(b.reset_happened.any().item())
            return steps
    window(a.warmup)
    torch.cuda.synchronize()
    for _ in range(a.windows):
        t0 = time.perf_counter()
        n = window(a.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ran.append(n)
        rates.append(a.envs * n / dt)
    b.sync()
    print(json.dumps({"leg": a.leg, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "code_object": _lib.code_object_hash(),
                      "envs": a.envs, "steps": ran, "check_every": a.check_every,
                      "env_steps_per_s": [round(r, 1) for r in rates],
                      "us_per_step": [round(a.envs / r * 1e6, 2) for r in rates]}), flush=True)
    b.close()


if __name__ == "__main__":
    main()
