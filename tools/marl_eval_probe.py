"""Diagnostics: env-steps/s of the DTDE driver's on-device evaluation loop at configs[4]'s size, 4096 envs x (4 drones,
32 cattle), f64, with the reference's trained RLlib weights (tests/golden/policy_marl_rllib.npz) from near-herd start
states, against the best loop a user writes without it.

  --leg native   cattleherd.marl_eval's native loop (ch_marl_evaluate_policy): forward, action kernel (recorder, mark,
                 clamp), step, ``remaining`` read every --check-every steps.  The table is sized so that no quota fills
                 inside a window (4 slots per env; if it does, the rate is over the steps that ran).
  --leg loop     ``policy.forward_batch`` into a fixed buffer, torch's slice and clamp into the action tensor,
                 ``batch.step(autoreset=True)``; no bookkeeping and no host read.  Needs nothing of the evaluation, so
                 it also runs on an older library (CH_LIB_PATH=<the parent commit's libcattleherd.so>).

One process runs one leg.  Before each of --windows timed windows of --steps steps, every env's drones are put
0.6-1.4 m from a random cow of their herd (bench.py near_herd_leg's placement, untimed, seeded: both legs start every
window from the same states) and --burn untimed steps of the leg run; each window ends with a device synchronise.
Prints one JSON line.  Run the legs alternating, several times each (profiles/marl_eval/).
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
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--burn", type=int, default=32)
    ap.add_argument("--check-every", type=int, default=16)
    a = ap.parse_args()
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.policy import DevicePolicy
    n, m = 4, 32
    d = np.load(os.path.join(ROOT, "tests", "golden", "policy_marl_rllib.npz"))
    policy = DevicePolicy.rllib_policy({k.replace("__", "."): d[k] for k in d.files if "__" in k}, cache_packed=True)
    b = HerdBatch(a.envs, n, m, mode="marl", precision="f64")
    b.reset()
    rng = np.random.default_rng(11)

    def place():
        s = b.get_state()
        pick = rng.integers(0, m, (a.envs, n))
        ang = rng.uniform(-np.pi, np.pi, (a.envs, n))
        rad = rng.uniform(0.6, 1.4, (a.envs, n))
        c = np.take_along_axis(s["cow_pos"][:, :m], pick[..., None].repeat(2, -1), 1)
        dp = s["drone_pos"].copy()
        dp[:, :, 0] = c[..., 0] + rad * np.cos(ang)
        dp[:, :, 1] = c[..., 1] + rad * np.sin(ang)
        b.set_state({"drone_pos": dp})

    if a.leg == "native":
        from cattleherd.marl_eval import DeviceMarlEvalTable
        table = DeviceMarlEvalTable(b, 4)

        def window(steps):
            table.begin(4 * a.envs)
            return table.run(policy, steps, a.check_every)[0]
    else:
        out = torch.zeros((a.envs * n, policy.dims[-1]), dtype=torch.float32, device=b.device)
        act = torch.zeros((a.envs, n, 4), dtype=torch.float32, device=b.device)

        def window(steps):
            for _ in range(steps):
                policy.forward_batch(b, out)
                torch.clamp(out.view(a.envs, n, -1)[:, :, :4], -1.0, 1.0, out=act)
                b.step(act, autoreset=True, terminal_obs=False)
            return steps
    rates, ran = [], []
    for _ in range(a.windows):
        place()
        window(a.burn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = window(a.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ran.append(k)
        rates.append(a.envs * k / dt)
    b.sync()
    print(json.dumps({"leg": a.leg, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "code_object": _lib.code_object_hash(),
                      "envs": a.envs, "drones": n, "cattle": m, "steps": ran, "check_every": a.check_every,
                      "env_steps_per_s": [round(r, 1) for r in rates],
                      "us_per_step": [round(a.envs / r * 1e6, 2) for r in rates]}), flush=True)
    b.close()


if __name__ == "__main__":
    main()
