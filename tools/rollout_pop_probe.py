"""Diagnostics: the population collection against solo collections.  The collection alone -- no
update -- with the driver's nets (1032-128-128-48 / 1032-128-128-1, packed), 2 drones x 8 cattle, --steps steps.  One
process runs one leg for one P and one E:

  --leg solo   P ch_rollout_collect calls one after another on P batches of E envs (env_id_offset p * E); the call an
               older library has too, so the same leg runs on a parent library through CH_LIB_PATH -- leg (a), on
               both libraries.  --copy: the solo copy-each-step path (ch__set_rollout_path bit 0), the path the
               population call restates
  --leg pop    one ch_rollout_collect_pop on one batch of P * E envs                               -- leg (b)

A window is one collection for all P members between two device synchronisations; two untimed windows, then --reps
timed ones.  Prints one JSON line: every window's milliseconds, their median with min and max, and member env-steps
per second at the median.  Launch each process under its own `timeout`, once, the legs alternating, never two at a
time."""
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
    ap.add_argument("--envs", type=int, default=32, help="envs per member")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--copy", action="store_true")
    a = ap.parse_args()
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.policy import DevicePolicy
    from cattleherd.rollout import DeviceRolloutBuffer
    P, E, T, n, m = a.members, a.envs, a.steps, 2, 8
    nets = []
    for p in range(P):
        actor = DevicePolicy(DevicePolicy.random_layers([12 * 86, 128, 128, 48], seed=10 + p), "tanh", None)
        critic = DevicePolicy(DevicePolicy.random_layers([12 * 86, 128, 128, 1], seed=20 + p), "tanh", None)
        nets.append((actor, critic, torch.full((48,), -1.0, device="cuda")))

    def batch(envs, offset):
        b = HerdBatch(envs, n, m, mode="ctde", curriculum_level=7, compat=False, env_id_offset=offset)
        b.reset()
        return b

    if a.leg == "pop":
        from cattleherd.rollout_pop import PopulationRollout
        b = batch(P * E, 0)
        pop = PopulationRollout(b, P, T, act_dim=48)

        def window():
            pop.collect([x[0] for x in nets], [x[1] for x in nets], [x[2] for x in nets], range(P))
    else:
        bs = [batch(E, p * E) for p in range(P)]
        if a.copy:
            for b in bs:
                assert _lib.lib().ch__set_rollout_path(b.handle, ctypes.c_int32(1)) == 0
        rbs = [DeviceRolloutBuffer(b, T, act_dim=48) for b in bs]

        def window():
            for p, rb in enumerate(rbs):
                rb.collect(*nets[p], seed=p)

    ms = []
    for r in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        window()
        torch.cuda.synchronize()
        if r >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    print(json.dumps({"leg": a.leg + ("_copy" if a.copy else ""), "members": P, "envs_per_member": E, "steps": T,
                      "library": os.path.relpath(_lib.LIB_PATH, ROOT), "code_object": _lib.code_object_hash(),
                      "ms_per_window": [round(x, 3) for x in ms], "median_ms": round(med, 3), "min": round(min(ms), 3),
                      "max": round(max(ms), 3), "member_env_steps_per_s": round(P * E * T * 1e3 / med, 1)}), flush=True)


if __name__ == "__main__":
    main()
