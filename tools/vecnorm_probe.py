"""Diagnostics: microseconds per collection step of ``DeviceRolloutBuffer.collect`` with and without a device-side
VecNormalize at 4096 envs x (4 drones, 16 cattle), f64, with the v16-6 actor and critic
(tests/golden/policy_ctde_v16_6.npz).

  --leg plain   ``collect(actor, critic, log_std)``: the collection as it is without a normaliser (with CH_LIB_PATH set
                to a parent commit's library this is the parent's leg; otherwise this build's).
  --leg norm    ``collect(..., normalizer=DeviceVecNormalize(batch))`` (ch_rollout_collect_norm).
  --leg kernels the two obs kernels alone on the batch's [4096, 1032] observation: ``update_obs`` (moments + merge)
                and ``normalize_obs`` (apply), --steps launches per window each; reports GB/s of the bytes they must
                move (one read; one read and one write).

One process runs one leg: --windows timed windows of one collection of --steps steps after a warm-up one, each ended
by a device synchronise.  Prints one JSON line.  Run the legs alternating (profiles/vecnorm/).
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
    ap.add_argument("--leg", choices=("plain", "norm", "kernels"), required=True)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.policy import DevicePolicy
    from cattleherd.rollout import DeviceRolloutBuffer
    d = np.load(os.path.join(ROOT, "tests", "golden", "policy_ctde_v16_6.npz"))
    sd = {k.replace("__", "."): torch.tensor(d[k]) for k in d.files if "__" in k}
    actor = DevicePolicy.sb3_actor(sd, clip=False, cache_packed=True)
    critic = DevicePolicy.sb3_critic(sd, cache_packed=True)
    b = HerdBatch(a.envs, 4, 16, mode="ctde", precision="f64")
    b.reset()
    log_std = torch.full((actor.dims[-1],), -1.0, device=b.device)
    out = {"leg": a.leg, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "code_object": _lib.code_object_hash(),
           "envs": a.envs, "steps": a.steps, "windows": a.windows}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / a.steps * 1e6)
        return us

    if a.leg == "kernels":
        from cattleherd.vec_normalize import DeviceVecNormalize
        n = DeviceVecNormalize(b)
        x = b.obs.view(a.envs, -1)
        nbytes = x.numel() * 4
        for name, fn, moved in (("update", lambda: [n.update_obs(x) for _ in range(a.steps)], nbytes),
                                ("apply", lambda: [n.normalize_obs(x, out=n.obs_n) for _ in range(a.steps)], 2 * nbytes)):
            us = timed(fn)
            out[name + "_us"] = [round(u, 2) for u in us]
            out[name + "_median_us"] = round(float(np.median(us)), 2)
            out[name + "_gb_per_s"] = round(moved / np.median(us) / 1e3, 1)
        out["obs_bytes"] = nbytes
    else:
        rb = DeviceRolloutBuffer(b, a.steps, act_dim=actor.dims[-1])
        kw = {}
        if a.leg == "norm":
            from cattleherd.vec_normalize import DeviceVecNormalize
            kw["normalizer"] = DeviceVecNormalize(b)
            kw["normalizer"].reset_obs()
        us = timed(lambda: rb.collect(actor, critic, log_std, seed=1, **kw))
        out["us_per_step"] = [round(u, 2) for u in us]
        out["median_us_per_step"] = round(float(np.median(us)), 2)
    b.sync()
    print(json.dumps(out), flush=True)
    b.close()


if __name__ == "__main__":
    main()
