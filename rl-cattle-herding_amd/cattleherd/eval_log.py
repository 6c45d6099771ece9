"""Device-side evaluator log: the reference's per-step evaluation data without ``get_state``.

The reference's last workflow stage is playback with ``is_evaluating`` set: ``update_evaluation_metrics`` logs every
step into the ``evaluator`` (drone and cattle poses and velocities, per-drone travelled distance, herding
effectiveness, episode time) and ``evaluation_data.pkl`` is what the plots are drawn from (cattleherd.evaluation).
``DeviceEvalLog`` keeps those rows in a device table (``ch_eval_log``) for a chosen subset of a batch's envs, filled
by a small kernel after each step; ``run`` plays a policy and fills the table in one native call with no host
synchronisation (``ch_eval_log_run``); ``to_evaluators`` turns the table into the reference's ``Evaluator`` objects.

The one restriction: the recorder reads the post-step, pre-reset state, so the step under it must not auto-reset
(``batch.step(..., autoreset=False)``, then ``batch.reset(mask=done)``).  CTDE batches with ``eval_metrics`` only.
"""
import ctypes

import numpy as np

from . import _lib as L
from .evaluation import Evaluator

FLAG_TERMINATED, FLAG_TRUNCATED, FLAG_TIMEOUT = 1, 2, 4


def _actor(policy):
    """The DevicePolicy of the action mean: ``policy`` itself, or an ``SB3ActorCritic``'s actor over its live storage."""
    return policy.device_nets()[0] if hasattr(policy, "device_nets") else policy


class DeviceEvalLog:
    """``capacity`` rows for each env of ``envs`` (distinct indices of ``batch``), as device arrays.

    Per logged env ``s`` and row ``t``: ``time``, ``effectiveness`` float64 [S, T]; ``num_drones``, ``episode`` int32
    [S, T]; ``flags`` uint8 [S, T] (FLAG_TERMINATED, FLAG_TRUNCATED, FLAG_TIMEOUT: where the reference's
    ``evaluation_episode_trigger`` fires); ``drone_xy``, ``drone_vxy`` float64 [S, T, N, 2] and ``drone_dist``
    [S, T, N] (zero for drones >= num_drones); ``cattle_xy`` [S, T, M, 2] after the step and ``cattle_vxy`` at its
    start.  ``rows`` / ``dropped`` int32 [S]: rows written, and steps not logged because the rows were full.
    Every array lives in one device buffer, so ``arrays()`` is one copy."""

    ROW_ARRAYS = ("time", "effectiveness", "num_drones", "episode", "flags", "drone_xy", "drone_vxy", "drone_dist",
                  "cattle_xy", "cattle_vxy")
    ARRAYS = ("sel_env", "rows", "dropped") + ROW_ARRAYS + ("start_cattle_vxy", "start_counter")

    def __init__(self, batch, envs, capacity, guard=0):
        if batch.mode != L.CH_MODE_CTDE:
            raise ValueError("the evaluator log is for CTDE batches")
        if not batch.cfg.eval_metrics:
            raise ValueError("the evaluator log needs a batch created with eval_metrics=True")
        envs = np.asarray(envs, np.int64).reshape(-1)
        if envs.size < 1:
            raise ValueError("envs must name at least one env")
        if envs.min() < 0 or envs.max() >= batch.n_envs:
            raise ValueError(f"envs must lie in [0, {batch.n_envs})")
        if len(np.unique(envs)) != envs.size:
            raise ValueError("envs must be distinct (each logged env's rows are owned by one wave)")
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1")
        torch = batch.torch
        self.batch, self.envs = batch, envs.astype(np.int32)
        S, T, N, M = envs.size, self.capacity, batch.num_drones, batch.num_cattle
        f8, i4, u1 = (np.float64, torch.float64), (np.int32, torch.int32), (np.uint8, torch.uint8)
        spec = {"sel_env": (i4, (S,)), "rows": (i4, (S,)), "dropped": (i4, (S,)), "time": (f8, (S, T)),
                "effectiveness": (f8, (S, T)), "num_drones": (i4, (S, T)), "episode": (i4, (S, T)),
                "flags": (u1, (S, T)), "drone_xy": (f8, (S, T, N, 2)), "drone_vxy": (f8, (S, T, N, 2)),
                "drone_dist": (f8, (S, T, N)), "cattle_xy": (f8, (S, T, M, 2)), "cattle_vxy": (f8, (S, T, M, 2)),
                "start_cattle_vxy": (f8, (S, M, 2)), "start_counter": (i4, (S,))}
        # one buffer, every array at a 256-byte boundary and followed by `guard` bytes nothing writes (tests)
        self._layout, off = {}, 0
        for k in self.ARRAYS:
            (npdt, _), shape = spec[k]
            nbytes = int(np.prod(shape)) * np.dtype(npdt).itemsize
            self._layout[k] = (off, nbytes, npdt, shape)
            off = -(-(off + nbytes + int(guard)) // 256) * 256
        self._buf = torch.zeros(off, dtype=torch.uint8, device=batch.device)
        lg = L.ChEvalLog()
        lg.n_sel, lg.capacity = S, T
        for k in self.ARRAYS:
            o, nbytes, _, shape = self._layout[k]
            t = self._buf[o:o + nbytes].view(spec[k][0][1]).view(shape)
            setattr(self, k, t)
            setattr(lg, k, t.data_ptr())
        self._lg = lg
        self.sel_env.copy_(torch.from_numpy(self.envs))
        self._mean = None
        self.env_actions = torch.zeros((batch.n_envs, N, 4), dtype=torch.float32, device=batch.device)
        self.done_mask = torch.zeros(batch.n_envs, dtype=torch.uint8, device=batch.device)
        self._lib = L.lib()
        self.begin()

    # ---- the three kernels -------------------------------------------------------------------------------------------
    def begin(self):
        """Empty the table: ``rows = dropped = 0`` (ch_eval_log_begin)."""
        b = self.batch
        L.check(self._lib.ch_eval_log_begin(b.handle, ctypes.byref(self._lg), b._stream()), b.handle)
        return self

    def mark(self):
        """Before a step: keep the cattle velocities and the step counter of the step's start (ch_eval_log_mark)."""
        b = self.batch
        L.check(self._lib.ch_eval_log_mark(b.handle, ctypes.byref(self._lg), b._stream()), b.handle)

    def record(self, io=None):
        """After a step WITHOUT auto-reset, before the reset of the envs it ended: one row per logged env
        (ch_eval_log_record on the batch's step outputs, or on another ``ChStepIO``)."""
        b = self.batch
        L.check(self._lib.ch_eval_log_record(b.handle, ctypes.byref(self._lg),
                                             b._io_ref if io is None else ctypes.byref(io), b._stream()), b.handle)

    # ---- the playback loop -------------------------------------------------------------------------------------------
    def _scratch(self, actor):
        b = self.batch
        if self._mean is None or self._mean.shape[1] != actor.dims[-1]:
            self._mean = b.torch.zeros((b.n_envs, actor.dims[-1]), dtype=b.torch.float32, device=b.device)
        return self._mean

    def run(self, policy, n_steps):
        """``n_steps`` steps of every env under the deterministic ``policy`` (a ``DevicePolicy`` of the action mean or
        an ``SB3ActorCritic``) in one native call (ch_eval_log_run): forward, clamp, mark, step, record, masked reset.
        No host synchronisation; ``batch.sync()`` afterwards reports a device error."""
        b = self.batch
        actor = _actor(policy)
        actor._ensure_packed()
        sio = L.ChStepIO()
        ctypes.memmove(ctypes.byref(sio), ctypes.byref(b._io), ctypes.sizeof(sio))
        sio.flags, sio.terminal_obs = 0, None
        io = L.ChEvalLogIO()
        io.step = ctypes.pointer(sio)
        io.mean, io.env_actions = self._scratch(actor).data_ptr(), self.env_actions.data_ptr()
        io.done_mask = self.done_mask.data_ptr()
        L.check(self._lib.ch_eval_log_run(b.handle, ctypes.byref(actor._net), ctypes.byref(self._lg), ctypes.byref(io),
                                          int(n_steps), b._stream()), b.handle)
        return int(n_steps)

    def run_steps(self, policy, n_steps, log=True):
        """The same loop written with the existing Python primitives, one kernel at a time (the loop the native call
        restates; the reference of the parity test and, with ``log=False``, the bookkeeping-free baseline)."""
        b = self.batch
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        actor = _actor(policy)
        mean = self._scratch(actor)
        w = b.num_drones * 4
        if actor.dims[-1] < w:
            raise ValueError(f"the actor's output ({actor.dims[-1]} wide) must be at least num_drones * 4 = {w} wide")
        for _ in range(n_steps):
            actor.forward_batch(b, mean)
            self.env_actions.copy_(mean[:, :w].clamp(-1.0, 1.0).reshape(b.n_envs, b.num_drones, 4))
            if log:
                self.mark()
            _, _, te, tr = b.step(self.env_actions, autoreset=False)
            if log:
                self.record()
            b.torch.bitwise_or(te[:, 0], tr[:, 0], out=self.done_mask)
            b.reset(mask=self.done_mask)
        return n_steps

    # ---- the host side -----------------------------------------------------------------------------------------------
    def _host(self):
        return self._buf.cpu().numpy()   # one copy (synchronises)

    def _view(self, host, k):
        o, nbytes, npdt, shape = self._layout[k]
        return host[o:o + nbytes].view(npdt).reshape(shape)

    def guard_bytes(self):
        """Tests: the bytes of the buffer that belong to no array (the gap after each one), as one numpy array."""
        host = self._host()
        keep = np.ones(host.size, bool)
        for o, nbytes, _, _ in self._layout.values():
            keep[o:o + nbytes] = False
        return host[keep]

    def arrays(self):
        """Every array as numpy after one device-to-host copy: ``sel_env``, ``rows``, ``dropped`` [S] and the row
        arrays trimmed to the rows written ([S, max(rows), ...]; env ``s`` holds ``rows[s]`` of them)."""
        host = self._host()
        out = {k: self._view(host, k).copy() for k in ("sel_env", "rows", "dropped")}
        r = int(min(max(int(out["rows"].max()), 0), self.capacity))
        for k in self.ROW_ARRAYS:
            out[k] = self._view(host, k)[:, :r].copy()
        return out

    def to_evaluators(self, arrays=None):
        """One ``cattleherd.evaluation.Evaluator`` per logged env, holding what an ``EvalTracker`` fed the same steps
        would hold (see ``evaluators_from_arrays``)."""
        return evaluators_from_arrays(self.arrays() if arrays is None else arrays)

    def save_evaluation_data(self, path="evaluation_data.pkl", env=0):
        """Write logged env number ``env`` (an index into ``envs``) as the reference's ``evaluation_data.pkl``."""
        self.to_evaluators()[int(env)].save_evaluation_data(path)


def evaluators_from_arrays(a):
    """Replay the rows of ``DeviceEvalLog.arrays()`` through ``EvalTracker``'s data flow (cattleherd.evaluation):
    * a fresh distance list (``on_reset``) at the first row and wherever ``episode`` changes; every row's distances are
      that list object, updated in place, so all rows of an episode show its final distances -- and the first row
      after a time-out, logged before the reset, shows the previous episode's;
    * a row with FLAG_TIMEOUT first appends two episode entries (``evaluation_episode_trigger`` fires in both
      ``_computeTruncated`` calls of the step), so the time-out step itself is logged into the next episode."""
    out = []
    for s in range(len(a["rows"])):
        ev = Evaluator()
        dist = []
        for k in range(int(a["rows"][s])):
            n = int(a["num_drones"][s, k])
            if k == 0 or a["episode"][s, k] != a["episode"][s, k - 1]:
                dist = [np.zeros(2) for _ in range(n)]   # _housekeeping (BaseAviary.py:683-688)
            for i, d in enumerate(dist):
                d[:] = a["drone_dist"][s, k, i]
            drone_poses = np.array(a["drone_xy"][s, k, :n], np.float64)
            cattle_poses = np.array(a["cattle_xy"][s, k], np.float64)
            ep_time, eff = float(a["time"][s, k]), float(a["effectiveness"][s, k])
            if a["flags"][s, k] & FLAG_TIMEOUT:
                for _ in range(2):
                    ev.append_episode_data(dist, n, ep_time, eff)
            ev.append_timestep_data(dist, ep_time, eff, drone_poses, cattle_poses,
                                    np.array(a["drone_vxy"][s, k, :n], np.float64),
                                    np.array(a["cattle_vxy"][s, k], np.float64))
        out.append(ev)
    return out


def save_evaluation_data(log, path="evaluation_data.pkl", env=0):
    """``log.save_evaluation_data(path, env=env)``: the reference's pickle of one logged env."""
    log.save_evaluation_data(path, env=env)
