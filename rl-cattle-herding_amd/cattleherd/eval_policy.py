"""On-device ``evaluate_policy`` for the CTDE driver.

The reference evaluates with stable_baselines3: ``EvalCallback`` every ``eval_freq`` steps during training
(simulator/CTDECattleHerder.py:139-148) and ``evaluate_policy(model, env, n_eval_episodes=5)`` after it (:185) --
deterministic episodes, each one's Monitor return and length appended to a list, ``mean +- std`` the model-selection
signal, ``evaluations.npz`` the log.  ``evaluate_policy`` here runs that loop on the GPU in one native call
(``ch_evaluate_policy``): policy forward, clip to the action Box, env step with auto-reset, and a recorder kernel that
files each ended episode into a device table (``DeviceEvalTable``) under SB3's per-env episode quota.  The host reads
one integer every ``check_every`` steps to know when to stop.

Semantics restated from SB3 2.x ``evaluation.evaluate_policy`` / ``callbacks.EvalCallback``; SB3 is not installed
here, so the restatement is "parity unpinned" to its source.  CTDE batches only.
"""
import ctypes

import numpy as np

from . import _lib as L
from .spaces import CURRICULUM, DEFAULT_LEVEL


def episode_quota(n_eval_episodes, n_envs):
    """SB3's ``episode_count_targets``: how many of the ``n_eval_episodes`` each env contributes (int32 [n_envs]); the
    integer division leaves the later envs with one episode more."""
    return ((int(n_eval_episodes) + np.arange(int(n_envs), dtype=np.int64)) // int(n_envs)).astype(np.int32)


def max_episode_steps(batch):
    """The longest episode of ``batch`` in steps: the time limit of its curriculum level (the table entry
    ``CattleHerdVecEnv._episode_len`` reads) as the step kernel applies it -- the counter advances by the physics
    substeps and is compared with ``EPISODE_LEN_SEC * CTRL_FREQ`` before the step, so an episode is truncated by the
    step after the first one past the limit (602 steps for 40 s, 1202 for 80 s: SURVEY.md §5)."""
    cfg = batch.cfg
    lvl = cfg.curriculum_level
    sec = CURRICULUM[DEFAULT_LEVEL["ctde"] if lvl < 0 else lvl][2]
    substeps = cfg.pyb_freq // cfg.ctrl_freq
    return (sec * cfg.ctrl_freq) // substeps + 2


def _actor(policy):
    """The DevicePolicy of the action mean: ``policy`` itself, or an ``SB3ActorCritic``'s actor over its live storage."""
    return policy.device_nets()[0] if hasattr(policy, "device_nets") else policy


class DeviceEvalTable:
    """The episode lists of one evaluation as device arrays (``ch_eval_table``): ``capacity`` slots per env.

    ``quota`` / ``count`` int32 [E], ``ep_return`` float64 [E, C], ``ep_length`` / ``ep_end_step`` int32 [E, C],
    ``ep_flags`` uint8 [E, C] (bit 0 terminated, bit 1 truncated), ``remaining`` int64 [1].  Slot ``[e, k]`` is valid
    for ``k < count[e]``."""

    ARRAYS = ("quota", "count", "ep_return", "ep_length", "ep_flags", "ep_end_step", "remaining")

    def __init__(self, batch, capacity):
        if batch.mode != L.CH_MODE_CTDE:
            raise ValueError("the episode table is for CTDE batches")
        torch = batch.torch
        self.batch, self.capacity = batch, int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1")
        E, C = batch.n_envs, self.capacity
        z = dict(device=batch.device)
        self.quota = torch.zeros(E, dtype=torch.int32, **z)
        self.count = torch.zeros(E, dtype=torch.int32, **z)
        self.ep_return = torch.zeros((E, C), dtype=torch.float64, **z)
        self.ep_length = torch.zeros((E, C), dtype=torch.int32, **z)
        self.ep_flags = torch.zeros((E, C), dtype=torch.uint8, **z)
        self.ep_end_step = torch.zeros((E, C), dtype=torch.int32, **z)
        self.remaining = torch.zeros(1, dtype=torch.int64, **z)
        tb = L.ChEvalTable()
        tb.capacity = C
        for k in self.ARRAYS:
            setattr(tb, k, getattr(self, k).data_ptr())
        self._tb = tb
        self._mean = None   # scratch of run / run_steps: the actor's output [E, width]
        self.env_actions = torch.zeros((E, batch.num_drones, 4), dtype=torch.float32, **z)
        self._lib = L.lib()

    def begin(self, n_eval_episodes):
        """Start an evaluation of ``n_eval_episodes`` episodes (ch_eval_begin): quotas set, counts zeroed."""
        b = self.batch
        L.check(self._lib.ch_eval_begin(b.handle, ctypes.byref(self._tb), int(n_eval_episodes), b._stream()), b.handle)
        return self

    def record(self, step_index, io=None):
        """File the episodes that ended in the step that just ran (ch_eval_record on the batch's step outputs, or on
        another ``ChStepIO``)."""
        b = self.batch
        L.check(self._lib.ch_eval_record(b.handle, ctypes.byref(self._tb), b._io_ref if io is None else ctypes.byref(io),
                                         int(step_index), b._stream()), b.handle)

    def _scratch(self, actor):
        b = self.batch
        if self._mean is None or self._mean.shape[1] != actor.dims[-1]:
            self._mean = b.torch.zeros((b.n_envs, actor.dims[-1]), dtype=b.torch.float32, device=b.device)
        return self._mean

    def run(self, policy, max_steps, check_every=16, first_step_index=0):
        """The evaluation loop in one native call (ch_evaluate_policy) from the batch's current state and this table's
        current counts; returns ``(steps_run, remaining)``.  Stops when every quota is filled (seen at a multiple of
        ``check_every`` steps) or after ``max_steps``; hitting the cap is not an error here."""
        b = self.batch
        actor = _actor(policy)
        actor._ensure_packed()
        io = L.ChEvalIO()
        io.step = ctypes.pointer(b._io)
        io.mean, io.env_actions = self._scratch(actor).data_ptr(), self.env_actions.data_ptr()
        steps, rem = ctypes.c_int64(), ctypes.c_int64()
        L.check(self._lib.ch_evaluate_policy(b.handle, ctypes.byref(actor._net), ctypes.byref(self._tb), ctypes.byref(io),
                                             int(max_steps), int(check_every), int(first_step_index),
                                             ctypes.byref(steps), ctypes.byref(rem), b._stream()), b.handle)
        return steps.value, rem.value

    def run_steps(self, policy, max_steps, check_every=16, first_step_index=0, normalizer=None):
        """The same loop driven from Python one kernel at a time (the loop the native call restates; kept for the
        parity test): forward, clamp and slice, step, record; ``remaining`` read every ``check_every`` steps.
        ``normalizer`` (a ``vec_normalize.DeviceVecNormalize`` of this batch): the actor reads the observation
        normalised with its statistics as they stand -- they are never updated here, as SB3 evaluates with
        ``training=False`` -- through the dense forward (a normalised feature past ``NUM_DRONES`` is not zero)."""
        b = self.batch
        max_steps, check_every = int(max_steps), int(check_every)
        if max_steps < 1 or check_every < 1:
            raise ValueError("max_steps and check_every must be >= 1")
        actor = _actor(policy)
        mean = self._scratch(actor)
        w = b.num_drones * 4
        if actor.dims[-1] < w:
            raise ValueError(f"the actor's output ({actor.dims[-1]} wide) must be at least num_drones * 4 = {w} wide")
        if normalizer is not None and getattr(normalizer, "batch", None) is not b:
            raise ValueError("the normalizer belongs to another batch")
        t, rem = 0, -1
        while t < max_steps:
            if normalizer is None:
                actor.forward_batch(b, mean)
            else:
                actor.forward(normalizer.normalize_obs(b.obs.view(b.n_envs, -1), out=normalizer.obs_n), mean)
            self.env_actions.copy_(mean[:, :w].clamp(-1.0, 1.0).reshape(b.n_envs, b.num_drones, 4))
            b.step(self.env_actions, autoreset=True, terminal_obs=False)
            self.record(first_step_index + t)
            t += 1
            if t % check_every == 0 or t == max_steps:
                rem = int(self.remaining.item())
                b.sync()
                if rem == 0:
                    break
        return t, rem

    def arrays(self):
        """Every table array as numpy (one copy each; synchronises)."""
        return {k: getattr(self, k).cpu().numpy() for k in self.ARRAYS}

    def episodes(self):
        """The recorded episodes in SB3's append order -- by the step they ended in, then by env index:
        ``(returns float64, lengths int64, flags uint8, env int64, end_step int64)``."""
        a = self.arrays()
        env, slot = np.nonzero(np.arange(self.capacity)[None, :] < a["count"][:, None])
        end = a["ep_end_step"][env, slot].astype(np.int64)
        order = np.lexsort((env, end))
        env, slot, end = env[order], slot[order], end[order]
        return (a["ep_return"][env, slot], a["ep_length"][env, slot].astype(np.int64), a["ep_flags"][env, slot],
                env.astype(np.int64), end)


def _evaluate(run, batch, policy, n_eval_episodes, max_steps, check_every, reset, return_episode_rewards,
              monitor_rounding, **run_kw):
    n = int(n_eval_episodes)
    per_env = -(-n // batch.n_envs)
    table = DeviceEvalTable(batch, max(per_env, 1))
    if max_steps is None:
        max_steps = per_env * (max_episode_steps(batch) + 1)
    if reset:
        batch.reset()
    table.begin(n)
    steps, remaining = getattr(table, run)(policy, max_steps, check_every, **run_kw)
    if remaining != 0:
        raise RuntimeError(f"evaluate_policy: remaining = {remaining} of {n} episodes after max_steps = {steps} steps")
    returns, lengths = table.episodes()[:2]
    if monitor_rounding:
        returns = np.round(returns, 6)   # Monitor.step rounds the episode return (vec_env.py step_wait does too)
    if return_episode_rewards:
        return returns.tolist(), lengths.tolist()
    return float(np.mean(returns)), float(np.std(returns))


def evaluate_policy(batch, policy, n_eval_episodes=5, max_steps=None, check_every=16, reset=True,
                    return_episode_rewards=False, monitor_rounding=True):
    """SB3 ``evaluate_policy(model, env, n_eval_episodes, deterministic=True)`` on the device, in one native call.

    ``policy``: a ``DevicePolicy`` of the action mean (clipped or not: the loop clips to [-1, 1] itself), or an
    ``SB3ActorCritic``, whose actor is read over its live storage and re-packed, so an optimizer step is seen.
    ``reset``: ``batch.reset()`` first, as SB3 resets the env.  Returns ``(mean, std)`` of the episode returns
    (``np.mean`` / ``np.std``), or the ``(returns, lengths)`` lists in SB3's append order with
    ``return_episode_rewards``; ``monitor_rounding`` rounds the returns to 6 decimals as ``Monitor`` does.
    ``max_steps`` (default ``ceil(n / E) * (max_episode_steps(batch) + 1)``, enough for every env's quota of episodes
    that all run to their time limit) bounds the loop: ``RuntimeError`` naming ``remaining`` if it is hit."""
    return _evaluate("run", batch, policy, n_eval_episodes, max_steps, check_every, reset, return_episode_rewards,
                     monitor_rounding)


def evaluate_policy_steps(batch, policy, n_eval_episodes=5, max_steps=None, check_every=16, reset=True,
                          return_episode_rewards=False, monitor_rounding=True, normalizer=None):
    """``evaluate_policy`` driven from Python one kernel at a time (``DeviceEvalTable.run_steps``): the loop the native
    call restates, kept for the parity tests, as ``collect_steps`` is for ``collect``.  ``normalizer``: evaluate a
    policy trained under a ``DeviceVecNormalize`` -- observations normalised with its frozen statistics, dense forward
    (``run_steps``); the returns are the raw ones, as SB3 evaluates with ``norm_reward=False``."""
    kw = {} if normalizer is None else {"normalizer": normalizer}
    return _evaluate("run_steps", batch, policy, n_eval_episodes, max_steps, check_every, reset, return_episode_rewards,
                     monitor_rounding, **kw)


class EvalLog:
    """``EvalCallback``'s ``evaluations.npz``: ``timesteps`` [k], ``results`` [k, n] (episode returns),
    ``ep_lengths`` [k, n], one row per evaluation."""

    def __init__(self):
        self.timesteps, self.results, self.ep_lengths = [], [], []

    def add(self, timesteps, rewards, lengths):
        if len(rewards) != len(lengths) or (self.results and len(rewards) != len(self.results[0])):
            raise ValueError("every evaluation logs the same number of episode returns and lengths")
        self.timesteps.append(int(timesteps))
        self.results.append([float(r) for r in rewards])
        self.ep_lengths.append([int(n) for n in lengths])

    def save(self, path):
        np.savez(path, timesteps=np.asarray(self.timesteps, np.int64),
                 results=np.asarray(self.results, np.float64).reshape(len(self.timesteps), -1),
                 ep_lengths=np.asarray(self.ep_lengths, np.int64).reshape(len(self.timesteps), -1))
