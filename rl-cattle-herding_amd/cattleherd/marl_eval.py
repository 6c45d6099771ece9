"""On-device evaluation of the DTDE driver's shared policy (``ch_marl_eval_*``): the third stage of train, sample and
evaluate for MARL batches.

The reference plays a trained RLlib policy back through ``RLlibMultiAgentWrapper`` envs (``DTDEModelPlayback.py``) and
RLlib reports ``evaluation`` metrics -- ``episode_return_mean``, ``episode_len_mean``, per-agent returns.
``evaluate_marl_policy`` runs that on the GPU in one native call (``ch_marl_evaluate_policy``): the shared policy's
forward over every agent row, the deterministic action (``explore=False`` on a DiagGaussian: the mean half, clipped to
the Box), the env step with auto-reset, and a recorder kernel that keeps each agent's return and length and files every
ended episode into a device table (``DeviceMarlEvalTable``) under the CTDE table's per-env quota.  The host reads one
integer every ``check_every`` steps.

An episode is the wrapper's (``marl_wrapper.py:77-119``): agents that terminate drop out, the env ends once every agent
has terminated, and a truncation ends nothing -- so no step cap follows from a time limit and ``max_steps`` is
required.  RLlib is not installed here: the restatement is "parity unpinned" to its source.  MARL batches with the
wrapper's semantics (``marl_wrapper=True``) only.
"""
import ctypes

import numpy as np

from . import _lib as L


def _policy(policy):
    """The DevicePolicy of the shared policy: ``policy`` itself, or an ``RLlibActorCritic``'s over its live storage."""
    return policy.device_nets()[0] if hasattr(policy, "device_nets") else policy


class DeviceMarlEvalTable:
    """The episodes of one evaluation as device arrays (``ch_marl_eval_table``): ``capacity`` slots per env.

    ``quota`` / ``count`` int32 [E]; ``ep_return`` float64 [E, C] and ``agent_return`` float64 [E, C, N];
    ``ep_length`` / ``ep_end_step`` int32 [E, C] and ``agent_length`` int32 [E, C, N]; ``remaining`` int64 [1].  Slot
    ``[e, k]`` is valid for ``k < count[e]``.  The current episodes' running state: ``acc_return`` float64 [E, N],
    ``acc_length`` int32 [E, N], ``acc_steps`` int32 [E] and ``live`` uint8 [E, N] (the agents live at the start of
    the step about to run / that just ran)."""

    ARRAYS = ("quota", "count", "ep_return", "agent_return", "ep_length", "agent_length", "ep_end_step", "remaining",
              "acc_return", "acc_length", "acc_steps", "live")

    def __init__(self, batch, capacity):
        if batch.mode != L.CH_MODE_MARL:
            raise ValueError("the per-agent episode table is for MARL batches")
        torch = batch.torch
        self.batch, self.capacity = batch, int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1")
        E, C, N = batch.n_envs, self.capacity, batch.num_drones
        z = dict(device=batch.device)
        self.quota = torch.zeros(E, dtype=torch.int32, **z)
        self.count = torch.zeros(E, dtype=torch.int32, **z)
        self.ep_return = torch.zeros((E, C), dtype=torch.float64, **z)
        self.agent_return = torch.zeros((E, C, N), dtype=torch.float64, **z)
        self.ep_length = torch.zeros((E, C), dtype=torch.int32, **z)
        self.agent_length = torch.zeros((E, C, N), dtype=torch.int32, **z)
        self.ep_end_step = torch.zeros((E, C), dtype=torch.int32, **z)
        self.remaining = torch.zeros(1, dtype=torch.int64, **z)
        self.acc_return = torch.zeros((E, N), dtype=torch.float64, **z)
        self.acc_length = torch.zeros((E, N), dtype=torch.int32, **z)
        self.acc_steps = torch.zeros(E, dtype=torch.int32, **z)
        self.live = torch.zeros((E, N), dtype=torch.uint8, **z)
        tb = L.ChMarlEvalTable()
        tb.capacity = C
        for k in self.ARRAYS:
            setattr(tb, k, getattr(self, k).data_ptr())
        self._tb = tb
        self._out = None   # scratch of run / run_steps: the policy's output [E * N, width]
        self.env_actions = torch.zeros((E, N, 4), dtype=torch.float32, **z)
        self._lib = L.lib()

    def begin(self, n_eval_episodes):
        """Start an evaluation of ``n_eval_episodes`` episodes (ch_marl_eval_begin): quotas set, counts and the running
        state zeroed."""
        b = self.batch
        L.check(self._lib.ch_marl_eval_begin(b.handle, ctypes.byref(self._tb), int(n_eval_episodes), b._stream()),
                b.handle)
        return self

    def mark(self):
        """Before a step: ``live`` = the agents the wrapper has acting now (ch_marl_eval_mark)."""
        b = self.batch
        L.check(self._lib.ch_marl_eval_mark(b.handle, ctypes.byref(self._tb), b._stream()), b.handle)

    def record(self, step_index, io=None):
        """After a step: the live agents' rewards into the running sums, and the episodes that ended in the step into
        the table (ch_marl_eval_record on the batch's step outputs, or on another ``ChStepIO``)."""
        b = self.batch
        L.check(self._lib.ch_marl_eval_record(b.handle, ctypes.byref(self._tb),
                                              b._io_ref if io is None else ctypes.byref(io), int(step_index),
                                              b._stream()), b.handle)

    def _scratch(self, net):
        b = self.batch
        if self._out is None or self._out.shape[1] != net.dims[-1]:
            self._out = b.torch.zeros((b.n_envs * b.num_drones, net.dims[-1]), dtype=b.torch.float32, device=b.device)
        return self._out

    def run(self, policy, max_steps, check_every=16, first_step_index=0):
        """The evaluation loop in one native call (ch_marl_evaluate_policy) from the batch's current state and this
        table's current counts; returns ``(steps_run, remaining)``.  Stops when every quota is filled (seen at a
        multiple of ``check_every`` steps) or after ``max_steps``; hitting the cap is not an error here."""
        b = self.batch
        net = _policy(policy)
        net._ensure_packed()
        io = L.ChMarlEvalIO()
        io.step = ctypes.pointer(b._io)
        io.policy_out, io.env_actions = self._scratch(net).data_ptr(), self.env_actions.data_ptr()
        steps, rem = ctypes.c_int64(), ctypes.c_int64()
        L.check(self._lib.ch_marl_evaluate_policy(b.handle, ctypes.byref(net._net), ctypes.byref(self._tb),
                                                  ctypes.byref(io), int(max_steps), int(check_every),
                                                  int(first_step_index), ctypes.byref(steps), ctypes.byref(rem),
                                                  b._stream()), b.handle)
        return steps.value, rem.value

    def run_steps(self, policy, max_steps, check_every=16, first_step_index=0, on_step=None):
        """The same loop driven from Python one kernel at a time (the loop the native call restates; kept for the
        parity test): forward, mark, torch's clamp and slice masked by ``live``, step, record; ``remaining`` read every
        ``check_every`` steps.  ``on_step(t)`` is called after step ``t`` was recorded, with the step's outputs and
        ``live`` still in place."""
        b = self.batch
        torch = b.torch
        max_steps, check_every = int(max_steps), int(check_every)
        if max_steps < 1 or check_every < 1:
            raise ValueError("max_steps and check_every must be >= 1")
        net = _policy(policy)
        out = self._scratch(net)
        if net.dims[-1] < 4:
            raise ValueError(f"the policy's output ({net.dims[-1]} wide) must be at least 4 wide")
        E, N = b.n_envs, b.num_drones
        zero = torch.zeros((), dtype=torch.float32, device=b.device)
        t, rem = 0, -1
        while t < max_steps:
            net.forward_batch(b, out)
            self.mark()
            act = out[:, :4].clamp(-1.0, 1.0).reshape(E, N, 4)
            self.env_actions.copy_(torch.where(self.live[:, :, None] != 0, act, zero))
            b.step(self.env_actions, autoreset=True, terminal_obs=False)
            self.record(first_step_index + t)
            if on_step is not None:
                on_step(first_step_index + t)
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
        """The recorded episodes ordered by the step they ended in, then by env index: ``(returns float64 [k],
        lengths int64 [k], agent_returns float64 [k, N], agent_lengths int64 [k, N], env int64 [k], end_step int64
        [k])``."""
        return table_episodes(self.arrays(), self.capacity)


def table_episodes(a, capacity):
    """``DeviceMarlEvalTable.episodes()`` of the table arrays ``a`` (numpy, ``ARRAYS``' names)."""
    env, slot = np.nonzero(np.arange(int(capacity))[None, :] < a["count"][:, None])
    end = a["ep_end_step"][env, slot].astype(np.int64)
    order = np.lexsort((env, end))
    env, slot, end = env[order], slot[order], end[order]
    return (a["ep_return"][env, slot], a["ep_length"][env, slot].astype(np.int64), a["agent_return"][env, slot],
            a["agent_length"][env, slot].astype(np.int64), env.astype(np.int64), end)


def episode_metrics(returns, lengths, agent_returns, agent_lengths):
    """RLlib's evaluation metrics of a list of episodes: ``episode_return_mean`` / ``_min`` / ``_max``,
    ``episode_len_mean``, ``num_episodes`` and ``agent_episode_returns_mean`` -- ``{"agent_i": mean of agent i's
    return over the episodes it took part in}`` (``agent_lengths[:, i] > 0``; an agent of no episode has no key)."""
    returns, lengths = np.asarray(returns, np.float64), np.asarray(lengths, np.int64)
    agent_returns = np.asarray(agent_returns, np.float64).reshape(len(returns), -1)
    agent_lengths = np.asarray(agent_lengths, np.int64).reshape(len(returns), -1)
    if len(returns) == 0:
        raise ValueError("episode_metrics: no episode")
    per_agent = {}
    for i in range(agent_returns.shape[1]):
        took_part = agent_lengths[:, i] > 0
        if took_part.any():
            per_agent[f"agent_{i}"] = float(np.mean(agent_returns[took_part, i]))
    return {"episode_return_mean": float(np.mean(returns)), "episode_return_min": float(np.min(returns)),
            "episode_return_max": float(np.max(returns)), "episode_len_mean": float(np.mean(lengths)),
            "agent_episode_returns_mean": per_agent, "num_episodes": int(len(returns))}


def _evaluate(run, batch, policy, n_eval_episodes, max_steps, check_every, reset, return_episodes):
    if max_steps is None:
        raise ValueError("evaluate_marl_policy: max_steps is required -- a truncation does not end an episode under "
                         "the wrapper's \"__all__\" rule, so no cap follows from the time limit")
    n = int(n_eval_episodes)
    table = DeviceMarlEvalTable(batch, max(-(-n // batch.n_envs), 1))
    if reset:
        batch.reset()
    table.begin(n)
    steps, remaining = getattr(table, run)(policy, max_steps, check_every)
    if remaining != 0:
        raise RuntimeError(f"evaluate_marl_policy: remaining = {remaining} of {n} episodes after max_steps = {steps} "
                           "steps")
    eps = table.episodes()
    if return_episodes:
        return dict(zip(("episode_returns", "episode_lengths", "agent_returns", "agent_lengths", "env", "end_step"), eps))
    return episode_metrics(*eps[:4])


def evaluate_marl_policy(batch, policy, n_eval_episodes, max_steps=None, check_every=16, reset=True,
                         return_episodes=False):
    """Evaluate the shared DTDE policy on ``batch`` (MARL, wrapper semantics) for ``n_eval_episodes`` episodes, in one
    native call.

    ``policy``: a ``DevicePolicy`` whose first 4 outputs per agent row are the action mean (e.g.
    ``DevicePolicy.rllib_policy(w)``: 8 wide, mean then log_std), or a ``cattleherd.marl_ppo.RLlibActorCritic``, whose
    policy net is read over its live storage and re-packed, so an optimizer step is seen.  ``reset``:
    ``batch.reset()`` first.  Returns ``episode_metrics``' dict under RLlib's names, or with ``return_episodes`` the
    per-episode arrays (``episode_returns``, ``episode_lengths``, ``agent_returns``, ``agent_lengths``, ``env``,
    ``end_step``; ordered by end step, then env).  ``max_steps`` bounds the loop and is required (``ValueError``
    without it); ``RuntimeError`` naming ``remaining`` if it is hit."""
    return _evaluate("run", batch, policy, n_eval_episodes, max_steps, check_every, reset, return_episodes)


def evaluate_marl_policy_steps(batch, policy, n_eval_episodes, max_steps=None, check_every=16, reset=True,
                               return_episodes=False):
    """``evaluate_marl_policy`` driven from Python one kernel at a time (``DeviceMarlEvalTable.run_steps``): the loop
    the native call restates, kept for the parity tests."""
    return _evaluate("run_steps", batch, policy, n_eval_episodes, max_steps, check_every, reset, return_episodes)
