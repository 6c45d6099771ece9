"""The SB3 logger record of a native training run, from device-side data.

The reference is trained by watching SB3's logger: ``rollout/ep_rew_mean`` and ``rollout/ep_len_mean`` are the means
over ``ep_info_buffer``, a ``deque(maxlen=stats_window_size)`` that ``OnPolicyAlgorithm._update_info_buffer`` fills
with Monitor's ``info["episode"]`` step by step, in env order, inside ``collect_rollouts``; the ``train/`` keys come
from ``PPO.train``.  ``EpisodeRing`` is that deque as a ring in device memory, appended to by one small kernel per step
(``ch_ep_ring_record``; inside the native collection with ``DeviceRolloutBuffer.collect(..., ring=ring)``), read with
one small copy when the record is wanted.  The ``train/`` half is ``PPOUpdate(..., log_stats=True)`` (cattleherd/ppo.py),
over ``ch_ppo_train_log`` (``ch_ppo_train_opt`` with ``target_kl`` / ``clip_range_vf``), ``explained_variance`` and
``sb3_train_record`` below.

Semantics restated from SB3 2.x; SB3 is not installed here, so the restatement is "parity unpinned" to its source.
One difference is deliberate: SB3's ``explained_variance`` is float32 numpy, here the float32 inputs are widened
exactly and every sum is float64 (two passes: the means, then the squared deviations).  CTDE batches only.

A population (``PopulationRollout`` / ``PPOPopulation``) is watched member by member: ``PopulationEpisodeRing`` holds
one ring per member, filled by one launch per step inside ``PopulationRollout.collect(..., ring=ring)``, each row bit
for bit the member's solo ``EpisodeRing``; ``fitness()`` is the ``[P, 4]`` table (count, mean return, mean length,
total) reduced on the device, and ``explained_variance_pop`` the P explained variances in one set of launches.

The DTDE (MARL) driver is watched through RLlib's result dict instead: ``MarlEpisodeRing`` is the env runners' window
of the last ``metrics_num_episodes_for_smoothing`` episodes with per-agent returns, and their sampling counters, as
device arrays (``ch_marl_ep_ring``; inside the native collection with ``DeviceMarlRolloutBuffer.collect(...,
ring=ring)``); ``MarlPPOUpdate(..., log_stats=True)`` (cattleherd/marl_ppo.py) holds the learner's keys, and
``rllib_result`` nests the two as RLlib does.  RLlib is not installed either: restated, "parity unpinned".
"""
import ctypes

import numpy as np

from . import _lib as L


def summary_of(entries):
    """``{"rollout/ep_rew_mean", "rollout/ep_len_mean"}`` over ``(r, l, env)`` entries as SB3 logs them: ``np.mean``
    (``safe_mean``) of the returns rounded to 6 decimals (Monitor's ``round(ep_rew, 6)``, as ``vec_env.py`` rounds
    it) and of the lengths.  Empty for no entries: SB3 logs neither key while ``ep_info_buffer`` is empty."""
    if not entries:
        return {}
    return {"rollout/ep_rew_mean": float(np.mean([round(float(r), 6) for r, _, _ in entries])),
            "rollout/ep_len_mean": float(np.mean([int(n) for _, n, _ in entries]))}


class EpisodeRing:
    """SB3's ``ep_info_buffer`` for a CTDE ``HerdBatch`` as device arrays (``ch_ep_ring``): ``ep_return`` float64 [W],
    ``ep_length`` / ``ep_env`` int32 [W], ``total`` int64 [1] (episodes appended since ``begin``; episode k lives in
    slot ``k % W``).  The four are views of one device buffer, so ``entries()`` is one copy."""

    def __init__(self, batch, window=100):
        if batch.mode != L.CH_MODE_CTDE:
            raise ValueError("the episode ring is for CTDE batches")
        self.batch, self.window = batch, int(window)
        if self.window < 1:
            raise ValueError("window must be >= 1")
        torch = batch.torch
        W = self.window
        self._buf = torch.zeros(16 * W + 8, dtype=torch.uint8, device=batch.device)
        self.ep_return = self._buf[:8 * W].view(torch.float64)
        self.ep_length = self._buf[8 * W:12 * W].view(torch.int32)
        self.ep_env = self._buf[12 * W:16 * W].view(torch.int32)
        self.total = self._buf[16 * W:].view(torch.int64)
        ring = L.ChEpRing()
        ring.window = W
        for k in ("ep_return", "ep_length", "ep_env", "total"):
            setattr(ring, k, getattr(self, k).data_ptr())
        self._ring = ring
        self._lib = L.lib()

    def begin(self):
        """Empty the ring (ch_ep_ring_begin: ``total = 0``), as a fresh ``ep_info_buffer``."""
        b = self.batch
        L.check(self._lib.ch_ep_ring_begin(b.handle, ctypes.byref(self._ring), b._stream()), b.handle)
        return self

    def record(self, io=None):
        """Append the episodes that ended in the step that just ran, in env order (ch_ep_ring_record on the batch's
        step outputs, or on another ``ChStepIO``)."""
        b = self.batch
        L.check(self._lib.ch_ep_ring_record(b.handle, ctypes.byref(self._ring),
                                            b._io_ref if io is None else ctypes.byref(io), b._stream()), b.handle)

    def entries(self):
        """The deque's content, oldest to newest: a list of ``(r, l, env)`` (float64 as the device holds it, int,
        int).  One small device-to-host copy (synchronises)."""
        W = self.window
        raw = self._buf.cpu().numpy()
        ret, length = raw[:8 * W].view(np.float64), raw[8 * W:12 * W].view(np.int32)
        env, total = raw[12 * W:16 * W].view(np.int32), int(raw[16 * W:].view(np.int64)[0])
        return [(ret[k % W], int(length[k % W]), int(env[k % W])) for k in range(max(0, total - W), total)]

    def count(self):
        """Episodes appended since ``begin`` (one 8-byte copy; synchronises)."""
        return int(self.total.item())

    def summary(self):
        """``rollout/ep_rew_mean`` and ``rollout/ep_len_mean`` of the ring's content (``summary_of``)."""
        return summary_of(self.entries())


def _pop_lib():
    lib = L.lib()
    if not hasattr(lib, "ch_ep_ring_pop_record"):
        raise ImportError("this libcattleherd.so has no ch_ep_ring_pop_record (an older library?)")
    return lib


class PopulationEpisodeRing:
    """One ``ep_info_buffer`` per member of a population that collects on one CTDE ``HerdBatch``
    (``PopulationRollout``; member ``p`` owns envs ``[pE, (p + 1)E)``) as device arrays (``ch_ep_ring_pop``):
    ``ep_return`` float64 [P, W], ``ep_length`` / ``ep_env`` int32 [P, W] (``ep_env``: the member-local env index),
    ``total`` int64 [P].  Row ``p`` is bit for bit the solo ``EpisodeRing`` of a batch of the member's envs.  The four
    are views of one device buffer, so ``entries_all()`` is one copy for the whole population; ``fitness()`` reduces
    the rings on the device."""

    def __init__(self, batch, n_members, window=100):
        if batch.mode != L.CH_MODE_CTDE:
            raise ValueError("the episode ring is for CTDE batches")
        self.batch, self.n_members, self.window = batch, int(n_members), int(window)
        if self.window < 1:
            raise ValueError("window must be >= 1")
        if self.n_members < 1 or batch.n_envs % self.n_members:
            raise ValueError(f"the batch's {batch.n_envs} envs do not divide evenly among {n_members} members")
        self.member_envs = batch.n_envs // self.n_members
        torch = batch.torch
        P, W = self.n_members, self.window
        # the 8-byte arrays first: every view is aligned
        self._cut = (8 * P * W, 8 * P * W + 8 * P, 12 * P * W + 8 * P, 16 * P * W + 8 * P)
        c = self._cut
        self._buf = torch.zeros(c[3], dtype=torch.uint8, device=batch.device)
        self.ep_return = self._buf[:c[0]].view(torch.float64).view(P, W)
        self.total = self._buf[c[0]:c[1]].view(torch.int64)
        self.ep_length = self._buf[c[1]:c[2]].view(torch.int32).view(P, W)
        self.ep_env = self._buf[c[2]:].view(torch.int32).view(P, W)
        ring = L.ChEpRingPop()
        ring.window, ring.n_members = W, P
        for k in ("ep_return", "ep_length", "ep_env", "total"):
            setattr(ring, k, getattr(self, k).data_ptr())
        self._ring = ring
        self._lib = _pop_lib()

    def begin(self):
        """Empty every member's ring (ch_ep_ring_pop_begin: ``total[p] = 0``)."""
        b = self.batch
        L.check(self._lib.ch_ep_ring_pop_begin(b.handle, ctypes.byref(self._ring), b._stream()), b.handle)
        return self

    def record(self, io=None):
        """Append the episodes that ended in the step that just ran to their members' rings, one launch for the
        population (ch_ep_ring_pop_record on the batch's step outputs, or on another ``ChStepIO``)."""
        b = self.batch
        L.check(self._lib.ch_ep_ring_pop_record(b.handle, ctypes.byref(self._ring),
                                                b._io_ref if io is None else ctypes.byref(io), b._stream()), b.handle)

    def _host(self):
        c, P, W = self._cut, self.n_members, self.window
        raw = self._buf.cpu().numpy()   # the one copy
        return (raw[:c[0]].view(np.float64).reshape(P, W), raw[c[1]:c[2]].view(np.int32).reshape(P, W),
                raw[c[2]:].view(np.int32).reshape(P, W), raw[c[0]:c[1]].view(np.int64))

    def entries_all(self):
        """Every member's deque content, oldest to newest: a list of P lists of ``(r, l, env)`` (``env`` member-local).
        One device-to-host copy for the whole population (synchronises)."""
        W = self.window
        ret, length, env, total = self._host()
        return [[(ret[p, k % W], int(length[p, k % W]), int(env[p, k % W]))
                 for k in range(max(0, int(total[p]) - W), int(total[p]))] for p in range(self.n_members)]

    def entries(self, p):
        """Member ``p``'s deque content (``entries_all()[p]``)."""
        return self.entries_all()[p]

    def count(self):
        """Episodes appended per member since ``begin``: a list of P ints (one small copy; synchronises)."""
        return [int(v) for v in self.total.cpu().numpy()]

    def summary(self, p):
        """Member ``p``'s ``rollout/ep_rew_mean`` and ``rollout/ep_len_mean`` (``summary_of(entries(p))``): what a solo
        ``EpisodeRing`` of the member's envs reports."""
        return summary_of(self.entries(p))

    def fitness(self, out=None):
        """The population's fitness table, reduced on the device (ch_ep_ring_pop_summary): a float64 device tensor
        ``[P, 4]`` of ``(count, mean return, mean length, total)`` per member on the batch's stream, no host
        synchronisation.  The means are NaN for an empty ring; the returns are not rounded to 6 decimals as
        ``summary`` rounds them."""
        b = self.batch
        torch = b.torch
        if out is None:
            out = torch.empty((self.n_members, L.CH_EP_RING_POP_SUMMARY), dtype=torch.float64, device=b.device)
        L.check(self._lib.ch_ep_ring_pop_summary(ctypes.byref(self._ring), out.data_ptr(), b._stream()))
        return out


def explained_variance_pop(values_list, returns_list, out=None):
    """``explained_variance`` for P members in one set of launches (ch_explained_variance_pop): returns a float64
    device tensor ``[P, 2]`` whose row ``p`` is bit for bit ``explained_variance(values_list[p], returns_list[p])``,
    on the current stream, no host synchronisation.  The tensors: contiguous float32 on one CUDA device, all of one
    size (separate allocations are fine: the kernels take tables of pointers)."""
    import torch
    values_list, returns_list = list(values_list), list(returns_list)
    P = len(values_list)
    if P < 1 or len(returns_list) != P:
        raise ValueError("explained_variance_pop: one values and one returns tensor per member, at least one member")
    dev, n = values_list[0].device, values_list[0].numel()
    for t in values_list + returns_list:
        if t.dtype != torch.float32 or not t.is_cuda or t.device != dev or not t.is_contiguous() or t.numel() != n or n < 1:
            raise ValueError("explained_variance_pop: contiguous float32 tensors of one size >= 1 on one CUDA device")
    lib = _pop_lib()
    if out is None:
        out = torch.empty((P, 2), dtype=torch.float64, device=dev)
    scratch = torch.empty(lib.ch_explained_variance_pop_scratch(n, P), dtype=torch.float64, device=dev)
    # the pointer tables: one upload, values then returns; the copy is queued on the current stream before the launches
    table = torch.tensor([t.data_ptr() for t in values_list + returns_list], dtype=torch.int64).to(dev, non_blocking=False)
    with torch.cuda.device(dev):
        L.check(lib.ch_explained_variance_pop(table[:P].data_ptr(), table[P:].data_ptr(), P, n, out.data_ptr(),
                                              scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    # the table and the scratch go back to the caching allocator of the stream the launches are queued on: a later
    # allocation on it reuses them only behind those launches
    return out


def explained_variance(values, returns, out=None):
    """SB3 ``explained_variance(y_pred=values, y_true=returns)`` on the device (ch_explained_variance), in float64:
    returns a float64 device tensor ``[1 - var(returns - values) / var(returns), var(returns)]`` (the first NaN when
    ``var(returns) == 0``), on the current stream, no host synchronisation.  ``values`` / ``returns``: float32 device
    tensors of the same number of elements (flattened as they lie)."""
    import torch
    if values.dtype != torch.float32 or returns.dtype != torch.float32 or not values.is_cuda or \
            values.device != returns.device or not values.is_contiguous() or not returns.is_contiguous() or \
            values.numel() != returns.numel() or values.numel() < 1:
        raise ValueError("explained_variance: two contiguous float32 tensors of the same size >= 1 on one CUDA device")
    lib, n, dev = L.lib(), values.numel(), values.device
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    scratch = torch.empty(lib.ch_explained_variance_scratch(n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.ch_explained_variance(values.data_ptr(), returns.data_ptr(), n, out.data_ptr(), scratch.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream))
    return out


def sb3_train_record(stats, steps_per_epoch, ent_coef, vf_coef, clip_range, explained_variance, std, n_updates=0,
                     learning_rate=None, clip_range_vf=None):
    """SB3 ``PPO.train``'s logger record from a call's per-minibatch statistics -- a pure host function.  ``stats``:
    ``[steps, 6]`` (``ch_ppo_train_log``'s columns: policy loss, value loss, mean entropy, gradient norm, approx_kl,
    clip_fraction) or ``[steps, 7]`` (``ch_ppo_train_opt``'s: then ``state``, 1 applied / 0 tripped the KL gate / -1
    not run), epoch after epoch with ``steps_per_epoch`` rows each.  SB3 appends a minibatch's statistics before the
    gate, so each key's ``np.mean`` runs over the rows with ``state >= 0``, the tripping one included, and
    ``train/loss`` is the last such row's ``policy + ent_coef * entropy_loss + vf_coef * value`` (the value loss as the
    row holds it: clipped with ``clip_range_vf``).  ``train/n_updates`` is ``n_updates`` plus the epochs that ran at
    least one minibatch, the one that broke included.  ``train/learning_rate`` follows when ``learning_rate`` is given
    and ``train/clip_range_vf`` when set.  Returns ``(record, epochs_run)``."""
    st = np.asarray(stats, np.float64)
    state = st[:, 6] if st.shape[1] > 6 else np.ones(len(st))
    ran = state >= 0
    if not ran.any():
        raise ValueError("sb3_train_record: no minibatch ran (was the stop word zeroed before the call?)")
    epochs_run = len({k // int(steps_per_epoch) for k in np.flatnonzero(ran)})
    r = st[ran]
    pl, vl, ent, akl, cf = r[:, 0], r[:, 1], r[:, 2], r[:, 4], r[:, 5]
    # SB3: each list holds the minibatches' float32 .item()s; the logger records np.mean of each (float64)
    rec = {
        "train/entropy_loss": float(np.mean(-ent)),
        "train/policy_gradient_loss": float(np.mean(pl)),
        "train/value_loss": float(np.mean(vl)),
        "train/approx_kl": float(np.mean(akl)),
        "train/clip_fraction": float(np.mean(cf)),
        "train/loss": float(pl[-1] + ent_coef * -ent[-1] + vf_coef * vl[-1]),   # the last minibatch's
        "train/explained_variance": float(explained_variance),
        "train/std": float(std),
        "train/n_updates": int(n_updates) + epochs_run,
        "train/clip_range": float(clip_range),
    }
    if learning_rate is not None:
        rec["train/learning_rate"] = float(learning_rate)
    if clip_range_vf is not None:
        rec["train/clip_range_vf"] = float(clip_range_vf)
    return rec, epochs_run


# ---- the DTDE (MARL) driver: RLlib's result dict ----------------------------------------------------------------
POLICY_ID = "shared_policy"   # DTDECattleHerder.py: policies = {"shared_policy"}, every agent mapped to it


def marl_summary_of(entries, num_episodes, env_steps, agent_steps):
    """RLlib's env-runner keys of a window of episodes.  ``entries``: ``(return, length, agent_returns [N],
    agent_lengths [N], env)`` per episode, oldest first; ``num_episodes``: the episodes since the previous report;
    ``env_steps`` / ``agent_steps [N]``: the sampling counters.  ``episode_return_mean`` / ``_min`` / ``_max`` and
    ``episode_len_mean`` / ``_min`` / ``_max`` over the window; ``agent_episode_returns_mean/agent_i``: the mean of
    agent i's return over the window's episodes it took part in (``agent_length > 0``; an agent of no episode has no
    key: ``marl_eval.episode_metrics``' rule and ids); ``module_episode_returns_mean/shared_policy``: every agent acts
    through the one module, so its return of an episode is the episode's.  An empty window has no episode keys."""
    out = {}
    if entries:
        ret = np.array([e[0] for e in entries], np.float64)
        length = np.array([e[1] for e in entries], np.int64)
        a_ret = np.array([e[2] for e in entries], np.float64).reshape(len(entries), -1)
        a_len = np.array([e[3] for e in entries], np.int64).reshape(len(entries), -1)
        out.update({"episode_return_mean": float(ret.mean()), "episode_return_min": float(ret.min()),
                    "episode_return_max": float(ret.max()), "episode_len_mean": float(length.mean()),
                    "episode_len_min": int(length.min()), "episode_len_max": int(length.max())})
        for i in range(a_ret.shape[1]):
            took_part = a_len[:, i] > 0
            if took_part.any():
                out[f"agent_episode_returns_mean/agent_{i}"] = float(a_ret[took_part, i].mean())
        out[f"module_episode_returns_mean/{POLICY_ID}"] = float(ret.mean())
    out["num_episodes"] = int(num_episodes)
    out["num_env_steps_sampled"] = int(env_steps)
    for i, n in enumerate(agent_steps):
        out[f"num_agent_steps_sampled/agent_{i}"] = int(n)
    return out


class MarlEpisodeRing:
    """The env runners' episode window of a MARL ``HerdBatch`` as device arrays (``ch_marl_ep_ring``; N =
    ``batch.num_drones``): ``ep_return`` float64 [W], ``agent_return`` float64 [W, N], ``ep_length`` / ``ep_env``
    int32 [W], ``agent_length`` int32 [W, N], ``total`` int64 [1] (episodes appended since ``begin``; episode k lives
    in slot ``k % W``), the counters ``env_steps`` int64 [1] and ``agent_steps`` int64 [N], and the open episodes'
    running state ``acc_return`` float64 [E, N], ``acc_length`` int32 [E, N], ``acc_steps`` int32 [E].  All are views
    of one device buffer, the window and the counters at its head, so ``entries()`` and ``summary()`` are one copy."""

    HEAD = ("ep_return", "agent_return", "total", "env_steps", "agent_steps", "ep_length", "agent_length", "ep_env")
    ARRAYS = HEAD + ("acc_return", "acc_length", "acc_steps")

    def __init__(self, batch, window=100):
        if batch.mode != L.CH_MODE_MARL:
            raise ValueError("the per-agent episode ring is for MARL batches")
        self.batch, self.window = batch, int(window)
        if self.window < 1:
            raise ValueError("window must be >= 1")
        torch = batch.torch
        W, E, N = self.window, batch.n_envs, batch.num_drones
        f64, i64, i32 = (torch.float64, np.float64, 8), (torch.int64, np.int64, 8), (torch.int32, np.int32, 4)
        shapes = {"ep_return": (f64, (W,)), "agent_return": (f64, (W, N)), "total": (i64, (1,)),
                  "env_steps": (i64, (1,)), "agent_steps": (i64, (N,)), "ep_length": (i32, (W,)),
                  "agent_length": (i32, (W, N)), "ep_env": (i32, (W,)), "acc_return": (f64, (E, N)),
                  "acc_length": (i32, (E, N)), "acc_steps": (i32, (E,))}
        # the 8-byte arrays of each part come first, and the head is padded to 8 bytes: every view is aligned
        at, off = {}, 0   # name -> (byte offset, bytes, torch dtype, numpy dtype, shape): the one table every view uses
        for k in self.ARRAYS:
            if k == "acc_return":
                off = self._head = (off + 7) // 8 * 8
            (dt, np_dt, size), shape = shapes[k]
            at[k] = (off, int(np.prod(shape)) * size, dt, np_dt, shape)
            off += at[k][1]
        self._buf = torch.zeros(off, dtype=torch.uint8, device=batch.device)
        self._at = at
        ring = L.ChMarlEpRing()
        ring.window = W
        for k, (o, n, dt, _, shape) in at.items():
            setattr(self, k, self._buf[o:o + n].view(dt).view(shape))
            setattr(ring, k, getattr(self, k).data_ptr())
        self._ring = ring
        self._reported = 0   # `total` at the previous summary()

    def begin(self):
        """Empty the ring (ch_marl_ep_ring_begin): ``total``, the counters and the open episodes' sums to zero -- an
        episode that is open now counts from zero."""
        b = self.batch
        L.check(L.lib().ch_marl_ep_ring_begin(b.handle, ctypes.byref(self._ring), b._stream()), b.handle)
        self._reported = 0
        return self

    def record(self, live, io=None):
        """After a step: the rewards of the agents that were live at its start (``live``: uint8 [E, N] device tensor)
        into the open episodes' sums, and the episodes that ended in it into the ring, in env order
        (ch_marl_ep_ring_record on the batch's step outputs, or on another ``ChStepIO``)."""
        b = self.batch
        torch = b.torch
        if live.dtype != torch.uint8 or not live.is_contiguous() or live.numel() != b.n_envs * b.num_drones or \
                live.device != self._buf.device:
            raise ValueError("live must be a contiguous uint8 [n_envs, num_drones] tensor on the batch's device")
        L.check(L.lib().ch_marl_ep_ring_record(b.handle, ctypes.byref(self._ring), live.data_ptr(),
                                               b._io_ref if io is None else ctypes.byref(io), b._stream()), b.handle)

    def _views(self, raw):
        out = {}
        for k, (o, n, _, np_dt, shape) in self._at.items():
            if o + n > len(raw):   # (a copy of the head alone)
                break
            out[k] = raw[o:o + n].view(np_dt).reshape(shape)
        return out

    def arrays(self):
        """Every array as numpy (one copy of the whole buffer; synchronises)."""
        return self._views(self._buf.cpu().numpy())

    def _head_arrays(self):
        return self._views(self._buf[:self._head].cpu().numpy())   # the one copy

    @staticmethod
    def _entries(a, W):
        total = int(a["total"][0])
        return [(a["ep_return"][k % W], int(a["ep_length"][k % W]), a["agent_return"][k % W].copy(),
                 a["agent_length"][k % W].astype(np.int64), int(a["ep_env"][k % W]))
                for k in range(max(0, total - W), total)]

    def entries(self):
        """The window's content, oldest to newest: a list of ``(return, length, agent_returns [N], agent_lengths [N],
        env)``.  One small device-to-host copy (synchronises)."""
        return self._entries(self._head_arrays(), self.window)

    def count(self):
        """Episodes appended since ``begin`` (one 8-byte copy; synchronises)."""
        return int(self.total.item())

    def summary(self):
        """RLlib's env-runner keys (``marl_summary_of``) from one copy of the window and the counters;
        ``num_episodes`` counts the episodes appended since the previous ``summary()`` (or ``begin``)."""
        a = self._head_arrays()
        total = int(a["total"][0])
        out = marl_summary_of(self._entries(a, self.window), total - self._reported, int(a["env_steps"][0]),
                              a["agent_steps"].tolist())
        self._reported = total
        return out


def rllib_result(ring, update):
    """One training iteration's record as RLlib's result dict nests it: ``{"env_runners": ring.summary(), "learners":
    {"shared_policy": update.last_log}}`` (a ``MarlEpisodeRing`` and a ``MarlPPOUpdate(log_stats=True)`` after
    ``train``)."""
    if not update.last_log:
        raise ValueError("rllib_result: the update holds no record (MarlPPOUpdate(log_stats=True), after train())")
    return {"env_runners": ring.summary(), "learners": {POLICY_ID: dict(update.last_log)}}
