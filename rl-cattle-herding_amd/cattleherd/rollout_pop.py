"""A population's rollout collection on one env batch: ``PopulationRollout(batch, P, T).collect(...)`` fills P members'
rollout buffers in one native call (``ch_rollout_collect_pop``, include/cattleherd.h) instead of one
``DeviceRolloutBuffer.collect`` per member on P batches.

The batch holds ``P * E`` envs and member ``p`` owns envs ``[pE, (p + 1)E)``: a member's env seeds are those of global
envs ``env_id_offset + pE .. env_id_offset + (p + 1)E - 1``, so its buffers are bit for bit what
``DeviceRolloutBuffer(HerdBatch(E, ..., env_id_offset=env_id_offset + pE)).collect`` gives from the same state with the
member's nets, ``log_std``, seed, ``gamma`` and ``gae_lambda``.  The env step is one launch for the whole batch; each
policy launch carries every member.  ``PPOPopulation.train(pop.members)`` takes the buffers as they are.
"""
import ctypes

from . import _lib as L
from .rollout import ChRollout, ChRolloutIO

BUFFER_ARRAYS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns",
                 "last_episode_starts")


class ChRolloutMember(ctypes.Structure):
    """One member of ch_rollout_collect_pop's population (include/cattleherd.h ch_rollout_member)."""
    _fields_ = [("rb", ChRollout), ("actor", ctypes.POINTER(L.ChMlp)), ("critic", ctypes.POINTER(L.ChMlp)),
                ("log_std", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("gamma", ctypes.c_float),
                ("gae_lambda", ctypes.c_float)]


def member_slices(n_envs, n_members, p, obs_rows, num_drones, act_dim):
    """Where member ``p``'s rows start in each handle-wide scratch array (elements), and its env count: the
    arithmetic ``ch_rollout_collect_pop`` uses.  The queue entry is in rows; a member's share of the deferred-bootstrap
    queue is the whole queue of a solo batch of its size (its flush period times its envs)."""
    if n_members < 1 or n_envs < 1 or n_envs % n_members or not 0 <= p < n_members:
        raise ValueError("n_envs must be a positive multiple of n_members and 0 <= p < n_members")
    E = n_envs // n_members
    obs_dim = obs_rows * 86
    every = min(16, max(1, (1 << 30) // (E * obs_dim * 4)))
    e0 = p * E
    return {"n_envs": E, "obs": e0 * obs_dim, "mean": e0 * act_dim, "row": e0, "env_actions": e0 * num_drones * 4,
            "flags": e0, "queue": e0 * every}


def _bind():
    lib = L.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    if not hasattr(lib, "ch_rollout_collect_pop"):
        raise ImportError("this libcattleherd.so has no ch_rollout_collect_pop (an older library?)")
    lib.ch_rollout_pop_create.argtypes = [i32, i32, ctypes.POINTER(vp)]
    lib.ch_rollout_pop_destroy.argtypes = [vp]
    lib.ch_rollout_collect_pop.argtypes = [vp, vp, ctypes.POINTER(ChRolloutMember), i32, ctypes.POINTER(ChRolloutIO), i32, vp]
    if hasattr(lib, "ch_rollout_collect_pop_log"):   # (an older library, e.g. an A/B baseline, lacks it)
        lib.ch_rollout_collect_pop_log.argtypes = [vp, vp, ctypes.POINTER(ChRolloutMember), i32, ctypes.POINTER(ChRolloutIO),
                                                   i32, ctypes.POINTER(L.ChEpRingPop), vp]
        lib.ch_rollout_collect_pop_log.restype = ctypes.c_int
    lib.ch__rollout_pop_slice.argtypes = [ctypes.c_int64, i32, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_int64 * 7)]
    for f in (lib.ch_rollout_pop_create, lib.ch_rollout_pop_destroy, lib.ch_rollout_collect_pop, lib.ch__rollout_pop_slice):
        f.restype = ctypes.c_int
    return lib


def lib_member_slices(n_envs, n_members, p, obs_rows, num_drones, act_dim):
    """Internal (tests): ``member_slices`` as the library computes it (ch__rollout_pop_slice; host only)."""
    out = (ctypes.c_int64 * 7)()
    L.check(_bind().ch__rollout_pop_slice(n_envs, n_members, p, obs_rows, num_drones, act_dim, ctypes.byref(out)))
    return dict(zip(("n_envs", "obs", "mean", "row", "env_actions", "flags", "queue"), (int(v) for v in out)))


class MemberBuffer:
    """One member's rollout buffer: the attributes of ``DeviceRolloutBuffer`` that a PPO update reads, each
    ``[T, E, ...]`` and contiguous, in allocations of the member's own."""

    def __init__(self, torch, device, T, E, obs_dim, act_dim, gamma, gae_lambda):
        self.T, self.gamma, self.gae_lambda, self.act_dim = int(T), float(gamma), float(gae_lambda), int(act_dim)
        z = dict(dtype=torch.float32, device=device)
        self.obs = torch.zeros((T, E, obs_dim), **z)
        self.actions = torch.zeros((T, E, act_dim), **z)
        for k in ("rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            setattr(self, k, torch.zeros((T, E), **z))
        self.last_episode_starts = torch.ones(E, **z)          # SB3: _last_episode_starts = ones after reset

    def struct(self):
        rb = ChRollout()
        rb.n_steps, rb.act_dim = self.T, self.act_dim
        for k in BUFFER_ARRAYS:
            setattr(rb, k, getattr(self, k).data_ptr())
        return rb


def _per_member(v, n, name):
    if isinstance(v, (int, float)):
        return [float(v)] * n
    v = [float(x) for x in v]
    if len(v) != n:
        raise ValueError(f"{name} must be a float or one value per member ({n})")
    return v


class PopulationRollout:
    """``batch``: a CTDE ``HerdBatch`` whose ``n_envs`` is a multiple of ``n_members``; member ``p`` collects on envs
    ``[pE, (p + 1)E)`` (its env seeds are those of global envs ``env_id_offset + pE ...``).  ``gammas`` /
    ``gae_lambdas``: a float, or one value per member.  ``.members``: the P ``MemberBuffer`` objects; the object owns
    the batch-wide scratch and the kernels' argument tables.  Use it from one stream at a time."""

    def __init__(self, batch, n_members, n_steps, act_dim=None, gammas=0.99, gae_lambdas=0.95):
        if batch.mode != L.CH_MODE_CTDE:
            raise ValueError("the SB3 rollout buffer is for CTDE batches")
        P = int(n_members)
        if P < 1 or P > 65535:
            raise ValueError("n_members must be 1..65535")
        if batch.n_envs % P:
            raise ValueError(f"the batch's {batch.n_envs} envs do not divide evenly among {P} members")
        if int(n_steps) < 1:
            raise ValueError("n_steps must be >= 1")
        gammas, lams = _per_member(gammas, P, "gammas"), _per_member(gae_lambdas, P, "gae_lambdas")
        torch = batch.torch
        self.batch, self.n_members, self.T = batch, P, int(n_steps)
        self.member_envs = E = batch.n_envs // P
        self.act_dim = int(act_dim or batch.num_drones * 4)
        od = batch.obs_rows * 86
        self.members = [MemberBuffer(torch, batch.device, self.T, E, od, self.act_dim, g, l) for g, l in zip(gammas, lams)]
        z = dict(dtype=torch.float32, device=batch.device)
        n = batch.n_envs
        self.env_actions = torch.zeros((n, batch.num_drones, 4), **z)
        self.mean = torch.zeros((n, self.act_dim), **z)
        self.value = torch.zeros((n, 1), **z)
        self.terminal_value = torch.zeros((n, 1), **z)
        self._lib, self._pop = None, ctypes.c_void_p()   # the tables: made by the first collect

    def collect(self, actors, critics, log_stds, seeds, bootstrap_truncated=True, ring=None):
        """SB3 collect_rollouts for ``n_steps`` steps of every member on its envs, in one native call on the batch's
        stream.  ``actors`` / ``critics``: one ``DevicePolicy`` per member (one architecture; packed here if they are
        not), ``log_stds``: one float32 ``[act_dim]`` tensor per member, ``seeds``: one sampling seed per member.
        ``ring``: a ``train_log.PopulationEpisodeRing`` of this batch with one ring per member; every step's ended
        episodes are appended to their members' rings (ch_rollout_collect_pop_log: one small launch more per step
        whatever P is; the buffers and the env state do not depend on it).  The ring is not begun here."""
        b, P = self.batch, self.n_members
        actors, critics, log_stds, seeds = list(actors), list(critics), list(log_stds), list(seeds)
        for name, v in (("actors", actors), ("critics", critics), ("log_stds", log_stds), ("seeds", seeds)):
            if len(v) != P:
                raise ValueError(f"collect takes one of {name} per member ({P}), got {len(v)}")
        if any(c is None for c in critics) or any(a is None for a in actors):
            raise ValueError("every member needs an actor and a critic (a fused actor-critic is not supported here)")
        if ring is not None:
            if ring.batch is not b:
                raise ValueError("the episode ring belongs to another batch")
            if ring.n_members != P:
                raise ValueError(f"the episode ring holds {ring.n_members} members, the population {P}")
        if not self._pop:
            self._lib = _bind()
            L.check(self._lib.ch_rollout_pop_create(P, b.device.index or 0, ctypes.byref(self._pop)))
        torch = b.torch
        log_stds = [ls.to(device=b.device, dtype=torch.float32).contiguous() for ls in log_stds]
        members = (ChRolloutMember * P)()
        for mb, rb, actor, critic, ls, seed in zip(members, self.members, actors, critics, log_stds, seeds):
            actor._ensure_packed()
            critic._ensure_packed()
            mb.rb = rb.struct()
            mb.actor, mb.critic = ctypes.pointer(actor._net), ctypes.pointer(critic._net)
            mb.log_std, mb.seed, mb.gamma, mb.gae_lambda = ls.data_ptr(), int(seed), rb.gamma, rb.gae_lambda
        io = ChRolloutIO()
        io.step = ctypes.pointer(b._io)
        io.mean, io.value = self.mean.data_ptr(), self.value.data_ptr()
        io.terminal_value, io.env_actions = self.terminal_value.data_ptr(), self.env_actions.data_ptr()
        keep = b._io.terminal_obs, b._io.reset_happened, b._io.episode_stats
        b._io.terminal_obs = b.terminal_obs.data_ptr()
        b._io.reset_happened, b._io.episode_stats = b.reset_happened.data_ptr(), b.episode_stats.data_ptr()
        try:
            if ring is None:
                L.check(self._lib.ch_rollout_collect_pop(b.handle, self._pop, members, P, ctypes.byref(io),
                                                         int(bool(bootstrap_truncated)), b._stream()), b.handle)
            else:
                if not hasattr(self._lib, "ch_rollout_collect_pop_log"):
                    raise ImportError("this libcattleherd.so has no ch_rollout_collect_pop_log (an older library?)")
                L.check(self._lib.ch_rollout_collect_pop_log(b.handle, self._pop, members, P, ctypes.byref(io),
                                                             int(bool(bootstrap_truncated)), ctypes.byref(ring._ring),
                                                             b._stream()), b.handle)
        finally:
            b._io.terminal_obs, b._io.reset_happened, b._io.episode_stats = keep
        self._keep = (log_stds, actors, critics)   # alive until the queued launches have read them
        return self

    def close(self):
        """Frees the argument tables (after the device's work: the launches read them)."""
        if getattr(self, "_pop", None):
            self.batch.torch.cuda.synchronize(self.batch.device)
            self._lib.ch_rollout_pop_destroy(self._pop)
            self._pop = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter shutdown)
            pass
