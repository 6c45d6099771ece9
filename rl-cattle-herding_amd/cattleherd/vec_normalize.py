"""SB3's ``VecNormalize`` for the on-device CTDE PPO path: running observation and return statistics in device memory.

The reference's observations are metres and metres per second and its rewards unscaled sums, the case SB3 users wrap in
``VecNormalize``.  ``DeviceVecNormalize`` keeps its two ``RunningMeanStd`` (``obs_rms`` over the ``obs_rows * 86``
features, ``ret_rms`` over the envs' discounted returns) and the returns themselves in one float64 device block,
updated and applied by HIP kernels on the stream (``ch_norm_*``, csrc/ch_norm.hip) with no host read, so the normalised
observation exists on the device before the actor reads it: ``DeviceRolloutBuffer.collect(..., normalizer=n)``.

Semantics restated from SB3 2.x ``RunningMeanStd`` / ``VecNormalize`` (``reset``, ``step_wait``, ``normalize_obs``,
``normalize_reward``); SB3 is not installed here, so the restatement is "parity unpinned" to its source.  Not restated:
``norm_obs_keys`` / dict observations, SB3's pickled file (``save`` / ``load`` here are ``.npz``), MARL batches.

One thing differs for the policy: a normalised observation is dense.  The raw CTDE observation is zero past an env's
``NUM_DRONES`` rows and ``DevicePolicy.forward_batch`` does not multiply those features; normalised they are
``(0 - mean) / std``, so the normalised paths use the dense ``DevicePolicy.forward``.
"""
import ctypes

import numpy as np

from . import _lib as L

HYPER = ("training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon")


def _check_hyper(clip_obs, clip_reward, gamma, epsilon):
    if not clip_obs >= 0 or not clip_reward >= 0:
        raise ValueError("clip_obs and clip_reward must be >= 0")
    if not epsilon >= 0:
        raise ValueError("epsilon must be >= 0")
    if not 0 <= gamma <= 1:
        raise ValueError("gamma must be in [0, 1]")


def check_state_dict(state, dim, n_envs):
    """Validate a ``state_dict`` against a normaliser of ``dim`` features and ``n_envs`` envs (host only); returns the
    float64 arrays ``(obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count, ret)``."""
    missing = [k for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "ret") + HYPER
               if k not in state]
    if missing:
        raise ValueError(f"state_dict lacks {missing}")
    mean, var = np.asarray(state["obs_mean"], np.float64), np.asarray(state["obs_var"], np.float64)
    ret = np.asarray(state["ret"], np.float64)
    if mean.shape != (dim,) or var.shape != (dim,):
        raise ValueError(f"obs_mean / obs_var must have shape ({dim},), got {mean.shape} / {var.shape}")
    if ret.shape != (n_envs,):
        raise ValueError(f"ret must have shape ({n_envs},), got {ret.shape}: the state is of another batch size")
    _check_hyper(float(state["clip_obs"]), float(state["clip_reward"]), float(state["gamma"]), float(state["epsilon"]))
    return (mean, var, float(state["obs_count"]), float(state["ret_mean"]), float(state["ret_var"]),
            float(state["ret_count"]), ret)


class DeviceNormalizer:
    """The statistics block and the kernels without a batch: ``dim`` features, ``n_envs`` returns, on ``device``; any
    contiguous float32 ``[rows, dim]`` device matrix of up to ``max_rows`` rows (default ``n_envs``) can be passed to
    ``update_obs`` / ``normalize_obs``.  One float64 device block ``[mean (dim) | var (dim) | count | ret_mean ret_var
    ret_count | ret (E)]`` holds every statistic (a checkpoint is one copy each way); ``obs_n`` [E, dim],
    ``terminal_obs_n`` [E, dim] and ``reward_n`` [E] are the normalised step outputs the collection works in."""

    def __init__(self, device, dim, n_envs, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0,
                 clip_reward=10.0, gamma=0.99, epsilon=1e-8, max_rows=None):
        import torch
        _check_hyper(clip_obs, clip_reward, gamma, epsilon)
        self.torch, self.device = torch, torch.device(device)
        self.dim, self.n_envs = int(dim), int(n_envs)
        D, E = self.dim, self.n_envs
        if D < 1 or E < 1:
            raise ValueError("dim and n_envs must be >= 1")
        self._lib = L.lib()
        # (the chunk count is not monotonic in the rows past 16384: sized for both ends)
        n_scratch = max(self._lib.ch_norm_scratch_size(r, D) for r in {E, int(max_rows or E), min(int(max_rows or E), 16384)})
        if n_scratch < 0:
            raise ValueError("dim and rows must be at most 2^24")
        self._block = torch.zeros(2 * D + 4 + E, dtype=torch.float64, device=self.device)
        self.mean, self.var = self._block[:D], self._block[D:2 * D]
        self.count, self.ret_stats, self.ret = self._block[2 * D:2 * D + 1], self._block[2 * D + 1:2 * D + 4], self._block[2 * D + 4:]
        self._scratch = torch.zeros(n_scratch, dtype=torch.float64, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs_n = torch.zeros((E, D), **f32)
        self.terminal_obs_n = torch.zeros((E, D), **f32)
        self.reward_n = torch.zeros(E, **f32)
        n = L.ChNorm()
        n.dim, n.n_envs = D, E
        n.clip_obs, n.clip_reward, n.epsilon, n.gamma = float(clip_obs), float(clip_reward), float(epsilon), float(gamma)
        for k in ("mean", "var", "count", "ret_stats", "ret", "obs_n", "terminal_obs_n", "reward_n"):
            setattr(n, k, getattr(self, k).data_ptr())
        n.scratch, n.scratch_doubles = self._scratch.data_ptr(), n_scratch
        self._n = n
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        with torch.cuda.device(self.device):
            L.check(self._lib.ch_norm_begin(ctypes.byref(n), self._stream()))

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the switches (SB3: evaluate with training = False, norm_reward = False) ---------------------------------
    training = property(lambda self: bool(self._n.training), lambda self, v: setattr(self._n, "training", int(bool(v))))
    norm_obs = property(lambda self: bool(self._n.norm_obs), lambda self, v: setattr(self._n, "norm_obs", int(bool(v))))
    norm_reward = property(lambda self: bool(self._n.norm_reward),
                           lambda self, v: setattr(self._n, "norm_reward", int(bool(v))))
    clip_obs = property(lambda self: self._n.clip_obs)
    clip_reward = property(lambda self: self._n.clip_reward)
    gamma = property(lambda self: self._n.gamma)
    epsilon = property(lambda self: self._n.epsilon)

    # ---- kernels --------------------------------------------------------------------------------------------------
    def _matrix(self, x):
        torch = self.torch
        if x.dtype != torch.float32 or x.device != self._block.device or not x.is_contiguous() or \
                x.numel() == 0 or x.numel() % self.dim:
            raise ValueError(f"a contiguous float32 tensor of rows x {self.dim} on {self._block.device} is required")
        return x.numel() // self.dim

    def update_obs(self, obs):
        """``obs_rms.update(obs)`` on the stream (ch_norm_obs_update); a no-op unless training and norm_obs."""
        rows = self._matrix(obs)
        L.check(self._lib.ch_norm_obs_update(ctypes.byref(self._n), obs.data_ptr(), rows, self._stream()))

    def normalize_obs(self, obs, out=None, row_mask=None):
        """``normalize_obs(obs)`` with the statistics as they stand (ch_norm_obs_apply) into ``out`` (default: a new
        tensor; ``out=obs`` runs in place).  ``row_mask`` (uint8 [rows]): only the selected rows of ``out`` are written."""
        torch = self.torch
        rows = self._matrix(obs)
        if out is None:
            out = torch.empty_like(obs)
        elif out.dtype != torch.float32 or out.device != obs.device or not out.is_contiguous() or out.numel() != obs.numel():
            raise ValueError("out must be a contiguous float32 tensor of obs's size on its device")
        m = None
        if row_mask is not None:
            if row_mask.dtype != torch.uint8 or row_mask.device != obs.device or not row_mask.is_contiguous() or \
                    row_mask.numel() != rows:
                raise ValueError(f"row_mask must be a contiguous uint8 [{rows}] tensor on the observation's device")
            m = row_mask.data_ptr()
        L.check(self._lib.ch_norm_obs_apply(ctypes.byref(self._n), obs.data_ptr(), rows, m, out.data_ptr(),
                                            self._stream()))
        return out

    def reset_obs(self, obs):
        """``VecNormalize.reset`` after the env's own reset: ``ret = 0``, the statistics updated with ``obs`` (when
        training and norm_obs), and its normalisation in ``self.obs_n``."""
        self.ret.zero_()
        self.update_obs(obs)
        return self.normalize_obs(obs, out=self.obs_n)

    def step_reward(self, reward, terminated, truncated, out=None):
        """The reward half of ``step_wait`` for the step that just ran (ch_norm_reward): returns and ``ret_rms``
        updated (when training), the normalised reward in ``out`` (default ``self.reward_n``), ``ret = 0`` where done.
        ``reward`` float32 / ``terminated`` / ``truncated`` uint8 device tensors of n_envs entries; ``reward`` is only read."""
        torch = self.torch
        out = self.reward_n if out is None else out
        for t, dt in ((reward, torch.float32), (out, torch.float32), (terminated, torch.uint8), (truncated, torch.uint8)):
            if t.dtype != dt or t.device != self._block.device or not t.is_contiguous() or t.numel() != self.n_envs:
                raise ValueError(f"reward / out (float32) and terminated / truncated (uint8) must be contiguous "
                                 f"[{self.n_envs}] tensors on {self._block.device}")
        L.check(self._lib.ch_norm_reward(ctypes.byref(self._n), reward.data_ptr(), terminated.data_ptr(),
                                         truncated.data_ptr(), self.n_envs, out.data_ptr(), self._stream()))
        return out

    # ---- statistics and checkpoints -------------------------------------------------------------------------------
    def _host(self):
        return self._block.cpu().numpy()   # the one copy (synchronises)

    @property
    def obs_rms(self):
        """``(mean [dim], var [dim], count)`` as numpy float64 (one copy of the block; synchronises)."""
        h, D = self._host(), self.dim
        return h[:D].copy(), h[D:2 * D].copy(), float(h[2 * D])

    @property
    def ret_rms(self):
        """``(mean, var, count)`` of the returns as floats (one copy of the block; synchronises)."""
        h, D = self._host(), self.dim
        return float(h[2 * D + 1]), float(h[2 * D + 2]), float(h[2 * D + 3])

    def state_dict(self):
        """The statistics as numpy float64 and the hyper-parameters."""
        h, D = self._host(), self.dim
        out = {"obs_mean": h[:D].copy(), "obs_var": h[D:2 * D].copy(), "obs_count": float(h[2 * D]),
               "ret_mean": float(h[2 * D + 1]), "ret_var": float(h[2 * D + 2]), "ret_count": float(h[2 * D + 3]),
               "ret": h[2 * D + 4:].copy()}
        out.update({k: getattr(self, k) for k in HYPER})
        return out

    def load_state_dict(self, state):
        mean, var, count, rm, rv, rc, ret = check_state_dict(state, self.dim, self.n_envs)
        torch = self.torch
        h = np.concatenate([mean, var, [count, rm, rv, rc], ret])
        self._block.copy_(torch.from_numpy(h))
        n = self._n
        n.clip_obs, n.clip_reward = float(state["clip_obs"]), float(state["clip_reward"])
        n.gamma, n.epsilon = float(state["gamma"]), float(state["epsilon"])
        self.training, self.norm_obs, self.norm_reward = state["training"], state["norm_obs"], state["norm_reward"]
        return self

    def save(self, path):
        np.savez(path, **self.state_dict())

    @staticmethod
    def read(path):
        """The ``state_dict`` a ``save(path)`` wrote (host only)."""
        with np.load(path) as z:
            return {k: (z[k] if z[k].ndim else z[k].item()) for k in z.files}


class DeviceVecNormalize(DeviceNormalizer):
    """``VecNormalize(venv, training, norm_obs, norm_reward, clip_obs, clip_reward, gamma, epsilon)`` for a CTDE
    ``HerdBatch``: a ``DeviceNormalizer`` of the batch's ``obs_rows * 86`` features and ``n_envs`` returns on its
    device, which ``DeviceRolloutBuffer.collect`` / ``collect_steps`` and ``evaluate_policy_steps`` take."""

    def __init__(self, batch, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0,
                 gamma=0.99, epsilon=1e-8):
        if batch.mode != L.CH_MODE_CTDE:
            raise ValueError("DeviceVecNormalize is for CTDE batches (RLlib normalises with connectors)")
        self.batch = batch
        super().__init__(batch.device, batch.obs_rows * 86, batch.n_envs, training, norm_obs, norm_reward, clip_obs,
                         clip_reward, gamma, epsilon)

    def reset_obs(self, obs=None):
        """``VecNormalize.reset`` after ``batch.reset()`` (``obs``: default the batch's observations)."""
        return super().reset_obs(self.batch.obs.view(self.n_envs, self.dim) if obs is None else obs)

    @classmethod
    def load(cls, path, batch):
        """A normaliser of ``batch`` with the statistics and hyper-parameters ``save(path)`` wrote."""
        return cls(batch).load_state_dict(cls.read(path))
