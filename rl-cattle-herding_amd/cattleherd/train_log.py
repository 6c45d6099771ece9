"""The SB3 logger record of a native training run, from device-side data.

The reference is trained by watching SB3's logger: ``rollout/ep_rew_mean`` and ``rollout/ep_len_mean`` are the means
over ``ep_info_buffer``, a ``deque(maxlen=stats_window_size)`` that ``OnPolicyAlgorithm._update_info_buffer`` fills
with Monitor's ``info["episode"]`` step by step, in env order, inside ``collect_rollouts``; the ``train/`` keys come
from ``PPO.train``.  ``EpisodeRing`` is that deque as a ring in device memory, appended to by one small kernel per step
(``ch_ep_ring_record``; inside the native collection with ``DeviceRolloutBuffer.collect(..., ring=ring)``), read with
one small copy when the record is wanted.  The ``train/`` half is ``PPOUpdate(..., log_stats=True)`` (cattleherd/ppo.py),
over ``ch_ppo_train_log`` and ``explained_variance`` below.

Semantics restated from SB3 2.x; SB3 is not installed here, so the restatement is "parity unpinned" to its source.
One difference is deliberate: SB3's ``explained_variance`` is float32 numpy, here the float32 inputs are widened
exactly and every sum is float64 (two passes: the means, then the squared deviations).  CTDE batches only.
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
