"""Shared pieces of the SB3 training log's tests (test_train_log_cpu.py, test_gpu_train_log.py): SB3's ``ep_info_buffer``
as a host deque fed per step in env order, a numpy restatement of the device ring's slot rule, and the float64
formulas of ``PPO.train``'s diagnostics (approx_kl, clip_fraction) and of ``explained_variance``."""
import collections

import numpy as np


class DequeRef:
    """``OnPolicyAlgorithm.ep_info_buffer``: ``deque(maxlen=W)`` of ``(r, l, env)``, appended to by ``step`` for every
    env with ``reset_happened[e] != 0`` in ascending env order (``_update_info_buffer`` walks ``infos`` in env order).
    ``per_step`` keeps how many episodes each step ended."""

    def __init__(self, window):
        self.buf = collections.deque(maxlen=int(window))
        self.total = 0
        self.per_step = []

    def step(self, reset_happened, episode_stats):
        ended = np.nonzero(np.asarray(reset_happened))[0]
        for e in ended:
            self.buf.append((np.float64(episode_stats[e, 0]), int(episode_stats[e, 1]), int(e)))
        self.total += len(ended)
        self.per_step.append(len(ended))

    def entries(self):
        return list(self.buf)


class HostDeque(DequeRef):
    """A ``DequeRef`` that ``DeviceRolloutBuffer.collect_steps(ring=...)`` can drive: ``record()`` pulls the batch's
    ``reset_happened`` and ``episode_stats`` of the step that just ran to the host."""

    def __init__(self, batch, window):
        super().__init__(window)
        self.batch = batch

    def record(self):
        self.step(self.batch.reset_happened.cpu().numpy(), self.batch.episode_stats.cpu().numpy())


class RingSim:
    """The device ring's slot rule in numpy (include/cattleherd.h ch_ep_ring_record): of the C envs that ended in a
    step, the one of rank r (ascending env order) is episode ``total + r`` and goes to slot ``(total + r) % W``; with
    C > W only ranks ``r >= C - W`` are written; then ``total += C``.  ``writers`` counts the stores per slot of the
    last step (the rule's claim: at most one)."""

    def __init__(self, window):
        self.W = int(window)
        self.ep_return = np.zeros(self.W, np.float64)
        self.ep_length = np.zeros(self.W, np.int32)
        self.ep_env = np.zeros(self.W, np.int32)
        self.total = 0
        self.writers = np.zeros(self.W, np.int64)

    def step(self, reset_happened, episode_stats):
        ended = np.nonzero(np.asarray(reset_happened))[0]
        C = len(ended)
        self.writers[:] = 0
        for r in range(max(0, C - self.W), C):
            slot = (self.total + r) % self.W
            e = ended[r]
            self.ep_return[slot], self.ep_length[slot], self.ep_env[slot] = episode_stats[e, 0], int(episode_stats[e, 1]), e
            self.writers[slot] += 1
        self.total += C

    def entries(self):
        W = self.W
        return [(self.ep_return[k % W], int(self.ep_length[k % W]), int(self.ep_env[k % W]))
                for k in range(max(0, self.total - W), self.total)]


def same_entries(got, want):
    """Exact equality of two entry lists: the returns as float64 bit patterns, lengths and envs as integers."""
    if len(got) != len(want):
        return False
    for (gr, gl, ge), (wr, wl, we) in zip(got, want):
        if np.float64(gr).view(np.int64) != np.float64(wr).view(np.int64) or int(gl) != int(wl) or int(ge) != int(we):
            return False
    return True


def update_diagnostics(model, data, idx, clip_range):
    """SB3 ``PPO.train``'s two diagnostics of one minibatch in the model's dtype (float64 for the reference):
    ``log_ratio = log_prob - old_log_prob``, ``approx_kl = mean((exp(log_ratio) - 1) - log_ratio)`` and the COUNT of
    rows with ``|ratio - 1| > clip_range`` (clip_fraction = count / B).  Returns (approx_kl [1] tensor, count, ratio)."""
    import torch
    obs, act, old, _, _ = (t.index_select(0, idx) for t in data)
    with torch.no_grad():
        _, lp, _ = model.evaluate_actions(obs, act)
        log_ratio = lp - old
        ratio = torch.exp(log_ratio)
        approx_kl = ((ratio - 1) - log_ratio).mean().view(1)
        count = int((torch.abs(ratio - 1) > clip_range).sum())
    return approx_kl, count, ratio


def explained_variance64(values, returns):
    """``1 - var(returns - values) / var(returns)`` and ``var(returns)`` in float64 numpy (population variances); the
    first is NaN when ``var(returns) == 0``, as SB3's explained_variance returns it."""
    v, y = np.asarray(values, np.float64), np.asarray(returns, np.float64)
    var_y = np.var(y)
    return (np.nan if var_y == 0 else 1.0 - np.var(y - v) / var_y), var_y


def ev_tolerance(n, ref):
    """|ev - ref| <= 4 n 2^-53 (1 + |1 - ref|): the worst-case bound of the four n-term float64 sums involved."""
    return 4.0 * n * 2.0 ** -53 * (1.0 + abs(1.0 - ref))


# The minibatch sequences of the update-statistics test on ppo_native_ref.DRIVER's 96 rows: (name, batch_size, rows).
# One step of 1, 8 and 64 rows (ppo_native_ref.idx_for's seeded rows), and 96 rows in minibatches of 64 (a partial last
# one of 32, on the weights the first step left).  PARTIAL_SEED was chosen so that the float64 reference meets
# check_clip_conditions in both steps (test_train_log_cpu.py asserts it).
PARTIAL_SEED = 1
UPDATE_CASES = (("one", 1), ("eight", 8), ("full", 64), ("partial", 64))


def update_case_idx(name, batch):
    import torch
    import ppo_native_ref as R
    if name == "partial":
        return torch.randperm(R.DRIVER["rows"], generator=torch.Generator().manual_seed(PARTIAL_SEED))
    return R.idx_for(R.DRIVER, batch)


def update_reference(model, data, idx, batch_size, hp):
    """The minibatch steps of ``idx`` in ``model``'s dtype through the project's torch restatement (ppo_native_ref.ref_grad
    + clip_grad_norm_ + Adam): per step (stats4, approx_kl [1], clip count, ratio, clipped), each from the weights the
    step starts from."""
    import torch
    import ppo_native_ref as R
    opt = torch.optim.Adam(model.parameters(), lr=hp["learning_rate"], eps=1e-5)
    out = []
    for lo in range(0, idx.numel(), batch_size):
        mb = idx[lo:lo + batch_size]
        akl, count, _ = update_diagnostics(model, data, mb, hp["clip_range"])
        _, st, ratio, clipped = R.ref_grad(model, data, mb, **hp)     # (leaves the gradients in p.grad)
        torch.nn.utils.clip_grad_norm_(model.parameters(), hp["max_grad_norm"])
        opt.step()
        out.append((st, akl, count, ratio, clipped))
    return out
