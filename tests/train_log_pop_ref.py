"""Shared pieces of the population training log's tests (test_train_log_pop_cpu.py, test_gpu_train_log_pop.py): one SB3
``ep_info_buffer`` deque per member, fed with the member's slice of a step's ``reset_happened`` / ``episode_stats``
under the solo append rule (train_log_ref.DequeRef), and the fixed summation order of ``ch_ep_ring_pop_summary``
(include/cattleherd.h) restated in numpy float64."""
import numpy as np

from train_log_ref import DequeRef

SUMMARY_THREADS = 64


class PopDequeRef:
    """P deques of window W; member p owns envs ``[pE, (p + 1)E)`` and its entries carry member-local env indices."""

    def __init__(self, n_members, member_envs, window):
        self.P, self.E, self.W = int(n_members), int(member_envs), int(window)
        self.members = [DequeRef(window) for _ in range(self.P)]

    def step(self, reset_happened, episode_stats):
        rh, st = np.asarray(reset_happened), np.asarray(episode_stats)
        assert rh.shape == (self.P * self.E,) and st.shape == (self.P * self.E, 2)
        for p, m in enumerate(self.members):
            m.step(rh[p * self.E:(p + 1) * self.E], st[p * self.E:(p + 1) * self.E])

    def entries(self, p):
        return self.members[p].entries()

    def totals(self):
        return [m.total for m in self.members]


def ring_entries(ep_return, ep_length, ep_env, total, window):
    """One ring's content, oldest first, from its raw arrays ([W] each) and its total."""
    W, total = int(window), int(total)
    return [(ep_return[k % W], int(ep_length[k % W]), int(ep_env[k % W])) for k in range(max(0, total - W), total)]


def bits_equal64(got, want):
    """float64 arrays equal bit for bit where `want` is not NaN, NaN exactly where `want` is (any payload)."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and \
        bool(np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


def fixed_order_sum(x):
    """The sum of ``x`` (chronological order, oldest first) as the summary kernel adds it: 64 threads, thread t starts
    from 0.0 and adds positions t, t + 64, ... in order; then the halving tree s[t] += s[t + w] for w = 32 .. 1."""
    x = np.asarray(x, np.float64)
    s = np.zeros(SUMMARY_THREADS, np.float64)
    for t in range(SUMMARY_THREADS):
        for v in x[t::SUMMARY_THREADS]:
            s[t] = s[t] + v
    w = SUMMARY_THREADS // 2
    while w > 0:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    return s[0]


def fitness_ref(entries_per_member, totals):
    """``[P, 4]`` float64: count, mean return, mean length (both ``fixed_order_sum / count``; NaN for an empty ring)
    and total, from every member's entries (oldest first) and its total."""
    out = np.full((len(entries_per_member), 4), np.nan, np.float64)
    for p, (entries, total) in enumerate(zip(entries_per_member, totals)):
        count = len(entries)
        out[p, 0], out[p, 3] = count, total
        if count:
            out[p, 1] = fixed_order_sum([r for r, _, _ in entries]) / np.float64(count)
            out[p, 2] = fixed_order_sum([float(n) for _, n, _ in entries]) / np.float64(count)
    return out
