"""Reference for the episode books across explicit resets (tests/test_reset_ref_cpu.py, tests/test_gpu_reset.py).

``Monitor`` is SB3's ``Monitor`` wrapper (stable_baselines3/common/monitor.py: ``reset`` clears the reward list,
``step`` appends and, on done, reports ``{"r": sum, "l": len}``) for E envs at once, in plain numpy float64: the
device keeps the same books in the per-env metric rows (running return and length) and reports them through
``episode_stats`` and the EPISODES / RETURN_SUM / LENGTH_SUM sums of ``metrics()``.

``books_schedule`` is the one schedule both the CPU test (on oracle envs) and the GPU test (on a HerdBatch) run, so
that the cases it must contain are asserted once, without a device.
"""
import numpy as np


def marl_reward(per_agent):
    """The env's reward of a MARL step as the kernel's ``ret`` sums it: the per-agent rewards over the non-NaN
    entries (agents not live at the start of the step report NaN)."""
    return np.nansum(np.asarray(per_agent, np.float64), axis=-1)


class Monitor:
    """Per env: the open episode's running return and length.  ``step(reward, done)``: both grow; where ``done``,
    the pair is emitted as that env's last episode and counted in the sums, then zeroed.  ``reset(mask)``: both
    zeroed, nothing emitted, nothing counted (Monitor.reset).  ``last`` starts at zero, as the device's
    ``episode_stats`` buffer does, so envs that never end compare too."""

    def __init__(self, E):
        self.E = E
        self.ret = np.zeros(E, np.float64)
        self.len = np.zeros(E, np.int64)
        self.abs = np.zeros(E, np.float64)          # sum |r| of the open episode (the error bound's scale)
        self.last = np.zeros((E, 2), np.float64)    # last ended episode: return, length
        self.last_abs = np.zeros(E, np.float64)
        self.episodes, self.return_sum, self.length_sum, self.abs_sum = 0, 0.0, 0, 0.0
        self.steps = 0
        self.abandoned = 0                          # steps of episodes an explicit reset cut off
        self.n_ended = np.zeros(E, np.int64)
        self.n_reset_open = np.zeros(E, np.int64)   # explicit resets that hit an open episode (length > 0)
        self.n_reset_fresh = np.zeros(E, np.int64)  # ... an env that ended on the previous step (or was just reset)

    def step(self, reward, done):
        r = np.asarray(reward, np.float64).reshape(self.E)
        done = np.asarray(done).astype(bool).reshape(self.E)
        self.ret = self.ret + r
        self.abs = self.abs + np.abs(r)
        self.len = self.len + 1
        self.steps += self.E
        for e in np.nonzero(done)[0]:
            self.last[e] = (self.ret[e], self.len[e])
            self.last_abs[e] = self.abs[e]
            self.episodes += 1
            self.return_sum += self.ret[e]
            self.length_sum += int(self.len[e])
            self.abs_sum += self.abs[e]
        self.n_ended += done
        self.ret[done] = 0
        self.len[done] = 0
        self.abs[done] = 0
        return done

    def reset(self, mask=None):
        m = np.ones(self.E, bool) if mask is None else np.asarray(mask).astype(bool).reshape(self.E)
        opened = m & (self.len > 0)
        self.n_reset_open += opened
        self.n_reset_fresh += m & ~opened
        self.abandoned += int(self.len[m].sum())
        self.ret[m] = 0
        self.len[m] = 0
        self.abs[m] = 0


# ---- the schedule of the episode-books tests ------------------------------------------------------------------------
K_BEFORE, J_AFTER = 9, 6
VARIANTS = ("full", "masked", "masked_with")


def books_schedule(E, variant, k=K_BEFORE, j=J_AFTER):
    """``k`` steps, one explicit reset, ``j`` steps, and one step in which every env is forced to end.

    Returns ``(reset_mask, force)``: the bool [E] mask of the explicit reset after step ``k`` (``full``: every env;
    ``masked`` / ``masked_with``: the odd envs), and ``force`` = {step (1-based): bool [E]} of the envs rigged, just
    before that step, to end in it:
      envs = 3 mod 8 end in step k          -> reset on the step after they ended (books already zero)
      envs = 5 mod 8 end in step k // 2     -> reset with an open episode shorter than k
      envs = 2 mod 8 end in step k // 2     -> (masked variants) never reset, ended before and after the reset
      every env ends in step k + j + 1."""
    assert variant in VARIANTS
    e = np.arange(E)
    mask = np.ones(E, bool) if variant == "full" else e % 2 == 1
    force = {k: e % 8 == 3, k // 2: (e % 8 == 5) | (e % 8 == 2), k + j + 1: np.ones(E, bool)}
    return mask, force


def ring_positions(cow_pos, n):
    """Drone positions [..., n, 3] in a row through the herd centroid at the hover altitude: the MARL episode's
    level-2 termination (the drone centroid within approach_min of the herd's) for every agent at once."""
    c = np.asarray(cow_pos, np.float64).mean(axis=-2)
    out = np.zeros(c.shape[:-1] + (n, 3))
    for i in range(n):
        out[..., i, 0] = c[..., 0] + 0.3 * (i - (n - 1) / 2)
        out[..., i, 1] = c[..., 1]
        out[..., i, 2] = 0.45
    return out
