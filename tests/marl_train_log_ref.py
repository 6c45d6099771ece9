"""Shared pieces of the device-side RLlib training log's tests (test_marl_train_log_cpu.py, test_gpu_marl_train_log.py).

``MarlRingRef`` is the reference of the MARL episode ring (cattleherd.train_log.MarlEpisodeRing, ch_marl_ep_ring_*): a
host ``deque(maxlen=W)`` plus the open episodes' accumulators and the sampling counters, in float64, fed one step at a
time.  Beside the deque it keeps the image the device arrays must hold (episode k in slot k % W, slots never cleared),
so that a test can compare every array exactly.

``ref_train_log`` restates one training iteration with RLlib's learner statistics (marl_ppo_ref.ref_train with the
three columns ch_marl_ppo_train_log adds), in the model's dtype: float64 is the reference, float32 the yardstick.

The synthetic step outputs, the bias policy and the graded near-herd injection are restated from
tests/test_gpu_marl_eval.py."""
from collections import deque

import numpy as np
import torch

import marl_ppo_ref as R

LOG_KEYS = ["policy_loss", "vf_loss", "vf_loss_unclipped", "vf_explained_var", "entropy", "mean_kl_loss", "total_loss",
            "curr_kl_coeff", "curr_entropy_coeff", "gradients_default_optimizer_global_norm",
            "num_module_steps_trained"]
RING_ARRAYS = ("ep_return", "agent_return", "ep_length", "agent_length", "ep_env", "total", "acc_return", "acc_length",
               "acc_steps", "env_steps", "agent_steps")


class MarlRingRef:
    def __init__(self, E, N, W):
        self.E, self.N, self.W = E, N, W
        self.ep_return = np.zeros(W, np.float64)
        self.agent_return = np.zeros((W, N), np.float64)
        self.ep_length = np.zeros(W, np.int32)
        self.agent_length = np.zeros((W, N), np.int32)
        self.ep_env = np.zeros(W, np.int32)
        self.acc_return = np.zeros((E, N), np.float64)
        self.acc_length = np.zeros((E, N), np.int32)
        self.acc_steps = np.zeros(E, np.int32)
        self.agent_steps = np.zeros(N, np.int64)
        self.begin()
        # what a run exercised
        self.max_ended, self.steps_without_end, self.steps = 0, 0, 0
        self.filed = []   # (step, env, ep_length, agent_length) of every appended episode, dropped ones included

    def begin(self):
        """total, the counters and the accumulators to zero: an open episode counts from zero."""
        self.buf = deque(maxlen=self.W)
        self.total, self.env_steps = 0, 0
        self.acc_return[:] = 0.0
        self.acc_length[:] = 0
        self.acc_steps[:] = 0
        self.agent_steps[:] = 0

    def step(self, live, reward, reset):
        """live uint8 [E, N] (at the step's start), reward float32 [E, N], reset uint8 [E]."""
        live = np.asarray(live).reshape(self.E, self.N) != 0
        reward = np.asarray(reward, np.float32).reshape(self.E, self.N)
        for e, i in zip(*np.nonzero(live)):   # (a reward that is not live is never touched)
            self.acc_return[e, i] += np.float64(reward[e, i])
            self.acc_length[e, i] += 1
        self.acc_steps += 1
        self.env_steps += self.E
        self.agent_steps += live.sum(0)
        ended = np.flatnonzero(np.asarray(reset).reshape(self.E))
        for e in ended:   # ascending env order
            s = 0.0
            for i in range(self.N):   # agent order
                s += self.acc_return[e, i]
            entry = (s, int(self.acc_steps[e]), self.acc_return[e].copy(), self.acc_length[e].copy(), int(e))
            self.buf.append(entry)
            k = self.total % self.W
            self.ep_return[k], self.ep_length[k], self.ep_env[k] = entry[0], entry[1], entry[4]
            self.agent_return[k], self.agent_length[k] = entry[2], entry[3]
            self.filed.append((self.steps, int(e), entry[1], entry[3].copy()))
            self.total += 1
            self.acc_return[e] = 0.0
            self.acc_length[e] = 0
            self.acc_steps[e] = 0
        self.max_ended = max(self.max_ended, len(ended))
        self.steps_without_end += len(ended) == 0
        self.steps += 1

    def arrays(self):
        out = {k: getattr(self, k) for k in RING_ARRAYS if k not in ("total", "env_steps")}
        out["total"] = np.array([self.total], np.int64)
        out["env_steps"] = np.array([self.env_steps], np.int64)
        return out

    def entries(self):
        return list(self.buf)


def assert_ring(got, want, what):
    """Every array of the device ring (MarlEpisodeRing.arrays()) equals the reference's, exactly."""
    for k in RING_ARRAYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, k, np.flatnonzero((g != w).reshape(-1))[:8])


def assert_entries(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[4] == w[4]
        assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3])


def synthetic(E, W, N=3, S=30):
    """Seeded step outputs (test_gpu_marl_eval._synthetic's): live [S, E, N] with p = 0.7, float32 rewards [S, E, N]
    with NaN / 1e30 at the slots that are not live (summing one of them shows), reset_happened [S, E] with p = 0.3."""
    rng = np.random.default_rng(1000 * E + W)
    live = (rng.random((S, E, N)) < 0.7).astype(np.uint8)
    reward = rng.normal(0.0, 10.0, (S, E, N)).astype(np.float32)
    poison = np.where(rng.random((S, E, N)) < 0.5, np.float32(np.nan), np.float32(1e30)).astype(np.float32)
    reward = np.where(live != 0, reward, poison)
    rh = (rng.random((S, E)) < 0.3).astype(np.uint8)
    return live, reward, rh


# ---- the graded near-herd injection and the approach-biased policy (restated from tests/test_gpu_marl_eval.py) -------
APPROACH = [0.0, -1.0, 0.0, 1.0, -3.0, -3.0, -3.0, -3.0]   # fly along -y at the speed limit, log_std -3
CLOSE = 0.31


def bias_policy(bias):
    """A policy whose output is `bias` exactly on every row (zero weights)."""
    from cattleherd.policy import DevicePolicy
    return DevicePolicy([(torch.zeros(len(bias), 86), torch.tensor(bias, dtype=torch.float32))], "tanh", None)


def inject_graded(b, n):
    """The envs e % 8 == 4 start 0.45 m from the herd centroid, inside level 2's approach radius: every agent
    terminates and the env ends in the next step.  Those with e % 8 == 0 are n + 2 successes short of level 3 and start
    CLOSE m out: agent 0 drops out in the first step, the others terminate a few steps later inside level 3's 0.3 m.
    The drones of the others start 0.6 .. 1.0 m out and fly towards the herd (APPROACH), crossing the radius at steps
    spread over the run; every other one of those is n + 2 successes short as well."""
    E = b.n_envs
    s = b.get_state()
    e = np.arange(E)
    near = e % 4 == 0
    far = np.flatnonzero(~near)
    dist = np.full(E, 0.45)
    dist[far] = np.linspace(0.6, 1.0, len(far))
    dist[e % 8 == 0] = CLOSE
    c = s["cow_pos"].mean(1)
    for k in range(n):
        s["drone_pos"][:, k, 0] = c[:, 0] + 0.5 * (k - (n - 1) / 2)
        s["drone_pos"][:, k, 1] = c[:, 1] + dist
    tally = s["tally"].copy()
    tally[e % 8 == 0] = 100 - n - 2
    tally[far[::2]] = 100 - n - 2
    b.set_state({"drone_pos": s["drone_pos"], "tally": tally})


def make_graded(E, n, m):
    from cattleherd.env import HerdBatch
    b = HerdBatch(E, n, m, mode="marl", curriculum_level=2, min_drones=n, max_drones=n)
    b.reset()
    inject_graded(b, n)
    return b


def feed_from_buffer(ref, rb):
    """Feed the reference a collected buffer step by step: live = agent_mask[t], reward = rewards[t]; an env ended at t
    where every agent that is live at t has terminated[t]."""
    E, N = ref.E, ref.N
    mask = rb.agent_mask.cpu().numpy().reshape(rb.T, E, N)
    rew = rb.rewards.cpu().numpy().reshape(rb.T, E, N)
    term = rb.terminated.cpu().numpy().reshape(rb.T, E, N)
    for t in range(rb.T):
        live = mask[t] != 0
        ended = live.any(1) & ((term[t] != 0) | ~live).all(1)
        ref.step(mask[t], rew[t], ended.astype(np.uint8))


# ---- the learner statistics -------------------------------------------------------------------------------------------
def explained_variance(y, v):
    """max(-1, 1 - var(y - v) / (var(y) + 1e-6)), unbiased variances, in the tensors' dtype (numpy-free torch; a one-row
    input gives NaN)."""
    def var(x):
        return ((x - x.mean()) ** 2).sum() / (x.numel() - 1)
    ev = 1.0 - var(y - v) / (var(y) + 1e-6)
    return torch.where(ev < -1.0, torch.full_like(ev, -1.0), ev)


def log_columns(model, mb, hp, kl_coeff=None):
    """[vf_loss_unclipped, total_loss, vf_explained_var] of one minibatch at the model's current parameters, from
    marl_ppo_ref.loss's own terms."""
    with torch.no_grad():
        total, _, aux = R.loss(model, mb, hp, kl_coeff)
        v = R.head(model, mb[0], hp["log_std_clip"])[3]
        return torch.stack([aux["e2"].mean(), total, explained_variance(mb[5], v)])


def ref_epoch_log(model, opt, data, idx, batch, hp, kl_coeff=None):
    """marl_ppo_ref.ref_epoch with the three log columns: [steps, 8], each row evaluated before that step's update."""
    rows = []
    for j in range(0, idx.numel(), batch):
        mb_idx = idx[j:j + batch]
        extra = log_columns(model, tuple(t.index_select(0, mb_idx) for t in data), hp, kl_coeff)
        _, st, _ = R.ref_grad(model, data, mb_idx, hp, kl_coeff)
        R.clip_and_step(model, opt, hp["grad_clip"])
        rows.append(torch.cat([st, extra]))
    return torch.stack(rows)


def ref_train_log(model, rb, hp, kl_target, num_epochs, minibatch_size, seed):
    """marl_ppo_ref.ref_train with the log columns: (steps, stats [steps, 8], the coefficient afterwards, live rows)."""
    dev = model.device
    n_all = rb.T * rb.rows
    obs = rb.obs.view(n_all, -1)
    live = torch.nonzero(rb.agent_mask.view(n_all)).view(-1)
    with torch.no_grad():
        mean, _, ls, _ = R.head(model, obs, hp["log_std_clip"])
        old_dist = torch.cat([mean, ls], 1)
    adv = rb.advantages.view(n_all)
    a = adv[live]
    adv = (adv - a.mean()) / max(1e-4, float(a.std(unbiased=False)))
    data = (obs, rb.actions.view(n_all, -1), rb.log_probs.view(n_all), old_dist, adv, rb.returns.view(n_all))
    klc = torch.full((1,), hp["kl_coeff"], dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    opt = R.adam(model, hp)
    stats = []
    for _ in range(num_epochs):
        perm = live[torch.randperm(live.numel(), device=dev, generator=gen)]
        stats.append(ref_epoch_log(model, opt, data, perm, minibatch_size, hp, klc))
    stats = torch.cat(stats)
    kl = float(stats[-1, 3])
    if kl > 2.0 * kl_target:
        klc = klc * 1.5
    elif kl < 0.5 * kl_target:
        klc = klc * 0.5
    return stats.shape[0], stats, klc, int(live.numel())


def cpu_buffer(shape, dtype=torch.float64, T=2):
    """A buffer-like object on the host from marl_ppo_ref's synthetic data of `shape` (rows split over T steps), every
    row live but a few: the fields MarlPPOUpdate.train reads."""
    import types
    obs, act, old_lp, _, adv, ret = R.make_data(shape, "cpu")
    rows = shape["rows"] // T
    mask = torch.ones(T * rows, dtype=torch.uint8)
    mask[::7] = 0
    f = lambda t: t[:T * rows].to(dtype).reshape(T, rows, *t.shape[1:]).contiguous()   # noqa: E731
    return types.SimpleNamespace(T=T, rows=rows, obs=f(obs), actions=f(act), log_probs=f(old_lp), advantages=f(adv),
                                 returns=f(ret), agent_mask=mask.reshape(T, rows))
