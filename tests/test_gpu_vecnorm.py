"""Device-side VecNormalize (csrc/ch_norm.hip, cattleherd/vec_normalize.py) against the float64 numpy restatement of
SB3's RunningMeanStd / VecNormalize (tests/vecnorm_ref.py).

Tolerances.  Statistics: any summation order of n float64 terms errs by at most (n - 1) 2^-53 sum|term|, so a running
statistic is accepted within 4 n 2^-53 sum|terms| of the reference's, the terms being those of that statistic's sum
(vecnorm_ref.abs_terms computes them from the input); the count is exact.  The apply is numpy's bit for bit on the
device's own statistics.  Normalised values compared across two sets of statistics (device's and reference's) get the
float32 image of the statistics' bound.
"""
import ctypes

import numpy as np
import pytest

import vecnorm_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _inputs(rows, dim, seed):
    """A seeded normal times per-column scales over 1e-3..1e3 plus offsets up to 1e3 (cancellation); from 3 columns
    on, column 0 is all zero and column 1 the constant 3.5 (batch variance exactly 0)."""
    rng = np.random.default_rng(seed)
    scales = rng.permutation(np.logspace(-3, 3, dim))
    x = rng.normal(size=(rows, dim)) * scales + rng.uniform(-1e3, 1e3, dim)
    if dim >= 3:
        x[:, 0], x[:, 1] = 0.0, 3.5
    return x.astype(np.float32)


def _dev(x, misalign=False):
    """x on the device; misalign: at a 4-byte offset from a 16-byte boundary (the scalar path whatever dim is)."""
    import torch
    if not misalign:
        return torch.from_numpy(x).cuda()
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    buf[1:].copy_(torch.from_numpy(x).reshape(-1))
    return buf[1:].view(x.shape)


def _check_stats(got, ref, batches):
    n, mt, vt = R.abs_terms(batches)
    mean, var, count = got
    assert count == ref.count
    em, ev = np.abs(mean - ref.mean), np.abs(var - ref.var)
    assert np.all(em <= 4 * n * U * mt), (n, float(np.max(em / np.maximum(4 * n * U * mt, 1e-300))))
    assert np.all(ev <= 4 * n * U * vt), (n, float(np.max(ev / np.maximum(4 * n * U * vt, 1e-300))))
    return 4 * n * U * vt


CASES = [(r, d, False) for r in (1, 3, 64, 65, 1100) for d in (1, 7, 86, 172, 1032)] + \
    [(65, 172, True), (1100, 8, True), (16400, 7, False)]   # 16-byte-misaligned base; chunks of more than one sub-block


@pytest.mark.parametrize("rows,dim,misalign", CASES)
def test_moments_and_running_update(rows, dim, misalign):
    from cattleherd.vec_normalize import DeviceNormalizer
    sizes = (rows, rows + 2, rows // 3 + 1)
    n = DeviceNormalizer("cuda", dim, 1, max_rows=max(sizes))
    ref = R.RunningMeanStd((dim,))
    m0, v0, c0 = n.obs_rms
    assert np.all(m0 == 0) and np.all(v0 == 1) and c0 == 1e-4
    batches = []
    for k, r in enumerate(sizes):
        x = _inputs(r, dim, seed=100 * rows + dim + k)
        batches.append(x)
        n.update_obs(_dev(x, misalign))
        ref.update(x)
        _check_stats(n.obs_rms, ref, batches)
    if dim >= 3:   # the zero column stays at mean 0; the constant one has no batch variance to add
        mean, var, count = n.obs_rms
        assert mean[0] == 0.0 and var[0] == ref.var[0] and var[1] == ref.var[1]


@pytest.mark.parametrize("rows,dim,misalign", [(65, 7, False), (65, 172, False), (300, 1032, False), (65, 172, True)])
def test_apply_is_numpys_bit_for_bit(rows, dim, misalign):
    import torch
    from cattleherd.vec_normalize import DeviceNormalizer
    n = DeviceNormalizer("cuda", dim, 1, clip_obs=2.5, max_rows=rows)
    x = _inputs(rows, dim, seed=7 * dim + rows)
    n.update_obs(_dev(x))
    s = n.state_dict()
    s["obs_var"][:2] = 0.0            # zero-variance columns: (x - mean) / sqrt(eps), clipped
    n.load_state_dict(s)
    mean, var, _ = n.obs_rms           # the device's own statistics
    assert np.array_equal(var, s["obs_var"])
    x2 = _inputs(rows, dim, seed=dim + rows + 1)   # another draw: values beyond +- clip_obs standard deviations
    x2[0, :] = 1e30
    want = np.clip((x2.astype(np.float64) - mean) / np.sqrt(var + 1e-8), -2.5, 2.5).astype(np.float32)
    assert (np.abs(want) == 2.5).any() and (np.abs(want) < 2.5).any()
    dx = _dev(x2, misalign)
    got = n.normalize_obs(dx).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.all(var[:2] == 0.0) and np.all(got[1:, 0] == 0.0) and np.all(np.abs(got[0]) == 2.5)
    # a row mask: unselected rows of y keep the sentinel
    mask = (np.arange(rows) % 3 == 1).astype(np.uint8)
    y = torch.full((rows, dim), 777.0, dtype=torch.float32, device="cuda")
    n.normalize_obs(dx, out=y, row_mask=torch.from_numpy(mask).cuda())
    y = y.cpu().numpy()
    assert np.array_equal(y[mask == 1].view(np.int32), want[mask == 1].view(np.int32)) and np.all(y[mask == 0] == 777.0)
    # in place
    z = dx.clone() if not misalign else dx
    n.normalize_obs(z, out=z)
    assert np.array_equal(z.cpu().numpy().view(np.int32), want.view(np.int32))
    # norm_obs off: a copy
    n.norm_obs = False
    assert np.array_equal(n.normalize_obs(_dev(x2)).cpu().numpy().view(np.int32), x2.view(np.int32))


def _done_pattern(E, t):
    """Dones at step 0, and consecutive ones (env 0: steps 0, 1, 2; env e: steps e % 5 and e % 5 + 1)."""
    e = np.arange(E)
    te = ((e % 5 == t) | ((e == 0) & (t < 3))).astype(np.uint8)
    tr = ((e % 5 + 1 == t) & (e > 0)).astype(np.uint8)
    return te, tr


@pytest.mark.parametrize("E", [1, 65, 1100, 4100])   # 4100: past one workgroup's envs (the chunked launches)
def test_reward_kernel(E):
    import torch
    from cattleherd.vec_normalize import DeviceNormalizer
    n = DeviceNormalizer("cuda", 1, E, gamma=0.9, clip_reward=1.5)
    ref = R.VecNormalize(E, (1,), gamma=0.9, clip_reward=1.5)
    rng = np.random.default_rng(E)
    obs = np.zeros((E, 1), np.float32)
    rets, abs_ret = [], np.zeros(E)
    for t in range(6):
        rew = (rng.normal(size=E) * 3 + 0.5).astype(np.float32)
        te, tr = _done_pattern(E, t)
        d_rew = torch.from_numpy(rew).cuda()
        out = n.step_reward(d_rew, torch.from_numpy(te).cuda(), torch.from_numpy(tr).cuda()).cpu().numpy()
        assert np.array_equal(d_rew.cpu().numpy().view(np.int32), rew.view(np.int32))   # the raw reward stays
        ret_before_zero = ref.ret * 0.9 + rew.astype(np.float64)
        _, want, _ = ref.step(obs, rew, (te | tr).astype(bool))
        rets.append(ret_before_zero)
        mean, var, count = n.ret_rms
        bound_v = _check_stats((np.float64(mean), np.float64(var), count), ref.ret_rms, rets)
        ret = n.ret.cpu().numpy()
        done = (te | tr).astype(bool)
        assert np.all(ret[done] == 0.0)
        # ret is a sum of t + 1 terms gamma^k r: the same bound (the device forms it with the reference's operations)
        abs_ret = abs_ret * 0.9 + np.abs(rew.astype(np.float64))
        assert np.all(np.abs(ret - ref.ret) <= 4 * (t + 1) * U * abs_ret)
        abs_ret[done] = 0.0
        q = rew.astype(np.float64) / np.sqrt(ref.ret_rms.var + 1e-8)
        tol = np.abs(q) * (bound_v / ref.ret_rms.var) + np.spacing(np.abs(want))   # the bound's float32 image
        assert np.all(np.abs(out.astype(np.float64) - want) <= tol)
        assert (np.abs(want) == 1.5).any() or E == 1
    # training off: nothing moves but the zeroing; norm_reward off: the raw reward out
    n.training = False
    before = n.state_dict()
    te, tr = _done_pattern(E, 1)
    rew = rng.normal(size=E).astype(np.float32)
    out = n.step_reward(torch.from_numpy(rew).cuda(), torch.from_numpy(te).cuda(), torch.from_numpy(tr).cuda()).cpu().numpy()
    after = n.state_dict()
    assert after["ret_var"] == before["ret_var"] and after["ret_count"] == before["ret_count"]
    keep = (te | tr) == 0
    assert np.array_equal(after["ret"][keep], before["ret"][keep]) and np.all(after["ret"][~keep] == 0)
    want = np.clip(rew.astype(np.float64) / np.sqrt(before["ret_var"] + 1e-8), -1.5, 1.5).astype(np.float32)
    assert np.array_equal(out.view(np.int32), want.view(np.int32))
    n.norm_reward = False
    out = n.step_reward(torch.from_numpy(rew).cuda(), torch.from_numpy(te).cuda(), torch.from_numpy(tr).cuda()).cpu().numpy()
    assert np.array_equal(out.view(np.int32), rew.view(np.int32))


def test_two_runs_are_bit_identical():
    import torch
    from cattleherd.vec_normalize import DeviceNormalizer
    E, dim = 4100, 172
    xs = [_dev(_inputs(r, dim, seed=r)) for r in (1100, 4100, 65)]
    rew = torch.from_numpy(np.random.default_rng(3).normal(size=E).astype(np.float32)).cuda()
    te, tr = (torch.from_numpy(a).cuda() for a in _done_pattern(E, 0))
    blocks, outs = [], []
    for _ in range(2):
        n = DeviceNormalizer("cuda", dim, E)
        for x in xs:
            n.update_obs(x)
        for _ in range(3):
            r = n.step_reward(rew, te, tr).clone()
        outs.append((n.normalize_obs(xs[1]).cpu().numpy(), r.cpu().numpy()))
        blocks.append(n._block.cpu().numpy())
    assert np.array_equal(blocks[0].view(np.int64), blocks[1].view(np.int64))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the collection ---------------------------------------------------------------------------------------------
E_C, T_C, ACT = 256, 8, 16
RB_KEYS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns",
           "last_episode_starts")


def _setup(seed=0x5EED, **norm_kw):
    import torch
    from cattleherd.env import HerdBatch
    from cattleherd.policy import DevicePolicy
    from cattleherd.rollout import DeviceRolloutBuffer
    from cattleherd.vec_normalize import DeviceVecNormalize
    # NUM_DRONES varies between envs (3 or 4; with 2 drones the reference's CTDE reward is NaN, DESIGN "Quirks")
    b = HerdBatch(E_C, 4, 16, mode="ctde", min_drones=3, max_drones=4, curriculum_level=7, seed=seed)
    b.reset()
    # level 7's 80 s limit is a step counter of 4800: three groups of envs reach it inside the rollout (truncations)
    b.set_state({"step_counter": 4800 - 4 * np.array([0, 0, 2, 2, 5, 1000, 1000, 1000])[np.arange(E_C) % 8]})
    actor = DevicePolicy(DevicePolicy.random_layers([12 * 86, 64, 64, ACT], seed=1), "tanh", None)
    critic = DevicePolicy(DevicePolicy.random_layers([12 * 86, 64, 64, 1], seed=2), "tanh", None)
    rb = DeviceRolloutBuffer(b, T_C, act_dim=ACT)
    n = DeviceVecNormalize(b, **norm_kw)
    n.reset_obs()
    return b, actor, critic, rb, n, torch.full((ACT,), -1.0, device=b.device)


def _equal_bits(a, b):
    return np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


@pytest.fixture(scope="module")
def steps_run():
    """collect_steps(normalizer=...) once, with the raw step outputs recorded from the Python loop; shared, unchanged."""
    from cattleherd.train_log import EpisodeRing
    b, actor, critic, rb, n, log_std = _setup()
    obs0 = b.obs.view(E_C, -1).cpu().numpy().copy()
    num = b.env_ints()["n"].copy()
    ring = EpisodeRing(b, window=512).begin()
    rec = []

    def on_step(t):
        rec.append({"obs": b.obs.view(E_C, -1).cpu().numpy().copy(), "reward": b.reward.view(E_C).cpu().numpy().copy(),
                    "terminated": b.terminated.view(E_C).cpu().numpy().copy(),
                    "truncated": b.truncated.view(E_C).cpu().numpy().copy(),
                    "reset": b.reset_happened.cpu().numpy().copy(), "n": b.env_ints()["n"].copy()})

    rb.collect_steps(actor, critic, log_std, seed=9, ring=ring, normalizer=n, on_step=on_step)
    out = {"rb": {k: getattr(rb, k).clone() for k in RB_KEYS}, "state": n.state_dict(), "block": n._block.clone(),
           "rec": rec, "obs0": obs0, "num": num, "ring": ring.entries(), "critic": critic}
    b.close()
    return out


def test_collect_equals_collect_steps_bit_for_bit(steps_run):
    from cattleherd.train_log import EpisodeRing
    b, actor, critic, rb, n, log_std = _setup()
    ring = EpisodeRing(b, window=512).begin()
    rb.collect(actor, critic, log_std, seed=9, ring=ring, normalizer=n)
    for k in RB_KEYS:
        assert _equal_bits(getattr(rb, k), steps_run["rb"][k]), k
    assert np.array_equal(n._block.cpu().numpy().view(np.int64), steps_run["block"].cpu().numpy().view(np.int64))
    assert ring.entries() == steps_run["ring"]
    b.close()


def test_collect_steps_agrees_with_the_host_replay(steps_run):
    rec, st = steps_run["rec"], steps_run["state"]
    D = 12 * 86
    ref = R.VecNormalize(E_C, (D,))
    def obs_tolerance(o):
        """The float32 image of the statistics' bound under which ``o`` was normalised: the quotient's sensitivity to
        the mean (1 / sd) and to the variance (|q| / var), plus one float32 spacing for the cast."""
        n_t, mt, vt = R.abs_terms(batches)
        v = ref.obs_rms.var + 1e-8
        return 4 * n_t * U * (mt / np.sqrt(v) + np.abs(o.astype(np.float64)) * vt / v) + np.spacing(np.abs(o))

    batches, rets, want_rew = [steps_run["obs0"]], [], []
    want_obs = [ref.reset(steps_run["obs0"])]
    tol_obs = [obs_tolerance(want_obs[0])]
    for t, r in enumerate(rec):
        rets.append(ref.ret * 0.99 + r["reward"].astype(np.float64))
        o, rw, _ = ref.step(r["obs"], r["reward"], (r["terminated"] | r["truncated"]).astype(bool))
        batches.append(r["obs"])
        want_obs.append(o)
        tol_obs.append(obs_tolerance(o))
        want_rew.append(rw)
    _check_stats((st["obs_mean"], st["obs_var"], st["obs_count"]), ref.obs_rms, batches)
    bound_r = _check_stats((np.float64(st["ret_mean"]), np.float64(st["ret_var"]), st["ret_count"]), ref.ret_rms, rets)
    got_obs = steps_run["rb"]["obs"].cpu().numpy()
    for t in range(T_C):
        assert np.all(np.abs(got_obs[t].astype(np.float64) - want_obs[t]) <= tol_obs[t]), t
    # rewards: without a bootstrap term where no env was truncated and not terminated
    got_rew = steps_run["rb"]["rewards"].cpu().numpy()
    for t, r in enumerate(rec):
        plain = ~((r["truncated"] == 1) & (r["terminated"] == 0))
        q = np.abs(want_rew[t].astype(np.float64))
        tol = q * bound_r / ref.ret_rms.var + np.spacing(np.abs(want_rew[t]))
        assert np.all(np.abs(got_rew[t].astype(np.float64) - want_rew[t])[plain] <= tol[plain]), t


def test_forward_is_dense_on_the_normalised_observation(steps_run):
    import torch
    critic, obs = steps_run["critic"], steps_run["rb"]["obs"]
    h = obs.double().cpu().reshape(-1, critic.dims[0])
    for i, (w, bias) in enumerate(zip(critic.weights, critic.biases)):
        h = h @ w.double().cpu().t() + bias.double().cpu()
        if i < len(critic.weights) - 1:
            h = torch.tanh(h)
    got = steps_run["rb"]["values"].cpu().double().reshape(-1, 1)
    assert torch.allclose(got, h, rtol=2e-5, atol=2e-5), float((got - h).abs().max())
    # NUM_DRONES varies, and the tail features of an env with fewer drones are not zero once normalised: a forward
    # that skipped them (ch_policy_forward's rule) would miss the reference above
    num = steps_run["num"]
    assert num.min() < 4 and num.max() == 4
    e = int(np.argmin(num))
    assert np.isfinite(steps_run["rb"]["rewards"].cpu().numpy()).all()
    tail = obs[0, e].cpu().numpy().reshape(12, 86)[num[e]:4]
    assert np.abs(tail).max() > 1e-3
    skipped = obs.clone()
    for t in range(T_C):
        n_t = num if t == 0 else steps_run["rec"][t - 1]["n"]
        rows = torch.from_numpy(np.flatnonzero(n_t <= 3)).to(obs.device)
        skipped[t].view(E_C, 12, 86)[rows, 3] = 0.0
    hs = skipped.double().cpu().reshape(-1, critic.dims[0])
    for i, (w, bias) in enumerate(zip(critic.weights, critic.biases)):
        hs = hs @ w.double().cpu().t() + bias.double().cpu()
        if i < len(critic.weights) - 1:
            hs = torch.tanh(hs)
    assert not torch.allclose(got, hs, rtol=2e-5, atol=2e-5)


def test_ring_holds_raw_returns_under_a_normaliser(steps_run):
    from cattleherd.train_log import EpisodeRing
    b, actor, critic, rb, n, log_std = _setup()
    n.norm_obs, n.norm_reward, n.training = False, False, False   # the same actions as without a normaliser ...
    ring = EpisodeRing(b, window=512).begin()
    rb.collect(actor, critic, log_std, seed=9, ring=ring, normalizer=n)
    b.close()
    b2, actor, critic, rb2, _, log_std = _setup()
    ring2 = EpisodeRing(b2, window=512).begin()
    rb2.collect(actor, critic, log_std, seed=9, ring=ring2)
    # the same episodes; the returns to the last bits of the float32 actions (the dense forward adds the zero features'
    # products the live-width forward of the plain collection leaves out, so an action may differ in its last bit)
    got, want = ring.entries(), ring2.entries()
    assert len(got) == len(want) > 0
    for (r1, l1, e1), (r2, l2, e2) in zip(got, want):
        assert (l1, e1) == (l2, e2) and abs(r1 - r2) <= 1e-6 * max(1.0, abs(r2))
    b2.close()
    # ... and with one: the ring's returns are the sums of the raw rewards the loop recorded, not of the normalised ones
    rec = steps_run["rec"]
    acc = np.zeros(E_C)
    want = []
    for r in rec:
        acc += r["reward"].astype(np.float64)
        for e in np.flatnonzero(r["reset"]):
            want.append((e, acc[e]))
            acc[e] = 0.0
    got = steps_run["ring"]
    assert len(got) == len(want) > 0
    first = {}
    for (ret, length, env), (e, s) in zip(got, want):
        assert env == e
        if e not in first:   # the env's first episode began at the reset: its whole return was recorded
            first[e] = True
            assert length <= T_C and abs(ret - s) <= 1e-6 * max(1.0, abs(s))


def test_training_off_freezes_the_statistics():
    b, actor, critic, rb, n, log_std = _setup()
    rb.collect(actor, critic, log_std, seed=9, normalizer=n)
    n.training = False
    before = n._block.cpu().numpy().copy()
    D = n.dim
    rb.collect(actor, critic, log_std, seed=10, normalizer=n)
    after = n._block.cpu().numpy()
    assert np.array_equal(before[:2 * D + 4].view(np.int64), after[:2 * D + 4].view(np.int64))
    b.close()


def test_norm_reward_off_keeps_raw_rewards():
    b, actor, critic, rb, n, log_std = _setup(norm_reward=False)
    rec = []
    rb.collect_steps(actor, critic, log_std, seed=9, normalizer=n,
                     on_step=lambda t: rec.append((b.reward.view(E_C).clone(), b.terminated.view(E_C).clone(),
                                                   b.truncated.view(E_C).clone())))
    got = rb.rewards.cpu().numpy()
    for t, (rew, te, tr) in enumerate(rec):
        boot = ((tr == 1) & (te == 0)).cpu().numpy()
        assert np.array_equal(got[t][~boot].view(np.int32), rew.cpu().numpy()[~boot].view(np.int32))
    mean, var, count = n.ret_rms
    assert count == 1e-4 + T_C * E_C and var != 1.0
    b.close()


def test_rejections_on_a_device():
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.rollout import _bind
    from cattleherd.vec_normalize import DeviceNormalizer, DeviceVecNormalize
    b, actor, critic, rb, n, log_std = _setup()
    other = HerdBatch(8, 4, 16, mode="ctde")
    n_other = DeviceVecNormalize(other)
    for fn in (rb.collect, rb.collect_steps):
        with pytest.raises(ValueError, match="another batch"):
            fn(actor, critic, log_std, normalizer=n_other)
        with pytest.raises(ValueError, match="fused"):
            fn(actor, None, log_std, normalizer=n)
    m = HerdBatch(8, 4, 16, mode="marl")
    with pytest.raises(ValueError, match="CTDE"):
        DeviceVecNormalize(m)
    # the C ABI itself: a MARL handle, a wrong dim, a NULL normaliser, NULL arrays
    L = _bind()
    from cattleherd.rollout import ChRolloutIO
    io = ChRolloutIO()
    io.step = ctypes.pointer(b._io)
    b._io.terminal_obs = b.terminal_obs.data_ptr()
    io.mean, io.value, io.terminal_value = rb.mean.data_ptr(), rb.value.data_ptr(), rb.terminal_value.data_ptr()
    io.env_actions = rb.env_actions.data_ptr()
    actor._ensure_packed()
    critic._ensure_packed()

    def call(handle, norm):
        return L.ch_rollout_collect_norm(handle, ctypes.byref(rb._rb), ctypes.byref(io), ctypes.byref(actor._net),
                                         ctypes.byref(critic._net), log_std.data_ptr(), 0, 0.99, 0.95, 1, None,
                                         None if norm is None else ctypes.byref(norm), b._stream())
    assert call(m.handle, n._n) == _lib.CH_ERR_UNSUPPORTED and b"CTDE" in L.ch_last_error(m.handle)
    assert call(b.handle, None) == _lib.CH_ERR_INVALID and b"NULL normaliser" in L.ch_last_error(b.handle)
    wrong = DeviceNormalizer(b.device, 86, E_C)
    assert call(b.handle, wrong._n) == _lib.CH_ERR_INVALID and b"obs_rows * 86" in L.ch_last_error(b.handle)
    assert call(b.handle, n_other._n) == _lib.CH_ERR_INVALID and b"n_envs" in L.ch_last_error(b.handle)
    keep = n._n.var
    n._n.var = None
    assert call(b.handle, n._n) == _lib.CH_ERR_INVALID and b"statistic array" in L.ch_last_error(b.handle)
    n._n.var = keep
    keep = n._n.obs_n
    n._n.obs_n = None
    assert call(b.handle, n._n) == _lib.CH_ERR_INVALID and b"obs_n" in L.ch_last_error(b.handle)
    n._n.obs_n = keep
    x = torch.zeros((4, n.dim), dtype=torch.float32, device=b.device)
    assert L.ch_norm_obs_update(ctypes.byref(n._n), None, 4, None) == _lib.CH_ERR_INVALID
    assert L.ch_norm_obs_apply(ctypes.byref(n._n), x.data_ptr(), 4, None, None, None) == _lib.CH_ERR_INVALID
    with pytest.raises(ValueError):
        n.update_obs(x.double())
    for h in (b, other, m):
        h.close()


def test_one_native_training_iteration_under_a_normaliser():
    import torch
    from cattleherd.env import HerdBatch
    from cattleherd.ppo import PPOUpdate, SB3ActorCritic
    from cattleherd.rollout import DeviceRolloutBuffer
    from cattleherd.vec_normalize import DeviceVecNormalize
    b = HerdBatch(64, 2, 8, mode="ctde", compat=False)
    b.reset()
    model = SB3ActorCritic(obs_dim=b.obs_rows * 86, act_dim=48, device=b.device, seed=0)
    actor, critic, log_std = model.device_nets()
    n = DeviceVecNormalize(b)
    n.reset_obs()
    rb = DeviceRolloutBuffer(b, 8, act_dim=48)
    rb.collect(actor, critic, log_std, seed=1, normalizer=n)
    assert torch.isfinite(rb.obs).all() and float(rb.obs.abs().max()) <= 10.0 and torch.isfinite(rb.returns).all()
    before = [p.detach().clone() for p in model.parameters()]
    upd = PPOUpdate(model, batch_size=64, n_epochs=1, seed=5, backend="native", log_stats=True)
    assert upd.train(rb) == 8
    torch.cuda.synchronize()
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert np.isfinite(upd.last_stats).all()
    b.close()
