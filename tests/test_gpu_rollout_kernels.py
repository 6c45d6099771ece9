"""GPU tests of the three public CTDE rollout entry points on synthetic device buffers: ch_rollout_store
(k_rollout_store / rollout_sample), ch_rollout_post (k_rollout_post / rollout_post_env) and ch_rollout_gae
(k_rollout_gae), each against the plain NumPy references of tests/rollout_ref.py (kept honest on the CPU by
tests/test_rollout_ref_cpu.py).  The handles are HerdBatch(E, 2, 8, "ctde"): they only supply rows = E and the env's
action width 8, no env step runs.  Every buffer is allocated here, filled with a sentinel and followed by a guard
tail, so a write outside the addressed row shows.

What is exact: the Philox4x32-10 counter (t, k, row_lo, row_hi) and key (seed_lo, seed_hi) (through the recovered
noise), the clipped env actions, the copied rows, the post's truth table and flags, and the GAE recursion bit for bit
(gae_f32).  What has a bar, derived in rollout_ref (action_bar, logprob_bar, gae_f64_bar) and not from the device:
the samples and log-probabilities (logf / cosf / sqrtf / expf on the device, fp64 in the reference), the bootstrapped
reward (1 float32 ulp: the reference rounds twice, the kernel's fmaf once), GAE against fp64.

Measured on an MI355X, worst ratio of error to bar over all cases (each test prints its own): actions 0.133
(E = 130, A = 256), log-probabilities 0.138 (E = 130, A = 8), bootstrapped rewards 0 ulp of the 1 allowed, GAE
against fp64 0.500 in every case (the device equals gae_f32 bit for bit and the bar is twice gae_f32's own error)."""
import ctypes

import numpy as np
import pytest

import rollout_ref as R

pytestmark = pytest.mark.gpu

SENT = -12345.678      # the sentinel every buffer starts with (its float32 rounding)
GUARD = 64             # floats after every buffer
OBS_DIM = 12 * 86
ENV_A = 8              # 2 drones x 4
NAMES = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns",
         "last_episode_starts")


class _Bufs:
    """A rollout buffer and the store's env_actions, each a flat sentinel-filled tensor with a guard tail."""

    def __init__(self, b, T, A):
        import torch
        from cattleherd.rollout import ChRollout, _bind
        E = b.n_envs
        self.torch, self.b, self.T, self.E, self.A = torch, b, T, E, A
        shapes = {"obs": (T, E, OBS_DIM), "actions": (T, E, A), "last_episode_starts": (E,), "env_actions": (E, ENV_A)}
        self.flat, self.view = {}, {}
        for k in NAMES + ("env_actions",):
            shape = shapes.get(k, (T, E))
            n = int(np.prod(shape))
            self.flat[k] = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=b.device)
            self.view[k] = self.flat[k][:n].view(shape)
        self.rb = ChRollout()
        self.rb.n_steps, self.rb.act_dim = T, A
        for k in NAMES:
            setattr(self.rb, k, self.view[k].data_ptr())
        self.lib = _bind()

    def __getitem__(self, k):
        return self.view[k]

    def dev(self, x, dtype=None):
        return self.torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(self.b.device).contiguous()

    def untouched(self, written):
        """Every guard tail, every buffer not in `written`, and every row of a [T, ...] buffer other than
        written[name] (a step index; None: the whole buffer may be written) still hold the sentinel."""
        s = self.torch.tensor(SENT, dtype=self.torch.float32, device=self.b.device)
        for k, f in self.flat.items():
            assert bool((f[-GUARD:] == s).all()), f"guard tail of {k}"
            if k not in written:
                assert bool((f == s).all()), k
            elif written[k] is not None:
                rows = [i for i in range(self.T) if i != written[k]]
                assert bool((self.view[k][rows] == s).all()), f"rows of {k} other than {written[k]}"


def _batch(E):
    from cattleherd.env import HerdBatch
    return HerdBatch(E, 2, 8, mode="ctde")


def _check(rc, b):
    from cattleherd import _lib
    _lib.check(rc, b.handle)


def _store(bufs, t, obs, mean, value, log_std, seed):
    b = bufs.b
    _check(bufs.lib.ch_rollout_store(b.handle, ctypes.byref(bufs.rb), t, obs.data_ptr(), mean.data_ptr(),
                                     value.data_ptr(), log_std.data_ptr(), int(seed),
                                     bufs["env_actions"].data_ptr(), b._stream()), b)
    bufs.torch.cuda.synchronize()


def _check_store(bufs, t, seed, obs, mean, value, log_std, les, ratios):
    """One ch_rollout_store call on fresh sentinel buffers against the references."""
    torch, E, A = bufs.torch, bufs.E, bufs.A
    for f in bufs.flat.values():
        f.fill_(SENT)
    bufs["last_episode_starts"].copy_(bufs.dev(les))
    d_obs, d_mean, d_value, d_ls = bufs.dev(obs), bufs.dev(mean), bufs.dev(value), bufs.dev(log_std)
    _store(bufs, t, d_obs, d_mean, d_value, d_ls, seed)
    act = bufs["actions"][t].cpu().numpy()
    eps = R.eps_grid(seed, t, E, A)
    mu, ls = mean.astype(np.float64), log_std.astype(np.float64)[None, :]
    ra = np.abs(act - R.sample_ref(mu, ls, eps)) / R.action_bar(mu, ls, eps)
    lp = bufs["log_probs"][t].cpu().numpy()
    want_lp = np.cumsum(R.logprob_terms_ref(act, mu, ls), axis=-1)[:, -1]      # summed in action order
    rl = np.abs(lp - want_lp) / R.logprob_bar(act, mu, ls)
    ratios["action"] = max(ratios.get("action", 0.0), float(ra.max()))
    ratios["log_prob"] = max(ratios.get("log_prob", 0.0), float(rl.max()))
    assert np.isfinite(act).all() and ra.max() <= 1.0, (t, seed, float(ra.max()), np.unravel_index(ra.argmax(), ra.shape))
    assert np.isfinite(lp).all() and rl.max() <= 1.0, (t, seed, float(rl.max()), int(rl.argmax()))
    env = bufs["env_actions"]
    assert torch.equal(env, bufs["actions"][t][:, :ENV_A].clamp(-1.0, 1.0))
    assert float(env.min()) >= -1.0 and float(env.max()) <= 1.0
    assert torch.equal(bufs["obs"][t], d_obs) and torch.equal(bufs["values"][t], d_value[:, 0])
    assert torch.equal(bufs["episode_starts"][t], bufs["last_episode_starts"])
    assert torch.equal(bufs["last_episode_starts"], bufs.dev(les))
    bufs.untouched({"obs": t, "actions": t, "log_probs": t, "values": t, "episode_starts": t,
                    "env_actions": None, "last_episode_starts": None})
    return act


def _store_inputs(E, A, seed):
    rng = np.random.default_rng(seed)
    return dict(obs=rng.standard_normal((E, OBS_DIM)).astype(np.float32),
                mean=rng.standard_normal((E, A)).astype(np.float32),
                value=rng.standard_normal((E, 1)).astype(np.float32),
                log_std=rng.uniform(-2.0, 0.5, A).astype(np.float32),
                les=(rng.random(E) < 0.5).astype(np.float32))


@pytest.mark.parametrize("A", [8, 48, 65, 256])
@pytest.mark.parametrize("E", [1, 5, 130])
def test_store_matches_the_references(E, A):
    """ch_rollout_store at row counts that leave the last workgroup of 4 envs partial (1, 5, 130) and action widths
    of one lane pass, a partial pass, two passes and the whole 256-wide LDS row, at the first and last step and three
    seeds (low word only, both words, all ones): the samples and log-probabilities within their bars of the fp64
    references with the documented Philox counter and key, everything else exact, nothing else written.  With
    mean = 0 and log_std = 0 the stored action is the device's noise itself."""
    T = 3
    b = _batch(E)
    bufs = _Bufs(b, T, A)
    ratios = {}
    x = _store_inputs(E, A, 100 * E + A)
    for t in (0, T - 1):
        for seed in R.SEEDS:
            _check_store(bufs, t, seed, ratios=ratios, **x)
    zero = dict(x, mean=np.zeros((E, A), np.float32), log_std=np.zeros(A, np.float32))
    act = _check_store(bufs, T - 1, R.SEEDS[1], ratios=ratios, **zero)
    eps = R.eps_grid(R.SEEDS[1], T - 1, E, A)
    assert np.all(np.abs(act - eps) <= 1e-5 + 4 * R.U * np.abs(eps))
    print(f"store E={E} A={A} worst ratios {ratios}")
    b.close()


@pytest.mark.parametrize("seed,want", [(R.SEED_U1_ONE, 0.0), (R.SEED_U1_MIN, 3.0381764)], ids=["u1_one", "u1_min"])
def test_store_box_muller_edges(seed, want):
    """The two ends of u1 at counter (0, 0, 0, 0): u1 == 1 gives log 1 = 0 and eps == 0 exactly; u1 == 2^-24 gives
    the largest amplitude the sampler can produce, within the action bar."""
    b = _batch(1)
    bufs = _Bufs(b, 3, ENV_A)
    ratios = {}
    x = _store_inputs(1, ENV_A, 9)
    zero = dict(x, mean=np.zeros((1, ENV_A), np.float32), log_std=np.zeros(ENV_A, np.float32))
    act = _check_store(bufs, 0, seed, ratios=ratios, **zero)
    eps = float(R.eps_ref(seed, 0, 0, 0))
    assert abs(eps - want) < 1e-7
    if want == 0.0:
        assert act[0, 0] == 0.0
    else:
        assert abs(float(act[0, 0]) - eps) <= 1e-5 + 4 * R.U * abs(eps)
    _check_store(bufs, 0, seed, ratios=ratios, **x)
    print(f"store edge seed {seed} worst ratios {ratios}")
    b.close()


@pytest.mark.parametrize("gamma", [0.99, 0.5])
@pytest.mark.parametrize("with_tv", [True, False], ids=["tv", "tv_null"])
@pytest.mark.parametrize("t", [0, 2])
def test_post_truth_table(t, with_tv, gamma):
    """ch_rollout_post over 257 envs (a second workgroup of one env): every (terminated, truncated) combination with
    flag bytes from {0, 1, 2, 255}, terminal_value given or NULL.  The reward is bootstrapped only where truncated,
    not terminated and terminal_value is given (1 ulp: post_ref rounds twice), copied bit for bit elsewhere; the next
    episode start is exactly te | tr; nothing else is written."""
    T = 3
    p = R.post_inputs()
    E = len(p["reward"])
    b = _batch(E)
    bufs = _Bufs(b, T, ENV_A)
    torch = bufs.torch
    rew, te, tr, tv = bufs.dev(p["reward"]), bufs.dev(p["te"]), bufs.dev(p["tr"]), bufs.dev(p["tv"])
    assert te.dtype == torch.uint8 and tr.dtype == torch.uint8
    _check(bufs.lib.ch_rollout_post(b.handle, ctypes.byref(bufs.rb), t, rew.data_ptr(), te.data_ptr(), tr.data_ptr(),
                                    tv.data_ptr() if with_tv else None, gamma, b._stream()), b)
    torch.cuda.synchronize()
    want, les, boot = R.post_ref(p["reward"], p["te"], p["tr"], p["tv"] if with_tv else None, gamma)
    got = bufs["rewards"][t].cpu().numpy()
    assert boot.sum() == (64 if with_tv else 0)
    assert np.array_equal(got[~boot].view(np.uint32), p["reward"][~boot].view(np.uint32))
    ulps = R.ulp_diff(got[boot], want[boot]) if boot.any() else np.zeros(1, np.int64)
    print(f"post t={t} tv={with_tv} gamma={gamma}: worst bootstrapped reward error {int(ulps.max())} ulp (bar 1)")
    assert ulps.max() <= 1
    if with_tv:   # the bootstrap did happen: the exact gamma tv + r differs from r by far more than an ulp
        assert np.all(got[boot] != p["reward"][boot])
    assert np.array_equal(bufs["last_episode_starts"].cpu().numpy(), les)
    bufs.untouched({"rewards": t, "last_episode_starts": None})
    b.close()


@pytest.mark.parametrize("T,E", R.gae_cases())
def test_gae_is_the_float32_recursion_bit_for_bit(T, E):
    """ch_rollout_gae at buffer lengths around the 16-step chunk (1, 2, 15, 16, 17, 32, 33) and row counts around the
    64-env workgroup (1, 63, 64, 65, 130), four (gamma, lambda) pairs: advantages and returns equal gae_f32 bit for bit
    (NaN where it is NaN: one env has a NaN reward in mid-buffer and it stays in that column), and lie within the
    fp64 bar of gae_f64 where that is finite; the inputs are not written."""
    b = _batch(E)
    bufs = _Bufs(b, T, ENV_A)
    torch = bufs.torch
    d = R.gae_inputs(T, E)
    worst = 0.0
    for gamma, lam in R.GAE_PARAMS:
        for f in bufs.flat.values():
            f.fill_(SENT)
        for k, src in (("rewards", "rewards"), ("values", "values"), ("episode_starts", "episode_starts"),
                       ("last_episode_starts", "last_es")):
            bufs[k].copy_(bufs.dev(d[src]))
        lv = bufs.dev(d["last_value"])
        _check(bufs.lib.ch_rollout_gae(b.handle, ctypes.byref(bufs.rb), lv.data_ptr(), gamma, lam, b._stream()), b)
        torch.cuda.synchronize()
        adv, ret = bufs["advantages"].cpu().numpy(), bufs["returns"].cpu().numpy()
        a32, r32 = R.gae_f32(*R.gae_args(d), gamma, lam)
        assert R.bits_equal(adv, a32), (gamma, lam, R.max_err(adv, a32))
        assert R.bits_equal(ret, r32), (gamma, lam, R.max_err(ret, r32))
        bar, a64, r64 = R.gae_f64_bar(d, gamma, lam)
        err = max(R.max_err(adv, a64), R.max_err(ret, r64))
        worst = max(worst, err / bar)
        assert err <= bar, (gamma, lam, err, bar)
        nan = np.zeros((T, E), bool)
        nan[:d["nan_step"] + 1, d["nan_env"]] = True
        assert np.array_equal(np.isnan(adv), nan) and np.array_equal(np.isnan(ret), nan)
        for k, src in (("rewards", "rewards"), ("values", "values"), ("episode_starts", "episode_starts"),
                       ("last_episode_starts", "last_es")):
            assert R.bits_equal(bufs[k].cpu().numpy(), d[src]), k
        bufs.untouched({k: None for k in ("rewards", "values", "episode_starts", "last_episode_starts", "advantages",
                                          "returns")})
    print(f"gae T={T} E={E} worst ratio to the fp64 bar {worst:.3f}")
    b.close()
