"""CPU-only checks of the rollout references (tests/rollout_ref.py), so that the GPU tests that pin the PPO
collection kernels to them (tests/test_gpu_rollout_kernels.py, tests/test_gpu_marl_rollout.py) compare with
something that is itself pinned: Philox4x32-10 to Random123's known answers, the Box-Muller edge seeds, the float32
GAE restatement to fp64 within a bound derived from its roundings and, bit for bit, to the recursion the existing
T = 40 test uses, and a census of the synthetic inputs (a case that misses a floor is fixed in the generator)."""
import numpy as np
import pytest

import rollout_ref as R


def _hex(words):
    return " ".join(format(int(w), "08x") for w in words)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    """Random123's philox4x32_10 vectors (kat_vectors)."""
    assert _hex(R.philox4x32_10(counter, key)) == want


def test_philox_is_vectorised_and_masks_to_32_bits():
    c = np.array([[0, 0xFFFFFFFF, 0x243F6A88]], np.uint64).T + np.zeros((1, 2), np.uint64)   # [3, 2]
    out = R.philox4x32_10((c, [[0], [0xFFFFFFFF], [0x85A308D3]], [[0], [0xFFFFFFFF], [0x13198A2E]],
                           [[0], [0xFFFFFFFF], [0x03707344]]),
                          ([[0], [0xFFFFFFFF], [0xA4093822]], [[0], [0xFFFFFFFF], [0x299F31D0]]))
    assert all(o.shape == (3, 2) and o.dtype == np.uint64 and int(o.max()) <= 0xFFFFFFFF for o in out)
    assert _hex(o[0, 1] for o in out) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(o[2, 0] for o in out) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # words above 32 bits are masked, not carried into the product
    assert _hex(R.philox4x32_10((2 ** 32, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_eps_ref_uses_every_counter_and_key_word():
    """The draws of (t, k, row_lo, row_hi) and (seed_lo, seed_hi) are all different from one another: a reference
    that dropped or swapped a word would not be."""
    base = dict(seed=5, t=1, k=2, row=3)
    seen = {float(R.eps_ref(**base))}
    for kw in (dict(seed=5 + 2 ** 32), dict(seed=6), dict(t=2), dict(k=1), dict(row=2), dict(row=3 + 2 ** 32),
               dict(t=2, k=1), dict(k=3, row=2), dict(t=3, row=1)):
        seen.add(float(R.eps_ref(**{**base, **kw})))
    assert len(seen) == 10
    g = R.eps_grid(7, 1, 6, 5)
    assert g.shape == (6, 5) and g[4, 3] == R.eps_ref(7, 1, 3, 4) and len(np.unique(g)) == 30


def test_box_muller_edge_seeds():
    u1, _ = R.uniforms_ref(R.SEED_U1_ONE, 0, 0, 0)
    assert u1 == 1.0 and R.eps_ref(R.SEED_U1_ONE, 0, 0, 0) == 0.0
    u1, _ = R.uniforms_ref(R.SEED_U1_MIN, 0, 0, 0)
    assert u1 == 2.0 ** -24
    assert abs(R.eps_ref(R.SEED_U1_MIN, 0, 0, 0) - 3.0381764) < 1e-7
    # the uniforms are exact float32 values, so the device's float32 u1 and u2 equal these
    for s in R.SEEDS:
        for u in R.uniforms_ref(s, 2, np.arange(7)[None, :], np.arange(9)[:, None]):
            assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
            assert u.min() >= 0.0 and u.max() <= 1.0


def test_sample_and_logprob_refs_match_torch_normal():
    import torch
    rng = np.random.default_rng(3)
    mu, ls, eps = rng.standard_normal((5, 7)), rng.uniform(-2, 0.5, 7), rng.standard_normal((5, 7))
    a = R.sample_ref(mu, ls, eps).astype(np.float32)
    want = torch.distributions.Normal(torch.tensor(mu), torch.tensor(np.exp(ls))).log_prob(torch.tensor(a).double())
    assert np.allclose(R.logprob_terms_ref(a, mu, ls), want.numpy(), rtol=1e-12, atol=1e-12)


def test_post_ref_truth_table():
    r = np.array([1.5, 1.5, 1.5, 1.5, 1.5], np.float32)
    te = np.array([0, 1, 0, 255, 0], np.uint8)
    tr = np.array([0, 0, 2, 1, 255], np.uint8)
    tv = np.array([2.0, 2.0, 2.0, 2.0, -4.0], np.float32)
    out, les, boot = R.post_ref(r, te, tr, tv, 0.5)
    assert out.dtype == np.float32 and out.tolist() == [1.5, 1.5, 2.5, 1.5, -0.5]
    assert les.tolist() == [0, 1, 1, 1, 1] and boot.tolist() == [False, False, True, False, True]
    out, les, boot = R.post_ref(r, te, tr, None, 0.5)
    assert out.tolist() == [1.5] * 5 and les.tolist() == [0, 1, 1, 1, 1] and not boot.any()


def _gae_f32_bound(d, gamma, lam):
    """First-order bound of |gae_f32 - gae_f64|, from the float32 roundings of one step (u = 2^-24 each, relative to
    the operation's result; the multiplies by nnt in {0, 1} are exact): g nv, r + ., . - v, (gl nnt) last with gl
    itself rounded once, delta + ., and for the returns last + v; the previous step's error enters times gl nnt.
    Second-order terms are covered by the factor 1.01."""
    r, v, es, les, lv = (np.asarray(x, np.float64) for x in R.gae_args(d))
    g, gl = R._g_gl(gamma, lam, np.float64)
    T = r.shape[0]
    last, B = np.zeros_like(lv), np.zeros_like(lv)
    nnt, nv = 1.0 - les, lv
    Ba, Br = np.empty_like(r), np.empty_like(r)
    with np.errstate(invalid="ignore"):
        for s in reversed(range(T)):
            p = g * nv * nnt
            sm = r[s] + p
            delta = sm - v[s]
            q = gl * nnt * last
            last = delta + q
            B = gl * nnt * B + R.U * (np.abs(p) + np.abs(sm) + np.abs(delta) + 2.0 * np.abs(q) + np.abs(last))
            Ba[s] = B
            Br[s] = B + R.U * np.abs(last + v[s])
            nnt, nv = 1.0 - es[s], v[s]
    return 1.01 * Ba, 1.01 * Br


def test_gae_f32_against_fp64_on_the_gpu_tests_inputs():
    """What gae_f32 needs against gae_f64 on every case of the GPU test stays inside the bound its roundings give, so
    the GPU test's fp64 bar (twice that need) is bounded by reasoning."""
    worst = {}
    for T, E in R.gae_cases():
        d = R.gae_inputs(T, E)
        for gamma, lam in R.GAE_PARAMS:
            a32, r32 = R.gae_f32(*R.gae_args(d), gamma, lam)
            bar, a64, r64 = R.gae_f64_bar(d, gamma, lam)
            Ba, Br = _gae_f32_bound(d, gamma, lam)
            ok = np.isfinite(a64)
            assert np.array_equal(np.isnan(a32), ~ok) and np.array_equal(np.isnan(r32), ~ok)
            assert np.all(np.abs(a32 - a64)[ok] <= Ba[ok]) and np.all(np.abs(r32 - r64)[ok] <= Br[ok])
            assert 0.0 < bar <= 2.0 * float(Br[ok].max())
            worst[(gamma, lam, T, E)] = bar
    top = max(worst, key=worst.get)
    print("fp64 bars: worst", top, worst[top])
    # With episode starts at 0.3 per step a trajectory is a few steps long whatever T is, so the need does not grow
    # with T or with gamma = lambda = 1: every case is a few tens of ulp of O(1) sums (3.3e-6 at most)
    assert worst[top] < 1e-5


def test_gae_f32_equals_the_existing_numpy_form_bit_for_bit():
    """The recursion test_gpu_rollout.py compares the T = 40 collection with (SB3's NumPy expression with Python-float
    gamma and lambda) and gae_f32 are the same float32 computation."""
    from test_gpu_rollout import _gae_numpy
    for T, E in R.gae_cases():
        d = R.gae_inputs(T, E)
        for gamma, lam in R.GAE_PARAMS:
            a, r = R.gae_f32(*R.gae_args(d), gamma, lam)
            with np.errstate(invalid="ignore"):
                a0, r0 = _gae_numpy(d["rewards"], d["values"], d["episode_starts"], d["last_value"], d["last_es"],
                                    gamma, lam)
            assert a0.dtype == np.float32 and R.bits_equal(a, a0) and R.bits_equal(r, r0)


def test_gae_marl_f32_and_f64_agree_and_mask():
    rng = np.random.default_rng(5)
    T, rows = 33, 40
    rew, val = rng.standard_normal((T, rows)).astype(np.float32), rng.standard_normal((T, rows)).astype(np.float32)
    mask = (rng.random((T, rows)) < 0.8).astype(np.uint8)
    term = ((rng.random((T, rows)) < 0.1) * 255).astype(np.uint8)
    lv = rng.standard_normal(rows).astype(np.float32)
    a32, r32 = R.gae_marl_f32(rew, val, mask, term, lv, 0.97, 0.9)
    a64, r64 = R.gae_marl_f64(rew, val, mask, term, lv, 0.97, 0.9)
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    assert np.all(a32[mask == 0] == 0) and np.all(r32[mask == 0] == 0)
    assert 0.0 < R.max_err(a32, a64) < 1e-5 and R.max_err(r32, r64) < 1e-5
    # a terminated step cuts the trajectory: its advantage is r - v alone
    cut = (mask != 0) & (term != 0)
    assert cut.any() and np.array_equal(a32[cut], (rew - val)[cut])


def test_census_of_the_synthetic_inputs():
    p = R.post_inputs()
    te, tr = p["te"] != 0, p["tr"] != 0
    for a in (False, True):
        for b in (False, True):
            assert ((te == a) & (tr == b)).sum() >= 60
    assert set(p["te"].tolist()) == set(R.POST_FLAG_BYTES) and set(p["tr"].tolist()) == set(R.POST_FLAG_BYTES)
    assert len(p["te"]) == 257 and np.isfinite(p["reward"]).all() and np.isfinite(p["tv"]).all()
    assert R.gae_chunks(33) == [(17, 33), (1, 17), (0, 1)] and R.gae_chunks(16) == [(0, 16)]
    assert sorted(set(R.gae_cases())) == sorted(set([(T, 130) for T in (1, 2, 15, 16, 17, 32, 33)] +
                                                    [(17, E) for E in (1, 63, 64, 65)]))
    for T, E in R.gae_cases():
        d = R.gae_inputs(T, E)
        es = d["episode_starts"]
        assert set(np.unique(es)) <= {0.0, 1.0} and (0.0 in es or T * E < 4)
        for s0, s1 in R.gae_chunks(T):
            assert es[s0].any() and es[s1 - 1].any()
        assert es[T - 1].any()
        if E > 1:
            assert set(d["last_es"].tolist()) == {0.0, 1.0}
        nan_cols = np.isnan(d["rewards"]).any(0)
        assert nan_cols.sum() == 1 and nan_cols[d["nan_env"]] and np.isnan(d["rewards"]).sum() == 1
        assert np.isfinite(d["values"]).all() and np.isfinite(d["last_value"]).all()
        tiny = np.finfo(np.float32).tiny
        for k in ("rewards", "values", "last_value"):
            x = d[k][np.isfinite(d[k])]
            assert np.all((x == 0) | (np.abs(x) >= tiny))
        # the NaN stays in its column: steps up to the NaN's, nothing else
        a, r = R.gae_f32(*R.gae_args(d), 0.99, 0.95)
        want = np.zeros((T, E), bool)
        want[:d["nan_step"] + 1, d["nan_env"]] = True
        assert np.array_equal(np.isnan(a), want) and np.array_equal(np.isnan(r), want)
