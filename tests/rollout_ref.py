"""Plain NumPy references of the PPO collection kernels (csrc/ch_rollout_dev.h rollout_sample / rollout_post_env,
csrc/ch_aux.hip k_rollout_store / k_rollout_post / k_rollout_gae / k_marl_store / k_marl_gae), and the synthetic
inputs the GPU tests feed them (tests/test_gpu_rollout_kernels.py, tests/test_gpu_marl_rollout.py).  A helper module
like directed_states.py; tests/test_rollout_ref_cpu.py keeps it honest without a GPU.

Two kinds of reference:

* exact ones, whose result the device must reproduce bit for bit: the Philox4x32-10 words and the uniforms made from
  them (integers and exact float32 values), the float32 GAE recursions in the kernels' association (the kernels hold
  only IEEE float32 adds and multiplies and the library is built with -ffp-contract=off), the post's flags;
* fp64 ones, for what the device computes with logf / cosf / sqrtf / expf: the Box-Muller normal, the sample and the
  log-probability terms.  Their bars (action_bar, logprob_bar) are derived from the float32 chain, not measured.

gamma and lambda cross the C ABI as float32, so every reference rounds them to float32 first; gamma * lambda is the
float32 rounding of the fp64 product of those two, as ch_rollout_gae computes it."""
import numpy as np

U = 2.0 ** -24            # float32 unit roundoff
M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)
SEEDS = (0, 2 ** 32 + 5, 2 ** 64 - 1)
# Box-Muller edge seeds at counter (0, 0, 0, 0), found by a CPU search over seeds (asserted in the CPU test)
SEED_U1_ONE = 16390493      # u1 == 1.0: eps == 0
SEED_U1_MIN = 12121362      # u1 == 2^-24: the largest amplitude, eps ~ 3.0381764


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123): counter = 4 and key = 2 array-likes of 32-bit words (broadcast
    against each other); returns the 4 output words as uint64 arrays, in the order philox_k leaves them in c[0..3]."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & M32 for x in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniforms_ref(seed, t, k, row):
    """(u1, u2) of rollout_sample as fp64: u1 in (0, 1], u2 in [0, 1), both multiples of 2^-24 (exact in float32)."""
    seed = int(seed) & (2 ** 64 - 1)
    row = np.asarray(row, dtype=np.uint64)
    c = philox4x32_10((t, k, row & M32, row >> np.uint64(32)), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((c[0] >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0 ** 24
    u2 = (c[1] >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    return u1, u2


def eps_ref(seed, t, k, row):
    """The N(0, 1) draw of action k of row `row` at step t, fp64: Box-Muller on Philox4x32-10 with counter
    (t, k, row_lo, row_hi) and key (seed_lo, seed_hi)."""
    u1, u2 = uniforms_ref(seed, t, k, row)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def eps_grid(seed, t, rows, act_dim):
    """eps_ref for every (row, k): [rows, act_dim]."""
    return eps_ref(seed, t, np.arange(act_dim)[None, :], np.arange(rows)[:, None])


def sample_ref(mu, log_std, eps):
    return np.asarray(mu, np.float64) + np.exp(np.asarray(log_std, np.float64)) * eps


def logprob_terms_ref(act, mu, log_std):
    """Normal(mu, exp(log_std)).log_prob(act) per dimension, fp64; `act` is the stored float32 action."""
    a, mu, ls = (np.asarray(x, np.float64) for x in (act, mu, log_std))
    return -(a - mu) ** 2 / (2.0 * np.exp(ls) ** 2) - ls - LOG_SQRT_2PI


def action_bar(mu, log_std, eps):
    """|a_dev - sample_ref| allowed.  The device's eps is a float32 chain: 2 pi rounded once (2.8e-8 relative), the
    product rounded once, cosf / logf / sqrtf good to a few ulp, amplitude at most sqrt(-2 ln 2^-24) = 5.77: about
    6e-6 absolute, taken as 1e-5 (an emulation of the chain in NumPy float32 over 2 M draws measured 1.7e-6).  Then
    expf, one multiply and one add in float32: 4 ulp of the terms' magnitudes."""
    sd = np.exp(np.asarray(log_std, np.float64))
    return sd * 1e-5 + 4.0 * U * (np.abs(mu) + sd * np.abs(eps))


def logprob_bar(act, mu, log_std):
    """|log_prob_dev - sum of logprob_terms_ref| allowed: the sequential float32 sum of A terms, each computed with a
    handful of float32 roundings -- (A + 8) u times the sum of the terms' magnitudes."""
    a, mu, ls = (np.asarray(x, np.float64) for x in (act, mu, log_std))
    q = (a - mu) ** 2 / (2.0 * np.exp(ls) ** 2)
    A = q.shape[-1]
    return (A + 8) * U * (q + np.abs(ls) + LOG_SQRT_2PI).sum(-1)


def post_ref(reward, te, tr, tv, gamma):
    """rollout_post_env: (rewards row float32, next episode start float32).  The bootstrap applies where tr != 0,
    te == 0 and tv is given: fp64 gamma * tv + r rounded once to float32 (the kernel's fmaf rounds the exact value
    once; this one rounds twice, hence the 1 ulp the GPU test allows there).  Returns the bootstrap mask too."""
    reward = np.asarray(reward, np.float32)
    te, tr = np.asarray(te) != 0, np.asarray(tr) != 0
    boot = tr & ~te & (tv is not None)
    out = reward.copy()
    if tv is not None:
        b = np.float64(np.float32(gamma)) * np.asarray(tv, np.float64) + reward.astype(np.float64)
        out[boot] = b.astype(np.float32)[boot]
    return out, (te | tr).astype(np.float32), boot


def _g_gl(gamma, lam, dtype):
    g, l = np.float32(gamma), np.float32(lam)
    gl = np.float64(g) * np.float64(l)
    return dtype(g), dtype(gl)


def _gae(rewards, values, episode_starts, last_es, last_value, gamma, lam, dtype):
    rewards, values, episode_starts = (np.asarray(x).astype(dtype) for x in (rewards, values, episode_starts))
    g, gl = _g_gl(gamma, lam, dtype)
    one = dtype(1.0)
    T = rewards.shape[0]
    adv, ret = np.empty_like(rewards), np.empty_like(rewards)
    last = np.zeros_like(rewards[0])
    nnt, nv = one - np.asarray(last_es).astype(dtype), np.asarray(last_value).astype(dtype)
    with np.errstate(invalid="ignore"):
        for s in reversed(range(T)):
            delta = (rewards[s] + (g * nv) * nnt) - values[s]
            last = delta + (gl * nnt) * last
            adv[s] = last
            ret[s] = last + values[s]
            nnt, nv = one - episode_starts[s], values[s]
    return adv, ret


def gae_f32(rewards, values, episode_starts, last_es, last_value, gamma, lam):
    """k_rollout_gae in NumPy float32, in the kernel's association: delta = (r + (g nv) nnt) - v,
    last = delta + (gl nnt) last, ret = last + v."""
    return _gae(rewards, values, episode_starts, last_es, last_value, gamma, lam, np.float32)


def gae_f64(rewards, values, episode_starts, last_es, last_value, gamma, lam):
    """The same recursion in fp64 (gamma and lambda as the float32 the ABI carries, their product not rounded)."""
    return _gae(rewards, values, episode_starts, last_es, last_value, gamma, lam, np.float64)


def _gae_marl(rew, val, mask, term, last_v, gamma, lam, dtype):
    rew, val = np.asarray(rew).astype(dtype), np.asarray(val).astype(dtype)
    g, gl = _g_gl(gamma, lam, dtype)
    zero, one = dtype(0), dtype(1)
    T = rew.shape[0]
    adv = np.zeros_like(rew)
    last = np.zeros_like(rew[0])
    nv = np.asarray(last_v).astype(dtype).copy()
    with np.errstate(invalid="ignore"):
        for t in reversed(range(T)):
            m = mask[t] != 0
            nnt = np.where(term[t] != 0, zero, one).astype(dtype)
            delta = (rew[t] + (g * nv) * nnt) - val[t]
            cur = delta + (gl * nnt) * last
            adv[t] = np.where(m, cur, zero)
            last = np.where(m, cur, zero).astype(dtype)
            nv = np.where(m, val[t], zero).astype(dtype)
        return adv, np.where(mask != 0, adv + val, zero).astype(dtype)


def gae_marl_f32(rew, val, mask, term, last_v, gamma, lam):
    """k_marl_gae in NumPy float32: per-agent GAE, a trajectory ends where the agent terminates; masked rows are 0."""
    return _gae_marl(rew, val, mask, term, last_v, gamma, lam, np.float32)


def gae_marl_f64(rew, val, mask, term, last_v, gamma, lam):
    return _gae_marl(rew, val, mask, term, last_v, gamma, lam, np.float64)


def max_err(got, want):
    """max |got - want| over the positions where `want` is finite (0 where there are none)."""
    want = np.asarray(want, np.float64)
    ok = np.isfinite(want)
    return float(np.max(np.abs(np.asarray(got, np.float64)[ok] - want[ok]))) if ok.any() else 0.0


def bits_equal(got, want):
    """float32 arrays equal bit for bit where `want` is not NaN, NaN exactly where `want` is (any payload)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and \
        bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def ulp_diff(got, want):
    """|got - want| in float32 units in the last place, by the ordered-integer view (finite inputs)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(got) - key(want))


# ---- synthetic inputs --------------------------------------------------------------------------------------------
GAE_CHUNK = 16          # kGaeChunk / kMarlGaeChunk
GAE_T = (1, 2, 15, 16, 17, 32, 33)
GAE_E = (1, 63, 64, 65)
GAE_E_MAIN, GAE_T_MAIN = 130, 17
GAE_PARAMS = ((0.99, 0.95), (0.9, 0.5), (1.0, 1.0), (0.99, 0.0))


def gae_chunks(T):
    """The [s0, s1) step ranges the GAE kernels load at once, in the order they fold them (from the end)."""
    out, s1 = [], T
    while s1 > 0:
        s0 = max(s1 - GAE_CHUNK, 0)
        out.append((s0, s1))
        s1 = s0
    return out


def gae_cases():
    """(T, E) of the GPU GAE test: every T at E = 130, every E at T = 17."""
    return [(T, GAE_E_MAIN) for T in GAE_T] + [(GAE_T_MAIN, E) for E in GAE_E]


def gae_inputs(T, E, seed=0):
    """Synthetic buffers for ch_rollout_gae: O(1) normal rewards and values (no denormals), Bernoulli(0.3) episode
    starts with a start forced onto the first step of every chunk (env 0) and onto its last step (env 1, or 0 when
    there is one env; the first chunk's last step is T - 1), mixed last_episode_starts, and a NaN reward at step
    T // 2 of env E // 2 (the recursion runs backwards: that column is NaN up to that step and finite after it)."""
    rng = np.random.default_rng(1000 * T + E + seed)
    d = {"rewards": rng.standard_normal((T, E)).astype(np.float32),
         "values": rng.standard_normal((T, E)).astype(np.float32),
         "episode_starts": (rng.random((T, E)) < 0.3).astype(np.float32),
         "last_es": (rng.random(E) < 0.5).astype(np.float32),
         "last_value": rng.standard_normal(E).astype(np.float32)}
    c_first, c_last = 0, min(1, E - 1)
    for s0, s1 in gae_chunks(T):
        d["episode_starts"][s0, c_first] = 1.0
        d["episode_starts"][s1 - 1, c_last] = 1.0
    if E > 1:
        d["last_es"][0], d["last_es"][1] = 0.0, 1.0
    d["nan_env"], d["nan_step"] = E // 2, T // 2
    d["rewards"][d["nan_step"], d["nan_env"]] = np.nan
    return d


def gae_args(d):
    return d["rewards"], d["values"], d["episode_starts"], d["last_es"], d["last_value"]


def gae_f64_bar(d, gamma, lam):
    """The fp64 bar of the GAE tests: twice what the float32 restatement itself needs against fp64 on these inputs
    (bit equality with gae_f32 is the real assertion).  Returns (bar, adv64, ret64)."""
    a32, r32 = gae_f32(*gae_args(d), gamma, lam)
    a64, r64 = gae_f64(*gae_args(d), gamma, lam)
    return 2.0 * max(max_err(a32, a64), max_err(r32, r64)), a64, r64


POST_E = 257
POST_FLAG_BYTES = (0, 1, 2, 255)


def post_inputs(E=POST_E, seed=0):
    """Synthetic step outputs for ch_rollout_post: the flags cycle through the four (te, tr) combinations with the
    set bytes drawn from {1, 2, 255} in turn (so every byte of {0, 1, 2, 255} occurs in both arrays), O(1) rewards and
    terminal values."""
    rng = np.random.default_rng(77 + seed)
    e = np.arange(E)
    nz = np.array(POST_FLAG_BYTES[1:], np.uint8)
    te = np.where(e % 2 == 1, nz[(e // 4) % 3], 0).astype(np.uint8)
    tr = np.where((e // 2) % 2 == 1, nz[(e // 4 + 1) % 3], 0).astype(np.uint8)
    return {"reward": rng.standard_normal(E).astype(np.float32), "te": te, "tr": tr,
            "tv": rng.standard_normal(E).astype(np.float32)}
