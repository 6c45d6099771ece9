"""The pipelined step loop's whole-env cheap pass (alpha_cheap_env: one unit per flocking env, both chunks' loads ahead
of the tests, one queue reservation per env) against the same number of plain ch_step launches, bit for bit: state,
outputs, metrics and the drawn actions.  The plain launch (k_step2) keeps alpha_cheap, so every comparison is the new
pass against the old one.

Geometry: 4 drones x 16 cattle, f64, CTDE, on the (16 envs, 512 threads) geometry the pipelined instantiation runs at;
16 envs (one workgroup), 24 (a second workgroup with 8 of its 16 env slots live), 48; n = 1, 2, 3, 8 steps.

Placements (``_states``), on states the CPU oracle reaches after a reset and two steps.  The cattle are placed at rest,
and the flock parity is chosen so that the plain step after set_state (the one the first-step rule needs) does not run
the flock where a count has to be exact: the first step of the launch then tests the positions exactly as placed.
  parity    every env at the same parity: the launch's steps alternate between 16 flocking envs and none
  full      a 4 x 4 herd 0.25 m apart (diagonal 1.06 m) in every env, same parity: all 120 pairs inside 1.2 m, the
            queue reaches its capacity G * P exactly
  empty     a 4 x 4 herd 1.5 m apart in every env: no pair inside 1.2 m, an empty queue
  boundary  env 3: cow 0 at the origin, cow 1 on the x axis at the largest x with x * x <= kAlphaSupport2, cow 2 on the
            y axis one ulp further out, cow 3 at x = -1.2 (n^2 = 1.2 * 1.2), the other cows 1.5 m apart far away
  reset     mixed parities; envs a few substeps short of the time limit, each at the parity that makes it flock in the
            step it resets in
The cattle move at most 0.2 m/s (1/300 m per step), so the counts of `full` and `empty` hold over the launch.
test_placements_on_oracle checks every count on the CPU oracle alone; the GPU test asserts them again from the plain
handle's states.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import directed_states as D
from helpers import stack

N, M, P = 4, 16, 120
GEOM = (16, 512)
SIZES = (16, 24, 48)
STEPS = (1, 2, 3, 8)
CASES = ("parity", "full", "empty", "boundary", "reset")
K_SUPPORT2 = 1.44 * (1.0 + 1e-9)   # kAlphaSupport2 (csrc/ch_step_flock.h)
E_BOUNDARY = 3
# env slot within each group of 16 -> step of the sequence at which it reaches the time limit (step 0: the plain launch
# after set_state, step j >= 1: step j - 1 of the multi-step launch; "n": the last one)
SCHEDULE = {1: 1, 5: 2, 6: 3, 9: "n", 12: 2}


def _boundary_x():
    """The largest double x with x * x <= kAlphaSupport2 (as the pass computes it: zx * zx + 0), and the next one."""
    x = math.sqrt(K_SUPPORT2)
    while x * x > K_SUPPORT2:
        x = math.nextafter(x, 0.0)
    while math.nextafter(x, math.inf) ** 2 <= K_SUPPORT2:
        x = math.nextafter(x, math.inf)
    return x, math.nextafter(x, math.inf)


def _grid(spacing, origin):
    return np.array([[origin[0] + spacing * (j % 4), origin[1] + spacing * (j // 4)] for j in range(M)], np.float64)


@functools.lru_cache(maxsize=None)
def _base(E):
    import torch  # noqa: F401  (before the library, as HerdBatch loads them: one HIP runtime for both in this process)
    import oracle as O
    from cattleherd._lib import spawn_table
    table = spawn_table(M)
    out = []
    for e in range(E):
        env = O.Env(0, N, M, table, env_id=e)
        env.reset()
        for t in range(2):
            env.step(env.random_actions(t), autoreset=True)
        out.append(env.get_state())
    return table, out


def _states(case, E, n):
    """(oracle envs at the placed states, the states)."""
    import oracle as O
    table, base = _base(E)
    envs, states = [], []
    x_in, x_out = _boundary_x()
    for e in range(E):
        s = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in base[e].items()}
        centre = np.asarray(s["cow_pos"])[:M].mean(axis=0)
        par = 0   # even step_counter_A: the plain step does not flock, the launch's first step does
        if case == "full":
            s["cow_pos"][:M] = _grid(0.25, centre - 0.375)
        elif case == "empty":
            s["cow_pos"][:M] = _grid(1.5, centre - 2.25)
        elif case == "boundary" and e == E_BOUNDARY:
            s["cow_pos"][:M] = _grid(1.5, (5.0, 5.0))
            s["cow_pos"][0] = (0.0, 0.0)
            s["cow_pos"][1] = (x_in, 0.0)
            s["cow_pos"][2] = (0.0, x_out)
            s["cow_pos"][3] = (-1.2, 0.0)
        elif case == "reset":
            par = (e * 5 // 3) % 2
            k = SCHEDULE.get(e % 16)
            k = n if k == "n" else k
            if k is not None and k <= n:
                limit = int(D.LEVELS[int(s["level"])][7]) * D.CTRL_FREQ
                s["step_counter"] = limit + D.SUBSTEPS - D.SUBSTEPS * k
                par = 0 if k % 2 == 1 else 1   # it flocks in the step it resets in
        if case != "reset":
            s["cow_vel"][:M] = 0.0
        s["step_counter_A"] = 4 + par
        env = O.Env(0, N, M, table, env_id=e)
        env.reset()
        env.set_state(s)
        envs.append(env)
        states.append(env.get_state())
    return envs, states


def _n2(pos):
    """Squared pair distances [E, M, M] as the cheap pass forms them: (hi - lo) differences, zx * zx + zy * zy."""
    z = pos[:, None, :, :] - pos[:, :, None, :]   # [e, lo, hi] = pos[hi] - pos[lo]
    return z[..., 0] * z[..., 0] + z[..., 1] * z[..., 1]


def _check(case, E, n, placed, sca, pos, reset):
    """sca [n + 1, E]: step_counter_A before each step of the sequence; pos [n + 1, E, M, 2]: the cattle after it (the
    positions its flock ran on); reset [n + 1, E]; placed [E, M, 2]."""
    flock = (sca + 1) % 2 == 0
    iu = np.triu_indices(M, 1)
    cnt = np.stack([(_n2(pos[t])[:, iu[0], iu[1]] <= K_SUPPORT2).sum(axis=1) for t in range(n + 1)])   # [n + 1, E]
    if case in ("parity", "full", "empty", "boundary"):
        assert not flock[0].any() and not reset.any()
        for t in range(1, n + 1):
            assert flock[t].all() == (t % 2 == 1) and flock[t].any() == (t % 2 == 1), t
        assert np.array_equal(pos[1], placed), "the launch's first step does not see the cattle as placed"
    if case == "full":
        assert (cnt[1:][flock[1:]] == P).all()
    if case == "empty":
        assert (cnt[1:][flock[1:]] == 0).all()
    if case == "boundary":
        x_in, x_out = _boundary_x()
        n2 = _n2(pos[1])[E_BOUNDARY]
        assert n2[0, 1] == x_in * x_in <= K_SUPPORT2 < x_out * x_out == n2[0, 2]
        assert n2[0, 3] == 1.2 * 1.2 <= K_SUPPORT2
        assert cnt[1, E_BOUNDARY] == 2
    if case == "reset":
        assert flock[1:].any(axis=1).all() and not flock[1:].all(axis=1).any(), "the parities are not mixed"
        assert (reset[1:] & flock[1:]).any(), "no reset inside the launch in a flocking env"
        assert (reset[1] & flock[1]).any(), "no reset in a flocking env at the launch's first step"


@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_placements_on_oracle(case, E, n):
    """The CPU oracle alone, from the placed states with its own action stream: the flock parities, the pair counts
    (120, 0, the boundary pairs on their sides) and the resets fall where the GPU test needs them."""
    envs, states = _states(case, E, n)
    placed = np.stack([np.asarray(s["cow_pos"])[:M] for s in states])
    sca = np.zeros((n + 1, E), int)
    pos = np.zeros((n + 1, E, M, 2))
    reset = np.zeros((n + 1, E), bool)
    for t in range(n + 1):
        for e, env in enumerate(envs):
            sca[t, e] = int(env.st.step_counter_A)
            out = env.step(env.random_actions(2 + t), autoreset=True)
            reset[t, e] = bool(np.any(out[2]) or np.any(out[3]))
            pos[t, e] = np.array([[env.st.cp[j][0], env.st.cp[j][1]] for j in range(M)])
    if case == "reset":   # a reset env's cattle are the new episode's: no count is read from them
        pos[reset] = 0.0
    _check(case, E, n, placed, sca, pos, reset)


def _pair(E):
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    hs = [HerdBatch(E, N, M, mode="ctde") for _ in range(2)]
    # the first handle runs ch_step_n on the pipelined geometry, the second plain steps on the default one
    assert _lib.lib().ch__set_geometry(hs[0].handle, ctypes.c_int32(GEOM[0]), ctypes.c_int32(GEOM[1])) == 0
    return hs


def _assert_same(a, b):
    import torch
    torch.cuda.synchronize()
    outs = lambda h: (h.obs, h.reward, h.terminated, h.truncated, h.reset_happened)  # noqa: E731
    for i, (x, y) in enumerate(zip(outs(a), outs(b))):
        assert torch.equal(torch.nan_to_num(x.float(), nan=7.0), torch.nan_to_num(y.float(), nan=7.0)), i
    assert torch.equal(a.actions, b.actions)
    (da, ia), (db, ib) = a.get_state_raw(), b.get_state_raw()
    assert np.array_equal(da, db, equal_nan=True) and np.array_equal(ia, ib)
    assert np.array_equal(a.metrics(), b.metrics(), equal_nan=True)
    for h in (a, b):
        h.sync()   # raises on a device error (an expired hand-off wait)


@pytest.mark.gpu
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_env_unit_cheap_pass_equals_plain_steps(case, E, n):
    import torch
    from cattleherd import _lib
    _, states = _states(case, E, n)
    placed = np.stack([np.asarray(s["cow_pos"])[:M] for s in states])
    s = stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states])
    a, b = _pair(E)
    sca = np.zeros((n + 1, E), int)
    pos = np.zeros((n + 1, E, M, 2))
    reset = np.zeros((n + 1, E), bool)

    def plain(t):
        sca[t] = b.get_state()["step_counter_A"]
        b.step(random_actions=True, autoreset=True, terminal_obs=False)
        torch.cuda.synchronize()
        reset[t] = b.reset_happened.cpu().numpy().reshape(E).astype(bool)
        pos[t] = b.get_state()["cow_pos"]
    for h in (a, b):
        h.reset()
        h.set_state(s)
    a.step(random_actions=True, autoreset=True, terminal_obs=False)   # writes the observation blocks in full
    plain(0)
    m0 = _lib.lib().ch__multi_steps(a.handle)
    a.step_n(n, random_actions=True)
    for t in range(1, n + 1):
        plain(t)
    assert _lib.lib().ch__multi_steps(a.handle) - m0 == n   # every step ran inside the pipelined launch
    if case == "reset":
        pos[reset] = 0.0
    _check(case, E, n, placed, sca, pos, reset)
    _assert_same(a, b)
    for h in (a, b):
        h.close()
