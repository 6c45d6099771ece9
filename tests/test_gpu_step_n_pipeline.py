"""ch_step_n's pipelined multi-step kernel (k_step2_multi at 16 envs x 4 drones x 16 cattle, f64, CTDE: two drone waves
that alternate steps, LDS hand-off of the chain state, no workgroup barrier between steps) against the same number
of plain ch_step launches, bit for bit: state, outputs, metrics, drawn actions.

Shapes: the smallest that reach every path of the step loop -- 16 envs (one full workgroup), 24 (a second workgroup
with 8 of its 16 env slots live), 48; n = 1 leaves the second drone wave idle, even n ends on it, odd n on the first.
The handles get the (16 envs, 512 threads) geometry ch_create picks from 4096 envs up, so the pipelined instantiation
runs at these sizes, and every case asserts that the steps ran inside the multi-step kernel.

Resets: `_reset_states` staggers time-limit truncations over the launch so that an env resets at its first step, in
two consecutive steps of one workgroup, at its last step, and (NUM_DRONES drawn from 2..4) with fewer and with more
live drones than before -- the places where the next step's chain starts from a body the books of the previous step
have just rebuilt.  test_reset_positions_on_oracle checks that schedule on the CPU oracle alone; the GPU test asserts
it again from the single-step handle's reset_happened and NUM_DRONES.
"""
import ctypes

import numpy as np
import pytest

import directed_states as D
from helpers import stack

N, M, LEVEL = 4, 16, 0
GEOM = (16, 512)
SIZES = (16, 24, 48)
STEPS = (1, 2, 3, 8, 23)


def _table():
    import torch  # noqa: F401  (before the library, as HerdBatch loads them: one HIP runtime for both in this process)
    from cattleherd._lib import spawn_table
    return spawn_table(M)


def _pair(E, **kw):
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    hs = [HerdBatch(E, N, M, mode="ctde", **kw) for _ in range(2)]
    # the first handle runs ch_step_n on the pipelined geometry, the second plain steps on the default one
    assert _lib.lib().ch__set_geometry(hs[0].handle, ctypes.c_int32(GEOM[0]), ctypes.c_int32(GEOM[1])) == 0
    return hs


def _outs(h):
    return [x.clone() for x in (h.obs, h.reward, h.terminated, h.truncated, h.reset_happened)]


def _assert_same(a, b, actions=True):
    import torch
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(_outs(a), _outs(b))):
        assert torch.equal(torch.nan_to_num(x.float(), nan=7.0), torch.nan_to_num(y.float(), nan=7.0)), i
    if actions:
        assert torch.equal(a.actions, b.actions)
    (da, ia), (db, ib) = a.get_state_raw(), b.get_state_raw()
    assert np.array_equal(da, db, equal_nan=True) and np.array_equal(ia, ib)
    assert np.array_equal(a.metrics(), b.metrics(), equal_nan=True)
    for h in (a, b):
        h.sync()   # raises on a device error (an expired hand-off wait)


def _multi(h):
    from cattleherd import _lib
    return _lib.lib().ch__multi_steps(h.handle)


# ---- reset schedule ----------------------------------------------------------------------------------------------
# env slot within each group of 16 (its directed class) -> step of the sequence at which it reaches the time limit;
# step 0 is the plain launch after set_state, step j >= 1 is step j - 1 of the multi-step launch; "n": the last one
SCHEDULE = {15: 1, 0: 2, 6: 3, 14: "n", 2: 1, 4: "n"}   # inherd, oncow, oncow, oncow, ring, close


def _reset_states(E, n):
    """Directed oracle envs (NUM_DRONES varying in 2..4) with the schedule's envs 4 k substeps short of the time limit."""
    envs, states = D.directed_states(0, N, M, LEVEL, E, 4242, _table(), min_drones=2)
    limit = int(D.LEVELS[LEVEL][7]) * D.CTRL_FREQ
    for e, env in enumerate(envs):
        k = SCHEDULE.get(e % 16)
        if k is None:
            continue
        k = n if k == "n" else k
        if k > n:
            continue
        s = states[e]
        s["step_counter"] = limit + D.SUBSTEPS - D.SUBSTEPS * k
        env.set_state(s)
        states[e] = env.get_state()
    return envs, states


def _actions(E):
    # small actions: the formation the directed state placed stays together over the window
    return (0.05 * np.random.default_rng(11).uniform(-1, 1, (E, N, 4))).astype(np.float32)


def _check_positions(reset, n_before, n_after, E, n):
    """reset [n + 1, E] (step 0: the plain launch), NUM_DRONES before / after each step: the positions (i)-(iv)."""
    assert reset[1].any(), "(i) no reset at the first step of the launch"
    assert reset[n].any(), "(iii) no reset at the last step of the launch"
    if n >= 2:
        wg = [reset[:, g:g + 16].any(axis=1) for g in range(0, E, 16)]
        assert any(w[t] and w[t + 1] for w in wg for t in range(1, n)), "(ii) no two consecutive steps with a reset in one workgroup"
    if n >= 8 and E >= 48:
        r = reset[1:]
        assert (r & (n_after[1:] < n_before[1:])).any(), "(iv) no reset lowers NUM_DRONES"
        assert (r & (n_after[1:] > n_before[1:])).any(), "(iv) no reset raises NUM_DRONES"


RESET_CASES = [(16, 1), (16, 2), (24, 3), (48, 8), (48, 23)]


@pytest.mark.parametrize("E,n", RESET_CASES)
def test_reset_positions_on_oracle(E, n):
    """The CPU oracle alone, from the staggered states with the test's actions: resets fall on the first step of the
    launch, on two consecutive steps of a workgroup, on the last step, and change NUM_DRONES both ways."""
    envs, states = _reset_states(E, n)
    acts = _actions(E)
    reset = np.zeros((n + 1, E), bool)
    nb, na = np.zeros((n + 1, E), int), np.zeros((n + 1, E), int)
    for t in range(n + 1):
        for e, env in enumerate(envs):
            nb[t, e] = int(env.get_state()["n"])
            out = env.step(acts[e], autoreset=True)
            reset[t, e] = bool(np.any(out[2]) or np.any(out[3]))
            na[t, e] = int(env.get_state()["n"])
    _check_positions(reset, nb, na, E, n)


@pytest.mark.gpu
@pytest.mark.parametrize("E,n", RESET_CASES)
def test_resets_where_the_pipeline_is_exposed(E, n):
    import torch
    _, states = _reset_states(E, n)
    s = stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states])
    a, b = _pair(E, curriculum_level=LEVEL, min_drones=2, max_drones=N)
    act = torch.tensor(_actions(E), device=a.device)
    for h in (a, b):
        h.reset()
        h.set_state(s)
        h.step(act, random_actions=False, autoreset=True, terminal_obs=False)   # writes the observation blocks in full
    reset = np.zeros((n + 1, E), bool)
    nb, na = np.zeros((n + 1, E), int), np.zeros((n + 1, E), int)
    m0 = _multi(a)
    a.step_n(n, actions=act, autoreset=True, random_actions=False)
    for t in range(1, n + 1):
        nb[t] = b.get_state()["n"]
        b.step(act, random_actions=False, autoreset=True, terminal_obs=False)
        torch.cuda.synchronize()
        reset[t] = b.reset_happened.cpu().numpy().reshape(E).astype(bool)
        na[t] = b.get_state()["n"]
    assert _multi(a) - m0 == n
    _check_positions(reset, nb, na, E, n)
    _assert_same(a, b, actions=False)
    for h in (a, b):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("E", SIZES)
def test_pipelined_step_n_equals_n_steps(E, n):
    """Device-drawn actions from a burnt-in state (episodes end at their long-run rate inside the window)."""
    a, b = _pair(E)
    for h in (a, b):
        h.reset()
        for _ in range(140):
            h.step(random_actions=True, autoreset=True, terminal_obs=False)
    m0 = _multi(a)
    a.step_n(n, random_actions=True)
    for _ in range(n):
        b.step(random_actions=True, autoreset=True, terminal_obs=False)
    assert _multi(a) - m0 == n
    _assert_same(a, b)
    for h in (a, b):
        h.close()


@pytest.mark.gpu
def test_sequences_around_a_pipelined_launch():
    """What a pipelined launch leaves in global memory (state, Euler cache and its flag) is what the next call reads:
    two ch_step_n back to back, a plain ch_step, ch_step_n again; then a call after invalidate_obs and one after
    set_state (each starts with a plain step that rewrites the observation blocks, the rest runs pipelined)."""
    E = 24
    a, b = _pair(E)
    for h in (a, b):
        h.reset()
        for _ in range(140):
            h.step(random_actions=True, autoreset=True, terminal_obs=False)

    def both(k, plain_first=0):
        m0 = _multi(a)
        a.step_n(k, random_actions=True)
        for _ in range(k):
            b.step(random_actions=True, autoreset=True, terminal_obs=False)
        assert _multi(a) - m0 == k - plain_first
        _assert_same(a, b)
    both(5)
    both(4)
    for h in (a, b):
        h.step(random_actions=True, autoreset=True, terminal_obs=False)
    _assert_same(a, b)
    both(7)
    for h in (a, b):
        h.invalidate_obs()
    both(6, plain_first=1)
    s = b.get_state()
    s["drone_quat"] = s["drone_quat"] + 1e-3
    s["drone_quat"] /= np.linalg.norm(s["drone_quat"], axis=-1, keepdims=True)
    for h in (a, b):
        h.set_state(s)
    both(6, plain_first=1)
    for h in (a, b):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("autoreset", [False, True])
def test_pipelined_step_n_given_actions(autoreset):
    """Caller actions (the same buffer every step), auto-reset off and on, as test_step_n_given_actions."""
    import torch
    E, K = 48, 17
    a, b = _pair(E)
    for h in (a, b):
        h.reset()
        for _ in range(60):
            h.step(random_actions=True, autoreset=True, terminal_obs=False)
    g = torch.Generator(device="cpu").manual_seed(5)
    act = (torch.rand((E, N, 4), generator=g) * 2 - 1).to(a.device)
    m0 = _multi(a)
    a.step_n(K, actions=act, autoreset=autoreset, random_actions=False)
    for _ in range(K):
        b.step(act, random_actions=False, autoreset=autoreset, terminal_obs=False)
    assert _multi(a) - m0 == K
    _assert_same(a, b, actions=False)
    for h in (a, b):
        h.close()
