"""ch_step_n's pipelined kernel at the workgroup shapes test_gpu_step_n_pipeline.py does not pin, bit for bit against
plain ch_step launches (that file's _assert_same: outputs, drawn actions, raw state, metrics, no expired wait).

The pipelined instantiation of k_step2_multi has a launch bound of its own, S = 640 threads (2 drone waves + 8 cow
waves); a handle's block is clamped to it inside the launch.  The cow waves share their work out dynamically, so the
number of cow waves must not show in any output.  Shapes (envs per workgroup, block set on the ch_step_n handle; the
reference handle keeps the default geometry):
  (16, S)    the shipped shape: the existing file's full matrix, its reset schedule and its call sequences
  (16, 768)  the production handle's block, clamped to S
  (16, 256), (16, 320)  the fewest cow waves the launch accepts (2 and 3): two cows per lane in the integration loop,
             no co-SIMD skip (fewer than 4 cow waves), a cow-wave barrier of two waves
  flock-parity mix at (16, S): step_counter_A odd in half of a workgroup's envs and even in the rest, so the flock list
             is neither empty nor full on any step, with a reset on a flocking and on a non-flocking step
"""
import ctypes

import numpy as np
import pytest

import directed_states as D
import step_rows as SR
from helpers import stack
from test_gpu_step_n_pipeline import (LEVEL, M, N, RESET_CASES, SIZES, STEPS, _actions, _assert_same, _check_positions,
                                      _multi, _reset_states)

S = 640                       # the pipelined instantiation's launch bound (csrc/ch_step_multi.hip)
NARROW = [(16, 256), (16, 320)]
CLAMPED = (16, 768)
SMALL_CASES = [(24, 8), (48, 23)]   # (E, n) for the shapes beside S: a half-live workgroup, an even and an odd n


def _pair(E, geom, **kw):
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    hs = [HerdBatch(E, N, M, mode="ctde", **kw) for _ in range(2)]
    assert _lib.lib().ch__set_geometry(hs[0].handle, ctypes.c_int32(geom[0]), ctypes.c_int32(geom[1])) == 0
    # every shape of this file keeps ch_step_n on the pipelined row, with the 16 x 4 x 16 body for its plain first step
    assert SR.held_names(hs[0]) == {"step_row": "k_step2<double,0,16,4,16>", "multi_row": "k_step2_multi<double,0,16,4,16>",
                                    "step_row_tobs": "k_step2<double,0,16,4,16,false,false,true>"}
    return hs


def _burnt_in(E, geom, steps=140):
    a, b = _pair(E, geom)
    for h in (a, b):
        h.reset()
        for _ in range(steps):
            h.step(random_actions=True, autoreset=True, terminal_obs=False)
    return a, b


def _run_random(E, n, geom):
    a, b = _burnt_in(E, geom)
    m0 = _multi(a)
    a.step_n(n, random_actions=True)
    for _ in range(n):
        b.step(random_actions=True, autoreset=True, terminal_obs=False)
    assert _multi(a) - m0 == n
    _assert_same(a, b)
    for h in (a, b):
        h.close()


def _run_states(E, n, geom, states):
    """From oracle state dicts with the pipeline file's caller actions: one plain step (it writes the observation blocks
    in full), then n steps in one launch against n plain steps.  Returns reset [n + 1, E], NUM_DRONES before / after."""
    import torch
    s = stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states])
    a, b = _pair(E, geom, curriculum_level=LEVEL, min_drones=2, max_drones=N)
    act = torch.tensor(_actions(E), device=a.device)
    for h in (a, b):
        h.reset()
        h.set_state(s)
        h.step(act, random_actions=False, autoreset=True, terminal_obs=False)
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
    _assert_same(a, b, actions=False)
    for h in (a, b):
        h.close()
    return reset, nb, na


# ---- (16, S): the existing file's matrix ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("E", SIZES)
def test_wide_step_n_equals_n_steps(E, n):
    _run_random(E, n, (16, S))


@pytest.mark.gpu
@pytest.mark.parametrize("E,n", RESET_CASES)
def test_wide_resets_where_the_pipeline_is_exposed(E, n):
    _, states = _reset_states(E, n)
    reset, nb, na = _run_states(E, n, (16, S), states)
    _check_positions(reset, nb, na, E, n)


@pytest.mark.gpu
def test_wide_sequences_around_a_pipelined_launch():
    """Back-to-back calls, a plain step between, and calls after invalidate_obs / set_state (each of those starts with
    a plain step that rewrites the observation blocks), as test_sequences_around_a_pipelined_launch."""
    E = 24
    a, b = _burnt_in(E, (16, S))

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


# ---- (16, 768) clamped to S; (16, 256) and (16, 320): the fewest cow waves --------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("E,n", SMALL_CASES)
@pytest.mark.parametrize("geom", [CLAMPED] + NARROW, ids=lambda g: f"{g[0]}x{g[1]}")
def test_other_blocks_equal_n_steps(geom, E, n):
    _run_random(E, n, geom)


@pytest.mark.gpu
@pytest.mark.parametrize("E,n", SMALL_CASES)
@pytest.mark.parametrize("geom", [CLAMPED] + NARROW, ids=lambda g: f"{g[0]}x{g[1]}")
def test_other_blocks_with_resets(geom, E, n):
    _, states = _reset_states(E, n)
    reset, nb, na = _run_states(E, n, geom, states)
    _check_positions(reset, nb, na, E, n)


# ---- flock-parity mix ----------------------------------------------------------------------------------------------
MIX_E, MIX_N = 16, 3


def _mixed_parity_states():
    """The staggered reset schedule at 16 envs, with step_counter_A's parity set to the env index's: after the plain
    step, half of the workgroup's envs flock on the odd steps of the launch and the other half on the even ones."""
    envs, states = _reset_states(MIX_E, MIX_N)
    for e, env in enumerate(envs):
        s = states[e]
        s["step_counter_A"] = 2 * (int(s["step_counter_A"]) // 2) + e % 2
        env.set_state(s)
        states[e] = env.get_state()
    return envs, states


def _check_mix(flock, reset):
    """flock, reset [n + 1, E] (row 0: the plain step): a mixed flock list on every step of the launch, and a reset
    both on a step its env flocks in and on one it does not."""
    nf = flock[1:].sum(axis=1)
    assert ((nf > 0) & (nf < MIX_E)).all(), nf
    assert (reset[1:] & flock[1:]).any(), "no reset on a flocking step"
    assert (reset[1:] & ~flock[1:]).any(), "no reset on a non-flocking step"


def test_mixed_parity_schedule_on_oracle():
    """The CPU oracle alone: the schedule keeps the flock list mixed and resets envs on both kinds of step."""
    envs, _ = _mixed_parity_states()
    acts = _actions(MIX_E)
    flock, reset = np.zeros((MIX_N + 1, MIX_E), bool), np.zeros((MIX_N + 1, MIX_E), bool)
    for t in range(MIX_N + 1):
        for e, env in enumerate(envs):
            flock[t, e] = D.flock_runs(env.get_state())
            out = env.step(acts[e], autoreset=True)
            reset[t, e] = bool(np.any(out[2]) or np.any(out[3]))
    _check_mix(flock, reset)


@pytest.mark.gpu
def test_mixed_flock_parity_with_resets():
    import torch
    _, states = _mixed_parity_states()
    E, n = MIX_E, MIX_N
    s = stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states])
    a, b = _pair(E, (16, S), curriculum_level=LEVEL, min_drones=2, max_drones=N)
    act = torch.tensor(_actions(E), device=a.device)
    for h in (a, b):
        h.reset()
        h.set_state(s)
        h.step(act, random_actions=False, autoreset=True, terminal_obs=False)
    flock, reset = np.zeros((n + 1, E), bool), np.zeros((n + 1, E), bool)
    m0 = _multi(a)
    a.step_n(n, actions=act, autoreset=True, random_actions=False)
    for t in range(1, n + 1):
        flock[t] = (np.asarray(b.get_state()["step_counter_A"]).reshape(E) + 1) % 2 == 0
        b.step(act, random_actions=False, autoreset=True, terminal_obs=False)
        torch.cuda.synchronize()
        reset[t] = b.reset_happened.cpu().numpy().reshape(E).astype(bool)
    assert _multi(a) - m0 == n
    _check_mix(flock, reset)
    _assert_same(a, b, actions=False)
    for h in (a, b):
        h.close()
