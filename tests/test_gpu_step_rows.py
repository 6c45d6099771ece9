"""Every row of the step-kernel table (csrc/ch_step_plan.h kStepTable) stepped from the directed batch of
tests/directed_states.py, by the recipes of tests/step_rows.py; tests/test_step_rows_cpu.py shows with no device that
each recipe plans to its row at any CU count and that the batches reach every branch.  Every test first asserts, from
ch__step_plan_of, that its handle holds the row it is about.

k_step2, f64 (13 rows): test_directed_step_vs_oracle's six lockstep steps against the CPU oracle (its body,
  tests/test_gpu_directed.py _steps_vs_oracle), at the project's f64 bars unchanged -- obs 1e-6 / 1e-7, reward 1e-6 /
  1e-6, drone state 1e-9 / 1e-12, cow_pos 1e-12 / 1e-13, cow_vel 1e-12 / 1e-14, integers, flags and actions exact.  The
  seven bodies compiled for one geometry run at ch__set_geometry(GT, block) with 96 envs, where 16 envs of different
  classes share a workgroup, and again with a half-filled last workgroup: 96 + GT / 2 envs (104, 100, 98), device env
  e at the state of oracle env e % 96, the oracle twin of e >= 96 a new env of that id.  The TOBS twin steps with
  terminal observations; the rows it writes for the envs that reset are bit-equal to the observations the plain
  16 x 4 x 16 row gives a twin handle that takes the same state and actions without auto-reset.
k_step2, f32 (13 rows): one step judged per class with section A of tests/test_gpu_f32_parity.py (its budget, its
  neighbour-tie rule, its helpers), the body-rate misses it knows aside (RATE_KNOWN there, ROW_RATE_KNOWN here for the
  cases it does not step).  A handle runs the TOBS twin only on a step with auto-reset and a terminal-observation
  buffer, so that row's step has both: an env that reset is judged on its terminal observation, reward and flags, and
  its carried state, the new episode's, is left to the comparison with v1.  And 40 steps with auto-reset from the
  batch tiled to 257 envs, bit-identical to the f32 v1 kernel, terminal observations included wherever asking for them
  keeps the handle on the row.
k_step2_multi (7 rows): ch_step_n(40) against 40 ch_step calls on a handle of the same geometry -- the row's
  plain-step twin, held to the oracle above -- from the tiled, staggered batch: outputs, state, metrics and evaluation
  distances bit for bit, more than 20 resets after step 2.  Three rows are held by tests/test_gpu_directed.py's IDENT
  (step_rows.HELD), which asserts their names; the WPE = 4 row needs more than 256 workgroups, 4112 envs.
k_step2_actor (2 rows): held by tests/test_gpu_rollout.py::test_fused_step_actor_is_bit_identical.

Two-drone shapes (CTDE 2 x 8): the reference's own reward is NaN (tests/test_step_rows_cpu.py); they compare NaN with
NaN and are judged numerically on observations, cattle state and flags.

Measured on an MI355X (each test prints its figures).  k_step2 f64, per row: the worst ratio of error to bar over the
six steps for the drone state and cow_vel, then terminations / truncations / resets; `+` the half-filled run.  In every
run of every row the observations, the rewards and cow_pos equal the oracle's bit for bit (ratio 0).
  <double,1,0,0,0,true>                   5.8e-4  4.3e-4   12 / 222 / 12
  <double,0,16,4,16,true>                 1.7e-4  4.4e-4    0 /  36 / 36    + 104 envs: the same ratios, 0 / 38 / 38
  <double,0,0,0,0,true>                   4.5e-4  2.5e-4    0 /  37 / 37
  <double,1,16,4,32,false,true>           1.4e-4  7.9e-4   12 / 222 / 12    + 104: the same, 13 / 234 / 13
  <double,1,0,0,0,false,true>             1.4e-4  7.9e-4   12 / 222 / 12
  <double,0,0,0,0,false,true>             8.6e-4  1.5e-3    0 /  39 / 39
  <double,1,0,0,0>                        1.6e-4  3.8e-4   12 / 216 / 12
  <double,0,8,4,16>                       1.4e-4  5.5e-4    0 /  36 / 36    + 100: the same, 0 / 36 / 36
  <double,0,16,4,16,false,false,true>     1.4e-4  5.5e-4    0 /  36 / 36    + 104: the same, 0 / 38 / 38
  <double,0,16,4,16>                      1.4e-4  5.5e-4    0 /  36 / 36    + 104: the same, 0 / 38 / 38
  <double,0,16,2,8>                       1.9e-4  2.5e-4    0 /  44 / 44    + 104: 2.0e-4, 2.5e-4, 0 / 46 / 46
  <double,0,4,2,8>                        1.9e-4  2.5e-4    0 /  44 / 44    + 98: the same, 0 / 44 / 44
  <double,0,0,0,0>                        1.7e-4  2.5e-4   12 /  35 / 47
  (MARL counts a truncation per env-step of an episode no agent has ended; the level-7 cases have no terminating
  branch.)  The TOBS twin's terminal observations equal the plain row's on all 36 / 38 resets.
k_step2 f32: every class of every row meets section A's bounds; the only misses are four body-rate entries
  (ROW_RATE_KNOWN), the same entry on every row of a case.  Against v1 over 40 steps of 257 envs: 54 to 129 resets per
  row, no difference.
k_step2_multi: resets after step 2 -- <double,0,16,4,16> 74, <double,0,16,2,8> 76, <double,0,4,2,8> 76 (1001 envs),
  <float,0,16,4,16,false,false,4> 314 (4112 envs); no difference from the plain steps.
"""
import functools

import numpy as np
import pytest

import directed_states as D
import step_rows as SR
import test_gpu_f32_parity as FP
from test_gpu_directed import (_batch, _lockstep, _same_state, _set_geometry, _set_kernel, _stagger, _step_n_vs_steps,
                               _steps_vs_oracle, _table, _tiled)

pytestmark = pytest.mark.gpu

F64_ROWS = [n for n, e in SR.STEP_ROWS.items() if e[5] == SR.F64]
F32_ROWS = [n for n, e in SR.STEP_ROWS.items() if e[5] == SR.F32]
ORACLE_RUNS = [(n, SR.E_DIRECTED) for n in F64_ROWS] + [(n, SR.partial_envs(n)) for n in F64_ROWS if SR.specialised(n)]
MULTI_HERE = [n for n in SR.MULTI_ROWS if n not in SR.HELD]
TOBS_ROW, PLAIN_ROW = "k_step2<double,0,16,4,16,false,false,true>", "k_step2<double,0,16,4,16>"


def _handle(name, E):
    """A handle of the row's recipe at E envs, its geometry forced, holding the row."""
    mode, n, m, level, kw, prec, geom, tobs = SR.CENSUS[name]
    b = _batch(mode, n, m, E, level, precision=prec, **kw)
    _hold(b, name, geom)
    return b


def _hold(b, name, geom):
    if geom is not None:
        _set_geometry(b, geom)
    held = SR.held_names(b)
    assert held[SR.plan_key(name, SR.CENSUS[name])] == name, (name, held)


def _oracle_envs(case, E):
    """E oracle envs at the directed states: env e >= 96 is a new env of id e at the state of env e % 96."""
    import oracle as O
    mode, n, m, level, kw = case
    assert set(kw) <= {"physics"}, kw   # (the extra envs below are built with no other option of directed_states)
    envs, states = D.directed_states(mode, n, m, level, D.E_DIRECTED, D.case_seed(case), _table(m), **kw)
    for e in range(D.E_DIRECTED, E):
        env = O.Env(mode, n, m, _table(m), max_drones=n, start_level=level, env_id=e, physics=kw.get("physics", 0))
        env.reset()
        env.set_state(states[e % D.E_DIRECTED])
        envs.append(env)
        states.append(env.get_state())
    return envs, states


@pytest.mark.parametrize("name,E", ORACLE_RUNS, ids=[f"{n}-{E}" for n, E in ORACLE_RUNS])
def test_f64_row_vs_oracle(name, E):
    """Module docstring, k_step2 f64: the row's handle against the oracle over six steps with auto-reset."""
    import torch
    entry = SR.CENSUS[name]
    case, tobs = entry[:5], entry[7]
    mode, n, m, level, kw = case
    envs, states = _oracle_envs(case, E)
    assert all(D.class_of(e) == D.class_of(e % D.E_DIRECTED) for e in range(E))
    b = _handle(name, E)
    twin, hook, seen = None, None, []
    if name == TOBS_ROW:
        twin = _handle(PLAIN_ROW, E)
        twin.reset()

        def hook(t, pre, acts, dn):
            twin.set_state(pre)
            twin.step(torch.tensor(acts, device=twin.device), autoreset=False, terminal_obs=False)
            torch.cuda.synchronize()
            idx = torch.tensor(np.flatnonzero(dn), device=b.device)
            assert torch.equal(b.terminal_obs[idx], twin.obs[idx]), t
            assert torch.isfinite(b.terminal_obs[idx]).all()
            seen.append(int(dn.sum()))
    f = _steps_vs_oracle(b, envs, states, case, terminal_obs=tobs, after_step=hook)
    w = f["worst"]
    print(f"ROW {name} E {E}: worst error / bar obs {w['obs']:.2e} reward {w['reward']:.2e} drone {w['drone']:.2e} "
          f"cow_pos {w['cow_pos']:.2e} cow_vel {w['cow_vel']:.2e}; terms {f['terms']} truncs {f['truncs']} resets {f['resets']}")
    assert f["truncs"] > 0 and f["resets"] > 0 and (level == 7 or f["terms"] > 0)
    assert SR.held_names(b)[SR.plan_key(name, entry)] == name
    if twin is not None:
        assert sum(seen) == f["resets"] > 0
        twin.close()
    b.close()


# ---- k_step2, f32 --------------------------------------------------------------------------------------------------

# Body-rate entries beyond their elementwise bound (FP.RATE_KNOWN's kind, same cause, same treatment) in the cases
# section A of tests/test_gpu_f32_parity.py does not step; device vs oracle, rad/s, measured on an MI355X.  The v2
# geometries compute the same arithmetic in the same order, so a case misses on the same entries on every row.
ROW_RATE_KNOWN = {
    "ctde-4x16-L7-oncow": {        # (tests/test_gpu_directed.py F32_XFAIL names the same entry by class)
        "env 48 drone 3 column 9": "-0.00010850272 vs -0.0001085504",
    },
    "ctde-4x16-L7-trunc_collision": {
        "env 56 drone 1 column 8": "-9.3215662e-05 vs -9.3159462e-05",
    },
    "marl-4x32-L0-spaced": {
        "env 3 drone 3 column 8": "-0.00022451603 vs -0.00022458741",
    },
    "marl-4x16-L0-oncow": {        # f32 MARL 4 x 16 under PYB is stepped against the oracle here for the first time
        "env 86 drone 1 column 9": "0.00018401694 vs 0.00018391389",
    },
}


@functools.lru_cache(maxsize=None)
def _f32_row_step(name):
    mode, n, m, level, kw, prec, geom, tobs = SR.CENSUS[name]
    return FP._f32_step_of((mode, n, m, level, kw), prepare=lambda b: _hold(b, name, geom), tobs=tobs)


def _rate_known(name, cls):
    i = f"{D.case_id(SR.CENSUS[name][:5])}-{cls}"
    return dict(FP.RATE_KNOWN.get(i, {}), **ROW_RATE_KNOWN.get(i, {}))


F32_PARAMS = [(n, cls) for n in F32_ROWS for cls in FP.CLASSES]


@pytest.mark.parametrize("name,cls", F32_PARAMS, ids=[f"{n}-{cls}" for n, cls in F32_PARAMS])
def test_f32_row_step(name, cls):
    """Module docstring, k_step2 f32: one step on the row's handle, one class of the batch, every check of section A."""
    d = _f32_row_step(name)
    if cls == FP.CLASSES[0]:   # the TOBS twin steps with auto-reset: its terminal observations are what is judged
        assert d["reset"].any() == SR.CENSUS[name][7], int(d["reset"].sum())
    assert d["kept"] and set(d["tie_classes"]) <= {"ring", "term", "levelup"}, d["tie_classes"]
    FP._check_flags_and_rewards(d, cls)
    found, c, worst = FP._obs_misses_of(d, cls)
    figs = FP._state_figures_of(d, cls)
    state = max(figs, key=lambda f: f[1])
    rates = FP._step_rate_misses_of(d, cls)
    print(f"ROW {name} {cls}: geometry {d['geom']}; obs column {c} at {worst:.2e} of its scale, misses {found}; state "
          f"{state[0]}[{state[2]}] {state[1]:.2e}; rate misses {rates}")
    assert not found, (cls, found)
    FP._check_integer_state(d, cls)
    bad = {k: f"column {col} {r:.2e} of its scale ({dv:.8g} vs {ov:.8g})" for k, r, col, dv, ov in figs if not r <= FP.BUDGET}
    assert not bad, (cls, bad)
    new = FP._new(rates, _rate_known(name, cls))
    assert not new, (cls, new)


@pytest.mark.parametrize("i", FP._known_params(ROW_RATE_KNOWN))
def test_f32_row_body_rates_known_misses(i):
    """The bound of test_f32_row_step on the entries ROW_RATE_KNOWN names alone, on every row of their case."""
    case_id, cls = i.rsplit("-", 1)
    rows = [n for n in F32_ROWS if D.case_id(SR.CENSUS[n][:5]) == case_id]
    assert rows
    for n in rows:
        found = FP._step_rate_misses_of(_f32_row_step(n), cls)
        assert not set(found) & set(ROW_RATE_KNOWN[i]), (n, found)


@pytest.mark.parametrize("name", F32_ROWS)
def test_f32_row_equals_v1(name):
    """40 steps of device Philox actions with auto-reset from the batch tiled to 257 envs (no multiple of any
    workgroup's env count): the row against the f32 v1 kernel, outputs and state bit for bit."""
    entry = SR.CENSUS[name]
    mode, n, m, level, kw, prec, geom, tobs = entry
    E, T = 257, 40
    s = _tiled(entry[:5], E)
    hs = [_batch(mode, n, m, E, level, precision=prec, **kw) for _ in range(2)]
    _set_kernel(hs[0], 1)
    _set_kernel(hs[1], 2)
    _hold(hs[1], name, geom)
    held = SR.held_names(hs[1])
    ask = tobs or held["step_row_tobs"] == held["step_row"]   # asking for them moves 16 x 4 x 16 to its TOBS twin
    for h in hs:
        h.reset()
        h.set_state(s)
    resets = _lockstep(hs, T, terminal_obs=ask)
    print(f"ROW {name}: {resets} resets in {T} steps of {E} envs, terminal observations {'compared' if ask else 'not asked for'}")
    assert resets > 0
    _same_state(*hs)
    for h in hs:
        h.close()


# ---- k_step2_multi -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MULTI_HERE)
def test_multi_row_equals_steps(name):
    """Module docstring, k_step2_multi: ch_step_n(40) on the row against 40 ch_step calls on its plain-step twin."""
    entry = SR.CENSUS[name]
    mode, n, m, level, kw, prec, geom, tobs = entry
    E, T = SR.MULTI_ENVS[name], 40
    s = _stagger(_tiled(entry[:5], E), mode, level)
    hs = [_batch(mode, n, m, E, level, precision=prec, **kw) for _ in range(2)]
    for h in hs:
        _hold(h, name, geom)
        h.reset()
        h.set_state(s)
    twin = SR.held_names(hs[1])["step_row"]
    assert twin in SR.STEP_ROWS and SR.STEP_ROWS[twin][:7] == entry[:7]
    later = _step_n_vs_steps(hs, T)
    print(f"ROW {name}: {later} resets after step 2 in {T} steps of {E} envs; plain-step twin {twin}")
    assert later > 20
    _same_state(*hs)
    for h in hs:
        h.close()
