"""GPU tests of the device-side evaluator log (cattleherd.eval_log; ch_eval_log_begin / _mark / _record / _run) against
tests/eval_log_ref.py, the numpy reference that builds the same rows through ``get_state()`` per step.  The log copies
state and evaluates comparisons written as numpy evaluates them, so every comparison here is exact (``==``)."""
import ctypes
import os

import numpy as np
import pytest

import eval_log_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, SEL, STEPS, EP_LEN = 12, [0, 3, 4, 7, 11], 24, 80   # level 7: 80 s
SHAPES = {"4x16-f64": (4, 16, {}), "2x8-f64-nan-reward": (2, 8, {}), "12x64-f64": (12, 64, {}),
          "4x16-f32": (4, 16, {"precision": "f32"}), "3x1-varying-n": (3, 1, {"min_drones": 2, "max_drones": 3})}


def _batch(n, m, kw, envs=E):
    from cattleherd.env import HerdBatch
    b = HerdBatch(envs, n, m, mode="ctde", **kw)
    b.reset()
    return b


def _actions(n, steps=STEPS, envs=E):
    return np.random.default_rng(100 * n + steps).uniform(-1, 1, (steps, envs, n, 4)).astype(np.float32)


def _logged(b, envs, actions, capacity=None, guard=0, prepare=None):
    """The table of the Python-primitive loop: mark, step without auto-reset, record, masked reset."""
    from cattleherd.eval_log import DeviceEvalLog
    torch = b.torch
    log = DeviceEvalLog(b, envs, len(actions) if capacity is None else capacity, guard=guard)
    if prepare:
        prepare(log)
    for a in actions:
        log.mark()
        _, _, te, tr = b.step(torch.from_numpy(a).to(b.device), autoreset=False)
        log.record()
        b.reset(mask=(te[:, 0] | tr[:, 0]))
    b.sync()
    return log


def _assert_rows(got, want, rows=None, what=""):
    for k in ("sel_env", "rows", "dropped") + R.ROW_ARRAYS:
        g, w = got[k], want[k]
        if rows is not None and k in R.ROW_ARRAYS:
            w = w[:, :rows]
        if rows is not None and k in ("rows", "dropped"):
            continue
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what} {k}"


_REF = {}


def _reference(shape):
    """The numpy reference of a shape's 24 random-action steps, computed once."""
    if shape not in _REF:
        n, m, kw = SHAPES[shape]
        b = _batch(n, m, kw)
        _REF[shape] = R.reference_rows(b, SEL, _actions(n), EP_LEN)
        b.close()
    return _REF[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_table_equals_the_get_state_reference_bit_for_bit(shape):
    """12 envs, 24 steps of random actions drawn once on the host, logged envs [0, 3, 4, 7, 11] (five waves: a partly
    filled second workgroup).  Every array equals the reference exactly: poses, velocities, start-of-step cattle
    velocities, distances, time, effectiveness, num_drones, episode, flags."""
    n, m, kw = SHAPES[shape]
    want, _, _ = _reference(shape)
    b = _batch(n, m, kw)
    log = _logged(b, SEL, _actions(n))
    got = log.arrays()
    _assert_rows(got, want, what=shape)
    if shape == "2x8-f64-nan-reward":
        assert np.isnan(b.reward.cpu().numpy()).all()          # (compat mode with two drones: the log does not care)
    if shape == "3x1-varying-n":
        assert set(np.unique(got["num_drones"])) == {2, 3}      # the polygon uses the live drones only
        assert np.all(got["drone_xy"][got["num_drones"] == 2][:, 2] == 0.0)
    assert got["drone_xy"].any() and got["cattle_vxy"].any() and got["drone_dist"].any()
    b.close()


@pytest.mark.parametrize("kind", ["timeout", "collision"])
def test_episode_ends_inside_the_window(kind):
    """From a placed state.  timeout: step_counter 4790 of 4800 with the drones in formation about the herd -- the
    fourth step starts past the limit: truncated with the time-out trigger (bit 2), the ``episode`` column increments
    on the next row and time and distances restart.  collision: two drones 0.25 m apart on closing actions -- a failure
    truncation with bit 2 clear.  No threshold comparison of any row is within 1e-9 of a tie (the same states on the
    CPU oracle: tests/test_eval_log_cpu.py)."""
    n, m, envs, sel = 4, 16, 4, [0, 2, 3]
    steps = 7 if kind == "timeout" else 24
    actions = np.zeros((steps, envs, n, 4), np.float32) if kind == "timeout" else R.closing_actions(steps, envs, n)
    out = []
    for path in ("ref", "log"):
        b = _batch(n, m, {}, envs)
        s = b.get_state()
        b.set_state(R.timeout_state(s, n, m, 4790) if kind == "timeout" else R.collision_state(s, n, m))
        if path == "ref":
            out.append(R.reference_rows(b, sel, actions, EP_LEN))
        else:
            out.append(_logged(b, sel, actions).arrays())
        b.close()
    (want, margins, done), got = out
    assert margins.min() >= 1e-9
    _assert_rows(got, want, what=kind)
    f = got["flags"]
    if kind == "timeout":
        assert np.all(f[:, :3] == 0) and np.all(f[:, 3] == 2 | 4) and np.all(f[:, 4:] == 0)
        assert np.all(got["episode"][:, 4] == got["episode"][:, 3] + 1) and np.all(got["time"][:, 4] == 0.0)
        assert np.all(got["time"][:, 3] == 4802 / 60)
        # the accumulator restarted: the reset zeroes it (the first step of the new episode then adds its own)
        assert not np.array_equal(got["drone_dist"][:, 4], got["drone_dist"][:, 3])
    else:
        assert np.all((f & 2).any(axis=1)) and not (f & 4).any()
        first = int(np.argmax(f[0] & 2))
        assert 0 < first < steps - 1 and got["episode"][0, first + 1] == got["episode"][0, first] + 1


def _actor():
    import torch
    from cattleherd.policy import DevicePolicy
    d = np.load(os.path.join(ROOT, "tests", "golden", "policy_ctde_v16_6.npz"))
    return DevicePolicy.sb3_actor({k.replace("__", "."): torch.tensor(d[k]) for k in d.files if "__" in k}, clip=False)


def test_native_loop_equals_the_python_primitive_loop():
    """ch_eval_log_run with the trained v16-6 actor, 16 envs x (4, 16), 24 steps, every env logged: the table is
    identical to run_steps' on a second handle with the same seed, and so is the two handles' whole state.  Envs 3 and
    9 start a few steps before the time limit, so the loop's masked reset runs on some envs and not on others."""
    from cattleherd.eval_log import DeviceEvalLog
    envs = 16
    res = []
    for path in ("run", "run_steps"):
        b = _batch(4, 16, {}, envs)
        sc = b.get_state()["step_counter"]
        sc[[3, 9]] = 4790
        b.set_state({"step_counter": sc})
        log = DeviceEvalLog(b, np.arange(envs), STEPS)
        assert getattr(log, path)(_actor(), STEPS) == STEPS
        b.sync()
        res.append((log.arrays(), b.get_state_raw()))
        b.close()
    (nat, nat_state), (py, py_state) = res
    _assert_rows(nat, py, what="native vs python")
    assert np.array_equal(nat["rows"], np.full(envs, STEPS, np.int32)) and not nat["dropped"].any()
    assert (nat["flags"][[3, 9]] & 4).any() and len(np.unique(nat["episode"][3])) == 2
    assert np.array_equal(nat_state[0], py_state[0], equal_nan=True) and np.array_equal(nat_state[1], py_state[1])


def test_full_rows_are_dropped_and_nothing_is_written_past_them():
    """capacity 5 over 9 steps: rows == 5, dropped == 4, the five rows are the reference's first five, and the guard
    band after every array of the table keeps the pattern it was filled with."""
    n, m, kw = SHAPES["4x16-f64"]
    want, _, _ = _reference("4x16-f64")

    def fill(log):
        sel = log.sel_env.clone()
        log._buf.fill_(0xA5)
        log.sel_env.copy_(sel)
        log.begin()

    b = _batch(n, m, kw)
    log = _logged(b, SEL, _actions(n)[:9], capacity=5, guard=512, prepare=fill)
    got = log.arrays()
    assert np.array_equal(got["rows"], np.full(len(SEL), 5, np.int32))
    assert np.array_equal(got["dropped"], np.full(len(SEL), 4, np.int32))
    _assert_rows(got, want, rows=5, what="capacity")
    guard = log.guard_bytes()
    assert guard.size >= 512 * len(log.ARRAYS) and np.all(guard == 0xA5)
    b.close()


def test_refusals():
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.eval_log import DeviceEvalLog
    L = _lib.lib()
    b = _batch(4, 16, {}, 8)
    log = DeviceEvalLog(b, [1, 5], 4)
    # a record after a step with CH_STEP_AUTORESET: the state it would read is already the next episode's
    b.step(random_actions=True, autoreset=True)
    with pytest.raises(_lib.ChError, match="CH_STEP_AUTORESET") as ei:
        log.record()
    assert ei.value.code == _lib.CH_ERR_INVALID
    b.step(random_actions=True, autoreset=False)
    log.record()
    b.sync()
    assert log.arrays()["rows"].tolist() == [1, 1]
    # MARL handles and handles without the distance accumulator
    for kw, word in (({"mode": "marl"}, b"CTDE"), ({"mode": "ctde", "eval_metrics": False}, b"eval_metrics")):
        o = HerdBatch(8, 4, 16, **kw)
        with pytest.raises(ValueError):
            DeviceEvalLog(o, [0], 4)
        lg = ctypes.byref(log._lg)
        assert L.ch_eval_log_begin(o.handle, lg, o._stream()) == _lib.CH_ERR_UNSUPPORTED
        assert word in L.ch_last_error(o.handle)
        assert L.ch_eval_log_mark(o.handle, lg, o._stream()) == _lib.CH_ERR_UNSUPPORTED
        assert L.ch_eval_log_record(o.handle, lg, o._io_ref, o._stream()) == _lib.CH_ERR_UNSUPPORTED
        o.close()
    # argument checks with a handle
    bad = _lib.ChEvalLog()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(log._lg), ctypes.sizeof(bad))
    bad.capacity = 0
    assert L.ch_eval_log_begin(b.handle, ctypes.byref(bad), b._stream()) == _lib.CH_ERR_INVALID
    bad.capacity, bad.n_sel = 4, 0
    assert L.ch_eval_log_mark(b.handle, ctypes.byref(bad), b._stream()) == _lib.CH_ERR_INVALID
    bad.n_sel, bad.dropped = 2, None
    assert L.ch_eval_log_record(b.handle, ctypes.byref(bad), b._io_ref, b._stream()) == _lib.CH_ERR_INVALID
    b.sync()
    assert log.arrays()["rows"].tolist() == [1, 1]
    b.close()


def test_pickle_equals_the_one_env_adapter():
    """``to_evaluators()[0].evaluation_data()`` from the device table equals the dict the one-env CattleAviary adapter
    builds with is_evaluating set (get_state per step, EvalTracker) over the same actions and the same seed-exact
    resets; the window holds a time-out, so the doubled episode entry and the aliased distance rows are in it."""
    from cattleherd.env import HerdBatch
    from cattleherd.eval_log import DeviceEvalLog
    from cattleherd.seeded import ReferenceResetRNG
    from cattleherd.spaces import CURRICULUM
    from gym_pybullet_drones.sb3_envs.CattleAviary import CattleAviary
    n, m, steps, seed = 12, 16, 9, 11
    actions = np.random.default_rng(3).uniform(-1, 1, (steps, n, 4)).astype(np.float32)
    env = CattleAviary(num_drones=n, num_cattle=m, reference_rng_seed=seed)
    env.reset()
    env.batch.set_state({"step_counter": np.array([4790])})
    env._sync_counts()
    env.is_evaluating = True
    for a in actions:
        _, _, te, tr, _ = env.step(a)
        if te or tr:
            env.reset()
    want = env.eval_system.evaluation_data()
    assert len(want["time_taken"]) == 2            # one time-out inside the window: two episode entries
    # the batch side: E = 1, S = 1
    lo, hi, _ = CURRICULUM[7]
    rng = ReferenceResetRNG(seed, lo, hi, m)
    b = HerdBatch(1, n, m, mode="ctde", min_drones=env.MIN_NUM_DRONES, max_drones=env.MAX_NUM_DRONES, curriculum_level=7)

    def reset(scA):
        nd, vel = rng.reset(scA)
        b.reset(num_drones=[nd], cow_vel=vel[None])

    reset(0)
    b.set_state({"step_counter": np.array([4790])})
    log = DeviceEvalLog(b, [0], steps)
    for a in actions:
        log.mark()
        _, _, te, tr = b.step(b.torch.from_numpy(a[None]).to(b.device), autoreset=False)
        log.record()
        if bool((te | tr).any().item()):
            reset(int(b.env_ints()["step_counter_A"][0]))
    b.sync()
    got_ev, = log.to_evaluators()
    got = got_ev.evaluation_data()
    assert sorted(got) == sorted(want)
    for k in want:
        R.same(got[k], want[k], k)
    assert R.alias_pattern(got) == R.alias_pattern(want)
    R.same(got_ev.curr_drone_distances, env.eval_system.curr_drone_distances)
    R.same(got_ev.curr_cattle_vel, env.eval_system.curr_cattle_vel)
    R.same(got_ev.curr_time, env.eval_system.curr_time)
    env.close()
    b.close()
