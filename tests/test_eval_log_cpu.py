"""CPU tests of the device-side evaluator log's host half (cattleherd.eval_log): the replay of the table into the
reference's ``Evaluator``, the constructor's refusals, the C entry points' argument checks that need no device, and the
directed states of tests/test_gpu_eval_log.py stepped on the CPU oracle."""
import ctypes
import types

import numpy as np
import pytest

from cattleherd.evaluation import EvalTracker, Evaluator, herding_effectiveness
from eval_log_ref import alias_pattern as _alias_pattern, same as _same

N, M, LEN, FREQ = 3, 4, 40, 60


def _state(rng, n, centre, spread=0.8):
    """One env's state as EvalTracker reads it: n live drones in a ring about ``centre``, M cows inside it."""
    ang = 2 * np.pi * np.arange(n) / n + rng.uniform(0, 1)
    s = {"drone_pos": np.zeros((1, N, 3)), "drone_vel": rng.normal(0, 0.1, (1, N, 3)),
         "cow_pos": (centre + rng.uniform(-spread, spread, (M, 2)))[None], "cow_vel": rng.normal(0, 0.05, (1, M, 2))}
    s["drone_pos"][0, :n, :2] = centre + 2.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    s["drone_pos"][0, :, 2] = 0.45
    return s


def _script():
    """Resets and steps of one env over three episodes.  Episode 0 (2 drones) runs into the time limit: its last step
    starts past EPISODE_LEN_SEC with the formation intact -- the time-out trigger.  Episode 1 (3 drones) ends in a
    failure truncation (drones 0 and 1 0.1 m apart) on a step that also starts past the limit: no trigger.  Episode 2
    logs one more step.  Returns the events and, per step, (episode, flags) as the device would log them."""
    rng = np.random.default_rng(5)
    ev, meta = [], []
    lim = LEN * FREQ
    ev.append(("reset", _state(rng, 2, np.array([1.0, -2.0])), 2))
    for sc, flags in ((lim - 8, 0), (lim - 4, 0), (lim, 0), (lim + 4, 2 | 4)):   # (lim / FREQ is not > LEN)
        ev.append(("step", _state(rng, 2, np.array([1.0, -2.0])), rng.uniform(0, 5, N), sc, 2))
        meta.append((0, flags))
    ev.append(("reset", _state(rng, 3, np.array([-3.0, 0.5])), 3))
    for sc, flags in ((0, 0), (4, 0), (lim + 8, 2)):
        s = _state(rng, 3, np.array([-3.0, 0.5]))
        if flags:
            s["drone_pos"][0, 1, :2] = s["drone_pos"][0, 0, :2] + (0.1, 0.0)
        ev.append(("step", s, rng.uniform(0, 5, N), sc, 3))
        meta.append((1, flags))
    ev.append(("reset", _state(rng, 2, np.array([0.0, 0.0])), 2))
    ev.append(("step", _state(rng, 2, np.array([0.0, 0.0])), rng.uniform(0, 5, N), 0, 2))
    meta.append((2, 0))
    return ev, meta


def _tracker_evaluator(events):
    ev = Evaluator()
    tr = EvalTracker(ev)
    for e in events:
        if e[0] == "reset":
            tr.on_reset(e[1], e[2])
        else:
            _, s, dist, sc, n = e
            tr.after_step(s, dist, n, M, sc, FREQ, LEN)
    return ev


def _arrays(events, meta):
    """The same steps as one logged env's rows of DeviceEvalLog.arrays()."""
    steps = [e for e in events if e[0] == "step"]
    T = len(steps)
    a = {"sel_env": np.zeros(1, np.int32), "rows": np.full(1, T, np.int32), "dropped": np.zeros(1, np.int32),
         "time": np.zeros((1, T)), "effectiveness": np.zeros((1, T)), "num_drones": np.zeros((1, T), np.int32),
         "episode": np.zeros((1, T), np.int32), "flags": np.zeros((1, T), np.uint8),
         "drone_xy": np.zeros((1, T, N, 2)), "drone_vxy": np.zeros((1, T, N, 2)), "drone_dist": np.zeros((1, T, N)),
         "cattle_xy": np.zeros((1, T, M, 2)), "cattle_vxy": np.zeros((1, T, M, 2))}
    k, prev_vel = 0, None
    for e in events:
        if e[0] == "reset":
            prev_vel = e[1]["cow_vel"][0]
            continue
        _, s, dist, sc, n = e
        a["time"][0, k] = sc / FREQ
        a["effectiveness"][0, k] = herding_effectiveness(s["cow_pos"][0], s["drone_pos"][0, :n, :2])
        a["num_drones"][0, k] = n
        a["episode"][0, k], a["flags"][0, k] = meta[k]
        a["drone_xy"][0, k, :n] = s["drone_pos"][0, :n, :2]
        a["drone_vxy"][0, k, :n] = s["drone_vel"][0, :n, :2]
        a["drone_dist"][0, k, :n] = dist[:n]
        a["cattle_xy"][0, k] = s["cow_pos"][0]
        a["cattle_vxy"][0, k] = prev_vel
        prev_vel = s["cow_vel"][0]
        k += 1
    return a


def test_to_evaluators_equals_the_tracker_fed_the_same_steps():
    from cattleherd.eval_log import evaluators_from_arrays
    events, meta = _script()
    want = _tracker_evaluator(events).evaluation_data()
    got_ev, = evaluators_from_arrays(_arrays(events, meta))
    got = got_ev.evaluation_data()
    assert sorted(got) == sorted(want)
    for k in want:
        _same(got[k], want[k], k)
    # the script is what its docstring says: one time-out (two episode entries, the second empty) and nothing else
    assert len(want["time_taken"]) == 2 and want["num_drones"] == [2, 2]
    assert [len(r) for r in want["time_per_step"]] == [3, 0]
    assert len(got_ev.curr_time) == len(_tracker_evaluator(events).curr_time) == 5   # the rows since the time-out
    _same(got_ev.curr_drone_poses, _tracker_evaluator(events).curr_drone_poses)
    _same(got_ev.curr_cattle_vel, _tracker_evaluator(events).curr_cattle_vel)
    # aliasing: every distance row of an episode is that episode's list; the time-out step's row is the old one
    assert _alias_pattern(got) == _alias_pattern(want)
    ref = _tracker_evaluator(events)
    pat = lambda e: _alias_pattern({"distances": [], "distances_per_step": e.curr_drone_distances})  # noqa: E731
    assert pat(got_ev) == pat(ref)
    _same(got_ev.curr_drone_distances, ref.curr_drone_distances)
    assert got_ev.curr_drone_distances[0] is got["distances"][0]        # logged into the next episode, old list
    assert got_ev.curr_drone_distances[1] is not got_ev.curr_drone_distances[0]
    assert got_ev.curr_drone_distances[1] is got_ev.curr_drone_distances[3]


def test_rows_beyond_the_count_are_ignored():
    from cattleherd.eval_log import evaluators_from_arrays
    events, meta = _script()
    a = _arrays(events, meta)
    a["rows"][0] = 3
    got, = evaluators_from_arrays(a)
    assert len(got.curr_time) == 3 and got.total_time_taken == []


def _stub(mode=0, eval_metrics=1, n_envs=12):
    return types.SimpleNamespace(mode=mode, cfg=types.SimpleNamespace(eval_metrics=eval_metrics), n_envs=n_envs,
                                 num_drones=4, num_cattle=16)


@pytest.mark.parametrize("kw,envs,capacity,match", [
    ({}, [0, 3, 3], 4, "distinct"), ({}, [0, 12], 4, r"\[0, 12\)"), ({}, [-1], 4, r"\[0, 12\)"), ({}, [], 4, "at least"),
    ({"mode": 1}, [0], 4, "CTDE"), ({"eval_metrics": 0}, [0], 4, "eval_metrics"), ({}, [0], 0, "capacity")])
def test_constructor_refusals(kw, envs, capacity, match):
    """Refused before anything is allocated (no device needed)."""
    from cattleherd.eval_log import DeviceEvalLog
    with pytest.raises(ValueError, match=match):
        DeviceEvalLog(_stub(**kw), envs, capacity)


def test_entry_points_reject_null_arguments_without_a_device():
    from cattleherd import _lib
    L = _lib.lib()
    lg = _lib.ChEvalLog()
    io = _lib.ChEvalLogIO()
    net = _lib.ChMlp()
    assert ctypes.sizeof(_lib.ChEvalLog) == 8 + 15 * 8 and ctypes.sizeof(_lib.ChEvalLogIO) == 4 * 8
    for call, name in ((lambda: L.ch_eval_log_begin(None, ctypes.byref(lg), None), b"ch_eval_log_begin"),
                       (lambda: L.ch_eval_log_mark(None, ctypes.byref(lg), None), b"ch_eval_log_mark"),
                       (lambda: L.ch_eval_log_record(None, ctypes.byref(lg), None, None), b"ch_eval_log_record"),
                       (lambda: L.ch_eval_log_begin(None, None, None), b"ch_eval_log_begin"),
                       (lambda: L.ch_eval_log_run(None, ctypes.byref(net), ctypes.byref(lg), ctypes.byref(io), 4, None),
                        b"ch_eval_log_run"),
                       (lambda: L.ch_eval_log_run(None, ctypes.byref(net), ctypes.byref(lg), ctypes.byref(io), 0, None),
                        b"ch_eval_log_run: n_steps")):
        assert call() == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None).startswith(name)


# ---- the directed states of the GPU test, stepped on the CPU oracle ----------------------------------------------------
def _oracle_batch(E, n, m, level):
    from fake_batch import FakeBatch
    from helpers import stack

    class OracleBatch(FakeBatch):
        def get_state(self):   # (unsliced: set_state takes it back)
            return stack([env.get_state() for env in self.envs])

    b = OracleBatch(E, n, m, mode="ctde", curriculum_level=level)
    b.reset()
    return b


def test_directed_timeout_state_on_the_oracle():
    """4 x 16 at level 7 (80 s), step_counter 4790: the fourth step starts at 4802 / 60 > 80 with the formation intact --
    truncated with the time-out trigger; the next row belongs to the next episode; no comparison is within 1e-9 of
    its threshold."""
    import eval_log_ref as R
    b = _oracle_batch(2, 4, 16, 7)
    b.set_state(R.timeout_state(b.get_state(), 4, 16, 4790))
    rows, margins, done = R.reference_rows(b, [0, 1], np.zeros((7, 2, 4, 4), np.float32), 80)
    assert margins.min() >= 1e-9
    assert rows["flags"][:, :3].max() == 0 and np.all(rows["flags"][:, 3] == 2 | 4) and rows["flags"][:, 4:].max() == 0
    assert np.all(rows["episode"][:, 4] == rows["episode"][:, 3] + 1) and np.all(done[3]) and done.sum() == 2
    assert np.all(rows["time"][:, 4] == 0.0)


def test_directed_collision_state_on_the_oracle():
    """Drones 0 and 1 0.25 m apart on closing actions: a failure truncation (bit 1) without the trigger (bit 2) inside
    the window, early in the episode; margins as above."""
    import eval_log_ref as R
    b = _oracle_batch(2, 4, 16, 7)
    b.set_state(R.collision_state(b.get_state(), 4, 16))
    rows, margins, done = R.reference_rows(b, [0, 1], R.closing_actions(24, 2, 4), 80)
    assert margins.min() >= 1e-9
    assert np.all((rows["flags"] & 2).sum(axis=1) >= 1) and not np.any(rows["flags"] & 4)
    first = int(np.argmax(rows["flags"][0] & 2))
    assert 0 < first < 23 and rows["episode"][0, first + 1] == rows["episode"][0, first] + 1
