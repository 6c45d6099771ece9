"""CPU tests of the on-device evaluate_policy's host side (cattleherd/eval_policy.py, ch_eval_* in the built library):
the SB3 bookkeeping reference itself on hand-written sequences, the quota rule, EvalCallback's evaluations.npz, and the
entry points' rejections that need no device."""
import ctypes

import numpy as np
import pytest

from eval_ref import EvalRef


def _step(ref, t, ended, stats=None, term=(), trunc=()):
    """One step in which the envs in ``ended`` finish an episode (return 10 e + t, length t + 1 unless ``stats``)."""
    E = ref.E
    rh = np.zeros(E, np.uint8)
    rh[list(ended)] = 1
    st = np.zeros((E, 2))
    for e in ended:
        st[e] = (10.0 * e + t, t + 1) if stats is None else stats[e]
    te, tr = np.zeros(E, np.uint8), np.zeros(E, np.uint8)
    te[list(term)] = 1
    tr[list(trunc)] = 1
    ref.step(rh, st, te, tr, t)


def test_ref_env_ending_twice_with_quota_one():
    ref = EvalRef(2, 2, 1)
    assert ref.targets.tolist() == [1, 1] and ref.remaining == 2
    _step(ref, 0, [0], trunc=[0])
    assert ref.counts.tolist() == [1, 0] and ref.remaining == 1 and ref.running()
    _step(ref, 1, [0], term=[0])          # env 0 again: at its target, not counted
    assert ref.counts.tolist() == [1, 0] and ref.remaining == 1 and ref.ignored_full == 1
    _step(ref, 2, [])
    _step(ref, 3, [1], term=[1], trunc=[1])
    assert not ref.running() and ref.remaining == 0
    r, n, f, env, end = ref.episodes()
    assert r.tolist() == [0.0, 13.0] and n.tolist() == [1, 4] and f.tolist() == [2, 3]
    assert env.tolist() == [0, 1] and end.tolist() == [0, 3]
    a = ref.arrays()
    assert a["ep_return"].tolist() == [[0.0], [13.0]] and a["ep_end_step"].tolist() == [[0], [3]]
    assert a["remaining"].tolist() == [0] and a["count"].dtype == np.int32


def test_ref_fewer_episodes_than_envs():
    """n < E: the first E - n envs have quota 0 and never contribute, however often they end."""
    ref = EvalRef(2, 5, 1)
    assert ref.targets.tolist() == [0, 0, 0, 1, 1]
    _step(ref, 0, [0, 1, 2])
    assert ref.remaining == 2 and ref.episode_rewards == [] and (ref.ignored_zero, ref.ignored_full) == (3, 0)
    _step(ref, 1, [0, 4])
    _step(ref, 2, [3])
    assert not ref.running()
    assert ref.episodes()[3].tolist() == [4, 3] and ref.episodes()[0].tolist() == [41.0, 32.0]


def test_ref_same_step_orders_by_env_and_fills_two_slots():
    ref = EvalRef(5, 3, 2)
    assert ref.targets.tolist() == [1, 2, 2]
    _step(ref, 0, [2, 1])                 # two envs in one step: appended by env index
    _step(ref, 1, [0, 1, 2])
    assert not ref.running()
    r, n, f, env, end = ref.episodes()
    assert env.tolist() == [1, 2, 0, 1, 2] and end.tolist() == [0, 0, 1, 1, 1]
    assert ref.arrays()["ep_return"].tolist() == [[1.0, 0.0], [10.0, 11.0], [20.0, 21.0]]
    assert ref.arrays()["count"].tolist() == [1, 2, 2]


def test_quota_helper_is_sb3s_rule():
    from cattleherd.eval_policy import episode_quota
    for E in (1, 2, 5, 64):
        for n in range(1, 3 * E + 2):
            q = episode_quota(n, E)
            assert q.dtype == np.int32 and q.tolist() == [(n + i) // E for i in range(E)]
            assert q.sum() == n and q.tolist() == EvalRef(n, E, int(q.max())).targets.tolist()


def test_eval_log_round_trips(tmp_path):
    from cattleherd.eval_policy import EvalLog
    log = EvalLog()
    log.add(1000, [1.5, -2.0, 3.25], [602, 17, 602])
    log.add(2000, [0.5, 0.25, -1.0], [10, 20, 30])
    path = tmp_path / "evaluations.npz"
    log.save(str(path))
    d = np.load(str(path))
    assert sorted(d.files) == ["ep_lengths", "results", "timesteps"]
    assert d["timesteps"].tolist() == [1000, 2000]
    assert d["results"].shape == (2, 3) and d["results"].tolist() == [[1.5, -2.0, 3.25], [0.5, 0.25, -1.0]]
    assert d["ep_lengths"].shape == (2, 3) and d["ep_lengths"].tolist() == [[602, 17, 602], [10, 20, 30]]
    with pytest.raises(ValueError):
        log.add(3000, [1.0], [5])


def test_max_episode_steps_follows_the_level_table():
    """The default step cap's episode length: 602 steps at the 40 s levels, 1202 at the 80 s ones."""
    from types import SimpleNamespace as NS
    from cattleherd.eval_policy import max_episode_steps
    mk = lambda lvl: NS(cfg=NS(curriculum_level=lvl, ctrl_freq=60, pyb_freq=240))  # noqa: E731
    assert max_episode_steps(mk(2)) == 602 and max_episode_steps(mk(7)) == 1202 and max_episode_steps(mk(-1)) == 1202


def test_entry_points_reject_null_arguments_without_a_device():
    """ch_eval_begin / ch_eval_record / ch_evaluate_policy reject a NULL table or handle on entry, with the reason in
    ch_last_error(NULL) (no device needed, as test_abi_cpu's null-handle checks)."""
    from cattleherd import _lib
    L = _lib.lib()
    tb = _lib.ChEvalTable()
    io = _lib.ChStepIO()
    steps, rem = ctypes.c_int64(), ctypes.c_int64()
    calls = {
        "ch_eval_begin": lambda t: L.ch_eval_begin(None, t, 5, None),
        "ch_eval_record": lambda t: L.ch_eval_record(None, t, ctypes.byref(io), 0, None),
        "ch_evaluate_policy": lambda t: L.ch_evaluate_policy(None, None, t, None, 10, 1, 0, ctypes.byref(steps),
                                                             ctypes.byref(rem), None),
    }
    for name, call in calls.items():
        assert call(None) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None) == (name + ": NULL table").encode()
        assert call(ctypes.byref(tb)) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None) == (name + ": NULL handle").encode()


def test_evaluate_policy_rejects_an_unbounded_loop_without_a_device():
    from cattleherd import _lib
    L = _lib.lib()
    tb = _lib.ChEvalTable()
    steps, rem = ctypes.c_int64(7), ctypes.c_int64(7)
    args = lambda max_steps, check_every: (None, None, ctypes.byref(tb), None, max_steps, check_every, 0,  # noqa: E731
                                           ctypes.byref(steps), ctypes.byref(rem), None)
    for bad in (0, -3):
        assert L.ch_evaluate_policy(*args(bad, 16)) == _lib.CH_ERR_INVALID
        assert b"max_steps must be >= 1" in L.ch_last_error(None)
        assert L.ch_evaluate_policy(*args(100, bad)) == _lib.CH_ERR_INVALID
        assert b"check_every must be >= 1" in L.ch_last_error(None)
    assert steps.value == 7 and rem.value == 7   # nothing ran
