"""CPU tests of the DTDE evaluation's host side (cattleherd/marl_eval.py, ch_marl_eval_* in the built library): the
per-agent bookkeeping reference itself on hand-written sequences, the metrics dict, and the entry points' rejections
that need no device."""
import ctypes

import numpy as np
import pytest

from marl_eval_ref import MarlEvalRef


def _f32(x):
    return np.asarray(x, np.float32)


def test_ref_agent_dropping_out_two_steps_before_its_env_ends():
    """One env, 3 agents, 5 steps: agent 1 is live for the first 3 only (it terminated in step 2), the env ends in
    step 4.  Its length is 3 and the rewards at its slot in steps 3 and 4 are not summed."""
    ref = MarlEvalRef(1, 1, 3, 1)
    rewards = _f32([[1.0, 10.0, 100.0], [2.0, 20.0, 200.0], [3.0, 30.0, 300.0], [4.0, 4e6, 400.0],
                    [5.0, np.nan, 500.0]])
    for t in range(5):
        live = [1, 1 if t < 3 else 0, 1]
        ref.step(live, rewards[t], [1 if t == 4 else 0], t)
        if t < 4:
            assert ref.acc_steps.tolist() == [t + 1] and ref.remaining == 1
            assert ref.acc_length.tolist() == [[t + 1, min(t + 1, 3), t + 1]]
    a = ref.arrays()
    assert a["agent_return"].tolist() == [[[15.0, 60.0, 1500.0]]] and a["agent_length"].tolist() == [[[5, 3, 5]]]
    assert a["ep_return"].tolist() == [[1575.0]] and a["ep_length"].tolist() == [[5]] and a["ep_end_step"].tolist() == [[4]]
    assert a["count"].tolist() == [1] and a["remaining"].tolist() == [0] and not ref.running()
    assert not a["acc_return"].any() and not a["acc_length"].any() and not a["acc_steps"].any()
    assert a["live"].tolist() == [[1, 0, 1]] and a["live"].dtype == np.uint8
    assert a["agent_return"].dtype == np.float64 and a["agent_length"].dtype == np.int32
    r, n, ar, al, env, end = ref.episodes()
    assert r.tolist() == [1575.0] and n.tolist() == [5] and al.tolist() == [[5, 3, 5]] and env.tolist() == [0]
    assert n.dtype == np.int64 and al.dtype == np.int64 and end.tolist() == [4]


def test_ref_sums_float32_rewards_in_float64_step_order():
    """The adds are float64 adds of the float32 values one step at a time: 1e8 + 1 + 1 - 1e8 is 2 in float64 (0 in
    float32), and the float32 value of 0.1 enters, not the double 0.1."""
    ref = MarlEvalRef(1, 1, 2, 1)
    seq = _f32([[1e8, 0.1], [1.0, 0.1], [1.0, 0.1], [-1e8, 0.1]])
    for t in range(4):
        ref.step([1, 1], seq[t], [t == 3], t)
    want1 = ((np.float64(np.float32(0.1)) + np.float64(np.float32(0.1))) + np.float64(np.float32(0.1))) + \
        np.float64(np.float32(0.1))
    assert ref.agent_return[0, 0].tolist() == [2.0, want1] and want1 != 0.4
    assert ref.ep_return[0, 0] == (np.float64(0.0) + 2.0) + want1


def test_ref_env_ending_twice_with_quota_one():
    ref = MarlEvalRef(2, 2, 2, 1)
    assert ref.targets.tolist() == [1, 1] and ref.remaining == 2
    one = _f32(np.ones((2, 2)))
    ref.step([[1, 1], [1, 1]], one, [1, 0], 0)
    assert ref.counts.tolist() == [1, 0] and ref.remaining == 1 and ref.running()
    assert ref.acc_steps.tolist() == [0, 1] and ref.acc_return.tolist() == [[0.0, 0.0], [1.0, 1.0]]
    ref.step([[1, 0], [1, 1]], 2 * one, [1, 0], 1)      # env 0 again: at its target, ignored -- and zeroed all the same
    assert ref.counts.tolist() == [1, 0] and (ref.ignored_full, ref.ignored_zero) == (1, 0)
    assert ref.acc_steps.tolist() == [0, 2] and ref.acc_return[0].tolist() == [0.0, 0.0]
    assert ref.arrays()["ep_return"].tolist() == [[2.0], [0.0]] and ref.arrays()["ep_length"].tolist() == [[1], [0]]
    ref.step([[1, 1], [0, 1]], 3 * one, [0, 1], 2)
    assert not ref.running() and ref.remaining == 0
    r, n, ar, al, env, end = ref.episodes()
    assert r.tolist() == [2.0, 9.0] and n.tolist() == [1, 3] and env.tolist() == [0, 1] and end.tolist() == [0, 2]
    assert ar.tolist() == [[1.0, 1.0], [3.0, 6.0]] and al.tolist() == [[1, 1], [2, 3]]


def test_ref_fewer_episodes_than_envs():
    """n < E: the first E - n envs have quota 0 and never contribute, however often they end."""
    ref = MarlEvalRef(2, 5, 1, 1)
    assert ref.targets.tolist() == [0, 0, 0, 1, 1]
    live = np.ones((5, 1), np.uint8)
    ref.step(live, _f32(np.arange(5)[:, None]), [1, 1, 1, 0, 0], 0)
    assert ref.remaining == 2 and (ref.ignored_zero, ref.ignored_full) == (3, 0) and len(ref.episodes()[0]) == 0
    ref.step(live, _f32(np.arange(5)[:, None]), [1, 0, 0, 0, 1], 1)
    ref.step(live, _f32(np.arange(5)[:, None]), [0, 0, 0, 1, 0], 2)
    assert not ref.running() and ref.ignored_zero == 4
    r, n, ar, al, env, end = ref.episodes()
    assert env.tolist() == [4, 3] and r.tolist() == [8.0, 9.0] and n.tolist() == [2, 3] and end.tolist() == [1, 2]


def test_table_episodes_orders_by_end_step_then_env():
    from cattleherd.marl_eval import table_episodes
    ref = MarlEvalRef(5, 3, 2, 2)
    assert ref.targets.tolist() == [1, 2, 2]
    rng = np.random.default_rng(0)
    for t, ended in enumerate(([0, 1, 1], [0, 0, 0], [1, 1, 1])):
        ref.step(rng.random((3, 2)) < 0.7, _f32(rng.normal(size=(3, 2))), ended, t)
    got, want = table_episodes(ref.arrays(), 2), ref.episodes()
    assert want[4].tolist() == [1, 2, 0, 1, 2] and want[5].tolist() == [0, 0, 2, 2, 2]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_metrics_dict_from_a_hand_built_episode_list():
    """RLlib's names; an agent's mean is over the episodes it took part in (agent_length > 0), and an agent of no
    episode has no key."""
    from cattleherd.marl_eval import episode_metrics
    returns = [6.0, -3.0, 9.0]
    lengths = [10, 20, 60]
    agent_returns = [[1.0, 2.0, 3.0, 0.0], [-3.0, 0.0, 0.0, 0.0], [4.0, 5.0, 0.0, 0.0]]
    agent_lengths = [[10, 4, 10, 0], [20, 0, 0, 0], [60, 60, 0, 0]]
    m = episode_metrics(returns, lengths, agent_returns, agent_lengths)
    assert m == {"episode_return_mean": 4.0, "episode_return_min": -3.0, "episode_return_max": 9.0,
                 "episode_len_mean": 30.0, "num_episodes": 3,
                 "agent_episode_returns_mean": {"agent_0": 2.0 / 3.0, "agent_1": 3.5, "agent_2": 3.0}}
    assert all(type(m[k]) is float for k in m if k.startswith("episode_")) and type(m["num_episodes"]) is int
    with pytest.raises(ValueError):
        episode_metrics([], [], np.zeros((0, 4)), np.zeros((0, 4)))


def test_evaluate_needs_an_explicit_step_cap():
    """A truncation ends no MARL episode, so no cap follows from the time limit: max_steps=None is a ValueError,
    raised before the batch is touched."""
    from cattleherd.marl_eval import evaluate_marl_policy
    with pytest.raises(ValueError, match="max_steps is required"):
        evaluate_marl_policy(object(), object(), 5)


def test_struct_layout_matches_the_header():
    from cattleherd import _lib
    assert ctypes.sizeof(_lib.ChMarlEvalTable) == 8 + 12 * 8 and _lib.ChMarlEvalTable.quota.offset == 8
    assert _lib.ChMarlEvalTable.live.offset == 8 + 11 * 8
    assert ctypes.sizeof(_lib.ChMarlEvalIO) == 3 * 8
    assert _lib.ABI_VERSION == 6


def test_entry_points_reject_null_arguments_without_a_device():
    """ch_marl_eval_begin / _mark / _record / ch_marl_evaluate_policy reject a NULL table or handle on entry, with the
    reason in ch_last_error(NULL) (no device needed)."""
    from cattleherd import _lib
    L = _lib.lib()
    tb = _lib.ChMarlEvalTable()
    io = _lib.ChStepIO()
    steps, rem = ctypes.c_int64(), ctypes.c_int64()
    calls = {
        "ch_marl_eval_begin": lambda t: L.ch_marl_eval_begin(None, t, 5, None),
        "ch_marl_eval_mark": lambda t: L.ch_marl_eval_mark(None, t, None),
        "ch_marl_eval_record": lambda t: L.ch_marl_eval_record(None, t, ctypes.byref(io), 0, None),
        "ch_marl_evaluate_policy": lambda t: L.ch_marl_evaluate_policy(None, None, t, None, 10, 1, 0,
                                                                       ctypes.byref(steps), ctypes.byref(rem), None),
    }
    for name, call in calls.items():
        assert call(None) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None) == (name + ": NULL table").encode()
        assert call(ctypes.byref(tb)) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None) == (name + ": NULL handle").encode()


def test_evaluate_rejects_an_unbounded_loop_without_a_device():
    from cattleherd import _lib
    L = _lib.lib()
    tb = _lib.ChMarlEvalTable()
    steps, rem = ctypes.c_int64(7), ctypes.c_int64(7)
    args = lambda max_steps, check_every: (None, None, ctypes.byref(tb), None, max_steps, check_every, 0,  # noqa: E731
                                           ctypes.byref(steps), ctypes.byref(rem), None)
    for bad in (0, -3):
        assert L.ch_marl_evaluate_policy(*args(bad, 16)) == _lib.CH_ERR_INVALID
        assert b"max_steps must be >= 1" in L.ch_last_error(None)
        assert L.ch_marl_evaluate_policy(*args(100, bad)) == _lib.CH_ERR_INVALID
        assert b"check_every must be >= 1" in L.ch_last_error(None)
    assert steps.value == 7 and rem.value == 7   # nothing ran
