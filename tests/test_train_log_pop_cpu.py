"""Host-only checks of the population training log (cattleherd/train_log.py PopulationEpisodeRing,
explained_variance_pop; ch_ep_ring_pop_*, ch_rollout_collect_pop_log, ch_explained_variance_pop): the ctypes struct
against the header, the Python class's ValueErrors on the CPU stand-in batch, the entry points' rejections (everything
here is rejected before any launch: no GPU), and the numpy restatement of the summary's fixed summation order against
np.mean."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_log_pop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_the_header():
    from cattleherd import _lib
    src = open(os.path.join(ROOT, "include", "cattleherd.h")).read()
    body = re.search(r"typedef struct ch_ep_ring_pop \{(.*?)\} ch_ep_ring_pop;", src, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t\*|int32_t\*|double\*)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in _lib.ChEpRingPop._fields_]
    off = 0
    for ctype, name in fields:
        size = 4 if ctype == "int32_t" else 8
        off = (off + size - 1) // size * size
        assert getattr(_lib.ChEpRingPop, name).offset == off and getattr(_lib.ChEpRingPop, name).size == size, name
        off += size
    assert ctypes.sizeof(_lib.ChEpRingPop) == off == 40
    assert int(re.search(r"#define CH_EP_RING_POP_SUMMARY (\d+)", src).group(1)) == _lib.CH_EP_RING_POP_SUMMARY == 4
    L = _lib.lib()
    for name in _lib._TRAIN_LOG_POP_EXPORTS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name


def test_population_ring_value_errors_and_views_on_the_stand_in_batch():
    from fake_batch import FakeBatch
    from cattleherd.train_log import PopulationEpisodeRing
    b = FakeBatch(6, 2, 8, mode="ctde")
    with pytest.raises(ValueError, match="CTDE"):
        PopulationEpisodeRing(FakeBatch(4, 2, 8, mode="marl"), 2)
    for window in (0, -3):
        with pytest.raises(ValueError, match="window"):
            PopulationEpisodeRing(b, 3, window=window)
    for members in (4, 5, 0, 7):
        with pytest.raises(ValueError, match="divide"):
            PopulationEpisodeRing(b, members)
    ring = PopulationEpisodeRing(b, 3, window=5)
    assert ring.member_envs == 2 and ring.window == 5 and ring.n_members == 3
    assert tuple(ring.ep_return.shape) == tuple(ring.ep_length.shape) == tuple(ring.ep_env.shape) == (3, 5)
    assert tuple(ring.total.shape) == (3,) and ring._ring.window == 5 and ring._ring.n_members == 3
    for k in ("ep_return", "ep_length", "ep_env", "total"):
        t = getattr(ring, k)
        assert getattr(ring._ring, k) == t.data_ptr() and t.data_ptr() % t.element_size() == 0
    # the views tile one buffer: entries_all is one copy
    lo, hi = ring._buf.data_ptr(), ring._buf.data_ptr() + ring._buf.numel()
    spans = sorted((getattr(ring, k).data_ptr(), getattr(ring, k).numel() * getattr(ring, k).element_size())
                   for k in ("ep_return", "ep_length", "ep_env", "total"))
    assert spans[0][0] == lo and all(a + n == c for (a, n), (c, _) in zip(spans, spans[1:])) and sum(spans[-1]) == hi
    # the host half of the readers, on a hand-filled buffer: member 1 has wrapped, member 2 is empty
    ring.total[:] = ring.total.new_tensor([2, 7, 0])
    ring.ep_return[1] = ring.ep_return.new_tensor([10.0, 11.0, 12.0, 13.0, 14.0])
    ring.ep_length[1] = ring.ep_length.new_tensor([5, 6, 7, 8, 9])
    ring.ep_return[0, :2] = ring.ep_return.new_tensor([1.23456749, -2.0])
    ring.ep_length[0, :2] = ring.ep_length.new_tensor([3, 4])
    got = ring.entries_all()
    assert [len(g) for g in got] == [2, 5, 0] and ring.count() == [2, 7, 0]
    assert [e[0] for e in got[1]] == [12.0, 13.0, 14.0, 10.0, 11.0] and [e[1] for e in got[1]] == [7, 8, 9, 5, 6]
    assert ring.entries(0) == got[0] and ring.summary(2) == {}
    assert ring.summary(0) == {"rollout/ep_rew_mean": float(np.mean([1.234567, -2.0])), "rollout/ep_len_mean": 3.5}


def _ring(window=8, members=2):
    from cattleherd import _lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    r = _lib.ChEpRingPop()
    r.window, r.n_members, r.ep_return, r.ep_length, r.ep_env, r.total = window, members, p, p, p, p
    return r, buf


def test_entry_points_reject_bad_arguments_before_any_launch():
    from cattleherd import _lib
    from cattleherd.rollout_pop import _bind
    L = _bind()
    INV = _lib.CH_ERR_INVALID
    io = _lib.ChStepIO()
    out = (ctypes.c_double * 8)()
    ring, _keep = _ring()
    calls = (("ch_ep_ring_pop_begin", lambda r: L.ch_ep_ring_pop_begin(None, r, None)),
             ("ch_ep_ring_pop_record", lambda r: L.ch_ep_ring_pop_record(None, r, ctypes.byref(io), None)),
             ("ch_ep_ring_pop_summary", lambda r: L.ch_ep_ring_pop_summary(r, out, None)))
    for name, fn in calls:
        assert fn(None) == INV
        assert L.ch_last_error(None) == name.encode() + b": NULL ring"
        for kw, word in ((dict(window=0), b"window"), (dict(window=-1), b"window"), (dict(members=0), b"n_members")):
            bad, _k = _ring(**kw)
            assert fn(ctypes.byref(bad)) == INV
            assert L.ch_last_error(None).startswith(name.encode() + b": ") and word in L.ch_last_error(None)
        for field in ("ep_return", "ep_length", "ep_env", "total"):
            bad, _k = _ring()
            setattr(bad, field, None)
            assert fn(ctypes.byref(bad)) == INV and b"ring array" in L.ch_last_error(None)
    for name, fn in calls[:2]:     # whole rings, no handle
        assert fn(ctypes.byref(ring)) == INV and b"NULL handle" in L.ch_last_error(None)
    assert L.ch_ep_ring_pop_record(None, ctypes.byref(ring), None, None) == INV
    assert L.ch_last_error(None) == b"ch_ep_ring_pop_record: NULL step io"
    assert L.ch_ep_ring_pop_summary(ctypes.byref(ring), None, None) == INV
    assert L.ch_last_error(None) == b"ch_ep_ring_pop_summary: NULL out_dev"
    assert L.ch_rollout_collect_pop_log(None, None, None, 1, None, 1, ctypes.byref(ring), None) == INV
    assert L.ch_last_error(None).startswith(b"ch_rollout_collect_pop")
    # the explained variances
    p = ctypes.addressof(out)
    assert L.ch_explained_variance_pop_scratch(0, 3) == -1 and L.ch_explained_variance_pop_scratch(5, 0) == -1
    assert L.ch_last_error(None).startswith(b"ch_explained_variance_pop_scratch: ")
    for n in (1, 456, 8229, 1 << 24):
        assert L.ch_explained_variance_pop_scratch(n, 3) == 3 * L.ch_explained_variance_scratch(n)
    for args in ((None, p, 2, 4, p, p), (p, None, 2, 4, p, p), (p, p, 2, 4, None, p), (p, p, 2, 4, p, None)):
        assert L.ch_explained_variance_pop(*args, None) == INV
        assert L.ch_last_error(None) == b"ch_explained_variance_pop: NULL argument"
    for members in (0, -1, 65536):
        assert L.ch_explained_variance_pop(p, p, members, 4, p, p, None) == INV and b"n_members" in L.ch_last_error(None)
    for n in (0, -3):
        assert L.ch_explained_variance_pop(p, p, 2, n, p, p, None) == INV
        assert L.ch_last_error(None) == b"ch_explained_variance_pop: n < 1"


def test_explained_variance_pop_value_errors():
    import torch
    from cattleherd.train_log import explained_variance_pop
    a = torch.zeros(8)
    with pytest.raises(ValueError):
        explained_variance_pop([], [])
    with pytest.raises(ValueError):
        explained_variance_pop([a], [a, a])
    with pytest.raises(ValueError):
        explained_variance_pop([a], [a])          # not on a CUDA device


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100])
def test_fixed_summation_order_agrees_with_np_mean(n):
    """|restated mean - np.mean| <= n * eps * sum(|x|) / n with eps = 2^-52: each of the n - 1 additions of either
    order rounds a partial sum no larger than sum(|x|) by at most eps / 2 of it, so the two sums differ by at most
    (n - 1) eps sum(|x|); each division by n adds eps / 2 of a quotient no larger than sum(|x|) / n."""
    rng = np.random.default_rng(n)
    eps = float(np.finfo(np.float64).eps)
    for trial in range(20):
        x = rng.normal(0.0, 100.0, n) * 10.0 ** rng.integers(-3, 4)
        got = R.fixed_order_sum(x) / n
        assert abs(got - np.mean(x)) <= n * eps * np.sum(np.abs(x)) / n, (n, trial)
    # the order is fixed, and it is the stated one: 64 partial sums of stride 64, then the tree
    x = rng.normal(0.0, 1.0, n)
    s = [sum(x[t::64], 0.0) for t in range(64)]
    while len(s) > 1:
        s = [a + b for a, b in zip(s[:len(s) // 2], s[len(s) // 2:])]
    assert R.fixed_order_sum(x) == s[0]
    assert R.fitness_ref([[], [(2.0, 3, 0)]], [0, 9]).tolist()[1] == [1.0, 2.0, 3.0, 9.0]
    assert np.isnan(R.fitness_ref([[]], [0])[0, 1:3]).all() and R.fitness_ref([[]], [0])[0, 0] == 0.0
