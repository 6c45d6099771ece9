"""Host-only checks of the SB3 training log (cattleherd/train_log.py; ch_ep_ring_*, ch_ppo_train_log,
ch_explained_variance): the ring's slot rule against SB3's deque, the summary's rounding and means, the entry points'
rejections (everything here is rejected before any launch: no GPU), and the data conditions of the GPU test's
minibatches, which depend on the float64 reference alone.

test_slot_rule_equals_the_deque and test_update_cases_meet_the_clip_conditions check only the references of
tests/train_log_ref.py (the numpy slot rule against the deque, the float64 minibatches against ppo_native_ref's clip
conditions): they run none of the library's code.  The other tests here need cattleherd.train_log and the new entry
points."""
import ctypes
import types

import numpy as np
import pytest

from train_log_ref import DequeRef, RingSim, same_entries


def _random_steps(rng, E, W, steps):
    """Ended-masks whose counts cover C = 0, 1, C > W and a wrap over several steps."""
    counts = [0, 1, W + 3, 0, 2, W, W - 1, 3 * W + 1] + list(rng.integers(0, 2 * W + 2, steps))
    for C in counts:
        C = min(int(C), E)
        rh = np.zeros(E, np.uint8)
        rh[rng.choice(E, C, replace=False)] = 1
        stats = np.stack([rng.normal(0.0, 100.0, E), rng.integers(1, 1203, E).astype(np.float64)], -1)
        yield rh, stats


@pytest.mark.parametrize("W,E", [(1, 5), (8, 64), (100, 1100), (7, 300)])
def test_slot_rule_equals_the_deque(W, E):
    rng = np.random.default_rng(100 * W + E)
    ref, ring = DequeRef(W), RingSim(W)
    seen = set()
    for rh, stats in _random_steps(rng, E, W, 12):
        ref.step(rh, stats)
        ring.step(rh, stats)
        assert ring.writers.max() <= 1                 # plain stores suffice: one writer per slot
        assert ring.total == ref.total
        assert same_entries(ring.entries(), ref.entries())
        C = ref.per_step[-1]
        seen |= {"zero"} if C == 0 else {"over"} if C > W else {"some"}
    assert seen == {"zero", "some", "over"} and ref.total > 3 * W


def test_summary_rounds_the_returns_and_takes_plain_means():
    from cattleherd.train_log import EpisodeRing, summary_of
    entries = [(1.23456749, 10, 0), (-2.00000051, 21, 3), (100.0, 1202, 1)]
    fake = types.SimpleNamespace(entries=lambda: entries)
    got = EpisodeRing.summary(fake)
    assert set(got) == {"rollout/ep_rew_mean", "rollout/ep_len_mean"}
    assert got["rollout/ep_rew_mean"] == float(np.mean([1.234567, -2.000001, 100.0]))   # Monitor's round(r, 6)
    assert got["rollout/ep_rew_mean"] != float(np.mean([e[0] for e in entries]))
    assert got["rollout/ep_len_mean"] == float(np.mean([10, 21, 1202]))
    assert summary_of([]) == {}        # SB3 logs neither key while ep_info_buffer is empty


def _ring(window=8):
    from cattleherd import _lib
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    r = _lib.ChEpRing()
    r.window, r.ep_return, r.ep_length, r.ep_env, r.total = window, p, p, p, p
    return r, buf


def test_ring_entry_points_reject_bad_arguments():
    from cattleherd import _lib
    from cattleherd.rollout import _bind
    L = _bind()
    ring, _keep = _ring()
    io = _lib.ChStepIO()
    for fn, args in ((L.ch_ep_ring_begin, ()), (L.ch_ep_ring_record, (ctypes.byref(io),))):
        name = b"ch_ep_ring_begin: " if not args else b"ch_ep_ring_record: "
        assert fn(None, None, *args, None) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None).startswith(name)
        bad, _k = _ring(window=0)
        assert fn(None, ctypes.byref(bad), *args, None) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None).startswith(name) and b"window" in L.ch_last_error(None)
        for field in ("ep_return", "ep_length", "ep_env", "total"):
            bad, _k = _ring()
            setattr(bad, field, None)
            assert fn(None, ctypes.byref(bad), *args, None) == _lib.CH_ERR_INVALID
            assert b"ring array" in L.ch_last_error(None)
        assert fn(None, ctypes.byref(ring), *args, None) == _lib.CH_ERR_INVALID      # a whole ring, no handle
        assert b"NULL handle" in L.ch_last_error(None)
    assert L.ch_ep_ring_record(None, ctypes.byref(ring), None, None) == _lib.CH_ERR_INVALID
    assert L.ch_last_error(None) == b"ch_ep_ring_record: NULL step io"
    assert L.ch_rollout_collect_log(None, None, None, None, None, None, 0, 0.99, 0.95, 1, ctypes.byref(ring), None) == _lib.CH_ERR_INVALID
    assert L.ch_last_error(None).startswith(b"ch_rollout_collect")


def test_train_log_rejects_like_train_and_needs_its_stats():
    from cattleherd import _lib, ppo
    from test_ppo_native_cpu import _net
    lib = ppo._bind()
    assert _lib.CH_PPO_LOG_STATS == 6
    assert lib.ch_ppo_train_log(None, None, None, None, 1, 1, None, None, None, None, None, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None) == b"ch_ppo_train_log: NULL argument"
    hp, data = ppo.ChPpoHparams(), ppo.ChPpoData()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    net = _net()
    # everything but the statistics: ch_ppo_train takes that, ch_ppo_train_log does not
    assert lib.ch_ppo_train_log(ctypes.byref(net), ctypes.byref(hp), ctypes.byref(data), p, 1, 1, p, p, p, None, p, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None) == b"ch_ppo_train_log: NULL argument"
    # non-NULL arguments that are never read: an unsupported net is rejected before any pointer is used
    bad = _net(pi=(300, 128))
    assert lib.ch_ppo_train_log(ctypes.byref(bad), ctypes.byref(hp), ctypes.byref(data), p, 1, 1, p, p, p, p, p, None) == _lib.CH_ERR_UNSUPPORTED
    assert lib.ch_last_error(None).startswith(b"ch_ppo_train_log: ")
    # a supported net whose weight pointers are NULL, and bad sizes
    assert lib.ch_ppo_train_log(ctypes.byref(net), ctypes.byref(hp), ctypes.byref(data), p, 1, 1, p, p, p, p, p, None) == _lib.CH_ERR_INVALID
    assert b"NULL weight" in lib.ch_last_error(None)
    # the scratch holds the two diagnostics' partials too, and still answers -1 for bad input
    assert lib.ch_ppo_scratch_size(ctypes.byref(net), 64) > lib.ch_ppo_param_count(ctypes.byref(net))
    assert lib.ch_ppo_scratch_size(ctypes.byref(net), 0) == -1


def test_explained_variance_rejects_bad_arguments():
    from cattleherd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    assert L.ch_explained_variance_scratch(0) == -1
    assert L.ch_last_error(None) == b"ch_explained_variance_scratch: n < 1"
    assert 4 <= L.ch_explained_variance_scratch(1) <= L.ch_explained_variance_scratch(1 << 24) <= 4096
    for args in ((None, p, 4, p, p), (p, None, 4, p, p), (p, p, 4, None, p), (p, p, 4, p, None)):
        assert L.ch_explained_variance(*args, None) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None) == b"ch_explained_variance: NULL argument"
    for n in (0, -3):
        assert L.ch_explained_variance(p, p, n, p, p, None) == _lib.CH_ERR_INVALID
        assert L.ch_last_error(None) == b"ch_explained_variance: n < 1"


def test_log_stats_needs_the_native_backend():
    from cattleherd import ppo
    model = ppo.SB3ActorCritic(obs_dim=172, act_dim=8, pi=(32,), vf=(32,), device="cpu")
    with pytest.raises(ValueError, match="log_stats"):
        ppo.PPOUpdate(model, graph=False, backend="torch", log_stats=True)
    upd = ppo.PPOUpdate(model, graph=False, backend="torch")
    assert upd.log_stats is False and upd.last_log == {}
    assert len(ppo.PPOUpdate.LOG_KEYS) == 10 and all(k.startswith("train/") for k in ppo.PPOUpdate.LOG_KEYS)


def test_update_cases_meet_the_clip_conditions():
    """The GPU test's minibatch sequences, on the float64 reference alone (each step from the weights it starts from):
    no ratio within 1e-3 of a clip edge, and in minibatches of 8 rows and more both edges occur."""
    import torch
    import ppo_native_ref as R
    import train_log_ref as T
    data64 = R.make_data(R.DRIVER, "cpu")
    for name, batch in T.UPDATE_CASES:
        m64 = R.make_model(R.DRIVER, "cpu", torch.float64)
        steps = T.update_reference(m64, data64, T.update_case_idx(name, batch), batch, R.HP)
        assert len(steps) == (2 if name == "partial" else 1)
        for st, akl, count, ratio, clipped in steps:
            R.check_clip_conditions(ratio, clipped)
            assert torch.isfinite(st).all() and float(akl) > 0 and 0 <= count <= ratio.numel()
        assert steps[-1][3].numel() == (32 if name == "partial" else batch)
