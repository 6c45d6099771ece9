"""CPU tests of the device-side VecNormalize's host half: the float64 reference (tests/vecnorm_ref.py) against numpy
over concatenated batches, the step order on a hand-made example, state_dict round trips, and the rejections that need
no device (the C ABI judges a ch_norm before it touches one)."""
import ctypes

import numpy as np
import pytest

import vecnorm_ref as R


def test_incremental_updates_equal_the_concatenation():
    """k updates with different batch sizes = numpy over the concatenation, the count = 1e-4 prior (mean 0, var 1)
    accounted for as 1e-4 of a sample at 0 with variance 1; 1e-12 relative."""
    rng = np.random.default_rng(0)
    dim = 7
    batches = [rng.normal(size=(n, dim)) * np.logspace(-3, 3, dim) + rng.uniform(-1e3, 1e3, dim) for n in (5, 1, 64, 33)]
    rms = R.RunningMeanStd((dim,))
    for b in batches:
        rms.update(b)
    x = np.concatenate(batches)
    n, c0 = x.shape[0], 1e-4
    tot = c0 + n
    mean = x.mean(0) * n / tot
    var = (c0 * (1.0 + mean ** 2) + n * (x.var(0) + (x.mean(0) - mean) ** 2)) / tot
    assert rms.count == pytest.approx(tot, rel=1e-15)
    assert np.allclose(rms.mean, mean, rtol=1e-12, atol=0)
    assert np.allclose(rms.var, var, rtol=1e-12, atol=0)


def test_step_order_on_three_envs():
    """Update before apply; the reward normalised with the updated return variance, ret zeroed after it; the terminal
    observation normalised with the post-update statistics and kept out of the update."""
    v = R.VecNormalize(3, (2,), gamma=0.5, clip_obs=1.5, clip_reward=10.0)
    obs0 = np.array([[0.0, 1.0], [2.0, 1.0], [4.0, 1.0]], np.float32)
    o0 = v.reset(obs0)
    rms = R.RunningMeanStd((2,))
    rms.update(obs0)
    assert np.array_equal(v.obs_rms.mean, rms.mean) and v.obs_rms.count == 3 + 1e-4
    want = np.clip((obs0 - rms.mean) / np.sqrt(rms.var + 1e-8), -1.5, 1.5).astype(np.float32)
    assert np.array_equal(o0, want) and o0[0, 0] < 0 < o0[2, 0]
    assert np.all(v.ret == 0)

    obs1 = np.array([[1.0, 1.0], [3.0, 1.0], [5.0, 1.0]], np.float32)
    term = np.array([[9.0, 9.0], [100.0, -100.0], [9.0, 9.0]], np.float32)
    rew = np.array([1.0, 2.0, 3.0], np.float32)
    done = np.array([False, True, False])
    before = v.obs_rms.mean.copy()
    o1, r1, t1 = v.step(obs1, rew, done, term)
    rms.update(obs1)   # the terminal observation is not in it
    assert np.array_equal(v.obs_rms.mean, rms.mean) and not np.array_equal(rms.mean, before)
    sd = np.sqrt(rms.var + 1e-8)
    assert np.array_equal(o1, np.clip((obs1 - rms.mean) / sd, -1.5, 1.5).astype(np.float32))   # post-update statistics
    assert np.array_equal(t1, np.clip((term[1:2] - rms.mean) / sd, -1.5, 1.5).astype(np.float32))
    assert np.array_equal(t1, np.array([[1.5, -1.5]], np.float32))   # clipped
    ret_rms = R.RunningMeanStd(())
    ret_rms.update(np.array([1.0, 2.0, 3.0]))   # ret = 0 * gamma + reward, done env included
    assert v.ret_rms.var == ret_rms.var
    assert np.array_equal(r1, (rew / np.sqrt(ret_rms.var + 1e-8)).astype(np.float32))
    assert np.array_equal(v.ret, [1.0, 0.0, 3.0])   # zeroed after the reward was normalised

    o2, r2, _ = v.step(obs1, rew, np.array([False, True, True]), term)
    ret_rms.update(np.array([1.5, 2.0, 4.5]))   # env 1 started again from 0
    assert v.ret_rms.var == ret_rms.var and np.array_equal(v.ret, [1.5, 0.0, 0.0])

    v.training = False
    s = v.state_dict()
    v.step(obs1 * 3, rew, done, term)
    assert np.array_equal(v.obs_rms.mean, s["obs_mean"]) and v.ret_rms.var == s["ret_var"]
    assert np.array_equal(v.ret, [1.5, 0.0, 0.0])   # not advanced; zeroed where done

    w = R.VecNormalize(3, (2,), norm_reward=False)
    _, rw, _ = w.step(obs1, rew, done)
    assert np.array_equal(rw, rew) and w.ret_rms.count == 3 + 1e-4   # raw reward out, ret_rms still moves


def test_reference_state_dict_round_trip():
    rng = np.random.default_rng(1)
    a = R.VecNormalize(4, (3,), gamma=0.9, clip_obs=5.0)
    a.reset(rng.normal(size=(4, 3)))
    a.step(rng.normal(size=(4, 3)), rng.normal(size=4), np.array([0, 1, 0, 0], bool))
    b = R.VecNormalize(4, (3,)).load_state_dict(a.state_dict())
    obs, rew, done = rng.normal(size=(4, 3)), rng.normal(size=4), np.array([1, 0, 0, 0], bool)
    for x, y in zip(a.step(obs, rew, done)[:2], b.step(obs, rew, done)[:2]):
        assert np.array_equal(x, y)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


def test_check_state_dict_rejects_other_shapes(tmp_path):
    """The host half of load_state_dict / load: keys, shapes (another batch size) and hyper-parameters; and the .npz
    round trip of a state (DeviceNormalizer.read)."""
    from cattleherd.vec_normalize import DeviceNormalizer, check_state_dict
    s = R.VecNormalize(4, (6,)).state_dict()
    mean, var, count, rm, rv, rc, ret = check_state_dict(s, 6, 4)
    assert mean.dtype == np.float64 and count == 1e-4 and rv == 1.0 and ret.shape == (4,)
    with pytest.raises(ValueError, match="another batch size"):
        check_state_dict(s, 6, 5)
    with pytest.raises(ValueError, match="obs_mean"):
        check_state_dict(s, 7, 4)
    with pytest.raises(ValueError, match="lacks"):
        check_state_dict({k: v for k, v in s.items() if k != "ret_var"}, 6, 4)
    with pytest.raises(ValueError, match="clip"):
        check_state_dict(dict(s, clip_obs=-1.0), 6, 4)
    np.savez(tmp_path / "n.npz", **s)
    back = DeviceNormalizer.read(tmp_path / "n.npz")
    assert back.keys() == s.keys() and back["training"] is True and back["gamma"] == 0.99
    assert np.array_equal(back["obs_var"], s["obs_var"])
    check_state_dict(back, 6, 4)


def _norm(_lib, dim=4, n_envs=2, **kw):
    """A ch_norm whose arrays are host memory: good enough for the checks that run before any launch."""
    keep = np.zeros(64, np.float64)
    n = _lib.ChNorm()
    n.dim, n.n_envs, n.training, n.norm_obs, n.norm_reward = dim, n_envs, 1, 1, 1
    n.clip_obs, n.clip_reward, n.epsilon, n.gamma = 10.0, 10.0, 1e-8, 0.99
    for k in ("mean", "var", "count", "ret_stats", "ret", "scratch"):
        setattr(n, k, keep.ctypes.data)
    n.scratch_doubles = 0
    for k, v in kw.items():
        setattr(n, k, v)
    n._keep = keep
    return n


def test_abi_rejections_without_a_device():
    from cattleherd import _lib
    from cattleherd.rollout import _bind
    L = _bind()
    x = np.zeros(8, np.float32)
    u8 = np.zeros(2, np.uint8)
    xp, up = x.ctypes.data, u8.ctypes.data
    assert L.ch_norm_scratch_size(0, 4) == -1 and L.ch_norm_scratch_size(4, 0) == -1
    assert L.ch_norm_scratch_size(1100, 7) == 2 * 18 * 7 + 18 + 1   # 18 chunks of 64 rows
    assert L.ch_norm_scratch_size(4096, 1032) == 2 * 64 * 1032 + 64 + 1
    assert L.ch_norm_scratch_size(16400, 1) == max(2 * 129 + 129 + 1, 3 * 5)   # 128-row chunks past 256 chunks
    err = lambda: L.ch_last_error(None)   # noqa: E731
    assert L.ch_norm_begin(None, None) == _lib.CH_ERR_INVALID and b"NULL normaliser" in err()
    assert L.ch_norm_obs_update(ctypes.byref(_norm(_lib, dim=0)), xp, 2, None) == _lib.CH_ERR_INVALID and b"dim" in err()
    assert L.ch_norm_obs_update(ctypes.byref(_norm(_lib)), xp, 0, None) == _lib.CH_ERR_INVALID and b"rows" in err()
    assert L.ch_norm_obs_update(ctypes.byref(_norm(_lib)), None, 2, None) == _lib.CH_ERR_INVALID and b"NULL matrix" in err()
    assert L.ch_norm_obs_update(ctypes.byref(_norm(_lib, mean=None)), xp, 2, None) == _lib.CH_ERR_INVALID
    assert b"statistic array" in err()
    assert L.ch_norm_obs_update(ctypes.byref(_norm(_lib)), xp, 2, None) == _lib.CH_ERR_INVALID and b"scratch" in err()
    assert L.ch_norm_obs_apply(ctypes.byref(_norm(_lib, clip_obs=-1.0)), xp, 2, None, xp, None) == _lib.CH_ERR_INVALID
    assert b"clip_obs" in err()
    assert L.ch_norm_obs_apply(ctypes.byref(_norm(_lib)), xp, 2, None, None, None) == _lib.CH_ERR_INVALID
    assert b"NULL output" in err()
    n = _norm(_lib, scratch_doubles=64)
    assert L.ch_norm_reward(ctypes.byref(n), None, up, up, 2, xp, None) == _lib.CH_ERR_INVALID and b"NULL array" in err()
    assert L.ch_norm_reward(ctypes.byref(n), xp, up, up, 3, xp + 16, None) == _lib.CH_ERR_INVALID and b"n_envs" in err()
    assert L.ch_norm_reward(ctypes.byref(n), xp, up, up, 2, xp, None) == _lib.CH_ERR_INVALID and b"raw reward" in err()
    assert L.ch_norm_reward(ctypes.byref(_norm(_lib, clip_reward=-0.5, scratch_doubles=64)), xp, up, up, 2, xp + 16,
                            None) == _lib.CH_ERR_INVALID and b"clip_reward" in err()
    assert L.ch_rollout_collect_norm(None, None, None, None, None, None, 0, 0.99, 0.95, 1, None, None, None) == \
        _lib.CH_ERR_INVALID
    assert err().startswith(b"ch_rollout_collect_norm: ")


def test_struct_layout_and_hyper_rejections():
    from cattleherd import _lib
    from cattleherd.vec_normalize import _check_hyper
    assert ctypes.sizeof(_lib.ChNorm) == 4 * 4 + 4 * 8 + 8 + 6 * 8 + 8 + 3 * 8
    assert _lib.ChNorm.clip_obs.offset == 16 and _lib.ChNorm.mean.offset == 56
    for bad in (dict(clip_obs=-1.0), dict(clip_reward=-1.0), dict(epsilon=-1e-8), dict(gamma=1.5)):
        with pytest.raises(ValueError):
            _check_hyper(**dict(dict(clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8), **bad))
