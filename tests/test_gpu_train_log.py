"""GPU tests of the device-side SB3 training log (cattleherd/train_log.py; ch_ep_ring_*, ch_rollout_collect_log,
ch_ppo_train_log, ch_explained_variance) against tests/train_log_ref.py.

The episode ring is integer bookkeeping and float64 values copied from the step's own outputs: every comparison with
SB3's deque is exact (returns as bit patterns).  ch_ppo_train_log's first four columns, the weights and Adam's state
are bit-equal to ch_ppo_train; clip_fraction is the float64 reference's count / B exactly (the data keeps every ratio
1e-3 away from a clip edge); approx_kl is held by ppo_native_ref.accept -- err(native) <= 4 max(err(torch32),
32 * 2**-24) against the float64 reference -- and the explained variance by 4 n 2^-53 (1 + |1 - ref|), the worst-case
bound of its four n-term float64 sums."""
import ctypes

import numpy as np
import pytest

import train_log_ref as T

pytestmark = pytest.mark.gpu

BUFS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


# ---- 1. the recorder alone, on synthetic flags ------------------------------------------------------------------
@pytest.mark.parametrize("E,W", [(1100, 8), (1100, 100), (64, 8)])
def test_recorder_equals_the_deque_after_every_step(E, W):
    """Steps that end C = 0, 1, 3, W, W + 5, 0, 2 envs; the W + 5 are consecutive envs straddling index 1024 (the
    chunk boundary of the one-workgroup kernel; E = 1100 is no multiple of 64), the others spread over the batch."""
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.train_log import EpisodeRing
    rng = np.random.default_rng(10 * E + W)
    b = HerdBatch(E, 2, 8, mode="ctde")
    ring = EpisodeRing(b, W).begin()
    ref = T.DequeRef(W)
    assert ring.entries() == [] and ring.summary() == {}
    io = _lib.ChStepIO()
    for C in (0, 1, 3, W, W + 5, 0, 2):
        rh = np.zeros(E, np.uint8)
        if C == W + 5 and E > 1024:
            lo = 1024 - C // 2
            rh[lo:lo + C] = 1
            assert rh[:1024].any() and rh[1024:].any()
        else:
            rh[rng.choice(E, C, replace=False)] = 1
        stats = np.stack([rng.normal(0.0, 100.0, E), rng.integers(1, 1203, E).astype(np.float64)], -1)
        d_rh, d_st = torch.as_tensor(rh).to(b.device), torch.as_tensor(stats).to(b.device)
        io.reset_happened, io.episode_stats = d_rh.data_ptr(), d_st.data_ptr()
        ring.record(io)
        ref.step(rh, stats)
        assert ring.count() == ref.total
        assert T.same_entries(ring.entries(), ref.entries()), C
    assert ref.total == 2 * W + 11 and len(ref.entries()) == min(W, ref.total)
    want = {"rollout/ep_rew_mean": float(np.mean([round(float(r), 6) for r, _, _ in ref.entries()])),
            "rollout/ep_len_mean": float(np.mean([n for _, n, _ in ref.entries()]))}
    assert ring.summary() == want
    ring.begin()
    assert ring.count() == 0 and ring.entries() == []
    b.close()


def test_ring_rejections_on_a_device():
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.train_log import EpisodeRing
    L = _lib.lib()
    b = HerdBatch(8, 2, 8, mode="ctde")
    ring = EpisodeRing(b, 4).begin()
    for field in ("reset_happened", "episode_stats"):
        sio = _lib.ChStepIO()
        ctypes.memmove(ctypes.byref(sio), ctypes.byref(b._io), ctypes.sizeof(sio))
        setattr(sio, field, None)
        with pytest.raises(_lib.ChError, match=field) as ei:
            ring.record(sio)
        assert ei.value.code == _lib.CH_ERR_INVALID
    m = HerdBatch(8, 2, 8, mode="marl")
    with pytest.raises(ValueError):
        EpisodeRing(m, 4)
    assert L.ch_ep_ring_begin(m.handle, ctypes.byref(ring._ring), m._stream()) == _lib.CH_ERR_UNSUPPORTED
    assert L.ch_ep_ring_record(m.handle, ctypes.byref(ring._ring), m._io_ref, m._stream()) == _lib.CH_ERR_UNSUPPORTED
    assert b"CTDE" in L.ch_last_error(m.handle)
    m.close()
    b.torch.cuda.synchronize()
    assert ring.count() == 0
    b.close()


# ---- 2. inside the collection -----------------------------------------------------------------------------------
W_COLLECT, T_COLLECT = 8, 10
# step counters (level 7: the 80 s limit is 4800) per env modulo 8: three groups that reach the limit at different
# steps of the rollout, and three that stay far from it
COUNTER_OFFSETS = np.array([0, 0, 2, 2, 5, 1000, 1000, 1000])


def _collect_batch(E):
    from cattleherd.env import HerdBatch
    b = HerdBatch(E, 4, 16, mode="ctde", curriculum_level=7)
    b.reset()
    b.set_state({"step_counter": 4800 - 4 * COUNTER_OFFSETS[np.arange(E) % 8]})
    return b


def _nets(fused=False):
    from cattleherd.policy import DevicePolicy
    actor = DevicePolicy(DevicePolicy.random_layers([12 * 86, 128, 128, 16], seed=1), "tanh", None)
    critic = DevicePolicy(DevicePolicy.random_layers([12 * 86, 128, 128, 1], seed=2), "tanh", None)
    return (DevicePolicy.fuse(actor, critic), None) if fused else (actor, critic)


def _reference(E):
    """collect_steps (the Python loop) with a host deque that reads reset_happened and episode_stats after every
    step; the conditions the test rests on are asserted on it alone."""
    import torch
    from cattleherd.rollout import DeviceRolloutBuffer
    b = _collect_batch(E)
    actor, critic = _nets()
    ref = T.HostDeque(b, W_COLLECT)
    rb = DeviceRolloutBuffer(b, T_COLLECT)
    rb.collect_steps(actor, critic, torch.full((16,), -1.0, device=b.device), seed=9, ring=ref)
    torch.cuda.synchronize()
    b.close()
    assert len(ref.per_step) == T_COLLECT
    assert ref.total > W_COLLECT, ref.per_step              # more episodes than the window holds
    assert max(ref.per_step) >= 2 and min(ref.per_step) == 0, ref.per_step
    return ref


_REFS = {}


def _ref_for(E):
    if E not in _REFS:
        _REFS[E] = _reference(E)
    return _REFS[E]


@pytest.mark.parametrize("E,path,fused", [(256, 0, False), (256, 2, False), (256, 1, False), (256, 8, False),
                                          (256, 0, True), (256, 2, True), (4096, 4, False)],
                         ids=["epilogues", "store_kernel", "copy_each", "never_fused", "fused_net", "fused_net_store_kernel",
                              "fused_step_actor"])
def test_collection_fills_the_ring_like_the_host_deque(E, path, fused):
    """collect(ring=...) on each path of the collection (ch__set_rollout_path; the fused step + actor kernel needs the
    4096-env geometry) and with a fused actor-critic: the ring's entries equal the host deque's exactly, and every
    rollout-buffer tensor is bit-equal to collect() without a ring."""
    import torch
    from cattleherd import _lib
    from cattleherd.rollout import DeviceRolloutBuffer
    from cattleherd.train_log import EpisodeRing
    L = _lib.lib()
    L.ch__rollout_fused_steps.restype = ctypes.c_int64
    ref = _ref_for(E)
    bufs = []
    for with_ring in (True, False):
        b = _collect_batch(E)
        assert L.ch__set_rollout_path(b.handle, ctypes.c_int32(path)) == 0
        actor, critic = _nets(fused)
        rb = DeviceRolloutBuffer(b, T_COLLECT)
        ring = EpisodeRing(b, W_COLLECT).begin() if with_ring else None
        rb.collect(actor, critic, torch.full((16,), -1.0, device=b.device), seed=9, ring=ring)
        torch.cuda.synchronize()
        if path == 4:
            assert L.ch__rollout_fused_steps(b.handle) == T_COLLECT - 1     # the fused kernel is the one that ran
        if with_ring:
            assert ring.count() == ref.total
            assert T.same_entries(ring.entries(), ref.entries())
        bufs.append({k: getattr(rb, k).cpu() for k in BUFS})
        b.close()
    for k in BUFS:
        assert torch.equal(bufs[0][k], bufs[1][k]), k


def test_python_loop_fills_the_ring_too_and_a_ring_needs_episode_stats():
    import torch
    from cattleherd import _lib
    from cattleherd.rollout import ChRolloutIO, DeviceRolloutBuffer
    from cattleherd.train_log import EpisodeRing
    E = 256
    ref = _ref_for(E)
    b = _collect_batch(E)
    actor, critic = _nets()
    rb = DeviceRolloutBuffer(b, T_COLLECT)
    ring = EpisodeRing(b, W_COLLECT).begin()
    log_std = torch.full((16,), -1.0, device=b.device)
    rb.collect_steps(actor, critic, log_std, seed=9, ring=ring)
    assert T.same_entries(ring.entries(), ref.entries())
    # a ring and a step io without episode_stats: rejected on entry, nothing runs
    sio = _lib.ChStepIO()
    ctypes.memmove(ctypes.byref(sio), ctypes.byref(b._io), ctypes.sizeof(sio))
    sio.terminal_obs, sio.episode_stats = b.terminal_obs.data_ptr(), None
    io = ChRolloutIO()
    io.step = ctypes.pointer(sio)
    io.mean, io.value, io.terminal_value = rb.mean.data_ptr(), rb.value.data_ptr(), rb.terminal_value.data_ptr()
    io.env_actions = rb.env_actions.data_ptr()
    for net in (actor, critic):
        net._ensure_packed()
    args = (b.handle, ctypes.byref(rb._rb), ctypes.byref(io), ctypes.byref(actor._net), ctypes.byref(critic._net),
            log_std.data_ptr(), 9, 0.99, 0.95, 1)
    before = ring.count()
    assert rb._lib.ch_rollout_collect_log(*args, ctypes.byref(ring._ring), b._stream()) == _lib.CH_ERR_INVALID
    assert b"episode_stats" in rb._lib.ch_last_error(b.handle)
    assert ring.count() == before
    b.close()


# ---- 3. the update's statistics ---------------------------------------------------------------------------------
def _native_train(fn, mn, data32, idx, batch_size, ncol):
    import torch
    from cattleherd import ppo
    from cattleherd._lib import check
    from ppo_native_ref import HP
    lib = ppo._bind()
    dev = mn.device
    net = ppo.ppo_net(mn)
    h = ppo.ChPpoHparams(HP["learning_rate"], 0.9, 0.999, 1e-5, HP["clip_range"], HP["ent_coef"], HP["vf_coef"],
                         HP["max_grad_norm"], 1, 0)
    d = ppo.ChPpoData(*(t.data_ptr() for t in data32), data32[0].shape[0])
    n = lib.ch_ppo_param_count(ctypes.byref(net))
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    steps = -(-idx.numel() // batch_size)
    stats = torch.full((steps, ncol), float("nan"), device=dev)
    scratch = torch.empty(lib.ch_ppo_scratch_size(ctypes.byref(net), min(batch_size, idx.numel())), device=dev)
    check(getattr(lib, fn)(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), idx.data_ptr(), idx.numel(), batch_size,
                           ea.data_ptr(), es.data_ptr(), step.data_ptr(), stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    return stats, ea, es, int(step), [p.detach().clone() for p in mn.parameters()]


@pytest.mark.parametrize("name,batch", T.UPDATE_CASES, ids=[c[0] for c in T.UPDATE_CASES])
def test_update_statistics(name, batch):
    """ch_ppo_train_log against ch_ppo_train (bit-equal), the float64 count (clip_fraction, exact) and the float64
    approx_kl under ppo_native_ref.accept.

    Measured on an MI355X, approx_kl err(native) / err(torch32) / bound: B = 64: 1.544e-7 / 5.871e-8 / 7.629e-6;
    96 rows in minibatches of 64: 3.462e-7 / 1.547e-6 / 7.629e-6, then (32 rows) 8.673e-7 / 2.090e-6 / 8.361e-6;
    B = 8: 1.164e-6 / 5.733e-6 / 2.293e-5; B = 1: 4.139e-6 / 1.418e-6 / 7.629e-6.

    (ratio - 1) - log_ratio cancels: at the one-row case log_ratio = 0.18292 and approx_kl = 0.017799, so the bound is
    1.36e-7 absolute, while half an ulp of the row's log-probability (-13.05) times (ratio - 1) is 0.96e-7 and half
    an ulp of the ratio 0.60e-7.  The kernel sums the row's log-probability a second time in float64, from the same
    float32 mean, and evaluates expm1(log_ratio) - log_ratio in float64 for this column alone; what is left is the
    float32 forward's error in the mean."""
    import torch
    import ppo_native_ref as R
    shape = R.DRIVER
    dev = torch.device("cuda", 0)
    data64 = R.make_data(shape, dev)
    data32 = tuple(t.float().contiguous() for t in data64)
    idx = T.update_case_idx(name, batch).to(dev)
    m0 = R.make_model(shape, dev)
    ref64 = T.update_reference(R.make_model(shape, dev, torch.float64, like=m0), data64, idx, batch, R.HP)
    ref32 = T.update_reference(R.make_model(shape, dev, like=m0), data32, idx, batch, R.HP)
    for st, akl, count, ratio, clipped in ref64:
        R.check_clip_conditions(ratio, clipped)
    plain = _native_train("ch_ppo_train", R.make_model(shape, dev, like=m0), data32, idx, batch, 4)
    log = _native_train("ch_ppo_train_log", R.make_model(shape, dev, like=m0), data32, idx, batch, 6)
    again = _native_train("ch_ppo_train_log", R.make_model(shape, dev, like=m0), data32, idx, batch, 6)
    # columns 0-3, Adam's state, the step count and the weights: ch_ppo_train's, bit for bit
    assert torch.equal(log[0][:, :4], plain[0]) and torch.isfinite(log[0]).all()
    assert torch.equal(log[1], plain[1]) and torch.equal(log[2], plain[2]) and log[3] == plain[3] == len(ref64)
    for p, q, p0 in zip(log[4], plain[4], m0.parameters()):
        assert torch.equal(p, q) and not torch.equal(p, p0)
    # two runs from the same state: the same bits
    assert torch.equal(again[0], log[0]) and all(torch.equal(p, q) for p, q in zip(again[4], log[4]))
    ok = True
    for k, ((_, akl64, count64, ratio, _), (_, akl32, _, _, _)) in enumerate(zip(ref64, ref32)):
        B = ratio.numel()
        assert float(log[0][k, 5]) == float(np.float32(count64 / B)), (k, float(log[0][k, 5]), count64, B)
        ok &= R.accept(f"approx_kl {name} step {k} B={B}", log[0][k, 4:5], akl32, akl64)
    assert ok


# ---- 4. explained variance --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_explained_variance_matches_float64_numpy(n):
    import torch
    from cattleherd.train_log import explained_variance
    rng = np.random.default_rng(n)
    ret = (rng.normal(0.0, 3.0, n) + 0.5).astype(np.float32)
    val = (0.7 * ret + rng.normal(0.0, 1.0, n)).astype(np.float32)
    if n > 1:
        assert (ret > 0).any() and (ret < 0).any() and (val > 0).any() and (val < 0).any()
    dev = torch.device("cuda", 0)
    d_val, d_ret = torch.as_tensor(val).to(dev), torch.as_tensor(ret).to(dev)
    got = explained_variance(d_val, d_ret).cpu().numpy()
    twice = explained_variance(d_val, d_ret).cpu().numpy()
    assert got.tobytes() == twice.tobytes()
    ref, var_y = T.explained_variance64(val, ret)
    print(f"n={n}: ev {got[0]!r} ref {ref!r} var(returns) {got[1]!r} ref {var_y!r}")
    if n == 1:
        assert np.isnan(ref) and np.isnan(got[0]) and got[1] == 0.0      # one element: var(returns) = 0
        return
    assert abs(got[0] - ref) <= T.ev_tolerance(n, ref)
    assert abs(got[1] - var_y) <= 4.0 * n * 2.0 ** -53 * var_y
    # constant returns: NaN, as SB3 returns it
    const = torch.full((n,), 2.5, device=dev)
    out = explained_variance(d_val, const).cpu().numpy()
    assert np.isnan(out[0]) and out[1] == 0.0


# ---- 5. PPOUpdate(log_stats=True) -------------------------------------------------------------------------------
def test_ppo_update_logs_sb3_s_train_keys():
    import torch
    import ppo_native_ref as R
    from cattleherd.env import HerdBatch
    from cattleherd.ppo import PPOUpdate, SB3ActorCritic
    from cattleherd.rollout import DeviceRolloutBuffer
    b = HerdBatch(64, 2, 8, mode="ctde", compat=False)
    b.reset()
    model = SB3ActorCritic(obs_dim=b.obs_rows * 86, act_dim=48, device=b.device, seed=0)
    actor, critic, log_std = model.device_nets()
    rb = DeviceRolloutBuffer(b, 8, act_dim=48)
    rb.collect(actor, critic, log_std, seed=1)
    shape = dict(obs_dim=b.obs_rows * 86, act_dim=48, pi=(128, 128), vf=(128, 128))
    kw = dict(batch_size=48, n_epochs=2, seed=5, backend="native")     # 512 rows: 2 x (10 of 48 + a partial 32)
    with pytest.raises(ValueError, match="log_stats"):
        PPOUpdate(model, backend="torch", graph=False, log_stats=True)
    m_log, m_plain = R.make_model(shape, b.device, like=model), R.make_model(shape, b.device, like=model)
    upd = PPOUpdate(m_log, log_stats=True, **kw)
    plain = PPOUpdate(m_plain, **kw)
    assert upd.train(rb) == plain.train(rb) == 22
    torch.cuda.synchronize()
    assert plain.last_log == {} and plain.last_stats is None
    for p, q, p0 in zip(m_log.parameters(), m_plain.parameters(), model.parameters()):
        assert torch.equal(p, q) and not torch.equal(p, p0)       # log_stats changes nothing of the update
    log, st = upd.last_log, upd.last_stats
    assert tuple(log) == PPOUpdate.LOG_KEYS and len(log) == 10
    assert st.shape == (22, 6) and st.dtype == np.float32 and np.isfinite(st).all()
    s64 = st.astype(np.float64)
    assert log["train/entropy_loss"] == float(np.mean(-s64[:, 2]))
    assert log["train/policy_gradient_loss"] == float(np.mean(s64[:, 0]))
    assert log["train/value_loss"] == float(np.mean(s64[:, 1]))
    assert log["train/approx_kl"] == float(np.mean(s64[:, 4])) and log["train/approx_kl"] > 0
    assert log["train/clip_fraction"] == float(np.mean(s64[:, 5])) and 0 <= log["train/clip_fraction"] <= 1
    assert log["train/loss"] == float(s64[-1, 0] + 0.1 * -s64[-1, 2] + 0.7 * s64[-1, 1])
    n = rb.values.numel()
    ref, _ = T.explained_variance64(rb.values.cpu().numpy().ravel(), rb.returns.cpu().numpy().ravel())
    assert abs(log["train/explained_variance"] - ref) <= T.ev_tolerance(n, ref)
    assert log["train/std"] == float(torch.exp(m_log.log_std.data).mean())
    assert log["train/n_updates"] == 2 and log["train/clip_range"] == 0.1
    upd.train(rb)
    assert upd.last_log["train/n_updates"] == 4 and upd.last_stats.shape == (22, 6)
    b.close()
