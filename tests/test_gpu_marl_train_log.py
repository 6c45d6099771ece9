"""The device-side RLlib training log of the native MARL PPO path on the GPU: the episode ring's recorder
(ch_marl_ep_ring_*), its wiring into the collection (ch_marl_rollout_collect_log), the learner statistics
(ch_marl_ppo_train_log) and the Python record (train_log.MarlEpisodeRing, MarlPPOUpdate(log_stats=True), rllib_result).

References (tests/marl_train_log_ref.py): MarlRingRef, a host deque plus accumulators in float64 fed one step at a time
-- the ring must equal it exactly; and the float64 torch restatement of the loss with the three log columns, against
which the native columns pass under the project's rule err(native) <= 4 * max(err(torch32), 32 * 2**-24) with torch32
measured in the same test (marl_ppo_ref.accept).  vf_explained_var is compared as it is (it lies between -0.04 and 0.03
in these cases, nowhere near 1).  Each test prints its figures before it asserts.

Measured on an MI355X, err(native) / err(torch32) of vf_loss_unclipped, total_loss, vf_explained_var (the largest over
the case's three steps):
  DRIVER batch 128: 6.3e-09 / 6.3e-09   3.8e-08 / 4.5e-08   2.2e-06 / 5.2e-05
  DRIVER batch 40:  5.5e-08 / 3.2e-08   9.1e-08 / 6.9e-08   2.6e-06 / 1.4e-05
  DRIVER batch 8:   5.1e-08 / 9.1e-08   4.2e-08 / 1.4e-07   3.5e-07 / 3.2e-06
  DRIVER batch 1:   3.3e-08 / 3.3e-08   7.8e-08 / 1.4e-07   NaN natively and in the reference
  SMALL batch 24:   8.8e-08 / 2.3e-08   4.4e-08 / 5.8e-08   6.6e-07 / 1.1e-04
  WIDE batch 24:    1.4e-08 / 1.4e-08   9.0e-08 / 4.3e-08   4.1e-06 / 8.8e-05
  SMALL batch 24, log_std_clip 0.5: 5.9e-08 / 1.2e-07   4.1e-08 / 3.8e-08   1.3e-06 / 7.2e-05
  end to end, the last minibatch: 1.7e-07 / 3.6e-09   7.4e-08 / 7.0e-09   9.5e-08 / 1.9e-07
The collection test's run: 21 episodes over the two collections of 12 steps, 13 of them ending in the second one after
starting in the first (lengths 12 .. 24), the envs 0, 4, 12, 16, 20, 28 ending twice.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N3, M8 = 3, 8
NEW = ("vf_loss_unclipped", "total_loss", "vf_explained_var")


def _dev():
    import torch
    return torch.device("cuda", 0)


# ---- 1. the recorder alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,W", [(1, 4), (63, 4), (65, 100), (1100, 100), (1100, 8)])
def test_recorder_equals_the_reference_after_every_step(E, W):
    """ch_marl_ep_ring_begin / _record on synthetic inputs, N = 3, 30 steps: live with p = 0.7, float32 rewards with NaN
    or 1e30 wherever the agent is not live, reset_happened with p = 0.3.  After every step every ring array, total, the
    accumulators and the counters equal MarlRingRef exactly.  E = 1100 has about 330 endings per step (C > W) and a
    second chunk of 1024 envs; E = 1 has steps that end nothing."""
    import torch
    import marl_train_log_ref as T
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.train_log import MarlEpisodeRing
    live, reward, rh = T.synthetic(E, W)
    b = HerdBatch(E, N3, M8, mode="marl")
    dev = [torch.as_tensor(np.ascontiguousarray(a)).to(b.device) for a in (live, reward, rh)]
    ring = MarlEpisodeRing(b, W).begin()
    ref = T.MarlRingRef(E, N3, W)
    T.assert_ring(ring.arrays(), ref.arrays(), "begin")
    io = _lib.ChStepIO()
    for t in range(len(rh)):
        io.reward, io.reset_happened = dev[1][t].data_ptr(), dev[2][t].data_ptr()
        ring.record(dev[0][t], io)
        ref.step(live[t], reward[t], rh[t])
        T.assert_ring(ring.arrays(), ref.arrays(), f"step {t}")
    T.assert_entries(ring.entries(), ref.entries())
    assert ring.count() == ref.total > 0
    print(f"recorder E={E} W={W}: {ref.total} episodes, most endings in a step {ref.max_ended}, "
          f"steps without one {ref.steps_without_end}")
    if E == 1100:
        assert ref.max_ended > W and any(env >= 1024 for _, env, _, _ in ref.filed)
    if E == 1:
        assert ref.steps_without_end > 0
    for k in ("ep_return", "agent_return", "acc_return"):      # no poisoned value was summed
        assert np.isfinite(ref.arrays()[k]).all() and np.isfinite(ring.arrays()[k]).all()
    # begin again: an open episode counts from zero, the slots stay
    ring.begin()
    ref.begin()
    T.assert_ring(ring.arrays(), ref.arrays(), "second begin")
    b.close()


# ---- 2. the collection ---------------------------------------------------------------------------------------------------
BUFFER = ("obs", "actions", "log_probs", "values", "rewards", "agent_mask", "terminated", "truncated", "advantages",
          "returns", "last_values")


def _collect_twice(E, n, m, T_steps, with_ring):
    """Two collections of T_steps with the graded injection before each, on one ring; returns the buffer tensors after
    each, the final state, and (with a ring) its arrays, entries and the reference fed from the buffers."""
    import torch
    import marl_train_log_ref as T
    from cattleherd.rollout import DeviceMarlRolloutBuffer
    from cattleherd.train_log import MarlEpisodeRing
    b = T.make_graded(E, n, m)
    policy, value = T.bias_policy(T.APPROACH), T.bias_policy([0.25])
    rb = DeviceMarlRolloutBuffer(b, T_steps)
    ring = MarlEpisodeRing(b, 100).begin() if with_ring else None
    ref = T.MarlRingRef(E, n, 100) if with_ring else None
    bufs = []
    for k in range(2):
        if k > 0:
            T.inject_graded(b, n)
        rb.collect(policy, value, seed=1 + k, ring=ring)
        torch.cuda.synchronize()
        bufs.append({name: getattr(rb, name).clone() for name in BUFFER})
        if with_ring:
            T.feed_from_buffer(ref, rb)
    out = dict(bufs=bufs, state=b.get_state())
    if with_ring:
        out.update(arrays=ring.arrays(), entries=ring.entries(), ref=ref, summary=ring.summary())
    b.close()
    return out


def _assert_same_run(a, b):
    import torch
    for x, y in zip(a["bufs"], b["bufs"]):
        for name in BUFFER:
            assert torch.equal(x[name].view(torch.uint8), y[name].view(torch.uint8)), name   # bit for bit
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b["state"][k], equal_nan=True), k


def test_collection_fills_the_ring_and_leaves_the_buffer_alone():
    """E = 32, N = 4, T = 12, the approach-biased policy (log_std -3), two collections on one ring with a re-injection
    between them: the ring equals MarlRingRef fed from the buffer (live = agent_mask[t], reward = rewards[t], an env
    ended at t where every agent live at t has terminated[t]); every buffer tensor and the final state equal a
    ring-less run of the same seeds bit for bit."""
    import marl_train_log_ref as T
    E, n, T_steps = 32, 4, 12
    got = _collect_twice(E, n, 16, T_steps, True)
    ref = got["ref"]
    filed = ref.filed
    print(f"collection: {ref.total} episodes, (step, env, length) {[(s, e, ln) for s, e, ln, _ in filed]}")
    # the run holds what it is meant to test (asserted on the reference)
    assert any(s >= T_steps and ln > s - T_steps + 1 for s, _, ln, _ in filed)      # an episode spans the boundary
    assert any(len(set(al.tolist())) > 1 for _, _, _, al in filed)                   # unequal agent lengths
    envs = [e for _, e, _, _ in filed]
    assert len(set(envs)) < len(envs)                                                # an env ended twice
    T.assert_ring(got["arrays"], ref.arrays(), "collection")
    T.assert_entries(got["entries"], ref.entries())
    assert got["summary"]["num_episodes"] == ref.total
    assert got["summary"]["num_env_steps_sampled"] == 2 * T_steps * E
    _assert_same_run(got, _collect_twice(E, n, 16, T_steps, False))


def test_collection_on_the_not_in_place_path():
    """E = 3, N = 3: an odd number of agent rows, so every step writes the env's own observation buffer and the store
    kernel copies it (the collection's not-in-place path)."""
    import marl_train_log_ref as T
    got = _collect_twice(3, 3, 8, 12, True)
    assert got["ref"].total > 0
    T.assert_ring(got["arrays"], got["ref"].arrays(), "odd rows")
    _assert_same_run(got, _collect_twice(3, 3, 8, 12, False))


# ---- 3. the update's statistics ------------------------------------------------------------------------------------------
_DATA = {}


def _data(shape, clamp):
    import marl_ppo_ref as R
    key = (shape["name"], clamp)
    if key not in _DATA:
        d64 = R.make_data(shape, _dev(), clamp)
        _DATA[key] = (d64, tuple(t.float().contiguous() for t in d64))
    return _DATA[key]


def _native_epoch(model, data32, perm, batch, hp, log):
    import torch
    from cattleherd import marl_ppo
    from cattleherd._lib import check, CH_MARL_PPO_LOG_STATS
    dev = model.device
    lib = marl_ppo._bind()
    net = marl_ppo.marl_ppo_net(model)
    klc = torch.full((1,), hp["kl_coeff"], dtype=torch.float32, device=dev)
    h = marl_ppo.ChMarlPpoHparams(hp["lr"], 0.9, 0.999, hp["eps"], hp["clip_param"], hp["vf_clip_param"],
                                  hp["vf_loss_coeff"], hp["entropy_coeff"], hp["log_std_clip"],
                                  hp["grad_clip"] if hp["grad_clip"] is not None else 0.0, klc.data_ptr())
    d = marl_ppo.ChMarlPpoData(*(t.data_ptr() for t in data32), data32[0].shape[0])
    n = lib.ch_marl_ppo_param_count(ctypes.byref(net))
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    steps = -(-perm.numel() // batch)
    stats = torch.full((steps, CH_MARL_PPO_LOG_STATS if log else 5), float("nan"), device=dev)
    scratch = torch.empty(lib.ch_marl_ppo_scratch_size(ctypes.byref(net), batch), device=dev)
    fn = lib.ch_marl_ppo_train_log if log else lib.ch_marl_ppo_train
    check(fn(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), perm.data_ptr(), perm.numel(), batch, ea.data_ptr(),
             es.data_ptr(), step.data_ptr(), stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(step) == steps
    return stats, ea, es


STAT_CASES = [("DRIVER", 128, False), ("DRIVER", 40, False), ("DRIVER", 8, False), ("DRIVER", 1, False),
              ("SMALL", 24, False), ("WIDE", 24, False), ("SMALL", 24, True)]


@pytest.mark.parametrize("which,batch,clamp", STAT_CASES)
def test_log_columns_match_float64_reference_and_the_update_is_unchanged(which, batch, clamp):
    """ch_marl_ppo_train_log over three minibatches of `batch` rows (the last one partial where the shape allows):
    the three new columns against the float64 reference under the project's rule, torch32 measured here; the one-row
    case gives NaN for vf_explained_var; columns 0-4, the parameters and Adam's moments equal ch_marl_ppo_train's bit
    for bit."""
    import torch
    import marl_ppo_ref as R
    import marl_train_log_ref as T
    shape, dev = getattr(R, which), _dev()
    hp = R.hp_for(clamp, eps=R.TRAIN_EPS)
    data64, data32 = _data(shape, clamp)
    n_idx = min(3 * batch - (batch // 3), shape["rows"])
    perm = torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(R.TRAIN_SEED))[:n_idx].to(dev)
    m0 = R.make_model(shape, dev, clamp=clamp)
    m32 = R.make_model(shape, dev, like=m0, clamp=clamp)
    m64 = R.make_model(shape, dev, torch.float64, like=m0, clamp=clamp)
    s32 = T.ref_epoch_log(m32, R.adam(m32, hp), data32, perm, batch, hp)
    s64 = T.ref_epoch_log(m64, R.adam(m64, hp), data64, perm, batch, hp)
    mn, mp = R.make_model(shape, dev, like=m0, clamp=clamp), R.make_model(shape, dev, like=m0, clamp=clamp)
    sn, ea, es = _native_epoch(mn, data32, perm, batch, hp, True)
    sp, pa, ps = _native_epoch(mp, data32, perm, batch, hp, False)
    assert torch.equal(sn[:, :5], sp) and torch.equal(ea, pa) and torch.equal(es, ps)
    for p, q, p0 in zip(mn.parameters(), mp.parameters(), m0.parameters()):
        assert torch.equal(p, q) and not torch.equal(p, p0)
    ok = True
    for j, name in enumerate(NEW):
        col = 5 + j
        if name == "vf_explained_var" and batch == 1:
            assert torch.isnan(sn[:, col]).all() and torch.isnan(s64[:, col]).all()
            continue
        assert torch.isfinite(sn[:, col]).all()
        for k in range(sn.shape[0]):
            if name == "vf_explained_var" and min(batch, n_idx - k * batch) == 1:
                assert torch.isnan(sn[k, col]) and torch.isnan(s64[k, col])
                continue
            ok &= R.accept(f"log {which} B={batch} clamp={clamp} step {k} {name}", sn[k, col:col + 1],
                           s32[k, col:col + 1], s64[k, col:col + 1])
    print(f"{which} B={batch}: vf_explained_var (float64) {s64[:, 7].tolist()}")
    assert ok


def test_train_log_requires_the_statistics_buffer():
    """ch_marl_ppo_train takes stats = NULL; ch_marl_ppo_train_log does not (CH_ERR_INVALID, nothing launched)."""
    import torch
    import marl_ppo_ref as R
    from cattleherd import _lib as L, marl_ppo
    dev, hp = _dev(), R.hp_for()
    _, data32 = _data(R.SMALL, False)
    m = R.make_model(R.SMALL, dev)
    before = [p.detach().clone() for p in m.parameters()]
    lib = marl_ppo._bind()
    net = marl_ppo.marl_ppo_net(m)
    klc = torch.full((1,), hp["kl_coeff"], dtype=torch.float32, device=dev)
    h = marl_ppo.ChMarlPpoHparams(hp["lr"], 0.9, 0.999, hp["eps"], hp["clip_param"], hp["vf_clip_param"],
                                  hp["vf_loss_coeff"], hp["entropy_coeff"], hp["log_std_clip"], 0.0, klc.data_ptr())
    d = marl_ppo.ChMarlPpoData(*(t.data_ptr() for t in data32), data32[0].shape[0])
    n = lib.ch_marl_ppo_param_count(ctypes.byref(net))
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    perm = torch.arange(24, device=dev)
    scratch = torch.empty(lib.ch_marl_ppo_scratch_size(ctypes.byref(net), 24), device=dev)
    rc = lib.ch_marl_ppo_train_log(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), perm.data_ptr(), 24, 24,
                                   ea.data_ptr(), es.data_ptr(), step.data_ptr(), None, scratch.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == L.CH_ERR_INVALID and b"ch_marl_ppo_train_log" in lib.ch_last_error(None)
    assert int(step) == 0 and all(torch.equal(p, q) for p, q in zip(m.parameters(), before))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
E2E = dict(num_epochs=2, minibatch_size=48, seed=5)


def _iteration(backend, dtype=None, log_stats=True):
    """One collect(ring=) + train at E = 32 from the same start; returns (result, update, ring entries, live rows,
    the buffer).  dtype float64: the reference run over the same collected buffer (torch backend, float64 model)."""
    import torch
    import marl_ppo_ref as R
    import marl_train_log_ref as T
    from cattleherd.marl_ppo import MarlPPOUpdate, RLlibActorCritic
    from cattleherd.rollout import DeviceMarlRolloutBuffer
    from cattleherd.train_log import MarlEpisodeRing, rllib_result
    b = T.make_graded(32, 4, 16)
    model = RLlibActorCritic(device=b.device, seed=0)
    rb = DeviceMarlRolloutBuffer(b, 8)
    ring = MarlEpisodeRing(b).begin()
    rb.collect(*model.device_nets(), seed=1, ring=ring)
    torch.cuda.synchronize()
    live = int((rb.agent_mask != 0).sum())
    if dtype is not None:
        model = R.make_model(dict(obs_dim=86, act_dim=4, hiddens=(256, 256), vf_hiddens=(256, 256)), b.device, dtype,
                             like=model)
        rb = R.fake_buffer(rb, dtype)
    upd = MarlPPOUpdate(model, lr=3e-4, eps=R.TRAIN_EPS, backend=backend, log_stats=log_stats, **E2E)
    steps = upd.train(rb)
    torch.cuda.synchronize()
    out = (rllib_result(ring, upd) if log_stats else None, upd, ring.entries(), live, steps)
    b.close()
    return out


def test_one_iteration_yields_rllib_s_result_on_both_backends():
    import torch
    import marl_ppo_ref as R
    import marl_train_log_ref as T
    res_n, upd_n, ent_n, live, steps = _iteration("native")
    res_t, upd_t, ent_t, live_t, _ = _iteration("torch")
    res_r, upd_r, _, _, _ = _iteration("torch", torch.float64)
    assert list(res_n) == ["env_runners", "learners"] and list(res_n["learners"]) == ["shared_policy"]
    log = res_n["learners"]["shared_policy"]
    assert list(log) == T.LOG_KEYS and tuple(upd_n.stats.shape) == (steps, 8)
    runners = res_n["env_runners"]
    for k in ("episode_return_mean", "episode_return_min", "episode_return_max", "episode_len_mean", "episode_len_min",
              "episode_len_max", "module_episode_returns_mean/shared_policy", "num_episodes", "num_env_steps_sampled"):
        assert k in runners, k
    for i in range(4):
        assert f"agent_episode_returns_mean/agent_{i}" in runners and f"num_agent_steps_sampled/agent_{i}" in runners
    assert runners["num_episodes"] == len(ent_n) > 0 and runners["num_env_steps_sampled"] == 8 * 32
    assert sum(runners[f"num_agent_steps_sampled/agent_{i}"] for i in range(4)) == live
    assert log["curr_kl_coeff"] == float(upd_n.kl_coeff)
    assert log["num_module_steps_trained"] == live * E2E["num_epochs"]
    assert steps == E2E["num_epochs"] * -(-live // E2E["minibatch_size"])
    # the torch backend: the same ring exactly, the same record within the rule
    assert live_t == live
    T.assert_entries(ent_t, ent_n)
    assert res_t["env_runners"] == runners
    ok = True
    for j, name in enumerate(("policy_loss", "vf_loss", "entropy", "kl", "grad_norm") + NEW):
        ok &= R.accept(f"e2e last step {name}", upd_n.stats[-1, j:j + 1], upd_t.stats[-1, j:j + 1],
                       upd_r.stats[-1, j:j + 1])
    assert ok
    assert torch.equal(upd_n.kl_coeff.cpu(), upd_r.kl_coeff.cpu()) and torch.equal(upd_t.kl_coeff.cpu(), upd_r.kl_coeff.cpu())
    # the native update without the log: the same coefficient, statistics, parameters and moments, bit for bit
    _, upd_p, _, _, steps_p = _iteration("native", log_stats=False)
    assert steps_p == steps and tuple(upd_p.stats.shape) == (steps, 5) and upd_p.last_log == {}
    assert torch.equal(upd_p.kl_coeff, upd_n.kl_coeff)
    assert torch.equal(upd_p.stats, upd_n.stats[:, :5])
    assert torch.equal(upd_p.exp_avg, upd_n.exp_avg) and torch.equal(upd_p.exp_avg_sq, upd_n.exp_avg_sq)
    assert all(torch.equal(p, q) for p, q in zip(upd_p.model.parameters(), upd_n.model.parameters()))


# ---- 5. rejections -----------------------------------------------------------------------------------------------------------
def test_rejections():
    import torch
    from cattleherd import _lib as L
    from cattleherd.env import HerdBatch
    from cattleherd.rollout import ChMarlRolloutIO, DeviceMarlRolloutBuffer
    from cattleherd.train_log import MarlEpisodeRing
    import marl_train_log_ref as T
    lib = L.lib()
    b = HerdBatch(4, N3, M8, mode="marl")
    b.reset()
    ring = MarlEpisodeRing(b, 4).begin()
    live = torch.ones((4, N3), dtype=torch.uint8, device=b.device)
    before = ring.arrays()

    def rc_of(fn, *args):
        rc = fn(*args)
        assert rc != L.CH_OK and lib.ch_last_error(args[0])
        return rc
    # a CTDE handle
    c = HerdBatch(4, N3, M8, mode="ctde")
    assert rc_of(lib.ch_marl_ep_ring_begin, c.handle, ctypes.byref(ring._ring), None) == L.CH_ERR_UNSUPPORTED
    assert rc_of(lib.ch_marl_ep_ring_record, c.handle, ctypes.byref(ring._ring), live.data_ptr(), c._io_ref,
                 None) == L.CH_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        MarlEpisodeRing(c)
    c.close()
    # a missing reward / reset_happened
    for missing in ("reward", "reset_happened"):
        io = L.ChStepIO()
        io.reward, io.reset_happened = b.reward.data_ptr(), b.reset_happened.data_ptr()
        setattr(io, missing, None)
        assert rc_of(lib.ch_marl_ep_ring_record, b.handle, ctypes.byref(ring._ring), live.data_ptr(),
                     ctypes.byref(io), None) == L.CH_ERR_INVALID
    assert rc_of(lib.ch_marl_ep_ring_record, b.handle, ctypes.byref(ring._ring), None, b._io_ref, None) == L.CH_ERR_INVALID
    # W < 1
    bad = L.ChMarlEpRing.from_buffer_copy(ring._ring)
    bad.window = 0
    assert rc_of(lib.ch_marl_ep_ring_begin, b.handle, ctypes.byref(bad), None) == L.CH_ERR_INVALID
    with pytest.raises(ValueError):
        MarlEpisodeRing(b, 0)
    # a ring given to the collection without reset_happened in the step io
    rb = DeviceMarlRolloutBuffer(b, 2)
    policy, value = T.bias_policy(T.APPROACH), T.bias_policy([0.0])
    for net in (policy, value):
        net._ensure_packed()
    sio = L.ChStepIO.from_buffer_copy(b._io)
    sio.reset_happened = None
    io = ChMarlRolloutIO()
    io.step = ctypes.pointer(sio)
    io.policy_out, io.value_out, io.env_actions = rb.policy_out.data_ptr(), rb.value_out.data_ptr(), rb.env_actions.data_ptr()
    args = (b.handle, ctypes.byref(rb._rb), ctypes.byref(io), ctypes.byref(policy._net), ctypes.byref(value._net), 1,
            0.99, 1.0)
    assert rc_of(lib.ch_marl_rollout_collect_log, *args, ctypes.byref(ring._ring), None) == L.CH_ERR_INVALID
    b.sync()
    T.assert_ring(ring.arrays(), before, "a rejected call changes nothing")
    b.close()
