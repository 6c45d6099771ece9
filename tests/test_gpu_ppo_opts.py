"""GPU tests of the native PPO update's options (ch_ppo_train_opt; PPOUpdate(target_kl=, clip_range_vf=, callable
learning_rate / clip_range)) against the torch backend: float64 the reference, float32 the yardstick, held by
ppo_native_ref.accept (err(native) <= 4 max(err(torch32), 32 * 2**-24)) wherever values are compared, and bit for bit
wherever the issue is what was -- or was not -- written.

Shapes: 64 envs x (2, 8) x 8 steps = 512 rows on the driver's net 1032-128-128-48 for the loops; ppo_native_ref's
synthetic DRIVER / SMALL data for single gradients.  The collected buffer's old_log_prob is the model's own, so its
approx_kl is not separable: the gate tests add +-0.6 to the old_log_prob of the rows of the minibatch that is to trip
(ppo_opts_ref.spike_log_probs), and assert on the float64 reference alone that this separates it.  The value-clip
gradient of one minibatch is read without updating by one ch_ppo_train_opt step with learning_rate = 0, from the
gradient region at the end of the scratch (include/cattleherd.h).

Measured on an MI355X (each test prints its figures before it asserts), the largest err(native) / err(torch32) of a
group: gated run, parameters 1.4e-6 / 7.7e-7, m 2.4e-6 / 3.2e-6, v 1.9e-6 / 2.1e-6, the tripping row's statistics
1.8e-6 / 3.3e-7 (policy loss) against bounds of 7.6e-6 and more; value-clip loop of 16 steps, parameters 4.2e-6 / 5.5e-6,
m 7.2e-6 / 7.9e-6, v 4.1e-6 / 4.0e-6; value-clip gradients and statistics of one minibatch below 2e-6; the tripping
row's gradient norm (against the torch gradients of that minibatch at the stopped parameters) 1.6e-6 / 2.6e-6."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, EPOCHS, SEED = 512, 3, 5
SHAPE = dict(obs_dim=1032, act_dim=48, pi=(128, 128), vf=(128, 128))


@pytest.fixture(scope="module")
def collected():
    import torch
    from cattleherd.env import HerdBatch
    from cattleherd.ppo import SB3ActorCritic
    from cattleherd.rollout import DeviceRolloutBuffer
    b = HerdBatch(64, 2, 8, mode="ctde", compat=False)
    b.reset()
    model = SB3ActorCritic(obs_dim=b.obs_rows * 86, act_dim=48, device=b.device, seed=0)
    actor, critic, log_std = model.device_nets()
    rb = DeviceRolloutBuffer(b, 8, act_dim=48)
    rb.collect(actor, critic, log_std, seed=1)
    torch.cuda.synchronize()
    yield b, model, rb
    b.close()


def _buffers(collected, s=None, batch=64, sigma=None, vseed=17):
    """Float32 and float64 copies of the collected buffer holding the same values; `s`: the step whose minibatch gets
    the log-prob spikes; sigma: old values = the model's own + N(0, sigma^2) (seeded)."""
    import torch
    import ppo_opts_ref as P
    b, model, rb = collected
    b32 = P.fake_buffer(rb, torch.float32)
    if s is not None:
        perms = P.perms_of(SEED, N, EPOCHS, b.device)
        nb = N // batch
        P.spike_log_probs(b32.log_probs, perms[s // nb][(s % nb) * batch:(s % nb + 1) * batch])
    if sigma is not None:
        with torch.no_grad():
            v, _, _ = model.evaluate_actions(rb.obs.view(N, -1), rb.actions.view(N, -1))
        g = torch.Generator().manual_seed(vseed)
        b32.values = (v.view_as(rb.values) + sigma * torch.randn(rb.values.shape, generator=g).to(b.device)).contiguous()
    return b32, P.fake_buffer(b32, torch.float64)


def _run(collected, buf, backend, dtype=None, batch=64, n_epochs=EPOCHS, **kw):
    import torch
    import ppo_native_ref as R
    from cattleherd.ppo import PPOUpdate
    b, model, _ = collected
    m = R.make_model(SHAPE, b.device, dtype or torch.float32, like=model)
    upd = PPOUpdate(m, batch_size=batch, n_epochs=n_epochs, seed=SEED, graph=False, backend=backend, **kw)
    upd.train(buf)
    torch.cuda.synchronize()
    return m, upd


def _adam_state(m, upd):
    import torch
    if upd.backend == "native":
        return upd.exp_avg, upd.exp_avg_sq
    return (torch.cat([upd.opt.state[p]["exp_avg"].flatten() for p in m.parameters()]),
            torch.cat([upd.opt.state[p]["exp_avg_sq"].flatten() for p in m.parameters()]))


def _c_train(model, buf, chunks, batch, fn="ch_ppo_train_opt", opts=None, state=None, lr=3e-4, poison=0):
    """Direct calls: one per chunk of row indices.  Returns (stats [steps + poison, ncol], m, v, step, rc list)."""
    import torch
    from cattleherd import _lib, ppo
    lib = ppo._bind()
    dev = model.device
    data = (buf.obs.view(N, -1), buf.actions.view(N, -1), buf.log_probs.view(N), buf.advantages.view(N), buf.returns.view(N))
    net = ppo.ppo_net(model)
    h = ppo.ChPpoHparams(lr, 0.9, 0.999, 1e-5, 0.1, 0.1, 0.7, 0.5, 1, 0)
    d = ppo.ChPpoData(*(t.data_ptr() for t in data), N)
    n = lib.ch_ppo_param_count(ctypes.byref(net))
    if state is None:
        state = (torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    ea, es, step = state
    ncol = 7 if fn == "ch_ppo_train_opt" else 6
    steps = sum(-(-len(c) // batch) for c in chunks)
    stats = torch.full((steps + poison, ncol), 12345.0, device=dev)
    scratch = torch.empty(lib.ch_ppo_scratch_size(ctypes.byref(net), batch), device=dev)
    k, rcs = 0, []
    for c in chunks:
        args = [ctypes.byref(net), ctypes.byref(h), ctypes.byref(d)]
        if fn == "ch_ppo_train_opt":
            args.append(None if opts is None else ctypes.byref(opts))
        rcs.append(getattr(lib, fn)(*args, c.data_ptr(), len(c), batch, ea.data_ptr(), es.data_ptr(), step.data_ptr(),
                                    stats[k].data_ptr(), scratch.data_ptr(), None))
        k += -(-len(c) // batch)
    torch.cuda.synchronize()
    return stats, ea, es, int(step), rcs, scratch


def _grad_norm(m, upd, buf, idx):
    """The unclipped gradient norm of the minibatch `idx` at `m`'s present parameters, through the updater's own loss."""
    import torch
    data = upd._flat(buf) + ((buf.values.view(N),) if upd.clip_range_vf is not None else ())
    for p in m.parameters():
        p.grad = None
    upd._loss(*(t.index_select(0, idx) for t in data)).backward()
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in m.parameters()])).detach().view(1)


def _params(m):
    return [p.detach().clone() for p in m.parameters()]


# ---- 1. options off ---------------------------------------------------------------------------------------------------
def test_options_off_is_ch_ppo_train_log_bit_for_bit(collected):
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    from cattleherd import _lib
    b, model, rb = collected
    perms = P.perms_of(SEED, N, 2, b.device)          # 2 x (10 minibatches of 48 + a partial one of 32)
    ma, mb = R.make_model(SHAPE, b.device, like=model), R.make_model(SHAPE, b.device, like=model)
    log = _c_train(ma, rb, perms, 48, fn="ch_ppo_train_log")
    opt = _c_train(mb, rb, perms, 48, opts=_lib.ChPpoOpts(0.0, 0.0, None, None))
    assert log[4] == opt[4] == [0, 0] and log[3] == opt[3] == 22
    assert torch.equal(opt[0][:, :6], log[0]) and torch.isfinite(log[0]).all()
    assert torch.equal(opt[0][:, 6], torch.ones(22, device=b.device))
    assert torch.equal(opt[1], log[1]) and torch.equal(opt[2], log[2])
    for p, q, p0 in zip(ma.parameters(), mb.parameters(), model.parameters()):
        assert torch.equal(p, q) and not torch.equal(p, p0)


# ---- 2. / 6. the gate, alone and with the value clip --------------------------------------------------------------------
S = 11     # epoch 2 (steps 8..15), its fourth minibatch


@pytest.mark.parametrize("sigma", [None, 0.25], ids=["gate", "gate_and_value_clip"])
def test_gate_stops_all_three_at_the_same_minibatch(collected, sigma):
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    from cattleherd import _lib
    from cattleherd.train_log import sb3_train_record
    b, model, rb = collected
    b32, b64 = _buffers(collected, s=S, sigma=sigma)
    kw = {} if sigma is None else {"clip_range_vf": sigma}
    _, free = _run(collected, b64, "torch", torch.float64, target_kl=1e9, **kw)       # ref64, the gate never trips
    kls = free.last_stats[:, 4]
    assert free.last_stats.shape == (24, 7) and (free.last_stats[:, 6] == 1).all()
    T = float(kls[S]) / 1.2
    print(f"ref64 approx_kl: max before {kls[:S].max():.5f}, at s {kls[S]:.5f}, T {T:.5f}")
    assert kls[:S].max() < 0.9 * T and kls[S] > 1.1 * T                               # on ref64 alone
    kw["target_kl"] = T / 1.5
    mn, un = _run(collected, b32, "native", log_stats=True, **kw)
    mt, ut = _run(collected, b32, "torch", **kw)
    mr, ur = _run(collected, b64, "torch", torch.float64, **kw)
    want = [1] * S + [0] + [-1] * (23 - S)
    for u in (un, ut, ur):
        assert list(u.last_stats[:, 6]) == want and u.stopped_early and u.steps_applied == S and u.n_updates == 2
    assert int(un.step_count) == S
    st = un.last_stats
    assert st.shape == (24, 7) and np.isnan(st[S + 1:, :6]).all() and np.isfinite(st[:S + 1, :6]).all()
    ok = True
    an, at, ar = _adam_state(mn, un), _adam_state(mt, ut), _adam_state(mr, ur)
    for name, pn, pt, pr in zip(R.param_names(mn), mn.parameters(), mt.parameters(), mr.parameters()):
        ok &= R.accept(f"gate param {name}", pn.detach(), pt.detach(), pr.detach())
    for i, name in enumerate(("m", "v")):
        ok &= R.accept(f"gate {name}", an[i], at[i], ar[i])
    for col, name in ((0, "policy_loss"), (1, "value_loss"), (2, "entropy"), (4, "approx_kl")):
        f = lambda u: torch.tensor([u.last_stats[S, col]], dtype=torch.float64)
        ok &= R.accept(f"gate row s {name}", f(un), f(ut), f(ur))
    # clip_fraction is a count / 64: after s - 1 updates a row may sit at a clip edge, where float32 and float64 differ
    assert abs(float(st[S, 5]) - ur.last_stats[S, 5]) <= 1 / 64 and st[S, 5] > 0.9     # (the 64 spiked rows are clipped)
    assert ok
    # the tripping and the skipped steps wrote nothing: a run handed only the first s minibatches, bit for bit
    perms = P.perms_of(SEED, N, 2, b.device)
    # ... except the statistics row: its gradient norm is that of the tripping minibatch at the parameters the run
    # stopped with, which the two torch runs hold too (SB3 never forms this gradient: their tables have NaN there)
    idx_s = perms[1][(S - 8) * 64:(S - 7) * 64]
    assert R.accept("gate row s grad_norm", torch.as_tensor(st[S, 3:4]).double(), _grad_norm(mt, ut, b32, idx_s).cpu(),
                    _grad_norm(mr, ur, b64, idx_s).cpu())
    mc = R.make_model(SHAPE, b.device, like=model)
    o = _lib.ChPpoOpts(0.0, sigma or 0.0, b32.values.data_ptr() if sigma else None, None)
    cut = _c_train(mc, b32, [perms[0], perms[1][:(S - 8) * 64].contiguous()], 64, opts=o)
    assert cut[3] == S and torch.equal(cut[1], an[0]) and torch.equal(cut[2], an[1])
    assert all(torch.equal(p, q) for p, q in zip(mc.parameters(), mn.parameters()))
    assert torch.equal(cut[0][:, :6].cpu(), torch.as_tensor(st[:S, :6]))
    # the record
    ev, std = un.last_log["train/explained_variance"], un.last_log["train/std"]
    rec, epochs = sb3_train_record(st, 8, 0.1, 0.7, 0.1, ev, std, learning_rate=3e-4, clip_range_vf=sigma)
    assert un.last_log == rec and epochs == 2 and rec["train/n_updates"] == 2
    assert ("train/clip_range_vf" in rec) == (sigma is not None) and rec["train/learning_rate"] == 3e-4
    assert rec["train/loss"] == float(st[S, 0].astype(np.float64) + 0.1 * -st[S, 2].astype(np.float64)
                                      + 0.7 * st[S, 1].astype(np.float64))


# ---- 3. armed, never trips / 7. bit reproducibility ---------------------------------------------------------------------
def test_armed_gate_that_never_trips_changes_nothing_and_runs_are_reproducible(collected):
    import torch
    b32, _ = _buffers(collected, s=S, sigma=0.25)
    mp, up = _run(collected, b32, "native", n_epochs=2)
    ma, ua = _run(collected, b32, "native", n_epochs=2, target_kl=1e6)
    assert not ua.stopped_early and ua.steps_applied == up.steps_applied == 16 and ua.n_updates == 2
    assert (ua.last_stats[:, 6] == 1).all() and up.last_stats is None
    assert all(torch.equal(p, q) for p, q in zip(mp.parameters(), ma.parameters()))
    assert torch.equal(up.exp_avg, ua.exp_avg) and torch.equal(up.exp_avg_sq, ua.exp_avg_sq)
    kls = ua.last_stats[:, 4]
    T = float(kls[S]) / 1.2
    assert kls[:S].max() < 0.9 * T                          # the spiked minibatch stands out
    kw = dict(target_kl=T / 1.5, clip_range_vf=0.25)        # trips there
    m1, u1 = _run(collected, b32, "native", **kw)
    m2, u2 = _run(collected, b32, "native", **kw)
    assert u1.stopped_early and u1.steps_applied == S
    assert np.array_equal(u1.last_stats, u2.last_stats, equal_nan=True)
    assert all(torch.equal(p, q) for p, q in zip(m1.parameters(), m2.parameters()))
    assert torch.equal(u1.exp_avg, u2.exp_avg) and torch.equal(u1.exp_avg_sq, u2.exp_avg_sq)


# ---- 4. the stop word is sticky -------------------------------------------------------------------------------------------
def test_stop_word_is_sticky_across_calls(collected):
    """A call that really trips (at the spiked minibatch, the fourth of the first epoch), a second call handed the word still set, then the same call after zeroing it; and a word preset
    to another non-zero value."""
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    from cattleherd import _lib
    b, model, rb = collected
    b32, _ = _buffers(collected, s=3)
    perms = P.perms_of(SEED, N, 2, b.device)
    m = R.make_model(SHAPE, b.device, like=model)
    stop = torch.zeros(1, dtype=torch.int32, device=b.device)
    # the threshold from an armed run of the same epoch that never trips (bit-identical up to the trip, test 3)
    kls = _c_train(R.make_model(SHAPE, b.device, like=model), b32, perms[:1], 64,
                   opts=_lib.ChPpoOpts(1e6, 0.0, None, stop.data_ptr()))[0][:, 4].cpu().numpy()
    T = float(kls[3]) / 1.2
    print(f"approx_kl of the epoch: {kls}, T {T:.5f}")
    assert kls[:3].max() < 0.9 * T and int(stop) == 0
    o = _lib.ChPpoOpts(T / 1.5, 0.0, None, stop.data_ptr())
    first = _c_train(m, b32, perms[:1], 64, opts=o)
    assert first[4] == [0] and first[3] == 3 and int(stop) != 0
    assert list(first[0][:, 6].cpu()) == [1, 1, 1, 0, -1, -1, -1, -1] and float(first[0][3, 4]) == kls[3]
    word, state, before = int(stop), (first[1].clone(), first[2].clone()), _params(m)
    second = _c_train(m, b32, perms[1:], 64, opts=o, state=(first[1], first[2], torch.full_like(stop, 3, dtype=torch.int64)))
    assert second[4] == [0] and second[3] == 3 and int(stop) == word          # the step count and the word as they were
    assert torch.equal(second[1], state[0]) and torch.equal(second[2], state[1])
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), before))
    assert (second[0][:, 6] == -1).all() and torch.isnan(second[0][:, :6]).all()
    stop.zero_()
    o = _lib.ChPpoOpts(1e6, 0.0, None, stop.data_ptr())
    again = _c_train(m, b32, perms[1:], 64, opts=o, state=(second[1], second[2], torch.full_like(stop, 3, dtype=torch.int64)))
    assert again[3] == 11 and int(stop) == 0 and (again[0][:, 6] == 1).all()
    assert all(not torch.equal(p, q) for p, q in zip(m.parameters(), before))
    # any non-zero word stops, and stays what it was
    stop.fill_(3)
    held = _params(m)
    third = _c_train(m, b32, perms[:1], 64, opts=o)
    assert third[3] == 0 and int(stop) == 3 and (third[0][:, 6] == -1).all() and not third[1].any()
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), held))


# ---- 5. the value clip ----------------------------------------------------------------------------------------------------
SIGMA = 0.25
VSEED_LOOP = 22    # the loop's old-values seed, chosen on the float64 reference alone for the conditions it asserts


def _vf_case(which, batch):
    """ppo_native_ref's synthetic data with old values = ref64's own + N(0, SIGMA^2); the data conditions on ref64."""
    import torch
    import ppo_native_ref as R
    shape = getattr(R, which)
    dev = torch.device("cuda", 0)
    data64 = R.make_data(shape, dev)
    m32 = R.make_model(shape, dev)
    m64 = R.make_model(shape, dev, torch.float64, like=m32)
    with torch.no_grad():
        v, _, _ = m64.evaluate_actions(data64[0], data64[1])
    g = torch.Generator().manual_seed(21)    # chosen, on the float64 reference alone, for the conditions below
    old = (v + SIGMA * torch.randn(shape["rows"], generator=g, dtype=torch.float64).to(dev)).float().double()
    idx = R.idx_for(shape, batch).to(dev)
    dv = (v - old)[idx]
    assert ((dv.abs() - SIGMA).abs() > 1e-3 * SIGMA).all()
    if batch >= 8:
        frac = float((dv.abs() > SIGMA).double().mean())
        assert 0.1 <= frac <= 0.6 and (dv > SIGMA).any() and (dv < -SIGMA).any(), frac
    return shape, data64 + (old,), idx, m32, m64


def _ref_grad_vf(model, data, idx, c):
    import torch
    import ppo_native_ref as R
    upd = R.updater(model, clip_range_vf=c, **R.HP)
    for p in model.parameters():
        p.grad = None
    batch = [t.index_select(0, idx) for t in data]
    pl, vl, el, log_ratio, ratio = upd._terms(*batch)
    (pl + upd.ent_coef * el + upd.vf_coef * vl).backward()
    grads = [p.grad.detach().clone() for p in model.parameters()]
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    akl = torch.mean((ratio - 1) - log_ratio)
    return grads, torch.stack([pl, vl, -el, norm, akl]).detach()


def _native_grad_vf(model, data32, idx, c):
    """One ch_ppo_train_opt step with learning_rate = 0: the flat gradient from the scratch's last region."""
    import torch
    from cattleherd import _lib, ppo
    lib = ppo._bind()
    dev = model.device
    net = ppo.ppo_net(model)
    h = ppo.ChPpoHparams(0.0, 0.9, 0.999, 1e-5, 0.1, 0.1, 0.7, 0.5, 1, 0)
    d = ppo.ChPpoData(*(t.data_ptr() for t in data32[:5]), data32[0].shape[0])
    n = lib.ch_ppo_param_count(ctypes.byref(net))
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    stats = torch.zeros(7, device=dev)
    total = lib.ch_ppo_scratch_size(ctypes.byref(net), idx.numel())
    scratch = torch.full((total,), float("nan"), device=dev)
    o = _lib.ChPpoOpts(0.0, c, data32[5].data_ptr() if c else None, None)
    before = _params(model)
    _lib.check(lib.ch_ppo_train_opt(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), ctypes.byref(o), idx.data_ptr(),
                                    idx.numel(), idx.numel(), ea.data_ptr(), es.data_ptr(), step.data_ptr(),
                                    stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(step) == 1 and float(stats[6]) == 1.0
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))     # learning_rate 0 moves nothing
    return scratch[total - (n + 3) // 4 * 4:][:n].clone(), stats


@pytest.mark.parametrize("which,batch", [("DRIVER", 64), ("DRIVER", 40), ("DRIVER", 1), ("SMALL", 24)])
def test_value_clip_gradient_matches_float64_reference(which, batch):
    import torch
    import ppo_native_ref as R
    shape, data64, idx, m32, m64 = _vf_case(which, batch)
    data32 = tuple(t.float().contiguous() for t in data64)
    g64, s64 = _ref_grad_vf(m64, data64, idx, SIGMA)
    g32, s32 = _ref_grad_vf(m32, data32, idx, SIGMA)
    flat, stats = _native_grad_vf(m32, data32, idx, SIGMA)
    plain, _ = _native_grad_vf(m32, data32, idx, 0.0)
    assert torch.isfinite(flat).all()
    ok = True
    names = R.param_names(m32)
    for name, gn, gt, gr in zip(names, R.split_flat(flat, m32), g32, g64):
        ok &= R.accept(f"vf grad {which} B={batch} {name}", gn, gt, gr)
    for i, name in enumerate(("policy_loss", "value_loss", "entropy", "grad_norm", "approx_kl")):
        ok &= R.accept(f"vf stat {which} B={batch} {name}", stats[i:i + 1], s32[i:i + 1], s64[i:i + 1])
    assert ok
    if batch >= 8:     # a variant that ignored c would give the unclipped run's value-net gradient
        k = names.index("value_net.weight")
        assert not torch.equal(R.split_flat(flat, m32)[k], R.split_flat(plain, m32)[k])
        k = names.index("action_net.weight")
        assert torch.equal(R.split_flat(flat, m32)[k], R.split_flat(plain, m32)[k])


def test_value_clip_training_loop_matches_float64_reference(collected):
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    b, model, _ = collected
    b32, b64 = _buffers(collected, sigma=SIGMA, vseed=VSEED_LOOP)
    # the data conditions, on the float64 restatement of the loop alone: every minibatch's rows as its step saw them
    data64 = (b64.obs.view(N, -1), b64.actions.view(N, -1), b64.log_probs.view(N), b64.advantages.view(N),
              b64.returns.view(N), b64.values.view(N))
    ref = P.sb3_train(R.make_model(SHAPE, b.device, torch.float64, like=model), data64, P.perms_of(SEED, N, 2, b.device),
                      64, clip_range_vf=SIGMA)
    assert len(ref["clipped_rows"]) == 16
    for k, (dv, _) in enumerate(ref["clipped_rows"]):
        frac, both, margin = P.vf_conditions(dv, SIGMA)
        print(f"vf loop step {k}: clipped {frac:.3f}, nearest row to the bound {margin:.2e} c")
        assert 0.1 <= frac <= 0.6 and both and margin > 1e-3, k
    kw = dict(n_epochs=2, clip_range_vf=SIGMA)
    mn, un = _run(collected, b32, "native", **kw)
    mt, ut = _run(collected, b32, "torch", **kw)
    mr, ur = _run(collected, b64, "torch", torch.float64, **kw)
    mp, _ = _run(collected, b32, "native", n_epochs=2)
    assert un.steps_applied == 16 and (un.last_stats[:, 6] == 1).all()
    ok = True
    an, at, ar = _adam_state(mn, un), _adam_state(mt, ut), _adam_state(mr, ur)
    for name, pn, pt, pr in zip(R.param_names(mn), mn.parameters(), mt.parameters(), mr.parameters()):
        ok &= R.accept(f"vf loop param {name}", pn.detach(), pt.detach(), pr.detach())
    for i, name in enumerate(("m", "v")):
        ok &= R.accept(f"vf loop {name}", an[i], at[i], ar[i])
    assert ok
    assert not torch.equal(mn.value_net.weight, mp.value_net.weight)


# ---- 8. error paths -------------------------------------------------------------------------------------------------------
def test_error_paths_launch_nothing(collected):
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    from cattleherd import _lib, ppo
    from cattleherd.ppo import PPOUpdate
    b, model, rb = collected
    perms = P.perms_of(SEED, N, 1, b.device)
    m = R.make_model(SHAPE, b.device, like=model)
    stop = torch.zeros(1, dtype=torch.int32, device=b.device)
    for o, word in ((None, "opts"), (_lib.ChPpoOpts(0.0, 0.2, None, None), "old_values"),
                    (_lib.ChPpoOpts(0.01, 0.0, None, None), "stop_dev")):
        out = _c_train(m, rb, perms, 64, opts=o)
        assert out[4] == [_lib.CH_ERR_INVALID] and word in (ppo._bind().ch_last_error(None) or b"").decode()
        assert out[3] == 0 and (out[0] == 12345.0).all() and not out[1].any()
        assert all(torch.equal(p, q) for p, q in zip(m.parameters(), model.parameters()))
    with pytest.raises(ValueError, match="graph=False"):
        PPOUpdate(m, backend="torch", graph=True, target_kl=0.01)
    # rows beyond `steps` are never written
    out = _c_train(m, rb, [perms[0][:130].contiguous()], 64, opts=_lib.ChPpoOpts(1e6, 0.0, None, stop.data_ptr()), poison=2)
    assert out[3] == 3 and (out[0][:3, 6] == 1).all() and (out[0][3:] == 12345.0).all()


# ---- 9. schedules ---------------------------------------------------------------------------------------------------------
def test_schedules_on_the_native_backend(collected):
    import torch
    import ppo_native_ref as R
    from cattleherd.ppo import PPOUpdate
    b, model, rb = collected
    runs = []
    for kw in (dict(learning_rate=lambda p: 3e-4 * p, clip_range=lambda p: 0.2 * p), dict(learning_rate=1.5e-4, clip_range=0.1)):
        m = R.make_model(SHAPE, b.device, like=model)
        upd = PPOUpdate(m, batch_size=64, n_epochs=1, seed=SEED, backend="native", log_stats=True, **kw)
        upd.train(rb, progress_remaining=0.5)
        torch.cuda.synchronize()
        runs.append((m, upd))
    (ma, ua), (mb, ub) = runs
    assert all(torch.equal(p, q) for p, q in zip(ma.parameters(), mb.parameters()))
    assert torch.equal(ua.exp_avg, ub.exp_avg) and torch.equal(ua.exp_avg_sq, ub.exp_avg_sq)
    assert ua.last_log["train/learning_rate"] == 1.5e-4 and ua.last_log["train/clip_range"] == 0.1
    assert tuple(ub.last_log) == PPOUpdate.LOG_KEYS and tuple(ua.last_log) == PPOUpdate.LOG_KEYS + ("train/learning_rate",)
    assert {k: v for k, v in ua.last_log.items() if k != "train/learning_rate"} == ub.last_log
