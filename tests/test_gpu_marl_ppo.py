"""The native MARL (RLlib-style) PPO minibatch update (csrc/ch_ppo.hip's kPpoRllib kernels through ch_marl_ppo_grad /
ch_marl_ppo_adam / ch_marl_ppo_train and MarlPPOUpdate(backend="native")) against the project's own torch
restatement of RLlib's PPO learner (RLlib is not installed: parity unpinned to its source).

Reference and yardstick (tests/marl_ppo_ref.py): ref64 is the restated loss + optional global-norm clip +
torch.optim.Adam in float64 on copies of the same parameters and data; torch32 is the same code in float32 eager on
the same GPU.  Per tensor err(x) = max|x - ref64| / max|ref64|, and the native result passes when
err(native) <= 4 * max(err(torch32), 32 * 2**-24) (tests/test_gpu_ppo_native.py's rule, unchanged).  A tensor that is
exactly zero in ref64 (a branch whose loss terms are switched off) must be exactly zero natively.

Inputs are synthetic and seeded on the host; tests/test_marl_ppo_cpu.py holds them to the data conditions on ref64
alone (both surrogate clip edges, the value clip on some rows only, KL > 0, the three log_std clamp regions, nothing
near a branch point).  Observations are 86 wide in the DRIVER shape: rows that are not 16-byte aligned, so layer 1
takes the kernels' non-vector path.  Each test prints its figures before it asserts.

Measured on an MI355X, the largest err over a group's tensors, err(native) / err(torch32):
  gradients 86-256-256-(8, 1)  batch 128: 5.5e-7 / 6.1e-7   40: 8.2e-7 / 1.1e-6   8: 1.5e-6 / 1.3e-6   1: 5.9e-7 / 5.1e-7
  stats5                       batch 128: 1.3e-7 / 1.3e-7   40: 6.4e-8 / 1.2e-7   8: 5.7e-7 / 1.0e-7   1: 4.8e-7 / 9.5e-7
  SMALL batch 24: gradients 2.9e-7 / 3.7e-7, stats5 1.2e-7 / 3.6e-7;  WIDE batch 24: 2.9e-6 / 2.9e-6, 7.5e-7 / 3.6e-7
  log_std_clip 0.5: SMALL 6.0e-7 / 9.3e-7, 2.5e-7 / 4.3e-7;  DRIVER batch 128: 2.6e-5 / 2.6e-5, 3.1e-7 / 4.2e-7
  one term alone, gradients: KL 1.9e-7 / 3.0e-7, entropy 1.6e-7 / 1.9e-7, clipped value 2.0e-7 / 2.5e-7
  Adam x 3 (params): no clip 1.5e-7 / 1.5e-7, clip 0.5 1.5e-7 / 1.5e-7
  ch_marl_ppo_train: 6 x 128 params 2.2e-6 / 7.4e-7, stats5 2.8e-7 / 2.8e-7; 4 x 48 + 32 params 2.5e-6 / 4.3e-6
  ch_marl_ppo_train at Adam eps 1e-8, 6 x 128: per-step stats5 2.1e-7 / 1.7e-7
  MarlPPOUpdate.train on a collected buffer: params 3.9e-6 / 2.0e-6, stats5 3.9e-7 / 3.6e-7
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAT_NAMES = ("policy_loss", "vf_loss", "entropy", "kl", "grad_norm")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _hparams(hp, klc):
    from cattleherd import marl_ppo
    return marl_ppo.ChMarlPpoHparams(hp["lr"], 0.9, 0.999, hp["eps"], hp["clip_param"], hp["vf_clip_param"],
                                     hp["vf_loss_coeff"], hp["entropy_coeff"], hp["log_std_clip"],
                                     hp["grad_clip"] if hp["grad_clip"] is not None else 0.0, klc.data_ptr())


def _native_grad(model, data32, idx, hp):
    import torch
    from cattleherd import marl_ppo
    from cattleherd._lib import check
    lib = marl_ppo._bind()
    net = marl_ppo.marl_ppo_net(model)
    klc = torch.full((1,), hp["kl_coeff"], dtype=torch.float32, device=model.device)
    h = _hparams(hp, klc)
    d = marl_ppo.ChMarlPpoData(*(t.data_ptr() for t in data32), data32[0].shape[0])
    n = lib.ch_marl_ppo_param_count(ctypes.byref(net))
    assert n == sum(p.numel() for p in model.parameters())
    grad = torch.full((n,), float("nan"), device=model.device)
    stats = torch.full((5,), float("nan"), device=model.device)
    scratch = torch.empty(lib.ch_marl_ppo_scratch_size(ctypes.byref(net), idx.numel()), device=model.device)
    before = [p.detach().clone() for p in model.parameters()]
    check(lib.ch_marl_ppo_grad(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), idx.data_ptr(), idx.numel(),
                               grad.data_ptr(), stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q)          # ch_marl_ppo_grad updates nothing
    return grad, stats


_DATA = {}


def _data(shape, clamp):
    """The shape's synthetic data (float64 and float32 on the GPU), made once and left unchanged."""
    import marl_ppo_ref as R
    key = (shape["name"], clamp)
    if key not in _DATA:
        d64 = R.make_data(shape, _dev(), clamp)
        _DATA[key] = (d64, tuple(t.float().contiguous() for t in d64))
    return _DATA[key]


def _compare_grad(tag, shape, batch, clamp, hp, zero_adv=False):
    import torch
    import marl_ppo_ref as R
    dev = _dev()
    data64, data32 = _data(shape, clamp)
    if zero_adv:   # the surrogate has no coefficient: zero advantages switch it off
        data64 = data64[:4] + (torch.zeros_like(data64[4]),) + data64[5:]
        data32 = data32[:4] + (torch.zeros_like(data32[4]),) + data32[5:]
    idx = R.idx_for(shape, batch, clamp).to(dev)
    m32 = R.make_model(shape, dev, clamp=clamp)
    m64 = R.make_model(shape, dev, torch.float64, like=m32, clamp=clamp)
    g64, s64, _ = R.ref_grad(m64, data64, idx, hp)
    g32, s32, _ = R.ref_grad(m32, data32, idx, hp)
    flat, stats = _native_grad(m32, data32, idx, hp)
    assert torch.isfinite(flat).all() and torch.isfinite(stats).all()
    ok = True
    for name, gn, gt, gr in zip(R.param_names(m32), R.split_flat(flat, m32), g32, g64):
        ok &= R.accept(f"grad {tag} {name}", gn, gt, gr)
    for i, name in enumerate(STAT_NAMES):
        ok &= R.accept(f"stat {tag} {name}", stats[i:i + 1], s32[i:i + 1], s64[i:i + 1])
    return ok, g64, s64


@pytest.mark.parametrize("which,batch,clamp", __import__("marl_ppo_ref").GRAD_CASES)
def test_gradients_match_float64_reference(which, batch, clamp):
    import marl_ppo_ref as R
    ok, g64, _ = _compare_grad(f"{which} B={batch} clamp={clamp}", getattr(R, which), batch, clamp, R.hp_for(clamp))
    assert all(float(g.abs().max()) > 0.0 for g in g64)     # every parameter takes part
    assert ok


@pytest.mark.parametrize("term", ["kl", "entropy", "vf"])
def test_each_loss_term_alone(term):
    """Zero advantages and the other coefficients at 0 leave one term: a wrong sign or a missing 1 / B in it cannot
    hide behind the surrogate.  The clamp case (log_std_clip 0.5), so that the term's clamped columns are in play."""
    import marl_ppo_ref as R
    hp = R.hp_for(True, vf_loss_coeff=0.0, entropy_coeff=0.0, kl_coeff=0.0)
    hp.update({"kl": dict(kl_coeff=0.7), "entropy": dict(entropy_coeff=0.3), "vf": dict(vf_loss_coeff=0.6)}[term])
    ok, g64, s64 = _compare_grad(f"only {term}", R.SMALL, 24, True, hp, zero_adv=True)
    names = R.param_names(R.make_model(R.SMALL, "cpu"))
    for name, g in zip(names, g64):   # the term reaches its own branch, and only that one
        mine = name.startswith("critic") or name.startswith("vf") if term == "vf" else \
            name.startswith("actor") or name.startswith("pi")
        assert (float(g.abs().max()) > 0.0) == mine, name
    assert float(s64[0]) == 0.0
    assert ok


@pytest.mark.parametrize("grad_clip", [None, 0.5])
def test_clip_and_adam_match_float64_reference(grad_clip):
    """Three consecutive ch_marl_ppo_adam steps from three given flat gradients: parameters, m, v and the step count.
    grad_clip None: the coefficient is exactly 1, against an unclipped torch Adam (eps 1e-8)."""
    import torch
    import marl_ppo_ref as R
    from cattleherd import marl_ppo
    from cattleherd._lib import check
    shape, dev = R.DRIVER, _dev()
    hp = R.hp_for(grad_clip=grad_clip)
    mn = R.make_model(shape, dev)
    m32 = R.make_model(shape, dev, like=mn)
    m64 = R.make_model(shape, dev, torch.float64, like=mn)
    n = sum(p.numel() for p in mn.parameters())
    g = torch.Generator().manual_seed(11)
    grads = [(0.01 * (k + 1) * torch.randn(n, generator=g)).to(dev) for k in range(3)]
    assert float(torch.linalg.vector_norm(grads[0])) > 0.5      # the clip at 0.5 is active
    opts = {}
    for m in (m32, m64):
        opts[m] = R.adam(m, hp)
        for gf in grads:
            for p, gp in zip(m.parameters(), R.split_flat(gf, m)):
                p.grad = gp.to(p.dtype).clone()
            R.clip_and_step(m, opts[m], grad_clip)
    lib = marl_ppo._bind()
    net = marl_ppo.marl_ppo_net(mn)
    klc = torch.full((1,), 0.2, device=dev)
    h = _hparams(hp, klc)
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.ch_marl_ppo_scratch_size(ctypes.byref(net), 1), device=dev)
    for gf in grads:
        check(lib.ch_marl_ppo_adam(ctypes.byref(net), ctypes.byref(h), gf.data_ptr(), ea.data_ptr(), es.data_ptr(),
                                   step.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(step) == 3
    ok = True
    for name, pn, pt, pr, an, sn in zip(R.param_names(mn), mn.parameters(), m32.parameters(), m64.parameters(),
                                        R.split_flat(ea, mn), R.split_flat(es, mn)):
        st32, st64 = opts[m32].state[pt], opts[m64].state[pr]
        ok &= R.accept(f"adam {grad_clip} param {name}", pn.detach(), pt.detach(), pr.detach())
        ok &= R.accept(f"adam {grad_clip} m {name}", an, st32["exp_avg"], st64["exp_avg"])
        ok &= R.accept(f"adam {grad_clip} v {name}", sn, st32["exp_avg_sq"], st64["exp_avg_sq"])
    assert ok


def _native_epoch(model, data32, perm, batch, hp, steps):
    import torch
    from cattleherd import marl_ppo
    from cattleherd._lib import check
    dev = model.device
    lib = marl_ppo._bind()
    net = marl_ppo.marl_ppo_net(model)
    klc = torch.full((1,), hp["kl_coeff"], dtype=torch.float32, device=dev)
    h = _hparams(hp, klc)
    d = marl_ppo.ChMarlPpoData(*(t.data_ptr() for t in data32), data32[0].shape[0])
    n = lib.ch_marl_ppo_param_count(ctypes.byref(net))
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    stats = torch.full((steps, 5), float("nan"), device=dev)
    scratch = torch.empty(lib.ch_marl_ppo_scratch_size(ctypes.byref(net), batch), device=dev)
    check(lib.ch_marl_ppo_train(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), perm.data_ptr(), perm.numel(),
                                batch, ea.data_ptr(), es.data_ptr(), step.data_ptr(), stats.data_ptr(),
                                scratch.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(step) == steps
    return stats


@pytest.mark.parametrize("n_idx,batch,steps", __import__("marl_ppo_ref").TRAIN_CASES)
def test_train_matches_float64_reference_and_is_reproducible(n_idx, batch, steps):
    """ch_marl_ppo_train over a caller-drawn index list: the final parameters and every step's stats5 against the
    float64 and float32 torch runs of the same steps; a second run from the same state gives the same bits.  Adam eps
    is marl_ppo_ref.TRAIN_EPS (the reasoning and the measurement are there)."""
    import torch
    import marl_ppo_ref as R
    shape, dev, hp = R.DRIVER, _dev(), R.hp_for(eps=R.TRAIN_EPS)
    data64, data32 = _data(shape, False)
    perm = torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(R.TRAIN_SEED))[:n_idx].to(dev)
    m0 = R.make_model(shape, dev)
    m32 = R.make_model(shape, dev, like=m0)
    m64 = R.make_model(shape, dev, torch.float64, like=m0)
    s32 = R.ref_epoch(m32, R.adam(m32, hp), data32, perm, batch, hp)
    s64 = R.ref_epoch(m64, R.adam(m64, hp), data64, perm, batch, hp)
    mn, mn2 = R.make_model(shape, dev, like=m0), R.make_model(shape, dev, like=m0)
    sn = _native_epoch(mn, data32, perm, batch, hp, steps)
    sn2 = _native_epoch(mn2, data32, perm, batch, hp, steps)
    assert torch.equal(sn, sn2)
    for p, q in zip(mn.parameters(), mn2.parameters()):
        assert torch.equal(p, q)
    ok = True
    for name, pn, pt, pr, p0 in zip(R.param_names(mn), mn.parameters(), m32.parameters(), m64.parameters(),
                                    m0.parameters()):
        assert not torch.equal(pn, p0), name      # the update moved every parameter
        ok &= R.accept(f"train {n_idx}/{batch} {name}", pn.detach(), pt.detach(), pr.detach())
    for k in range(steps):
        for i, name in enumerate(STAT_NAMES):
            ok &= R.accept(f"train {n_idx}/{batch} step {k} {name}", sn[k, i:i + 1], s32[k, i:i + 1], s64[k, i:i + 1])
    assert ok


def test_train_with_rllib_s_adam_eps_matches_on_every_step_s_statistics():
    """The same 6 steps of 128 with Adam eps 1e-8, RLlib's default: every step's stats5 against the float64 and
    float32 runs.  (The parameters are not compared at this eps: single elements with |g| of the order of eps make
    any two float32 runs differ beyond the rule, marl_ppo_ref.TRAIN_EPS.  The statistics are means over the
    minibatch and see the whole trajectory.)"""
    import torch
    import marl_ppo_ref as R
    n_idx, batch, steps = R.TRAIN_CASES[0]
    shape, dev, hp = R.DRIVER, _dev(), R.hp_for()
    assert hp["eps"] == 1e-8
    data64, data32 = _data(shape, False)
    perm = torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(R.TRAIN_SEED))[:n_idx].to(dev)
    m0 = R.make_model(shape, dev)
    m32 = R.make_model(shape, dev, like=m0)
    m64 = R.make_model(shape, dev, torch.float64, like=m0)
    s32 = R.ref_epoch(m32, R.adam(m32, hp), data32, perm, batch, hp)
    s64 = R.ref_epoch(m64, R.adam(m64, hp), data64, perm, batch, hp)
    mn = R.make_model(shape, dev, like=m0)
    sn = _native_epoch(mn, data32, perm, batch, hp, steps)
    assert all(torch.isfinite(p).all() and not torch.equal(p, q) for p, q in zip(mn.parameters(), m0.parameters()))
    ok = True
    for k in range(steps):
        for i, name in enumerate(STAT_NAMES):
            ok &= R.accept(f"train eps 1e-8 step {k} {name}", sn[k, i:i + 1], s32[k, i:i + 1], s64[k, i:i + 1])
    assert ok


def test_construction_leaves_the_cuda_generators_alone():
    """RLlibActorCritic seeds its initialisation without touching the global generators, the GPU's included."""
    import torch
    from cattleherd.marl_ppo import RLlibActorCritic
    dev = _dev()
    torch.cuda.manual_seed_all(4321)
    torch.rand(3, device=dev)
    cpu, cuda = torch.random.get_rng_state(), [s.clone() for s in torch.cuda.get_rng_state_all()]
    a = RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(32, 16), device=dev, seed=5)
    assert torch.equal(torch.random.get_rng_state(), cpu)
    assert all(torch.equal(s, t) for s, t in zip(torch.cuda.get_rng_state_all(), cuda))
    b = RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(32, 16), device="cpu", seed=5)
    assert all(torch.equal(p.cpu(), q) for p, q in zip(a.parameters(), b.parameters()))   # the same on every device


# ---- MarlPPOUpdate.train end to end on a real buffer -----------------------------------------------------------
E2E = dict(num_epochs=2, minibatch_size=48, seed=5)
E2E_HP = dict(lr=3e-4, eps=__import__("marl_ppo_ref").TRAIN_EPS)


@pytest.fixture(scope="module")
def collected():
    """8 envs x (4 drones, 16 cattle), T = 8, collected once with the model's own nets; agents drop out."""
    import torch
    import marl_ppo_ref as R
    from cattleherd.marl_ppo import RLlibActorCritic
    from cattleherd.rollout import DeviceMarlRolloutBuffer
    b = R.make_marl_batch(8, 4, 16)
    model = RLlibActorCritic(device=b.device, seed=0)
    rb = DeviceMarlRolloutBuffer(b, 8)
    rb.collect(*model.device_nets(), seed=1)
    torch.cuda.synchronize()
    mask = rb.agent_mask != 0
    assert mask.any() and not mask.all()
    # what dead rows hold must not matter: poison their observations and advantages
    rb.obs[~mask] = float("nan")
    rb.advantages[~mask] = float("nan")
    yield b, model, rb, int(mask.sum())
    b.close()


def _e2e_shape():
    return dict(obs_dim=86, act_dim=4, hiddens=(256, 256), vf_hiddens=(256, 256))


def _run(collected, backend, kl_target=0.01):
    import torch
    import marl_ppo_ref as R
    from cattleherd.marl_ppo import MarlPPOUpdate
    _, model, rb, _ = collected
    m = R.make_model(_e2e_shape(), rb.obs.device, like=model)
    upd = MarlPPOUpdate(m, kl_target=kl_target, backend=backend, **E2E, **E2E_HP)
    steps = upd.train(rb)
    torch.cuda.synchronize()
    assert upd.sgd_steps == steps and tuple(upd.stats.shape) == (steps, 5)
    return m, steps, upd


def _ref_run(collected, dtype, kl_target=0.01):
    import torch
    import marl_ppo_ref as R
    _, model, rb, _ = collected
    m = R.make_model(_e2e_shape(), rb.obs.device, dtype, like=model)
    buf = rb if dtype == torch.float32 else R.fake_buffer(rb, dtype)
    steps, stats, klc = R.ref_train(m, buf, R.hp_for(**E2E_HP), kl_target, E2E["num_epochs"], E2E["minibatch_size"],
                                    E2E["seed"])
    return m, steps, stats, klc


def test_update_trains_on_live_rows_only_and_matches_float64_reference(collected):
    import torch
    import marl_ppo_ref as R
    _, model, _, live = collected
    want = E2E["num_epochs"] * -(-live // E2E["minibatch_size"])
    mn, sn, un = _run(collected, "native")
    mt, st, ut = _run(collected, "torch")
    mr, sr, stats64, _ = _ref_run(collected, torch.float64)
    print(f"live rows {live}, steps {sn}")
    assert sn == st == sr == want and int(un.step_count) == want
    ok = True
    for name, pn, pt, pr, p0 in zip(R.param_names(mn), mn.parameters(), mt.parameters(), mr.parameters(),
                                    model.parameters()):
        assert torch.isfinite(pn).all() and torch.isfinite(pt).all(), name
        assert not torch.equal(pn, p0), name
        ok &= R.accept(f"e2e {name}", pn.detach(), pt.detach(), pr.detach())
    assert torch.isfinite(un.stats).all() and torch.isfinite(ut.stats).all()
    for i, name in enumerate(STAT_NAMES):   # each statistic's column over the steps
        ok &= R.accept(f"e2e stats {name}", un.stats[:, i], ut.stats[:, i], stats64[:, i])
    assert ok


def test_kl_coefficient_follows_the_reference_on_all_three_branches(collected):
    """kl_target chosen around the last minibatch's mean KL of the float64 run: x 1.5, x 0.5, unchanged."""
    import torch
    _, _, stats64, _ = _ref_run(collected, torch.float64)
    kl = float(stats64[-1, 3])
    assert kl > 0.0
    for kl_target, factor in ((kl / 4.0, 1.5), (kl * 4.0, 0.5), (kl, 1.0)):
        _, _, _, want = _ref_run(collected, torch.float64, kl_target)
        assert float(want) == pytest.approx(0.2 * factor, rel=1e-6)
        for backend in ("native", "torch"):
            _, _, upd = _run(collected, backend, kl_target)
            assert upd.kl_coeff.dtype == torch.float32 and tuple(upd.kl_coeff.shape) == (1,)
            assert torch.equal(upd.kl_coeff.cpu(), want.cpu()), (backend, kl_target)


def test_collect_after_train_uses_the_updated_weights():
    """The native update writes the storage device_nets() hands the rollout kernels: the next collection's
    log-probabilities and values are the updated model's (2e-5, as test_gpu_policy.py holds the MFMA forward)."""
    import torch
    import marl_ppo_ref as R
    from cattleherd.marl_ppo import MarlPPOUpdate, RLlibActorCritic
    from cattleherd.rollout import DeviceMarlRolloutBuffer
    b = R.make_marl_batch(8, 4, 16)
    model = RLlibActorCritic(device=b.device, seed=0)
    policy, value = model.device_nets()
    rb = DeviceMarlRolloutBuffer(b, 8)
    rb.collect(policy, value, seed=1)
    before = [p.detach().clone() for p in model.parameters()]
    MarlPPOUpdate(model, num_epochs=2, minibatch_size=48, lr=1e-3, backend="native").train(rb)
    rb.collect(policy, value, seed=2)      # the same DevicePolicy objects: they read the parameters' storage
    torch.cuda.synchronize()
    assert all(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    mask = (rb.agent_mask != 0).view(-1)
    obs, act = rb.obs.view(-1, 86)[mask], rb.actions.view(-1, 4)[mask]
    with torch.no_grad():
        mean, _, ls, v = R.head(model, obs, 20.0)
        lp = R.log_prob(act, mean, ls)
        old = [torch.nn.functional.linear(torch.tanh(torch.nn.functional.linear(torch.tanh(
            torch.nn.functional.linear(obs, before[0], before[1])), before[2], before[3])), before[8], before[9])]
    got = rb.log_probs.view(-1)[mask]
    assert np.allclose(got.cpu().numpy(), lp.cpu().numpy(), rtol=2e-5, atol=2e-5)
    assert np.allclose(rb.values.view(-1)[mask].cpu().numpy(), v.cpu().numpy(), rtol=2e-5, atol=2e-5)
    lp_old = R.log_prob(act, old[0][:, :4], old[0][:, 4:].clamp(-20.0, 20.0))
    assert float((got - lp_old).abs().max()) > 1e-3      # and not the weights from before the update
    b.close()


def test_unsupported_architecture_raises_value_error():
    from cattleherd.marl_ppo import MarlPPOUpdate, RLlibActorCritic
    model = RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(24, 24), device=_dev())
    with pytest.raises(ValueError, match="multiples of 16"):
        MarlPPOUpdate(model, backend="native")
