"""The native PPO minibatch update (csrc/ch_ppo.hip through ch_ppo_grad / ch_ppo_adam / ch_ppo_train and
PPOUpdate(backend="native")) against the project's own torch restatement of SB3 PPO.train.

Reference and yardstick (tests/ppo_native_ref.py): ref64 is evaluate_actions + PPOUpdate._loss + clip_grad_norm_ +
torch.optim.Adam in float64 on copies of the same parameters and data; torch32 is the same code in float32 eager.  Per
tensor err(x) = max|x - ref64| / max|ref64|, and the native result passes when
err(native) <= 4 * max(err(torch32), 32 * 2**-24): the floor is sqrt(1032) units of f32 roundoff (the random-walk error
of the longest sum), the factor 4 the ordering noise of two valid f32 evaluations.  A wrong term (a missing 1/B, a
biased std, a dropped clamp branch, a bias correction one step off) sits orders of magnitude above that.

Inputs are synthetic and seeded on the host: CTDE-shaped observation rows (live features, then a zero tail), advantages
of both signs, old_log_prob = the model's own log-probability + N(0, 0.15^2) so that the surrogate really clips.  On
ref64 alone: 20-80 % of a minibatch's rows take the clipped branch, both clip edges occur, and no ratio lies within 1e-3
of an edge (so float32 and float64 agree on the branch); a one-row minibatch can only be 0 % or 100 % clipped, so the
first two are asked of minibatches of 8 rows and more.  No row is excluded.  Two more shapes have dense observations
(no zero tail) with obs_dim % 64 in 1..12 and, one of them, act_dim 33: the masked last pass of the kernels' K loops meets
non-zero data there.

Measured on an MI355X (each test prints its figures before it asserts), the largest err over a group's tensors,
err(native) / err(torch32):
  gradients 1032-128-128-48   batch 64: 1.45e-6 / 1.46e-6   40: 1.95e-6 / 2.47e-6   8: 1.85e-6 / 3.75e-6   1: 1.10e-6 / 5.03e-7
  statistics                  batch 64: 5.22e-5 / 5.22e-5   40: 4.30e-5 / 4.21e-5   8: 5.10e-6 / 1.28e-5   1: 8.50e-7 / 1.31e-7
  172-(64,32)/(32,64)-8, batch 24: gradients 5.94e-7 / 7.70e-7, statistics 6.26e-7 / 7.11e-7
  dense obs 72-(32,16)/(16,32)-33, batch 24: gradients 2.16e-6 / 1.62e-6, statistics 1.84e-6 / 3.72e-6
  dense obs 1032-128-128-48, batch 40: gradients 2.40e-6 / 1.66e-6, statistics 5.58e-6 / 2.37e-6
  clip + Adam x 3, max_grad_norm 0.5: params 1.37e-7 / 1.51e-7, m 1.51e-7 / 1.37e-7, v 2.15e-7 / 2.53e-7
  clip + Adam x 3, max_grad_norm 1e3: params 1.48e-7 / 1.48e-7, m 1.04e-7 / 2.08e-7, v 1.33e-7 / 1.25e-7
  ch_ppo_train's per-step statistics (2 steps, 64 then 32 rows): 1.02e-5 / 9.38e-6
  training loop: 16 steps of 64: 1.16e-6 / 1.74e-6; 22 steps of 48 (partial last minibatch): 1.01e-6 / 1.62e-6
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from ppo_native_ref import HP, idx_for as _idx  # noqa: E402


def _native_grad(model, data32, idx, **hp):
    import torch
    from cattleherd import ppo
    from cattleherd._lib import check
    lib = ppo._bind()
    net = ppo.ppo_net(model)
    h = ppo.ChPpoHparams(hp["learning_rate"], 0.9, 0.999, 1e-5, hp["clip_range"], hp["ent_coef"], hp["vf_coef"],
                         hp["max_grad_norm"], 1, 0)
    d = ppo.ChPpoData(*(t.data_ptr() for t in data32), data32[0].shape[0])
    n = lib.ch_ppo_param_count(ctypes.byref(net))
    assert n == sum(p.numel() for p in model.parameters())
    grad = torch.full((n,), float("nan"), device=model.device)
    stats = torch.zeros(4, device=model.device)
    scratch = torch.empty(lib.ch_ppo_scratch_size(ctypes.byref(net), idx.numel()), device=model.device)
    before = [p.detach().clone() for p in model.parameters()]
    check(lib.ch_ppo_grad(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), idx.data_ptr(), idx.numel(),
                          grad.data_ptr(), stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q)          # ch_ppo_grad updates nothing
    return grad, stats


@pytest.mark.parametrize("which,batch", [("DRIVER", 64), ("DRIVER", 40), ("DRIVER", 8), ("DRIVER", 1), ("SMALL", 24),
                                         ("DENSE", 24), ("DRIVER_DENSE", 40)])
def test_gradients_match_float64_reference(which, batch):
    import torch
    import ppo_native_ref as R
    shape = getattr(R, which)
    dev = torch.device("cuda", 0)
    data64 = R.make_data(shape, dev)
    data32 = tuple(t.float().contiguous() for t in data64)
    idx = _idx(shape, batch).to(dev)
    m32 = R.make_model(shape, dev)
    m64 = R.make_model(shape, dev, torch.float64, like=m32)
    g64, s64, ratio, clipped = R.ref_grad(m64, data64, idx, **HP)
    R.check_clip_conditions(ratio, clipped)
    g32, s32, _, _ = R.ref_grad(m32, data32, idx, **HP)
    flat, stats = _native_grad(m32, data32, idx, **HP)
    assert torch.isfinite(flat).all()
    ok = True
    for name, gn, gt, gr in zip(R.param_names(m32), R.split_flat(flat, m32), g32, g64):
        ok &= R.accept(f"grad {which} B={batch} {name}", gn, gt, gr)
    for i, name in enumerate(("policy_loss", "value_loss", "entropy", "grad_norm")):
        ok &= R.accept(f"stat {which} B={batch} {name}", stats[i:i + 1], s32[i:i + 1], s64[i:i + 1])
    assert ok


@pytest.mark.parametrize("max_grad_norm", [0.5, 1e3])
def test_clip_and_adam_match_float64_reference(max_grad_norm):
    """Three consecutive ch_ppo_adam steps from three given flat gradients: parameters, m, v and the step count."""
    import torch
    import ppo_native_ref as R
    from cattleherd import ppo
    from cattleherd._lib import check
    shape = R.DRIVER
    dev = torch.device("cuda", 0)
    mn = R.make_model(shape, dev)
    m32 = R.make_model(shape, dev, like=mn)
    m64 = R.make_model(shape, dev, torch.float64, like=mn)
    n = sum(p.numel() for p in mn.parameters())
    g = torch.Generator().manual_seed(11)
    grads = [(0.01 * (k + 1) * torch.randn(n, generator=g)).to(dev) for k in range(3)]
    opts = {}
    for m in (m32, m64):
        opts[m] = torch.optim.Adam(m.parameters(), lr=3e-4, eps=1e-5)
        for gf in grads:
            for p, gp in zip(m.parameters(), R.split_flat(gf, m)):
                p.grad = gp.to(p.dtype).clone()
            total = torch.nn.utils.clip_grad_norm_(m.parameters(), max_grad_norm)
            assert (float(total) > max_grad_norm) == (max_grad_norm < 1)   # clipping active at 0.5 only
            opts[m].step()
    lib = ppo._bind()
    net = ppo.ppo_net(mn)
    h = ppo.ChPpoHparams(3e-4, 0.9, 0.999, 1e-5, 0.1, 0.1, 0.7, max_grad_norm, 1, 0)
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.ch_ppo_scratch_size(ctypes.byref(net), 1), device=dev)
    for gf in grads:
        check(lib.ch_ppo_adam(ctypes.byref(net), ctypes.byref(h), gf.data_ptr(), ea.data_ptr(), es.data_ptr(),
                              step.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(step) == 3
    ok = True
    names = R.param_names(mn)
    for name, pn, pt, pr, an, sn in zip(names, mn.parameters(), m32.parameters(), m64.parameters(),
                                        R.split_flat(ea, mn), R.split_flat(es, mn)):
        st32, st64 = opts[m32].state[pt], opts[m64].state[pr]
        ok &= R.accept(f"adam {max_grad_norm} param {name}", pn.detach(), pt.detach(), pr.detach())
        ok &= R.accept(f"adam {max_grad_norm} m {name}", an, st32["exp_avg"], st64["exp_avg"])
        ok &= R.accept(f"adam {max_grad_norm} v {name}", sn, st32["exp_avg_sq"], st64["exp_avg_sq"])
    assert ok


def test_train_writes_each_step_s_statistics():
    """ch_ppo_train's optional stats [steps][4] (written by the Adam launch's first workgroup): two steps over the 96
    synthetic rows, 64 then a partial 32, against the float64 and float32 torch runs of the same two steps."""
    import torch
    import ppo_native_ref as R
    from cattleherd import ppo
    from cattleherd._lib import check
    shape = R.DRIVER
    dev = torch.device("cuda", 0)
    data64 = R.make_data(shape, dev)
    data32 = tuple(t.float().contiguous() for t in data64)
    perm = torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(21)).to(dev)
    mn = R.make_model(shape, dev)
    ref = {}
    for m, data in ((R.make_model(shape, dev, like=mn), data32), (R.make_model(shape, dev, torch.float64, like=mn), data64)):
        opt = torch.optim.Adam(m.parameters(), lr=HP["learning_rate"], eps=1e-5)
        rows = []
        for lo, hi in ((0, 64), (64, 96)):
            _, st, _, _ = R.ref_grad(m, data, perm[lo:hi], **HP)     # (leaves the gradients in p.grad)
            torch.nn.utils.clip_grad_norm_(m.parameters(), HP["max_grad_norm"])
            opt.step()
            rows.append(st)
        ref[data[0].dtype] = torch.stack(rows)
    lib = ppo._bind()
    net = ppo.ppo_net(mn)
    h = ppo.ChPpoHparams(HP["learning_rate"], 0.9, 0.999, 1e-5, HP["clip_range"], HP["ent_coef"], HP["vf_coef"],
                         HP["max_grad_norm"], 1, 0)
    d = ppo.ChPpoData(*(t.data_ptr() for t in data32), shape["rows"])
    n = lib.ch_ppo_param_count(ctypes.byref(net))
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    stats = torch.full((2, 4), float("nan"), device=dev)
    scratch = torch.empty(lib.ch_ppo_scratch_size(ctypes.byref(net), 64), device=dev)
    check(lib.ch_ppo_train(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), perm.data_ptr(), shape["rows"], 64,
                           ea.data_ptr(), es.data_ptr(), step.data_ptr(), stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(step) == 2
    ok = True
    for k in range(2):
        for i, name in enumerate(("policy_loss", "value_loss", "entropy", "grad_norm")):
            ok &= R.accept(f"train stats step {k} {name}", stats[k, i:i + 1], ref[torch.float32][k, i:i + 1],
                           ref[torch.float64][k, i:i + 1])
    assert ok


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


def _train(collected, backend, batch_size, dtype=None):
    import torch
    import ppo_native_ref as R
    from cattleherd.ppo import PPOUpdate
    b, model, rb = collected
    shape = dict(obs_dim=b.obs_rows * 86, act_dim=48, pi=(128, 128), vf=(128, 128))
    dtype = dtype or torch.float32
    m = R.make_model(shape, b.device, dtype, like=model)
    buf = rb if dtype == torch.float32 else R.fake_buffer(rb, dtype)
    upd = PPOUpdate(m, batch_size=batch_size, n_epochs=2, seed=5, graph=False, backend=backend)
    steps = upd.train(buf)
    torch.cuda.synchronize()
    assert upd.sgd_steps == steps
    return m, steps, upd


@pytest.mark.parametrize("batch_size,steps", [(64, 16), (48, 22)])
def test_training_loop_matches_float64_reference(collected, batch_size, steps):
    """PPOUpdate(backend="native").train against the float64 and float32 torch runs of the same minibatch sequence
    (512 rows: 16 steps of 64, or 2 x (10 of 48 + a partial one of 32))."""
    import torch
    import ppo_native_ref as R
    _, model, _ = collected
    mn, sn, upd = _train(collected, "native", batch_size)
    mt, st, _ = _train(collected, "torch", batch_size)
    mr, sr, _ = _train(collected, "torch", batch_size, torch.float64)
    assert sn == st == sr == steps
    assert int(upd.step_count) == steps
    ok = True
    for name, pn, pt, pr, p0 in zip(R.param_names(mn), mn.parameters(), mt.parameters(), mr.parameters(),
                                    model.parameters()):
        assert not torch.equal(pn, p0), name      # the update moved every parameter
        ok &= R.accept(f"train bs={batch_size} {name}", pn.detach(), pt.detach(), pr.detach())
    assert ok


def test_native_training_is_bit_reproducible(collected):
    import torch
    a, _, _ = _train(collected, "native", 64)
    b, _, _ = _train(collected, "native", 64)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)


def test_native_update_reaches_the_next_collection():
    """The native update writes the storage device_nets() hands the rollout kernels (tolerances:
    test_gpu_ppo.test_update_weights_reach_the_next_collection)."""
    import torch
    from cattleherd.env import HerdBatch
    from cattleherd.ppo import PPOUpdate, SB3ActorCritic
    from cattleherd.rollout import DeviceRolloutBuffer
    b = HerdBatch(64, 2, 8, mode="ctde", compat=False)
    b.reset()
    model = SB3ActorCritic(obs_dim=b.obs_rows * 86, act_dim=48, device=b.device, seed=0)
    actor, critic, log_std = model.device_nets()
    rb = DeviceRolloutBuffer(b, 8, act_dim=48)
    rb.collect(actor, critic, log_std, seed=1)
    before = [p.detach().clone() for p in model.parameters()]
    PPOUpdate(model, batch_size=64, n_epochs=1, backend="native").train(rb)
    actor, critic, log_std = model.device_nets()
    rb.collect(actor, critic, log_std, seed=2)
    torch.cuda.synchronize()
    assert all(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    with torch.no_grad():
        v, _, _ = model.evaluate_actions(rb.obs.view(-1, rb.obs.shape[-1]), rb.actions.view(-1, 48))
    assert np.allclose(rb.values.view(-1).cpu().numpy(), v.cpu().numpy(), rtol=1e-4, atol=1e-4)
    b.close()


def test_unsupported_architecture_raises_value_error():
    import torch
    from cattleherd.ppo import PPOUpdate, SB3ActorCritic
    model = SB3ActorCritic(obs_dim=172, act_dim=8, pi=(24, 24), vf=(32, 32), device=torch.device("cuda", 0))
    with pytest.raises(ValueError, match="multiples of 16"):
        PPOUpdate(model, backend="native")
