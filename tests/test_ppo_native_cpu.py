"""Host-only checks of the native PPO update's C ABI and of PPOUpdate's backend switch (no GPU: everything here is
rejected or answered before any launch), and the data conditions of the GPU tests' synthetic minibatches, which depend
on the float64 reference alone."""
import ctypes

import pytest


def _net(obs_dim=1032, act_dim=48, pi=(128, 128), vf=(128, 128)):
    from cattleherd import ppo
    net = ppo.ChPpoNet()
    net.obs_dim, net.act_dim, net.n_pi, net.n_vf = obs_dim, act_dim, len(pi), len(vf)
    for i, w in enumerate(pi):
        net.pi[i] = w
    for i, w in enumerate(vf):
        net.vf[i] = w
    return net


def test_param_count_is_the_torch_model_s():
    from cattleherd import ppo
    lib = ppo._bind()
    model = ppo.SB3ActorCritic(device="cpu")
    assert lib.ch_ppo_param_count(ctypes.byref(_net())) == sum(p.numel() for p in model.parameters())
    small = ppo.SB3ActorCritic(obs_dim=172, act_dim=8, pi=(64,), vf=(32, 64), device="cpu")
    assert lib.ch_ppo_param_count(ctypes.byref(_net(172, 8, (64,), (32, 64)))) == sum(p.numel() for p in small.parameters())
    assert lib.ch_ppo_scratch_size(ctypes.byref(_net()), 64) > lib.ch_ppo_param_count(ctypes.byref(_net()))
    assert lib.ch_ppo_scratch_size(ctypes.byref(_net()), 0) == -1


@pytest.mark.parametrize("kw", [dict(pi=(300, 128)), dict(vf=(128, 24)), dict(act_dim=65), dict(obs_dim=0),
                                dict(pi=())])
def test_unsupported_nets_are_rejected_on_entry(kw):
    from cattleherd import _lib, ppo
    lib = ppo._bind()
    net = _net(**kw)
    assert lib.ch_ppo_param_count(ctypes.byref(net)) == -1
    assert lib.ch_ppo_scratch_size(ctypes.byref(net), 64) == -1
    # non-NULL arguments that are never read: the net is rejected before any pointer is used or anything is launched
    hp, data = ppo.ChPpoHparams(), ppo.ChPpoData()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    assert lib.ch_ppo_grad(ctypes.byref(net), ctypes.byref(hp), ctypes.byref(data), p, 1, p, p, p, None) == _lib.CH_ERR_UNSUPPORTED
    assert lib.ch_last_error(None).startswith(b"ch_ppo_grad: ")
    assert lib.ch_ppo_adam(ctypes.byref(net), ctypes.byref(hp), p, p, p, p, p, None) == _lib.CH_ERR_UNSUPPORTED
    assert lib.ch_last_error(None).startswith(b"ch_ppo_adam: ")
    assert lib.ch_ppo_train(ctypes.byref(net), ctypes.byref(hp), ctypes.byref(data), p, 1, 1, p, p, p, None, p, None) == _lib.CH_ERR_UNSUPPORTED
    assert lib.ch_last_error(None).startswith(b"ch_ppo_train: ")


def test_null_arguments_are_invalid():
    from cattleherd import _lib, ppo
    lib = ppo._bind()
    assert lib.ch_ppo_param_count(None) == -1
    assert lib.ch_ppo_grad(None, None, None, None, 1, None, None, None, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None).startswith(b"ch_ppo_grad: ")
    assert lib.ch_ppo_adam(None, None, None, None, None, None, None, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None).startswith(b"ch_ppo_adam: ")
    assert lib.ch_ppo_train(None, None, None, None, 1, 1, None, None, None, None, None, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None).startswith(b"ch_ppo_train: ")
    # a supported net whose weight pointers are NULL
    net, hp, data = _net(), ppo.ChPpoHparams(), ppo.ChPpoData()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    assert lib.ch_ppo_grad(ctypes.byref(net), ctypes.byref(hp), ctypes.byref(data), p, 1, p, p, p, None) == _lib.CH_ERR_INVALID
    assert b"NULL weight" in lib.ch_last_error(None)


def test_backend_switch(monkeypatch):
    from cattleherd import ppo
    model = ppo.SB3ActorCritic(obs_dim=172, act_dim=8, pi=(32,), vf=(32,), device="cpu")
    with pytest.raises(ValueError, match="bogus"):
        ppo.PPOUpdate(model, graph=False, backend="bogus")
    monkeypatch.delenv("CH_PPO_BACKEND", raising=False)
    assert ppo.PPOUpdate(model, graph=False).backend == "torch"
    monkeypatch.setenv("CH_PPO_BACKEND", "bogus")
    with pytest.raises(ValueError):
        ppo.PPOUpdate(model, graph=False)
    assert ppo.PPOUpdate(model, graph=False, backend="torch").backend == "torch"
    with pytest.raises(ValueError, match="multiples of 16"):
        ppo.PPOUpdate(ppo.SB3ActorCritic(obs_dim=172, act_dim=8, pi=(24,), vf=(32,), device="cpu"), graph=False,
                      backend="native")
    with pytest.raises(ValueError, match="CUDA"):     # a supported net, but on the host: no CPU path exists
        ppo.PPOUpdate(ppo.SB3ActorCritic(obs_dim=172, act_dim=8, pi=(32,), vf=(32,), device="cpu"), graph=False,
                      backend="native")


def test_host_only_calls_leave_their_reason():
    from cattleherd import ppo
    lib = ppo._bind()
    assert lib.ch_ppo_param_count(ctypes.byref(_net(obs_dim=0))) == -1
    assert lib.ch_last_error(None) == b"ch_ppo_param_count: obs_dim must be >= 1"
    assert lib.ch_ppo_scratch_size(ctypes.byref(_net(pi=(24, 128))), 64) == -1
    assert lib.ch_last_error(None).startswith(b"ch_ppo_scratch_size: ")
    # the message is the library's own reason, not one text for every rejection
    with pytest.raises(ValueError, match=r"act_dim must be 1\.\.64"):
        ppo.PPOUpdate(ppo.SB3ActorCritic(obs_dim=172, act_dim=65, pi=(32,), vf=(32,), device="cpu"), graph=False,
                      backend="native")


@pytest.mark.parametrize("which,batch", [("DRIVER", 64), ("DRIVER", 40), ("DRIVER", 8), ("DRIVER", 1), ("SMALL", 24),
                                         ("DENSE", 24), ("DRIVER_DENSE", 40)] + __import__("ppo_native_ref").LIMIT_CASES)
def test_synthetic_minibatches_meet_the_clip_conditions(which, batch):
    """The GPU tests' inputs, on the float64 reference alone: the surrogate really clips, on both edges, and no ratio
    sits where float32 and float64 could disagree on the branch.  The gapped-noise shapes (ppo_native_ref.LIMIT_CASES)
    keep every ratio 1e-2 away from an edge; their clipped fractions: SMALL_ROWS 0.374 (530 rows) and 0.354 (1030),
    WIDE 0.500, MANY_WG 0.312, EDGE_A 0.458, EDGE_B 0.333, EDGE_C 0.417."""
    import numpy as np
    import torch
    import ppo_native_ref as R
    shape = getattr(R, which)
    data64 = R.make_data(shape, "cpu")
    m64 = R.make_model(shape, "cpu", torch.float64)
    _, stats, ratio, clipped = R.ref_grad(m64, data64, R.idx_for(shape, batch), **R.HP)
    R.check_clip_conditions(ratio, clipped)
    assert torch.isfinite(stats).all()
    assert (data64[3] > 0).any() and (data64[3] < 0).any()
    if shape.get("gapped"):
        r = ratio.numpy()
        print(f"{which} B={batch}: clipped fraction {float(clipped.double().mean()):.3f}")
        assert min(np.abs(r - (1 - R.CLIP)).min(), np.abs(r - (1 + R.CLIP)).min()) > 1e-2


def test_limit_training_minibatches_meet_the_clip_conditions():
    """SMALL_ROWS's training sequence (1100 rows in minibatches of 530: 530, 530 and 40 rows) in the float64 reference
    run of the three steps: the first minibatch meets check_clip_conditions by construction, the later ones -- on
    weights that one and two Adam steps moved -- keep 20-80 % of their rows clipped and both edges populated; the rows
    that an update carried to within 1e-3 of an edge are counted (the GPU test's clip_fraction allows exactly those)."""
    import numpy as np
    import torch
    import ppo_native_ref as R
    import train_log_ref as T
    shape = R.SMALL_ROWS
    data64 = R.make_data(shape, "cpu")
    ref = T.update_reference(R.make_model(shape, "cpu", torch.float64), data64, R.limit_train_perm(), R.LIMIT_TRAIN_BATCH, R.HP)
    assert [r[3].numel() for r in ref] == [530, 530, 40]
    R.check_clip_conditions(ref[0][3], ref[0][4])
    for k, (st, akl, count, ratio, clipped) in enumerate(ref):
        r = ratio.numpy()
        near = int(((np.abs(r - (1 - R.CLIP)) <= 1e-3) | (np.abs(r - (1 + R.CLIP)) <= 1e-3)).sum())
        frac = float(clipped.double().mean())
        print(f"step {k}: clipped {frac:.3f}, clip count {count}, rows within 1e-3 of an edge {near}, approx_kl {float(akl):.5f}")
        assert torch.isfinite(st).all() and 0.2 <= frac <= 0.8 and (r < 1 - R.CLIP).any() and (r > 1 + R.CLIP).any()
