"""Host-only checks of the native MARL PPO update's C ABI (ch_marl_ppo_*), of RLlibActorCritic and of MarlPPOUpdate's
backend switch (no GPU: everything here is rejected or answered before any launch), and the data conditions of the
GPU tests' synthetic minibatches, which depend on the float64 reference alone."""
import ctypes

import pytest

SHAPES = ["DRIVER", "SMALL", "WIDE"]


def _net(obs_dim=86, act_dim=4, actor=(256, 256), critic=(256, 256)):
    from cattleherd import marl_ppo
    net = marl_ppo.ChMarlPpoNet()
    net.obs_dim, net.act_dim, net.n_actor, net.n_critic = obs_dim, act_dim, len(actor), len(critic)
    for i, w in enumerate(actor):
        net.actor[i] = w
    for i, w in enumerate(critic):
        net.critic[i] = w
    return net


@pytest.mark.parametrize("which", SHAPES)
def test_param_count_is_the_torch_model_s(which):
    import marl_ppo_ref as R
    from cattleherd import marl_ppo
    lib = marl_ppo._bind()
    shape = getattr(R, which)
    model = R.make_model(shape, "cpu")
    net = _net(shape["obs_dim"], shape["act_dim"], shape["hiddens"], shape["vf_hiddens"])
    n = lib.ch_marl_ppo_param_count(ctypes.byref(net))
    assert n == sum(p.numel() for p in model.parameters())
    assert lib.ch_marl_ppo_scratch_size(ctypes.byref(net), 128) > n
    assert lib.ch_marl_ppo_scratch_size(ctypes.byref(net), 0) == -1


@pytest.mark.parametrize("kw", [dict(actor=(300, 256)), dict(critic=(256, 24)), dict(act_dim=33), dict(obs_dim=0),
                                dict(actor=())])
def test_unsupported_nets_are_rejected_on_entry(kw):
    from cattleherd import _lib, marl_ppo
    lib = marl_ppo._bind()
    net = _net(**kw)
    assert lib.ch_marl_ppo_param_count(ctypes.byref(net)) == -1
    assert lib.ch_marl_ppo_scratch_size(ctypes.byref(net), 64) == -1
    # non-NULL arguments that are never read: the net is rejected before any pointer is used or anything is launched
    hp, data = marl_ppo.ChMarlPpoHparams(), marl_ppo.ChMarlPpoData()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    B = ctypes.byref
    assert lib.ch_marl_ppo_grad(B(net), B(hp), B(data), p, 1, p, p, p, None) == _lib.CH_ERR_UNSUPPORTED
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_grad: ")
    assert lib.ch_marl_ppo_adam(B(net), B(hp), p, p, p, p, p, None) == _lib.CH_ERR_UNSUPPORTED
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_adam: ")
    assert lib.ch_marl_ppo_train(B(net), B(hp), B(data), p, 1, 1, p, p, p, None, p, None) == _lib.CH_ERR_UNSUPPORTED
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_train: ")


def test_act_dim_32_is_the_widest_head():
    from cattleherd import marl_ppo
    lib = marl_ppo._bind()
    assert lib.ch_marl_ppo_param_count(ctypes.byref(_net(act_dim=32))) > 0
    assert lib.ch_marl_ppo_param_count(ctypes.byref(_net(act_dim=1))) > 0
    assert lib.ch_marl_ppo_param_count(ctypes.byref(_net(act_dim=0))) == -1


def test_null_arguments_are_invalid():
    from cattleherd import _lib, marl_ppo
    lib = marl_ppo._bind()
    B = ctypes.byref
    assert lib.ch_marl_ppo_param_count(None) == -1
    assert lib.ch_marl_ppo_scratch_size(None, 64) == -1
    assert lib.ch_marl_ppo_grad(None, None, None, None, 1, None, None, None, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_grad: ")
    assert lib.ch_marl_ppo_adam(None, None, None, None, None, None, None, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_adam: ")
    assert lib.ch_marl_ppo_train(None, None, None, None, 1, 1, None, None, None, None, None, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_train: ")
    # a supported net whose weight pointers are NULL
    net, hp, data = _net(), marl_ppo.ChMarlPpoHparams(), marl_ppo.ChMarlPpoData()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    assert lib.ch_marl_ppo_grad(B(net), B(hp), B(data), p, 1, p, p, p, None) == _lib.CH_ERR_INVALID
    assert b"NULL weight" in lib.ch_last_error(None)
    # weights and data given, the KL coefficient's device pointer not
    for arr in (net.actor_weight, net.actor_bias, net.critic_weight, net.critic_bias):
        for i in range(3):
            arr[i] = p
    data = marl_ppo.ChMarlPpoData(p, p, p, p, p, p, 1)
    assert lib.ch_marl_ppo_grad(B(net), B(hp), B(data), p, 1, p, p, p, None) == _lib.CH_ERR_INVALID
    assert b"NULL kl_coeff_dev" in lib.ch_last_error(None)
    assert lib.ch_marl_ppo_train(B(net), B(hp), B(data), p, 1, 1, p, p, p, None, p, None) == _lib.CH_ERR_INVALID
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_train: NULL kl_coeff_dev")


def test_backend_switch(monkeypatch):
    from cattleherd import marl_ppo
    model = marl_ppo.RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(32,), device="cpu")
    with pytest.raises(ValueError, match="bogus"):
        marl_ppo.MarlPPOUpdate(model, backend="bogus")
    monkeypatch.delenv("CH_PPO_BACKEND", raising=False)
    upd = marl_ppo.MarlPPOUpdate(model)
    assert upd.backend == "torch"
    # RLlib's defaults, so that a driver that sets none of them gets them
    assert (upd.lr, upd.betas, upd.eps, upd.clip_param, upd.vf_clip_param, upd.vf_loss_coeff, upd.entropy_coeff,
            upd.kl_target, upd.num_epochs, upd.minibatch_size, upd.grad_clip, upd.log_std_clip) == \
        (5e-5, (0.9, 0.999), 1e-8, 0.3, 10.0, 1.0, 0.0, 0.01, 30, 128, None, 20.0)
    assert abs(float(upd.kl_coeff) - 0.2) < 1e-7 and tuple(upd.kl_coeff.shape) == (1,)
    monkeypatch.setenv("CH_PPO_BACKEND", "bogus")
    with pytest.raises(ValueError):
        marl_ppo.MarlPPOUpdate(model)
    assert marl_ppo.MarlPPOUpdate(model, backend="torch").backend == "torch"
    with pytest.raises(ValueError, match="multiples of 16"):
        marl_ppo.MarlPPOUpdate(marl_ppo.RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(24,), device="cpu"),
                               backend="native")
    with pytest.raises(ValueError, match="CUDA"):     # a supported net, but on the host: no CPU path exists
        marl_ppo.MarlPPOUpdate(model, backend="native")
    monkeypatch.setenv("CH_PPO_BACKEND", "native")
    with pytest.raises(ValueError, match="CUDA"):     # the environment variable reaches the same switch
        marl_ppo.MarlPPOUpdate(model)
    # the message is the library's own reason, not one text for every rejection
    with pytest.raises(ValueError, match=r"act_dim must be 1\.\.32"):
        marl_ppo.MarlPPOUpdate(marl_ppo.RLlibActorCritic(obs_dim=22, act_dim=33, hiddens=(32,), device="cpu"),
                               backend="native")


def test_host_only_calls_leave_their_reason():
    from cattleherd import marl_ppo
    lib = marl_ppo._bind()
    assert lib.ch_marl_ppo_param_count(ctypes.byref(_net(obs_dim=0))) == -1
    assert lib.ch_last_error(None) == b"ch_marl_ppo_param_count: obs_dim must be >= 1"
    assert lib.ch_marl_ppo_scratch_size(ctypes.byref(_net(actor=(24, 256))), 64) == -1
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_scratch_size: hidden widths must be multiples of 16")
    assert lib.ch_marl_ppo_scratch_size(ctypes.byref(_net()), 0) == -1
    assert lib.ch_last_error(None).startswith(b"ch_marl_ppo_scratch_size: batch_size")


def test_default_device_without_a_gpu_says_what_to_do():
    import torch
    from cattleherd.marl_ppo import RLlibActorCritic
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError, match="device='cpu'"):
        RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(32,))


def test_construction_leaves_the_global_generator_alone():
    import torch
    from cattleherd.marl_ppo import RLlibActorCritic
    torch.manual_seed(1234)
    torch.rand(3)
    before = torch.random.get_rng_state()
    a = RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(32, 16), device="cpu", seed=5)
    assert torch.equal(torch.random.get_rng_state(), before)
    b = RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(32, 16), device="cpu", seed=5)
    c = RLlibActorCritic(obs_dim=22, act_dim=3, hiddens=(32, 16), device="cpu", seed=6)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))     # seeded
    assert not torch.equal(a.pi.weight, c.pi.weight)


def test_state_dict_and_load_weights_round_trip():
    import numpy as np
    import torch
    from cattleherd.marl_ppo import RLlibActorCritic
    a = RLlibActorCritic(device="cpu", seed=1)
    sd = a.state_dict_rllib()
    assert sorted(sd) == sorted(f"{k}.{s}" for k in ("encoder.actor_encoder.net.mlp.0", "encoder.actor_encoder.net.mlp.2",
                                                     "pi.net.mlp.0", "encoder.critic_encoder.net.mlp.0",
                                                     "encoder.critic_encoder.net.mlp.2", "vf.net.mlp.0")
                                for s in ("weight", "bias"))
    assert tuple(sd["pi.net.mlp.0.weight"].shape) == (8, 256) and tuple(sd["vf.net.mlp.0.weight"].shape) == (1, 256)
    assert sd["pi.net.mlp.0.weight"] is a.pi.weight                          # live tensors, no copies
    assert sum(v.numel() for v in sd.values()) == sum(p.numel() for p in a.parameters())
    weights = {k: v.detach().numpy().copy() for k, v in sd.items()}          # an algo.get_weights()[policy]-style dict
    weights["pi.log_std_clip_param_const"] = np.array([20.0], np.float32)
    b = RLlibActorCritic(device="cpu", seed=2)
    assert not torch.equal(a.pi.weight, b.pi.weight)
    ptr = b.pi.weight.data_ptr()
    b.load_weights(weights)
    assert b.pi.weight.data_ptr() == ptr                                     # in place
    for k, v in b.state_dict_rllib().items():
        assert np.array_equal(v.detach().numpy(), weights[k]), k
    del weights["vf.net.mlp.0.bias"]
    with pytest.raises(KeyError):
        b.load_weights(weights)
    weights["vf.net.mlp.0.bias"] = np.zeros(2, np.float32)
    with pytest.raises(ValueError, match="shape"):
        b.load_weights(weights)


def test_torch_update_on_a_cpu_buffer_and_no_live_row():
    """The torch backend runs anywhere torch does: live rows only (dead rows poisoned with NaN), the step count, the
    per-step statistics, the KL coefficient's three branches; a buffer without a live row raises."""
    import types
    import torch
    from cattleherd.marl_ppo import MarlPPOUpdate, RLlibActorCritic
    g = torch.Generator().manual_seed(0)
    T, rows, A = 4, 10, 3
    mask = torch.ones(T, rows, dtype=torch.uint8)
    mask[1:, ::3] = 0
    dead = mask == 0
    rb = types.SimpleNamespace(T=T, rows=rows, agent_mask=mask, obs=torch.randn(T, rows, 22, generator=g),
                               actions=torch.randn(T, rows, A, generator=g), log_probs=-4.0 + 0.3 * torch.randn(T, rows, generator=g),
                               advantages=torch.randn(T, rows, generator=g), returns=torch.randn(T, rows, generator=g))
    rb.obs[dead] = float("nan")
    rb.advantages[dead] = float("nan")
    live = int(mask.sum())
    for kl_target, factor in ((1e-9, 1.5), (1e9, 0.5)):
        model = RLlibActorCritic(obs_dim=22, act_dim=A, hiddens=(32, 16), device="cpu", seed=0)
        before = [p.detach().clone() for p in model.parameters()]
        upd = MarlPPOUpdate(model, num_epochs=2, minibatch_size=8, kl_target=kl_target, backend="torch")
        steps = upd.train(rb)
        assert steps == upd.sgd_steps == 2 * -(-live // 8) and tuple(upd.stats.shape) == (steps, 5)
        assert torch.isfinite(upd.stats).all() and all(torch.isfinite(p).all() for p in model.parameters())
        assert all(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
        assert float(upd.kl_coeff) == pytest.approx(0.2 * factor, rel=1e-6)
    rb.agent_mask = torch.zeros_like(mask)
    with pytest.raises(ValueError, match="no live row"):
        upd.train(rb)


@pytest.mark.parametrize("which,batch,clamp", __import__("marl_ppo_ref").GRAD_CASES +
                         __import__("marl_ppo_ref").LIMIT_GRAD_CASES)
def test_synthetic_minibatches_meet_the_data_conditions(which, batch, clamp):
    """The GPU tests' inputs, on the float64 reference alone (marl_ppo_ref.check_conditions)."""
    import torch
    import marl_ppo_ref as R
    shape = getattr(R, which)
    data64 = R.make_data(shape, "cpu", clamp)
    m64 = R.make_model(shape, "cpu", torch.float64, clamp=clamp)
    hp = R.hp_for(clamp)
    _, stats, aux = R.ref_grad(m64, data64, R.idx_for(shape, batch, clamp), hp)
    R.check_conditions(aux, hp, clamp, stats)
    assert (data64[4] > 0).any() and (data64[4] < 0).any()


@pytest.mark.parametrize("eps", [__import__("marl_ppo_ref").TRAIN_EPS, 1e-8])
@pytest.mark.parametrize("n_idx,batch,steps", __import__("marl_ppo_ref").TRAIN_CASES)
def test_training_minibatches_meet_the_data_conditions(n_idx, batch, steps, eps):
    """Every step of the GPU tests' ch_marl_ppo_train runs (Adam eps TRAIN_EPS, and RLlib's 1e-8 for the per-step
    statistics), in the float64 reference run of the same steps."""
    import torch
    import marl_ppo_ref as R
    shape = R.DRIVER
    data64 = R.make_data(shape, "cpu")
    m64 = R.make_model(shape, "cpu", torch.float64)
    perm = torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(R.TRAIN_SEED))[:n_idx]
    aux, hp = [], R.hp_for(eps=eps)
    stats = R.ref_epoch(m64, R.adam(m64, hp), data64, perm, batch, hp, aux_out=aux)
    assert stats.shape[0] == steps == len(aux)
    for a, row in zip(aux, stats):
        R.check_conditions(a, hp, False, row)


def test_limit_training_minibatches_meet_the_data_conditions():
    """SMALL_ROWS's 1100 rows in minibatches of 530 (530, 530 and a partial 40), every step of the float64 run."""
    import torch
    import marl_ppo_ref as R
    shape = R.SMALL_ROWS
    n_idx, batch, steps = R.LIMIT_TRAIN_CASE
    data64 = R.make_data(shape, "cpu")
    m64 = R.make_model(shape, "cpu", torch.float64)
    perm = torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(R.LIMIT_TRAIN_SEED))[:n_idx]
    aux, hp = [], R.hp_for(eps=R.TRAIN_EPS)
    stats = R.ref_epoch(m64, R.adam(m64, hp), data64, perm, batch, hp, aux_out=aux)
    assert stats.shape[0] == steps == len(aux) and [a["ratio"].numel() for a in aux] == [530, 530, 40]
    for a, row in zip(aux, stats):
        R.check_conditions(a, hp, False, row)
