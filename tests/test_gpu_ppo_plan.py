"""The native PPO update's dispatch on the device: every training entry of the C ABI, and *_grad / *_adam of both
flavours, launches the rows csrc/ch_ppo.h's plan gives (tests/test_ppo_plan_cpu.py asserts the plan itself with no
device), and writes exactly steps x width words of statistics.

One small shape for all of them: obs 20, policy MLP (16,), value MLP (16, 16), act 3 (RLlib head 6), 40 rows in
minibatches of 24 -- two steps, 24 rows (two tiles, the second ragged) then 16 (one tile).  Weights from the model
constructors with a fixed seed, data seeded; target_kl = 1e6 arms the KL gate without tripping it.  Every call is a
valid one; what the kernels compute is the other PPO tests' business."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

OBS, ACT, ROWS, BATCH, STEPS = 20, 3, 40, 24, 2
POISON = 12345.0
SB3_TRAIN = ("k_ppo_fb<0>", "k_ppo_dw<0>", "k_ppo_adam<0>")
RLLIB_TRAIN = ("k_ppo_fb<1>", "k_ppo_dw<1>", "k_ppo_adam<1>")
# entry -> (flavour, the step's rows, update bits, statistics columns (a name: the constant of cattleherd._lib))
CASES = {
    "ch_ppo_train": ("sb3", SB3_TRAIN, 1, 4),
    "ch_ppo_train_log": ("sb3", ("k_ppo_fb<2>", "k_ppo_dw<0>", "k_ppo_adam<0>"), 3, "CH_PPO_LOG_STATS"),
    "ch_ppo_train_opt": ("sb3", ("k_ppo_fb_opt<4>", "k_ppo_dw_opt", "k_ppo_adam_opt"), 3, "CH_PPO_OPT_STATS"),
    "ch_ppo_train_opt+vf": ("sb3", ("k_ppo_fb_opt<5>", "k_ppo_dw_opt", "k_ppo_adam_opt"), 3, "CH_PPO_OPT_STATS"),
    "ch_marl_ppo_train": ("rllib", RLLIB_TRAIN, 1, 5),
    "ch_marl_ppo_train_log": ("rllib", ("k_ppo_fb<3>", "k_ppo_dw<1>", "k_ppo_adam<3>"), 3, "CH_MARL_PPO_LOG_STATS"),
    "ch_ppo_grad": ("sb3", SB3_TRAIN, 0, 4),
    "ch_marl_ppo_grad": ("rllib", RLLIB_TRAIN, 0, 5),
    "ch_ppo_adam": ("sb3", ("none", "k_ppo_sumsq", "k_ppo_adam<0>"), 1, 0),
    "ch_marl_ppo_adam": ("rllib", ("none", "k_ppo_sumsq", "k_ppo_adam<1>"), 1, 0),
}


@pytest.fixture(scope="module")
def setup():
    """Per flavour: the model, its net / hparams / data structs and the tensors they point to (kept alive here)."""
    import torch
    from cattleherd import _lib, marl_ppo, ppo
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)

    def rand(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=g)).to(dev)

    obs, act, lp, adv, ret = rand(ROWS, OBS, scale=0.5), rand(ROWS, ACT), rand(ROWS, scale=0.1) - 3.0, rand(ROWS), rand(ROWS)
    old_dist = torch.cat([rand(ROWS, ACT, scale=0.3), rand(ROWS, ACT, scale=0.1) - 1.0], dim=1).contiguous()
    old_values, klc = rand(ROWS), torch.full((1,), 0.2, device=dev)
    idx = torch.randperm(ROWS, generator=g).to(dev)
    out = {"idx": idx, "old_values": old_values, "keep": (obs, act, lp, adv, ret, old_dist, klc)}
    m = ppo.SB3ActorCritic(obs_dim=OBS, act_dim=ACT, pi=(16,), vf=(16, 16), device=dev, seed=0)
    out["sb3"] = (m, ppo.ppo_net(m), _lib.ChPpoHparams(3e-4, 0.9, 0.999, 1e-5, 0.1, 0.1, 0.7, 0.5, 1, 0),
                  _lib.ChPpoData(*(t.data_ptr() for t in (obs, act, lp, adv, ret)), ROWS))
    m = marl_ppo.RLlibActorCritic(obs_dim=OBS, act_dim=ACT, hiddens=(16,), vf_hiddens=(16, 16), device=dev, seed=0)
    out["rllib"] = (m, marl_ppo.marl_ppo_net(m),
                    _lib.ChMarlPpoHparams(5e-5, 0.9, 0.999, 1e-8, 0.3, 10.0, 1.0, 0.01, 20.0, 0.0, klc.data_ptr()),
                    _lib.ChMarlPpoData(*(t.data_ptr() for t in (obs, act, lp, old_dist, adv, ret)), ROWS))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_entry_launches_the_plans_rows(setup, case):
    import torch
    from cattleherd import _lib
    lib = _lib.lib()
    flavour, rows, update, width = CASES[case]
    width = getattr(_lib, width) if isinstance(width, str) else width
    model, net, hp, data = setup[flavour]
    dev, idx = model.device, setup["idx"]
    pre = "ch_ppo_" if flavour == "sb3" else "ch_marl_ppo_"
    n = getattr(lib, pre + "param_count")(ctypes.byref(net))
    assert n == sum(p.numel() for p in model.parameters())
    scratch = torch.empty(getattr(lib, pre + "scratch_size")(ctypes.byref(net), BATCH), device=dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    entry = case.split("+")[0]
    steps = STEPS if "train" in entry else 1
    stats = torch.full((steps * width + 16,), POISON, device=dev)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    lead = [ctypes.byref(net), ctypes.byref(hp)]
    if entry.endswith("_adam"):
        grad = torch.full((n,), 0.01, device=dev)
        rc = getattr(lib, entry)(*lead, grad.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), scratch.data_ptr(), None)
    elif entry.endswith("_grad"):
        grad = torch.zeros(n, device=dev)
        rc = getattr(lib, entry)(*lead, ctypes.byref(data), idx.data_ptr(), BATCH, grad.data_ptr(), stats.data_ptr(),
                                 scratch.data_ptr(), None)
    else:
        lead.append(ctypes.byref(data))
        if entry == "ch_ppo_train_opt":
            opts = _lib.ChPpoOpts(1e6, 0.2 if case.endswith("+vf") else 0.0, setup["old_values"].data_ptr(), stop.data_ptr())
            lead.append(ctypes.byref(opts))
        rc = getattr(lib, entry)(*lead, idx.data_ptr(), ROWS, BATCH, m.data_ptr(), v.data_ptr(), step.data_ptr(),
                                 stats.data_ptr(), scratch.data_ptr(), None)
    _lib.check(rc)
    torch.cuda.synchronize()
    grid = 1 if update == 0 else min((n + 1023) // 1024, 512)
    got = _lib.ppo_last_step()
    print(case, got)
    assert got == (*rows, update, grid)
    # exactly steps x width words written, all finite: the rest still holds the poison
    assert torch.isfinite(stats).all()
    assert int((stats[:steps * width] != POISON).sum()) == steps * width
    assert bool((stats[steps * width:] == POISON).all())
    assert int(step) == (0 if entry.endswith("_grad") else steps)
    if entry == "ch_ppo_train_opt":   # the gate is armed and does not trip: every step applied, the word untouched
        assert stats[:steps * width].view(steps, width)[:, 6].tolist() == [1.0] * steps and int(stop) == 0
