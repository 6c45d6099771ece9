"""Shared pieces of the native MARL (RLlib-style) PPO update's tests (test_gpu_marl_ppo.py, test_marl_ppo_cpu.py):
seeded synthetic minibatch data, an independent torch restatement of the loss, of the optional global-norm clip +
Adam step and of the training loop (run in float64 as the reference and in float32 as the yardstick), and the
project's error measure err(x) = max|x - ref64| / max|ref64| with its acceptance rule
err(native) <= 4 * max(err(torch32), 32 * 2**-24) (tests/ppo_native_ref.py's, unchanged).

Shapes: DRIVER, SMALL and WIDE at the driver's sizes (minibatches of up to 128 rows), and SMALL_ROWS, EDGE_1, EDGE_32
beyond them (LIMIT_GRAD_CASES, LIMIT_TRAIN_CASE; test_gpu_ppo_limits.py).  check_conditions' margins are narrow enough
(1e-4 at a ratio edge, a relative 1e-3 at vf_clip_param, 1e-3 at +-log_std_clip) that under make_data's Gaussian noise
a minibatch of 530 rows expects about 0.1 rows inside one of them, so the index seeds are still found by search on the
float64 reference and this module needs no gapped noise; ppo_native_ref's SB3 data, whose 1e-3 ratio margin expects
4.5 such rows at 530, does (ppo_native_ref.gapped_noise)."""
import math
import types

import numpy as np
import torch

from ppo_native_ref import FACTOR, FLOOR, accept, err, split_flat  # noqa: F401

# RLlib's defaults, with a learning rate at which a few steps move the parameters well above float32 roundoff
HP = dict(lr=3e-4, eps=1e-8, clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2,
          grad_clip=None, log_std_clip=20.0)
# Multi-step runs from real gradients use Adam eps 1e-5.  With RLlib's 1e-8 a parameter's step lr * m / (sqrt(v) + eps)
# has the sensitivity lr / eps = 3e4 to the gradient wherever |g| <~ eps, so a gradient rounding of 1e-10 moves that
# parameter by 3e-6, 3e-5 of the first layer's largest weight: some element of a 22 k-entry tensor sits there, and any
# two float32 evaluations then differ by more than the rule allows.  Measured on an MI355X with eps 1e-8 (6 steps of
# 128): err(torch32) up to 6.6e-5 on one weight matrix where err(native) was 6.1e-6, and the reverse (2.3e-5 against
# 2.3e-6) on another, every per-step statistic within 2.2e-7.  eps 1e-8 itself is pinned by the ch_marl_ppo_adam test,
# whose given gradients (N(0, 0.01^2 .. 0.03^2)) keep clear of that range.
TRAIN_EPS = 1e-5
CLAMP = 0.5   # log_std_clip of the clamp cases

# idx_seed[(batch, clamp)]: chosen so that the float64 reference meets check_conditions
DRIVER = dict(name="DRIVER", obs_dim=86, hiddens=(256, 256), vf_hiddens=(256, 256), act_dim=4, rows=768, seed=3,
              idx_seed={(128, False): 1, (40, False): 1, (8, False): 3, (1, False): 3, (128, True): 1})
SMALL = dict(name="SMALL", obs_dim=22, hiddens=(32, 16), vf_hiddens=(16, 32), act_dim=3, rows=96, seed=4,
             idx_seed={(24, False): 1, (24, True): 1})
WIDE = dict(name="WIDE", obs_dim=40, hiddens=(64,), vf_hiddens=(64,), act_dim=32, rows=96, seed=6,
            idx_seed={(24, False): 1})
# every (shape, batch, clamp) whose gradient the GPU tests take
GRAD_CASES = [("DRIVER", 128, False), ("DRIVER", 40, False), ("DRIVER", 8, False), ("DRIVER", 1, False),
              ("SMALL", 24, False), ("WIDE", 24, False), ("SMALL", 24, True), ("DRIVER", 128, True)]
# ch_marl_ppo_train: (rows of the index list, minibatch) -> 6 steps of 128; 4 steps of 48 and one of 32
TRAIN_CASES = [(768, 128, 6), (224, 48, 5)]
TRAIN_SEED = 21
# Beyond the driver's sizes (test_gpu_ppo_limits.py).  SMALL_ROWS: SMALL's net over 1100 rows, a minibatch of 530 -- 34
# row tiles with 2 rows in the last, two passes of the explained variance's 256-thread loops -- and the 1100 rows in
# minibatches of 530 (530, 530, 40).  EDGE_1 / EDGE_32: obs_dim 257 (a scalar first layer one column into a second
# 256-column k-group of the weight gradient), a one-hidden-layer actor, a critic of 240 and 144 (15 and 9 column tiles
# over 8 waves), the narrowest and the widest head.
SMALL_ROWS = dict(SMALL, name="SMALL_ROWS", rows=1100, seed=14, idx_seed={(530, False): 1})
EDGE_1 = dict(name="EDGE_1", obs_dim=257, hiddens=(16,), vf_hiddens=(240, 144), act_dim=1, rows=96, seed=17,
              idx_seed={(24, False): 1})
EDGE_32 = dict(EDGE_1, name="EDGE_32", act_dim=32, seed=18)
LIMIT_GRAD_CASES = [("SMALL_ROWS", 530, False), ("EDGE_1", 24, False), ("EDGE_32", 24, False)]
LIMIT_TRAIN_CASE = (1100, 530, 3)    # (rows of the index list, minibatch, steps) on SMALL_ROWS
LIMIT_TRAIN_SEED = 1                 # the permutation's seed, chosen like idx_seed: every step meets check_conditions


def hp_for(clamp=False, **kw):
    hp = dict(HP, **kw)
    if clamp:
        hp["log_std_clip"] = CLAMP
    return hp


def idx_for(shape, batch, clamp=False):
    """`batch` distinct rows of the data in a seeded order: non-contiguous, the last row always among them (a one-row
    minibatch is a row on the unclipped branch of both the surrogate and the value loss, so that all three terms reach
    the gradient)."""
    g = torch.Generator().manual_seed(shape["idx_seed"][(batch, clamp)])
    perm = torch.randperm(shape["rows"] - 1, generator=g)[:batch]
    if batch > 1:
        perm[batch // 2] = shape["rows"] - 1
    return perm


def make_model(shape, device, dtype=torch.float32, like=None, clamp=False):
    """An RLlibActorCritic of `shape` (seeded init, the same on every device).  `clamp`: pi's log_std biases are set
    to +1.5, -1.5, 0, ... so that with log_std_clip 0.5 some raw log_std outputs sit above +c, some below -c and some
    inside.  `like`: copy another model's parameters."""
    from cattleherd.marl_ppo import RLlibActorCritic
    m = RLlibActorCritic(obs_dim=shape["obs_dim"], act_dim=shape["act_dim"], hiddens=shape["hiddens"],
                         vf_hiddens=shape["vf_hiddens"], device=device, seed=0)
    if clamp:
        A = shape["act_dim"]
        with torch.no_grad():
            m.pi.bias[A:] = torch.tensor([1.5, -1.5, 0.0] * A)[:A].to(m.pi.bias)
    if dtype == torch.float64:
        m.modules.double()
    if like is not None:
        with torch.no_grad():
            for p, q in zip(m.parameters(), like.parameters()):
                p.copy_(q.to(p.dtype))
    return m


def head(model, obs, c):
    """mean, raw log_std, clamped log_std of the policy, and the values."""
    z = model.pi(model.actor_encoder(obs))
    A = model.act_dim
    return z[:, :A], z[:, A:], torch.clamp(z[:, A:], -c, c), model.vf(model.critic_encoder(obs)).flatten()


def make_data(shape, device, clamp=False):
    """Float64 data of `rows` live agent rows, as float32 buffers would hold it: dense observations; actions drawn
    from the model's own Gaussian; old_log_prob = the model's log-probability + N(0, 0.6^2), so that the surrogate
    clips on both edges; old dist inputs = the model's + N(0, 0.1^2), so KL > 0; advantages N(0.5, 1) (both signs, and a policy loss that does not cancel to nothing);
    value targets = the model's value -+ an error drawn from [0.5, 2.5] or from [3.6, 5], so that the value clip at
    10 is active on about half of the rows.  (obs, actions, old_log_prob, old_dist, advantages, value_targets)."""
    g = torch.Generator().manual_seed(shape["seed"] + (100 if clamp else 0))
    R, D, A = shape["rows"], shape["obs_dim"], shape["act_dim"]
    c = CLAMP if clamp else HP["log_std_clip"]

    def rn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float64)
    obs = (0.5 * rn(R, D)).float().double()
    m64 = make_model(shape, "cpu", torch.float64, clamp=clamp)
    with torch.no_grad():
        mean, _, ls, v = head(m64, obs, c)
        act = (mean + torch.exp(ls) * rn(R, A)).float().double()
        lp = log_prob(act, mean, ls)
        old = (lp + 0.6 * rn(R)).float().double()
        dist = torch.cat([mean + 0.1 * rn(R, A), ls + 0.1 * rn(R, A)], 1).float().double()
        adv = (0.5 + rn(R)).float().double()
        u = torch.rand(R, 3, generator=g, dtype=torch.float64)
        e = torch.where(u[:, 0] < 0.5, 0.5 + 2.0 * u[:, 1], 3.6 + 1.4 * u[:, 1]) * torch.where(u[:, 2] < 0.5, -1.0, 1.0)
        ret = (v + e).float().double()
    return tuple(t.to(device) for t in (obs, act, old, dist, adv, ret))


def log_prob(act, mean, ls):
    return (-((act - mean) ** 2) / (2.0 * torch.exp(2.0 * ls)) - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)


def loss(model, mb, hp, kl_coeff=None):
    """The issue's loss of one minibatch (obs, actions, old_log_prob, old_dist, advantages, value_targets), in the
    model's dtype: total, [policy loss, value loss, mean entropy, mean KL] and what check_conditions looks at."""
    obs, act, old_lp, old_dist, adv, ret = mb
    A, c = model.act_dim, hp["log_std_clip"]
    mean, raw, ls, v = head(model, obs, c)
    mean_p, ls_p = old_dist[:, :A], old_dist[:, A:]
    ratio = torch.exp(log_prob(act, mean, ls) - old_lp)
    s1, s2 = adv * ratio, adv * torch.clamp(ratio, 1.0 - hp["clip_param"], 1.0 + hp["clip_param"])
    surr = torch.min(s1, s2)
    ent = (ls + 0.5 + 0.5 * math.log(2.0 * math.pi)).sum(-1)
    kl = (ls - ls_p + (torch.exp(2.0 * ls_p) + (mean_p - mean) ** 2) / (2.0 * torch.exp(2.0 * ls)) - 0.5).sum(-1)
    e2 = (v - ret) ** 2
    vf = torch.clamp(e2, 0.0, hp["vf_clip_param"])
    klc = hp["kl_coeff"] if kl_coeff is None else kl_coeff.to(kl.dtype).reshape(())
    total = torch.mean(-surr + hp["vf_loss_coeff"] * vf - hp["entropy_coeff"] * ent) + klc * torch.mean(kl)
    stats = torch.stack([-surr.mean(), vf.mean(), ent.mean(), kl.mean()]).detach()
    aux = dict(ratio=ratio.detach(), clipped=(s2 < s1).detach(), e2=e2.detach(), raw=raw.detach(), kl=kl.detach())
    return total, stats, aux


def ref_grad(model, data, idx, hp, kl_coeff=None):
    """Gradient (a list per parameter), stats5 and the condition inputs of one minibatch."""
    for p in model.parameters():
        p.grad = None
    total, st, aux = loss(model, tuple(t.index_select(0, idx) for t in data), hp, kl_coeff)
    total.backward()
    grads = [p.grad.detach().clone() for p in model.parameters()]
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    return grads, torch.cat([st, norm.reshape(1)]), aux


def clip_and_step(model, opt, grad_clip):
    """The issue's clip (none: coefficient exactly 1; else min(1, c / (norm + 1e-6)) on the global norm) and Adam."""
    if grad_clip is not None:
        params = model.parameters()
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
        coef = torch.clamp(grad_clip / (norm + 1e-6), max=1.0)
        for p in params:
            p.grad.mul_(coef.to(p.grad.dtype))
    opt.step()


def adam(model, hp):
    return torch.optim.Adam(model.parameters(), lr=hp["lr"], betas=(0.9, 0.999), eps=hp["eps"])


def ref_epoch(model, opt, data, idx, batch, hp, kl_coeff=None, aux_out=None):
    """ceil(len(idx) / batch) consecutive minibatch steps over idx; the per-step stats5 [steps, 5]."""
    rows = []
    for j in range(0, idx.numel(), batch):
        _, st, aux = ref_grad(model, data, idx[j:j + batch], hp, kl_coeff)
        clip_and_step(model, opt, hp["grad_clip"])
        rows.append(st)
        if aux_out is not None:
            aux_out.append(aux)
    return torch.stack(rows)


def ref_train(model, rb, hp, kl_target, num_epochs, minibatch_size, seed):
    """The issue's training iteration over a buffer's fields (any dtype): the live rows, the sampling policy's dist
    inputs, advantages standardised over the live rows (population std, floor 1e-4), a fresh permutation of the live
    rows per epoch from a generator seeded like the update's, the KL coefficient's rule on the last minibatch's KL.
    Returns (steps, stats [steps, 5], the coefficient afterwards as a float32 tensor)."""
    dev = model.device
    n_all = rb.T * rb.rows
    obs = rb.obs.view(n_all, -1)
    live = torch.nonzero(rb.agent_mask.view(n_all)).view(-1)
    c = hp["log_std_clip"]
    with torch.no_grad():
        mean, _, ls, _ = head(model, obs, c)
        old_dist = torch.cat([mean, ls], 1)
    adv = rb.advantages.view(n_all)
    a = adv[live]
    adv = (adv - a.mean()) / max(1e-4, float(a.std(unbiased=False)))
    data = (obs, rb.actions.view(n_all, -1), rb.log_probs.view(n_all), old_dist, adv, rb.returns.view(n_all))
    klc = torch.full((1,), hp["kl_coeff"], dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    opt = adam(model, hp)
    stats = []
    for _ in range(num_epochs):
        perm = live[torch.randperm(live.numel(), device=dev, generator=gen)]
        stats.append(ref_epoch(model, opt, data, perm, minibatch_size, hp, klc))
    stats = torch.cat(stats)
    kl = float(stats[-1, 3])
    if kl > 2.0 * kl_target:
        klc = klc * 1.5
    elif kl < 0.5 * kl_target:
        klc = klc * 0.5
    return stats.shape[0], stats, klc


def check_conditions(aux, hp, clamp=False, stats=None):
    """The data conditions on ref64 alone.  No ratio within 1e-4 of a clip edge, no squared value error within a
    relative 1e-3 of vf_clip_param, no raw log_std within 1e-3 of +-c: float32 and float64 cannot disagree on a
    branch.  For minibatches of 8 rows and more: 20-80 % of the rows on the surrogate's clipped branch with both clip
    edges present, 20-80 % value-clipped.  Clamp cases: a head element in each of the three clamp regions.  With
    `stats`: all finite, and the policy loss (a mean of terms of both signs and unit scale) at least 0.05 in magnitude,
    so that its relative error measures the terms and not how closely they happen to cancel."""
    if stats is not None:
        assert torch.isfinite(stats).all() and abs(float(stats[0])) >= 0.05, stats
    r, e2, raw = aux["ratio"].cpu().numpy(), aux["e2"].cpu().numpy(), aux["raw"].cpu().numpy()
    lo, hi, vc, c = 1.0 - hp["clip_param"], 1.0 + hp["clip_param"], hp["vf_clip_param"], hp["log_std_clip"]
    assert np.abs(r - lo).min() > 1e-4 and np.abs(r - hi).min() > 1e-4
    assert np.abs(e2 / vc - 1.0).min() > 1e-3
    assert np.abs(np.abs(raw) - c).min() > 1e-3
    assert (aux["kl"] > 0).all()
    if r.size >= 8:
        frac = float(aux["clipped"].double().mean())
        assert 0.2 <= frac <= 0.8, frac
        assert (r < lo).any() and (r > hi).any()
        vfrac = float((e2 > vc).mean())
        assert 0.2 <= vfrac <= 0.8, vfrac
    if clamp:
        assert (raw > c).any() and (raw < -c).any() and (np.abs(raw) < c).any()


def param_names(model):
    names = []
    for k, seq in (("actor", model.actor_encoder), ("critic", model.critic_encoder)):
        for i, m in enumerate(x for x in seq if hasattr(x, "weight")):
            names += [f"{k}{i}.weight", f"{k}{i}.bias"]
    return names + ["pi.weight", "pi.bias", "vf.weight", "vf.bias"]


def fake_buffer(rb, dtype):
    """The fields a training iteration reads of a DeviceMarlRolloutBuffer, as copies (the floats in `dtype`)."""
    f = {k: getattr(rb, k).detach().clone().to(dtype) for k in ("obs", "actions", "log_probs", "advantages", "returns")}
    return types.SimpleNamespace(T=rb.T, rows=rb.rows, agent_mask=rb.agent_mask.clone(), **f)


def make_marl_batch(E, n, m):
    """A MARL batch whose even envs start with the drones inside level 2's approach radius, half of those n + 2
    successes short of level 3: whole envs end and single agents drop out within the first steps
    (test_gpu_marl_rollout._make's construction), so a rollout's agent_mask has zeros."""
    from cattleherd.env import HerdBatch
    b = HerdBatch(E, n, m, mode="marl", curriculum_level=2, min_drones=n, max_drones=n)
    b.reset()
    s = b.get_state()
    near = np.arange(E) % 2 == 0
    c = s["cow_pos"].mean(1)
    for k in range(n):
        s["drone_pos"][near, k, 0] = c[near, 0] + 0.5 * (k - (n - 1) / 2)
        s["drone_pos"][near, k, 1] = c[near, 1] + 0.45
    tally = s["tally"].copy()
    tally[near & (np.arange(E) % 4 == 0)] = 100 - n - 2
    b.set_state({"drone_pos": s["drone_pos"], "tally": tally})
    return b
