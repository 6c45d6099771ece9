"""Shared pieces of the native PPO update's tests (test_gpu_ppo_native.py, test_ppo_native_cpu.py): seeded synthetic
minibatch data, the float64 reference (the project's own evaluate_actions + PPOUpdate._loss + clip_grad_norm_ + Adam on
float64 copies), and the error measure err(x) = max|x - ref64| / max|ref64| with its acceptance rule
err(native) <= 4 * max(err(torch32), 32 * 2**-24).

Shapes.  DRIVER, SMALL, DENSE and DRIVER_DENSE are the driver's sizes (minibatches of 1 .. 64 rows, nets up to 128-128).
The shapes of LIMIT_CASES (test_gpu_ppo_limits.py) go where the kernels' loops change behaviour above those sizes:
  SMALL_ROWS  SMALL's net over 1100 rows: minibatches of 530 and 1030 rows (34 and 65 row tiles, a ragged last one; two
              and three passes of the 512-thread advantage loops), and 1100 rows in minibatches of 530 (530, 530, 40)
  WIDE        1032-(256,256)/(256,256)-48: 16 column tiles per layer (two per wave) and 673121 parameters, above the
              Adam grid's cap of 512 workgroups x 1024 elements
  MANY_WG     1800-(256,)/(256,)-48, dense: 261 weight-gradient workgroups, so the Adam launch's partial sum takes a
              second pass of its 256 threads.  Its longest sum has 1800 terms: floor ceil(sqrt(1800)) = 43 units
  EDGE_A/B/C  dense, one hidden layer in one of the nets: obs_dim 257 (scalar first layer, one column into a second
              256-column k-group), 256 (ends on a k-group) and 260 (float4, four columns past one); heads of 64, 1 and
              5; hidden widths of 144 and 240 (9 and 15 column tiles over 8 waves)

Gapped noise (shape["gapped"], these shapes only).  check_clip_conditions asks that no ratio lies within 1e-3 of
1 +- CLIP.  Under make_data's N(0, 0.15^2) noise a row falls in one of those two windows with probability
(2e-3 / 1.1) phi(0.0953 / 0.15) / 0.15 + (2e-3 / 0.9) phi(0.1054 / 0.15) / 0.15 = 0.0086 (phi the standard normal
density), so a minibatch of 530 rows expects 4.5 such rows and one of 1030 rows 8.8: no index seed satisfies the
condition there (the driver's 64 rows expect 0.55, which a seed does).  The opt-in noise
keeps clear of the edges by construction: |noise| uniform on [0.02, 0.085] u [0.12, 0.30] with a random sign, the edges
being 0.0953 and 0.1054 in log space.  At the starting weights ref64's log-ratio is minus the noise up to the float32
rounding of old_log_prob, so every ratio is more than 1e-2 from an edge, 73 % of the rows lie outside the clip range
(clip_fraction) and about half of those, by the advantage's sign, take the clipped branch."""
import types

import numpy as np
import torch

FLOOR = 32 * 2.0 ** -24   # sqrt(1032) units of f32 roundoff: the random-walk error of the longest sum
FACTOR = 4.0              # ordering noise of two legitimate f32 evaluations
CLIP = 0.1

# (obs_dim, pi, vf, act_dim, buffer rows, live features per row, data seed)
DRIVER = dict(obs_dim=1032, pi=(128, 128), vf=(128, 128), act_dim=48, rows=96, live=4 * 86, seed=3,
              idx_seed={64: 5, 40: 1, 8: 1, 1: 1})
SMALL = dict(obs_dim=172, pi=(64, 32), vf=(32, 64), act_dim=8, rows=200, live=86, seed=4, idx_seed={24: 2})
# dense observations (no zero tail) whose width leaves a partial last pass of the first layer's K loop (obs_dim % 64 in
# 1..12), and an action width one past a whole pass of the backward loop (33): every lane's last loads are masked
DENSE = dict(obs_dim=72, pi=(32, 16), vf=(16, 32), act_dim=33, rows=64, live=72, seed=6, idx_seed={24: 1})
DRIVER_DENSE = dict(obs_dim=1032, pi=(128, 128), vf=(128, 128), act_dim=48, rows=64, live=1032, seed=7,
                    idx_seed={40: 2})
# beyond the driver's sizes (the module docstring): gapped noise, and a tolerance floor of its own where the longest sum
# has more than 1032 terms
SMALL_ROWS = dict(SMALL, rows=1100, seed=14, gapped=True, idx_seed={530: 1, 1030: 1})
WIDE = dict(obs_dim=1032, pi=(256, 256), vf=(256, 256), act_dim=48, rows=32, live=4 * 86, seed=15, gapped=True,
            idx_seed={24: 1})
MANY_WG = dict(obs_dim=1800, pi=(256,), vf=(256,), act_dim=48, rows=24, live=1800, seed=16, gapped=True,
               idx_seed={16: 2}, floor=43 * 2.0 ** -24)
EDGE_A = dict(obs_dim=257, pi=(16,), vf=(240, 144), act_dim=64, rows=32, live=257, seed=17, gapped=True, idx_seed={24: 1})
EDGE_B = dict(obs_dim=256, pi=(144,), vf=(16, 16), act_dim=1, rows=32, live=256, seed=18, gapped=True, idx_seed={24: 1})
EDGE_C = dict(obs_dim=260, pi=(32, 240), vf=(64,), act_dim=5, rows=32, live=260, seed=19, gapped=True, idx_seed={24: 1})
# every (shape, batch) of test_gpu_ppo_limits.py's single gradients
LIMIT_CASES = [("SMALL_ROWS", 530), ("SMALL_ROWS", 1030), ("WIDE", 24), ("MANY_WG", 16), ("EDGE_A", 24), ("EDGE_B", 24),
               ("EDGE_C", 24)]
# SMALL_ROWS's training sequence: its 1100 rows in this seeded order, in minibatches of 530 (530, 530 and a partial 40)
LIMIT_TRAIN_SEED, LIMIT_TRAIN_BATCH = 31, 530


HP = dict(learning_rate=3e-4, clip_range=CLIP, ent_coef=0.1, vf_coef=0.7, max_grad_norm=0.5)   # the driver's


def idx_for(shape, batch):
    """`batch` distinct rows of the buffer in a seeded order: non-contiguous, the last buffer row always among them.
    The seeds (shape["idx_seed"]) were chosen so that the float64 reference meets check_clip_conditions."""
    g = torch.Generator().manual_seed(shape["idx_seed"][batch])
    perm = torch.randperm(shape["rows"] - 1, generator=g)[:batch]
    perm[batch // 2] = shape["rows"] - 1
    return perm


def make_model(shape, device, dtype=torch.float32, like=None):
    """An SB3ActorCritic of `shape` (seeded init, the same on every device); `like`: copy another model's parameters."""
    from cattleherd.ppo import SB3ActorCritic
    m = SB3ActorCritic(obs_dim=shape["obs_dim"], act_dim=shape["act_dim"], pi=shape["pi"], vf=shape["vf"],
                       device=device, seed=0)
    if dtype == torch.float64:
        m.modules.double()
        m.log_std.data = m.log_std.data.double()
    if like is not None:
        with torch.no_grad():
            for p, q in zip(m.parameters(), like.parameters()):
                p.copy_(q.to(p.dtype))
    return m


def make_data(shape, device):
    """Float64 host data shaped like a CTDE rollout: obs rows with `live` features then a zero tail, actions drawn
    from the model's own Gaussian, old_log_prob = the model's log-probability + N(0, 0.15^2) (shape["gapped"]: +
    gapped_noise), advantages and returns of both signs.  Returns the five flat tensors in float64 on `device`."""
    g = torch.Generator().manual_seed(shape["seed"])
    R, D, A = shape["rows"], shape["obs_dim"], shape["act_dim"]
    obs = torch.zeros(R, D, dtype=torch.float64)
    obs[:, :shape["live"]] = 0.5 * torch.randn(R, shape["live"], generator=g, dtype=torch.float64)
    m64 = make_model(shape, "cpu", torch.float64)
    with torch.no_grad():
        mean = m64.action_net(m64.policy_net(obs))
        act = mean + torch.exp(m64.log_std) * torch.randn(R, A, generator=g, dtype=torch.float64)
        act = act.float().double()   # (what a float32 buffer holds)
        obs = obs.float().double()
        _, lp, _ = m64.evaluate_actions(obs, act)
    noise = gapped_noise(R, g) if shape.get("gapped") else 0.15 * torch.randn(R, generator=g, dtype=torch.float64)
    old = (lp + noise).float().double()
    adv = torch.randn(R, generator=g, dtype=torch.float64).float().double()
    ret = torch.randn(R, generator=g, dtype=torch.float64).float().double()
    return tuple(t.to(device) for t in (obs, act, old, adv, ret))


def gapped_noise(R, g):
    """|noise| uniform on [0.02, 0.085] u [0.12, 0.30], the sign random: no exp(-noise) within 1e-2 of 1 +- CLIP (the
    edges are 0.0953 and 0.1054 in log space), rows on both sides of both edges."""
    u = torch.rand(R, 2, generator=g, dtype=torch.float64)
    x = u[:, 0] * (0.065 + 0.18)
    mag = torch.where(x < 0.065, 0.02 + x, 0.12 + (x - 0.065))
    return mag * torch.where(u[:, 1] < 0.5, -1.0, 1.0)


def limit_train_perm(shape=None):
    shape = shape or SMALL_ROWS
    return torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(LIMIT_TRAIN_SEED))


def updater(model, **kw):
    from cattleherd.ppo import PPOUpdate
    return PPOUpdate(model, graph=False, backend="torch", **kw)


def ref_grad(model, data, idx, **kw):
    """Gradient (list per parameter), [policy loss, value loss, mean entropy, gradient norm] and the ratios of one
    minibatch through the project's own _loss, in the model's dtype."""
    upd = updater(model, **kw)
    obs, act, old, adv, ret = (t.index_select(0, idx) for t in data)
    for p in model.parameters():
        p.grad = None
    loss = upd._loss(obs, act, old, adv, ret)
    loss.backward()
    grads = [p.grad.detach().clone() for p in model.parameters()]
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    with torch.no_grad():
        values, lp, ent = model.evaluate_actions(obs, act)
        a = adv
        if upd.normalize_advantage and a.shape[0] > 1:
            a = (a - a.mean()) / (a.std() + 1e-8)
        ratio = torch.exp(lp - old)
        s1, s2 = a * ratio, a * torch.clamp(ratio, 1 - upd.clip_range, 1 + upd.clip_range)
        pl = -torch.min(s1, s2).mean()
        vl = torch.nn.functional.mse_loss(ret, values)
        stats = torch.stack([pl, vl, ent.mean(), norm])
        clipped = s2 < s1
    return grads, stats, ratio, clipped


def check_clip_conditions(ratio, clipped):
    """The data conditions, on ref64 alone: 20-80 % of the rows on the clipped branch, both clip edges present, no
    ratio within 1e-3 of an edge (a one-row minibatch can only be 0 % or 100 %: the first two are asked of minibatches
    of 8 rows and more)."""
    r = ratio.cpu().numpy()
    assert np.abs(r - (1 - CLIP)).min() > 1e-3 and np.abs(r - (1 + CLIP)).min() > 1e-3
    if r.size >= 8:
        frac = float(clipped.double().mean())
        assert 0.2 <= frac <= 0.8, frac
        assert (r < 1 - CLIP).any() and (r > 1 + CLIP).any()


def err(x, ref):
    ref = ref.double()
    return float((x.double() - ref).abs().max() / ref.abs().max())


def accept(name, native, t32, ref, floor=FLOOR):
    """Print the two errors, then hold the native one to the rule.  A tensor that is exactly zero in the reference
    (the gradient of a branch whose loss terms are switched off) has no scale: the native one must be zero too.
    `floor`: FLOOR's derivation for a shape whose longest sum has more than 1032 terms (shape["floor"])."""
    if float(ref.abs().max()) == 0.0:
        print(f"{name}: reference is exactly 0, native max {float(native.abs().max()):.3e}")
        return float(native.abs().max()) == 0.0
    en, et = err(native, ref), err(t32, ref)
    bound = FACTOR * max(et, floor)
    print(f"{name}: err(native) {en:.3e}  err(torch32) {et:.3e}  bound {bound:.3e}")
    return en <= bound


def param_names(model):
    names = []
    for k, seq in (("pi", model.policy_net), ("vf", model.value_net_mlp)):
        for i, m in enumerate(x for x in seq if hasattr(x, "weight")):
            names += [f"{k}{i}.weight", f"{k}{i}.bias"]
    return names + ["action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias", "log_std"]


def split_flat(flat, model):
    out, o = [], 0
    for p in model.parameters():
        out.append(flat[o:o + p.numel()].view_as(p))
        o += p.numel()
    assert o == flat.numel()
    return out


def fake_buffer(rb, dtype):
    """The fields PPOUpdate.train reads of a DeviceRolloutBuffer, as copies in `dtype`."""
    return types.SimpleNamespace(T=rb.T, batch=types.SimpleNamespace(n_envs=rb.batch.n_envs),
                                 **{k: getattr(rb, k).detach().clone().to(dtype)
                                    for k in ("obs", "actions", "log_probs", "advantages", "returns")})

