"""The native PPO update (csrc/ch_ppo.hip: k_ppo_fb*, k_ppo_dw*, k_ppo_adam*) held to its float64 references past the
driver's sizes: minibatches of 530 and 1030 rows, hidden widths of 256, 144 and 240, heads of 64 and 1 columns, first
layers that end on, one past and four past a 256-column k-group, 673121 parameters, 261 weight-gradient workgroups.
The other PPO modules stop at 128 rows, 128-128 (SB3) and 304 k parameters; every loop below takes another pass, or
another number of passes, only above that:

  advantage mean / std, `i += 512` (ch_ppo_fb_body.inc)                       B = 530: 2 passes, 1030: 3
  rllib_log_stats' two-pass variances, `i += 256` (ch_ppo.hip)                B = 530: 3 passes
  serial tile sums (loss partials, approx_kl, clip_fraction, gate_trips,
  tile_dls, the RLlib log's sums) and dw_loop's bp / 16 passes                34 and 65 tiles against 8
  Adam's grid-stride loop and segment scan at the grid's cap                  grid 512 < 658 = ceil(n / 1024)
  the Adam launch's sum of the partials, `i += 256`                           261 partials
  a wave's second column tile (`t += 8` waves), an uneven split               16, 9 and 15 tiles
  k_ppo_dw's scalar first layer over two k-groups                             obs_dim 257; 256 and 260 (float4)
  the SB3 head's `tid < NO` at 64, the log's columns behind it; NO = 1        EDGE_A, EDGE_B
  an SB3 one-hidden-layer net (the backward loop runs once from `os`)         EDGE_A's policy, EDGE_B's, MANY_WG

References and rule: ppo_native_ref / marl_ppo_ref, unchanged -- err(native) <= 4 max(err(torch32), FLOOR) per tensor
against the float64 torch run of the same step, torch32 measured in the same test, FLOOR = 32 * 2**-24 (every sum here
has at most 1032 terms) but for MANY_WG, whose obs_dim of 1800 gives ceil(sqrt(1800)) = 43 units (shape["floor"]).
Inputs are seeded on the host; the SB3 shapes use ppo_native_ref's gapped noise, so no ratio lies within 1e-2 of a clip
edge at the starting weights and clip_fraction is an exact count there (tests/test_ppo_native_cpu.py and
test_marl_ppo_cpu.py assert the data conditions with no device).  A training-type case runs twice and must give the
same bits.  The population case is bit-compared with the solo entry through test_gpu_ppo_pop's own helpers.

Measured on an MI355X (each test prints its figures before it asserts), the largest err(native) / err(torch32) of a
group:
  SMALL_ROWS gradients   B = 530: 1.10e-6 / 9.68e-7   B = 1030: 1.15e-6 / 1.35e-6   B = 530, raw advantages: 1.10e-6 / 9.68e-7
  SMALL_ROWS statistics  B = 530: 1.40e-7 / 9.04e-8   B = 1030: 5.33e-7 / 5.33e-7   B = 530, raw advantages: 6.28e-7 / 6.92e-8
  WIDE B = 24: gradients 1.53e-6 / 2.22e-6, statistics 8.15e-6 / 3.76e-5
  MANY_WG B = 16 (floor 43 units): gradients 1.08e-6 / 1.97e-6, statistics 4.25e-5 / 2.56e-5; one ch_ppo_train step:
    statistics 4.25e-5 / 2.56e-5, parameters 3.32e-6 / 2.56e-6
  EDGE_A: gradients 1.48e-6 / 1.86e-6, statistics 6.55e-6 / 1.33e-5; EDGE_B: 1.20e-6 / 1.95e-6, 8.24e-7 / 7.56e-7;
  EDGE_C: 8.95e-7 / 7.61e-7, 1.49e-6 / 6.71e-6
  EDGE_A, one ch_ppo_train_log step: approx_kl 2.30e-6 / 2.20e-6, parameters 7.52e-7 / 1.00e-6, clip count exact
  530 + 530 + 40 rows, statistics (policy loss, value loss, entropy, approx_kl), then parameters / m / v:
    ch_ppo_train_log 5.11e-7 / 1.25e-6, 7.09e-7 / 4.23e-7;  ch_ppo_train_opt 5.11e-7 / 1.25e-6, 7.09e-7 / 4.23e-7;
    ch_ppo_train_opt + clip_range_vf 4.88e-7 / 1.78e-6, 7.07e-7 / 4.32e-7
    clip counts 373, 388 and 31 of 530, 530 and 40 rows, the float64 run's exactly in every step (no row of the
    float64 run within 1e-3 of an edge in any of them)
  value-clip gradient B = 530: gradients 9.91e-7 / 1.08e-6, statistics 1.40e-7 / 6.53e-8
  gate (float64 approx_kl 0.0172, 0.2122, threshold 0.1147; trips at the second minibatch): the two rows' statistics
    1.97e-7 / 4.32e-7, parameters / m / v after the one applied step 7.06e-7 / 4.14e-7; with clip_range_vf
    1.27e-7 / 3.33e-7, 7.15e-7 / 4.90e-7
  Adam x 3 on 673121 parameters, grid 512: max_grad_norm 0.5 params 1.58e-7 / 1.58e-7, m 1.26e-7 / 1.66e-7,
    v 2.16e-7 / 2.55e-7; max_grad_norm 1e3: 1.52e-7 / 1.67e-7, 9.06e-8 / 7.91e-8, 1.27e-7 / 1.23e-7
  RLlib SMALL_ROWS B = 530: gradients 1.17e-6 / 1.04e-6, stats5 1.97e-7 / 1.17e-7; EDGE_1 4.48e-7 / 1.13e-6,
    4.67e-7 / 3.65e-7; EDGE_32 1.32e-6 / 1.16e-6, 7.87e-7 / 6.99e-7
  RLlib 530 + 530 + 40 rows: the three log columns 5.48e-7 / 7.27e-4 (vf_explained_var, 2.3e-4 in the reference;
    vf_loss_unclipped and total_loss below 1.7e-7), stats5 2.07e-7 / 1.02e-7, parameters 1.57e-7 / 1.46e-7
Every test takes 0.01 - 0.25 s (the first one 3.6 s with the device's start-up).
"""
import ctypes

import numpy as np
import pytest

import test_gpu_ppo_pop as POP
from test_gpu_ppo_pop import pop  # noqa: F401  (the population handle's fixture)

pytestmark = pytest.mark.gpu

STATS4 = ("policy_loss", "value_loss", "entropy", "grad_norm")
SIGMA = 0.25     # clip_range_vf, and the scale of the old values' noise (test_gpu_ppo_opts.py's)
# seeds of the old values' noise, chosen on the float64 reference alone for ppo_opts_ref.vf_conditions: the three
# minibatches of the training sequence, and the single minibatch of 530 rows
VSEED_LOOP, VSEED_GRAD = 5, 5

_CACHE = {}
_WORST = {}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _case(which):
    """The shape's data (float64 and float32 on the GPU) and its starting model, made once and left unchanged."""
    import ppo_native_ref as R
    if which not in _CACHE:
        shape = getattr(R, which)
        d64 = R.make_data(shape, _dev())
        _CACHE[which] = (shape, d64, tuple(t.float().contiguous() for t in d64), R.make_model(shape, _dev()))
    return _CACHE[which]


def _accept(group, name, native, t32, ref, floor=None):
    """ppo_native_ref.accept, keeping the group's largest pair of errors for the figures line."""
    import ppo_native_ref as R
    ok = R.accept(name, native, t32, ref, R.FLOOR if floor is None else floor)
    if float(ref.abs().max()) > 0.0:
        en, et = R.err(native, ref), R.err(t32, ref)
        w = _WORST.setdefault(group, [0.0, 0.0])
        w[0], w[1] = max(w[0], en), max(w[1], et)
    return ok


def _figures(*groups):
    print("FIGURES " + "; ".join(f"{g}: {_WORST[g][0]:.2e} / {_WORST[g][1]:.2e}" for g in groups if g in _WORST))


def _hparams(hp, normalize=True, lr=None):
    from cattleherd import ppo
    return ppo.ChPpoHparams(hp["learning_rate"] if lr is None else lr, 0.9, 0.999, 1e-5, hp["clip_range"],
                            hp["ent_coef"], hp["vf_coef"], hp["max_grad_norm"], int(normalize), 0)


def _native_grad(model, data32, idx, normalize=True):
    """ch_ppo_grad: the flat gradient, the four statistics and the launches' record."""
    import torch
    import ppo_native_ref as R
    from cattleherd import _lib, ppo
    lib = ppo._bind()
    net, h = ppo.ppo_net(model), _hparams(R.HP, normalize)
    d = ppo.ChPpoData(*(t.data_ptr() for t in data32), data32[0].shape[0])
    n = lib.ch_ppo_param_count(ctypes.byref(net))
    assert n == sum(p.numel() for p in model.parameters())
    grad = torch.full((n,), float("nan"), device=model.device)
    stats = torch.full((4,), float("nan"), device=model.device)
    scratch = torch.empty(lib.ch_ppo_scratch_size(ctypes.byref(net), idx.numel()), device=model.device)
    before = [p.detach().clone() for p in model.parameters()]
    _lib.check(lib.ch_ppo_grad(ctypes.byref(net), ctypes.byref(h), ctypes.byref(d), idx.data_ptr(), idx.numel(),
                               grad.data_ptr(), stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))     # ch_ppo_grad updates nothing
    return grad, stats


def _compare_grad(which, batch, normalize=True):
    """One ch_ppo_grad of `batch` rows of the shape against ref64 / torch32: every parameter's gradient and the four
    statistics."""
    import torch
    import ppo_native_ref as R
    shape, data64, data32, m0 = _case(which)
    dev = _dev()
    idx = R.idx_for(shape, batch).to(dev)
    m32 = R.make_model(shape, dev, like=m0)
    m64 = R.make_model(shape, dev, torch.float64, like=m0)
    hp = dict(R.HP, normalize_advantage=normalize)
    g64, s64, ratio, clipped = R.ref_grad(m64, data64, idx, **hp)
    R.check_clip_conditions(ratio, clipped)
    g32, s32, _, _ = R.ref_grad(m32, data32, idx, **hp)
    flat, stats = _native_grad(m32, data32, idx, normalize)
    assert torch.isfinite(flat).all() and torch.isfinite(stats).all()
    tag = f"{which} B={batch}" + ("" if normalize else " raw adv")
    ok, floor = True, shape.get("floor")
    for name, gn, gt, gr in zip(R.param_names(m32), R.split_flat(flat, m32), g32, g64):
        assert float(gr.abs().max()) > 0.0, name
        ok &= _accept(f"grad {tag}", f"grad {tag} {name}", gn, gt, gr, floor)
    for i, name in enumerate(STATS4):
        ok &= _accept(f"stat {tag}", f"stat {tag} {name}", stats[i:i + 1], s32[i:i + 1], s64[i:i + 1], floor)
    _figures(f"grad {tag}", f"stat {tag}")
    return ok


def _dw_workgroups(shape):
    """csrc/ch_ppo.hip dw_workgroups for an SB3 net: per layer ceil(N / 16) row tiles x ceil(K / 256) k-groups, and one
    workgroup for log_std."""
    wg = 1
    for hidden, head in ((shape["pi"], shape["act_dim"]), (shape["vf"], 1)):
        dims = (shape["obs_dim"],) + tuple(hidden) + (head,)
        wg += sum(-(-dims[i + 1] // 16) * -(-dims[i] // 256) for i in range(len(dims) - 1))
    return wg


# ---- 1. large minibatch: SB3 gradient and statistics -----------------------------------------------------------------------
@pytest.mark.parametrize("batch,normalize", [(530, True), (1030, True), (530, False)],
                         ids=["530", "1030", "530_raw_advantages"])
def test_large_minibatch_gradients_match_float64_reference(batch, normalize):
    """SMALL_ROWS: 34 / 65 row tiles (2 / 6 rows in the last), the 512-thread advantage loops' second and third pass;
    once with normalize_advantage off, so that a wrong mean or scale cannot hide in either branch."""
    assert batch > 512 and batch % 16 != 0 and -(-batch // 16) > 8 and batch <= 1032
    assert _compare_grad("SMALL_ROWS", batch, normalize)


# ---- 2. large minibatch: the log and option flavours -----------------------------------------------------------------------
def _old_values(which, seed):
    """The shape's old values, ref64's own + N(0, SIGMA^2) as float32 holds them: (float64, float32) on the GPU."""
    import torch
    import ppo_native_ref as R
    shape, data64, _, m0 = _case(which)
    m64 = R.make_model(shape, _dev(), torch.float64, like=m0)
    with torch.no_grad():
        v, _, _ = m64.evaluate_actions(data64[0], data64[1])
    g = torch.Generator().manual_seed(seed)
    old = (v + SIGMA * torch.randn(shape["rows"], generator=g, dtype=torch.float64).to(_dev())).float().double()
    return old, old.float().contiguous()


def _native_train(fn, model, data32, idx, batch, opts=None, lr=None):
    """ch_ppo_train / _log / _opt over `idx` in minibatches of `batch`: (stats, m, v, step, parameters)."""
    import torch
    import ppo_native_ref as R
    from cattleherd import _lib, ppo
    lib = ppo._bind()
    dev = model.device
    net, h = ppo.ppo_net(model), _hparams(R.HP, lr=lr)
    d = ppo.ChPpoData(*(t.data_ptr() for t in data32[:5]), data32[0].shape[0])
    n = lib.ch_ppo_param_count(ctypes.byref(net))
    ea, es = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    steps = -(-idx.numel() // batch)
    ncol = {"ch_ppo_train": 4, "ch_ppo_train_log": _lib.CH_PPO_LOG_STATS, "ch_ppo_train_opt": _lib.CH_PPO_OPT_STATS}[fn]
    stats = torch.full((steps, ncol), 12345.0, device=dev)
    scratch = torch.empty(lib.ch_ppo_scratch_size(ctypes.byref(net), min(batch, idx.numel())), device=dev)
    args = [ctypes.byref(net), ctypes.byref(h), ctypes.byref(d)] + ([ctypes.byref(opts)] if fn == "ch_ppo_train_opt" else [])
    _lib.check(getattr(lib, fn)(*args, idx.data_ptr(), idx.numel(), batch, ea.data_ptr(), es.data_ptr(), step.data_ptr(),
                                stats.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    return stats, ea, es, int(step), [p.detach().clone() for p in model.parameters()]


def _same_run(a, b):
    import torch
    return (POP.same(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
            and all(torch.equal(p, q) for p, q in zip(a[4], b[4])))


def _sb3(which, data, perm, dtype, **kw):
    """ppo_opts_ref.sb3_train on a copy of the shape's starting model in `dtype`: (its record, the model)."""
    import ppo_native_ref as R
    import ppo_opts_ref as P
    shape, _, _, m0 = _case(which)
    m = R.make_model(shape, _dev(), dtype, like=m0)
    hp = R.HP
    return P.sb3_train(m, data, [perm], R.LIMIT_TRAIN_BATCH, learning_rate=hp["learning_rate"], clip_range=hp["clip_range"],
                       ent_coef=hp["ent_coef"], vf_coef=hp["vf_coef"], max_grad_norm=hp["max_grad_norm"], **kw), m


def _adam_flat(m, opt, key):
    import torch
    return torch.cat([opt.state[p][key].flatten() for p in m.parameters()])


def _accept_rows(tag, stats, out32, out64, rows):
    """Columns 0, 1, 2, 4 of the statistics rows `rows` against sb3_train's lists."""
    import torch
    ok = True
    for k in rows:
        for col, name, key, sign in ((0, "policy_loss", "pg_losses", 1.0), (1, "value_loss", "value_losses", 1.0),
                                     (2, "entropy", "entropy_losses", -1.0), (4, "approx_kl", "approx_kl_divs", 1.0)):
            f = lambda out: torch.tensor([sign * out[key][k]], dtype=torch.float64)   # noqa: E731
            ok &= _accept(f"{tag} stats", f"{tag} step {k} {name}", stats[k, col:col + 1].cpu(), f(out32), f(out64))
    return ok


def _accept_state(tag, run, m32, out32, m64, out64):
    import ppo_native_ref as R
    ok = True
    for name, pn, pt, pr in zip(R.param_names(m32), run[4], m32.parameters(), m64.parameters()):
        ok &= _accept(f"{tag} state", f"{tag} param {name}", pn, pt.detach(), pr.detach())
    for i, key in ((1, "exp_avg"), (2, "exp_avg_sq")):
        ok &= _accept(f"{tag} state", f"{tag} {key}", run[i], _adam_flat(m32, out32["opt"], key), _adam_flat(m64, out64["opt"], key))
    return ok


def _assert_clip_fractions(stats, out64, clip):
    """clip_fraction is count / B.  Where no ratio of the float64 run lies within 1e-3 of a clip edge the native count
    is the reference's exactly (the first step, by the noise's construction: asserted); a later step may differ by the
    rows an update carried inside that margin, counted on the reference alone."""
    for k, ratio in enumerate(out64["ratios"]):
        r = ratio.cpu().numpy()
        B = r.size
        near = int(((np.abs(r - (1 - clip)) <= 1e-3) | (np.abs(r - (1 + clip)) <= 1e-3)).sum())
        count64 = int((np.abs(r - 1) > clip).sum())
        got = float(stats[k, 5]) * B
        print(f"clip_fraction step {k} B={B}: native count {got:.3f}, float64 {count64}, rows within 1e-3 of an edge {near}")
        assert k > 0 or near == 0
        if near == 0:
            assert float(stats[k, 5]) == float(np.float32(count64 / B)), k
        else:
            assert abs(got - count64) <= near + 1e-3, k


@pytest.mark.parametrize("variant", ["log", "opt", "opt_vf"])
def test_large_minibatch_training_statistics_match_float64_reference(variant):
    """SMALL_ROWS's 1100 rows in minibatches of 530 (530, 530 and a partial 40) through ch_ppo_train_log (k_ppo_fb<2>),
    ch_ppo_train_opt with the gate armed at 1e6 (k_ppo_fb_opt<4>) and with clip_range_vf (k_ppo_fb_opt<5>), against
    SB3's loop restated (ppo_opts_ref.sb3_train) in float64 and float32: approx_kl, the losses, the entropy, the exact
    clip count, and the parameters and moments the three steps leave."""
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    from cattleherd import _lib
    shape, data64, data32, m0 = _case("SMALL_ROWS")
    dev = _dev()
    perm = R.limit_train_perm().to(dev)
    c = SIGMA if variant == "opt_vf" else None
    old64, old32 = _old_values("SMALL_ROWS", VSEED_LOOP)
    out64, m64 = _sb3("SMALL_ROWS", data64 + (old64,), perm, torch.float64, clip_range_vf=c)
    out32, m32 = _sb3("SMALL_ROWS", data32 + (old32,), perm, torch.float32, clip_range_vf=c)
    assert [r.numel() for r in out64["ratios"]] == [530, 530, 40] and out64["steps_applied"] == 3
    if c:   # the value clip's data conditions, on the float64 run alone
        for k, (dv, _) in enumerate(out64["clipped_rows"]):
            frac, both, margin = P.vf_conditions(dv, c)
            print(f"vf step {k}: clipped {frac:.3f}, nearest row to the bound {margin:.2e} c")
            assert 0.1 <= frac <= 0.6 and both and margin > 1e-3, k
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    fn = "ch_ppo_train_log" if variant == "log" else "ch_ppo_train_opt"
    opts = None if variant == "log" else _lib.ChPpoOpts(1e6, c or 0.0, old32.data_ptr() if c else None, stop.data_ptr())
    run = _native_train(fn, R.make_model(shape, dev, like=m0), data32, perm, 530, opts)
    again = _native_train(fn, R.make_model(shape, dev, like=m0), data32, perm, 530, opts)
    assert _same_run(run, again)                                   # fixed-order sums: the same bits
    stats = run[0]
    assert run[3] == 3 and torch.isfinite(stats).all() and int(stop) == 0
    if variant != "log":
        assert stats[:, 6].tolist() == [1.0, 1.0, 1.0]
    if variant != "opt_vf":   # columns 0-3, Adam's state and the weights are ch_ppo_train's, bit for bit
        plain = _native_train("ch_ppo_train", R.make_model(shape, dev, like=m0), data32, perm, 530)
        assert torch.equal(stats[:, :4], plain[0]) and _same_run((plain[0],) + run[1:], plain)
    tag = f"train {variant}"
    ok = _accept_rows(tag, stats, out32, out64, range(3))
    ok &= _accept_state(tag, run, m32, out32, m64, out64)
    _assert_clip_fractions(stats, out64, R.CLIP)
    _figures(f"{tag} stats", f"{tag} state")
    assert ok


def test_large_minibatch_value_clip_gradient_matches_float64_reference():
    """k_ppo_fb_opt<5> at B = 530: the value-clipped gradient and statistics of one minibatch (a ch_ppo_train_opt step
    with learning_rate 0, test_gpu_ppo_opts.py's construction and reference)."""
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    from test_gpu_ppo_opts import _native_grad_vf, _ref_grad_vf
    shape, data64, data32, m0 = _case("SMALL_ROWS")
    dev = _dev()
    old64, old32 = _old_values("SMALL_ROWS", VSEED_GRAD)
    idx = R.idx_for(shape, 530).to(dev)
    m32 = R.make_model(shape, dev, like=m0)
    m64 = R.make_model(shape, dev, torch.float64, like=m0)
    with torch.no_grad():
        v, _, _ = m64.evaluate_actions(data64[0], data64[1])
    frac, both, margin = P.vf_conditions((v - old64)[idx], SIGMA)
    print(f"vf B=530: clipped {frac:.3f}, nearest row to the bound {margin:.2e} c")
    assert 0.1 <= frac <= 0.6 and both and margin > 1e-3
    g64, s64 = _ref_grad_vf(m64, data64 + (old64,), idx, SIGMA)
    g32, s32 = _ref_grad_vf(m32, data32 + (old32,), idx, SIGMA)
    flat, stats = _native_grad_vf(m32, data32 + (old32,), idx, SIGMA)
    plain, _ = _native_grad_vf(m32, data32 + (old32,), idx, 0.0)
    assert torch.isfinite(flat).all()
    ok, names = True, R.param_names(m32)
    for name, gn, gt, gr in zip(names, R.split_flat(flat, m32), g32, g64):
        ok &= _accept("vf grad", f"vf grad B=530 {name}", gn, gt, gr)
    for i, name in enumerate(STATS4 + ("approx_kl",)):
        ok &= _accept("vf stat", f"vf stat B=530 {name}", stats[i:i + 1], s32[i:i + 1], s64[i:i + 1])
    _figures("vf grad", "vf stat")
    assert ok
    k = names.index("value_net.weight")     # a variant that ignored c would give the unclipped run's gradient
    assert not torch.equal(R.split_flat(flat, m32)[k], R.split_flat(plain, m32)[k])


@pytest.mark.parametrize("vclip", [False, True], ids=["gate", "gate_and_value_clip"])
def test_large_minibatch_gate_stops_at_the_reference_step(vclip):
    """The second minibatch's old_log_prob spiked by +-0.6 (ppo_opts_ref.spike_log_probs); 1.5 * target_kl is the
    midpoint of the float64 run's approx_kl of the first and the second step, both at least 10 % away from it.  The
    native run stops where the reference does: state column [1, 0, -1], one step counted, the stop word set, the third
    row NaN; the tripping row's statistics and the once-updated parameters under the rule."""
    import torch
    import ppo_native_ref as R
    import ppo_opts_ref as P
    from cattleherd import _lib
    shape, data64, data32, m0 = _case("SMALL_ROWS")
    dev = _dev()
    perm = R.limit_train_perm().to(dev)
    old64, old32 = _old_values("SMALL_ROWS", VSEED_LOOP)
    lp32 = data32[2].clone()
    P.spike_log_probs(lp32, perm[530:1060])
    d32 = data32[:2] + (lp32,) + data32[3:] + (old32,)
    d64 = tuple(t.double() for t in d32[:5]) + (old64,)
    c = SIGMA if vclip else None
    free, _ = _sb3("SMALL_ROWS", d64, perm, torch.float64, clip_range_vf=c)
    kl = free["approx_kl_divs"]
    thr = 0.5 * (kl[0] + kl[1])
    print(f"ref64 approx_kl {kl}, threshold {thr:.5f}")
    assert kl[0] <= 0.9 * thr and kl[1] >= 1.1 * thr                   # on ref64 alone
    target = thr / 1.5
    out64, m64 = _sb3("SMALL_ROWS", d64, perm, torch.float64, clip_range_vf=c, target_kl=target)
    out32, m32 = _sb3("SMALL_ROWS", d32, perm, torch.float32, clip_range_vf=c, target_kl=target)
    for out in (out64, out32):
        assert out["steps_applied"] == 1 and not out["continue_training"] and len(out["approx_kl_divs"]) == 2
    runs = []
    for _ in range(2):
        stop = torch.zeros(1, dtype=torch.int32, device=dev)
        opts = _lib.ChPpoOpts(target, c or 0.0, old32.data_ptr() if c else None, stop.data_ptr())
        runs.append(_native_train("ch_ppo_train_opt", R.make_model(shape, dev, like=m0), d32, perm, 530, opts))
        assert int(stop) != 0
    run = runs[0]
    assert _same_run(*runs)
    stats = run[0]
    assert stats[:, 6].tolist() == [1.0, 0.0, -1.0] and run[3] == 1
    assert torch.isfinite(stats[:2, :6]).all() and torch.isnan(stats[2, :6]).all()
    tag = "gate+vf" if vclip else "gate"
    ok = _accept_rows(tag, stats, out32, out64, range(2))
    ok &= _accept_state(tag, run, m32, out32, m64, out64)
    assert float(stats[1, 5]) > 0.9                                  # (the 530 spiked rows are outside the clip range)
    _assert_clip_fractions(stats[:1], dict(ratios=out64["ratios"][:1]), R.CLIP)
    _figures(f"{tag} stats", f"{tag} state")
    assert ok


# ---- 3. large minibatch: RLlib --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,batch,clamp", __import__("marl_ppo_ref").LIMIT_GRAD_CASES)
def test_rllib_gradients_match_float64_reference(which, batch, clamp):
    """ch_marl_ppo_grad at B = 530 (34 tile sums of the surrogate, the value error, the entropy and the KL), and at
    obs_dim 257 with a one-hidden-layer actor, a 240-144 critic and heads of 2 and 64 columns (case 6's RLlib shapes):
    every gradient and the five statistics (test_gpu_marl_ppo.py's comparison)."""
    import marl_ppo_ref as R
    from test_gpu_marl_ppo import _compare_grad as marl_compare
    ok, g64, _ = marl_compare(f"rllib {which} B={batch}", getattr(R, which), batch, clamp, R.hp_for(clamp))
    assert all(float(g.abs().max()) > 0.0 for g in g64)
    assert ok


def test_rllib_large_minibatch_log_columns_match_float64_reference():
    """ch_marl_ppo_train_log over SMALL_ROWS's 1100 rows in minibatches of 530 (530, 530, 40): three passes of
    rllib_log_stats' 256-thread variance loops, 34 tile sums.  The three log columns, the five statistics of every step
    and the parameters against the float64 and float32 runs; columns 0-4, the parameters and the moments equal
    ch_marl_ppo_train's bit for bit; a second run gives the same bits."""
    import torch
    import marl_ppo_ref as R
    import marl_train_log_ref as T
    from test_gpu_marl_ppo import STAT_NAMES, _data
    from test_gpu_marl_train_log import NEW, _native_epoch
    shape, dev = R.SMALL_ROWS, _dev()
    n_idx, batch, steps = R.LIMIT_TRAIN_CASE
    assert batch > 2 * 256 and -(-batch // 16) > 8
    hp = R.hp_for(eps=R.TRAIN_EPS)
    data64, data32 = _data(shape, False)
    perm = torch.randperm(shape["rows"], generator=torch.Generator().manual_seed(R.LIMIT_TRAIN_SEED))[:n_idx].to(dev)
    m0 = R.make_model(shape, dev)
    m32 = R.make_model(shape, dev, like=m0)
    m64 = R.make_model(shape, dev, torch.float64, like=m0)
    s32 = T.ref_epoch_log(m32, R.adam(m32, hp), data32, perm, batch, hp)
    s64 = T.ref_epoch_log(m64, R.adam(m64, hp), data64, perm, batch, hp)
    mn, mp, ma = (R.make_model(shape, dev, like=m0) for _ in range(3))
    sn, ea, es = _native_epoch(mn, data32, perm, batch, hp, True)
    sp, pa, ps = _native_epoch(mp, data32, perm, batch, hp, False)
    sa, aa, as_ = _native_epoch(ma, data32, perm, batch, hp, True)
    assert sn.shape == (steps, 8) and torch.isfinite(sn).all()
    assert torch.equal(sn[:, :5], sp) and torch.equal(ea, pa) and torch.equal(es, ps)
    assert torch.equal(sn, sa) and torch.equal(ea, aa) and torch.equal(es, as_)
    ok = True
    for pn, pq, pr2, pt, pr, p0, name in zip(mn.parameters(), mp.parameters(), ma.parameters(), m32.parameters(),
                                             m64.parameters(), m0.parameters(), R.param_names(mn)):
        assert torch.equal(pn, pq) and torch.equal(pn, pr2) and not torch.equal(pn, p0)
        ok &= _accept("rllib train params", f"rllib train param {name}", pn.detach(), pt.detach(), pr.detach())
    for k in range(steps):
        for i, name in enumerate(STAT_NAMES):
            ok &= _accept("rllib train stats5", f"rllib train step {k} {name}", sn[k, i:i + 1], s32[k, i:i + 1], s64[k, i:i + 1])
        for j, name in enumerate(NEW):
            ok &= _accept("rllib train log", f"rllib train step {k} {name}", sn[k, 5 + j:6 + j], s32[k, 5 + j:6 + j],
                          s64[k, 5 + j:6 + j])
    print(f"vf_explained_var (float64) {s64[:, 7].tolist()}")
    _figures("rllib train log", "rllib train stats5", "rllib train params")
    assert ok


# ---- 4. Adam past the grid cap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grad_norm", [0.5, 1e3])
def test_adam_past_the_grid_cap_matches_float64_reference(max_grad_norm):
    """Three ch_ppo_adam steps from three given gradients on WIDE's 673121 parameters: the grid is capped at 512
    workgroups where ceil(n / 1024) is 658, so the grid-stride loop's trip count and the segment scan leave the range
    the other tests cover.  Parameters, m, v and the step count (test_gpu_ppo_native.py's comparison)."""
    import torch
    import ppo_native_ref as R
    from cattleherd import _lib, ppo
    shape, _, _, m0 = _case("WIDE")
    dev = _dev()
    mn = R.make_model(shape, dev, like=m0)
    m32 = R.make_model(shape, dev, like=m0)
    m64 = R.make_model(shape, dev, torch.float64, like=m0)
    n = sum(p.numel() for p in mn.parameters())
    assert n == 673121 and (n + 1023) // 1024 > 512
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
        _lib.check(lib.ch_ppo_adam(ctypes.byref(net), ctypes.byref(h), gf.data_ptr(), ea.data_ptr(), es.data_ptr(),
                                   step.data_ptr(), scratch.data_ptr(), None))
    torch.cuda.synchronize()
    last = _lib.ppo_last_step()
    print(last)
    assert last[2] == "k_ppo_adam<0>" and last[4] == 512
    assert int(step) == 3
    ok, tag = True, f"adam {max_grad_norm}"
    for name, pn, pt, pr, an, sn in zip(R.param_names(mn), mn.parameters(), m32.parameters(), m64.parameters(),
                                        R.split_flat(ea, mn), R.split_flat(es, mn)):
        st32, st64 = opts[m32].state[pt], opts[m64].state[pr]
        ok &= _accept(f"{tag} params", f"{tag} param {name}", pn.detach(), pt.detach(), pr.detach())
        ok &= _accept(f"{tag} m", f"{tag} m {name}", an, st32["exp_avg"], st64["exp_avg"])
        ok &= _accept(f"{tag} v", f"{tag} v {name}", sn, st32["exp_avg_sq"], st64["exp_avg_sq"])
    _figures(f"{tag} params", f"{tag} m", f"{tag} v")
    assert ok


def test_sixteen_column_tiles_per_layer():
    """ch_ppo_grad on WIDE (hidden 256-256) at B = 24: every wave of the SB3 forward and backward takes two column
    tiles per layer."""
    import ppo_native_ref as R
    assert all(w // 16 == 16 for w in R.WIDE["pi"] + R.WIDE["vf"])
    assert _compare_grad("WIDE", 24)


# ---- 5. more than 256 weight-gradient workgroups -----------------------------------------------------------------------------
def _train_step_against_reference(which, batch, fn, tag):
    """One `fn` step over the shape's idx_for rows against T.update_reference's step in float64 / float32: the
    statistics and the parameters; twice, for the same bits."""
    import torch
    import ppo_native_ref as R
    import train_log_ref as T
    shape, data64, data32, m0 = _case(which)
    dev = _dev()
    idx = R.idx_for(shape, batch).to(dev)
    m32 = R.make_model(shape, dev, like=m0)
    m64 = R.make_model(shape, dev, torch.float64, like=m0)
    (st64, akl64, count64, ratio, clipped), = T.update_reference(m64, data64, idx, batch, R.HP)
    (st32, akl32, _, _, _), = T.update_reference(m32, data32, idx, batch, R.HP)
    R.check_clip_conditions(ratio, clipped)
    run = _native_train(fn, R.make_model(shape, dev, like=m0), data32, idx, batch)
    assert _same_run(run, _native_train(fn, R.make_model(shape, dev, like=m0), data32, idx, batch))
    stats, floor = run[0], shape.get("floor")
    assert run[3] == 1 and torch.isfinite(stats).all()
    ok = True
    for i, name in enumerate(STATS4):
        ok &= _accept(f"{tag} stats", f"{tag} {name}", stats[0, i:i + 1], st32[i:i + 1], st64[i:i + 1], floor)
    for name, pn, pt, pr, p0 in zip(R.param_names(m32), run[4], m32.parameters(), m64.parameters(), m0.parameters()):
        assert not torch.equal(pn, p0), name
        ok &= _accept(f"{tag} params", f"{tag} param {name}", pn, pt.detach(), pr.detach(), floor)
    if fn == "ch_ppo_train_log":
        ok &= _accept(f"{tag} approx_kl", f"{tag} approx_kl", stats[0, 4:5], akl32, akl64, floor)
        assert float(stats[0, 5]) == float(np.float32(count64 / batch)), (float(stats[0, 5]), count64)
    _figures(f"{tag} stats", f"{tag} approx_kl", f"{tag} params")
    return ok


def test_more_than_256_weight_gradient_workgroups():
    """MANY_WG (1800-(256,)/(256,)-48, dense): 261 workgroups of k_ppo_dw, so the 256 threads that sum their
    sum-of-squares partials take a second pass.  The gradient-norm statistic of a ch_ppo_grad and the clipped update
    of one ch_ppo_train step are what a wrong partial sum would move."""
    import ppo_native_ref as R
    assert _dw_workgroups(R.MANY_WG) == 261 > 256
    assert R.MANY_WG["floor"] == int(np.ceil(np.sqrt(R.MANY_WG["obs_dim"]))) * 2.0 ** -24
    ok = _compare_grad("MANY_WG", 16)
    ok &= _train_step_against_reference("MANY_WG", 16, "ch_ppo_train", "MANY_WG train")
    assert ok


# ---- 6. shape edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["EDGE_A", "EDGE_B", "EDGE_C"])
def test_shape_edges_match_float64_reference(which):
    """obs_dim 257 / 256 / 260 (dense), heads of 64, 1 and 5 columns, hidden widths of 16, 144 and 240, an SB3
    one-hidden-layer net in each shape."""
    import ppo_native_ref as R
    shape = getattr(R, which)
    assert shape["obs_dim"] > 256 or shape["obs_dim"] % 256 == 0
    assert min(len(shape["pi"]), len(shape["vf"])) == 1 and shape["live"] == shape["obs_dim"]
    assert _compare_grad(which, 24)


def test_log_columns_behind_the_widest_head():
    """EDGE_A's head is 64 wide, the widest: the log flavour's per-row diagnostics sit in the two columns right behind
    it.  One ch_ppo_train_log step: approx_kl, the exact clip count, the statistics and the parameters."""
    import ppo_native_ref as R
    assert R.EDGE_A["act_dim"] == 64
    assert _train_step_against_reference("EDGE_A", 24, "ch_ppo_train_log", "EDGE_A log")


# ---- 7. population at a large minibatch --------------------------------------------------------------------------------------
def test_population_at_a_large_minibatch_equals_solo(pop, monkeypatch):   # noqa: F811
    """ch_ppo_train_pop with P = 2 on case 1's net, 1100 rows in minibatches of 530 (530, 530, 40), two epochs; member
    1's second minibatch is spiked and trips its gate, member 0 carries on.  Bit-identical to ch_ppo_train_opt per
    member (test_gpu_ppo_pop.py's members and comparison, at these sizes)."""
    import torch
    import ppo_native_ref as R
    for k, v in (("ROWS", 1100), ("BATCH", 530), ("NB", 3)):
        monkeypatch.setattr(POP, k, v)
    shape = dict(obs_dim=R.SMALL_ROWS["obs_dim"], act_dim=R.SMALL_ROWS["act_dim"], pi=R.SMALL_ROWS["pi"], vf=R.SMALL_ROWS["vf"])
    members = POP.make(shape, 2, target_kl=1e6)
    rows = members[1].perms[0][530:1060]
    sign = torch.ones(530, device=rows.device)
    sign[1::2] = -1.0
    members[1].old_lp[rows] += 0.6 * sign
    free = [m.clone().solo() for m in members]                    # armed, never trips
    kls = free[1].stats[:, 4].cpu().numpy()
    T = float(kls[1]) / 1.2
    assert kls[0] < 0.9 * T and kls[1] > 1.1 * T and all(int(f.stop) == 0 and int(f.step) == 6 for f in free)
    members[1].target_kl = T / 1.5
    members[0].target_kl = 10.0 * float(free[0].stats[:, 4].max()) / 1.5
    want = [m.clone().solo() for m in members]
    assert list(want[1].stats[:, 6].cpu()) == [1, 0, -1, -1, -1, -1] and int(want[1].step) == 1 and int(want[1].stop) != 0
    assert list(want[0].stats[:, 6].cpu()) == [1] * 6 and int(want[0].step) == 6 and int(want[0].stop) == 0
    POP.run_pop(pop, members)
    POP.assert_equal_members(members, want)
    again = POP.make(shape, 2, target_kl=1e6)
    again[1].old_lp[rows] += 0.6 * sign
    again[0].target_kl, again[1].target_kl = members[0].target_kl, members[1].target_kl
    POP.run_pop(pop, again)
    POP.assert_equal_members(again, members)
