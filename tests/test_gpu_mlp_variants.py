"""Every instantiation of the on-device policy forward (csrc/ch_policy.hip, csrc/ch_mlp2_dev.h) against the float64
reference and the derived error bar of tests/mlp_ref.py, at the smallest shapes that reach each path: the seven k_mlp2
and three k_mlp kernels launch_mlp_multi dispatches to, the three weight-fetch modes (packed, raw float4, raw
element), the three input-row load paths (float4, float2, element), partial last tiles, row masks, missing biases,
the LDS back-off, and tanh_fast on its own.  Every case asserts the kernel it claims to reach (ch__mlp_last_launch)
and computes its row counts from the device's CU count, so a change of the dispatch thresholds fails the case
instead of moving it to another kernel.

tests/test_mlp_ref_cpu.py shows on the CPU what the bar admits and what it rejects.

Found with these cases (both fixed in launch_mlp_multi's dispatch, no kernel changed):
  * k_mlp2<4, 4, false, 2> stages a row tile's input through an 8-register ring that holds 512 columns, and was sent
    first layers of up to 896 live columns: columns past 512 of the staged rows were never written and the first layer
    multiplied stale LDS.  Before the fix, at 32 C + 17 = 8209 rows: 600-256-256-8 max error 0.125 (8208 rows
    outside the bar), 896-256-256-49 0.252 (every row); 512-256-256-8 was right (max error 2e-7).  Such
    nets now run one row tile per workgroup on k_mlp2<8, 2> (the r2w-600 and r2w-896 cases).
  * raw weights (ch_mlp.packed = NULL) with a hidden width that is no multiple of 16: the layer's last tile computes the
    clamped last weight row for the columns past the width and its epilogue writes them while other waves zero the
    same columns, unordered.  7-200-33-250-5 at 100 rows differed from the packed forward by up to 0.17.  Such nets
    now go to k_mlp (mlp_ref.RAW_KERNEL).

Worst err / bar per kernel on an MI355X (256 CUs), this module 12.9 s in all, the slowest case the three child
processes of the A/B switches at 6.7 s, every other case under 0.8 s (1.8 s for the first, which loads the library):
    k_mlp2<8,1> 0.069    k_mlp2<8,2> 0.0061    k_mlp2<4,2> 0.0088 (CH_MLP2_NW4)    k_mlp2<8,1,true> 1.2e-4 (collection)
    k_mlp2<8,1,false,2> 7.3e-4, two segments 1.5e-4 (collection)    k_mlp2<4,4,false,2> 8.4e-4
    k_mlp2<4,4,false,4> 0.0035    k_mlp<8,1,2> 0.0088    k_mlp<8,2,2> 8.5e-4    k_mlp<4,4,1> 5.3e-4 (CH_MLP_V1 CH_MLP_WIDE4)
    tanh_fast: 1.95e-7 = 0.44 TAU on both k_mlp2<8,1> and k_mlp<8,1,2>; exactly +-1 at +-44.5, +-100 and +-inf.
(+-inf and +-100 go through a net whose units all read column 0: through an identity matrix inf x 0 is NaN.)
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mlp_ref as R

pytestmark = pytest.mark.gpu

WORST = {}   # kernel -> worst err / bar seen in this run (printed at the end: the record in the docstring above)
SENTINEL = 12345.0
GUARD = 32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\nworst err / bar  {k:24s} {WORST[k]:.3g}", end="")
    print()


def _cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _offset_copy(t, off_bytes):
    """``t`` as a contiguous view ``off_bytes`` into a larger device buffer."""
    import torch
    k = off_bytes // 4
    buf = torch.zeros(t.numel() + k + 4, dtype=torch.float32, device="cuda")
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off_bytes % 16 and v.is_contiguous()
    return v


def _policy(case, layers):
    import torch
    from cattleherd.policy import DevicePolicy
    tl = [(torch.from_numpy(w).cuda(), None if b is None else torch.from_numpy(b)) for w, b in layers]
    if case.w_off:
        tl[0] = (_offset_copy(tl[0][0], 4), tl[0][1])
    pol = DevicePolicy(tl, case.act, case.clip)
    assert pol.weights[0].data_ptr() % 16 == (4 if case.w_off else 0)
    return pol


def _forward(pol, x, rows, mask=None):
    """ch_mlp_forward / ch_mlp_forward_masked straight on ``x`` (DevicePolicy.forward may re-lay the tensor out) into
    a NaN-filled buffer with GUARD sentinel rows behind it; returns (the rows, the guard rows, the launch record)."""
    import torch
    from cattleherd import _lib as L
    n = pol.dims[-1]
    full = torch.full((rows + GUARD, n), float("nan"), dtype=torch.float32, device="cuda")
    full[rows:] = SENTINEL
    pol._ensure_packed() if pol._net.packed else None
    st = pol._stream()
    vp = ctypes.c_void_p
    if mask is None:
        L.check(L.lib().ch_mlp_forward(ctypes.byref(pol._net), vp(x.data_ptr()), rows, vp(full.data_ptr()), st))
    else:
        L.check(L.lib().ch_mlp_forward_masked(ctypes.byref(pol._net), vp(x.data_ptr()), rows, vp(mask.data_ptr()),
                                              vp(full.data_ptr()), st))
    rec = L.mlp_last_launch()
    torch.cuda.synchronize()
    return full[:rows], full[rows:], rec


def check_forward(case, cus):
    """The whole procedure for one case; returns (kernel, rt, max err / bar)."""
    import torch
    rows = R.case_rows(case, cus)
    layers, x_np = R.case_data(case, cus)
    y64 = R.forward64(layers, case.act, case.clip, x_np)
    bar = R.bar(layers, case.act, case.clip, x_np)
    pol = _policy(case, layers)
    x = torch.from_numpy(x_np).cuda()
    xs = _offset_copy(x, case.x_off) if case.x_off else x
    m_np = R.case_mask(case, rows)
    mask = None if m_np is None else torch.from_numpy(m_np).cuda()

    def one(xin, msk, kernel=case.kernel):
        y, guard, rec = _forward(pol, xin, rows, msk)
        assert torch.all(guard == SENTINEL), "wrote past the last row"
        if kernel is not None:
            assert rec[0] == kernel and rec[1] == case.rt, (rec, kernel, case.rt)
            assert rec[2] == (rows + 16 * case.rt - 1) // (16 * case.rt) and rec[3] > 0, rec
        return y, rec

    y, rec = one(xs, mask)
    if case.raw:
        keep = pol._net.packed
        pol._net.packed = None                    # the raw nn.Linear weights (fetch mode 1 / 2; k_mlp reads them anyway)
        try:
            y_raw, rec_raw = one(xs, mask, R.RAW_KERNEL.get(case.id, case.kernel))
        finally:
            pol._net.packed = keep
        if rec_raw[0] == rec[0]:   # the same kernel: the same fma chains, bit for bit
            assert torch.equal(torch.nan_to_num(y_raw, nan=7.0), torch.nan_to_num(y, nan=7.0)), "raw != packed"
        else:
            raw = y_raw.double().cpu().numpy()
            keep_rows = ~np.isnan(raw).any(1)
            r_raw = np.abs(raw[keep_rows] - y64[keep_rows]) / bar[keep_rows]
            assert np.all(r_raw <= 1.0), float(r_raw.max())
            WORST[rec_raw[0]] = max(WORST.get(rec_raw[0], 0.0), float(r_raw.max()))
    if case.x_off:
        y_al, _ = one(x, mask)
        assert torch.equal(y_al, y), "offset input != aligned input"
    got = y.double().cpu().numpy()
    sel = np.ones(rows, bool) if m_np is None else m_np.astype(bool)
    assert not np.isnan(got[sel]).any(), "a computed row holds NaN"
    assert np.isnan(got[~sel]).all(), "a row the mask leaves out was written"
    ratio = np.abs(got[sel] - y64[sel]) / bar[sel]
    print(f"{case.id}: {rec} err/bar {ratio.max():.3g} (max err {np.abs(got[sel] - y64[sel]).max():.3g})")
    assert np.all(ratio <= 1.0), float(ratio.max())
    if mask is not None:   # an all-zero mask writes nothing
        y0, _ = one(xs, torch.zeros(rows, dtype=torch.uint8, device="cuda"))
        assert torch.isnan(y0).all()
    WORST[rec[0]] = max(WORST.get(rec[0], 0.0), float(ratio.max()))
    return rec[0], rec[1], float(ratio.max())


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_forward_vs_fp64(case):
    check_forward(case, _cus())


def test_rows_zero_launches_nothing():
    import torch
    from cattleherd import _lib as L
    case = R.CASES[1]
    pol = _policy(case, R.random_net(case.dims, 1))
    x = torch.zeros(16, case.dims[0], device="cuda")
    _forward(pol, x, 16)
    before = L.mlp_launch_counts()
    y, guard, rec = _forward(pol, x, 0)
    after = L.mlp_launch_counts()
    assert rec == ("none", rec[1], 0, 0) and torch.all(guard == SENTINEL)
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {"none": 1}


# ---- tanh_fast ---------------------------------------------------------------------------------------------------
def _tanh_net(k0, ones_column):
    """(k0, 16, 16) with no bias whose output is tanh_fast of the input: identity blocks (column i -> unit i), or
    (for values whose products with a zero weight are NaN) every unit reading column 0."""
    w0 = np.zeros((16, k0), np.float32)
    if ones_column:
        w0[:, 0] = 1.0
    else:
        w0[:, :16] = np.eye(16, dtype=np.float32)
    return [(w0, None), (np.eye(16, dtype=np.float32), None)]


@pytest.mark.parametrize("k0,kernel", [(16, R.K81), (1153, R.V81)])
def test_tanh_fast_sweep(k0, kernel):
    """tanh_fast (act_fn in k_mlp, the fused-bias form in k_mlp2's epilogue) against np.tanh within TAU over the sweep;
    exactly +-1 at +-100 and +-inf."""
    import torch
    v = R.tanh_sweep()
    pad = (-len(v)) % 16
    grid = np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, 16)
    x = np.zeros((grid.shape[0], k0), np.float32)
    x[:, :16] = grid
    case = R.Case("tanh", (k0, 16, 16), "tanh", x.shape[0], kernel, 1, False, None, False, False, 0, None, 0)
    pol = _policy(case, _tanh_net(k0, False))
    y, guard, rec = _forward(pol, torch.from_numpy(x).cuda(), x.shape[0])
    assert rec[0] == kernel and torch.all(guard == SENTINEL)
    got = y.double().cpu().numpy().reshape(-1)[:len(v)]
    err = np.abs(got - np.tanh(v.astype(np.float64)))
    print(f"tanh_fast on {rec[0]}: max err {err.max():.3g} = {err.max() / R.TAU:.3g} TAU")
    assert not np.isnan(got).any() and err.max() <= R.TAU, float(err.max() / R.TAU)
    WORST[f"tanh_fast / TAU, {rec[0]}"] = float(err.max() / R.TAU)
    sp = np.array([100.0, -100.0, np.inf, -np.inf, 44.5, -44.5], np.float32)
    xs = np.zeros((len(sp), k0), np.float32)
    xs[:, 0] = sp
    pol = _policy(case, _tanh_net(k0, True))
    y, guard, rec = _forward(pol, torch.from_numpy(xs).cuda(), len(sp))
    assert rec[0] == kernel
    got = y.cpu().numpy()
    assert np.array_equal(got, np.repeat(np.sign(sp)[:, None], 16, 1)), got[:, 0]


# ---- the kernels only a collection reaches ---------------------------------------------------------------------
@pytest.mark.parametrize("e_per_cu,kernel", [(0, "k_mlp2<8,1,true>"), (16, R.K81R2)])
def test_collection_forwards_vs_fp64(e_per_cu, kernel):
    """ch_rollout_collect's actor + critic launch: two segments in one grid -- k_mlp2<8, 1, true> at 64 envs, the
    two-row-tile kernel at 16 C envs (32 C rows in all).  The values it stored and the action means (log_std -20: the
    stored action is the mean to 2e-8) against forward64 of the stored observations, live width 4 x 86."""
    import torch
    from cattleherd import _lib as L
    from cattleherd.env import HerdBatch
    from cattleherd.policy import DevicePolicy
    from cattleherd.rollout import DeviceRolloutBuffer
    E, T, A = (e_per_cu * _cus() or 64), 2, 16
    b = HerdBatch(E, 4, 16, mode="ctde")
    b.reset()
    la, lc = R.random_net((1032, 128, 128, A), 71), R.random_net((1032, 128, 128, 1), 72)
    mk = lambda ls: DevicePolicy([(torch.from_numpy(w), torch.from_numpy(bb)) for w, bb in ls], "tanh", None)  # noqa: E731
    actor, critic = mk(la), mk(lc)
    rb = DeviceRolloutBuffer(b, T, act_dim=A)
    log_std = torch.full((A,), -20.0, device="cuda")
    c0 = L.mlp_launch_counts()
    rb.collect(actor, critic, log_std, seed=3, bootstrap_truncated=False)
    torch.cuda.synchronize()
    c1 = L.mlp_launch_counts()
    delta = {k: c1[k] - c0[k] for k in c1 if c1[k] != c0[k]}
    assert delta == {kernel: T, R.K81: 1}, delta   # T two-segment launches, then V(last obs) alone
    obs = rb.obs.view(T * E, -1).double().cpu().numpy()
    assert np.all(obs[:, 4 * 86:] == 0.0)
    live = np.full(T * E, 4 * 86)
    worst = 0.0
    for layers, got in ((lc, rb.values.reshape(-1, 1)), (la, rb.actions.view(T * E, A))):
        want = R.forward64(layers, "tanh", None, obs, live)
        bar = R.bar(layers, "tanh", None, obs, live) + (np.exp(-20.0) * 8.0 + R.U * np.abs(want) if layers is la else 0.0)
        ratio = np.abs(got.double().cpu().numpy() - want) / bar
        assert np.all(ratio <= 1.0), float(ratio.max())
        worst = max(worst, float(ratio.max()))
    print(f"collect E={E}: {kernel} err/bar {worst:.3g}")
    key = kernel + " (2 segments)"
    WORST[key] = max(WORST.get(key, 0.0), worst)
    b.close()


# ---- the A/B switches, read once per process ---------------------------------------------------------------------
CHILD = """
import json, sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import mlp_ref as R, test_gpu_mlp_variants as T
out = []
for i, (dims, act) in enumerate(R.SWITCH_SHAPES):
    c = R.Case("switch", dims, act, 100, None, 1, True, None, False, False, 0, None, 90 + i)
    out.append(T.check_forward(c, T._cus()))
print("RESULT " + json.dumps(out))
"""


def test_ab_switches_in_fresh_processes():
    """CH_MLP_V1, CH_MLP2_NW4 and CH_MLP_WIDE4 (with CH_MLP_V1: it chooses among the k_mlp kernels) are read once per
    process: one child each, one after the other, running three shapes at 100 rows -- this is what runs
    k_mlp2<4, 2> and k_mlp<4, 4, 1>, kept for A/B."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = CHILD.format(tests=tests, pkg=os.path.join(os.path.dirname(tests), "rl-cattle-herding_amd"))
    for switches, kernels in R.SWITCH_KERNELS:
        env = {k: v for k, v in os.environ.items() if k not in ("CH_MLP_V1", "CH_MLP2_NW4", "CH_MLP_WIDE4", "CH_MLP_RT")}
        env.update({s: "1" for s in switches})
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert [r[0] for r in res] == list(kernels), (switches, res)
        for kernel, _rt, ratio in res:
            assert ratio <= 1.0
            key = f"{kernel} ({' '.join(switches)})"
            WORST[key] = max(WORST.get(key, 0.0), ratio)
