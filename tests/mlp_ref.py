"""The float64 reference of the on-device MLP forward (csrc/ch_policy.hip, csrc/ch_mlp2_dev.h), the error bar the
GPU tests hold the kernels to (tests/test_gpu_mlp_variants.py), and the case matrix both they and the CPU checks of
the bar (tests/test_mlp_ref_cpu.py) run.

The bar is derived here from the reference and the number formats, never from what a kernel gives.

One layer.  The kernels form each pre-activation as an f32 fma chain over the K live input terms (MFMA 16x16x4 f32,
zero columns add +0 exactly) and then add the bias.  With u = 2^-24 the chain's error is at most K u sum|w h| in any
order, the bias add one more rounding of |acc| + |b|: (K + 1) u (|W||h| + |b|).  k_mlp2's tanh epilogue instead folds
the bias into the exponent's fma, s = fma(acc, c, fl(b c)) with c = fl(2 log2 e): against c_exact (acc + b) that is
two roundings on acc (c, the fma) and three on b -- (K + 2) u |W||h| + 3 u |b|, inside (K + 2) u (|W||h| + |b|) for
every K >= 1.  An incoming per-element bound e on the activations adds |W| e.  So

    err_pre <= (K + 2) u (|W||h| + |b|) + |W| e            (h: the float64 activations, K: the live terms)

That bound holds for any order of the sum, and at K ~ 1000 a float32 forward uses 1e-5 of it: it would admit a
forward that lost an input column.  Both kernels add in pairs of 32 columns in increasing order (k_mlp2: pair p, then
its 8 MFMAs of 4 columns; k_mlp: chunks of 64 = two pairs, 16 MFMAs in column order), and a rounding is relative to
the partial sum it rounds, not to sum|w h|.  Inside pair p every partial sum is at most |S_p| + T_p in magnitude
(S_p: the exact sum before the pair, T_p: the pair's sum|w h|), and the pair rounds at most 32 times whatever the
order inside it and inside an MFMA.  With the three epilogue roundings above,

    err_pre <= 32 u (sum_p |S_p| + |W||h|) + 3 u (|W||h| + |b|) + |W| e

The bar takes the smaller of the two per output; it is never wider than the first.

relu, none and the output clip are 1-Lipschitz and exact: they pass the bound through.  tanh is 1-Lipschitz and adds
u (the rounding of a correctly rounded float32 tanh, which is what a float32 reference forward commits) + TAU.

TAU, the absolute error of tanh_fast(v) = 1 - 2 rcp(exp2(s) + 1), s = c v, against tanh(v).  The hardware exp2 and
reciprocal (v_exp_f32, v_rcp_f32) are documented to 1 ulp, i.e. a relative error of at most 2^-23 = 2 u each.

  * s.  act_fn's s = fl(v fl(c)) carries two relative roundings of u; the fused form's are counted above, so this
    term covers both forms.  A relative error d of s moves tanh by |v| d (1 - tanh^2 v) <= 0.448 d (the maximum of
    v sech^2 v, at v = 0.7717): 0.9 u.
  * E = exp2(s) (1 + e1), |e1| <= 2 u;  D = fl(E + 1) = (E + 1)(1 + d1), |d1| <= u;  R = rcp(D)(1 + e2), |e2| <= 2 u.
    With p = 1 / (E + 1) in (0, 1], R = p (1 + r), |r| <= 2 u (1 - p) + u + 2 u, so 2 R is off by at most
    2 p u (5 - 2 p) <= 6 u.
  * the final fma 1 - 2 R rounds once: the result is in [-1, 1], so at most half an ulp of [0.5, 1) = u / 2.

TAU = (0.9 + 6 + 0.5) u = 7.4 u = 4.4e-7.  (Overflow and underflow are exact: exp2 -> inf gives rcp = 0 and 1;
exp2 -> 0 gives rcp(1) = 1 and -1.  The first-order bounds above neglect terms of order K u^2.)
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
TAU = 7.4 * U
TANH_SCALE = np.float32(2.8853900817779268)   # ch_mlp2_dev.h kTanhScale


def random_net(dims, seed, bias=True):
    """DevicePolicy.random_layers (nn.Linear's default initialisation) as float32 numpy (weight [out, in], bias)."""
    from cattleherd.policy import DevicePolicy
    return [(w.numpy().copy(), b.numpy().copy() if bias else None) for w, b in DevicePolicy.random_layers(list(dims), seed)]


def random_input(rows, k, seed):
    """0.3 randn, float32, no zero in it (a dropped column must change the output)."""
    import torch
    x = (torch.randn(rows, k, generator=torch.Generator().manual_seed(seed)) * 0.3).numpy()
    x[x == 0.0] = 0.3
    return x


def _live_mask(x, live):
    if live is None:
        return x
    return np.where(np.arange(x.shape[1])[None, :] < np.asarray(live).reshape(-1, 1), x, 0.0)


def _act(h, act):
    return np.tanh(h) if act == "tanh" else (np.maximum(h, 0.0) if act == "relu" else h)


def forward64(layers, act, clip, x, live=None):
    """The plain float64 forward; ``live`` [rows]: the input columns at and past a row's live width count as zero."""
    h = _live_mask(np.asarray(x, np.float64), live)
    for i, (w, b) in enumerate(layers):
        h = h @ np.asarray(w, np.float64).T
        if b is not None:
            h = h + np.asarray(b, np.float64)
        if i < len(layers) - 1:
            h = _act(h, act)
    if clip is not None:
        h = np.clip(h, clip[0], clip[1])
    return h


def forward32(layers, act, clip, x, live=None):
    """The same forward in float32 with a correctly rounded tanh: what the bar must admit."""
    h = _live_mask(np.asarray(x, np.float32), live).astype(np.float32)
    for i, (w, b) in enumerate(layers):
        h = h @ np.asarray(w, np.float32).T
        if b is not None:
            h = h + np.asarray(b, np.float32)
        if i < len(layers) - 1:
            h = np.tanh(h.astype(np.float64)).astype(np.float32) if act == "tanh" else _act(h, act)
    if clip is not None:
        h = np.clip(h, np.float32(clip[0]), np.float32(clip[1]))
    return h


def bar(layers, act, clip, x, live=None, paired=True):
    """The per-output bound on |device - forward64| derived in the module docstring, propagated layer by layer
    (``paired=False``: the order-free term alone)."""
    h = _live_mask(np.asarray(x, np.float64), live)
    k = np.full((h.shape[0], 1), h.shape[1], np.float64) if live is None else \
        np.minimum(np.asarray(live, np.float64).reshape(-1, 1), h.shape[1])
    e = np.zeros_like(h)
    for i, (w, b) in enumerate(layers):
        w64 = np.asarray(w, np.float64)
        mag = np.abs(h) @ np.abs(w64).T
        pre = h @ w64.T
        if b is not None:
            mag = mag + np.abs(np.asarray(b, np.float64))
            pre = pre + np.asarray(b, np.float64)
        flat = (np.maximum(k, 1.0) + 2.0) * U * mag
        # the pair-ordered bound: |S_p| summed over the pairs (the exact partial sum before each pair of 32 columns)
        part, before = np.zeros_like(pre), np.zeros_like(pre)
        for p in range(0, h.shape[1], 32):
            before += np.abs(part)
            part += h[:, p:p + 32] @ w64[:, p:p + 32].T
        absb = 0.0 if b is None else np.abs(np.asarray(b, np.float64))
        pair_term = 32.0 * U * ((mag - absb) + before) + 3.0 * U * mag
        e = (np.minimum(flat, pair_term) if paired else flat) + e @ np.abs(w64).T
        if i < len(layers) - 1:
            h = _act(pre, act)
            if act == "tanh":
                e = e + U + TAU
            k = np.full((h.shape[0], 1), h.shape[1], np.float64)
    return e


def tanh_fast_model(v, d_exp=0, d_rcp=0):
    """tanh_fast in float32 numpy: s = fl(v c), exp2 and the reciprocal correctly rounded and then moved d_exp /
    d_rcp ulps (their documented 1-ulp error), fl(e + 1), and the final fma rounded once."""
    def ulps(a, d):
        for _ in range(abs(d)):
            a = np.nextafter(a, np.float32(np.inf if d > 0 else -np.inf), dtype=np.float32)
        return a
    with np.errstate(over="ignore", divide="ignore", under="ignore"):
        s = (np.asarray(v, np.float32) * TANH_SCALE).astype(np.float32)
        e = ulps(np.exp2(s.astype(np.float64)).astype(np.float32), d_exp)
        e = np.where(np.isfinite(e), np.maximum(e, np.float32(0.0)), e).astype(np.float32)
        d = (e + np.float32(1.0)).astype(np.float32)
        r = ulps((1.0 / d.astype(np.float64)).astype(np.float32), d_rcp)
        r = np.where(np.isinf(d), np.float32(0.0), r)
        return (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)   # (2 r and 1 - 2 r are exact in float64)


def tanh_sweep():
    """The inputs tanh_fast is swept over: +-0, the smallest normal and a denormal, 4096 log-spaced magnitudes in
    [1e-6, 50] with both signs, +-44.5 and +-100 (float32; +-inf is checked beside them, not through a matrix)."""
    mags = np.concatenate([[0.0, 2.0 ** -126, 2.0 ** -140], np.geomspace(1e-6, 50.0, 4096), [44.5, 100.0]])
    return np.concatenate([mags, -mags]).astype(np.float32)


# ---- the case matrix ---------------------------------------------------------------------------------------------
# rows: an int, or (a, b) for a C + b with C the device's CU count (the dispatch thresholds are 32 C and 64 C rows).
# kernel / rt: what launch_mlp_multi must report.  raw: ch_mlp.packed = NULL (the fetch modes 1 and 2; the result
# must also equal the packed one bit for bit).  w_off: the first weight is a view 4 bytes into a larger buffer (fetch
# mode 2 on a mode-1 shape).  x_off: the input is a contiguous view that many bytes into a larger buffer (4: the
# element path, 8: float2; the result must equal the aligned one).  mask: "sparse" ~2 % of the rows and the last one.
Case = namedtuple("Case", "id dims act rows kernel rt bias clip raw w_off x_off mask seed")


def _c(id, dims, act, rows, kernel, rt=1, bias=True, clip=None, raw=False, w_off=False, x_off=0, mask=None, seed=0):
    return Case(id, tuple(dims), act, rows, kernel, rt, bias, clip, raw, w_off, x_off, mask, seed)


K81, K82, K81R2, K44R2, K44R4 = "k_mlp2<8,1>", "k_mlp2<8,2>", "k_mlp2<8,1,false,2>", "k_mlp2<4,4,false,2>", "k_mlp2<4,4,false,4>"
V81, V82 = "k_mlp<8,1,2>", "k_mlp<8,2,2>"
R2, R4 = (32, 17), (64, 33)   # a partial last tile inside [32 C, 64 C) and past 64 C

CASES = [
    # k_mlp2<8, 1>: narrow nets, one row tile, packed
    _c("n-1x1", (1, 1), "none", 1, K81),
    _c("n-3-15-16", (3, 15, 16), "tanh", 15, K81),
    _c("n-4-16-17-1", (4, 16, 17, 1), "relu", 16, K81),
    _c("n-7-17-127-128-15", (7, 17, 127, 128, 15), "tanh", 17, K81),
    _c("n-8-128-128", (8, 128, 128), "none", 100, K81),
    _c("n-31-127-16-nobias", (31, 127, 16), "tanh", 1, K81, bias=False),
    _c("n-33-1-17", (33, 1, 17), "tanh", 15, K81),
    _c("n-86-128-128-8-clip", (86, 128, 128, 8), "tanh", 17, K81, clip=(-0.1, 0.1)),
    _c("n-129-16-128-16-1", (129, 16, 128, 16, 1), "relu", 100, K81),
    _c("n-1152-128-128-48", (1152, 128, 128, 48), "tanh", 16, K81),
    # k_mlp2<8, 2>: wide nets, one row tile, packed and raw
    _c("w-86-129-8", (86, 129, 8), "tanh", 1, K82),
    _c("w-50-255-256-3", (50, 255, 256, 3), "relu", 15, K82),
    _c("w-33-129-255-256-17", (33, 129, 255, 256, 17), "tanh", 100, K82),
    _c("w-64-256-8-raw1", (64, 256, 8), "tanh", 16, K82, raw=True),
    _c("w-86-256-256-8-raw2", (86, 256, 256, 8), "tanh", 17, K82, raw=True),
    _c("w-7-200-33-250-5-raw2", (7, 200, 33, 250, 5), "none", 100, K82, raw=True),
    _c("w-64-256-8-raw2-woff", (64, 256, 8), "tanh", 17, K82, raw=True, w_off=True),
    # raw weights on the narrow kernel
    _c("n-1032-128-128-48-raw1", (1032, 128, 128, 48), "tanh", 100, K81, raw=True),
    _c("n-50-16-3-raw2", (50, 16, 3), "relu", 17, K81, raw=True),
    _c("n-1032-128-128-48-raw2-woff", (1032, 128, 128, 48), "tanh", 15, K81, raw=True, w_off=True),
    # input-row load paths: 4 bytes off (element loads), 8 bytes off (float2), packed and raw weights
    _c("x4-1032-128-128-48", (1032, 128, 128, 48), "tanh", 17, K81, x_off=4),
    _c("x8-1032-128-128-48", (1032, 128, 128, 48), "tanh", 17, K81, x_off=8),
    _c("x4-86-256-256-8", (86, 256, 256, 8), "tanh", 100, K82, x_off=4),
    _c("x4-64-256-8-raw", (64, 256, 8), "relu", 17, K82, raw=True, x_off=4),
    _c("x8-64-256-8-raw", (64, 256, 8), "relu", 17, K82, raw=True, x_off=8),
    # k_mlp2<8, 1, false, 2>: narrow nets, two row tiles
    _c("r2n-344-128-128-16@32C", (344, 128, 128, 16), "tanh", (32, 0), K81R2, 2),
    _c("r2n-344-128-128-16@32C+1", (344, 128, 128, 16), "tanh", (32, 1), K81R2, 2),
    _c("r2n-344-128-128-16@32C+17", (344, 128, 128, 16), "tanh", R2, K81R2, 2),
    _c("r2n-344-128-128-16@32C+17-mask", (344, 128, 128, 16), "tanh", R2, K81R2, 2, mask="sparse"),
    # k_mlp2<4, 4, false, 2>: wide nets, two row tiles (first layers up to 512 live columns)
    _c("r2w-86-256-256-8", (86, 256, 256, 8), "tanh", R2, K44R2, 2),
    _c("r2w-512-256-256-8-nobias", (512, 256, 256, 8), "tanh", R2, K44R2, 2, bias=False),
    # ... and past 512 columns, which that kernel's staging ring does not hold: one row tile, <8, 2>
    _c("r2w-600-256-256-8", (600, 256, 256, 8), "tanh", R2, K82, 1),
    _c("r2w-896-256-256-49", (896, 256, 256, 49), "tanh", R2, K82, 1),
    # k_mlp2<4, 4, false, 4>: wide nets, four row tiles; a single-tile output layer is row-split (mlp2_plan_out)
    _c("r4w-86-256-256-8", (86, 256, 256, 8), "tanh", R4, K44R4, 4),
    _c("r4w-256-256-1", (256, 256, 1), "relu", R4, K44R4, 4),
    _c("r4w-86-256-256-49", (86, 256, 256, 49), "tanh", R4, K44R4, 4),
    _c("r4w-86-129-255-256-8", (86, 129, 255, 256, 8), "relu", R4, K44R4, 4),
    _c("r4w-86-256-256-8-mask", (86, 256, 256, 8), "tanh", R4, K44R4, 4, mask="sparse"),
    # the LDS back-off: row counts that ask for row tiles the net's LDS tile does not leave room for
    _c("lds-1032-256-256-49@64C", (1032, 256, 256, 49), "tanh", (64, 0), K82, 1),
    _c("lds-1032-128-128-48@32C", (1032, 128, 128, 48), "tanh", (32, 0), K81, 1),
    # k_mlp: first layers wider than 1152 columns (1155: weight rows that are no multiple of 4 floats)
    _c("v1-1153-128-8@1", (1153, 128, 8), "tanh", 1, V81, raw=True),
    _c("v1-1153-128-8@17", (1153, 128, 8), "relu", 17, V81, raw=True),
    _c("v1-1153-128-8@100-nobias", (1153, 128, 8), "tanh", 100, V81, raw=True, bias=False),
    _c("v1-1200-256-256-8@1", (1200, 256, 256, 8), "tanh", 1, V82, raw=True),
    _c("v1-1200-256-256-8@17", (1200, 256, 256, 8), "none", 17, V82, raw=True),
    _c("v1-1200-256-256-8@100-mask", (1200, 256, 256, 8), "tanh", 100, V82, raw=True, mask="sparse"),
    _c("v1-1155-16-3@1", (1155, 16, 3), "tanh", 1, V81, raw=True),
    _c("v1-1155-16-3@17", (1155, 16, 3), "tanh", 17, V81, raw=True, clip=(-0.2, 0.2)),
    _c("v1-1155-16-3@100", (1155, 16, 3), "relu", 100, V81, raw=True),
]
# seeds: the case's index, but for the two one-row nets past 1152 columns, where the first seeds' single row happens to
# hold a small last column (a dropped column must clear the bar in that one row: tests/test_mlp_ref_cpu.py)
SEEDS = {"v1-1200-256-256-8@1": 103, "v1-1155-16-3@1": 100}
CASES = [c._replace(seed=SEEDS.get(c.id, 11 + i)) for i, c in enumerate(CASES)]
# the kernel of a case's raw-weight run where it is not the packed run's: raw weights with a hidden width that is no
# multiple of 16 go to k_mlp (mlp2_shape)
RAW_KERNEL = {"w-7-200-33-250-5-raw2": V82}
# the shapes the child processes of the A/B switches run, at 100 rows, and the kernels each set of switches gives them
SWITCH_SHAPES = [((1032, 128, 128, 48), "tanh"), ((86, 256, 256, 8), "tanh"), ((50, 16, 3), "relu")]
SWITCH_KERNELS = [(("CH_MLP_V1",), ("k_mlp<8,1,2>", "k_mlp<8,2,2>", "k_mlp<8,1,2>")),
                  (("CH_MLP2_NW4",), ("k_mlp2<4,2>", "k_mlp2<8,2>", "k_mlp2<4,2>")),
                  (("CH_MLP_V1", "CH_MLP_WIDE4"), ("k_mlp<8,1,2>", "k_mlp<4,4,1>", "k_mlp<8,1,2>"))]


def case_rows(case, cus):
    return case.rows if isinstance(case.rows, int) else case.rows[0] * cus + case.rows[1]


def case_mask(case, rows):
    """The row mask of a masked case (uint8 [rows]): about 2 % of the rows and the last one."""
    if case.mask is None:
        return None
    m = (np.random.default_rng(case.seed).random(rows) < 0.02).astype(np.uint8)
    m[-1] = 1
    return m


def case_data(case, cus):
    """(layers, x): the case's net and input at ``cus`` compute units."""
    rows = case_rows(case, cus)
    return random_net(case.dims, case.seed, case.bias), random_input(rows, case.dims[0], 1000 + case.seed)
