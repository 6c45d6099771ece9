"""CPU-only checks of the policy forward's reference and error bar (tests/mlp_ref.py), so that the GPU tests that pin
the forward kernels to them (tests/test_gpu_mlp_variants.py) compare with something that is itself pinned: over the
same case matrix, a float32 forward with an exact tanh lies inside the bar (it is not too tight), forwards that are
wrong the way a kernel goes wrong -- a dropped input column, a missing bias, a neighbour's row, a skipped activation,
a K-pair of stale values -- lie outside it (it is not too loose), and a float32 model of tanh_fast whose exp2 and
reciprocal are off by their documented ulp stays inside TAU.

The shapes are the GPU matrix's at CUS compute units: the row counts only choose the kernel, the bar depends on the
net and the input's distribution.

Why the bar has two terms.  The order-free bound (K + 2) u |W||h| alone is used to 1e-5 by a float32 forward of a
net whose first layer is a thousand columns wide, and on the 1200-256-256-8 net a dropped input column stayed at 0.30
to 0.54 of it and a skipped tanh at 0.23: it would not have seen a stale column.  With the pair-ordered term
(mlp_ref's docstring) every wrong forward below clears the bar on every shape."""
import numpy as np
import pytest

import mlp_ref as R

CUS = 64   # the row-tiled cases at 32 CUS + 17 and 64 CUS + 33 rows


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(case):
        if case.id not in cache:
            layers, x = R.case_data(case, CUS)
            cache[case.id] = (layers, x, R.forward64(layers, case.act, case.clip, x), R.bar(layers, case.act, case.clip, x))
            for a in cache[case.id][2:]:
                a.setflags(write=False)
        return cache[case.id]
    return get


def _ids(cases):
    return [c.id for c in cases]


def test_case_ids_are_unique_and_cover_every_instantiation_outside_collections():
    assert len(set(_ids(R.CASES))) == len(R.CASES)
    assert {c.kernel for c in R.CASES} == {R.K81, R.K82, R.K81R2, R.K44R2, R.K44R4, R.V81, R.V82}
    for group, want in ((R.K81, {1, 3, 4, 7, 8, 31, 33, 86, 129, 1152}),):
        assert want <= {c.dims[0] for c in R.CASES if c.kernel == group}
    narrow = [c for c in R.CASES if c.kernel == R.K81]
    assert {1, 15, 16, 17, 127, 128} <= {w for c in narrow for w in c.dims[1:]}
    assert {1, 2, 3, 4} <= {len(c.dims) - 1 for c in narrow} and {"tanh", "relu", "none"} <= {c.act for c in narrow}
    assert {1, 15, 16, 17, 100} <= {c.rows for c in narrow} and {1, 15, 16, 17, 100} <= {c.rows for c in R.CASES if c.kernel == R.K82}
    assert {129, 255, 256} <= {w for c in R.CASES if c.kernel == R.K82 for w in c.dims[1:]}


@pytest.mark.parametrize("case", R.CASES, ids=_ids(R.CASES))
def test_float32_forward_is_inside_the_bar(case, refs):
    layers, x, y64, bar = refs(case)
    err = np.abs(R.forward32(layers, case.act, case.clip, x).astype(np.float64) - y64)
    assert np.all(err <= bar), float((err / bar).max())
    assert np.all(bar > 0) and np.all(np.isfinite(bar))


@pytest.mark.parametrize("case", [c for c in R.CASES if isinstance(c.rows, int)][::4], ids=lambda c: c.id)
def test_bar_is_never_wider_than_the_order_free_bound(case, refs):
    layers, x, _y64, bar = refs(case)
    flat = R.bar(layers, case.act, case.clip, x, paired=False)
    assert np.all(bar <= flat)
    if case.dims[0] <= 30:
        assert np.array_equal(bar[:, :1], flat[:, :1]) or len(layers) > 1   # short sums: the order-free term governs


def test_live_width_zeroes_columns_and_counts_the_live_terms():
    layers = R.random_net((344, 16, 3), 5)
    x = R.random_input(6, 344, 6)
    live = np.array([344, 86, 172, 0, 258, 344])
    xz = np.where(np.arange(344)[None, :] < live[:, None], x, 0.0)
    assert np.array_equal(R.forward64(layers, "tanh", None, x, live), R.forward64(layers, "tanh", None, xz))
    b, bz = R.bar(layers, "tanh", None, x, live), R.bar(layers, "tanh", None, xz)
    assert np.all(b <= bz) and np.all(b[1] < bz[1]) and np.array_equal(b[0], bz[0])


# ---- forwards that are wrong the way a kernel goes wrong --------------------------------------------------------
def _drop_column(col):
    def f(case, layers, x):
        if not 0 <= (c := col(case)) < case.dims[0]:
            return None
        x = x.copy()
        x[:, c] = 0.0
        return layers, x, {}
    return f


def _no_bias(case, layers, x):
    if not case.bias:
        return None
    w, b = layers[-1]
    b = b.copy()
    b[int(np.argmax(np.abs(b)))] = 0.0
    return layers[:-1] + [(w, b)], x, {}


def _neighbour_row(case, layers, x):
    if x.shape[0] < 2:
        return None
    x = x.copy()
    x[-1] = x[-2]
    return layers, x, {}


def _skip_activation(case, layers, x):
    if len(layers) < 2 or case.act == "none":
        return None
    return layers, x, {"skip": True}


def _stale_pair(case, layers, x):
    """K-pair p (columns [32 p, 32 p + 32) of the input) of every row holds another row's values."""
    if x.shape[0] < 2:
        return None
    p = (case.dims[0] - 1) // 32
    x = x.copy()
    x[:, 32 * p:32 * p + 32] = np.roll(x[:, 32 * p:32 * p + 32], 1, axis=0)
    return layers, x, {}


WRONG = {"last-column-dropped": _drop_column(lambda c: c.dims[0] - 1),
         "column-512-dropped": _drop_column(lambda c: 512 if c.dims[0] > 512 else -1),
         "bias-omitted": _no_bias, "neighbour-row": _neighbour_row, "activation-skipped": _skip_activation,
         "stale-k-pair": _stale_pair}


def _forward_skipping_unit(layers, act, clip, x):
    """forward64 with one hidden unit left without its activation: in each hidden layer the unit the activation changes
    most; the layer whose skip moves the output most is returned."""
    best = None
    for skip in range(len(layers) - 1):
        h = np.asarray(x, np.float64)
        for i, (w, b) in enumerate(layers):
            h = h @ np.asarray(w, np.float64).T
            if b is not None:
                h = h + np.asarray(b, np.float64)
            if i < len(layers) - 1:
                a = R._act(h, act)
                if i == skip:
                    u = int(np.argmax(np.abs(a - h).max(axis=0)))
                    a[:, u] = h[:, u]
                h = a
        y = h if clip is None else np.clip(h, clip[0], clip[1])
        ref = R.forward64(layers, act, clip, x)
        if best is None or np.abs(y - ref).max() > np.abs(best - ref).max():
            best = y
    return best


@pytest.mark.parametrize("wrong", list(WRONG))
@pytest.mark.parametrize("case", R.CASES, ids=_ids(R.CASES))
def test_wrong_forward_is_outside_the_bar(case, wrong, refs):
    layers, x, y64, bar = refs(case)
    made = WRONG[wrong](case, layers, x)
    if made is None:
        return   # (the variant does not exist for this shape: no bias, one row, one layer, no activation, K0 <= 512)
    wl, wx, opt = made
    y = _forward_skipping_unit(wl, case.act, case.clip, wx) if opt.get("skip") else R.forward64(wl, case.act, case.clip, wx)
    ratio = np.abs(y - y64) / bar
    assert ratio.max() > 1.0, float(ratio.max())


def test_every_wrong_forward_applies_to_most_of_the_matrix():
    for name, make in WRONG.items():
        n = sum(make(c, *R.case_data(c, 1)[:2]) is not None for c in R.CASES if isinstance(c.rows, int))
        assert n >= (3 if name == "column-512-dropped" else 20), (name, n)


# ---- tanh_fast ---------------------------------------------------------------------------------------------------
def test_tau_is_the_docstrings_sum():
    assert R.TAU == 7.4 * 2.0 ** -24 and R.U == 2.0 ** -24
    v = np.linspace(0.0, 5.0, 200001)
    assert (v / np.cosh(v) ** 2).max() < 0.448    # the factor of the s term


@pytest.mark.parametrize("d_exp,d_rcp", [(0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_tanh_fast_model_is_within_tau(d_exp, d_rcp):
    v = R.tanh_sweep()
    t = R.tanh_fast_model(v, d_exp, d_rcp).astype(np.float64)
    err = np.abs(t - np.tanh(v.astype(np.float64)))
    assert err.max() <= R.TAU, float(err.max() / R.TAU)
    if (d_exp, d_rcp) == (0, 0):   # saturation is exact where exp2(-inf) = 0, rcp(1) = 1 and rcp(inf) = 0 are
        for big in (np.float32(100.0), np.float32(np.inf)):
            assert R.tanh_fast_model(np.array([big, -big])).tolist() == [1.0, -1.0]


def test_tanh_fast_model_two_ulps_off_is_caught_somewhere():
    """TAU is not slack by a large factor: exp2 and the reciprocal 8 ulps off pass it."""
    v = R.tanh_sweep()
    err = np.abs(R.tanh_fast_model(v, 8, 8).astype(np.float64) - np.tanh(v.astype(np.float64)))
    assert err.max() > R.TAU
