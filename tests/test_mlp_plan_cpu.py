"""The policy forward's dispatch on the CPU: csrc/ch_mlp_plan.cpp's planner (through the host-only ch__mlp_plan) and
csrc/ch_mlp_plan.h's kernel table (ch__mlp_kernel).  The planner is a pure function of (nets, row counts, CU count,
switches), so what tests/test_gpu_mlp_variants.py reads back after real launches is asserted here with no device: every
mlp_ref.CASES entry at three CU counts, the A/B switch sets, the collection's two-segment launches -- and, over a grid
of nets and row counts, the properties whose violations were the two dispatch bugs that module's docstring records.
"""
import ctypes
import itertools

import pytest

import mlp_ref as R

CUS = (64, 256, 304)
# restated here, not read from the library: k_mlp2's first layer holds 1152 live columns = 36 pairs of 32,
# its dynamic LDS is capped 1 KiB under the CU's 160 KiB
MAX_PAIR0 = 36
LDS_MAX2 = 160 * 1024 - 1024


def _net(dims, packed=True):
    """A ChMlp the planner can read: widths, and dummy non-NULL 16-byte aligned addresses (nothing is dereferenced)."""
    from cattleherd import _lib
    net = _lib.ChMlp()
    net.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        net.dims[i] = d
    for i in range(net.n_layers):
        net.weight[i] = 4096
    net.hidden_act = _lib.CH_ACT_TANH
    net.packed = 4096 if packed else None
    return net


def _plan(dims_list, rows, cus, packed=True, **kw):
    from cattleherd import _lib
    return _lib.mlp_plan([_net(d, packed) for d in dims_list], rows, cus, **kw)


def _pad_pairs(k):
    return ((max(k, 1) + 31) // 32 + 3) // 4 * 4


def test_table_names_are_the_bindings():
    from cattleherd import _lib
    table = _lib.mlp_kernel_table()
    assert tuple(r["name"] for r in table) == _lib.MLP_KERNELS
    for r in table[1:]:
        fam, args = r["name"].split("<")
        assert r["family"] == {"k_mlp2": 2, "k_mlp": 1}[fam]
        a = args.rstrip(">").split(",")
        assert (r["nw"], r["tw"]) == (int(a[0]), int(a[1]))
        if fam == "k_mlp2":
            assert r["share"] == (len(a) > 2 and a[2] == "true") and r["rt"] == (int(a[3]) if len(a) > 3 else 1)
            # the staging ring (ch_mlp2_dev.h mlp2_body): 4 NW threads a row, 8 float4 registers each where NW = 4
            # and RT > 1 (512 columns), else every first layer k_mlp2 takes
            assert r["max_pair0"] == (16 if r["nw"] == 4 and r["rt"] > 1 else MAX_PAIR0)
            assert r["packed_only"] == (r["nw"] == 4 and r["rt"] > 1) and not r["raw_ragged"]
        else:
            assert r["rt"] == 1 and not r["packed_only"] and r["raw_ragged"] and r["max_pair0"] > 1200 // 32


@pytest.mark.parametrize("cus", CUS)
def test_cases_plan_to_their_kernels(cus):
    for case in R.CASES:
        rows = R.case_rows(case, cus)
        grid = (rows + 16 * case.rt - 1) // (16 * case.rt)
        p = _plan([case.dims], [rows], cus)
        assert (p["kernel"], p["rt"], p["grid"]) == ([case.kernel], case.rt, [grid]), (case.id, p)
        assert p["v2"] == case.kernel.startswith("k_mlp2") and p["lds"] > 0
        if case.raw:
            p = _plan([case.dims], [rows], cus, packed=False)
            assert (p["kernel"], p["rt"], p["grid"]) == ([R.RAW_KERNEL.get(case.id, case.kernel)], case.rt, [grid]), (case.id, p)


def test_switches_in_process():
    for switches, kernels in R.SWITCH_KERNELS:
        kw = {{"CH_MLP_V1": "v1", "CH_MLP2_NW4": "nw4", "CH_MLP_WIDE4": "wide4"}[s]: True for s in switches}
        got = [_plan([dims], [100], 256, **kw)["kernel"] for dims, _act in R.SWITCH_SHAPES]
        assert got == [[k] for k in kernels], (switches, got)


@pytest.mark.parametrize("cus", CUS)
def test_collection_pair(cus):
    """ch_rollout_collect's actor + critic launch (tests/test_gpu_mlp_variants.py test_collection_forwards_vs_fp64)."""
    pair = [(1032, 128, 128, 16), (1032, 128, 128, 1)]
    p = _plan(pair, [64, 64], cus, kcap=[344, 344])
    assert p["v2"] and p["kernel"] == ["k_mlp2<8,1,true>"] * 2 and p["rt"] == 1 and p["grid"] == [4, 4]
    p = _plan(pair, [16 * cus, 16 * cus], cus, kcap=[344, 344])
    assert p["v2"] and p["kernel"] == ["k_mlp2<8,1,false,2>"] * 2 and p["rt"] == 2 and p["grid"] == [cus // 2] * 2
    # V(last obs) alone, and a zero-row segment in the middle is skipped
    assert _plan(pair[1:], [64], cus, kcap=[344])["kernel"] == ["k_mlp2<8,1>"]
    p = _plan([pair[0], pair[1], pair[1]], [64, 0, 17], cus, kcap=[344] * 3)
    assert p["kernel"] == ["k_mlp2<8,1,true>"] * 2 and p["grid"] == [4, 2]


def test_zero_rows_plan_nothing():
    for dims in ((3, 15, 16), (1200, 256, 256, 8)):
        for kw in ({}, {"v1": True}, {"rt": 4}):
            p = _plan([dims], [0], 256, **kw)
            assert p["kernel"] == [] and p["grid"] == [] and not p["v2"]
    p = _plan([(3, 15, 16)] * 3, [0, 0, 0], 256)
    assert p["kernel"] == [] and not p["v2"]


def _grid_nets():
    """dims[0] x hidden stacks (every one- and two-layer stack of the widths, the three-layer stacks of a diagonal and
    its rotations) x output widths."""
    hs = (16, 33, 127, 128, 129, 200, 255, 256)
    stacks = [(a,) for a in hs] + list(itertools.product(hs, hs)) + \
        [(hs[i], hs[(i + s) % 8], hs[(i + 2 * s + 1) % 8]) for i in range(8) for s in range(3)]
    for d0 in (1, 7, 86, 344, 512, 513, 600, 896, 1032, 1152, 1153, 1200):
        for st in stacks:
            for out in (1, 8, 49, 256):
                yield (d0,) + st + (out,)


def test_plan_invariants_over_the_grid():
    """At 256 CUs and default switches, for every net of the grid, packed and raw, full and 344-column live widths, one
    segment at each row count and two-segment launches beside a fixed partner: what a plan's table row tolerates holds
    for the nets it is given."""
    from cattleherd import _lib
    table = {r["name"]: r for r in _lib.mlp_kernel_table()}
    C = 256
    row_counts = (0, 1, 16, 17, 32 * C - 1, 32 * C, 32 * C + 17, 64 * C, 64 * C + 33)
    partner = ((86, 256, 256, 8), True, 86)   # a wide packed net beside each net of the grid
    n = 0
    for dims in _grid_nets():
        for packed in (True, False):
            for kcap in {dims[0], min(dims[0], 344)}:
                net = _net(dims, packed)
                ragged = any(d % 16 for d in dims[1:-1])
                for rows in row_counts:
                    for two in (False, True):
                        nets, rws, kc = [net], [rows], [kcap]
                        if two:
                            if rows not in (17, 32 * C):
                                continue
                            nets, rws, kc = [net, _net(partner[0], partner[1])], [rows, rows], [kcap, partner[2]]
                        p = _lib.mlp_plan(nets, rws, C, kcap=kc)
                        n += 1
                        assert len(p["kernel"]) == (0 if rows == 0 else len(nets))
                        if _pad_pairs(kcap) > MAX_PAIR0 and rows > 0:
                            assert not p["v2"], (dims, kcap)
                        for k in p["kernel"][:1 if p["v2"] else None]:
                            row = table[k]
                            assert (row["family"] == 2) == p["v2"] and row["rt"] == p["rt"]
                            if not p["v2"]:
                                continue
                            assert p["lds"] <= LDS_MAX2, (dims, p)
                            assert max(_pad_pairs(c) for c in kc) <= row["max_pair0"], (dims, kcap, p)
                            assert packed or not row["packed_only"], (dims, p)
                            assert packed or not ragged, (dims, p)
                            assert max(max(m.dims[1:m.n_layers + 1]) for m in nets) <= 16 * row["nw"] * row["tw"]
    assert n > 100000
