"""The env step's dispatch on the CPU: csrc/ch_step_plan.cpp's planner (through the host-only ch__step_plan) and
csrc/ch_step_plan.h's kernel table (ch__step_kernel).  The planner is a pure function of (shape, CU count, LDS budget,
overrides), so which kernel, geometry and table rows a handle gets is asserted here with no device.

The geometry reference is captured, not derived: tests/golden/step_geometry_parent.json holds ch__geometry's (G, block,
lds, kernel) of 1345 handles created on an MI355X by the commit before the planner existed (tools/
step_geometry_dump.py), with the device's CU count and LDS bytes per CU.

Coverage.  At the golden device (256 CUs, 160 KiB) two things cannot happen to a default plan, whatever the grid:
  * k_step2<double,0,4,2,8> and its k_step2_multi twin need 2 drones x 8 cattle in f64 at G = 4, i.e. 4 <= E / CUs < 8,
    and from 1024 envs up the 2x8 rule gives such a handle G = 16; below 1024 envs E / 256 < 4.  A device of fewer CUs
    plans it (and ch__set_geometry(4, 256) forces it, which tests/test_gpu_runtime.py steps), so the rows are covered
    over the grid at 16, 64, 256 and 304 CUs together.
  * the v1 fallback needs one env's shared tables above the budget; at num_cattle <= 64 they are 68.5 KB at the most.
    It is covered at a budget of 64 KiB, the one ch_create plans for when the device does not report its LDS size.
"""
import functools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_geometry_parent.json")
CUS = (64, 256, 304)
LDS_CAP = 160 * 1024   # restated: the step kernels opt in to the CU's 160 KiB and ch_create caps its budget there
PYB, PYB_DRAG, F64, F32, CTDE, MARL = 0, 3, 0, 1, 0, 1
STEP, MULTI, ACTOR = 0, 1, 2
PIPELINED = "k_step2_multi<double,0,16,4,16>"
# bench.py WORKLOADS at their benchmark sizes and BASELINE configs[0]: (mode, drones, cattle, precision, physics, envs)
C1, C2, C3, C4, C5 = (CTDE, 1, 4, F64, PYB, 1), (CTDE, 2, 8, F64, PYB, 1024), (CTDE, 2, 8, F64, PYB, 4096), \
    (CTDE, 4, 16, F64, PYB, 4096), (MARL, 4, 32, F64, PYB, 4096)


@functools.lru_cache(None)
def golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    assert g["columns"] == ["mode", "num_drones", "num_cattle", "precision", "physics", "n_envs", "G", "block", "lds", "kernel"]
    return g["cus"], min(g["lds_per_cu"], LDS_CAP), [tuple(p) for p in g["points"]]


@functools.lru_cache(None)
def table():
    from cattleherd import _lib
    return _lib.step_kernel_table()


@functools.lru_cache(None)
def plan(shape, cus, budget, kernel=0, geometry=(0, 0)):
    from cattleherd import _lib
    return _lib.step_plan(*shape, cus, budget, kernel=kernel, geometry=geometry)


def names(p):
    from cattleherd import _lib
    return {k: (_lib.STEP_KERNELS[p[k]] if p[k] >= 0 else None) for k in ("step_row", "step_row_tobs", "multi_row")}


def test_grid_is_the_issues():
    """Both modes x N {2, 3, 4, 6, 8, 12} and 1 x M {8, 14, 16, 17, 32, 64} x f64 / f32 x PYB and one variant x E {96,
    1024, 4096, 16384}, and the five BASELINE configs at their benchmark sizes."""
    _, _, pts = golden()
    shapes = {p[:6] for p in pts}
    assert len(shapes) == len(pts)
    variants = {s[4] for s in shapes} - {PYB}
    assert len(variants) == 1
    want = {(mode, n, m, prec, phys, E) for mode in (CTDE, MARL) for n in (1, 2, 3, 4, 6, 8, 12)
            for m in (8, 14, 16, 17, 32, 64) for prec in (F64, F32) for phys in (PYB,) + tuple(variants)
            for E in (96, 1024, 4096, 16384)}
    assert want | {C1, C2, C3, C4, C5} == shapes


def test_plan_equals_the_parent_geometry():
    cus, budget, pts = golden()
    assert (cus, budget) == (256, 163840)
    for pt in pts:
        p = plan(pt[:6], cus, budget)
        assert (p["G"], p["block"], p["lds"], p["kernel"]) == pt[6:], (pt, p)
        assert p["pw"] == (p["kernel"] == 2 and pt[2] >= 17 and pt[4] == PYB), (pt, p)


def test_directed_geometries():
    """What tests/test_gpu_directed.py records: ch__geometry's lds at 96 envs, and its two forced geometries."""
    cus, budget, _ = golden()
    lds_96 = {(4, 16): 8688, (3, 8): 4000, (6, 16): 9328, (12, 16): 11216, (4, 32): 19440, (8, 64): 68512}
    for (n, m), lds in lds_96.items():
        for mode in (CTDE, MARL):
            p = plan((mode, n, m, F64, PYB, 96), cus, budget)
            assert (p["G"], p["lds"], p["kernel"]) == (1, lds, 2) and (p["block"] == 128) == (m > 16), (n, m, p)
    p = plan((CTDE, 2, 14, F64, PYB, 96), cus, budget, geometry=(31, 256))
    assert (p["G"], p["block"], p["lds"], p["kernel"], p["sep"]) == (31, 256, 153280, 2, 0)   # `sep` would be 168912 B
    # a physics-variant handle with 18 cows: v1 by default, the shared-table kernel when forced to v2
    shape = (CTDE, 3, 18, F64, PYB_DRAG, 96)
    assert plan(shape, cus, budget)["kernel"] == 1
    p = plan(shape, cus, budget, kernel=2, geometry=(20, 256))
    assert (p["G"], p["block"], p["lds"], p["kernel"], p["sep"], p["pw"]) == (20, 256, 155680, 2, 0, 0)
    assert names(p)["step_row"] == "k_step2<double,0,0,0,0,true>"


def test_override_statuses():
    """ch__set_geometry's and ch__set_kernel's accept / reject results, as the setters gave them before the planner."""
    from cattleherd import _lib
    cus, budget, _ = golden()

    def rc(shape, **kw):
        try:
            plan(shape, cus, budget, **kw)
            return _lib.CH_OK
        except _lib.ChError as e:
            return e.code
    c4_96, c5_96 = C4[:5] + (96,), C5[:5] + (96,)
    for geom in ((0, 256), (65, 256), (17, 256), (4, 64), (4, 200), (4, 832)):   # G range, G * N <= 64, block range
        assert rc(c4_96, geometry=geom) == _lib.CH_ERR_INVALID, geom
    assert rc(c4_96, geometry=(16, 768)) == _lib.CH_OK
    assert rc(c5_96, geometry=(1, 768)) == _lib.CH_ERR_INVALID                     # per-wave tables: 512 at the most
    assert rc(C4[:4] + (PYB_DRAG, 96), geometry=(16, 768)) == _lib.CH_ERR_INVALID   # physics variants too
    assert rc(c4_96, geometry=(16, 128)) == _lib.CH_ERR_UNSUPPORTED                # 256 cows > 3 * 64 lanes
    # (tests/test_gpu_directed.py's docstring: 2 drones x 16 cattle fit the plain layout up to 26 envs per workgroup)
    assert rc((CTDE, 2, 16, F64, PYB, 96), geometry=(26, 256)) == _lib.CH_OK
    assert rc((CTDE, 2, 16, F64, PYB, 96), geometry=(32, 256)) == _lib.CH_ERR_UNSUPPORTED   # the LDS carve
    assert rc(c4_96, kernel=3) == _lib.CH_ERR_INVALID
    assert rc(c4_96, kernel=1) == _lib.CH_OK and plan(c4_96, cus, budget, kernel=1)["step_row"] == -1
    # one env's tables above a small budget: the v1 fallback, and no way to v2
    big = (CTDE, 8, 64, F64, PYB_DRAG, 96)
    p = plan(big, cus, 64 * 1024)
    assert p["kernel"] == 1 and "v1_fallback" in p["rules"] and p["lds"] > 64 * 1024
    with pytest.raises(_lib.ChError) as e:
        plan(big, cus, 64 * 1024, kernel=2)
    assert e.value.code == _lib.CH_ERR_UNSUPPORTED


def test_table_properties():
    from cattleherd import _lib
    t = table()
    assert tuple(r["name"] for r in t) == _lib.STEP_KERNELS and len(set(_lib.STEP_KERNELS)) == len(t)
    assert _lib.step_rules() == _lib.STEP_RULES
    for r in t:
        fam, args = r["name"].rstrip(">").split("<")
        a = args.split(",")
        assert r["family"] == {"k_step2": STEP, "k_step2_multi": MULTI, "k_step2_actor": ACTOR}[fam]
        assert r["precision"] == {"double": F64, "float": F32}[a[0]]
        assert [r["mode"], r["gt"], r["nt"], r["mt"]] == [int(x) for x in a[1:5]]
        assert len({r["gt"] > 0, r["nt"] > 0, r["mt"] > 0}) == 1, r
        rest = a[5:]
        if fam == "k_step2_actor":
            assert rest in (["false"], ["true"]) and r["tobs_wpe"] == (rest == ["true"]) and not r["phys"] and not r["pw"]
            assert r["max_block"] == 768 and not r["pipelined"]                       # __launch_bounds__(CH_V2_MAX_BLOCK)
            continue
        rest += ["false", "false", "false" if fam == "k_step2" else "1"][len(rest):]
        assert [r["phys"], r["pw"]] == [x == "true" for x in rest[:2]]
        if fam == "k_step2":
            assert r["tobs_wpe"] == (rest[2] == "true") and not r["pipelined"]
            assert r["max_block"] == (512 if r["pw"] or r["phys"] else 768)           # CH_V2_MAX_BLOCK_PW / CH_V2_MAX_BLOCK
        else:
            assert r["tobs_wpe"] == int(rest[2]) and not r["phys"]
            assert r["pipelined"] == (r["name"] == PIPELINED)
            assert r["max_block"] == (640 if r["pipelined"] else 512)                 # CH_MULTI_PIPE_MAX_BLOCK / CH_MULTI_MAX_BLOCK


def check_plan(shape, cus, budget, p):
    mode, n, m, prec, phys, E = shape
    t = table()
    if p["kernel"] != 2:
        assert (p["step_row"], p["step_row_tobs"], p["multi_row"], p["fused_actor"]) == (-1, -1, -1, 0), (shape, p)
        return
    G, block = p["G"], p["block"]
    assert G * n <= 64 and G * m <= 3 * (block - 64) and p["lds"] <= budget, (shape, p)
    for key, fam in (("step_row", STEP), ("step_row_tobs", STEP), ("multi_row", MULTI)):
        if p[key] < 0:
            assert key == "multi_row"
            continue
        r = t[p[key]]
        assert (r["family"], r["precision"], r["mode"], r["phys"], r["pw"]) == (fam, prec, mode, phys != PYB, p["pw"]), (shape, p, r)
        assert (r["gt"], r["nt"], r["mt"]) in ((0, 0, 0), (G, n, m)), (shape, p, r)
        assert (p["multi_block"] if fam == MULTI else block) <= r["max_block"], (shape, p, r)
    assert t[p["step_row"]]["tobs_wpe"] == 0
    if p["multi_row"] >= 0:
        r = t[p["multi_row"]]
        assert phys == PYB and p["multi_block"] == min(block, r["max_block"]) and p["multi_lds"] <= budget, (shape, p)
        if r["pipelined"]:
            assert p["sep"] and p["multi_block"] >= 256 and G * m <= 3 * (p["multi_block"] - 128) and p["multi_lds"] > p["lds"]
        else:
            assert p["multi_lds"] == p["lds"]
    if p["fused_actor"]:
        assert (prec, mode, n, m, G, block, phys, p["pw"]) == (F64, CTDE, 4, 16, 16, 768, PYB, 0), (shape, p)


@pytest.mark.parametrize("cus", CUS)
def test_plan_properties_over_the_grid(cus):
    _, budget, pts = golden()
    for pt in pts:
        check_plan(pt[:6], cus, budget, plan(pt[:6], cus, budget))
    # and under the overrides the GPU tests use
    for shape, kw in ((C4, dict(geometry=(8, 512))), (C4, dict(geometry=(16, 512))), (C4, dict(geometry=(16, 256))),
                      (C2, dict(geometry=(4, 256))), (C5, dict(geometry=(8, 512))), (C4, dict(kernel=1)),
                      ((CTDE, 3, 18, F64, PYB_DRAG, 96), dict(kernel=2, geometry=(20, 256)))):
        check_plan(shape, cus, budget, plan(shape, cus, budget, **kw))


def test_every_rule_and_row_is_reached():
    """Module docstring: over the grid at 16, 64, 256 and 304 CUs every table row is some plan's; at the golden device
    every rule but the v1 fallback fires, which does at a 64 KiB budget."""
    from cattleherd import _lib
    cus0, budget, pts = golden()
    rows, rules = set(), set()
    for cus in (16,) + CUS:
        for pt in pts:
            p = plan(pt[:6], cus, budget)
            rows |= {p["step_row"], p["step_row_tobs"], p["multi_row"]}
            if p["fused_actor"]:
                rows |= {i for i, r in enumerate(table()) if r["family"] == ACTOR}
            if cus == cus0:
                rules |= set(p["rules"])
    assert rows - {-1} == set(range(len(_lib.STEP_KERNELS))), [_lib.STEP_KERNELS[i] for i in set(range(len(table()))) - rows]
    assert rules == set(_lib.STEP_RULES) - {"v1_fallback"}
    assert any("v1_fallback" in plan(pt[:6], cus0, 64 * 1024)["rules"] for pt in pts)


def test_baseline_configs_plan_to_their_kernels():
    cus, budget, _ = golden()
    f32 = lambda s, E=None: s[:3] + (F32,) + s[4:5] + (E or s[5],)   # noqa: E731
    expect = [
        (C4, {}, "k_step2<double,0,16,4,16>", "k_step2<double,0,16,4,16,false,false,true>", PIPELINED),
        (C2, {}, "k_step2<double,0,16,2,8>", None, "k_step2_multi<double,0,16,2,8>"),
        (C3, {}, "k_step2<double,0,16,2,8>", None, "k_step2_multi<double,0,16,2,8>"),
        (C2, dict(geometry=(4, 256)), "k_step2<double,0,4,2,8>", None, "k_step2_multi<double,0,4,2,8>"),
        (C4, dict(geometry=(8, 512)), "k_step2<double,0,8,4,16>", None, "k_step2_multi<double,0,8,4,16>"),
        (C5, {}, "k_step2<double,1,16,4,32,false,true>", None, "k_step2_multi<double,1,16,4,32,false,true>"),
        (C1, {}, "k_step2<double,0,0,0,0>", None, None),
        (f32(C2), {}, "k_step2<float,0,4,2,8>", None, None),
        # f32: two workgroups per CU (WPE = 4) above 256 workgroups -- the threshold is the literal, not the device's CUs
        (f32(C4), {}, "k_step2<float,0,16,4,16>", "k_step2<float,0,16,4,16,false,false,true>", "k_step2_multi<float,0,16,4,16>"),
        (f32(C4, 4112), {}, "k_step2<float,0,16,4,16>", "k_step2<float,0,16,4,16,false,false,true>",
         "k_step2_multi<float,0,16,4,16,false,false,4>"),
        (f32(C4, 262144), {}, "k_step2<float,0,16,4,16>", "k_step2<float,0,16,4,16,false,false,true>",
         "k_step2_multi<float,0,16,4,16,false,false,4>"),
    ]
    for shape, kw, step, tobs, multi in expect:
        p = plan(shape, cus, budget, **kw)
        assert names(p) == {"step_row": step, "step_row_tobs": tobs or step, "multi_row": multi}, (shape, kw, p)
        assert p["fused_actor"] == (shape == C4 and not kw)
    p = plan(C4, cus, budget)
    assert (p["multi_block"], p["multi_lds"] - p["lds"]) == (640, 19360)   # V2Pipe<double>::kBytes
    assert plan(f32(C4, 262144), 304, budget)["multi_row"] == plan(f32(C4, 262144), cus, budget)["multi_row"]
    assert names(plan(f32(C4, 16 * 304), 304, budget))["multi_row"] == "k_step2_multi<float,0,16,4,16,false,false,4>"
