"""The step-kernel census on the CPU (tests/step_rows.py): every row of the kernel table has a recipe, every recipe
plans to exactly its row whatever the device's CU count, and every directed case the recipes add passes the census of
tests/test_directed_states_cpu.py.  tests/test_gpu_step_rows.py steps the recipes; this module is what keeps a row added
to kStepTable from going unstepped, and a planner edit from moving a recipe to another body unnoticed.

Two-drone shapes (CTDE 2 x 8): the reference's own reward is NaN there (the second-nearest drone distance is inf and
enters the spacing terms), as in the term-table case of tests/test_gpu_directed.py.  Their rewards compare NaN with
NaN; numerically they are judged on observations, cattle state and flags.
"""
import functools
import json
import os

import pytest

import directed_states as D
import step_rows as SR
import test_directed_states_cpu as DC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_geometry_parent.json")


@functools.lru_cache(None)
def _budget():
    """The LDS budget of the golden device (tests/test_step_plan_cpu.py: the CU's 160 KiB)."""
    with open(GOLDEN) as fh:
        g = json.load(fh)
    return min(g["lds_per_cu"], 160 * 1024)


def test_census_keys_are_the_table():
    """One recipe per row of the library's own table: a row added to kStepTable fails here until it gets one."""
    from cattleherd import _lib
    table = tuple(r["name"] for r in _lib.step_kernel_table())
    assert table == _lib.STEP_KERNELS
    assert set(SR.CENSUS) == set(table), set(table) ^ set(SR.CENSUS)
    assert len(SR.STEP_ROWS) == 26 and len(SR.MULTI_ROWS) == 7 and len(SR.ACTOR_ROWS) == 2
    # every row is stepped by tests/test_gpu_step_rows.py or named with the test that holds it
    here = {n for n in SR.CENSUS if SR.family(n) == "k_step2" or (SR.family(n) == "k_step2_multi" and n not in SR.HELD)}
    assert here | set(SR.HELD) == set(SR.CENSUS) and not here & set(SR.HELD)
    assert all(SR.family(n) == "k_step2_actor" for n in SR.CENSUS if n not in here and "multi" not in n)


@pytest.mark.parametrize("cus", SR.CENSUS_CUS)
@pytest.mark.parametrize("name", sorted(SR.CENSUS))
def test_recipe_plans_to_its_row(name, cus):
    """At the directed batch's size (k_step2_multi: the tiled batch's) the recipe's plan names exactly the row, at 16,
    64, 256 and 304 CUs; a specialised row's geometry is the one its body is compiled for."""
    from cattleherd import _lib
    entry = SR.CENSUS[name]
    mode, n, m, level, kw, prec, geom, tobs = entry
    fam = SR.family(name)
    E = SR.MULTI_ENVS[name] if fam == "k_step2_multi" else SR.E_DIRECTED
    p = _lib.step_plan(*SR.shape_of(entry, E), cus, _budget(), geometry=geom or (0, 0))
    assert p["kernel"] == 2
    if fam == "k_step2_actor":
        rows = [r for r in _lib.step_kernel_table() if r["family"] == 2]
        assert p["fused_actor"] == 1 and [r["name"] for r in rows] == sorted(SR.ACTOR_ROWS)
        assert [r["tobs_wpe"] for r in rows] == [0, 1]
        assert all((r["gt"], r["nt"], r["mt"]) == (p["G"], n, m) and r["max_block"] == p["block"] for r in rows)
        return
    assert SR.planned_names(p)[SR.plan_key(name, entry)] == name, (name, cus, p)
    if SR.specialised(name):
        assert geom is not None and (p["G"], p["block"]) == geom
        assert p["G"] == SR.gt_of(name)
    if fam == "k_step2" and SR.specialised(name):
        # the partly filled last workgroup of the second run plans to the same row
        q = _lib.step_plan(*SR.shape_of(entry, SR.partial_envs(name)), cus, _budget(), geometry=geom)
        assert SR.planned_names(q)[SR.plan_key(name, entry)] == name
    if fam == "k_step2_multi":
        # the plain-step twin that ch_step_n is compared with is the k_step2 row of the same geometry
        twin = SR.planned_names(p)["step_row"]
        assert twin in SR.STEP_ROWS and SR.STEP_ROWS[twin][:7] == entry[:7], (name, twin)


FORCED = [((0, 4, 16), (16, 512)), ((0, 4, 16), (16, 640)), ((0, 4, 16), (16, 768)), ((0, 4, 16), (16, 256)),
          ((0, 4, 16), (16, 320)), ((0, 4, 16), (16, 192)), ((0, 4, 16), (8, 512)), ((0, 4, 16), (8, 256)),
          ((0, 2, 8), (16, 512)), ((0, 2, 8), (4, 256)), ((1, 4, 32), (16, 512))]


@pytest.mark.parametrize("shape,geom", FORCED, ids=lambda x: "x".join(str(v) for v in x))
def test_forced_geometry_rows_do_not_depend_on_the_device(shape, geom):
    """The GPU tests that force a geometry assert their rows with no guard on the CU count: under ch__set_geometry the
    plan's rows are the same at 16, 64, 256 and 304 CUs, at every batch size those tests use, in both precisions.  (The
    f32 WPE = 4 row follows the workgroup count, not the device: 4112 envs are apart.)"""
    from cattleherd import _lib
    for prec in (0, 1):
        for E in (16, 24, 48, 96, 98, 100, 104, 257, 1001, 4112):
            plans = [SR.planned_names(_lib.step_plan(*shape, prec, 0, E, cus, _budget(), geometry=geom))
                     for cus in SR.CENSUS_CUS]
            assert all(p == plans[0] for p in plans), (shape, geom, prec, E, plans)
            if E < 4112:
                assert plans[0] == SR.planned_names(_lib.step_plan(*shape, prec, 0, 96, 256, _budget(), geometry=geom))


def test_partial_workgroup_sizes():
    """104 envs at GT = 16 (the last workgroup holds 8), 100 at GT = 8 (4), 98 at GT = 4 (2)."""
    got = {SR.gt_of(n): SR.partial_envs(n) for n in SR.STEP_ROWS if SR.specialised(n)}
    assert got == {16: 104, 8: 100, 4: 98}
    for gt, E in got.items():
        assert E % gt == gt // 2


def test_new_cases_are_what_the_census_adds():
    assert SR.C28 in SR.new_cases(SR.F64) and SR.C28 not in D.CASES
    for prec in (SR.F64, SR.F32):
        for case in SR.new_cases(prec):
            assert case not in (D.CASES if prec == SR.F64 else D.F32_STEP_CASES)


@pytest.mark.parametrize("case", SR.new_cases(SR.F64), ids=D.case_id)
def test_new_f64_case_census(case):
    """One oracle step from the directed batch of a case the f64 rows add: every class present, terminations and
    level-ups where the level has a terminating branch, every truncation cause on its own, pairs under 1 m, in the
    1 m band and the exact 1 m pair all above zero, both flock parities (test_directed_states_cpu's branch floors)."""
    assert {D.class_of(e) for e in range(D.E_DIRECTED)} == set(D.CLASSES)
    _, c = DC._census(case)
    print(f"CENSUS {D.case_id(case)}: pairs<1m {c['lt1']}/{c['pairs']} band {c['band']} exact {c['exact']} term "
          f"{c['term']} levelup {c['levelup']} trunc {c['trunc']} {c['cause']}")
    DC._assert_branch_floors(case, c)
    assert c["trunc"] > 0 and all(v > 0 for v in c["cause"].values()) and c["lt1"] > 0


@pytest.mark.parametrize("case", SR.new_cases(SR.F32), ids=D.case_id)
def test_new_f32_case_census(case):
    """A case the f32 rows add gets the census of D.F32_STEP_CASES: the branch floors, and every deciding quantity of
    the step at least 1e-4 relative from its threshold, so that exact flags are a fair demand of an f32 kernel."""
    DC.test_f32_step_census(case)
