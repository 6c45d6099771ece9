"""The step-kernel census: one recipe per row of the kernel table (csrc/ch_step_plan.h kStepTable, cattleherd._lib.
STEP_KERNELS), shared by tests/test_step_rows_cpu.py (every recipe plans to its row at 16, 64, 256 and 304 CUs; every
new directed case passes its census) and tests/test_gpu_step_rows.py (every row stepped from the directed batch).

A recipe is (mode, n, m, level, kw, precision, geometry, terminal_obs): the directed case of tests/directed_states.py,
the handle's precision, the ch__set_geometry override (None: the planner's own) and whether the step asks for terminal
observations -- k_step2 has a twin of the 16 x 4 x 16 body that writes them from their producers, and a handle runs
that twin exactly when the caller passes a terminal-observation buffer.  Specialised rows are forced at the directed
batch's 96 envs, so no recipe depends on the device's CU count; runtime-geometry rows take a shape for which the table
has no specialised body at any G, so whatever G the device's CU count gives them they stay on the runtime-geometry body.

Rows the census holds by reference (`HELD`) name the test that steps them; that test asserts the row itself.
"""
import functools
import importlib.util
import os

import directed_states as D

F64, F32 = "f64", "f32"
PREC = {F64: 0, F32: 1}
CENSUS_CUS = (16, 64, 256, 304)
E_DIRECTED = D.E_DIRECTED

C416, C28, C432, C38 = (0, 4, 16, 7, {}), (0, 2, 8, 7, {}), (1, 4, 32, 0, {}), (0, 3, 8, 0, {})
M416, C864 = (1, 4, 16, 0, {}), (0, 8, 64, 7, {})
# physics variants (D.F32_STEP_CASES' own): PYB_GND_DRAG_DW at the driver's shape and MARL 4 x 16, PYB_DW at 6 x 8
P416, PM416, P68 = (0, 4, 16, 7, {"physics": 5}), (1, 4, 16, 0, {"physics": 5}), (0, 6, 8, 7, {"physics": 4})

# k_step2's template arguments behind R -> (directed case, geometry override, terminal_obs); the same for each precision
_STEP2 = {
    "1,0,0,0,true": (PM416, None, False),
    "0,16,4,16,true": (P416, (16, 512), False),
    "0,0,0,0,true": (P68, None, False),
    "1,16,4,32,false,true": (C432, (16, 512), False),
    "1,0,0,0,false,true": (C432, None, False),
    "0,0,0,0,false,true": (C864, None, False),
    "1,0,0,0": (M416, None, False),
    "0,8,4,16": (C416, (8, 256), False),
    "0,16,4,16,false,false,true": (C416, (16, 512), True),
    "0,16,4,16": (C416, (16, 512), False),
    "0,16,2,8": (C28, (16, 512), False),
    "0,4,2,8": (C28, (4, 256), False),
    "0,0,0,0": (C38, None, False),
}
STEP_ROWS = {f"k_step2<{r},{a}>": c[0] + (p, c[1], c[2]) for r, p in (("double", F64), ("float", F32))
             for a, c in _STEP2.items()}

# k_step2_multi: ch_step_n's rows.  `envs`: the tiled batch's size (no multiple of the workgroup's env count; the WPE = 4
# row needs more than 256 workgroups).  The plain-step twin of each is the k_step2 row of the same geometry above.
MULTI_ROWS = {
    "k_step2_multi<double,1,16,4,32,false,true>": C432 + (F64, (16, 512), False),
    "k_step2_multi<double,0,16,4,16>": C416 + (F64, (16, 512), False),
    "k_step2_multi<double,0,8,4,16>": C416 + (F64, (8, 256), False),
    "k_step2_multi<double,0,16,2,8>": C28 + (F64, (16, 512), False),
    "k_step2_multi<double,0,4,2,8>": C28 + (F64, (4, 256), False),
    "k_step2_multi<float,0,16,4,16,false,false,4>": C416 + (F32, (16, 512), False),
    "k_step2_multi<float,0,16,4,16>": C416 + (F32, (16, 512), False),
}
MULTI_ENVS = {name: 1001 for name in MULTI_ROWS}
MULTI_ENVS["k_step2_multi<float,0,16,4,16,false,false,4>"] = 4112   # 257 workgroups of 16

# k_step2_actor: ch_rollout_collect's fused step, configs[3] at its production geometry.  A plan carries both rows or
# neither (`fused_actor`); which one a collection launches follows the terminal-observation buffer, as for k_step2.
ACTOR_ROWS = {
    "k_step2_actor<double,0,16,4,16,false>": C416 + (F64, (16, 768), False),
    "k_step2_actor<double,0,16,4,16,true>": C416 + (F64, (16, 768), True),
}

CENSUS = {**STEP_ROWS, **MULTI_ROWS, **ACTOR_ROWS}

# rows stepped by a test outside tests/test_gpu_step_rows.py, which asserts the row's name from the handle's plan
HELD = {
    "k_step2_multi<double,1,16,4,32,false,true>": "test_gpu_directed.py::test_directed_kernels_bit_identical[marl-4x32-L0-f64-step_n-(16, 512)]",
    "k_step2_multi<double,0,8,4,16>": "test_gpu_directed.py::test_directed_kernels_bit_identical[ctde-4x16-L7-f64-step_n-(8, 256)]",
    "k_step2_multi<float,0,16,4,16>": "test_gpu_directed.py::test_directed_kernels_bit_identical[ctde-4x16-L7-f32-step_n-(16, 512)]",
    "k_step2_actor<double,0,16,4,16,false>": "test_gpu_rollout.py::test_fused_step_actor_is_bit_identical",
    "k_step2_actor<double,0,16,4,16,true>": "test_gpu_rollout.py::test_fused_step_actor_is_bit_identical",
}


def family(name):
    return name.split("<")[0]


def specialised(name):
    """The row's body is compiled for one geometry (GT, NT, MT > 0)."""
    return name.split("<")[1].split(",")[2] != "0"


def gt_of(name):
    return int(name.split("<")[1].split(",")[2])


def partial_envs(name):
    """The smallest batch above the directed 96 envs -- a whole number of workgroups at GT = 16, 8 and 4 -- whose last
    workgroup is half filled: 96 + GT / 2, i.e. 104, 100 and 98 (E mod GT == GT / 2)."""
    gt = gt_of(name)
    assert gt and E_DIRECTED % gt == 0 and gt % 2 == 0
    E = E_DIRECTED + gt // 2
    assert E % gt == gt // 2 and (E + gt - 1) // gt == E_DIRECTED // gt + 1
    return E


def shape_of(entry, E=E_DIRECTED):
    """ch__step_plan's shape arguments of a census entry."""
    mode, n, m, level, kw, prec, geom, tobs = entry
    return mode, n, m, PREC[prec], int(kw.get("physics", 0)), E


def planned_names(p):
    """The names of a plan's rows (cattleherd._lib.step_plan / step_plan_of): step_row, step_row_tobs, multi_row."""
    from cattleherd import _lib
    return {k: (_lib.STEP_KERNELS[p[k]] if p[k] >= 0 else None) for k in ("step_row", "step_row_tobs", "multi_row")}


def held_names(batch):
    """The names of the rows a HerdBatch's handle holds."""
    from cattleherd import _lib
    return planned_names(_lib.step_plan_of(batch.handle))


def plan_key(name, entry):
    """Which of a plan's rows a census entry's row is."""
    if family(name) == "k_step2_multi":
        return "multi_row"
    return "step_row_tobs" if entry[7] else "step_row"


def new_cases(prec):
    """The directed cases the census steps at ``prec`` that tests/test_directed_states_cpu.py does not yet cover: f64
    cases outside D.CASES, f32 cases outside D.F32_STEP_CASES."""
    seen, out = list(D.CASES if prec == F64 else D.F32_STEP_CASES), []
    for entry in CENSUS.values():
        case = entry[:5]
        if entry[5] == prec and case not in seen:
            seen.append(case)
            out.append(case)
    return out


@functools.lru_cache(None)
def device_limits():
    """(compute units, LDS bytes per CU) of the current device, as tools/step_geometry_dump.py reads them; call it
    once torch has initialised the runtime."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("step_geometry_dump", os.path.join(root, "tools", "step_geometry_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.device_limits()


def ratio(a, b, rtol, atol):
    """max |a - b| / (atol + rtol |b|), NaN equal to NaN: at most 1 exactly where helpers.close holds."""
    import numpy as np
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not a.size:
        return 0.0
    both = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        r = np.where(both | (a == b), 0.0, np.abs(a - b) / (atol + rtol * np.abs(b)))
    return float(np.where(np.isnan(r), np.inf, r).max())
