"""The step plan on the device: a handle holds the plan the host-only planner gives its shape at the device's own CU
count and LDS size (tests/test_step_plan_cpu.py pins that planner with no device), ch__geometry shows the same plan,
and ch_step_n runs its multi-step kernel exactly where the plan has a row for it -- with, at 96 envs, the outputs,
drawn actions, raw state and metrics of the same number of ch_step calls, bit for bit.
"""
import ctypes

import pytest

from step_rows import device_limits
from test_gpu_step_n_pipeline import _assert_same, _multi

pytestmark = pytest.mark.gpu

F64, F32 = "f64", "f32"
SHAPES = [(mode, n, m, F64, E) for mode, n, m in (("ctde", 4, 16), ("ctde", 2, 8), ("marl", 4, 32)) for E in (96, 4096)] + \
    [("ctde", 4, 16, F32, 4096)]
# whether ch_step_n has a multi-step kernel there, restated from the plan's rules: the BASELINE geometries (16 envs per
# workgroup from 4096 envs up on MI355X's 256 CUs, 2 x 8 from 1024), and f32 at 4 x 16 only; at 96 envs G = 1 and every
# step is a launch
HAS_MULTI = {s: s[4] == 4096 for s in SHAPES}


def _batch(mode, n, m, prec, E):
    from cattleherd.env import HerdBatch
    return HerdBatch(E, n, m, mode=mode, precision=prec)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_handle_plan_and_step_n(shape):
    from cattleherd import _lib
    mode, n, m, prec, E = shape
    a = _batch(*shape)
    cus, lds = device_limits()   # (after torch has initialised the runtime)
    held = _lib.step_plan_of(a.handle)
    want = _lib.step_plan({"ctde": 0, "marl": 1}[mode], n, m, {F64: 0, F32: 1}[prec], 0, E, cus, min(lds, 160 * 1024))
    assert held == want
    g, blk, l, kv = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
    assert _lib.lib().ch__geometry(a.handle, ctypes.byref(g), ctypes.byref(blk), ctypes.byref(l), ctypes.byref(kv)) == 0
    assert (kv.value, g.value, blk.value, l.value) == (held["kernel"], held["G"], held["block"], held["lds"])
    if cus == 256:
        assert (held["multi_row"] >= 0) == HAS_MULTI[shape], held
    # three ch_step_n(4) from a reset: the reset wrote every observation block, so no plain step comes first
    b = _batch(*shape) if E == 96 else None
    a.reset()
    m0 = _multi(a)
    for _ in range(3):
        a.step_n(4, random_actions=True)
    a.sync()
    assert _multi(a) - m0 == (12 if held["multi_row"] >= 0 else 0)
    if b is not None:
        b.reset()
        for _ in range(12):
            b.step(random_actions=True, autoreset=True, terminal_obs=False)
        _assert_same(a, b)
        b.close()
    a.close()
