"""Dump the step geometry ch_create gives a grid of handles: tests/golden/step_geometry_parent.json.

usage: python tools/step_geometry_dump.py [out.json]          (needs the built library and a GPU)

The file is the captured reference tests/test_step_plan_cpu.py holds the host-only planner (csrc/ch_step_plan.cpp,
ch__step_plan) against: per grid point ch__geometry's (G, block, lds, kernel), and the device's CU count and LDS bytes
per CU the handles were planned for.  Only ch_create, ch__geometry and ch_destroy are used, so the script runs
unchanged on a library from before the planner.  Every ch_create has its own status check and the first failure ends
the run.

The grid: both modes x N in {2, 3, 4, 6, 8, 12} (and 1, with compat = 0) x M in {8, 14, 16, 17, 32, 64} x f64 / f32 x
PYB and one physics variant (DYN) x E in {96, 1024, 4096, 16384}; and BASELINE configs[0] (1 env, 1 drone, 4 cattle),
the one benchmark config the grid does not hold already.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-cattle-herding_amd"))

COLUMNS = ("mode", "num_drones", "num_cattle", "precision", "physics", "n_envs", "G", "block", "lds", "kernel")
# hipDeviceAttributeMultiprocessorCount, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor (hip_runtime_api.h, ROCm 7)
HIP_ATTR_CUS, HIP_ATTR_LDS_PER_CU = 63, 10002


def grid():
    pts = [(mode, n, m, prec, phys, E)
           for mode in (0, 1) for n in (1, 2, 3, 4, 6, 8, 12) for m in (8, 14, 16, 17, 32, 64) for prec in (0, 1)
           for phys in (0, 1) for E in (96, 1024, 4096, 16384)]
    return pts + [(0, 1, 4, 0, 0, 1)]


def device_limits(device=0):
    """(CU count, LDS bytes per CU) of a HIP device, through the runtime libcattleherd.so is linked against."""
    from cattleherd import _lib
    out = []
    for attr in (HIP_ATTR_CUS, HIP_ATTR_LDS_PER_CU):
        v = ctypes.c_int()
        rc = _lib.lib().hipDeviceGetAttribute(ctypes.byref(v), ctypes.c_int(attr), ctypes.c_int(device))
        if rc != 0:
            raise RuntimeError(f"hipDeviceGetAttribute({attr}) failed: {rc}")
        out.append(v.value)
    return tuple(out)


def main():
    from cattleherd import _lib
    L = _lib.lib()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_geometry_parent.json")
    dev = dict(zip(("cus", "lds_per_cu"), device_limits()))
    rows = []
    for mode, n, m, prec, phys, E in grid():
        cfg = _lib.default_config(mode, n, m)
        cfg.precision, cfg.physics = prec, phys
        if n == 1:
            cfg.compat = 0   # (the reference's rewards need two drones)
        h = ctypes.c_void_p()
        rc = L.ch_create(ctypes.byref(cfg), E, 0, ctypes.byref(h))
        if rc != _lib.CH_OK:
            sys.exit(f"ch_create{(mode, n, m, prec, phys, E)} failed: {rc} {L.ch_last_error(None)}")
        g, blk, lds, kv = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
        rc = L.ch__geometry(h, ctypes.byref(g), ctypes.byref(blk), ctypes.byref(lds), ctypes.byref(kv))
        L.ch_destroy(h)
        if rc != _lib.CH_OK:
            sys.exit(f"ch__geometry{(mode, n, m, prec, phys, E)} failed: {rc}")
        rows.append([mode, n, m, prec, phys, E, g.value, blk.value, lds.value, kv.value])
        if len(rows) % 200 == 0:
            print(f"{len(rows)} handles", flush=True)
    with open(out_path, "w") as fh:
        fh.write('{"cus": %d, "lds_per_cu": %d,\n "columns": %s,\n "points": [\n' %
                 (dev["cus"], dev["lds_per_cu"], json.dumps(list(COLUMNS))))
        fh.write(",\n".join("  " + json.dumps(r) for r in rows))
        fh.write("\n ]}\n")
    print(f"{len(rows)} handles on {dev['cus']} CUs, {dev['lds_per_cu']} B LDS per CU -> {out_path}")


if __name__ == "__main__":
    main()
