"""Directed oracle states: batches that put drones inside the herd and envs on every terminating / truncating
branch of the task, for the GPU-vs-oracle tests of tests/test_gpu_directed.py (states reached by random actions
leave every cow-drone pair beyond the predator range and end no episode).

``directed_states`` builds each env on the CPU oracle alone: a reset, a few random steps (so that PID state,
velocities, attitude and the flock parity vary -- the flock runs every other step), then plain NumPy placement
on the state dict by class, cycling over the envs, and ``Env.set_state``.  tests/test_directed_states_cpu.py
holds the census that keeps the GPU tests from passing vacuously.
"""
import numpy as np

# curriculum_learning.py:10-194 (oracle/ch_oracle.c LEVELS, which the oracle's binding does not expose): desired spacing, tolerance, hold, approach_min, min_eff,
# cattle_desired, cattle_tol, episode length (s), required tally
LEVELS = [(0.8, 0.3, 10, 0.0, 0, 0.0, 0.0, 40, 100), (0.8, 0.2, 25, 0.0, 0, 0.0, 0.0, 40, 300),
          (0.8, 0.2, 15, 0.6, 0, 0.0, 0.0, 40, 100), (0.8, 0.2, 15, 0.3, 0, 0.0, 0.0, 40, 400),
          (0.8, 0.2, 15, 0.3, 20, 0.0, 0.0, 80, 600), (0.8, 0.2, 15, 0.3, 50, 0.8, 0.1, 40, 600),
          (0.8, 0.3, 15, 0.2, 50, 0.0, 0.0, 80, 600), (0.8, 0.3, 15, 0.2, 50, 0.0, 0.0, 80, 600)]
TARGET_ALT, COLLISION, FORMATION, BOUNDARY, CTRL_FREQ, SUBSTEPS = 0.45, 0.2, 8.0, 15.0, 60, 4
CAUSES = ("altitude", "collision", "isolated", "boundary", "time")
PH_DYN, PH_GND, PH_DRAG, PH_DW, PH_ALL, PH_RK4 = 1, 2, 3, 4, 5, 6   # the Physics enum (BaseAviary.py:420-450)
DW_STEP = 0.05   # height difference of neighbouring drone indices under a downwash variant (`_stagger_heights`)

# one slot per env, cycled: the near-drone class three times (it is the one the flock comparisons are about)
CLASSES = ("oncow", "at1m", "ring", "spaced", "close", "far", "oncow", "trunc_altitude", "trunc_collision",
           "trunc_isolated", "trunc_boundary", "trunc_time", "levelup", "term", "oncow", "inherd")


def class_of(e):
    return CLASSES[e % len(CLASSES)]


def tick(mode):
    """One _computeTerminated call's advance of the spacing hold clock (term_call, oracle/ch_oracle.c)."""
    return 1.0 / 240 if mode == 0 else 1.0 / CTRL_FREQ


def _clear(xy, cows, others, cow_gap=0.05, drone_gap=0.3):
    """No cow within cow_gap (a drone exactly on a cow makes the reference itself NaN), no drone within drone_gap."""
    if np.min(np.linalg.norm(cows - xy, axis=1)) < cow_gap:
        return False
    return len(others) == 0 or np.min(np.linalg.norm(np.asarray(others) - xy, axis=1)) >= drone_gap


def _place_each(rng, nl, cows, draw):
    """nl drone positions, each redrawn until it is clear of the cows and of the drones placed so far."""
    out = []
    for i in range(nl):
        for _ in range(1000):
            xy = draw(i)
            if _clear(xy, cows, out):
                break
        else:
            raise RuntimeError("no free spot for a drone")
        out.append(xy)
    return np.array(out)


def _inherd(rng, nl, cows, herd_c):
    return _place_each(rng, nl, cows, lambda i: herd_c + rng.uniform(-1.5, 1.5, 2))


def _oncow(rng, nl, cows):
    def draw(i):
        r, a = rng.uniform(0.05, 1.4), rng.uniform(0, 2 * np.pi)
        return cows[rng.integers(len(cows))] + r * np.array([np.cos(a), np.sin(a)])
    return _place_each(rng, nl, cows, draw)


def _ring(rng, nl, centre, rad, even):
    ang = np.linspace(0, 2 * np.pi, nl, endpoint=False) + rng.uniform(0, 2 * np.pi) if even \
        else np.sort(rng.uniform(0, 2 * np.pi, nl))
    return centre + rad * np.stack([np.cos(ang), np.sin(ang)], 1)


def _line(rng, nl, cows, start, d):
    """Drones d apart along x with 2 cm of noise (the `spaced` layout), clear of the cows."""
    for _ in range(1000):
        xy = start + np.stack([np.arange(nl) * d, np.zeros(nl)], 1) + rng.normal(0, 0.02, (nl, 2))
        if all(_clear(p, cows, []) for p in xy):
            return xy
        start = start + rng.uniform(-0.1, 0.1, 2)
    raise RuntimeError("no free line")


def _window_spacing(rng, level):
    """A nearest-neighbour spacing well inside the level's window (levels 0, 1: desired +- tol; 5: the cattle one)."""
    L = LEVELS[level]
    half = L[5] * L[6] if level == 5 else L[0] * L[1]
    return 0.8 + rng.uniform(-0.4, 0.4) * half


def _short_of_hold(mode, level):
    """The spacing clock one tick short of the level's hold: the next in-window call reaches it."""
    hold, t = float(LEVELS[level][2]), tick(mode)
    c = hold - t
    return c if c + t >= hold else np.nextafter(c, np.inf)


def _terminating(rng, s, mode, level, nl, cows, herd_c):
    """Drone xy (and for level 5 the cows, for levels 0 / 1 the clock) that make _computeTerminated true at
    ``level``; level 7 has no terminating branch and gets the ring."""
    if level in (0, 1):
        s["clock"] = _short_of_hold(mode, level)
        return _line(rng, nl, cows, herd_c + rng.uniform(-1, 0, 2), _window_spacing(rng, level)), cows
    if level in (2, 3):   # drone centroid within approach_min of the herd centroid: a 0.5 m ring about it
        for _ in range(1000):
            xy = _ring(rng, nl, cows.mean(0) + rng.uniform(-0.1, 0.1, 2), 0.5, True)
            if all(_clear(p, cows, []) for p in xy):
                return xy, cows
        raise RuntimeError("no free ring")
    if level == 5:        # the herd inside a ring whose neighbours are 0.8 m apart
        rad = 0.4 / np.sin(np.pi / max(nl, 2))
        inr = rad * np.cos(np.pi / max(nl, 3))
        cows = herd_c + rng.uniform(-0.4, 0.4, cows.shape) * inr
        return _ring(rng, nl, herd_c, rad, True), cows
    # 4, 6 (and 7): every cow inside the drones' polygon
    reach = np.max(np.linalg.norm(cows - herd_c, axis=1))
    return _ring(rng, nl, herd_c, (reach + rng.uniform(0.3, 0.8)) / np.cos(np.pi / max(nl, 3)), True), cows


def _rest(s, i):
    """Drone i hovering at rest at the target altitude with a clean PID: zero action then leaves its xy unchanged."""
    for k in ("drone_vel", "drone_angv", "pid_last_rpy", "pid_int_pos", "pid_int_rpy", "last_rpm", "rpy_rates"):
        s[k][i] = 0
    s["drone_quat"][i] = (0, 0, 0, 1)
    s["drone_qlag"][i] = (0, 0, 0, 1)
    s["drone_pos"][i, 2] = TARGET_ALT


def _place(rng, s, cls, mode, level, m, low_z=None):
    nl = int(s["n"])
    herd_c = rng.uniform(-6, 6, 2)
    cows = herd_c + rng.uniform(-1.5, 1.5, (m, 2))   # _synthetic_layout's herd (tests/golden/make_golden.py)
    xy = None
    if cls == "oncow":
        xy = _oncow(rng, nl, cows)
    elif cls == "at1m":
        # cow 0 at rest at exactly representable coordinates, drone 0 exactly 1 m along x (dn == 1.0 bit for bit),
        # drone 1 at 1 - 2^-20 m along y (dn < 1 but dn + 1e-6 > 1); both drones at rest (zero action: at1m_mask)
        cows = cows - herd_c + np.array([2.0, 3.0]) + np.array([4.0, 0.0])   # the rest of the herd 4 m to the side
        cows[0] = (2.0, 3.0)
        s["cow_vel"][0] = 0
        xy = _inherd(rng, nl, cows, cows[1:].mean(0))
        xy[0] = (3.0, 3.0)
        _rest(s, 0)
        if nl > 1:
            xy[1] = (2.0, 4.0 - 2.0 ** -20)
            _rest(s, 1)
    elif cls == "ring":
        xy = _ring(rng, nl, herd_c, rng.uniform(1.0, 3.0), rng.random() < 0.5)
    elif cls == "spaced":
        d = _window_spacing(rng, level) if level in (0, 1, 5) else rng.uniform(0.5, 1.1)
        xy = _line(rng, nl, cows, herd_c + rng.uniform(-1, 0, 2), d)
        if level in (0, 1):
            s["clock"] = _short_of_hold(mode, level)
    elif cls == "close":
        xy = _place_each(rng, nl, cows, lambda i: cows.mean(0) + rng.normal(0, 0.6, 2))
    elif cls == "far":
        xy = herd_c + rng.uniform(-20, 20, (nl, 2))
    elif cls in ("term", "levelup"):
        xy, cows = _terminating(rng, s, mode, level, nl, cows, herd_c)
        if cls == "levelup":
            s["tally"] = LEVELS[level][8] - 1
    else:
        # `inherd` and the truncation causes, one at a time: drones inside the herd, 0.3 m or more apart, at the
        # target altitude, early in the episode -- then the one cause
        xy = _inherd(rng, nl, cows, herd_c)
        s["drone_pos"][:nl, 2] = TARGET_ALT + rng.uniform(-0.05, 0.05, nl)
        s["step_counter"] = SUBSTEPS * 10 if mode == 0 else 10
        if cls == "trunc_altitude":       # off by more than 60 %
            # (the low branch under a ground-effect variant: inside _groundEffect's clipped regime, half of
            # GND_EFF_H_CLIP above the ground, where the propeller height is held at the clip)
            s["drone_pos"][0, 2] = TARGET_ALT + (rng.uniform(0.35, 0.6) if rng.random() < 0.5 else
                                                 -0.35 if low_z is None else low_z - TARGET_ALT)
        elif cls == "trunc_collision":    # drone 1 within the 0.2 m threshold of drone 0
            for _ in range(1000):
                a = rng.uniform(0, 2 * np.pi)
                p = xy[0] + 0.1 * np.array([np.cos(a), np.sin(a)])
                if _clear(p, cows, xy[2:]):
                    break
            xy[1] = p
        elif cls == "trunc_isolated":     # the last drone more than 8 m from every other
            a = rng.uniform(0, 2 * np.pi)
            xy[nl - 1] = herd_c + 11.0 * np.array([np.cos(a), np.sin(a)])
        elif cls == "trunc_boundary":     # the formation as it is, its centroid beyond the 15 m mission boundary
            a = rng.uniform(0, 2 * np.pi)
            xy = xy + 17.0 * np.array([np.cos(a), np.sin(a)])
        elif cls == "trunc_time":
            # step_counter / ctrl_freq > episode_len.  CTDE counts simulation substeps and tests before it counts the
            # step: the first multiple of 4 past the limit.  MARL counts control steps and the wrapper's calls see the
            # step counted: the limit itself.
            limit = int(LEVELS[level][7]) * CTRL_FREQ
            s["step_counter"] = limit + SUBSTEPS if mode == 0 else limit
    s["drone_pos"][:nl, :2] = xy
    s["cow_pos"][:m] = cows


def _stagger_heights(s, cls):
    """Under a downwash variant: the live drones DW_STEP apart in height by index, about the target altitude.
    _downwash's force goes as 1 / dz^2 in the height difference of two drones, and the classes put drones 0.3 to
    1 m apart horizontally: at the heights the burn-in leaves, 1e-4 m apart and less, the reference itself
    diverges (vertical speeds of 1e2 to 1e33 m/s after one step) and nothing can be compared.  Centimetres apart
    the term is large and the reference resolves it.  Drone 0 of `trunc_altitude` keeps its out-of-range height."""
    nl = int(s["n"])
    for i in range(nl):
        if not (cls == "trunc_altitude" and i == 0):
            s["drone_pos"][i, 2] = TARGET_ALT + DW_STEP * (i - (nl - 1) / 2)


def directed_states(mode, n, m, level, E, seed, table, physics=0, compat=True, min_drones=None):
    """E oracle envs at directed states, and their state dicts (Env.get_state).  Env e is of class ``class_of(e)``.
    With ``min_drones`` < n the live drone count (``s["n"]``, ``active``) varies per env as the reset draws it."""
    import oracle as O
    rng = np.random.default_rng(seed)
    low_z = 0.5 * O.gnd_eff_h_clip() if physics in (PH_GND, PH_ALL) else None
    envs, states = [], []
    for e in range(E):
        env = O.Env(mode, n, m, table, min_drones=min_drones, max_drones=n, start_level=level, env_id=e,
                    compat=compat, physics=physics)
        env.reset()
        # burn-in: 2..7 random steps, the parity alternating within each class
        for t in range(2 + (e // len(CLASSES)) % 2 + 2 * int(rng.integers(0, 3))):
            env.step(rng.uniform(-1, 1, (n, 4)).astype(np.float32), autoreset=True)
        s = env.get_state()
        s["level"] = level
        _place(rng, s, class_of(e), mode, level, m, low_z)
        if physics in (PH_DW, PH_ALL):
            _stagger_heights(s, class_of(e))
        if mode == 1 and (e // len(CLASSES)) % 3 == 2 and int(s["n"]) > 2:
            s["active"][2] = 0   # an agent that terminated earlier in the episode
        env.set_state(s)
        envs.append(env)
        states.append(env.get_state())
    return envs, states


# (mode, n, m, level, kwargs of directed_states): what tests/test_gpu_directed.py steps, and so what the census of
# tests/test_directed_states_cpu.py covers.  Shapes first (one per flock path), then every level at 4 x 16 in both
# modes, then compat off per mode, a varying drone count, and the two term-table shapes (2 x 14 at 31 envs per workgroup: fused;
# 3 x 18 on a physics-variant handle at 20 envs per workgroup: unfused).
SHAPES = [(0, 4, 16, 7), (1, 4, 16, 0), (1, 4, 32, 0), (0, 8, 64, 7), (0, 3, 8, 0), (0, 6, 16, 6), (0, 12, 16, 7)]
TERM_TABLE_SHAPE = (0, 2, 14, 7)
UNFUSED_SHAPE, UNFUSED_PHYSICS = (0, 3, 18, 7), 3   # Physics.PYB_DRAG (BaseAviary.py:420-450)
CASES = [c + ({},) for c in SHAPES] + \
        [(mode, 4, 16, lvl, {}) for mode in (0, 1) for lvl in range(8) if (mode, 4, 16, lvl) not in SHAPES] + \
        [(0, 4, 16, 4, {"compat": False}), (1, 4, 16, 2, {"compat": False}), (0, 4, 16, 0, {"min_drones": 2}),
         TERM_TABLE_SHAPE + ({},), UNFUSED_SHAPE + ({"physics": UNFUSED_PHYSICS},)]
E_DIRECTED = 96


def case_id(c):
    mode, n, m, lvl, kw = c
    return f"{'ctde' if mode == 0 else 'marl'}-{n}x{m}-L{lvl}" + "".join(f"-{k}={v}" for k, v in kw.items())


def case_seed(c):
    mode, n, m, lvl, kw = c
    return 1000 * mode + 100 * n + m + 7 * lvl + 31 * len(kw)


def first_actions(states, n, seed):
    """Caller actions for the first step from directed states: uniform, but zero for the two resting drones of the
    `at1m` envs, whose distances to cow 0 must stay exact."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (len(states), n, 4)).astype(np.float32)
    for e in range(len(states)):
        if class_of(e) == "at1m":
            a[e, :2] = 0
    return a


def flock_runs(s):
    """The flock runs on the step from state s (every other step, BaseAviary.py:1352)."""
    return (int(s["step_counter_A"]) + 1) % 2 == 0


def pair_distances(s, m):
    """Cow-drone distances [n_live, m] of a state, as the flock forms them (drone minus cow, sqrt of squares)."""
    nl = int(s["n"])
    d = np.asarray(s["drone_pos"])[:nl, None, :2] - np.asarray(s["cow_pos"])[None, :m, :]
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def truncation_causes(pre, post, mode, m, ctor_level, active=None):
    """Each cause of _computeTruncated (CattleAviary.py:497-552) on its own, recomputed from the state the step's
    task saw (``post``, the positions after the physics; the step counter from ``pre``): a dict of bools.  With
    ``active`` (MARL: the agents' bits before the step) the per-drone causes count for active agents only, as the
    wrapper reports flags for those alone (marl_wrapper.py:104-113)."""
    nl = int(post["n"])
    act = np.ones(nl, bool) if active is None else np.asarray(active[:nl], bool)
    p = np.asarray(post["drone_pos"])[:nl]
    dd = np.linalg.norm(p[:, None, :2] - p[None, :, :2], axis=-1)
    off = ~np.eye(nl, dtype=bool)
    cows = np.asarray(post["cow_pos"])[:m]
    cent = np.linalg.norm(p[:, :2].mean(0) - cows.mean(0))
    counter = int(pre["step_counter"]) + (1 if mode == 1 else 0)
    return {"altitude": bool(np.any((np.abs(p[:, 2] - TARGET_ALT) > TARGET_ALT * 0.6) & act)),
            "collision": bool(np.any(((dd < COLLISION) & off)[act])),
            "isolated": bool(np.any([act[i] and np.all(dd[i][off[i]] > FORMATION) for i in range(nl)])),
            "boundary": bool(cent > BOUNDARY),
            "time": bool(counter / CTRL_FREQ > LEVELS[ctor_level][7])}


def term_calls(pre, mode):
    """_computeTerminated calls of one step (och_task, oracle/ch_oracle.c): CTDE the reward's nested call and the
    step's own; MARL env.step's reward and done passes over the live drones, then the wrapper's reward and done
    for every agent still active."""
    if mode == 0:
        return 2
    nl = int(pre["n"])
    return 2 * nl + 2 * int(np.asarray(pre["active"][:nl], int).sum())


def margins(pre, post, mode, m, ctor_level):
    """Relative distance |q - threshold| / threshold of every deciding quantity of the oracle's _computeTruncated
    and _computeTerminated (trunc_ctde / trunc_marl / term_call, oracle/ch_oracle.c) on one step, from oracle states
    alone: ``pre`` the state before the step (step counter, hold clock, level), ``post`` the state the step's task
    saw (``autoreset=False``: positions after the physics, level after the step).  A dict name -> smallest distance
    of that kind; a kind with no quantity on this step is absent.  The termination quantities are those of every
    level the env is at during the step (a level-up between two calls changes the test of the later ones)."""
    import oracle as O
    nl = int(post["n"])
    p = np.asarray(post["drone_pos"], np.float64)[:nl]
    cows = np.asarray(post["cow_pos"], np.float64)[:m]
    rel = lambda q, thr: float(np.min(np.abs(np.asarray(q, np.float64) - thr)) / thr)   # noqa: E731
    out = {"altitude": rel(np.abs(p[:, 2] - TARGET_ALT), TARGET_ALT * 0.6)}
    dd = np.linalg.norm(p[:, None, :2] - p[None, :, :2], axis=-1)[np.triu_indices(nl, 1)]
    if dd.size:
        out["collision"] = rel(dd, COLLISION)
        out["formation"] = rel(dd, FORMATION)
    cent = float(np.linalg.norm(p[:, :2].mean(0) - cows.mean(0)))
    out["boundary"] = rel(cent, BOUNDARY)
    counter = int(pre["step_counter"]) + (1 if mode == 1 else 0)
    out["time"] = rel(counter / CTRL_FREQ, float(LEVELS[ctor_level][7]))
    for lvl in range(int(pre["level"]), int(post["level"]) + 1):
        L = LEVELS[lvl]
        if lvl in (0, 1) and dd.size:
            up, lo = L[0] + L[0] * L[1], L[0] - L[0] * L[1]
            ms = float(dd.min())
            out["spacing"] = min(out.get("spacing", np.inf), rel(ms, up), rel(ms, lo))
            if lo < ms < up:   # the clock advances with every call of the step and is tested after each
                held = float(pre["clock"]) + tick(mode) * np.arange(1, term_calls(pre, mode) + 1)
                out["hold"] = min(out.get("hold", np.inf), rel(held, float(L[2])))
        elif lvl in (2, 3):
            out["approach"] = min(out.get("approach", np.inf), rel(cent, L[3]))
        elif lvl in (4, 5, 6):
            eff = O.effectiveness(cows, p[:, :2])
            out["eff"] = min(out.get("eff", np.inf), rel(eff, float(L[4])))
            if lvl == 5 and dd.size:
                up, lo = L[5] + L[5] * L[6], L[5] - L[5] * L[6]
                out["spacing"] = min(out.get("spacing", np.inf), rel(dd.min(), up), rel(dd.min(), lo))
    return out


def decision_margins(pre, post, mode, m, level):
    """The smallest relative distance of any deciding quantity of the step to its threshold (``margins``): a flag of
    an f32 kernel may differ from the oracle's only on a step where this is below the f32 budget, 1e-4."""
    return min(margins(pre, post, mode, m, level).values())


MARGIN = 1e-4
# Classes that `_place` puts on a threshold on purpose, per level of the case: at levels 0 and 1 `spaced`, `term` and
# `levelup` share one placement, `_short_of_hold` -- the hold clock one tick short, so that the step's first in-window
# call reaches the hold exactly (distance 0 by construction).  Only their "hold" distance may be below MARGIN.  The
# f32 kernel is still held to exact flags there: `hold_reached_in_f32` shows that the narrowed clock plus the narrowed
# tick is the hold itself in f32, so the flag does not hang on a rounding.
ON_THRESHOLD = {0: ("spaced", "term", "levelup"), 1: ("spaced", "term", "levelup")}


def hold_reached_in_f32(mode, level):
    """`_short_of_hold`'s clock narrowed to f32 plus the narrowed tick reaches the level's hold in f32 arithmetic."""
    c, t = np.float32(_short_of_hold(mode, level)), np.float32(tick(mode))
    return bool(np.float32(c + t) >= np.float32(LEVELS[level][2]))


# ---- the f32 cases of tests/test_gpu_f32_parity.py ----------------------------------------------------------------
# One f32 step from the directed batch, (mode, n, m, level, kwargs): the six physics variants at the driver's shape;
# downwash with more columns of drones, MARL, and 32 cows under a variant (ch_create's v1 route); PYB shapes the f32
# path is not compared at elsewhere (per-wave tables at block 128, 12 drones, 64 % N != 0, a varying drone count,
# compat off, two drones).
F32_STEP_CASES = [(0, 4, 16, 7, {"physics": p}) for p in range(1, 7)] + \
                 [(0, 6, 8, 7, {"physics": 4}), (1, 4, 16, 0, {"physics": 5}), (1, 3, 8, 0, {"physics": 1}),
                  (0, 4, 32, 7, {"physics": 5}),
                  (0, 8, 64, 7, {}), (0, 12, 16, 7, {}), (0, 3, 8, 0, {}), (0, 4, 16, 0, {"min_drones": 2}),
                  (0, 4, 16, 4, {"compat": False}), (0, 2, 8, 7, {})]

# Lockstep f32 rollouts with auto-reset, (physics, mode, n, m): 16 envs, 120 steps.  CTDE starts at curriculum level
# 2 (terminates on approach, 40 s episodes); MARL at level 0 with `rollout_start`'s placement.
ROLLOUT_CASES = [("pyb", 0, 4, 16), ("pyb", 1, 4, 16), ("dyn", 0, 4, 16), ("pyb_gnd_drag_dw", 0, 4, 16),
                 ("dyn_rk4", 0, 2, 8), ("pyb", 0, 4, 32)]
ROLLOUT_E, ROLLOUT_T = 16, 120
# env_id_offset per case: the first for which the oracle, free-running in f64 from the same resets with the same
# Philox actions, has no env-step within MARGIN of a threshold and ends episodes after the first ten steps
# (tests/test_directed_states_cpu.py::test_rollout_reference_keeps_its_margins)
ROLLOUT_OFFSET = {c: 0 for c in ROLLOUT_CASES}


def rollout_level(mode):
    return 2 if mode == 0 else 0


def rollout_start(s, mode, n):
    """The start of a lockstep rollout on a stacked state dict right after the reset.  MARL: an episode ends only
    when every agent has terminated (marl_wrapper.py:113-117), so half the envs start with their drones 0.8 m apart
    and the level-0 spacing clock short of its 10 s hold, as test_random_rollout_with_autoreset_vs_oracle does --
    here 3.5 ticks short instead of 3, so that no call's clock lands on the hold itself (a deciding quantity on
    its threshold by construction would be excused in f32, and the rollout's flags are to be exact), and two
    more steps' worth of calls short from one such env to the next, so that the episodes end on steps 0, 2, ..
    and some resets fall after the first ten steps."""
    if mode == 1:
        E = len(s["clock"])
        ev = np.arange(E) % 2 == 0
        s["drone_pos"][ev, :n, 0] = 0.8 * np.arange(n)[None, :]
        s["drone_pos"][ev, :n, 1] = 0.0
        s["clock"][ev] = 10.0 - (3.5 + 2 * 4 * n * (np.arange(E)[ev] // 2)) / CTRL_FREQ
    return s


def rollout_id(c):
    ph, mode, n, m = c
    return f"{ph}-{'ctde' if mode == 0 else 'marl'}-{n}x{m}"


def neighbour_blocks(xy, i, margin=MARGIN):
    """Every neighbour block of drone i's observation row (columns 10-13: the float32 offsets of its two nearest
    drones in order of distance, obs_row in oracle/ch_oracle.c) that the oracle's own distances allow when two
    distances within ``margin`` relative of each other count as tied.  More than one block: the order hangs on a
    rounding -- the reset line, where a middle drone has both neighbours at exactly 1.75 m, or a regular ring."""
    xy = np.asarray(xy, np.float64)
    others = [j for j in range(len(xy)) if j != i]
    d = {j: float(np.hypot(*(xy[j] - xy[i]))) for j in others}
    out = []
    for a in [j for j in others if d[j] <= min(d.values()) * (1 + margin)] if others else []:
        rest = [j for j in others if j != a]
        if not rest:
            out.append((a,))
        for b in [j for j in rest if d[j] <= min(d[k] for k in rest) * (1 + margin)]:
            out.append((a, b))
    blocks = []
    for pick in out:
        blk = np.zeros(4, np.float32)
        for k, j in enumerate(pick):
            blk[2 * k:2 * k + 2] = (xy[j] - xy[i]).astype(np.float32)
        blocks.append(blk)
    return blocks


def untie_neighbours(o, ro, n_live, pos_of):
    """The oracle's observations ``ro`` [E, rows, 86] with the neighbour block of every row that differs from the
    device's ``o`` replaced by the tied ordering (``neighbour_blocks``) nearest to the device's, where the oracle's
    positions after the step (``pos_of(e)`` -> [n, 3]) allow more than one; and the number of rows replaced.  A row
    without a tie is left as it is, so a wrong neighbour still fails the comparison that follows."""
    ro = ro.copy()
    bad = ~np.isclose(o[..., 10:14], ro[..., 10:14], rtol=1e-4, atol=1e-6).all(-1)
    count = 0
    for e, i in np.argwhere(bad):
        if i >= int(n_live[e]):
            continue
        blocks = neighbour_blocks(np.asarray(pos_of(e))[:int(n_live[e]), :2], int(i))
        if len(blocks) > 1:
            ro[e, i, 10:14] = min(blocks, key=lambda blk: float(np.abs(blk - o[e, i, 10:14]).max()))
            count += 1
    return ro, count
