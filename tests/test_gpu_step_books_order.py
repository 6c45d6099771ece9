"""The pipelined step loop's books (csrc/ch_step_body.h, k_step2_multi<double, 0, 16, 4, 16>): the env scalars go back
ahead of the reward (P_B), the books close behind it (P_K), the metric rows stay in LDS for the length of a launch and
the two constant tables are staged once per launch.  ch_step_n(n) against n plain ch_step launches from the same raw
state, bit for bit: outputs, state (envi / envr included), metrics, episode records and, where they are drawn, the
actions.  Every comparison ends with sync() on both handles, which raises if a hand-off wait expired.

States: tests/directed_states.py's batch with the ending classes delayed to the second step as in
tests/test_gpu_step_reset_order.py (the first step after set_state is always a plain launch, so the second step is
the first one of the ch_step_n launch), and on top of that a schedule of endings inside the launch, per 16-env
workgroup (`scheduled_states`; the step index counts from the plain launch = 0, the launch covers 1..n):
  term, trunc_boundary, trunc_time   end on step 1, the launch's first step (levelup changes level there)
  ring            the time limit on step 2
  close           the time limit on step 3 (with the two above: endings on consecutive steps, both step parities, so
                  both drone waves close books with an episode end)
  inherd          the time limit on the launch's last step n
  trunc_time      ends on step 1 at the time limit, and again inside a launch of 64: its drones are commanded towards
                  each other in pairs at full speed, so every new episode ends in a collision some 36 steps after its
                  reset (steps 38 and 74 on the oracle) -- the env's running return / length rows are zeroed and closed
                  a second time inside one launch, by the other drone wave (steps 1 and 38: both parities)
test_schedule_on_oracle checks the schedule on the CPU oracle alone; the GPU tests assert it again from the plain
handle's flags.  The metric rows are compared per env and per row (ch__metric_rows, the raw [rows][E] table), beside the
public sums and `episode_stats`.

Shapes: f64 CTDE 4 x 16 at 16 envs (one workgroup), 24 (a half-filled second workgroup) and 48.
"""
import ctypes

import numpy as np
import pytest

import directed_states as D
import step_rows as SR
from helpers import stack

LEVEL = 0
SEED = 4242
INSIDE = 0.004
N, M = 4, 16
LIMIT = int(D.LEVELS[LEVEL][7]) * D.CTRL_FREQ   # the time limit in substeps' units: truncates once step_counter > LIMIT
SHAPES = (16, 24, 48)


def _table(m):
    import torch  # noqa: F401  (before the library, as HerdBatch loads them: one HIP runtime for both in this process)
    from cattleherd._lib import spawn_table
    return spawn_table(m)


def _time_limit_on(step):
    """step_counter (CTDE: simulation substeps, tested before the step is counted) that truncates on step `step` >= 1."""
    return LIMIT - D.SUBSTEPS * (step - 1)


def scheduled_states(E, steps, min_drones=None):
    """Oracle envs and states of the module docstring's schedule for a launch of `steps` steps."""
    envs, states = D.directed_states(0, N, M, LEVEL, E, SEED, _table(M), min_drones=min_drones)
    hold = float(D.LEVELS[LEVEL][2])
    for e, env in enumerate(envs):
        s, cls = states[e], D.class_of(e)
        nl = int(s["n"])
        if cls in ("term", "levelup", "spaced"):
            s["clock"] = hold - 2.5 * D.tick(0)
        elif cls == "trunc_time":
            s["step_counter"] = _time_limit_on(1)
        elif cls == "trunc_boundary":
            for i in range(nl):
                D._rest(s, i)
            cows = np.asarray(s["cow_pos"])[:M]
            xy = np.asarray(s["drone_pos"])[:nl, :2]
            d = xy.mean(0) - cows.mean(0)
            u = d / np.linalg.norm(d)
            s["drone_pos"][:nl, :2] = xy + (D.BOUNDARY - INSIDE - np.linalg.norm(d)) * u
            s["cow_vel"][:M] = -0.2 * u
        elif cls == "ring":
            s["step_counter"] = _time_limit_on(2)
        elif cls == "close":
            s["step_counter"] = _time_limit_on(3)
        elif cls == "inherd":
            s["step_counter"] = _time_limit_on(max(steps, 1))
        env.set_state(s)
        states[e] = env.get_state()
    return envs, states


def _actions(E):
    a = (0.05 * np.random.default_rng(11).uniform(-1, 1, (E, N, 4))).astype(np.float32)
    for e in range(E):
        cls = D.class_of(e)
        if cls in ("trunc_boundary", "at1m"):
            a[e] = 0
        elif cls == "trunc_time":
            a[e] = [(1, 0, 0, 1), (-1, 0, 0, 1)] * (N // 2)   # neighbours fly at each other
    return a


def _ended_schedule(ended, steps):
    """ended [steps + 1, E] (step 0 = the plain launch): the docstring's schedule, in the first workgroup."""
    cls = np.array([D.class_of(e) for e in range(ended.shape[1])])
    wg = np.arange(ended.shape[1]) < 16
    at = lambda c, t: bool(ended[t][wg & (cls == c)].all())   # noqa: E731
    assert at("term", 1) and at("trunc_time", 1) and at("trunc_boundary", 1), "no ending on the launch's first step"
    if steps >= 2:
        assert at("ring", 2)
    if steps >= 3:
        assert at("close", 3)
    assert at("inherd", steps), "no ending on the launch's last step"
    if steps >= 64:
        twice = ended[1:, wg & (cls == "trunc_time")].reshape(steps, -1)[:, 0]
        when = np.nonzero(twice)[0] + 1
        assert len(when) >= 2, "no env ends twice inside the launch"
        assert len({int(t) % 2 for t in when}) == 2, "its endings fall on one step parity"


@pytest.mark.parametrize("steps", (1, 2, 3, 8, 23, 64))
def test_schedule_on_oracle(steps):
    """The CPU oracle alone: the endings fall where the docstring says."""
    E = 16
    envs, _ = scheduled_states(E, steps)
    acts = _actions(E)
    ended = np.zeros((steps + 1, E), bool)
    for t in range(steps + 1):
        for e, env in enumerate(envs):
            out = env.step(acts[e], autoreset=True)
            ended[t, e] = bool(np.any(out[2]) or np.any(out[3]))
    _ended_schedule(ended, steps)


# ch_step_n's row per geometry of this file: the pipelined one, none under its minimum block, the unpipelined 8-env one
MULTI_ROW = {(16, 512): "k_step2_multi<double,0,16,4,16>", (16, 192): None, (8, 512): "k_step2_multi<double,0,8,4,16>"}


def _pair(E, geom, **kw):
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    kw.setdefault("min_drones", N)
    hs = [HerdBatch(E, N, M, mode="ctde", curriculum_level=LEVEL, max_drones=N, **kw) for _ in range(2)]
    # the first handle runs ch_step_n on the multi-step kernel's geometry, the second plain steps on the default one
    assert _lib.lib().ch__set_geometry(hs[0].handle, ctypes.c_int32(geom[0]), ctypes.c_int32(geom[1])) == 0
    assert SR.held_names(hs[0])["multi_row"] == MULTI_ROW[geom], (geom, SR.held_names(hs[0]))
    assert SR.held_names(hs[0])["step_row"] == f"k_step2<double,0,{geom[0]},4,16>"
    return hs


def _multi(h):
    from cattleherd import _lib
    return _lib.lib().ch__multi_steps(h.handle)


def _metric_rows(h):
    """The per-env metric rows [rows, E] (the public sums' inputs, then the open episode's return and length)."""
    from cattleherd import _lib
    rows = len(_lib.METRIC_NAMES) + 2
    out = np.zeros((rows, h.n_envs), np.float64)
    f = _lib.lib().ch__metric_rows
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    assert f(h.handle, out.ctypes.data, h._stream()) == 0
    return out


def _assert_same(a, b, what=""):
    import torch
    torch.cuda.synchronize()
    names = ("obs", "reward", "terminated", "truncated", "reset_happened", "agent_active", "episode_stats")
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(torch.nan_to_num(x.double(), nan=7.0), torch.nan_to_num(y.double(), nan=7.0)), (what, k)
    (da, ia), (db, ib) = a.get_state_raw(), b.get_state_raw()
    assert np.array_equal(ia, ib), (what, "envi")
    assert np.array_equal(da, db, equal_nan=True), (what, "state reals")
    ra, rb = _metric_rows(a), _metric_rows(b)
    for r in range(len(ra)):
        assert np.array_equal(ra[r], rb[r], equal_nan=True), (what, "metric row", r)
    assert ra[0].min() > 0, "an env without a counted step"
    assert np.array_equal(a.metrics(), b.metrics(), equal_nan=True), (what, "metrics")
    for h in (a, b):
        h.sync()   # raises on a device error (an expired hand-off wait)


def _start(E, steps, geom=(16, 512), min_drones=None):
    """A pair of handles at the scheduled state, one plain step done on both (it writes the observation blocks in full)."""
    import torch
    _, states = scheduled_states(E, steps, min_drones=min_drones)
    s = stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states])
    a, b = _pair(E, geom, **({} if min_drones is None else {"min_drones": min_drones}))
    act = torch.tensor(_actions(E), device=a.device)
    for h in (a, b):
        h.reset()
        h.set_state(s)
        h.step(act, random_actions=False, autoreset=True, terminal_obs=False)
    return a, b, act


def _plain(b, act, steps, E):
    """`steps` plain launches on b; per step whether each env's episode ended, its level and NUM_DRONES after it."""
    import torch
    ended, level, nd = np.zeros((steps + 1, E), bool), np.zeros((steps + 1, E), int), np.zeros((steps + 1, E), int)
    g = b.env_ints()
    level[0], nd[0] = g["level"], g["n"]
    for t in range(1, steps + 1):
        b.step(act, random_actions=False, autoreset=True, terminal_obs=False)
        torch.cuda.synchronize()
        ended[t] = (b.terminated.cpu().numpy().reshape(E, -1).any(1) | b.truncated.cpu().numpy().reshape(E, -1).any(1))
        g = b.env_ints()
        level[t], nd[t] = g["level"], g["n"]
    return ended, level, nd


@pytest.mark.gpu
@pytest.mark.parametrize("steps", (1, 2, 3, 8, 23, 64))
@pytest.mark.parametrize("E", SHAPES)
def test_metrics_carried_in_lds(E, steps):
    """Episodes end on the first, on consecutive and on the last step of the launch, at both step parities, and (n = 64)
    twice in one env, once on each drone wave; n = 23 also crosses the level change of step 1, so the reward reads another row of the curriculum
    table late in the launch (the constant tables are staged once)."""
    a, b, act = _start(E, steps)
    m0 = _multi(a)
    a.step_n(steps, actions=act, autoreset=True, random_actions=False)
    ended, level, _ = _plain(b, act, steps, E)
    # every step of the launch ran inside the multi-step kernel (so its LDS, the metric rows included, fits the launch check)
    assert _multi(a) - m0 == steps
    _ended_schedule(ended, steps)
    cls = np.array([D.class_of(e) for e in range(E)])
    assert (level[1][cls == "levelup"] == LEVEL + 1).all() and (level[0][cls == "levelup"] == LEVEL).all()
    _assert_same(a, b)
    for h in (a, b):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reset", (False, True))
@pytest.mark.parametrize("E", SHAPES)
def test_two_launches_back_to_back(E, reset):
    """ch_step_n(5) then ch_step_n(4), with nothing or with a host-side metrics reset between them, against 9 plain
    steps with the same reset at the same point: the second launch's step 0 reads the global rows again."""
    a, b, act = _start(E, 8)
    m0 = _multi(a)
    a.step_n(5, actions=act, autoreset=True, random_actions=False)
    for _ in range(5):
        b.step(act, random_actions=False, autoreset=True, terminal_obs=False)
    if reset:
        assert np.array_equal(a.metrics(reset=True), b.metrics(reset=True), equal_nan=True)
    a.step_n(4, actions=act, autoreset=True, random_actions=False)
    for _ in range(4):
        b.step(act, random_actions=False, autoreset=True, terminal_obs=False)
    assert _multi(a) - m0 == 9
    _assert_same(a, b)
    if reset:
        assert a.metrics()[0] == 4 * E   # "steps": only the second launch's
    for h in (a, b):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("E", SHAPES)
def test_env_scalars_every_prefix(E):
    """A level-up, a time-limit truncation and NUM_DRONES changes in both directions inside one launch (min_drones 2:
    every auto-reset draws the count anew): the whole state after every prefix n = 1..6, since step k's write-back is
    what step k+1's cow waves load."""
    census = None
    for steps in range(1, 7):
        a, b, act = _start(E, 6, min_drones=2)
        m0 = _multi(a)
        a.step_n(steps, actions=act, autoreset=True, random_actions=False)
        ended, level, nd = _plain(b, act, steps, E)
        assert _multi(a) - m0 == steps
        _assert_same(a, b, what=f"prefix {steps}")
        census = (ended, level, nd)
        for h in (a, b):
            h.close()
    ended, level, nd = census
    cls = np.array([D.class_of(e) for e in range(E)])
    assert (level[1][cls == "levelup"] == LEVEL + 1).all()
    assert ended[1][cls == "trunc_time"].all() and ended[2][cls == "ring"].all() and ended[6][cls == "inherd"].all()
    # (nd[0] is the count after the plain launch: every change below happens inside the ch_step_n launch.  On the
    # oracle the first workgroup alone has `spaced` going from 2 to 4 drones and `close` from 3 to 2.)
    assert (np.diff(nd, axis=0) > 0).any() and (np.diff(nd, axis=0) < 0).any(), \
        "NUM_DRONES does not change in both directions"


@pytest.mark.gpu
@pytest.mark.parametrize("E,steps", [(16, 2), (24, 8), (48, 23)])
def test_drawn_actions(E, steps):
    """The same comparison with the actions drawn on the device, the drawn actions included."""
    import torch
    a, b, _ = _start(E, steps)
    for h in (a, b):
        for _ in range(20):
            h.step(random_actions=True, autoreset=True, terminal_obs=False)
    m0 = _multi(a)
    a.step_n(steps, random_actions=True)
    for _ in range(steps):
        b.step(random_actions=True, autoreset=True, terminal_obs=False)
    assert _multi(a) - m0 == steps
    _assert_same(a, b)
    assert torch.equal(a.actions, b.actions)
    for h in (a, b):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geom,multi", [((16, 192), False), ((8, 512), True)])
def test_fallback_geometry(geom, multi):
    """Below the pipelined instantiation's minimum (a 192-thread block: ch_step_n falls back to one k_step2 launch per
    step) and at 8 envs per workgroup (the unpipelined k_step2_multi): the other instantiations of the shared body."""
    E, steps = 24, 8
    a, b, act = _start(E, steps, geom=geom)
    m0 = _multi(a)
    a.step_n(steps, actions=act, autoreset=True, random_actions=False)
    ended, _, _ = _plain(b, act, steps, E)
    assert _multi(a) - m0 == (steps if multi else 0)
    assert ended[1:].any()
    _assert_same(a, b)
    for h in (a, b):
        h.close()
