"""The drone wave's reordered post-D section (csrc/ch_step_body.h: the reset decision's inputs ahead of the cow items'
hand-off H, the reward behind the reset list R): ch_step_n against plain ch_step launches bit for bit at every CTDE
instantiation of k_step2_multi and at MARL 4 x 32, and plain ch_step against the fp64 oracle.

States: tests/directed_states.py's batch (16 classes, one per env of a 16-env workgroup), with the ending classes
delayed by one step.  A handle's first step after set_state is always a plain launch (it writes the observation blocks
in full), so an episode that ends on that step never reaches the multi-step kernel; `delayed_states` moves each ending
to the second step, the first one of the ch_step_n launch, where all four outcomes then meet in one workgroup:
  term, levelup   the hold clock 2.5 ticks short of the hold (two _computeTerminated calls per step, one tick each: the
                  first call of the second step reaches it, the second call terminates; `levelup` leaves level 0 on the
                  first call, so its second call, at level 1's longer hold, does not terminate)
  trunc_time      the step counter one step short of the first value past the time limit
  trunc_boundary  the drones at rest under a zero action, 4 mm inside the mission boundary, and the herd walking away
                  from them at the cattle speed, 3.3 mm a step: inside after one step, outside after two
  the rest        as directed_states leaves them: the other truncating classes end on the plain launch, the near-herd
                  classes neither terminate nor truncate
test_delayed_states_on_oracle checks that schedule on the CPU oracle alone; the GPU tests assert it again from the
single-step handle's flags, level and tally.

Shapes: 16 envs (one workgroup), 24 (a second workgroup with 8 live env slots), 48; n = 1 (the second drone wave idle),
2, 3 and 23.  The oracle comparison uses the f64 bars of tests/test_gpu_directed.py: reward rtol 1e-6 / atol 1e-6,
flags, level and tally exact.
"""
import ctypes
import functools

import numpy as np
import pytest

import directed_states as D
import step_rows as SR
from helpers import close, oracle_view, stack

LEVEL = 0
SEED = 4242
INSIDE = 0.004   # trunc_boundary: the centroid distance starts this far inside the 15 m boundary


def _table(m):
    import torch  # noqa: F401  (before the library, as HerdBatch loads them: one HIP runtime for both in this process)
    from cattleherd._lib import spawn_table
    return spawn_table(m)


def delayed_states(mode, n, m, E, compat=True):
    """Directed oracle envs at level 0 whose ending classes end on the second step (module docstring)."""
    envs, states = D.directed_states(mode, n, m, LEVEL, E, SEED, _table(m), compat=compat)
    hold, limit = float(D.LEVELS[LEVEL][2]), int(D.LEVELS[LEVEL][7]) * D.CTRL_FREQ
    for e, env in enumerate(envs):
        s, cls = states[e], D.class_of(e)
        nl = int(s["n"])
        if cls in ("term", "levelup", "spaced"):
            # (`spaced` sits in the window one tick short of the hold like `term`: moved back with it.  MARL: 16
            # _computeTerminated calls a step with 4 agents, as tests/test_gpu_directed.py's _stagger counts them)
            s["clock"] = hold - (2.5 if mode == 0 else 16 * 3) * D.tick(mode)
        elif cls == "trunc_time":
            s["step_counter"] = limit if mode == 0 else limit - 1
        elif cls == "trunc_boundary":
            for i in range(nl):
                D._rest(s, i)
            cows = np.asarray(s["cow_pos"])[:m]
            xy = np.asarray(s["drone_pos"])[:nl, :2]
            d = xy.mean(0) - cows.mean(0)
            u = d / np.linalg.norm(d)
            s["drone_pos"][:nl, :2] = xy + (D.BOUNDARY - INSIDE - np.linalg.norm(d)) * u
            s["cow_vel"][:m] = -0.2 * u   # MAX_VEL_CATTLE (BaseAviary.py:579), every cow: the herd centroid moves with it
        env.set_state(s)
        states[e] = env.get_state()
    return envs, states


def _actions(E, n):
    """Small caller actions (the placed formations stay together); zero for the resting drones of trunc_boundary."""
    a = (0.05 * np.random.default_rng(11).uniform(-1, 1, (E, n, 4))).astype(np.float32)
    for e in range(E):
        if D.class_of(e) in ("trunc_boundary", "at1m"):
            a[e] = 0
    return a


def _check_outcomes(te, tr, level, tally, E):
    """te, tr [T, E] flags of steps 0 (the plain launch) and 1.. (the ch_step_n launch), level / tally [T + 1, E] before
    step 0 and after each step: in the first workgroup, on step 1, an env terminates with its tally advanced, one
    leaves level 0, one truncates at the boundary, one at the time limit, and one does neither; none of them ends on step 0."""
    cls = np.array([D.class_of(e) for e in range(E)])
    wg = np.arange(E) < 16
    late = np.isin(cls, ("term", "levelup", "trunc_boundary", "trunc_time"))
    assert not te[0][late].any() and not tr[0][late].any(), "a delayed episode ends on the plain launch"
    term = wg & (cls == "term")
    assert te[1][term].all() and (tally[2][term] == tally[1][term] + 1).all() and (level[2][term] == LEVEL).all()
    up = wg & (cls == "levelup")
    assert (level[1][up] == LEVEL).all() and (level[2][up] == LEVEL + 1).all() and (tally[2][up] == 0).all()
    assert ((level[2] != level[1]) & wg).sum() == 1, "the level advances once"
    assert tr[1][wg & (cls == "trunc_boundary")].all() and not te[1][wg & (cls == "trunc_boundary")].any()
    assert tr[1][wg & (cls == "trunc_time")].all() and not te[1][wg & (cls == "trunc_time")].any()
    assert (wg & ~te[1] & ~tr[1]).any(), "no env goes on"


def _boundary_is_the_cause(pre, post, e, m):
    """Env e's truncation on the step from `pre` to `post` (states of the task's view: no auto-reset) is the mission
    boundary alone."""
    c = D.truncation_causes(pre, post, 0, m, LEVEL)
    return c["boundary"] and not (c["altitude"] or c["collision"] or c["isolated"] or c["time"])


@pytest.mark.parametrize("mode,n,m,compat", [(0, 4, 16, True), (0, 2, 8, False)])
def test_delayed_states_on_oracle(mode, n, m, compat):
    """The CPU oracle alone: nothing ends on the first step, and on the second all four outcomes occur among the first
    16 envs, each truncation for its own cause."""
    E = 16
    envs, states = delayed_states(mode, n, m, E, compat=compat)
    acts = _actions(E, n)
    te, tr = np.zeros((2, E), bool), np.zeros((2, E), bool)
    level, tally = np.zeros((3, E), int), np.zeros((3, E), int)
    causes = {}
    for t in range(2):
        for e, env in enumerate(envs):
            pre = env.get_state()
            level[t, e], tally[t, e] = int(pre["level"]), int(pre["tally"])
            out = env.step(acts[e], autoreset=False)
            te[t, e], tr[t, e] = bool(np.any(out[2])), bool(np.any(out[3]))
            post = env.get_state()
            level[t + 1, e], tally[t + 1, e] = int(post["level"]), int(post["tally"])
            if t == 1:
                causes[e] = D.truncation_causes(pre, post, mode, m, LEVEL)
    _check_outcomes(te, tr, level, tally, E)
    for e in range(E):
        if D.class_of(e) == "trunc_boundary":
            assert causes[e] == dict(altitude=False, collision=False, isolated=False, boundary=True, time=False)
        if D.class_of(e) == "trunc_time":
            assert causes[e] == dict(altitude=False, collision=False, isolated=False, boundary=False, time=True)


# ch_step_n's row per (mode, drones, cattle, precision, geometry) of this file
MULTI_ROW = {(0, 4, 16, "f64", (16, 512)): "k_step2_multi<double,0,16,4,16>",
             (0, 2, 8, "f64", (16, 512)): "k_step2_multi<double,0,16,2,8>",
             (0, 4, 16, "f32", (16, 512)): "k_step2_multi<float,0,16,4,16>",
             (1, 4, 32, "f64", (16, 512)): "k_step2_multi<double,1,16,4,32,false,true>"}


def _pair(mode, n, m, E, geom, **kw):
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    hs = [HerdBatch(E, n, m, mode="ctde" if mode == 0 else "marl", curriculum_level=LEVEL, min_drones=n, max_drones=n,
                    **kw) for _ in range(2)]
    # the first handle runs ch_step_n on the multi-step kernel's geometry, the second plain steps on the default one
    assert _lib.lib().ch__set_geometry(hs[0].handle, ctypes.c_int32(geom[0]), ctypes.c_int32(geom[1])) == 0
    assert SR.held_names(hs[0])["multi_row"] == MULTI_ROW[(mode, n, m, kw.get("precision", "f64"), geom)], SR.held_names(hs[0])
    return hs


def _multi(h):
    from cattleherd import _lib
    return _lib.lib().ch__multi_steps(h.handle)


def _assert_same(a, b):
    import torch
    torch.cuda.synchronize()
    outs = [[x.clone() for x in (h.obs, h.reward, h.terminated, h.truncated, h.reset_happened, h.agent_active)] for h in (a, b)]
    for i, (x, y) in enumerate(zip(*outs)):
        assert torch.equal(torch.nan_to_num(x.float(), nan=7.0), torch.nan_to_num(y.float(), nan=7.0)), i
    (da, ia), (db, ib) = a.get_state_raw(), b.get_state_raw()
    assert np.array_equal(da, db, equal_nan=True) and np.array_equal(ia, ib)
    assert np.array_equal(a.metrics(), b.metrics(), equal_nan=True)
    for h in (a, b):
        h.sync()   # raises on a device error (an expired hand-off wait)


def _run(mode, n, m, E, steps, geom, check, compat=True, **kw):
    """set_state, one plain step, then `steps` steps in one ch_step_n launch against `steps` plain launches."""
    import torch
    _, states = delayed_states(mode, n, m, E, compat=compat)
    s = stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states])
    a, b = _pair(mode, n, m, E, geom, compat=compat, **kw)
    act = torch.tensor(_actions(E, n), device=a.device)
    T = steps + 1
    te, tr = np.zeros((T, E), bool), np.zeros((T, E), bool)
    level, tally = np.zeros((T + 1, E), int), np.zeros((T + 1, E), int)

    def note(t):
        torch.cuda.synchronize()
        te[t] = b.terminated.cpu().numpy().reshape(E, -1).any(1)
        tr[t] = b.truncated.cpu().numpy().reshape(E, -1).any(1)
        g = b.get_state()
        level[t + 1], tally[t + 1] = g["level"], g["tally"]
    for h in (a, b):
        h.reset()
        h.set_state(s)
    g = b.get_state()
    level[0], tally[0] = g["level"], g["tally"]
    for h in (a, b):
        h.step(act, random_actions=False, autoreset=True, terminal_obs=False)   # writes the observation blocks in full
    note(0)
    m0 = _multi(a)
    a.step_n(steps, actions=act, autoreset=True, random_actions=False)
    for t in range(1, T):
        b.step(act, random_actions=False, autoreset=True, terminal_obs=False)
        note(t)
    assert _multi(a) - m0 == steps   # every step of the launch ran inside the multi-step kernel
    if check:
        _check_outcomes(te, tr, level, tally, E)
    else:
        assert (te[1:] | tr[1:]).any(), "no episode ends inside the launch"
    _assert_same(a, b)
    for h in (a, b):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("steps", (1, 2, 3, 23))
@pytest.mark.parametrize("E", (16, 24, 48))
def test_step_n_equals_plain_steps_ctde_4x16(E, steps):
    """The pipelined instantiation (16 envs x 4 drones x 16 cattle, f64): two drone waves that alternate steps."""
    _run(0, 4, 16, E, steps, (16, 512), check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("steps", (1, 2, 3, 23))
def test_step_n_equals_plain_steps_ctde_2x8(steps):
    """2 drones x 8 cattle at 16 envs per workgroup, compat off (with two drones the reference's own reward is NaN in
    compat mode): the unpipelined k_step2_multi, whose env lanes read the per-drone terms back from LDS."""
    _run(0, 2, 8, 16, steps, (16, 512), check=True, compat=False)


@pytest.mark.gpu
@pytest.mark.parametrize("steps", (1, 2, 3, 23))
def test_step_n_equals_plain_steps_ctde_4x16_f32(steps):
    """The f32 instantiation of the 16 x 4 x 16 geometry (f64 positions and centroid beside the f32 state)."""
    _run(0, 4, 16, 16, steps, (16, 512), check=True, precision="f32")


@pytest.mark.gpu
def test_step_n_equals_plain_steps_marl_4x32():
    """MARL 4 x 32 (per-wave tables): its reward and terminated calls keep their order behind H; the env scalars and
    the centroid distance are read ahead of it as in CTDE.  8 steps."""
    _run(1, 4, 32, 16, 8, (16, 512), check=False)


@pytest.mark.gpu
@pytest.mark.parametrize("E,steps", [(16, 1), (24, 3), (48, 23)])
def test_step_n_drawn_actions_from_burnt_in_state(E, steps):
    """The directed cases above pass the caller's actions (a resting drone needs its zero action), so the drawn ones
    are compared here: the delayed batch burnt in with 140 device-drawn steps (episodes then end at their long-run
    rate, and the observation blocks are in place: no plain step first), then ch_step_n against plain steps with
    device-drawn actions -- outputs, state, metrics and the actions bit for bit."""
    import torch
    _, states = delayed_states(0, 4, 16, E)
    s = stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states])
    a, b = _pair(0, 4, 16, E, (16, 512))
    for h in (a, b):
        h.reset()
        h.set_state(s)
        for _ in range(140):
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


@functools.lru_cache(maxsize=None)
def _oracle_steps():
    """Three plain ch_step launches (no auto-reset) from the delayed batch, and the oracle's steps from the device state
    before each: computed once, shared, left unchanged."""
    import torch
    import oracle as O
    n, m, E = 4, 16, 16
    envs, states = delayed_states(0, n, m, E)
    from cattleherd.env import HerdBatch
    b = HerdBatch(E, n, m, mode="ctde", curriculum_level=LEVEL, min_drones=n, max_drones=n)
    b.reset()
    b.set_state(stack([{k: v for k, v in st.items() if k != "eval_dist"} for st in states]))
    acts = _actions(E, n)
    act = torch.tensor(acts, device=b.device)
    rows = []
    for t in range(3):
        g = b.get_state()
        for e, env in enumerate(envs):
            env.set_state(oracle_view(g, e, O.NMAX))
        b.step(act, random_actions=False, autoreset=False, terminal_obs=False)
        torch.cuda.synchronize()
        ref = [env.step(acts[e], autoreset=False) for e, env in enumerate(envs)]
        g1 = b.get_state()
        want = stack([env.get_state() for env in envs])
        rows.append(dict(reward=b.reward.cpu().numpy().reshape(E), te=b.terminated.cpu().numpy().reshape(E).astype(bool),
                         tr=b.truncated.cpu().numpy().reshape(E).astype(bool), level=np.asarray(g1["level"]),
                         tally=np.asarray(g1["tally"]), pre=g, post=g1,
                         want_reward=np.array([r[1][0] for r in ref], np.float32),
                         want_te=np.array([bool(np.any(r[2])) for r in ref]),
                         want_tr=np.array([bool(np.any(r[3])) for r in ref]),
                         want_level=want["level"], want_tally=want["tally"]))
    b.close()
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("t", (0, 1, 2))
def test_plain_step_vs_oracle(t):
    """The moved reward block itself: reward to the f64 bar of tests/test_gpu_directed.py (rtol 1e-6, atol 1e-6),
    terminated, truncated, level and tally exact, on each of three steps; on the second one the four outcomes, the
    boundary truncation for that cause alone."""
    r = _oracle_steps()[t]
    print("step", t, "max |reward - oracle|", float(np.nanmax(np.abs(r["reward"].astype(np.float64) - r["want_reward"]))))
    assert np.array_equal(r["te"], r["want_te"])
    assert np.array_equal(r["tr"], r["want_tr"])
    assert np.array_equal(r["level"], r["want_level"])
    assert np.array_equal(r["tally"], r["want_tally"])
    ok, worst = close(r["reward"], r["want_reward"], 1e-6, 1e-6)
    assert ok, worst
    if t == 1:
        cls = [D.class_of(e) for e in range(16)]
        assert r["te"][cls.index("term")] and r["tr"][cls.index("trunc_time")] and r["tr"][cls.index("trunc_boundary")]
        assert r["level"][cls.index("levelup")] == LEVEL + 1
        e = cls.index("trunc_boundary")
        pre, post = ({k: np.asarray(v[e]) for k, v in s.items()} for s in (r["pre"], r["post"]))
        assert _boundary_is_the_cause(pre, post, e, 16)
