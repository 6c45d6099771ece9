"""GPU tests of the explicit reset entry points: ch_reset with a mask and ch_reset_with (the k_env<..., RESET_ONLY>
instantiations of ch_kernels.hip), which every adapter starts from.

  a. a masked reset against the oracle's och_reset on exactly the masked envs, after 25 lockstep steps with
     auto-reset (episode counters and spawn indices differ between envs), twice; the other envs bit-equal to before
  b. step without auto-reset + reset(mask = done) equals the step's own auto-reset, bit for bit
  c. the episode books (episode_stats, EPISODES / RETURN_SUM / LENGTH_SUM) across an explicit reset against the
     numpy Monitor of tests/reset_ref.py: an explicit reset abandons the open episode, as SB3's Monitor.reset does
  d. the same through CattleHerdVecEnv's info["episode"] and train_log.EpisodeRing
  e. ch_reset_with: the mask, indexing by env, float32 storage, rejection of an invalid NUM_DRONES

Tolerances: f64 state rtol 1e-9, obs rtol 1e-6 / atol 1e-7 (tests/test_gpu_parity.py); cow_vel 1e-15
(test_reset_parity_and_spawn); f32 obs rtol 1e-4 / atol 1e-6 (test_f32_throughput_mode_error_budget); the return of
an episode within sum |r_i| 2^-24 of the Monitor's, which adds the float32 reward outputs where the device adds the
float64 rewards (derived: one float32 rounding per step).

What the f32 handle's tests can see: ch_get_state returns the f64 shadow positions (pos64, cpos64, prev64) in place of
the float32 position rows, which no step reads; those rows are held through the observations only.

ch_reset has no agent_active output (ch_step_io's is "after this step"); the adapters read the live agents of a
reset env from the state (marl_vec_env.refresh_agents).  "The live agents" below is therefore get_state()["active"];
in (b) the step's agent_active tensor of the auto-resetting handle equals the twin's state on every env, and the
twin's own tensor off the reset envs.

Largest errors observed on an MI355X: in each test's docstring.
"""
import ctypes

import numpy as np
import pytest

import reset_ref as R
from helpers import close, oracle_view, stack

pytestmark = pytest.mark.gpu

PERSIST = ("pid_last_rpy", "pid_int_pos", "pid_int_rpy", "prev_cent", "clock", "has_prev")   # kept in compat mode
DRONE_KEYS = ("drone_pos", "drone_quat", "drone_vel", "drone_angv", "pid_int_rpy", "pid_int_pos", "pid_last_rpy",
              "drone_qlag")
INT_KEYS = ("n", "step_counter", "step_counter_A", "episode", "spawn_index", "has_prev", "level", "tally")
# level 7: 80 s of 60 control steps.  The CTDE counter advances 4 per step and an env ends in the step it enters with
# the counter above the limit: from TIME_LIMIT - 4 x that is step x + 2
TIME_LIMIT = 4800


def _batch(mode, n, m, E, ctor_level, **kw):
    from cattleherd.env import HerdBatch
    return HerdBatch(E, n, m, mode="ctde" if mode == 0 else "marl", curriculum_level=ctor_level, **kw)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_bits(g, g0, rows, what):
    for k in g0:
        assert _bits(g[k][rows]) == _bits(g0[k][rows]), (what, k)


# ---- a. masked reset against the oracle -----------------------------------------------------------------------------
# name, mode, drones, cattle, level, batch kwargs, oracle kwargs; the team width of k_env (ch_create: 16 up to 16
# cattle, 32 up to 32, 64 above) is 16, 16, 32, 16, 64
MASKED_CASES = [
    ("ctde_4x16_f64", 0, 4, 16, None, {}, {}),
    ("ctde_4x16_f32", 0, 4, 16, None, {"precision": "f32"}, {}),
    ("marl_3x32_f64", 1, 3, 32, None, {}, {}),
    ("ctde_2x8_nocompat", 0, 2, 8, None, {"compat": False}, {"compat": False}),
    ("ctde_12x48_l7_draw", 0, 12, 48, 7, {"min_drones": 4, "max_drones": 12}, {"min_drones": 4, "max_drones": 12}),
]
E_MASKED = 130 + 1


def _masks(E, team, rng):
    """Two masks over E envs for workgroups of 64 / team envs: env 0 and env E - 1, every env of one workgroup,
    exactly one env of the next and none of the one after; elsewhere a random third.  The second mask uses other
    workgroups and shares envs with the first (their second explicit reset in a row of episodes)."""
    epb = 64 // team
    out = []
    for w in (3, 9):
        m = rng.random(E) < 0.33
        m[[0, E - 1]] = True
        m[w * epb:(w + 1) * epb] = True
        m[(w + 1) * epb:(w + 3) * epb] = False
        m[(w + 1) * epb + (epb > 1)] = True
        out.append(m)
    out[1][3 * epb] = True
    assert np.any(out[0] & out[1]) and np.any(out[0] & ~out[1]) and np.any(~out[0] & ~out[1])
    assert E % epb != 0 or epb == 1
    return out


def _lockstep(b, envs, steps, t0):
    """``steps`` random-action steps with auto-reset; before each the oracle envs take the device state."""
    import oracle as O
    import torch
    for t in range(t0, t0 + steps):
        g = b.get_state()
        for e, env in enumerate(envs):
            env.set_state(oracle_view(g, e, O.NMAX))
        b.step(random_actions=True, autoreset=True)
        torch.cuda.synchronize()
        acts = b.actions.cpu().numpy()
        dn = np.array([env.step(acts[e], autoreset=True)[4] for e, env in enumerate(envs)])
        assert np.array_equal(b.reset_happened.cpu().numpy().astype(bool), dn), t
    return t0 + steps


@pytest.mark.parametrize("name,mode,n,m,level,kw,okw", MASKED_CASES, ids=[c[0] for c in MASKED_CASES])
def test_masked_reset_vs_oracle_and_nothing_else_touched(name, mode, n, m, level, kw, okw):
    """Every team width ch_create can choose is run (16: 4x16, 2x8; 32: 3x32; 64: 12x48); E = 131 leaves the last
    workgroup partly filled at widths 16 and 32 (at 64 a workgroup is one env, so there is no such remainder).
    Observed: f64 obs and drone state equal to the oracle's (error 0), cow_vel <= 2.8e-17; f32 obs error 0, every
    cow_vel the float32 rounding of the oracle's (none of 2752 one ulp off), shadow positions exact."""
    import oracle as O
    import torch
    from cattleherd._lib import spawn_table
    E, f32, compat = E_MASKED, kw.get("precision") == "f32", kw.get("compat", True)
    table = spawn_table(m)
    b = _batch(mode, n, m, E, level, **kw)
    b.reset()
    envs = [O.Env(mode, n, m, table, env_id=e, start_level=level, **okw) for e in range(E)]
    for env in envs:
        env.reset()
    # episodes that end at different steps of the run-in, so that episode counters and spawn indices diverge: CTDE
    # close to the time limit; MARL (whose episodes do not end on truncation) with the drones 0.8 m apart and the
    # level-0 spacing clock close to its 10 s hold, as tests/test_gpu_parity.py rigs it
    ev = np.arange(E) % 2 == 0
    if mode == 0:
        b.set_state({"step_counter": np.where(ev, TIME_LIMIT - 4 * (np.arange(E) % 11), 0)})
    else:
        s = b.get_state()
        s["drone_pos"][ev, :, 0] = 0.8 * np.arange(n)[None, :]
        s["drone_pos"][ev, :, 1] = 0.0
        s["clock"][ev] = 10.0 - (1 + np.arange(E)[ev] % 5) / 60
        b.set_state({"drone_pos": s["drone_pos"], "clock": s["clock"]})
    t = _lockstep(b, envs, 25, 0)
    ep = b.get_state()["episode"]
    assert ep.min() == 1 and ep.max() >= 2, np.bincount(ep)
    width = 16 if m <= 16 else 32 if m <= 32 else 64
    worst = {}
    for r, mask in enumerate(_masks(E, width, np.random.default_rng(len(name)))):
        if r:
            t = _lockstep(b, envs, 3, t)
        g0, obs0 = b.get_state(), b.obs.cpu().numpy().copy()
        for e, env in enumerate(envs):
            env.set_state(oracle_view(g0, e, O.NMAX))
        b.reset(mask=torch.from_numpy(mask))
        torch.cuda.synchronize()
        want_obs = np.stack([envs[e].reset() for e in np.nonzero(mask)[0]])
        want = stack([envs[e].get_state() for e in np.nonzero(mask)[0]])
        g, obs = b.get_state(), b.obs.cpu().numpy()
        # the other envs: state and observation blocks bit-equal to before
        _same_bits(g, g0, ~mask, "unmasked")
        assert _bits(obs[~mask]) == _bits(obs0[~mask])
        # the masked envs against the oracle
        gm = {k: v[mask] for k, v in g.items()}
        ok, worst["obs"] = close(obs[mask], want_obs, *((1e-4, 1e-6) if f32 else (1e-6, 1e-7)))
        print(name, "reset", r, "envs", int(mask.sum()), "obs max err", worst["obs"])
        assert ok
        for k in INT_KEYS:
            assert np.array_equal(gm[k], want[k]), k
        assert np.all(gm["step_counter"] == 0) and np.all(gm["step_counter_A"] == 0)
        assert np.array_equal(gm["episode"], g0["episode"][mask] + 1)
        assert np.array_equal(gm["spawn_index"], (g0["spawn_index"][mask] + 1) % table.shape[0])
        assert np.array_equal(gm["active"], want["active"][:, :n])            # the live agents of the new episode
        assert np.array_equal(gm["active"], np.arange(n)[None, :] < gm["n"][:, None])
        if "min_drones" in kw:
            assert len(np.unique(g["n"])) > 2, np.bincount(g["n"])             # the NUM_DRONES draw really varies
        assert np.array_equal(gm["cow_pos"], want["cow_pos"][:, :m])           # f32: the f64 shadow, from the table
        assert np.array_equal(gm["cow_pos"], table[gm["spawn_index"], :m])
        if f32:
            assert np.array_equal(gm["drone_pos"], want["drone_pos"][:, :n])   # multiples of 1.75, the f64 shadow
            for k in ("drone_quat", "drone_vel", "drone_angv", "drone_qlag"):
                assert np.array_equal(gm[k], want[k][:, :n]), k
            cv, w32 = gm["cow_vel"], want["cow_vel"][:, :m].astype(np.float32)
            assert np.array_equal(cv, cv.astype(np.float32))                   # held as float32
            c32 = cv.astype(np.float32)
            near = (c32 == w32) | (c32 == np.nextafter(w32, np.float32(1))) | (c32 == np.nextafter(w32, np.float32(-1)))
            print(name, "cow_vel not the oracle's own float32 rounding:", int((c32 != w32).sum()), "of", c32.size)
            assert near.all()
        else:
            for k in DRONE_KEYS:
                ok, worst[k] = close(gm[k], want[k][:, :n], 1e-9, 1e-12)
                assert ok, (k, worst[k])
            ok, worst["cow_vel"] = close(gm["cow_vel"], want["cow_vel"][:, :m], 1e-15, 1e-15)
            assert ok, worst["cow_vel"]
            hp = gm["has_prev"] == 1
            assert close(gm["prev_cent"][hp], want["prev_cent"][hp], 1e-9, 1e-12)[0]
            assert close(gm["clock"], want["clock"], 1e-9, 1e-12)[0]
            print(name, "reset", r, "state max err", {k: v for k, v in worst.items() if k != "obs"})
        # what a reset keeps in compat mode (the reference creates its controllers and prev_cent_dists once) is
        # bit-equal to before; without compat it is zero
        for k in PERSIST:
            if compat:
                assert _bits(gm[k]) == _bits(g0[k][mask]), k
            else:
                assert not np.any(gm[k]), k
    b.close()


# ---- b. explicit reset of done envs equals auto-reset ---------------------------------------------------------------
TWIN_CASES = [("ctde_f64", 0, 4, 16, "f64", 2), ("ctde_f32", 0, 4, 16, "f32", 2), ("marl_f64", 1, 4, 32, "f64", 2),
              ("ctde_f64_v1", 0, 4, 16, "f64", 1)]


@pytest.mark.parametrize("name,mode,n,m,precision,kernel", TWIN_CASES, ids=[c[0] for c in TWIN_CASES])
def test_explicit_reset_of_done_envs_equals_autoreset(name, mode, n, m, precision, kernel):
    """Twin handles, the same given actions: A steps with auto-reset; B steps without and then resets the envs that
    ended.  State, observations, live agents, metrics and episode_stats agree bit for bit after every step.  At the
    start of the compared window a third of the envs is put close to an end (both handles alike), on top of the ends
    random actions bring, so that resets fall on many different steps.
    Observed: 31 resets on 29 steps of the window (CTDE f64, both kernels), 29 on 25 (f32), 17 on 2 (MARL); no bit
    differs."""
    import torch
    from cattleherd import _lib
    E, burn, T = 48, 140, 60
    hs = [_batch(mode, n, m, E, None, precision=precision) for _ in range(2)]
    rng = np.random.default_rng(41)
    for h in hs:
        if kernel == 1:
            assert _lib.lib().ch__set_kernel(h.handle, ctypes.c_int32(1)) == 0
        h.reset()
    A, B = hs

    def acts():
        return torch.from_numpy(rng.uniform(-1, 1, (E, n, 4)).astype(np.float32)).to(A.device)
    for _ in range(burn):
        a = acts()
        for h in hs:
            h.step(a, autoreset=True)
    near = np.arange(E) % 3 == 0
    s = A.get_state()
    if mode == 0:
        rig = {"step_counter": np.where(near, TIME_LIMIT - 4 * (2 + np.arange(E) % 40), s["step_counter"])}
    else:
        s["drone_pos"][near, :, 0] = 0.8 * np.arange(n)[None, :]
        s["drone_pos"][near, :, 1] = 0.0
        s["drone_vel"][near] = 0
        s["clock"][near] = 10.0 - (2 + np.arange(E)[near] % 8) / 60
        rig = {k: s[k] for k in ("drone_pos", "drone_vel", "clock")}
    for h in hs:
        h.set_state(rig)
    resets, reset_steps = 0, set()
    for t in range(T):
        a = acts()
        A.step(a, autoreset=True)
        _, _, te, tr = B.step(a, autoreset=False)
        done = A.reset_happened.bool()
        if mode == 0:
            mask = (te[:, 0] | tr[:, 0]).bool()
            assert torch.equal(mask, done), t
        else:
            mask = done
        if bool(mask.any()):
            B.reset(mask=mask)
            reset_steps.add(t)
        torch.cuda.synchronize()
        resets += int(mask.sum())
        ga, gb = A.get_state(), B.get_state()
        for k in ga:
            assert _bits(ga[k]) == _bits(gb[k]), (t, k)
        assert torch.equal(A.obs.view(torch.int32), B.obs.view(torch.int32)), t
        live_a = A.agent_active.cpu().numpy()
        assert np.array_equal(live_a, gb["active"]), t
        rows = ~mask.cpu().numpy()
        assert np.array_equal(live_a[rows], B.agent_active.cpu().numpy()[rows]), t
        if mode == 0:
            assert torch.equal(A.agent_active, B.agent_active), t
        assert _bits(A.metrics()) == _bits(B.metrics()), t
        assert torch.equal(A.episode_stats.view(torch.int64), B.episode_stats.view(torch.int64)), t
        assert torch.equal(A.reward.view(torch.int32), B.reward.view(torch.int32)), t
    print(name, "resets in the window:", resets, "on", len(reset_steps), "different steps")
    assert resets >= 1 and len(reset_steps) >= 2
    for h in hs:
        h.close()


# ---- c. the episode books across an explicit reset ------------------------------------------------------------------
def _force(b, mode, rows):
    """The envs ``rows`` end in the next step: CTDE past the time limit; MARL at level 2 with the drones in a row
    through the herd centroid (tests/test_gpu_host_outputs.py)."""
    if not rows.any():
        return
    s = b.get_state()
    if mode == 0:
        b.set_state({"step_counter": np.where(rows, 10 ** 6, s["step_counter"])})
    else:
        s["drone_pos"][rows] = R.ring_positions(s["cow_pos"], b.num_drones)[rows]
        s["drone_vel"][rows] = 0
        b.set_state({k: s[k] for k in ("drone_pos", "drone_vel")})


def _books_run(b, mode, variant, rng):
    """tests/reset_ref.py's schedule on the batch; the Monitor is fed the device's own float32 rewards and done
    flags, and the mask of the explicit reset."""
    import torch
    E, n, m = b.n_envs, b.num_drones, b.num_cattle
    k, j = R.K_BEFORE, R.J_AFTER
    mask, force = R.books_schedule(E, variant)
    mon = R.Monitor(E)
    b.reset()
    for t in range(1, k + j + 2):
        _force(b, mode, force.get(t, np.zeros(E, bool)))
        a = torch.from_numpy(rng.uniform(-1, 1, (E, n, 4)).astype(np.float32)).to(b.device)
        _, rew, te, tr = b.step(a, autoreset=True)
        torch.cuda.synchronize()
        done = b.reset_happened.cpu().numpy().astype(bool)
        rew = rew.cpu().numpy().astype(np.float64)
        if mode == 0:
            assert np.array_equal(done, (te[:, 0] | tr[:, 0]).cpu().numpy().astype(bool)), t
        mon.step(rew[:, 0] if mode == 0 else R.marl_reward(rew), done)
        assert np.all(done[force.get(t, np.zeros(E, bool))]), t        # the rigged ends happen
        if t == k:
            if variant == "full":
                b.reset()
            elif variant == "masked":
                b.reset(mask=torch.from_numpy(mask))
            else:
                ang = rng.uniform(-np.pi, np.pi, (E, m))
                b.reset(mask=torch.from_numpy(mask), num_drones=np.full(E, n, np.int32),
                        cow_vel=0.2 * np.stack([np.cos(ang), np.sin(ang)], -1))
            mon.reset(mask)
    return mon, mask


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("mode,n,m,level", [(0, 4, 16, 7), (1, 4, 32, 2)], ids=["ctde_4x16", "marl_4x32"])
def test_episode_books_across_an_explicit_reset(mode, n, m, level, variant):
    """9 steps, an explicit reset (full, masked, masked ch_reset_with), 6 steps, and a step in which every env ends:
    every env's episode_stats row and the EPISODES / RETURN_SUM / LENGTH_SUM sums equal the Monitor's.
    Before the reset kernel cleared the running return and length, every reset env whose episode was open reported
    length 9 + 6 + 1 = 16 (or 12, ended in step 4) instead of 7, and a return off by the abandoned steps' rewards.
    and RETURN_SUM was off by 7.8 to 75.
    Observed now: lengths exact; |return - Monitor| <= 5.2e-8 where the bound is 1.9e-7 (CTDE) and <= 5.5e-6 where
    it is 1.2e-5 (MARL, whose level-2 terminal bonus makes the rewards larger); RETURN_SUM within 1.8e-7 of a bound
    of 6e-6 (CTDE) and 5.3e-5 of 1.1e-3 (MARL)."""
    from cattleherd._lib import METRIC_NAMES
    E, k, j = 64, R.K_BEFORE, R.J_AFTER
    b = _batch(mode, n, m, E, level)
    mon, mask = _books_run(b, mode, variant, np.random.default_rng(5))
    stats = b.episode_stats.cpu().numpy()
    met = dict(zip(METRIC_NAMES, b.metrics()))
    b.close()
    assert np.all(mon.n_ended >= 1) and mon.n_reset_open.any() and mon.n_reset_fresh.any()
    err = np.abs(stats[:, 0] - mon.last[:, 0])
    bound = mon.last_abs * 2.0 ** -24
    print(variant, "lengths of the reset envs:", np.unique(stats[mask, 1]).tolist(), "Monitor:",
          np.unique(mon.last[mask, 1]).tolist(), "| max return err", float(err.max()), "bound at it",
          float(bound[err.argmax()]), "| return_sum err", abs(met["return_sum"] - mon.return_sum), "bound",
          mon.abs_sum * 2.0 ** -24)
    assert np.array_equal(stats[:, 1], mon.last[:, 1]), (stats[:, 1].tolist(), mon.last[:, 1].tolist())
    assert np.all(stats[mask, 1] == j + 1)
    assert np.all(err <= bound), (int(err.argmax()), float(err.max()))
    assert met["episodes"] == mon.episodes and met["length_sum"] == mon.length_sum
    assert abs(met["return_sum"] - mon.return_sum) <= mon.abs_sum * 2.0 ** -24
    assert met["steps"] == E * (k + j + 1)            # the abandoned steps were still steps
    assert mon.length_sum + mon.abandoned == E * (k + j + 1)


# ---- d. the adapters ------------------------------------------------------------------------------------------------
def test_vec_env_episode_info_after_a_second_reset():
    """CattleHerdVecEnv: reset, 9 steps, reset again; the first info["episode"] after it has "l" = the steps since
    the second reset.  Observed: l = 5 at step 5; before the reset kernel cleared the books, l = 15 at step 6 of a
    schedule one step longer."""
    from cattleherd.vec_env import CattleHerdVecEnv
    E, n, m = 64, 4, 16
    venv = CattleHerdVecEnv(E, num_drones=n, num_cattle=m, curriculum_level=7)
    rng = np.random.default_rng(2)
    venv.reset()
    for _ in range(9):
        venv.step(rng.uniform(-1, 1, (E, n, 4)).astype(np.float32))
    venv.reset()
    venv.batch.set_state({"step_counter": np.where(np.arange(E) % 4 == 1, TIME_LIMIT - 4 * 3, 0)})   # end in step 5
    seen = []
    for s in range(1, 9):
        _, _, dones, infos = venv.step(rng.uniform(-1, 1, (E, n, 4)).astype(np.float32))
        seen = [(e, infos[e]["episode"]["l"]) for e in np.nonzero(dones)[0]]
        if seen:
            break
    venv.close()
    print("first episodes after the second reset, (env, l):", seen[:4], "at step", s)
    assert seen and all(length == s for _, length in seen), (s, seen)


def test_episode_ring_after_a_mid_episode_reset():
    """train_log.EpisodeRing fed by the native collection after a mid-episode batch.reset(): each env's first
    recorded length is the steps since that reset.  Observed: lengths 1, 3 and 6; before the reset kernel cleared
    the books each was 9 more, the steps before the reset."""
    import torch
    from cattleherd.policy import DevicePolicy
    from cattleherd.rollout import DeviceRolloutBuffer
    from cattleherd.train_log import EpisodeRing
    E, T = 64, 10
    b = _batch(0, 4, 16, E, 7)
    b.reset()
    for _ in range(9):
        b.step(random_actions=True, autoreset=True)
    b.reset()
    ends_at = np.array([1, 1, 3, 3, 6, 1000, 1000, 1000])[np.arange(E) % 8]       # steps after the reset
    b.set_state({"step_counter": TIME_LIMIT - 4 * (ends_at - 2)})
    actor = DevicePolicy(DevicePolicy.random_layers([12 * 86, 128, 128, 16], seed=1), "tanh", None)
    critic = DevicePolicy(DevicePolicy.random_layers([12 * 86, 128, 128, 1], seed=2), "tanh", None)
    ring = EpisodeRing(b, 4 * E).begin()
    DeviceRolloutBuffer(b, T).collect(actor, critic, torch.full((16,), -1.0, device=b.device), seed=9, ring=ring)
    entries = ring.entries()
    b.close()
    first = {}
    for _, length, env in entries:
        first.setdefault(env, length)
    print("first recorded lengths:", sorted(set(first.values())))
    assert len(first) >= int((ends_at <= T).sum())
    for env, length in first.items():
        assert ends_at[env] <= T and length == ends_at[env], (env, length)


# ---- e. ch_reset_with -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_reset_with_honours_the_mask_and_indexes_by_env(precision):
    """Only masked envs take num_drones[e] / cow_vel[e] -- by env index, not by rank in the mask --; an f32 handle
    stores the velocities as their float32 rounding; the other envs are bit-equal to before."""
    import torch
    E, n, m = 37, 4, 16
    b = _batch(0, n, m, E, 7, precision=precision, min_drones=2, max_drones=4)
    b.reset()
    for _ in range(5):
        b.step(random_actions=True, autoreset=True)
    torch.cuda.synchronize()
    g0, obs0 = b.get_state(), b.obs.cpu().numpy().copy()
    mask = np.random.default_rng(8).random(E) < 0.5
    mask[[1, E - 1]] = True
    mask[[0, 2]] = False
    nd = (2 + np.arange(E) % 3).astype(np.int32)
    ang = 0.01 * np.arange(E)[:, None] + 0.1 * np.arange(m)[None, :]
    cv = 0.2 * np.stack([np.cos(ang), np.sin(ang)], -1)
    b.reset(mask=torch.from_numpy(mask), num_drones=nd, cow_vel=cv)
    g, obs = b.get_state(), b.obs.cpu().numpy()
    b.close()
    _same_bits(g, g0, ~mask, "unmasked")
    assert _bits(obs[~mask]) == _bits(obs0[~mask])
    assert np.array_equal(g["n"][mask], nd[mask])
    assert np.array_equal(g["active"][mask], np.arange(n)[None, :] < nd[mask][:, None])
    want = cv if precision == "f64" else cv.astype(np.float32).astype(np.float64)
    assert np.array_equal(g["cow_vel"][mask], want[mask])
    assert np.all(g["step_counter_A"][mask] == 0) and np.array_equal(g["episode"][mask], g0["episode"][mask] + 1)


@pytest.mark.parametrize("bad", [0, 5])
def test_reset_with_rejects_an_invalid_num_drones(bad):
    """NUM_DRONES of 0 or num_drones + 1 anywhere in the array, also at an env the mask leaves out: CH_ERR_INVALID
    and the state untouched."""
    import torch
    from cattleherd import _lib
    E, n, m = 37, 4, 16
    b = _batch(0, n, m, E, 7)
    b.reset()
    for _ in range(3):
        b.step(random_actions=True, autoreset=True)
    torch.cuda.synchronize()
    g0, obs0 = b.get_state(), b.obs.clone()
    mask = np.arange(E) % 2 == 0
    nd = np.full(E, n, np.int32)
    nd[E - 2] = bad                                   # E - 2 is odd: not in the mask
    with pytest.raises(_lib.ChError) as ei:
        b.reset(mask=torch.from_numpy(mask), num_drones=nd)
    assert ei.value.code == _lib.CH_ERR_INVALID
    g = b.get_state()
    _same_bits(g, g0, slice(None), "rejected")
    assert torch.equal(b.obs, obs0)
    b.close()
