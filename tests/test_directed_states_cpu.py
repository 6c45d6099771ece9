"""Census of the directed-state generator (tests/directed_states.py) on the CPU oracle alone: the condition that
keeps tests/test_gpu_directed.py from passing vacuously.  For every case the GPU tests step, one oracle step from
the directed batch must reach the near-drone flock terms, the exact 1 m pair, both flock parities, terminations at
every level that has a terminating branch, level increments, every truncation cause on its own and (MARL) cleared
`active` bits.  The floors are conditions on the generator, not measurements: a case that misses one is fixed in
the generator.  (Like the other CPU tests that read the spawn table, it needs the built libcattleherd.so beside
the oracle, for cattleherd._lib.spawn_table.)"""
import numpy as np
import pytest

import directed_states as D
from helpers import stack


def _table(m):
    from cattleherd._lib import spawn_table
    return spawn_table(m)


def _census(case):
    mode, n, m, level, kw = case
    E = D.E_DIRECTED
    envs, states = D.directed_states(mode, n, m, level, E, D.case_seed(case), _table(m), **kw)
    acts = D.first_actions(states, n, seed=7)
    outs = [env.step(acts[e], autoreset=False) for e, env in enumerate(envs)]
    post = [env.get_state() for env in envs]
    c = {"finite": True, "pairs": 0, "lt1": 0, "band": 0, "exact": 0, "flock": 0, "term": 0, "levelup": 0,
         "cleared": 0, "trunc": 0, "cause": dict.fromkeys(D.CAUSES, 0)}
    for e in range(E):
        o, r, te, tr = outs[e][:4]
        nl = int(post[e]["n"])
        live = np.asarray(states[e]["active"][:nl], bool) if mode == 1 else np.ones(1, bool)
        rr = r[:nl][live] if mode == 1 else r
        act = states[e]["active"] if mode == 1 else None
        # with fewer than 3 live drones the reference's own reward is NaN (the second-nearest drone distance is inf
        # and enters the spacing terms, CattleAviary.py:213-332; the GPU tests compare NaN with NaN there, as
        # test_step_vs_oracle does at 2 drones); everything else is finite everywhere
        c["finite"] &= bool(np.isfinite(o).all() and (nl < 3 or np.isfinite(rr).all()))
        for k in ("drone_pos", "drone_vel", "drone_quat", "cow_pos", "cow_vel", "clock"):
            c["finite"] &= bool(np.isfinite(np.asarray(post[e][k])).all())
        if D.flock_runs(states[e]):   # the pairs the flock of this step saw: the positions after the physics
            c["flock"] += 1
            d = D.pair_distances(post[e], m)
            c["pairs"] += d.size
            c["lt1"] += int((d < 1.0).sum())
            c["band"] += int(((d >= 1.0) & (d <= 1.1)).sum())
            c["exact"] += int((d == 1.0).sum())
        c["term"] += int(te.any())
        c["levelup"] += int(post[e]["level"] > states[e]["level"])
        c["cleared"] += int((np.asarray(states[e]["active"][:nl], int) - np.asarray(post[e]["active"][:nl], int) > 0).sum())
        if tr.any():
            c["trunc"] += 1
            causes = D.truncation_causes(states[e], post[e], mode, m, level, act)
            if sum(causes.values()) == 1:
                c["cause"][[k for k, v in causes.items() if v][0]] += 1
        else:
            # the recomputed conditions and the oracle's flag agree (a terminated MARL env reports no truncation)
            assert te.any() or not any(D.truncation_causes(states[e], post[e], mode, m, level, act).values()), (e, D.class_of(e))
    return envs, c


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_directed_census(case):
    mode, n, m, level, kw = case
    E = D.E_DIRECTED
    envs, c = _census(case)
    print(f"CENSUS {D.case_id(case):28s} flock envs {c['flock']:2d}/{E} | pairs<1m {c['lt1']:4d}/{c['pairs']:5d} "
          f"({100 * c['lt1'] / c['pairs']:4.1f}%) | band {c['band']:3d} ({100 * c['band'] / c['pairs']:4.1f}%) | "
          f"exact {c['exact']} | term {c['term']:2d} | levelup {c['levelup']:2d} | trunc {c['trunc']:2d} "
          + " ".join(f"{k[:4]} {v}" for k, v in c["cause"].items()) + f" | cleared {c['cleared']}")
    assert c["finite"]
    assert c["lt1"] >= 0.10 * c["pairs"]
    assert c["band"] >= 0.02 * c["pairs"]
    assert c["exact"] >= 1
    assert 0.25 * E <= c["flock"] <= 0.75 * E
    if level == 7:
        assert c["term"] == 0 and c["levelup"] == 0
    else:
        assert c["term"] >= 5
        assert c["levelup"] >= 3
        if mode == 1:
            assert c["cleared"] >= 3
    for k, v in c["cause"].items():
        assert v >= 3, k


@pytest.mark.parametrize("case", [(0, 4, 16, 7, {}), (1, 4, 32, 0, {}), (0, 12, 16, 7, {})], ids=D.case_id)
def test_directed_free_run_stays_near(case):
    """The bit-identity window of test_gpu_directed.py: 40 free-running steps of Philox actions with auto-reset from
    the directed batch still have 5 % of the live cow-drone pairs within the predator range at the end."""
    mode, n, m, level, kw = case
    envs, _ = D.directed_states(mode, n, m, level, D.E_DIRECTED, D.case_seed(case), _table(m), **kw)
    for t in range(40):
        for env in envs:
            env.step(env.random_actions(t), autoreset=True)
    d = np.concatenate([D.pair_distances(env.get_state(), m).ravel() for env in envs])
    print(f"FREE-RUN {D.case_id(case)}: pairs <= 1.1 m after 40 steps {int((d <= 1.1).sum())}/{d.size} "
          f"({100 * (d <= 1.1).mean():.1f}%)")
    assert np.isfinite(d).all()
    assert (d <= 1.1).mean() >= 0.05


def _assert_branch_floors(case, c):
    """test_directed_census's floors on the classes and branches of the batch (its floors on the share of near
    cow-drone pairs belong to the flock comparisons of tests/test_gpu_directed.py; here: some of each)."""
    mode, n, m, level, kw = case
    E = D.E_DIRECTED
    assert c["finite"]
    assert c["lt1"] >= 1 and c["band"] >= 1 and c["exact"] >= 1
    assert 0.25 * E <= c["flock"] <= 0.75 * E
    if level == 7:
        assert c["term"] == 0 and c["levelup"] == 0
    else:
        assert c["term"] >= 5
        assert c["levelup"] >= 3
        if mode == 1:
            assert c["cleared"] >= 3
    for k, v in c["cause"].items():
        assert v >= 3, k


@pytest.mark.parametrize("case", D.F32_STEP_CASES, ids=D.case_id)
def test_f32_step_census(case):
    """The cases of tests/test_gpu_f32_parity.py's one-step tests, on the oracle alone: the same floors as their f64
    twins (every class present, every terminating and truncating branch reached), each physics variant's own term
    really exercised, and every deciding quantity of the step at least 1e-4 relative from its threshold, so that
    exact flags are a fair demand of an f32 kernel -- the hold clock of the classes D.ON_THRESHOLD lists aside,
    which the generator puts on the hold on purpose and which f32 arithmetic reaches too."""
    import oracle as O
    mode, n, m, level, kw = case
    E = D.E_DIRECTED
    envs, states = D.directed_states(mode, n, m, level, E, D.case_seed(case), _table(m), **kw)
    assert {D.class_of(e) for e in range(E)} == set(D.CLASSES)
    ph = kw.get("physics", 0)
    if ph in (D.PH_DW, D.PH_ALL):
        # _downwash: a drone above another (dz > 0) within 10 m horizontally
        def above(s):
            p = np.asarray(s["drone_pos"])[:int(s["n"])]
            dz = p[:, None, 2] - p[None, :, 2]
            return int(((dz > 0) & (np.linalg.norm(p[:, None, :2] - p[None, :, :2], axis=-1) < 10)).sum())
        dw = sum(above(s) > 0 for s in states)
        print(f"DOWNWASH {D.case_id(case)}: envs with a drone above another within 10 m {dw}/{E}")
        assert dw >= 1
    if ph in (D.PH_GND, D.PH_ALL):
        # _groundEffect: drones on both sides of GND_EFF_H_CLIP (the oracle's own constant), before and after the step
        z0 = np.concatenate([np.asarray(s["drone_pos"])[:int(s["n"]), 2] for s in states])
    if ph in (D.PH_DRAG, D.PH_ALL):
        # _drag reads last_clipped_action: the burn-in steps left it non-zero in every env
        assert all(np.any(np.asarray(s["last_rpm"])[:int(s["n"])] != 0) for s in states)
    acts = D.first_actions(states, n, seed=7)
    _, c = _census(case)
    _assert_branch_floors(case, c)
    post = []
    for e, env in enumerate(envs):
        env.step(acts[e], autoreset=False)
        post.append(env.get_state())
    if ph in (D.PH_DW, D.PH_ALL):
        # 1 / dz^2: the generator staggers the heights so that the reference resolves the term -- no two live drones
        # within 10 m of each other come closer in height than 5 mm, before or after the step (an f32 height of
        # 0.45 m is good to 3e-8 m, a difference of two to 6e-8 m, the force then to 2 * 6e-8 / dz = 2.4e-5 relative,
        # inside the 1e-4 budget) -- and the term is no token either: pairs 1 m or less apart horizontally are one
        # stagger step, 5 cm, apart in height
        def dzs(s, reach):
            p = np.asarray(s["drone_pos"])[:int(s["n"])]
            iu = np.triu_indices(len(p), 1)
            near = np.linalg.norm(p[:, None, :2] - p[None, :, :2], axis=-1)[iu] < reach
            return np.abs(p[:, None, 2] - p[None, :, 2])[iu][near]
        dz = np.concatenate([dzs(s, 10) for s in states] + [dzs(s, 10) for s in post])
        close = np.concatenate([dzs(s, 1.0) for s in states])
        print(f"DOWNWASH {D.case_id(case)}: smallest height difference of two drones within 10 m {dz.min():.4f} m; "
              f"pairs within 1 m horizontally {close.size}, their smallest {close.min():.4f} m")
        assert dz.min() >= 0.005
        assert close.size >= E // 2 and close.min() <= 0.06
    if ph in (D.PH_GND, D.PH_ALL):
        z1 = np.concatenate([np.asarray(s["drone_pos"])[:int(s["n"]), 2] for s in post])
        clip = O.gnd_eff_h_clip()
        lowd = int(((z0 < 0.75 * clip) & (z1 < 0.75 * clip)).sum())   # (the propellers sit within 0.25 clip of the COM's height at these tilts)
        print(f"GROUND {D.case_id(case)}: GND_EFF_H_CLIP {clip:.5f} m, drones below it {lowd}, above {int((z0 > clip).sum())}")
        assert lowd >= 1 and int(((z0 > 2 * clip) & (z1 > 2 * clip)).sum()) >= 1
    on = D.ON_THRESHOLD.get(level, ())
    assert not on or D.hold_reached_in_f32(mode, level)
    worst, excused = np.inf, 0
    for e in range(E):
        mg = D.margins(states[e], post[e], mode, m, level)
        assert D.decision_margins(states[e], post[e], mode, m, level) == min(mg.values())
        if D.class_of(e) in on and mg.get("hold", 1.0) < D.MARGIN:
            excused += 1
            mg.pop("hold")
        k = min(mg, key=mg.get)
        assert mg[k] >= D.MARGIN, (e, D.class_of(e), k, mg[k])
        worst = min(worst, mg[k])
    print(f"MARGINS {D.case_id(case)}: smallest relative distance to a threshold {worst:.3e}; "
          f"envs on the hold by construction {excused} ({', '.join(on) if excused else 'none'})")
    assert excused <= sum(D.class_of(e) in on for e in range(E))


@pytest.mark.parametrize("case", D.ROLLOUT_CASES, ids=D.rollout_id)
def test_rollout_reference_keeps_its_margins(case):
    """The lockstep f32 rollouts of tests/test_gpu_f32_parity.py excuse a flag difference only on an env-step on
    which a deciding quantity of the oracle lies within 1e-4 relative of its threshold, on at most 1 % of the
    env-steps.  That cap must be one the reference alone respects: the oracle free-running in f64 from the same
    resets with the same Philox actions for the same 120 steps has no such env-step at all, ends episodes, and ends
    some after the first ten steps (D.ROLLOUT_OFFSET is chosen so)."""
    import oracle as O
    from cattleherd._lib import PHYSICS
    physics, mode, n, m = case
    E, T, level = D.ROLLOUT_E, D.ROLLOUT_T, D.rollout_level(mode)
    off = D.ROLLOUT_OFFSET[case]
    envs = [O.Env(mode, n, m, _table(m), start_level=level, env_id=off + e, physics=PHYSICS[physics]) for e in range(E)]
    for env in envs:
        env.reset()
    s = D.rollout_start(stack([env.get_state() for env in envs]), mode, n)
    for e, env in enumerate(envs):
        env.set_state({k: v[e] for k, v in s.items()})
    resets = later = 0
    worst = (np.inf, None)
    for t in range(T):
        for e, env in enumerate(envs):
            pre = env.get_state()
            done = env.step(env.random_actions(t), autoreset=False)[4]
            mg = D.margins(pre, env.get_state(), mode, m, level)
            k = min(mg, key=mg.get)
            if mg[k] < worst[0]:
                worst = (mg[k], (t, e, k))
            if done:
                env.reset()
                resets += 1
                later += t >= 10
    print(f"ROLLOUT {D.rollout_id(case)} offset {off}: resets {resets} ({later} after step 10), smallest relative "
          f"distance to a threshold {worst[0]:.3e} at (step, env, quantity) {worst[1]}")
    assert worst[0] >= D.MARGIN, worst
    assert resets > 0 and later > 0
