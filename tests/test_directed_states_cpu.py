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
            causes = D.truncation_causes(states[e], post[e], mode, m, level)
            if sum(causes.values()) == 1:
                c["cause"][[k for k, v in causes.items() if v][0]] += 1
        else:
            # the recomputed conditions and the oracle's flag agree (a terminated MARL env reports no truncation)
            assert te.any() or not any(D.truncation_causes(states[e], post[e], mode, m, level).values()), (e, D.class_of(e))
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
