"""CPU tests of the episode-books reference (tests/reset_ref.py): the numpy Monitor driven by oracle envs alone, with
explicit resets injected mid-episode and ends forced as the GPU tests force them, and the schedule the GPU tests
run checked for the cases it must contain."""
import numpy as np
import pytest

import reset_ref as R


def _envs(mode, n, m, E):
    import oracle as O
    from cattleherd._lib import spawn_table
    table = spawn_table(m)
    envs = [O.Env(mode, n, m, table, env_id=e, start_level=7 if mode == 0 else 2) for e in range(E)]
    for env in envs:
        env.reset()
    return envs


def _force_end(mode, env):
    """CTDE: past the time limit (the step counter high, as tests/test_gpu_host_outputs.py does on the device);
    MARL, where truncation does not end the episode: the drones in a row through the herd centroid."""
    if mode == 0:
        env.st.step_counter = 10 ** 6
        return
    n, m = env.st.n, env.cfg.m
    cow = np.array([[env.st.cp[j][0], env.st.cp[j][1]] for j in range(m)])
    for i, p in enumerate(R.ring_positions(cow, n)):
        for c in range(3):
            env.st.dp[i][c] = p[c]
            env.st.dv[i][c] = 0.0


def _run(mode, n, m, E, mask, force, steps, reset_after, seed):
    """The oracle envs through ``steps`` steps of random actions with auto-reset; before step t the envs of force[t]
    are rigged to end in it; after step ``reset_after`` the envs of ``mask`` get an explicit och_reset.  Returns the
    Monitor and, per step, the done flags."""
    envs = _envs(mode, n, m, E)
    mon = R.Monitor(E)
    rng = np.random.default_rng(seed)
    dones = []
    for t in range(1, steps + 1):
        for e in np.nonzero(force.get(t, np.zeros(E, bool)))[0]:
            _force_end(mode, envs[e])
        out = [env.step(rng.uniform(-1, 1, (n, 4)).astype(np.float32), autoreset=True) for env in envs]
        rew = np.stack([o[1] for o in out])
        rew = rew[:, 0] if mode == 0 else R.marl_reward(rew)
        dones.append(mon.step(rew, np.array([o[4] for o in out])).copy())
        if t == reset_after:
            for e in np.nonzero(mask)[0]:
                envs[e].reset()
            mon.reset(mask)
    return mon, np.array(dones)


def test_monitor_on_hand_made_rewards():
    mon = R.Monitor(3)
    mon.step([1.0, 2.0, 4.0], [0, 0, 1])
    mon.step([0.5, -3.0, 8.0], [0, 1, 0])
    mon.reset([1, 1, 0])                       # env 0: open (length 2); env 1: ended on the previous step
    mon.step([0.25, 1.0, 16.0], [1, 0, 1])
    assert mon.last.tolist() == [[0.25, 1.0], [-1.0, 2.0], [24.0, 2.0]]
    assert (mon.episodes, mon.return_sum, mon.length_sum) == (4, 4.0 - 1.0 + 0.25 + 24.0, 1 + 2 + 1 + 2)
    assert mon.abandoned == 2 and mon.n_reset_open.tolist() == [1, 0, 0] and mon.n_reset_fresh.tolist() == [0, 1, 0]
    assert mon.len.tolist() == [0, 1, 0] and mon.ret.tolist() == [0.0, 1.0, 0.0]
    assert mon.last_abs.tolist() == [0.25, 5.0, 24.0] and mon.abs_sum == 4.0 + 5.0 + 0.25 + 24.0
    assert np.array_equal(R.marl_reward([[1.0, np.nan, 2.0], [np.nan, np.nan, np.nan]]), [3.0, 0.0])


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_schedule_of_the_gpu_tests_contains_every_case(variant):
    """The schedule alone (no env): an env reset with an open episode, one reset on the step after it ended, and --
    in the masked variants -- one never reset that ends before and after the reset; every env ends in the last
    step."""
    E, k, j = 64, R.K_BEFORE, R.J_AFTER
    mask, force = R.books_schedule(E, variant)
    mon = R.Monitor(E)
    for t in range(1, k + j + 2):
        mon.step(np.ones(E), force.get(t, np.zeros(E, bool)))
        if t == k:
            mon.reset(mask)
    assert np.any(mon.n_reset_open == 1) and np.any(mon.n_reset_fresh == 1)
    assert np.any(mask & (mon.n_ended == 2) & (mon.n_reset_open == 1))        # ended early, then reset while open
    if variant == "full":
        assert mask.all()
    else:
        never = ~mask
        assert never.any() and np.all(mon.n_reset_open[never] + mon.n_reset_fresh[never] == 0)
        assert np.any(never & (mon.n_ended == 2)) and np.any(never & (mon.n_ended == 1))
        assert np.all(mon.last[never & (mon.n_ended == 1), 1] == k + j + 1)
    # an env reset after step k and ended in step k + j + 1 reports length j + 1, whatever happened before
    assert np.all(mon.last[mask, 1] == j + 1)
    assert mon.length_sum + mon.abandoned == E * (k + j + 1) and np.all(mon.len == 0)


@pytest.mark.parametrize("mode,n,m", [(0, 4, 16), (1, 4, 32)])
@pytest.mark.parametrize("k,j", [(R.K_BEFORE, R.J_AFTER), (30, 29)])
def test_monitor_driven_by_oracle_envs(mode, n, m, k, j):
    """Oracle envs under the GPU tests' schedule (16 steps) and a longer one (60 steps): every forced end happens,
    the lengths add up to the steps taken minus the abandoned ones, and an env reset after step k that ends in
    step k + j' reports length j'."""
    E = 8
    mask, force = R.books_schedule(E, "masked", k, j)
    T = k + j + 1
    mon, dones = _run(mode, n, m, E, mask, force, T, k, seed=10 * mode + k)
    for t, f in force.items():
        assert np.all(dones[t - 1][f]), (t, dones[t - 1])       # the rigging works on the oracle, both modes
    assert dones[-1].all()
    assert mon.steps == E * T
    assert mon.length_sum + mon.abandoned + int(mon.len.sum()) == E * T
    assert mon.abandoned == int(sum(k - (np.nonzero(dones[:k, e])[0].max() + 1 if dones[:k, e].any() else 0)
                                    for e in np.nonzero(mask)[0]))
    assert np.any(mon.n_reset_open) and np.any(mon.n_reset_fresh) and np.any(~mask)
    for e in range(E):
        ends = (np.nonzero(dones[:, e])[0] + 1).tolist()        # 1-based steps in which env e ended; the last is T
        starts = [0] + ends[:-1] + ([k] if mask[e] else [])     # where an episode of env e began
        assert mon.last[e, 1] == T - max(starts), (e, ends)
    assert mon.episodes == int(dones.sum()) and np.isfinite(mon.return_sum)
