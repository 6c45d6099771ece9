"""GPU tests of the DTDE driver's on-device evaluation (cattleherd.marl_eval; ch_marl_eval_begin / _mark / _record,
ch_marl_evaluate_policy) against tests/marl_eval_ref.py, the numpy restatement of the per-agent episode table.
Everything compared is integer bookkeeping, float32 values copied or clamped, or float64 sums in one fixed order, so
every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from marl_eval_ref import MarlEvalRef

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 3, 8


def _assert_tables(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what} {k}"
        assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), f"{what} {k}"


def _assert_episodes(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def _assert_states(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- 1. the recorder alone -----------------------------------------------------------------------------------------
def _synthetic(E, C, S=30):
    """Seeded step outputs: live [S, E, N], float32 rewards [S, E, N] with NaN / 1e30 at the slots that are not live
    (summing one of them shows), reset_happened [S, E] with p = 0.3."""
    rng = np.random.default_rng(1000 * E + C)
    live = (rng.random((S, E, N)) < 0.7).astype(np.uint8)
    reward = rng.normal(0.0, 10.0, (S, E, N)).astype(np.float32)
    poison = np.where(rng.random((S, E, N)) < 0.5, np.float32(np.nan), np.float32(1e30)).astype(np.float32)
    reward = np.where(live != 0, reward, poison)
    rh = (rng.random((S, E)) < 0.3).astype(np.uint8)
    return live, reward, rh


def _synthetic_ns(E, C):
    return sorted({1, E - 1, E, min(2 * E + 3, C * E)} - {0})


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 257])
def test_recorder_equals_the_reference_after_every_step(E, C):
    """ch_marl_eval_begin / ch_marl_eval_record on synthetic inputs, N = 3, 30 steps: seeded ``live`` written straight
    into the table's tensor, float32 rewards with NaN or 1e30 wherever the agent is not live, reset_happened with
    p = 0.3; after every step every table array and ``remaining`` equal the reference exactly.  E covers one partial
    wave, one wave less / exactly / plus one lane, and two workgroups (257 > 256 threads).  Every run has an env that
    ends again past its quota, and for E > 1 an env of quota 0 that ends -- both asserted on the reference."""
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.marl_eval import DeviceMarlEvalTable
    live, reward, rh = _synthetic(E, C)
    S = len(rh)
    b = HerdBatch(E, N, M, mode="marl")
    dev = [torch.as_tensor(np.ascontiguousarray(a)).to(b.device) for a in (live, reward, rh)]
    saw_zero = False
    for n in _synthetic_ns(E, C):
        table = DeviceMarlEvalTable(b, C).begin(n)
        ref = MarlEvalRef(n, E, N, C)
        _assert_tables(table.arrays(), ref.arrays(), f"n={n} begin")
        io = _lib.ChStepIO()
        for t in range(S):
            table.live.copy_(dev[0][t])
            io.reward, io.reset_happened = dev[1][t].data_ptr(), dev[2][t].data_ptr()
            table.record(t, io)
            ref.step(live[t], reward[t], rh[t], t)
            _assert_tables(table.arrays(), ref.arrays(), f"n={n} step {t}")
        _assert_episodes(table.episodes(), ref.episodes())
        assert ref.ignored_full > 0
        assert np.isfinite(ref.ep_return).all() and np.isfinite(ref.acc_return).all()   # no poisoned slot was summed
        saw_zero |= ref.ignored_zero > 0
    assert saw_zero or E == 1   # (one env: n >= 1 leaves no quota of 0)
    b.close()


# ---- the graded near-herd injection and the approach-biased policy (restated from tests/test_gpu_marl_rollout.py) ---
def _bias_policy(bias):
    """A policy whose output is `bias` exactly on every row (zero weights), on the device and in torch."""
    import torch
    from cattleherd.policy import DevicePolicy
    return DevicePolicy([(torch.zeros(len(bias), 86), torch.tensor(bias, dtype=torch.float32))], "tanh", None)


APPROACH = [0.0, -1.0, 0.0, 1.0, -3.0, -3.0, -3.0, -3.0]   # fly along -y at the speed limit
# the adjustment of the injection (below): where the drones of the envs e % 8 == 0 start, in m from the herd centroid
CLOSE = 0.31


def _inject_graded(b, n):
    """test_gpu_marl_rollout's _make_graded on the batch's current state.  The envs e % 4 == 0 start with their drone
    centroid 0.45 m from the herd centroid, inside level 2's approach radius (approach_min 0.6): every agent
    terminates and the env ends at once -- unless the env is n + 2 successes short of level 3 (approach_min 0.3, 100
    successes), where agent 0 alone drops out and the env goes on at level 3 (marl_wrapper.py:104-113).  The drones of
    the others start 0.6 .. 1.0 m out and fly towards the herd (APPROACH), crossing the radius at steps spread over the
    run; every other one of those is n + 2 successes short as well.
    Adjusted for the evaluation's cases: in _make_graded every env e % 4 == 0 is short of level 3, so none ends at
    once.  Here those with e % 8 == 4 keep their tally and end in the step after the injection (a second injection
    then ends them a second time: past their quota), and those with e % 8 == 0 start CLOSE m out: agent 0 drops out
    in the first step, and the others terminate when the centroid is inside level 3's 0.3 m a few steps later, so the
    filed episode has agent 0's length shorter than the others'."""
    E = b.n_envs
    s = b.get_state()
    e = np.arange(E)
    near = e % 4 == 0
    far = np.flatnonzero(~near)
    dist = np.full(E, 0.45)
    dist[far] = np.linspace(0.6, 1.0, len(far))
    dist[e % 8 == 0] = CLOSE
    c = s["cow_pos"].mean(1)
    for k in range(n):
        s["drone_pos"][:, k, 0] = c[:, 0] + 0.5 * (k - (n - 1) / 2)
        s["drone_pos"][:, k, 1] = c[:, 1] + dist
    tally = s["tally"].copy()
    tally[e % 8 == 0] = 100 - n - 2
    tally[far[::2]] = 100 - n - 2
    b.set_state({"drone_pos": s["drone_pos"], "tally": tally})


def _make_graded(E, n=N, m=M, **kw):
    from cattleherd.env import HerdBatch
    b = HerdBatch(E, n, m, mode="marl", curriculum_level=2, min_drones=n, max_drones=n, **kw)
    b.reset()
    _inject_graded(b, n)
    return b


# ---- 2. the three loops ---------------------------------------------------------------------------------------------
E2, N_EVAL2, C2, HALF2 = 32, 40, 2, 12


def _graded_run(path, check_every=16, halves=2):
    """The evaluation of test 2 through DeviceMarlEvalTable.<path>: `halves` times (inject, HALF2 steps), the later
    ones continuing with first_step_index.  Returns (arrays, episodes, final state, [(steps, remaining)], the
    reference fed with every step's outputs -- run_steps only)."""
    from cattleherd.marl_eval import DeviceMarlEvalTable
    b = _make_graded(E2)
    policy = _bias_policy(APPROACH)
    table = DeviceMarlEvalTable(b, C2).begin(N_EVAL2)
    ref = MarlEvalRef(N_EVAL2, E2, N, C2) if path == "run_steps" else None

    def feed(t):
        ref.step(table.live.cpu().numpy(), b.reward.cpu().numpy(), b.reset_happened.cpu().numpy(), t)

    runs = []
    for h in range(halves):
        if h > 0:
            _inject_graded(b, N)
        kw = dict(on_step=feed) if ref is not None else {}
        runs.append(getattr(table, path)(policy, HALF2, check_every, first_step_index=h * HALF2, **kw))
    out = (table.arrays(), table.episodes(), b.get_state(), runs, ref)
    b.close()
    return out


@pytest.fixture(scope="module")
def graded_python_loop():
    """run_steps over both halves, computed once and shared (left unchanged by the tests that read it)."""
    return _graded_run("run_steps")


def test_native_loop_equals_python_loop_equals_reference(graded_python_loop):
    """ch_marl_evaluate_policy, the same kernels launched from Python (run_steps) and the reference fed with
    run_steps' per-step ``live``, rewards and reset_happened fill identical tables; the two device loops also leave
    identical env states.  32 envs x (3 drones, 8 cattle) at level 2, n = 40 (quota 1 for the envs below 24, 2 for
    the others), C = 2, the approach-biased policy.
    Final values: 24 steps as two calls of 12 with the graded injection applied before each (the second call continues
    with first_step_index = 12).  Without the second injection no env ends twice inside a few dozen steps -- a fresh
    episode starts metres from the herd -- so none would be ignored at its quota; with it the envs 4, 12 and 20 (quota
    1) end at steps 0 and 12.  The envs e % 8 == 0 start 0.31 m out, so that agent 0 drops out at once and the
    others end the episode a few steps later.  All three facts are asserted on the reference.  Measured on an
    MI355X: 16 filed episodes (lengths 1, 1, 1, 1, 12, 12, 14, 14, 14, 14, 17, 19, 20, 22, 23, 24), 4 of them with
    agent 0's length shorter than agent 1's, 3 endings ignored at the quota, remaining 24."""
    nat = _graded_run("run")
    py = graded_python_loop
    ref = py[4]
    # the run holds what it is meant to test (asserted on the reference)
    r, ln, ar, al, env, end = ref.episodes()
    assert len(r) > 0                                              # an ended, filed episode
    assert (al[:, 0] < al[:, 1]).any()                             # agent 0's length shorter than agent 1's
    assert ref.ignored_full > 0                                    # an env ignored at its quota
    assert ref.remaining > 0 and (end >= HALF2).any() and (end < HALF2).any()
    print(f"graded run: {len(r)} episodes, {int((al[:, 0] < al[:, 1]).sum())} with agent 0 shorter, "
          f"{ref.ignored_full} ignored at quota, remaining {ref.remaining}, lengths {ln.tolist()}")
    assert nat[3] == py[3] and [s for s, _ in py[3]] == [HALF2, HALF2] and py[3][1][1] == ref.remaining
    _assert_tables(py[0], ref.arrays(), "python vs reference")
    _assert_tables(nat[0], ref.arrays(), "native vs reference")
    _assert_episodes(py[1], ref.episodes())
    _assert_episodes(nat[1], ref.episodes())
    _assert_states(nat[2], py[2])


# ---- 3. a varying number of agents --------------------------------------------------------------------------------
def test_agent_slots_follow_num_drones():
    """num_drones = 4 with min_drones = 2, max_drones = 4: every reset draws the episode's NUM_DRONES.  Three times
    (every env put next to its herd, NUM_DRONES read from env_ints, two native steps): each injection ends every env
    in its first step.  For every filed episode agent_length > 0 exactly for i < the episode's NUM_DRONES -- the value
    read before the step that ended it -- and the slots of the absent agents hold 0."""
    from cattleherd.env import HerdBatch
    from cattleherd.marl_eval import DeviceMarlEvalTable
    E, n, rounds = 64, 4, 3
    b = HerdBatch(E, n, M, mode="marl", curriculum_level=2, min_drones=2, max_drones=4)
    b.reset()
    policy = _bias_policy(APPROACH)
    table = DeviceMarlEvalTable(b, rounds).begin(rounds * E)
    n_at = {}
    for k in range(rounds):
        s = b.get_state()
        c = s["cow_pos"].mean(1)
        for i in range(n):   # 0.2 m apart: the centroid of the first 2, 3 or 4 drones is within 0.5 m of the herd's
            s["drone_pos"][:, i, 0] = c[:, 0] + 0.2 * (i - (n - 1) / 2)
            s["drone_pos"][:, i, 1] = c[:, 1] + 0.45
        b.set_state({"drone_pos": s["drone_pos"]})
        n_at[2 * k] = b.env_ints()["n"]
        steps, rem = table.run(policy, 2, first_step_index=2 * k)
        assert steps == 2
    assert rem == 0
    seen = np.concatenate(list(n_at.values()))
    assert seen.min() == 2 and seen.max() == 4 and len(np.unique(seen)) == 3
    r, ln, ar, al, env, end = table.episodes()
    assert len(r) == rounds * E and sorted(set(end.tolist())) == [0, 2, 4]
    n_ep = np.array([n_at[int(t)][e] for e, t in zip(env, end)])
    took_part = np.arange(n)[None, :] < n_ep[:, None]
    assert np.array_equal(al > 0, took_part)
    assert np.all(ar[~took_part] == 0.0) and np.all(al[~took_part] == 0)
    assert np.array_equal(al.max(1), ln) and ln.tolist() == [1] * E + [2] * (2 * E)
    # (the returns themselves are not looked at: in compat mode a 2-drone episode's rewards are NaN, as the reference's)
    b.close()


# ---- 4. check_every ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_every", [1, 5, 16])
def test_check_every_leaves_the_table_alone_and_a_second_call_continues(check_every, graded_python_loop):
    """The recorder runs stand-alone at every check and fused into the next action kernel between checks: with
    check_every 1 always stand-alone, with 16 fused but for each call's last step, with 5 both.  The tables, the
    episodes and the env state after two calls of 12 steps (the second with first_step_index = 12) equal the Python
    loop's, whose recorder is always a launch of its own; ``remaining`` stays above 0, so every call runs to its
    cap."""
    nat = _graded_run("run", check_every)
    py = graded_python_loop
    assert nat[3] == py[3] and nat[3][1][1] > 0
    _assert_tables(nat[0], py[0], f"check_every={check_every}")
    _assert_episodes(nat[1], py[1])
    _assert_states(nat[2], py[2])
    assert py[1][5].min() < HALF2 <= py[1][5].max()   # end steps from both calls


# ---- 5. the trained RLlib weights ---------------------------------------------------------------------------------
def _trained():
    """The reference's trained RLlib weights (simulator/policy_weights.pkl, via tests/golden/make_policy_marl_golden)."""
    from cattleherd.policy import DevicePolicy
    d = np.load(os.path.join(ROOT, "tests", "golden", "policy_marl_rllib.npz"))
    return DevicePolicy.rllib_policy({k.replace("__", "."): d[k] for k in d.files if "__" in k})


def test_metrics_and_the_trained_policys_env_actions():
    """evaluate_marl_policy on the graded batch, driven with the approach-biased policy (what the trained policy does
    next to a herd is not known to end episodes within a few dozen steps).  The quota rule gives the episodes to the
    last envs: over the first 29 envs of the graded injection n = 1 is env 28's, which ends in the first step -- finite
    metrics with num_episodes = n; over all 32, n = 4 is the envs 28 .. 31, of which 29 .. 31 are 0.95 .. 1.0 m out
    and do not end within the cap: RuntimeError naming ``remaining``.
    The trained weights: after two steps (agents have dropped out) the env actions of one native step equal
    clamp(forward[:, :4], -1, 1) bit for bit where ``live`` is set and 0 elsewhere."""
    from cattleherd.marl_eval import DeviceMarlEvalTable, evaluate_marl_policy
    approach = _bias_policy(APPROACH)
    b = _make_graded(29)
    m = evaluate_marl_policy(b, approach, 1, max_steps=4, reset=False)
    assert m["num_episodes"] == 1 and m["episode_len_mean"] == 1.0
    assert m["episode_return_min"] == m["episode_return_mean"] == m["episode_return_max"]
    assert np.isfinite(m["episode_return_mean"]) and sorted(m["agent_episode_returns_mean"]) == ["agent_0", "agent_1", "agent_2"]
    assert all(np.isfinite(v) for v in m["agent_episode_returns_mean"].values())
    b.close()
    b = _make_graded(E2)
    with pytest.raises(RuntimeError, match="remaining = 3 of 4"):
        evaluate_marl_policy(b, approach, 4, max_steps=4, reset=False)
    # the trained policy's deterministic action
    trained = _trained()
    assert trained.dims[-1] == 8
    table = DeviceMarlEvalTable(b, 1).begin(1)
    want = trained.forward_batch(b).clone()
    table.run(trained, 1)
    b.torch.cuda.synchronize()
    live = table.live.cpu().numpy().reshape(-1) != 0
    assert live.any() and not live.all()
    got = table.env_actions.cpu().numpy().reshape(-1, 4)
    want = want[:, :4].clamp(-1.0, 1.0).cpu().numpy()
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got[live].view(np.uint32), want[live].view(np.uint32))
    assert np.all(got[~live].view(np.uint32) == 0)
    b.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------
def test_rejections():
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.marl_eval import DeviceMarlEvalTable
    from cattleherd.policy import DevicePolicy
    L = _lib.lib()
    E = 8
    b = HerdBatch(E, N, M, mode="marl")
    b.reset()
    table = DeviceMarlEvalTable(b, 1)
    policy = _bias_policy(APPROACH)
    policy._ensure_packed()
    out = b.torch.zeros((E * N, 8), dtype=b.torch.float32, device=b.device)
    io = _lib.ChMarlEvalIO()
    io.step, io.policy_out, io.env_actions = ctypes.pointer(b._io), out.data_ptr(), table.env_actions.data_ptr()
    steps, rem = ctypes.c_int64(), ctypes.c_int64()

    def evaluate(batch, net, eio):
        return L.ch_marl_evaluate_policy(batch.handle, ctypes.byref(net._net), ctypes.byref(table._tb), ctypes.byref(eio),
                                         4, 1, 0, ctypes.byref(steps), ctypes.byref(rem), batch._stream())

    def all_four(batch):
        return (L.ch_marl_eval_begin(batch.handle, ctypes.byref(table._tb), E, batch._stream()),
                L.ch_marl_eval_mark(batch.handle, ctypes.byref(table._tb), batch._stream()),
                L.ch_marl_eval_record(batch.handle, ctypes.byref(table._tb), batch._io_ref, 0, batch._stream()),
                evaluate(batch, policy, io))

    # a CTDE handle, and a MARL handle with the bare-dict semantics: CH_ERR_UNSUPPORTED from all four
    c = HerdBatch(E, N, M, mode="ctde")
    with pytest.raises(ValueError):
        DeviceMarlEvalTable(c, 1)
    assert all_four(c) == (_lib.CH_ERR_UNSUPPORTED,) * 4
    assert b"MARL" in L.ch_last_error(c.handle)
    c.close()
    bare = HerdBatch(E, N, M, mode="marl", marl_wrapper=False)
    assert all_four(bare) == (_lib.CH_ERR_UNSUPPORTED,) * 4
    assert b"marl_wrapper = 1" in L.ch_last_error(bare.handle)
    bare.close()
    # more episodes per env than slots
    with pytest.raises(_lib.ChError, match="capacity") as ei:
        table.begin(E + 1)
    assert ei.value.code == _lib.CH_ERR_INVALID
    with pytest.raises(_lib.ChError) as ei:
        table.begin(0)
    assert ei.value.code == _lib.CH_ERR_INVALID
    table.begin(E)
    # a step io without reset_happened / reward
    for field in ("reset_happened", "reward"):
        sio = _lib.ChStepIO()
        ctypes.memmove(ctypes.byref(sio), ctypes.byref(b._io), ctypes.sizeof(sio))
        setattr(sio, field, None)
        with pytest.raises(_lib.ChError, match=field) as ei:
            table.record(0, sio)
        assert ei.value.code == _lib.CH_ERR_INVALID
        eio = _lib.ChMarlEvalIO()
        eio.step, eio.policy_out, eio.env_actions = ctypes.pointer(sio), io.policy_out, io.env_actions
        assert evaluate(b, policy, eio) == _lib.CH_ERR_INVALID
    # a policy narrower than one agent's action
    narrow = DevicePolicy(DevicePolicy.random_layers([86, 64, 3], seed=3), "tanh", None)
    narrow._ensure_packed()
    assert evaluate(b, narrow, io) == _lib.CH_ERR_INVALID
    assert b"at least 4 wide" in L.ch_last_error(b.handle)
    # nothing of the above ran a step or touched the table
    b.torch.cuda.synchronize()
    assert int(table.remaining.item()) == E and int(table.count.sum().item()) == 0
    assert int(table.acc_steps.sum().item()) == 0 and int(b.env_ints()["step_index"].sum()) == 0
    assert evaluate(b, policy, io) == _lib.CH_OK and steps.value == 4
    assert int(table.acc_steps.sum().item()) + int(table.count.sum().item()) > 0
    b.close()
