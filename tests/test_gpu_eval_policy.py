"""GPU tests of the on-device evaluate_policy (cattleherd.eval_policy; ch_eval_begin, ch_eval_record,
ch_evaluate_policy) against tests/eval_ref.py, the numpy restatement of SB3's evaluate_policy bookkeeping.  Everything
compared is integer bookkeeping or a float64 copied from the step's own outputs, so every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from eval_ref import EvalRef

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, T = 4, 16, 6


def _assert_tables(got, want, what=""):
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{what} {k}"


def _assert_episodes(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


# ---- 1. the recorder alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 257])
def test_recorder_equals_sb3_bookkeeping_after_every_step(E, C):
    """ch_eval_begin / ch_eval_record on synthetic step outputs: 40 steps of seeded random reset_happened (p = 0.3),
    episode statistics and flags; after every step every table array and ``remaining`` equal the reference exactly.
    E covers one partial wave, one wave less / exactly / plus one lane, and two workgroups (257 > 256 threads).
    Every case has an env that ends again after reaching its quota; the cases with n < E (every E > 1) have envs of
    quota 0 that end too -- both asserted on the reference."""
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.eval_policy import DeviceEvalTable
    S = 40
    rng = np.random.default_rng(1000 * E + C)
    rh = (rng.random((S, E)) < 0.3).astype(np.uint8)
    stats = np.stack([rng.normal(0.0, 100.0, (S, E)), rng.integers(1, 1203, (S, E)).astype(np.float64)], -1)
    te, tr = (rng.random((S, E)) < 0.5).astype(np.uint8), (rng.random((S, E)) < 0.5).astype(np.uint8)
    b = HerdBatch(E, N, M, mode="ctde")
    dev = [torch.as_tensor(np.ascontiguousarray(a)).to(b.device) for a in (rh, stats, te, tr)]
    saw_full = saw_zero = False
    for n in sorted({1, E - 1, E, min(2 * E + 3, C * E)} - {0}):
        table = DeviceEvalTable(b, C).begin(n)
        ref = EvalRef(n, E, C)
        _assert_tables(table.arrays(), ref.arrays(), f"n={n} begin")
        io = _lib.ChStepIO()
        for t in range(S):
            io.reset_happened, io.episode_stats = dev[0][t].data_ptr(), dev[1][t].data_ptr()
            io.terminated, io.truncated = dev[2][t].data_ptr(), dev[3][t].data_ptr()
            table.record(t, io)
            ref.step(rh[t], stats[t], te[t], tr[t], t)
            _assert_tables(table.arrays(), ref.arrays(), f"n={n} step {t}")
        _assert_episodes(table.episodes(), ref.episodes())
        assert ref.ignored_full > 0
        saw_full = True
        saw_zero |= ref.ignored_zero > 0
    assert saw_full and (saw_zero or E == 1)   # (one env: n >= 1 leaves no quota of 0)
    b.close()


# ---- the three loops -----------------------------------------------------------------------------------------------
def _actor(width):
    import torch
    from cattleherd.policy import DevicePolicy
    if width == 16:
        return DevicePolicy(DevicePolicy.random_layers([12 * 86, 128, 128, 16], seed=1), "tanh", None)
    d = np.load(os.path.join(ROOT, "tests", "golden", "policy_ctde_v16_6.npz"))
    return DevicePolicy.sb3_actor({k.replace("__", "."): torch.tensor(d[k]) for k in d.files if "__" in k}, clip=False)


def _inject(b, E):
    # every env reaches its time limit within T steps (test_native_collect_equals_python_loop's injection)
    b.set_state({"step_counter": 4800 - T // 2 + (np.arange(E) % T)})


def _batch(E, level):
    from cattleherd.env import HerdBatch
    b = HerdBatch(E, N, M, mode="ctde", curriculum_level=level)
    b.reset()
    _inject(b, E)
    return b


def _host_loop(b, actor, ref, max_steps, check_every=16, first_step_index=0):
    """The evaluation as a host program: the device steps, SB3's bookkeeping (EvalRef) on every step's outputs pulled
    to the host.  Returns (the steps a loop that looks at ``remaining`` every check_every steps runs, the step count
    at which the last quota filled or None)."""
    t, filled = 0, None
    while t < max_steps:
        mean = actor.forward_batch(b)
        b.step(mean[:, :N * 4].clamp(-1.0, 1.0).reshape(b.n_envs, N, 4).contiguous(), autoreset=True, terminal_obs=False)
        ref.step(b.reset_happened.cpu().numpy(), b.episode_stats.cpu().numpy(), b.terminated.cpu().numpy(),
                 b.truncated.cpu().numpy(), first_step_index + t)
        t += 1
        if filled is None and not ref.running():
            filled = t
        if (t % check_every == 0 or t == max_steps) and not ref.running():
            break
    return t, filled


def _run_three(E, level, width, n, C, max_steps, check_every=16):
    """Native loop, Python loop and host reference from the same state; returns their (arrays, episodes, steps, rem)."""
    from cattleherd.eval_policy import DeviceEvalTable
    out = []
    for path in ("run", "run_steps"):
        b = _batch(E, level)
        table = DeviceEvalTable(b, C).begin(n)
        steps, rem = getattr(table, path)(_actor(width), max_steps, check_every)
        out.append((table.arrays(), table.episodes(), steps, rem))
        b.close()
    b = _batch(E, level)
    ref = EvalRef(n, E, C)
    steps, filled = _host_loop(b, _actor(width), ref, max_steps, check_every)
    out.append((ref.arrays(), ref.episodes(), steps, ref.remaining))
    b.close()
    return out, filled


@pytest.mark.parametrize("n_kind", ["E", "half"])
@pytest.mark.parametrize("level,width", [(2, 16), (7, 48)], ids=["random16_level2", "v16_6_48wide_level7"])
def test_native_loop_equals_python_loop_equals_host_reference(level, width, n_kind):
    """ch_evaluate_policy, the same kernels launched from Python, and SB3's bookkeeping on the host fill identical
    tables: 64 envs whose time limits fall inside the T = 6 steps, n = E (every quota 1) and n = E / 2 + 3 (the first
    29 envs have quota 0).  The 48-wide v16-6 actor (clip off) at level 7 uses the slice and the clamp."""
    E = 64
    n = E if n_kind == "E" else E // 2 + 3
    (nat, py, ref), _ = _run_three(E, level, width, n, 1, T)
    assert ref[3] == 0 and len(ref[1][0]) == n          # the injected state ends every counted episode within T
    assert nat[2] == py[2] == ref[2] == T and nat[3] == py[3] == 0
    _assert_tables(nat[0], py[0], "native vs python")
    _assert_tables(nat[0], ref[0], "native vs reference")
    _assert_episodes(nat[1], ref[1])
    _assert_episodes(py[1], ref[1])
    if width == 48:
        assert _actor(48).dims[-1] == 48 and _actor(48).clip is None


def test_two_episodes_per_env_across_a_resumed_call():
    """C = 2, n = 2 E: the first call (max_steps = T) leaves remaining = E; with the time limits injected again, a
    second call with first_step_index = steps_run fills every env's second slot.  Equal to the reference driven the
    same way."""
    from cattleherd.eval_policy import DeviceEvalTable
    E = 64
    b = _batch(E, 2)
    actor = _actor(16)
    table = DeviceEvalTable(b, 2).begin(2 * E)
    s1, rem = table.run(actor, T)
    assert (s1, rem) == (T, E)
    _inject(b, E)
    s2, rem = table.run(actor, T, first_step_index=s1)
    assert (s2, rem) == (T, 0)
    got, eps = table.arrays(), table.episodes()
    b.close()
    assert np.array_equal(got["count"], np.full(E, 2, np.int32)) and got["remaining"].tolist() == [0]
    b = _batch(E, 2)
    ref = EvalRef(2 * E, E, 2)
    r1, _ = _host_loop(b, _actor(16), ref, T)
    assert ref.remaining == E
    _inject(b, E)
    _host_loop(b, _actor(16), ref, T, first_step_index=r1)
    b.close()
    _assert_tables(got, ref.arrays())
    _assert_episodes(eps, ref.episodes())
    assert eps[4].min() < s1 <= eps[4].max()   # end steps from both calls


@pytest.mark.parametrize("check_every", [1, 5, 16])
def test_check_every_changes_the_steps_run_and_not_the_table(check_every):
    """The loop looks at ``remaining`` only every check_every steps: steps_run is the first multiple of check_every
    at or after the step that filled the last quota (capped at max_steps), and the steps past that one leave the
    table as it was."""
    E = 64
    (nat, py, ref), filled = _run_three(E, 7, 16, E, 1, T, check_every)
    assert filled is not None and 1 < filled < 5     # the injected counters end the last episode at step 2
    want = min(T, -(-filled // check_every) * check_every)
    assert nat[2] == py[2] == ref[2] == want
    assert nat[3] == py[3] == 0
    _assert_tables(nat[0], py[0], "native vs python")
    _assert_tables(nat[0], ref[0], "native vs reference")
    _assert_episodes(nat[1], ref[1])


def test_step_cap_is_not_an_error_natively_and_raises_in_python():
    """max_steps = 2 from a fresh reset: no episode is over, ch_evaluate_policy returns CH_OK with remaining > 0 and
    the Python evaluate_policy raises RuntimeError naming remaining."""
    from cattleherd.env import HerdBatch
    from cattleherd.eval_policy import DeviceEvalTable, evaluate_policy
    E = 64
    b = HerdBatch(E, N, M, mode="ctde", curriculum_level=2)
    b.reset()
    actor = _actor(16)
    table = DeviceEvalTable(b, 1).begin(E)
    steps, rem = table.run(actor, 2, check_every=16)
    assert steps == 2 and 0 < rem <= E and rem == int(table.remaining.item())
    with pytest.raises(RuntimeError, match="remaining = "):
        evaluate_policy(b, actor, n_eval_episodes=E, max_steps=2)
    b.close()


def test_rejections():
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.eval_policy import DeviceEvalTable
    from cattleherd.policy import DevicePolicy
    L = _lib.lib()
    E = 8
    b = HerdBatch(E, N, M, mode="ctde")
    b.reset()
    table = DeviceEvalTable(b, 1)
    actor = _actor(16)
    actor._ensure_packed()
    io = _lib.ChEvalIO()
    io.step = ctypes.pointer(b._io)
    mean = b.torch.zeros((E, 16), dtype=b.torch.float32, device=b.device)
    io.mean, io.env_actions = mean.data_ptr(), table.env_actions.data_ptr()
    steps, rem = ctypes.c_int64(), ctypes.c_int64()

    def evaluate(handle, net, eio):
        return L.ch_evaluate_policy(handle, ctypes.byref(net._net), ctypes.byref(table._tb), ctypes.byref(eio), 4, 1, 0,
                                    ctypes.byref(steps), ctypes.byref(rem), b._stream())

    # a MARL handle: CH_ERR_UNSUPPORTED from all three
    m = HerdBatch(E, N, M, mode="marl")
    with pytest.raises(ValueError):
        DeviceEvalTable(m, 1)
    assert L.ch_eval_begin(m.handle, ctypes.byref(table._tb), E, m._stream()) == _lib.CH_ERR_UNSUPPORTED
    assert L.ch_eval_record(m.handle, ctypes.byref(table._tb), m._io_ref, 0, m._stream()) == _lib.CH_ERR_UNSUPPORTED
    assert evaluate(m.handle, actor, io) == _lib.CH_ERR_UNSUPPORTED
    assert b"CTDE" in L.ch_last_error(m.handle)
    m.close()
    # more episodes per env than slots
    with pytest.raises(_lib.ChError, match="capacity") as ei:
        table.begin(E + 1)
    assert ei.value.code == _lib.CH_ERR_INVALID
    with pytest.raises(_lib.ChError) as ei:
        table.begin(0)
    assert ei.value.code == _lib.CH_ERR_INVALID
    table.begin(E)
    # a step io without reset_happened / episode_stats
    for field in ("reset_happened", "episode_stats"):
        sio = _lib.ChStepIO()
        ctypes.memmove(ctypes.byref(sio), ctypes.byref(b._io), ctypes.sizeof(sio))
        setattr(sio, field, None)
        with pytest.raises(_lib.ChError, match=field) as ei:
            table.record(0, sio)
        assert ei.value.code == _lib.CH_ERR_INVALID
        eio = _lib.ChEvalIO()
        eio.step, eio.mean, eio.env_actions = ctypes.pointer(sio), io.mean, io.env_actions
        assert evaluate(b.handle, actor, eio) == _lib.CH_ERR_INVALID
    # an actor narrower than the env's action
    narrow = DevicePolicy(DevicePolicy.random_layers([12 * 86, 64, 4 * N - 4], seed=3), "tanh", None)
    narrow._ensure_packed()
    assert evaluate(b.handle, narrow, io) == _lib.CH_ERR_INVALID
    assert b"num_drones * 4 = 16" in L.ch_last_error(b.handle)
    # nothing of the above ran a step or touched the table
    b.torch.cuda.synchronize()
    assert int(table.remaining.item()) == E and int(table.count.sum().item()) == 0
    assert evaluate(b.handle, actor, io) == _lib.CH_OK and steps.value == 4
    b.close()


def test_live_weights_are_seen():
    """An SB3ActorCritic's actor is read over its live storage and re-packed per evaluation: after
    ``action_net.bias.data += 0.5`` the native evaluation changes, and equals evaluate_policy_steps (which re-packs
    before every forward) run after the same change from the same state."""
    from cattleherd.eval_policy import evaluate_policy, evaluate_policy_steps
    from cattleherd.ppo import SB3ActorCritic
    E = 64
    model = SB3ActorCritic(obs_dim=12 * 86, act_dim=16)
    kw = dict(n_eval_episodes=E, max_steps=T, reset=False, return_episode_rewards=True, monitor_rounding=False)

    def run(fn):
        b = _batch(E, 7)
        res = fn(b, model, **kw)
        b.close()
        return res

    before = run(evaluate_policy)
    model.action_net.bias.data += 0.5
    after = run(evaluate_policy)
    steps = run(evaluate_policy_steps)
    assert len(after[0]) == E and after == steps
    assert after[0] != before[0]
