"""The population collection's host side on the CPU: the ctypes layout of ch_rollout_member against the header, the
Python-side ValueErrors of cattleherd.rollout_pop.PopulationRollout (on tests/fake_batch.py's stand-in batch), the
member-slice arithmetic as a pure function against the library's own (ch__rollout_pop_slice), and the rejections of
the C ABI that need no device."""
import ctypes
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cattleherd.h")


def test_member_struct_layout_is_the_header():
    """ch_rollout_member: the buffer by value, two net pointers, log_std, the seed, two floats -- in the header's order."""
    from cattleherd import rollout, rollout_pop
    M = rollout_pop.ChRolloutMember
    text = open(HEADER).read()
    body = re.search(r"typedef struct ch_rollout_member \{(.*?)\} ch_rollout_member;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f[0] for f in M._fields_] == ["rb", "actor", "critic", "log_std", "seed", "gamma", "gae_lambda"]
    assert M.rb.offset == 0 and ctypes.sizeof(rollout.ChRollout) == 8 + 9 * 8
    assert M.actor.offset == ctypes.sizeof(rollout.ChRollout) and M.critic.offset == M.actor.offset + 8
    assert M.log_std.offset == M.critic.offset + 8 and M.seed.offset == M.log_std.offset + 8
    assert M.gamma.offset == M.seed.offset + 8 and M.gae_lambda.offset == M.gamma.offset + 4
    assert ctypes.sizeof(M) == M.seed.offset + 16
    for sym in ("ch_rollout_pop_create", "ch_rollout_pop_destroy", "ch_rollout_collect_pop"):
        assert re.search(r"\bint " + sym + r"\(", text), sym


@pytest.mark.parametrize("n_envs,P,rows,drones,act", [(72, 3, 12, 2, 8), (64, 4, 12, 2, 48), (32, 4, 12, 4, 16),
                                                      (24, 1, 12, 2, 8), (3 * 40000, 3, 12, 12, 48)])
def test_member_slices_are_the_librarys(n_envs, P, rows, drones, act):
    """Member p's rows start at p * E in every array, scaled by the array's row width; the queue share is E times the
    solo flush period (16 steps, fewer once 16 * E observation rows would pass 1 GiB: the last case)."""
    from cattleherd import rollout_pop
    E = n_envs // P
    every = min(16, max(1, 2 ** 30 // (E * rows * 86 * 4)))
    assert every == (16 if E < 16000 else 6)
    for p in range(P):
        want = {"n_envs": E, "obs": p * E * rows * 86, "mean": p * E * act, "row": p * E,
                "env_actions": p * E * drones * 4, "flags": p * E, "queue": p * E * every}
        assert rollout_pop.member_slices(n_envs, P, p, rows, drones, act) == want
        assert rollout_pop.lib_member_slices(n_envs, P, p, rows, drones, act) == want
    # consecutive members tile the arrays: nothing shared, nothing skipped
    ends = [rollout_pop.member_slices(n_envs, P, p, rows, drones, act)["obs"] + E * rows * 86 for p in range(P)]
    assert ends[-1] == n_envs * rows * 86 and all(
        rollout_pop.member_slices(n_envs, P, p + 1, rows, drones, act)["obs"] == ends[p] for p in range(P - 1))


def test_member_slices_reject_bad_arguments():
    from cattleherd import _lib, rollout_pop
    for bad in ((10, 3, 0), (12, 3, 3), (12, 3, -1), (12, 0, 0), (0, 1, 0)):
        with pytest.raises(ValueError):
            rollout_pop.member_slices(bad[0], bad[1], bad[2], 12, 2, 8)
        with pytest.raises(_lib.ChError):
            rollout_pop.lib_member_slices(bad[0], bad[1], bad[2], 12, 2, 8)


def test_python_side_value_errors():
    import torch
    from fake_batch import FakeBatch
    from cattleherd.rollout_pop import PopulationRollout
    b = FakeBatch(6, 2, 8, mode="ctde")
    with pytest.raises(ValueError, match="divide evenly"):
        PopulationRollout(b, 4, 5)
    for P in (0, -1, 65536):
        with pytest.raises(ValueError, match="n_members"):
            PopulationRollout(b, P, 5)
    with pytest.raises(ValueError, match="n_steps"):
        PopulationRollout(b, 3, 0)
    with pytest.raises(ValueError, match="CTDE"):
        PopulationRollout(FakeBatch(6, 2, 8, mode="marl"), 3, 5)
    with pytest.raises(ValueError, match="gammas"):
        PopulationRollout(b, 3, 5, gammas=[0.99, 0.9])
    with pytest.raises(ValueError, match="gae_lambdas"):
        PopulationRollout(b, 3, 5, gae_lambdas=[0.95] * 4)
    pop = PopulationRollout(b, 3, 5, gammas=[0.99, 0.9, 0.95], gae_lambdas=0.9)
    assert len(pop.members) == 3 and pop.member_envs == 2 and pop.act_dim == 8
    for rb, g in zip(pop.members, (0.99, 0.9, 0.95)):
        assert (rb.T, rb.gamma, rb.gae_lambda, rb.act_dim) == (5, g, 0.9, 8)
        assert rb.obs.shape == (5, 2, 12 * 86) and rb.actions.shape == (5, 2, 8) and rb.obs.is_contiguous()
        for k in ("rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            assert getattr(rb, k).shape == (5, 2)
        assert torch.equal(rb.last_episode_starts, torch.ones(2))
    assert pop.mean.shape == (6, 8) and pop.value.shape == (6, 1) and pop.env_actions.shape == (6, 2, 4)
    ls = [torch.zeros(8)] * 3
    for args in (([1, 2], [1, 2, 3], ls, [0, 1, 2]), ([1, 2, 3], [1, 2], ls, [0, 1, 2]),
                 ([1, 2, 3], [1, 2, 3], ls[:2], [0, 1, 2]), ([1, 2, 3], [1, 2, 3], ls, [0])):
        with pytest.raises(ValueError, match="per member"):
            pop.collect(*args)
    with pytest.raises(ValueError, match="critic"):
        pop.collect([1, 2, 3], [1, None, 3], ls, [0, 1, 2])


def test_host_checks_need_no_device():
    """The object-free rejections come before any device call."""
    from cattleherd import _lib, rollout_pop
    L = rollout_pop._bind()
    assert L.ch_rollout_pop_create(0, 0, ctypes.byref(ctypes.c_void_p())) == _lib.CH_ERR_INVALID
    assert L.ch_last_error(None).startswith(b"ch_rollout_pop_create: ")
    assert L.ch_rollout_pop_create(65536, 0, ctypes.byref(ctypes.c_void_p())) == _lib.CH_ERR_INVALID
    assert L.ch_rollout_pop_create(2, 0, None) == _lib.CH_ERR_INVALID
    assert L.ch_rollout_collect_pop(None, None, None, 1, None, 1, None) == _lib.CH_ERR_INVALID
    assert L.ch_last_error(None).startswith(b"ch_rollout_collect_pop: ")
    assert L.ch_rollout_pop_destroy(None) == _lib.CH_ERR_INVALID
    assert set(_lib._ROLLOUT_POP_EXPORTS) <= set(_lib.EXPORTS)


def test_ppo_update_takes_its_row_count_from_the_buffer():
    """PPOUpdate._flat flattens [T, E, ...] by the buffer's own shape: a population member's buffer has no batch."""
    import torch
    from cattleherd.ppo import PPOUpdate
    from cattleherd.rollout_pop import MemberBuffer
    rb = MemberBuffer(torch, torch.device("cpu"), 3, 5, 12 * 86, 8, 0.99, 0.95)
    flat = PPOUpdate._flat(None, rb)
    assert [tuple(t.shape) for t in flat] == [(15, 1032), (15, 8), (15,), (15,), (15,)]
    assert flat[0].data_ptr() == rb.obs.data_ptr()
