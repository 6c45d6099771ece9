"""GPU tests of the population collection (ch_rollout_collect_pop; cattleherd.rollout_pop.PopulationRollout): P members'
policies collect on one batch of P * E envs, member p on envs [pE, (p + 1)E).

The reference throughout is the existing solo path, DeviceRolloutBuffer(HerdBatch(E, ..., env_id_offset=p * E)).collect
from the same start (the same seed and config, the same step counters, so that envs hit the time limit inside the
rollout) with member p's nets, log_std, seed, gamma and gae_lambda.  The claim is bit identity, so every comparison is
rollout_ref.bits_equal (which compares NaNs by position) on every buffer array, on last_episode_starts and on the final
env state of the slice; there is no tolerance.

Shapes are the smallest that can still go wrong: 2 drones x 8 cattle with NaN-safe rewards; E = 24 (a tail tile inside
every member, member boundaries off the 16-row grid), 16 (exactly one tile) and 8 (less than one); T = 19 crosses the
16-step flush period of the deferred truncation bootstrap, so a mid-collection flush and the tail flush both run."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, LEVEL = 2, 8, 7
ARRAYS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns",
          "last_episode_starts")
# the driver's nets at 2 drones ({R * 86, 128, 128, 48} / {..., 1}), and odd hidden widths (no multiple of 16 or of 8:
# ragged tiles, which k_mlp2 takes from packed weights) with an odd action width
ARCH = {"driver": ((128, 128), (128, 128), 48), "odd": ((76, 44), (52, 20), 9)}
GAMMAS, LAMBDAS = (0.99, 0.95, 0.9, 0.97), (0.95, 0.9, 0.8, 0.92)
GUARD = 64   # floats of NaN on either side of every member array (a multiple of 4: obs stays 16-byte aligned)


def step_counters(E, P, T):
    """Every member: env e passes the 80 s time limit (step_counter / 60 > 80; a CTDE step adds 4) after e % T + 1 steps
    of the rollout, so with E >= T there are truncations at every step, before and after the flush at step 16."""
    return np.tile(4800 - 2 - 4 * (np.arange(E) % T), P)


def nets(arch, p, weights=0):
    import torch
    from cattleherd.policy import DevicePolicy
    pi, vf, A = ARCH[arch]
    actor = DevicePolicy(DevicePolicy.random_layers([12 * 86, *pi, A], seed=10 + p + 100 * weights), "tanh", None)
    critic = DevicePolicy(DevicePolicy.random_layers([12 * 86, *vf, 1], seed=20 + p + 100 * weights), "tanh", None)
    log_std = (-1.0 - 0.1 * p + 0.01 * torch.arange(A, dtype=torch.float32)).cuda()
    return actor, critic, log_std


def batch(E, offset, sc):
    from cattleherd.env import HerdBatch
    b = HerdBatch(E, N, M, mode="ctde", curriculum_level=LEVEL, compat=False, env_id_offset=offset)
    b.reset()
    b.set_state({"step_counter": sc})
    return b


def env_state(b, lo, hi):
    n = b.n_envs
    return {k: np.array(v)[lo:hi] for k, v in b.get_state().items() if np.ndim(v) and np.shape(v)[0] == n}


@functools.lru_cache(maxsize=None)
def solo(arch, E, P, T, boot, p, weights=0, seed=None):
    """The reference: member p alone on a batch of its own.  Computed once per case and shared; nothing changes it."""
    import torch
    from cattleherd.rollout import DeviceRolloutBuffer
    b = batch(E, p * E, step_counters(E, P, T)[p * E:(p + 1) * E])
    actor, critic, log_std = nets(arch, p, weights)
    rb = DeviceRolloutBuffer(b, T, act_dim=ARCH[arch][2], gamma=GAMMAS[p], gae_lambda=LAMBDAS[p])
    rb.collect(actor, critic, log_std, seed=100 + p if seed is None else seed, bootstrap_truncated=boot)
    torch.cuda.synchronize()
    out = {k: getattr(rb, k).cpu().numpy() for k in ARRAYS}
    out["state"] = env_state(b, 0, E)
    b.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def guard_bands(pop):
    """Every member array moved into the middle of a NaN-filled allocation; returns the allocations."""
    import torch
    bigs = []
    for rb in pop.members:
        for k in ARRAYS:
            t = getattr(rb, k)
            big = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=t.device)
            view = big[GUARD:GUARD + t.numel()].view(t.shape)
            view.copy_(t)
            setattr(rb, k, view)
            bigs.append(big)
    return bigs


def population(arch, E, P, T, boot, guard=False, changed=None):
    """One population collection; `changed`: the member whose weights and seed differ from the reference's."""
    import torch
    from cattleherd.rollout_pop import PopulationRollout
    b = batch(P * E, 0, step_counters(E, P, T))
    pop = PopulationRollout(b, P, T, act_dim=ARCH[arch][2], gammas=GAMMAS[:P], gae_lambdas=LAMBDAS[:P])
    bigs = guard_bands(pop) if guard else []
    ms = [nets(arch, p, int(p == changed)) for p in range(P)]
    seeds = [100 + p + (1000 if p == changed else 0) for p in range(P)]
    pop.collect([m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms], seeds, bootstrap_truncated=boot)
    torch.cuda.synchronize()
    out = []
    for p, rb in enumerate(pop.members):
        d = {k: getattr(rb, k).cpu().numpy() for k in ARRAYS}
        d["state"] = env_state(b, p * E, (p + 1) * E)
        out.append(d)
    for big in bigs:
        big = big.cpu().numpy()
        assert np.isnan(big[:GUARD]).all() and np.isnan(big[-GUARD:]).all()
    pop.close()
    b.close()
    return out


def assert_member_equal(got, want, who):
    from rollout_ref import bits_equal
    for k in ARRAYS:
        assert bits_equal(got[k], want[k]), (who, k)
    assert got["state"].keys() == want["state"].keys() and got["state"]
    for k, v in want["state"].items():
        assert np.array_equal(got["state"][k], v, equal_nan=np.issubdtype(v.dtype, np.floating)), (who, "state", k)


@pytest.mark.parametrize("arch", ["driver", "odd"])
def test_population_equals_solo_across_the_flush(arch):
    """P = 3, E = 24, T = 19, members differing in weights, log_std, seed, gamma and gae_lambda; NaN guard bands around
    every member array stay NaN."""
    E, P, T = 24, 3, 19
    got = population(arch, E, P, T, True, guard=True)
    for p in range(P):
        want = solo(arch, E, P, T, True, p)
        es = want["episode_starts"]
        # the queue is not empty on either side of the mid-collection flush (it follows step 16's forward, whose post
        # is step 15's): an env of this member was done at a step <= 15 and at a step >= 16.  A done here is the time
        # limit (the step counters), and the bootstrap shows: those rewards differ from a collection without it
        assert es[1:17].any() and (es[17:].any() or want["last_episode_starts"].any()), p
        plain = solo(arch, E, P, T, False, p)
        assert (plain["rewards"][:16] != want["rewards"][:16]).any() and (plain["rewards"][16:] != want["rewards"][16:]).any()
        assert_member_equal(got[p], want, (arch, p))


@pytest.mark.parametrize("arch", ["driver", "odd"])
def test_population_equals_solo_without_bootstrap(arch):
    E, P, T = 24, 3, 5
    got = population(arch, E, P, T, False)
    for p in range(P):
        assert_member_equal(got[p], solo(arch, E, P, T, False, p), (arch, p))


def test_population_of_one_equals_solo():
    got = population("driver", 24, 1, 19, True)
    assert_member_equal(got[0], solo("driver", 24, 1, 19, True, 0), 0)


@pytest.mark.parametrize("E", [16, 8])
def test_member_of_one_tile_and_less(E):
    P, T = 4, 19
    got = population("driver", E, P, T, True, guard=True)
    for p in range(P):
        assert_member_equal(got[p], solo("driver", E, P, T, True, p), (E, p))


def test_changing_one_member_leaves_the_others_alone():
    """Member 1's weights and seed changed: members 0 and 2 are bit-identical to the reference, member 1 is its own
    solo run with the changed nets."""
    from rollout_ref import bits_equal
    E, P, T = 24, 3, 19
    got = population("driver", E, P, T, True, changed=1)
    for p in (0, 2):
        assert_member_equal(got[p], solo("driver", E, P, T, True, p), p)
    assert not bits_equal(got[1]["actions"], solo("driver", E, P, T, True, 1)["actions"])
    assert_member_equal(got[1], solo("driver", E, P, T, True, 1, 1, 1101), "changed")


def test_three_collections_queued_back_to_back():
    """Three collections queued without a host synchronisation in between (the third reuses the first's table slot
    while the first two may still be queued) equal three synchronised ones."""
    import torch
    from rollout_ref import bits_equal
    from cattleherd.rollout_pop import PopulationRollout
    E, P, T = 24, 3, 6
    runs = []
    for sync in (True, False):
        b = batch(P * E, 0, step_counters(E, P, T))
        pops = [PopulationRollout(b, P, T, act_dim=48, gammas=GAMMAS[:P], gae_lambdas=LAMBDAS[:P]) for _ in range(3)]
        ms = [nets("driver", p) for p in range(P)]
        for i, q in enumerate(pops):
            q.collect([m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms], [7 * i + p for p in range(P)])
            if i == 0:   # one set of tables for the three calls
                for r in pops[1:]:
                    r._lib, r._pop = q._lib, q._pop
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        runs.append([{k: getattr(rb, k).cpu().numpy() for k in ARRAYS} for q in pops for rb in q.members])
        for q in pops[1:]:
            q._pop = ctypes.c_void_p()   # (the first owns the tables)
        pops[0].close()
        b.close()
    assert len(runs[0]) == 9
    for a, c in zip(*runs):
        for k in ARRAYS:
            assert bits_equal(c[k], a[k]), k
    assert not bits_equal(runs[0][0]["actions"], runs[0][3]["actions"])   # (the calls differ: another seed, a later state)


SENTINEL = 777.0


def test_error_paths_launch_nothing():
    """Every rejection: the return code, a non-empty ch_last_error, and buffers (pre-filled with a sentinel) untouched."""
    import torch
    from cattleherd import _lib as L
    from cattleherd.env import HerdBatch
    from cattleherd.rollout import ChRolloutIO
    from cattleherd.rollout_pop import ChRolloutMember, PopulationRollout, _bind
    E, P, T = 24, 3, 4
    b = batch(P * E, 0, step_counters(E, P, T))
    marl = HerdBatch(8, N, M, mode="marl")
    marl.reset()
    pop = PopulationRollout(b, P, T, act_dim=48)
    ms = [nets("driver", p) for p in range(P)]
    for m in ms:
        m[0]._ensure_packed()
        m[1]._ensure_packed()
    other_arch = nets("odd", 0)[0]
    other_arch._ensure_packed()
    for rb in pop.members:
        for k in ARRAYS:
            getattr(rb, k).fill_(SENTINEL)
    lib = _bind()
    tables, small = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.ch_rollout_pop_create(8, 0, ctypes.byref(tables)) == 0
    assert lib.ch_rollout_pop_create(2, 0, ctypes.byref(small)) == 0

    def members():
        arr = (ChRolloutMember * P)()
        for mb, rb, m, p in zip(arr, pop.members, ms, range(P)):
            mb.rb = rb.struct()
            mb.actor, mb.critic = ctypes.pointer(m[0]._net), ctypes.pointer(m[1]._net)
            mb.log_std, mb.seed, mb.gamma, mb.gae_lambda = m[2].data_ptr(), p, 0.99, 0.95
        return arr

    def io_of(bb):
        io = ChRolloutIO()
        bb._io.terminal_obs, bb._io.reset_happened = bb.terminal_obs.data_ptr(), bb.reset_happened.data_ptr()
        io.step = ctypes.pointer(bb._io)
        io.mean, io.value = pop.mean.data_ptr(), pop.value.data_ptr()
        io.terminal_value, io.env_actions = pop.terminal_value.data_ptr(), pop.env_actions.data_ptr()
        return io

    def call(code, h=b, tab=tables, arr="ok", n=P, io="ok", edit=None):
        arr = members() if arr == "ok" else arr
        if edit:
            edit(arr)
        io = io_of(h) if io == "ok" else io
        rc = lib.ch_rollout_collect_pop(h.handle, tab, arr, n, None if io is None else ctypes.byref(io), 1, None)
        assert rc == code, (rc, code, lib.ch_last_error(h.handle))
        assert lib.ch_last_error(h.handle), "the rejection says why"
        return lib.ch_last_error(h.handle).decode()

    INV, UNS = L.CH_ERR_INVALID, L.CH_ERR_UNSUPPORTED
    assert "NULL" in call(INV, tab=None)
    assert "NULL" in call(INV, arr=None)
    assert "NULL" in call(INV, io=None)
    assert "n_members" in call(INV, n=0)
    assert "n_members" in call(INV, tab=small)
    assert "divide" in call(INV, n=5, arr=(ChRolloutMember * 5)(*members(), *members()[:2]))
    assert "CTDE" in call(UNS, h=marl, n=2)
    assert "critic" in call(INV, edit=lambda a: setattr(a[1], "critic", None))
    assert "architecture" in call(INV, edit=lambda a: setattr(a[2], "actor", ctypes.pointer(other_arch._net)))

    def n_steps(a):
        a[1].rb.n_steps = T - 1
    assert "n_steps" in call(INV, edit=n_steps)

    def act_dim(a):
        a[2].rb.act_dim = 47
    assert "act_dim" in call(INV, edit=act_dim)
    # raw weights with ragged hidden widths are k_mlp's, not k_mlp2's: there is no fallback path here
    raw = nets("odd", 0)
    pop9 = PopulationRollout(b, P, T, act_dim=9)
    for rb in pop9.members:
        for k in ARRAYS:
            getattr(rb, k).fill_(SENTINEL)

    unpacked = []
    for net in raw[:2]:   # the same nets without their packed copy: nn.Linear rows only
        c = L.ChMlp()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(net._net), ctypes.sizeof(c))
        c.packed = None
        unpacked.append(c)

    def ragged(a):
        for mb, rb in zip(a, pop9.members):
            mb.rb = rb.struct()
            mb.actor, mb.critic = ctypes.pointer(unpacked[0]), ctypes.pointer(unpacked[1])
    assert "k_mlp2" in call(UNS, edit=ragged)

    def misaligned(a):
        a[1].rb.obs += 4
    assert "aligned" in call(INV, edit=misaligned)

    def shared(a):
        a[2].rb.rewards = a[0].rb.rewards
    assert "shared" in call(INV, edit=shared)
    torch.cuda.synchronize()
    for q in (pop, pop9):
        for rb in q.members:
            for k in ARRAYS:
                assert bool((getattr(rb, k) == SENTINEL).all()), k
    assert lib.ch_rollout_pop_destroy(tables) == 0 and lib.ch_rollout_pop_destroy(small) == 0
    marl.close()
    b.close()


def test_collect_and_train_equal_the_solo_chain():
    """P = 2, E = 32, T = 8, batch_size 64, n_epochs 2: PopulationRollout.collect + PPOPopulation.train(pop.members)
    leaves every member's parameters and Adam state bit-equal to the solo collect + PPOUpdate.train chain."""
    import torch
    from cattleherd.ppo import PPOUpdate, SB3ActorCritic
    from cattleherd.ppo_pop import PPOPopulation
    from cattleherd.rollout import DeviceRolloutBuffer
    from cattleherd.rollout_pop import PopulationRollout
    E, P, T = 32, 2, 8
    sc = step_counters(E, P, T)

    def updates():
        return [PPOUpdate(SB3ActorCritic(obs_dim=12 * 86, act_dim=4 * N, device="cuda:0", seed=50 + p),
                          learning_rate=(3e-4, 1e-3)[p], n_epochs=2, batch_size=64, seed=7 + p, backend="native")
                for p in range(P)]
    alone, together = updates(), updates()
    for p, u in enumerate(alone):
        b = batch(E, p * E, sc[p * E:(p + 1) * E])
        actor, critic, log_std = u.model.device_nets()
        rb = DeviceRolloutBuffer(b, T, gamma=GAMMAS[p], gae_lambda=LAMBDAS[p])
        rb.collect(actor, critic, log_std, seed=100 + p)
        u.train(rb)
        torch.cuda.synchronize()
        b.close()
    b = batch(P * E, 0, sc)
    pop = PopulationRollout(b, P, T, gammas=GAMMAS[:P], gae_lambdas=LAMBDAS[:P])
    dn = [u.model.device_nets() for u in together]
    pop.collect([d[0] for d in dn], [d[1] for d in dn], [d[2] for d in dn], [100 + p for p in range(P)])
    population = PPOPopulation(together)
    population.train(pop.members)
    torch.cuda.synchronize()

    def same(x, y):
        return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    for a, c in zip(together, alone):
        assert all(same(x.detach(), y.detach()) for x, y in zip(a.model.parameters(), c.model.parameters()))
        assert same(a.exp_avg, c.exp_avg) and same(a.exp_avg_sq, c.exp_avg_sq)
        assert a.n_updates == c.n_updates and a.sgd_steps == c.sgd_steps
    assert not same(together[0].model.log_std.detach(), updates()[0].model.log_std.detach())   # the update is live
    population.close()
    pop.close()
    b.close()
