"""GPU tests of the population training log (cattleherd/train_log.py PopulationEpisodeRing, explained_variance_pop;
ch_ep_ring_pop_*, ch_rollout_collect_pop_log, ch_explained_variance_pop; PPOPopulation.train's pooled record).

The claim throughout is that every member's record is bit for bit what the solo path gives it alone, so every
comparison is exact: integers as integers, float data as bit patterns (train_log_ref.same_entries,
train_log_pop_ref.bits_equal64); there is no tolerance.  The references are the per-member deque of
tests/train_log_pop_ref.py, the solo entry points (ch_ep_ring_record on offset pointers, EpisodeRing inside
DeviceRolloutBuffer.collect, explained_variance, PPOUpdate.train) and the numpy restatement of the summary's fixed
summation order."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import train_log_pop_ref as R
import train_log_ref as T

pytestmark = pytest.mark.gpu

GUARD = 64           # elements of guard band on either side of every guarded array
ROW_F, ROW_I = 777.0, 777          # what the ring rows hold before anything is recorded
BAND_I = -77777                    # the integer guard bands (the float64 ones are NaN)


def guarded(shape, dtype, fill):
    """A tensor of `shape` in the middle of an allocation whose bands hold NaN (float) or BAND_I: (allocation, view)."""
    import torch
    n = int(np.prod(shape))
    band = float("nan") if dtype.is_floating_point else BAND_I
    big = torch.full((n + 2 * GUARD,), band, dtype=dtype, device="cuda:0")
    view = big[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return big, view


def bands_intact(big):
    a = big.cpu().numpy()
    lo, hi = a[:GUARD], a[-GUARD:]
    return bool(np.isnan(lo).all() and np.isnan(hi).all()) if a.dtype.kind == "f" else bool((lo == BAND_I).all() and (hi == BAND_I).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the recorder alone, on crafted inputs -------------------------------------------------------------------
def crafted_step(rng, P, E, s):
    """Step s: member p's role is (p + s) % P -- 0 ends nothing, 1 ends every env, 2 ends its first and its last env
    only, 3 (P = 4) a random half."""
    rh = np.zeros(P * E, np.uint8)
    roles = []
    for p in range(P):
        role = (p + s) % P
        roles.append(role)
        m = rh[p * E:(p + 1) * E]
        if role == 1:
            m[:] = 1
        elif role == 2:
            m[0] = m[E - 1] = 1
        elif role == 3:
            m[rng.choice(E, E // 2, replace=False)] = 1
    stats = np.stack([rng.normal(0.0, 100.0, P * E), rng.integers(1, 1203, P * E).astype(np.float64)], -1)
    return rh, stats, roles


@pytest.mark.parametrize("W", [100, 5, 1])
@pytest.mark.parametrize("P,E", [(3, 1500), (4, 8)])
def test_recorder_equals_the_deques_and_the_solo_recorder(P, E, W):
    """P = 3, E = 1500: every member crosses the recorder's 1024-env chunk and the member boundaries (1500, 3000) are off
    the 64-lane and the 1024-env grid; P = 4, E = 8: members smaller than a wave.  Five steps; W = 100 wraps, W = 5 and
    W = 1 have C_p > W within one step (so does W = 100 at E = 1500)."""
    import torch
    from cattleherd import _lib
    from cattleherd.env import HerdBatch
    from cattleherd.train_log import PopulationEpisodeRing
    L = _lib.lib()
    rng = np.random.default_rng(1000 * P + 10 * E + W)
    b, solo_b = HerdBatch(P * E, 2, 8, mode="ctde"), HerdBatch(E, 2, 8, mode="ctde")
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    arrays = {"ep_return": guarded((P, W), f64, ROW_F), "ep_length": guarded((P, W), i32, ROW_I),
              "ep_env": guarded((P, W), i32, ROW_I), "total": guarded((P,), i64, ROW_I)}
    ring = _lib.ChEpRingPop()
    ring.window, ring.n_members = W, P
    for k, (_, view) in arrays.items():
        setattr(ring, k, view.data_ptr())
    assert L.ch_ep_ring_pop_begin(b.handle, ctypes.byref(ring), None) == 0
    solo = []
    for p in range(P):
        t = {"ep_return": torch.full((W,), ROW_F, dtype=f64, device="cuda:0"),
             "ep_length": torch.full((W,), ROW_I, dtype=i32, device="cuda:0"),
             "ep_env": torch.full((W,), ROW_I, dtype=i32, device="cuda:0"),
             "total": torch.full((1,), ROW_I, dtype=i64, device="cuda:0")}
        r = _lib.ChEpRing()
        r.window = W
        for k, v in t.items():
            setattr(r, k, v.data_ptr())
        assert L.ch_ep_ring_begin(solo_b.handle, ctypes.byref(r), None) == 0
        solo.append((r, t))
    by_class = PopulationEpisodeRing(b, P, W).begin()
    ref = R.PopDequeRef(P, E, W)
    host = lambda: {k: v.cpu().numpy() for k, (_, v) in arrays.items()}   # noqa: E731
    seen = set()
    for s in range(5):
        rh, stats, roles = crafted_step(rng, P, E, s)
        d_rh, d_st = torch.as_tensor(rh).cuda(), torch.as_tensor(stats).cuda()
        io = _lib.ChStepIO()
        io.reset_happened, io.episode_stats = d_rh.data_ptr(), d_st.data_ptr()
        before = host()
        assert L.ch_ep_ring_pop_record(b.handle, ctypes.byref(ring), ctypes.byref(io), None) == 0, L.ch_last_error(b.handle)
        by_class.record(io)
        for p, (r, _) in enumerate(solo):
            sio = _lib.ChStepIO()
            sio.reset_happened, sio.episode_stats = d_rh.data_ptr() + p * E, d_st.data_ptr() + 16 * p * E
            assert L.ch_ep_ring_record(solo_b.handle, ctypes.byref(r), ctypes.byref(sio), None) == 0
        ref.step(rh, stats)
        torch.cuda.synchronize()
        got = host()
        for p in range(P):
            C = ref.members[p].per_step[-1]
            seen |= {"zero"} if C == 0 else {"over"} if C > W else {"some"}
            if roles[p] == 0:   # nothing ended: the row and total[p] are bitwise what they were
                assert C == 0 and all(same_bits(got[k][p], before[k][p]) for k in got), (s, p)
            assert int(got["total"][p]) == ref.members[p].total
            entries = R.ring_entries(got["ep_return"][p], got["ep_length"][p], got["ep_env"][p], got["total"][p], W)
            assert T.same_entries(entries, ref.entries(p)), (s, p)
            for k, v in solo[p][1].items():   # the whole row, the slots never written included
                assert same_bits(got[k][p].reshape(-1), v.cpu().numpy().reshape(-1)), (s, p, k)
        if s == 0:   # member 0 has ended nothing yet: its row still holds what it held before begin
            assert (got["ep_return"][0] == ROW_F).all() and (got["ep_env"][0] == ROW_I).all() and got["total"][0] == 0
    assert "zero" in seen and (E <= W or "over" in seen) and (W == 1 or "some" in seen)
    assert all(t > W for t in ref.totals()) or E == 8   # every ring wrapped (the small members at W = 100 do not)
    assert all(bands_intact(big) for big, _ in arrays.values())
    for p, entries in enumerate(by_class.entries_all()):
        assert T.same_entries(entries, ref.entries(p)) and by_class.summary(p) == T_summary(ref.entries(p))
    assert by_class.count() == ref.totals()
    b.close()
    solo_b.close()


def T_summary(entries):
    from cattleherd.train_log import summary_of
    return summary_of(entries)


# ---- 2. inside the collection -----------------------------------------------------------------------------------
# test_gpu_rollout_pop.py's setup: 2 drones x 8 cattle, compat=False, step counters 4800 - 2 - 4 * (e % T): truncations
# at every step, and (E = 24 > T = 19) two envs per member end at steps 1-5
E_C, P_C, T_C = 24, 3, 19


def RP():
    import test_gpu_rollout_pop as m
    return m


@functools.lru_cache(maxsize=None)
def solo_collection(p, W, collections):
    """The reference: member p alone on a batch of its own with a solo EpisodeRing: (entries, total)."""
    import torch
    from cattleherd.rollout import DeviceRolloutBuffer
    from cattleherd.train_log import EpisodeRing
    rp = RP()
    b = rp.batch(E_C, p * E_C, rp.step_counters(E_C, P_C, T_C)[p * E_C:(p + 1) * E_C])
    actor, critic, log_std = rp.nets("driver", p)
    rb = DeviceRolloutBuffer(b, T_C, act_dim=48, gamma=rp.GAMMAS[p], gae_lambda=rp.LAMBDAS[p])
    ring = EpisodeRing(b, W).begin()
    for c in range(collections):
        rb.collect(actor, critic, log_std, seed=100 + p + 10 * c, ring=ring)
    torch.cuda.synchronize()
    out = ring.entries(), ring.count()
    b.close()
    return out


@functools.lru_cache(maxsize=None)
def pop_collection(W, collections):
    """One population run (W = None: no ring): the members' entries and totals, buffers and env state."""
    import torch
    from cattleherd.rollout_pop import PopulationRollout
    from cattleherd.train_log import PopulationEpisodeRing
    rp = RP()
    b = rp.batch(P_C * E_C, 0, rp.step_counters(E_C, P_C, T_C))
    pop = PopulationRollout(b, P_C, T_C, act_dim=48, gammas=rp.GAMMAS[:P_C], gae_lambdas=rp.LAMBDAS[:P_C])
    ring = None if W is None else PopulationEpisodeRing(b, P_C, W).begin()
    ms = [rp.nets("driver", p) for p in range(P_C)]
    for c in range(collections):   # queued back to back: no synchronisation, no begin in between
        pop.collect([m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms], [100 + p + 10 * c for p in range(P_C)],
                    ring=ring)
    torch.cuda.synchronize()
    out = {"buffers": [{k: getattr(rb, k).cpu().numpy() for k in rp.ARRAYS} for rb in pop.members],
           "state": [rp.env_state(b, p * E_C, (p + 1) * E_C) for p in range(P_C)]}
    if ring is not None:
        out["entries"], out["totals"] = ring.entries_all(), ring.count()
        out["fitness"] = ring.fitness().cpu().numpy()
    pop.close()
    b.close()
    return out


@pytest.mark.parametrize("W", [100, 1])
def test_collection_fills_every_member_s_ring_like_its_solo_collection(W):
    got = pop_collection(W, 1)
    for p in range(P_C):
        entries, total = solo_collection(p, W, 1)
        assert got["totals"][p] == total and total > 0, (p, total)
        assert T.same_entries(got["entries"][p], entries), p
        assert len(entries) == min(W, total)
        assert all(0 <= e < E_C for _, _, e in entries)   # member-local env indices
    if W == 100:
        assert all(t >= 10 for t in got["totals"])   # two envs per member end at each of steps 1-5
    assert R.bits_equal64(got["fitness"], R.fitness_ref(got["entries"], got["totals"]))


def test_buffers_and_env_state_do_not_depend_on_the_ring():
    rp = RP()
    from rollout_ref import bits_equal
    with_ring, plain = pop_collection(100, 1), pop_collection(None, 1)
    for p in range(P_C):
        for k in rp.ARRAYS:
            assert bits_equal(with_ring["buffers"][p][k], plain["buffers"][p][k]), (p, k)
        assert with_ring["state"][p].keys() == plain["state"][p].keys() and plain["state"][p]
        for k, v in plain["state"][p].items():
            assert np.array_equal(with_ring["state"][p][k], v, equal_nan=np.issubdtype(v.dtype, np.floating)), (p, k)


def test_two_collections_queued_on_one_ring_equal_two_solo_collections():
    got = pop_collection(100, 2)
    for p in range(P_C):
        entries, total = solo_collection(p, 100, 2)
        assert got["totals"][p] == total > solo_collection(p, 100, 1)[1] > 0
        assert T.same_entries(got["entries"][p], entries), p


# ---- 3. the fitness table ---------------------------------------------------------------------------------------
def test_fitness_equals_the_numpy_restatement():
    """W = 100 with total 0 (empty: count 0, NaN means), below W, equal to W and above W (wrapped)."""
    import torch
    from cattleherd.env import HerdBatch
    from cattleherd.train_log import PopulationEpisodeRing
    P, W = 5, 100
    b = HerdBatch(2 * P, 2, 8, mode="ctde")
    ring = PopulationEpisodeRing(b, P, W).begin()
    rng = np.random.default_rng(5)
    totals = [0, 37, 100, 250, 101]
    ring.ep_return.copy_(torch.as_tensor(rng.normal(0.0, 100.0, (P, W))))
    ring.ep_length.copy_(torch.as_tensor(rng.integers(1, 1203, (P, W)).astype(np.int32)))
    ring.total.copy_(torch.as_tensor(np.array(totals, np.int64)))
    big, out = guarded((P, 4), torch.float64, ROW_F)
    got = ring.fitness(out=out).cpu().numpy()
    entries = ring.entries_all()
    assert [len(e) for e in entries] == [0, 37, 100, 100, 100] and ring.count() == totals
    want = R.fitness_ref(entries, totals)
    assert R.bits_equal64(got, want), (got, want)
    assert got[0, 0] == 0 and np.isnan(got[0, 1:3]).all() and got[0, 3] == 0
    assert got[:, 0].tolist() == [0, 37, 100, 100, 100] and got[:, 3].tolist() == [float(t) for t in totals]
    assert np.isfinite(got[1:]).all() and bands_intact(big)
    again = ring.fitness().cpu().numpy()
    assert R.bits_equal64(again, got)
    # the order matters at the last bit somewhere in these rows: the restatement is not np.mean in disguise
    assert any(want[p, 1] != np.mean([r for r, _, _ in entries[p]]) for p in range(1, P))
    b.close()


# ---- 4. explained variance --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [456, 8229])
def test_explained_variance_pop_equals_the_solo_calls(n):
    """n = 456 = T * E of the collection (one workgroup), n = 8229 (three workgroups of 2743 elements: no multiple of the 256 threads); member 1's
    returns are constant: NaN and var 0, as the solo call gives."""
    import torch
    from cattleherd import _lib
    from cattleherd.train_log import explained_variance, explained_variance_pop
    L = _lib.lib()
    P = 3
    G = L.ch_explained_variance_scratch(n) // 4
    assert G == (1 if n == 456 else 3)
    rng = np.random.default_rng(n)
    rets = [torch.as_tensor((rng.normal(0.0, 3.0, n) + 0.5).astype(np.float32)).cuda() for _ in range(P)]
    rets[1] = torch.full((n,), 2.5, device="cuda:0")
    vals = [torch.as_tensor((0.7 * r.cpu().numpy() + rng.normal(0.0, 1.0, n)).astype(np.float32)).cuda() for r in rets]
    want = np.stack([explained_variance(v, r).cpu().numpy() for v, r in zip(vals, rets)])
    got = explained_variance_pop(vals, rets).cpu().numpy()
    assert got.shape == (P, 2) and R.bits_equal64(got, want), (got, want)
    assert np.isnan(got[1, 0]) and got[1, 1] == 0.0 and np.isfinite(got[[0, 2]]).all()
    assert not same_bits(got[0], got[2])
    # the entry point itself, its scratch and its outputs inside guard bands
    size = L.ch_explained_variance_pop_scratch(n, P)
    assert size == 4 * G * P
    big_s, scratch = guarded((size,), torch.float64, ROW_F)
    big_o, out = guarded((P, 2), torch.float64, ROW_F)
    table = torch.tensor([t.data_ptr() for t in vals + rets], dtype=torch.int64).cuda()
    assert L.ch_explained_variance_pop(table[:P].data_ptr(), table[P:].data_ptr(), P, n, out.data_ptr(),
                                       scratch.data_ptr(), None) == 0, L.ch_last_error(None)
    torch.cuda.synchronize()
    assert R.bits_equal64(out.cpu().numpy(), want) and bands_intact(big_s) and bands_intact(big_o)
    assert bool((scratch != ROW_F).all())   # every partial of every member was written


# ---- 5. PPOPopulation.train with log_stats ----------------------------------------------------------------------
def _log_bits(log):
    return [(k, struct.pack("<d", v) if isinstance(v, float) else v) for k, v in log.items()]


@pytest.mark.parametrize("logging", [(True, True, True), (True, False, True)], ids=["all", "mixed"])
def test_population_train_logs_what_each_solo_train_logs(logging):
    """test_gpu_ppo_pop.py's odd-width net, 200 rows in minibatches of 64: every member's last_log is key for key and
    bit for bit the solo PPOUpdate.train's from cloned state; non-logging members stay without a record."""
    import torch
    import test_gpu_ppo_pop as PP
    from cattleherd.ppo import PPOUpdate
    from cattleherd.ppo_pop import PPOPopulation
    members = PP.make(PP.SMALL)
    rbs = [PP._buffer(m) for m in members]

    def updates():
        return [PP._updates(members[i:i + 1], None, log_stats=flag, seed=7 + i)[0] for i, flag in enumerate(logging)]
    solo, together = updates(), updates()
    for rounds in range(2):   # twice: n_updates carries over
        want = [u.train(rb, 0.5) for u, rb in zip(solo, rbs)]
        population = PPOPopulation(together)
        got = population.train(rbs, 0.5)
        torch.cuda.synchronize()
        assert got == want
        for a, c, flag in zip(together, solo, logging):
            assert bool(c.last_log) == flag
            assert list(a.last_log) == list(c.last_log) and _log_bits(a.last_log) == _log_bits(c.last_log)
            if flag:
                assert tuple(c.last_log) == PPOUpdate.LOG_KEYS and c.last_log["train/n_updates"] == 2 * (rounds + 1)
                assert a.last_stats.dtype == c.last_stats.dtype and same_bits(a.last_stats, c.last_stats)
            else:
                assert a.last_stats is None and c.last_stats is None
            assert a.n_updates == c.n_updates and a.sgd_steps == c.sgd_steps
            assert all(PP.same(x.detach(), y.detach()) for x, y in zip(a.model.parameters(), c.model.parameters()))
        population.close()
    logs = [u.last_log for u, flag in zip(solo, logging) if flag]
    assert logs[0]["train/explained_variance"] != logs[-1]["train/explained_variance"]   # the members differ


# ---- 6. error paths launch nothing ------------------------------------------------------------------------------
def test_error_paths_return_their_codes_and_write_nothing():
    import torch
    from cattleherd import _lib as L
    from cattleherd.env import HerdBatch
    from cattleherd.rollout import ChRolloutIO
    from cattleherd.rollout_pop import ChRolloutMember, PopulationRollout, _bind
    from cattleherd.train_log import PopulationEpisodeRing
    rp = RP()
    lib = _bind()
    INV, UNS = L.CH_ERR_INVALID, L.CH_ERR_UNSUPPORTED
    E, P, T_ = 24, 3, 4
    b = rp.batch(P * E, 0, rp.step_counters(E, P, T_))
    marl = HerdBatch(6, 2, 8, mode="marl")
    marl.reset()
    ring = PopulationEpisodeRing(b, P, 5)
    ring._buf.fill_(0x5a)
    untouched = ring._buf.clone()
    d_rh = torch.ones(P * E, dtype=torch.uint8, device="cuda:0")   # every env "ended": a launch would show
    d_st = torch.ones((P * E, 2), dtype=torch.float64, device="cuda:0")
    io = L.ChStepIO()
    io.reset_happened, io.episode_stats = d_rh.data_ptr(), d_st.data_ptr()

    def edited(**kw):
        r = L.ChEpRingPop()
        ctypes.memmove(ctypes.byref(r), ctypes.byref(ring._ring), ctypes.sizeof(r))
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def record(code, word, h=b, r="ok", sio="ok"):
        r = ring._ring if r == "ok" else r
        sio = io if sio == "ok" else sio
        for fn, args in ((lib.ch_ep_ring_pop_record, (None if sio is None else ctypes.byref(sio),)), (lib.ch_ep_ring_pop_begin, ())):
            if fn is lib.ch_ep_ring_pop_begin and (sio is not io):
                continue   # (begin takes no io)
            rc = fn(h.handle, None if r is None else ctypes.byref(r), *args, None)
            assert rc == code and word in lib.ch_last_error(h.handle).decode(), (rc, lib.ch_last_error(h.handle))
    record(INV, "NULL ring", r=None)
    record(INV, "NULL step io", sio=None)
    record(INV, "window", r=edited(window=0))
    record(INV, "n_members", r=edited(n_members=0))
    record(INV, "divide", r=edited(n_members=5))
    record(INV, "ring array", r=edited(ep_env=None))
    record(INV, "ring array", r=edited(total=None))
    record(UNS, "CTDE", h=marl)
    for field in ("reset_happened", "episode_stats"):
        sio = L.ChStepIO()
        ctypes.memmove(ctypes.byref(sio), ctypes.byref(io), ctypes.sizeof(sio))
        setattr(sio, field, None)
        record(INV, field, sio=sio)
    out = torch.full((P, 4), ROW_F, dtype=torch.float64, device="cuda:0")
    assert lib.ch_ep_ring_pop_summary(ctypes.byref(edited(window=0)), out.data_ptr(), None) == INV
    assert lib.ch_ep_ring_pop_summary(ctypes.byref(ring._ring), None, None) == INV
    # the collection: the ring's own rejections, with every other argument in order
    pop = PopulationRollout(b, P, T_, act_dim=48)
    ms = [rp.nets("driver", p) for p in range(P)]
    for m in ms:
        m[0]._ensure_packed()
        m[1]._ensure_packed()
    for rb in pop.members:
        for k in rp.ARRAYS:
            getattr(rb, k).fill_(rp.SENTINEL)
    tables = ctypes.c_void_p()
    assert lib.ch_rollout_pop_create(8, 0, ctypes.byref(tables)) == 0
    arr = (ChRolloutMember * P)()
    for mb, rb, m, p in zip(arr, pop.members, ms, range(P)):
        mb.rb = rb.struct()
        mb.actor, mb.critic = ctypes.pointer(m[0]._net), ctypes.pointer(m[1]._net)
        mb.log_std, mb.seed, mb.gamma, mb.gae_lambda = m[2].data_ptr(), p, 0.99, 0.95

    def collect(code, word, r, stats=True, h=b, n=P):
        sio = L.ChStepIO()
        ctypes.memmove(ctypes.byref(sio), ctypes.byref(h._io), ctypes.sizeof(sio))
        sio.terminal_obs, sio.reset_happened = h.terminal_obs.data_ptr(), h.reset_happened.data_ptr()
        sio.episode_stats = h.episode_stats.data_ptr() if stats else None
        rio = ChRolloutIO()
        rio.step = ctypes.pointer(sio)
        rio.mean, rio.value = pop.mean.data_ptr(), pop.value.data_ptr()
        rio.terminal_value, rio.env_actions = pop.terminal_value.data_ptr(), pop.env_actions.data_ptr()
        rc = lib.ch_rollout_collect_pop_log(h.handle, tables, arr, n, ctypes.byref(rio), 1, ctypes.byref(r), None)
        assert rc == code and word in lib.ch_last_error(h.handle).decode(), (rc, lib.ch_last_error(h.handle))
    collect(INV, "episode_stats", ring._ring, stats=False)
    collect(INV, "n_members", edited(n_members=1))          # a whole ring for another population size
    collect(INV, "n_members", edited(n_members=0))
    collect(INV, "window", edited(window=-2))
    collect(INV, "ring array", edited(ep_return=None))
    collect(INV, "divide", edited(n_members=5))              # (the ring's own division is checked before the match)
    collect(UNS, "CTDE", edited(n_members=2), h=marl, n=2)
    torch.cuda.synchronize()
    assert torch.equal(ring._buf, untouched) and bool((out == ROW_F).all())
    for rb in pop.members:
        for k in rp.ARRAYS:
            assert bool((getattr(rb, k) == rp.SENTINEL).all()), k
    assert lib.ch_rollout_pop_destroy(tables) == 0
    marl.close()
    b.close()
