"""GPU tests of the population update (ch_ppo_train_pop; cattleherd.ppo_pop.PPOPopulation): P learners in one set of
launches.  The yardstick is the solo entry, ch_ppo_train_opt / PPOUpdate.train -- itself held to float64 references by
test_gpu_ppo_native.py and test_gpu_ppo_opts.py -- run on a clone of each member's state.  The claim is bit identity,
so every comparison is exact (bit patterns, which also compares NaNs by position); there is no tolerance.

Shapes: 200 rows in minibatches of 64 (4 steps an epoch, the last of 8 rows: a partial minibatch and a partial tile),
P = 3 members that differ in weights, data, permutation and hyper-parameters.  SMALL (37-[32]-5 / 37-[48, 16]-1) has
odd widths, so none of its rows take float4 loads, and a different layer count per net; DRIVER is the CTDE driver's
1032-128-128-48, whose rows do."""
import ctypes
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = dict(obs_dim=37, act_dim=5, pi=(32,), vf=(48, 16))
DRIVER = dict(obs_dim=1032, act_dim=48, pi=(128, 128), vf=(128, 128))
ROWS, BATCH, P, NB = 200, 64, 3, 4
# per member: learning_rate, clip_range, ent_coef, max_grad_norm
HPS = ((3e-4, 0.1, 0.1, 0.5), (1e-3, 0.2, 0.0, 0.3), (5e-4, 0.15, 0.05, 10.0))
POISON = 12345.0


def _lib():
    from cattleherd import _lib
    return _lib


class Member:
    """One learner as ch_ppo_train_opt takes it: a model, its rollout data, Adam state, options, statistics, scratch."""

    def __init__(self, shape, i, epochs=2, target_kl=0.0, clip_vf=0.0):
        import torch
        import ppo_native_ref as R
        from cattleherd.ppo import SB3ActorCritic
        dev = torch.device("cuda", 0)
        self.shape, self.i, self.epochs = shape, i, epochs
        src = SB3ActorCritic(obs_dim=shape["obs_dim"], act_dim=shape["act_dim"], pi=shape["pi"], vf=shape["vf"],
                             device=dev, seed=100 + i)
        self.model = R.make_model(shape, dev, like=src)
        g = torch.Generator().manual_seed(1000 + i)
        rn = lambda *s: torch.randn(*s, generator=g).to(dev)   # noqa: E731
        obs = 0.5 * rn(ROWS, shape["obs_dim"])
        with torch.no_grad():
            mean = self.model.action_net(self.model.policy_net(obs))
            act = (mean + torch.exp(self.model.log_std) * rn(ROWS, shape["act_dim"])).contiguous()
            val, lp, _ = self.model.evaluate_actions(obs, act)
        self.obs, self.act = obs.contiguous(), act
        self.old_lp = (lp + 0.15 * rn(ROWS)).contiguous()
        self.adv, self.ret = rn(ROWS), rn(ROWS)
        self.old_values = (val + 0.25 * rn(ROWS)).contiguous()
        self.perms = [torch.randperm(ROWS, generator=g).to(dev) for _ in range(epochs)]
        self.hp = HPS[i % len(HPS)]
        self.target_kl, self.clip_vf = target_kl, clip_vf
        self.n = sum(p.numel() for p in self.model.parameters())
        self.m, self.v = torch.zeros(self.n, device=dev), torch.zeros(self.n, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stop = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stats = torch.full((epochs * NB, 7), POISON, device=dev)
        from cattleherd import ppo
        size = ppo._bind().ch_ppo_scratch_size(ctypes.byref(ppo.ppo_net(self.model)), BATCH)
        self.scratch = torch.zeros(size, device=dev)

    def clone(self):
        import torch
        import ppo_native_ref as R
        c = Member.__new__(Member)
        c.__dict__.update(self.__dict__)
        c.model = R.make_model(self.shape, self.model.device, like=self.model)
        for k in ("m", "v", "step", "stop", "stats", "scratch"):
            setattr(c, k, getattr(self, k).clone())
        assert isinstance(c.m, torch.Tensor)
        return c

    # the ABI structs over the member's storage as it is now
    def structs(self):
        from cattleherd import ppo
        L = _lib()
        lr, clip, ent, gn = self.hp
        net = ppo.ppo_net(self.model)
        hp = L.ChPpoHparams(lr, 0.9, 0.999, 1e-5, clip, ent, 0.7, gn, 1, 0)
        data = L.ChPpoData(self.obs.data_ptr(), self.act.data_ptr(), self.old_lp.data_ptr(), self.adv.data_ptr(),
                           self.ret.data_ptr(), ROWS)
        opts = L.ChPpoOpts(self.target_kl, self.clip_vf, self.old_values.data_ptr() if self.clip_vf > 0 else None,
                           self.stop.data_ptr() if self.target_kl > 0 else None)
        return net, hp, data, opts

    def solo(self, epochs=None):
        """ch_ppo_train_opt, one call per epoch."""
        import torch
        from cattleherd import ppo
        net, hp, data, opts = self.structs()
        for e in epochs if epochs is not None else range(self.epochs):
            rc = ppo._bind().ch_ppo_train_opt(
                ctypes.byref(net), ctypes.byref(hp), ctypes.byref(data), ctypes.byref(opts), self.perms[e].data_ptr(), ROWS,
                BATCH, self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), self.stats[e * NB].data_ptr(),
                self.scratch.data_ptr(), None)
            assert rc == 0, _lib().lib().ch_last_error(None)
        torch.cuda.synchronize()
        return self

    def entry(self, e):
        L = _lib()
        mb = L.ChPpoMember()
        mb.net, mb.hp, mb.data, mb.opts = self.structs()
        mb.idx, mb.m, mb.v, mb.step_dev = self.perms[e].data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr()
        mb.stats, mb.scratch = self.stats[e * NB].data_ptr(), self.scratch.data_ptr()
        return mb

    def grad(self):
        """The flat gradient the last minibatch that ran left at the end of the scratch."""
        return self.scratch[self.scratch.numel() - (self.n + 3) // 4 * 4:][:self.n]

    def state(self):
        return [p.detach() for p in self.model.parameters()] + [self.m, self.v, self.step, self.stop, self.stats, self.grad()]


def bits(t):
    return t.contiguous().view(-1).view({4: __import__("torch").int32, 8: __import__("torch").int64}[t.element_size()])


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_equal_members(got, want):
    names = None
    for g, w in zip(got, want):
        names = [f"param{k}" for k in range(len(g.state()) - 6)] + ["m", "v", "step", "stop", "stats", "grad"]
        for name, x, y in zip(names, g.state(), w.state()):
            assert same(x, y), f"member {g.i}: {name} differs from the solo run's"


@pytest.fixture(scope="module")
def pop():
    import torch
    L = _lib()
    torch.zeros(1, device="cuda:0")   # torch brings the device up first, as in every use of the package
    h = ctypes.c_void_p()
    assert L.lib().ch_ppo_pop_create(4, 0, ctypes.byref(h)) == 0, L.lib().ch_last_error(None)
    yield h
    torch.cuda.synchronize()
    assert L.lib().ch_ppo_pop_destroy(h) == 0


def run_pop(pop, members, epochs=None, n=None, expect=0):
    """ch_ppo_train_pop, one call per epoch, no synchronisation between the calls."""
    import torch
    L = _lib()
    rcs = []
    for e in epochs if epochs is not None else range(members[0].epochs):
        arr = (L.ChPpoMember * len(members))(*[m.entry(e) for m in members])
        rcs.append(L.lib().ch_ppo_train_pop(pop, arr, len(members) if n is None else n, ROWS, BATCH, None))
    torch.cuda.synchronize()
    assert all(rc == expect for rc in rcs), (rcs, L.lib().ch_last_error(None))
    return members


def make(shape, count=P, **kw):
    return [Member(shape, i, **{k: (v[i] if isinstance(v, (tuple, list)) else v) for k, v in kw.items()}) for i in range(count)]


# ---- 1. / 2. equals solo --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, DRIVER], ids=["small", "driver"])
def test_population_equals_solo_options_off(pop, shape):
    import torch
    members = make(shape)
    want = [m.clone().solo() for m in members]
    run_pop(pop, members)
    assert_equal_members(members, want)
    for m, m0 in zip(want, make(shape)):   # the reference did something: 8 applied steps, every row written
        assert int(m.step) == 2 * NB and torch.equal(m.stats[:, 6], torch.ones(2 * NB, device=m.stats.device))
        assert torch.isfinite(m.stats).all() and not same(m.model.action_net.weight, m0.model.action_net.weight)
    assert not same(want[0].m, want[1].m)   # and the members are different learners


def test_population_of_one_equals_solo(pop):
    members = make(SMALL, 1)
    want = [m.clone().solo() for m in members]
    run_pop(pop, members)
    assert_equal_members(members, want)


# ---- 3. / 4. one member trips, the others carry on; the word is sticky ------------------------------------------------------
def _spiked(shape=SMALL):
    """Members armed with target_kl, member 1's second minibatch spiked by +-0.6 in old_log_prob (the construction of
    test_gpu_ppo_opts.py) and its threshold set between that minibatch's approx_kl and the others'."""
    import torch
    members = make(shape, target_kl=1e6)
    rows = members[1].perms[0][BATCH:2 * BATCH]
    sign = torch.ones(BATCH, device=rows.device)
    sign[1::2] = -1.0
    members[1].old_lp[rows] += 0.6 * sign
    free = [m.clone().solo() for m in members]                    # armed, never trips
    kls = free[1].stats[:, 4].cpu().numpy()
    T = float(kls[1]) / 1.2
    assert kls[:1].max() < 0.9 * T and kls[1] > 1.1 * T and all(int(f.stop) == 0 for f in free)
    members[1].target_kl = T / 1.5
    for i in (0, 2):   # armed with a threshold their own minibatches stay well below
        members[i].target_kl = 10.0 * float(free[i].stats[:, 4].max()) / 1.5
    return members


def test_one_member_trips_the_others_do_not(pop):
    import torch
    members = _spiked()
    want = [m.clone().solo() for m in members]
    # the solo reference itself shows the pattern
    st = want[1].stats.cpu()
    assert list(st[:, 6]) == [1, 0] + [-1] * 6 and int(want[1].step) == 1 and int(want[1].stop) != 0
    assert torch.isnan(st[2:, :6]).all() and torch.isfinite(st[:2, :6]).all()
    for i in (0, 2):
        assert list(want[i].stats[:, 6].cpu()) == [1] * 8 and int(want[i].stop) == 0 and int(want[i].step) == 8
    run_pop(pop, members)
    assert_equal_members(members, want)
    assert list(members[1].stats[:, 6].cpu()) == [1, 0] + [-1] * 6 and int(members[1].step) == 1 and int(members[1].stop) != 0
    for i in (0, 2):
        assert list(members[i].stats[:, 6].cpu()) == [1] * 8 and int(members[i].stop) == 0


def test_stop_word_is_sticky_across_population_calls(pop):
    members = _spiked()
    run_pop(pop, members, epochs=[0])
    assert int(members[1].stop) != 0 and int(members[1].step) == 1
    before = members[1].clone()
    others = [members[i].clone().solo(epochs=[1]) for i in (0, 2)]
    run_pop(pop, members, epochs=[1])
    for x, y in zip(members[1].state()[:-2], before.state()[:-2]):     # weights, m, v, step, stop
        assert same(x, y)
    assert same(members[1].grad(), before.grad())
    st = members[1].stats[NB:].cpu()
    assert list(st[:, 6]) == [-1] * NB and np.isnan(st[:, :6].numpy()).all()
    assert_equal_members([members[0], members[2]], others)
    assert int(members[0].step) == int(members[2].step) == 2 * NB


# ---- 5. value clip with different ranges ------------------------------------------------------------------------------------
def test_value_clip_with_different_ranges(pop):
    import torch
    ranges = (0.1, 0.25, 0.4)
    members = make(SMALL, clip_vf=ranges)
    for m, c in zip(members, ranges):   # the first minibatch at the initial weights: rows on both sides of the bound
        with torch.no_grad():
            v, _, _ = m.model.evaluate_actions(m.obs, m.act)
        dv = (v - m.old_values)[m.perms[0][:BATCH]].abs()
        assert (dv > c).any() and (dv < c).any()
    want = [m.clone().solo() for m in members]
    plain = make(SMALL)[0].solo()
    assert not same(want[0].stats, plain.stats)     # (the clip is live: the value loss differs from the unclipped one)
    run_pop(pop, members)
    assert_equal_members(members, want)


# ---- 6. per-member alignment flags ------------------------------------------------------------------------------------------
def test_misaligned_member(pop):
    import torch
    members = make(DRIVER)
    m = members[1]
    obs = torch.zeros(m.obs.numel() + 4, device=m.obs.device)
    obs[1:1 + m.obs.numel()] = m.obs.view(-1)
    m.obs = obs[1:1 + m.obs.numel()].view(ROWS, -1)
    w = m.model.policy_net[0].weight
    buf = torch.zeros(w.numel() + 4, device=w.device)
    buf[1:1 + w.numel()] = w.data.view(-1)
    w.data = buf[1:1 + w.numel()].view_as(w)
    assert m.obs.data_ptr() % 16 == 4 and w.data_ptr() % 16 == 4 and m.obs.is_contiguous() and w.is_contiguous()
    assert members[0].obs.data_ptr() % 16 == 0 and members[0].model.policy_net[0].weight.data_ptr() % 16 == 0

    def clone(x):   # a clone that keeps the misalignment
        c = x.clone()
        if x is m:
            c.obs = m.obs
            w2 = c.model.policy_net[0].weight
            b2 = torch.zeros(w2.numel() + 4, device=w2.device)
            b2[1:1 + w2.numel()] = w.data.view(-1)
            w2.data = b2[1:1 + w2.numel()].view_as(w2)
            assert w2.data_ptr() % 16 == 4
        return c
    want = [clone(x).solo() for x in members]
    run_pop(pop, members)
    assert_equal_members(members, want)


# ---- 7. isolation -----------------------------------------------------------------------------------------------------------
def test_members_write_nothing_outside_their_own_memory(pop):
    import torch
    members = make(SMALL)
    want = [m.clone().solo() for m in members]
    G = 64
    r4 = lambda k: (k + 3) // 4 * 4   # noqa: E731
    sizes = [r4(members[0].n), r4(members[0].n), r4(members[0].scratch.numel()), r4(members[0].stats.numel())]
    total = G + P * sum(s + G for s in sizes)
    arena = torch.zeros(total, device=members[0].m.device)
    guard = torch.zeros(total, dtype=torch.bool)
    pattern = torch.tensor([0x7fc0dead], dtype=torch.int32).view(torch.float32).item()
    o = 0
    for m in members:
        for k, size in zip(("m", "v", "scratch", "stats"), sizes):
            guard[o:o + G] = True
            o += G
            old = getattr(m, k)
            view = arena[o:o + old.numel()].view(old.shape)
            view.copy_(old)
            setattr(m, k, view)
            guard[o + old.numel():o + size] = True   # (the rounding, guarded too)
            o += size
    guard[o:o + G] = True
    guard = guard.to(arena.device)
    bits(arena)[guard] = 0x7fc0dead
    assert np.isnan(pattern) and members[0].scratch.data_ptr() % 16 == 0 and arena.data_ptr() % 16 == 0
    run_pop(pop, members)
    assert bool((bits(arena)[guard] == 0x7fc0dead).all())
    assert_equal_members(members, want)


# ---- 8. reproducible --------------------------------------------------------------------------------------------------------
def test_two_population_runs_are_bit_identical(pop):
    a, b = run_pop(pop, make(DRIVER)), run_pop(pop, make(DRIVER))
    assert_equal_members(a, b)


# ---- 9. error paths launch nothing ------------------------------------------------------------------------------------------
def _untouched(members, before):
    for m, b in zip(members, before):
        for x, y in zip(m.state()[:-3], b.state()[:-3]):   # weights, m, v, step
            assert same(x, y)
        assert same(m.stats, b.stats)


def test_error_paths_launch_nothing(pop):
    import torch
    L = _lib()
    err = lambda: L.lib().ch_last_error(None).decode()   # noqa: E731

    def rejected(members, code, word, **kw):
        before = [m.clone() for m in members]
        run_pop(pop, members, epochs=[0], expect=code, **kw)
        assert err().startswith("ch_ppo_train_pop: ") and word in err(), err()
        _untouched(members, before)

    other = dict(SMALL, vf=(48, 32))
    rejected(make(SMALL, 2) + [Member(other, 2)], L.CH_ERR_UNSUPPORTED, "architecture")
    rejected(make(SMALL, clip_vf=(0.2, 0.0, 0.2)), L.CH_ERR_UNSUPPORTED, "clip_range_vf")
    rejected(make(SMALL), L.CH_ERR_INVALID, "n_members", n=0)
    rejected(make(SMALL) + make(SMALL, 2), L.CH_ERR_INVALID, "n_members")      # 5 > max_members = 4
    ms = make(SMALL)
    keep = ms[2].stats
    ms[2].entry = lambda e, f=ms[2].entry: _with(f(e), stats=None)
    rejected(ms, L.CH_ERR_INVALID, "stats")
    assert same(keep, ms[2].stats)
    ms = make(SMALL)
    ms[1].entry = lambda e, f=ms[1].entry, p=ms[1].scratch.data_ptr() + 4: _with(f(e), scratch=p)
    rejected(ms, L.CH_ERR_INVALID, "16-byte aligned")
    ms = make(SMALL)

    def no_stop(e, f=ms[0].entry):
        mb = f(e)
        mb.opts.target_kl, mb.opts.stop_dev = 0.01, None
        return mb
    ms[0].entry = no_stop
    rejected(ms, L.CH_ERR_INVALID, "stop_dev")
    torch.cuda.synchronize()


def _with(mb, **kw):
    for k, v in kw.items():
        setattr(mb, k, v)
    return mb


# ---- 10. calls queued back to back: the staging slots -----------------------------------------------------------------------
def test_calls_queued_back_to_back_on_one_stream(pop):
    """Five epochs with a permutation each and no synchronisation between the calls: every staging slot is reused
    while earlier calls' copies and launches may still be queued."""
    members = make(SMALL, epochs=5)
    assert not same(members[0].perms[0], members[0].perms[1])
    want = [m.clone().solo() for m in members]
    run_pop(pop, members)
    assert_equal_members(members, want)
    assert all(int(m.step) == 5 * NB for m in members)


# ---- 11. / 12. the Python class ---------------------------------------------------------------------------------------------
def _buffer(m):
    return types.SimpleNamespace(T=ROWS, batch=types.SimpleNamespace(n_envs=1), obs=m.obs.view(ROWS, 1, -1),
                                 actions=m.act.view(ROWS, 1, -1), log_probs=m.old_lp.view(ROWS, 1),
                                 advantages=m.adv.view(ROWS, 1), returns=m.ret.view(ROWS, 1), values=m.old_values.view(ROWS, 1))


def _updates(members, variant, **kw):
    import ppo_native_ref as R
    from cattleherd.ppo import PPOUpdate
    ups = []
    for i, m in enumerate(members):
        lr, clip, ent, gn = m.hp
        k = dict(learning_rate=lr, clip_range=clip, ent_coef=ent, max_grad_norm=gn, n_epochs=2, batch_size=BATCH,
                 seed=7 + i, backend="native")
        if variant == "log_stats":
            k["log_stats"] = True
        elif variant == "target_kl":   # member 0 trips at once (its approx_kl is ~0.15^2 / 2), 1 never, 2 has no gate
            k["target_kl"] = (0.004, 1.0, None)[i]
            k["log_stats"] = i == 1
        elif variant == "schedule":
            k["learning_rate"] = lambda p, lr=lr: lr * p
        k.update(kw)
        ups.append(PPOUpdate(R.make_model(m.shape, m.model.device, like=m.model), **k))
    return ups


@pytest.mark.parametrize("variant", ["log_stats", "target_kl", "schedule"])
def test_population_train_equals_the_list_of_trains(variant):
    import torch
    from cattleherd.ppo_pop import PPOPopulation
    members = make(SMALL)
    rbs = [_buffer(m) for m in members]
    solo, together = _updates(members, variant), _updates(members, variant)
    want = [u.train(rb, 0.5) for u, rb in zip(solo, rbs)]
    population = PPOPopulation(together)
    got = population.train(rbs, 0.5)
    torch.cuda.synchronize()
    assert got == want == [2 * NB] * P
    for a, b in zip(together, solo):
        assert all(same(p.detach(), q.detach()) for p, q in zip(a.model.parameters(), b.model.parameters()))
        assert same(a.exp_avg, b.exp_avg) and same(a.exp_avg_sq, b.exp_avg_sq)
        assert (a.last_stats is None) == (b.last_stats is None)
        if b.last_stats is not None:
            assert a.last_stats.shape == b.last_stats.shape and a.last_stats.dtype == b.last_stats.dtype
            assert np.array_equal(a.last_stats, b.last_stats, equal_nan=True)
        assert a.last_log == b.last_log and a.n_updates == b.n_updates and a.sgd_steps == b.sgd_steps
        assert a.stopped_early == b.stopped_early and a.steps_applied == b.steps_applied
        assert a.learning_rate == b.learning_rate and a.clip_range == b.clip_range
        assert torch.equal(torch.randperm(ROWS, device=a.model.device, generator=a.gen),
                           torch.randperm(ROWS, device=b.model.device, generator=b.gen))
    if variant == "target_kl":    # the variant is live
        assert solo[0].stopped_early and solo[0].steps_applied == 0 and not solo[1].stopped_early
        assert solo[1].steps_applied == solo[2].steps_applied == 2 * NB and solo[1].last_log
    if variant == "log_stats":
        assert all(u.last_log and u.last_stats.shape == (2 * NB, 6) for u in solo)
    if variant == "schedule":
        assert [u.learning_rate for u in solo] == [0.5 * m.hp[0] for m in members]
    population.close()


def test_population_rejections():
    import ppo_native_ref as R
    from cattleherd.ppo import PPOUpdate
    from cattleherd.ppo_pop import PPOPopulation
    members = make(SMALL)
    ups = _updates(members, None)
    torch_member = PPOUpdate(R.make_model(SMALL, members[0].model.device), backend="torch", graph=False)
    with pytest.raises(ValueError):
        PPOPopulation(ups[:2] + [torch_member])
    with pytest.raises(ValueError):
        PPOPopulation(ups[:2] + _updates(members[2:], None, batch_size=32))
    with pytest.raises(ValueError):
        PPOPopulation(ups[:2] + _updates(members[2:], None, clip_range_vf=0.2))
    PPOPopulation(ups).close()
