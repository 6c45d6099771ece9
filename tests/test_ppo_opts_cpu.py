"""PPOUpdate's target_kl / clip_range_vf / schedules without a GPU: train_log.sb3_train_record on hand-made statistics
tables, schedule evaluation, and the torch backend on CPU tensors in float64 against ppo_opts_ref.sb3_train (SB3's loop
restated line by line) on a 12-16-16-4 net, 32 rows, minibatches of 8."""
import types

import numpy as np
import pytest
import torch

import ppo_opts_ref as P
from cattleherd.ppo import PPOUpdate, SB3ActorCritic
from cattleherd.train_log import sb3_train_record

KEYS10 = PPOUpdate.LOG_KEYS


def _table(states, seed=0):
    rng = np.random.default_rng(seed)
    t = rng.normal(size=(len(states), 7)).astype(np.float32)
    t[:, 6] = states
    t[np.asarray(states) < 0, :6] = np.nan
    return t


def _expect(t, rows, n_updates, **kw):
    s = t.astype(np.float64)[rows]
    rec = {"train/entropy_loss": float(np.mean(-s[:, 2])), "train/policy_gradient_loss": float(np.mean(s[:, 0])),
           "train/value_loss": float(np.mean(s[:, 1])), "train/approx_kl": float(np.mean(s[:, 4])),
           "train/clip_fraction": float(np.mean(s[:, 5])),
           "train/loss": float(s[-1, 0] + 0.1 * -s[-1, 2] + 0.7 * s[-1, 1]), "train/explained_variance": 0.25,
           "train/std": 0.5, "train/n_updates": n_updates, "train/clip_range": 0.2}
    rec.update(kw)
    return rec


@pytest.mark.parametrize("name,states,rows,epochs", [
    ("no trip", [1] * 12, list(range(12)), 3),
    ("middle of epoch 2 of 3", [1] * 5 + [0] + [-1] * 6, list(range(6)), 2),
    ("first minibatch", [0] + [-1] * 11, [0], 1),
    ("last minibatch of the last epoch", [1] * 11 + [0], list(range(12)), 3)])
def test_sb3_train_record(name, states, rows, epochs):
    t = _table(states)
    rec, ran = sb3_train_record(t, 4, 0.1, 0.7, 0.2, 0.25, 0.5, n_updates=7, learning_rate=3e-4, clip_range_vf=0.3)
    assert ran == epochs
    want = _expect(t, rows, 7 + epochs, **{"train/learning_rate": 3e-4, "train/clip_range_vf": 0.3})
    assert rec == want and tuple(rec) == KEYS10 + ("train/learning_rate", "train/clip_range_vf")
    assert all(np.isfinite(v) for v in rec.values())
    # neither option given: exactly the ten keys; a six-column table (ch_ppo_train_log's) is all state 1
    rec, ran = sb3_train_record(t, 4, 0.1, 0.7, 0.2, 0.25, 0.5)
    assert tuple(rec) == KEYS10 and rec["train/n_updates"] == epochs
    if min(states) == 1:
        rec6, ran6 = sb3_train_record(t[:, :6], 4, 0.1, 0.7, 0.2, 0.25, 0.5)
        assert rec6 == rec and ran6 == 3


def test_sb3_train_record_needs_a_row_that_ran():
    with pytest.raises(ValueError):
        sb3_train_record(_table([-1] * 4), 4, 0.1, 0.7, 0.2, 0.0, 1.0)


# ---- the torch backend on the CPU ---------------------------------------------------------------------------------
SHAPE = dict(obs_dim=12, act_dim=4, pi=(16, 16), vf=(16, 16))
ROWS, BATCH, EPOCHS, SEED = 32, 8, 3, 5


def _model():
    m = SB3ActorCritic(device="cpu", seed=0, **SHAPE)
    m.modules.double()
    m.log_std.data = m.log_std.data.double()
    return m


def _buffer(sigma=0.3):
    g = torch.Generator().manual_seed(2)
    m = _model()
    obs = torch.randn(ROWS, 12, generator=g, dtype=torch.float64)
    with torch.no_grad():
        mean = m.action_net(m.policy_net(obs))
        act = mean + torch.exp(m.log_std) * torch.randn(ROWS, 4, generator=g, dtype=torch.float64)
        values, lp, _ = m.evaluate_actions(obs, act)
    rb = types.SimpleNamespace(T=4, batch=types.SimpleNamespace(n_envs=8), obs=obs.view(4, 8, 12),
                               actions=act.view(4, 8, 4),
                               log_probs=(lp + 0.15 * torch.randn(ROWS, generator=g, dtype=torch.float64)).view(4, 8),
                               advantages=torch.randn(ROWS, generator=g, dtype=torch.float64).view(4, 8),
                               returns=torch.randn(ROWS, generator=g, dtype=torch.float64).view(4, 8),
                               values=(values + sigma * torch.randn(ROWS, generator=g, dtype=torch.float64)).view(4, 8))
    return rb


def _data(rb):
    return (rb.obs.view(ROWS, -1), rb.actions.view(ROWS, -1), rb.log_probs.view(-1), rb.advantages.view(-1),
            rb.returns.view(-1), rb.values.view(-1))


def _upd(model, **kw):
    return PPOUpdate(model, batch_size=BATCH, n_epochs=EPOCHS, seed=SEED, graph=False, backend="torch", **kw)


def test_gate_stops_where_the_restatement_does_and_leaves_a_truncated_run():
    rb = _buffer()
    perms = P.perms_of(SEED, ROWS, EPOCHS, "cpu")
    s = 5                                             # epoch 2, neither its first nor its last minibatch
    P.spike_log_probs(rb.log_probs, perms[1][BATCH:2 * BATCH])     # that minibatch's rows: a large log-ratio
    free = P.sb3_train(_model(), _data(rb), perms, BATCH)
    kls = free["approx_kl_divs"]
    assert len(kls) == 12
    T = kls[s] / 1.2
    assert max(kls[:s]) < 0.9 * T and kls[s] > 1.1 * T, kls       # on the ungated reference alone
    ref_m, got_m, cut_m = _model(), _model(), _model()
    ref = P.sb3_train(ref_m, _data(rb), perms, BATCH, target_kl=T / 1.5)
    cut = P.sb3_train(cut_m, _data(rb), perms, BATCH, max_steps=s)
    upd = _upd(got_m, target_kl=T / 1.5)
    assert upd.train(rb) == s and upd.stopped_early and upd.steps_applied == s and upd.n_updates == 2
    assert not ref["continue_training"] and ref["steps_applied"] == s and ref["n_updates"] == 2
    st = upd.last_stats
    assert st.shape == (12, 7) and list(st[:, 6]) == [1] * s + [0] + [-1] * (11 - s)
    assert np.isnan(st[s + 1:, :6]).all() and np.isnan(st[s, 3]) and np.isfinite(st[:s, :6]).all()
    want = P.table_of(ref, 12)
    assert np.array_equal(st[:, [0, 1, 2, 4, 5, 6]], want[:, [0, 1, 2, 4, 5, 6]], equal_nan=True)
    for p, q, r in zip(got_m.parameters(), ref_m.parameters(), cut_m.parameters()):
        assert torch.equal(p, q) and torch.equal(p, r)          # the tripping minibatch applied nothing
    for p in got_m.parameters():
        assert int(upd.opt.state[p]["step"]) == s
    rec, _ = sb3_train_record(st, 4, 0.1, 0.7, 0.1, 0.0, 1.0, learning_rate=3e-4)
    assert rec == P.sb3_logger_record(ref, 0.0, 1.0, 0.1, learning_rate=3e-4)
    # a gate that never trips changes nothing
    a, b = _model(), _model()
    _upd(a).train(rb)
    never = _upd(b, target_kl=1e9)
    assert never.train(rb) == 12 and not never.stopped_early and never.n_updates == 3
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))


def test_value_clip_gradient_vanishes_on_exactly_the_clipped_rows():
    c = 0.3
    rb = _buffer(sigma=c)
    data = _data(rb)
    m = _model()
    upd = _upd(m, clip_range_vf=c)
    with torch.no_grad():
        values, _, _ = m.evaluate_actions(data[0], data[1])
    dv = values - data[5]
    clipped = dv.abs() > c
    assert 0.1 <= float(clipped.double().mean()) <= 0.6 and (dv > c).any() and (dv < -c).any()
    # per-row gradient of the loss with respect to the value head's bias: 2 vf_coef (pred - ret) / B, or 0
    for i in range(ROWS):
        for p in m.parameters():
            p.grad = None
        upd._loss(*(t[i:i + 1] for t in data)).backward()
        g = float(m.value_net.bias.grad)
        if clipped[i]:
            assert g == 0.0
        else:
            assert g == pytest.approx(float(2 * 0.7 * (values[i] - data[4][i])), rel=1e-12) and g != 0.0
    # the loop: the update against the restatement, bit for bit, and different from the unclipped one
    perms = P.perms_of(SEED, ROWS, EPOCHS, "cpu")
    ref_m, got_m, plain_m = _model(), _model(), _model()
    ref = P.sb3_train(ref_m, data, perms, BATCH, clip_range_vf=c)
    assert _upd(got_m, clip_range_vf=c).train(rb) == 12 == ref["steps_applied"]
    _upd(plain_m).train(rb)
    assert all(torch.equal(p, q) for p, q in zip(got_m.parameters(), ref_m.parameters()))
    assert not torch.equal(got_m.value_net.weight, plain_m.value_net.weight)


def test_schedules_are_evaluated_once_per_train():
    rb = _buffer()
    calls = {"lr": [], "clip": []}

    def lr(p):
        calls["lr"].append(p)
        return 3e-4 * p

    def clip(p):
        calls["clip"].append(p)
        return 0.2 * p

    a, b = _model(), _model()
    upd = _upd(a, learning_rate=lr, clip_range=clip)
    assert calls == {"lr": [1.0], "clip": [1.0]} and upd.learning_rate == 3e-4 and upd.clip_range == 0.2
    upd.train(rb, progress_remaining=0.5)
    assert calls == {"lr": [1.0, 0.5], "clip": [1.0, 0.5]}
    assert upd.learning_rate == 1.5e-4 and upd.clip_range == 0.1
    assert all(g["lr"] == 1.5e-4 for g in upd.opt.param_groups)
    _upd(b, learning_rate=1.5e-4, clip_range=0.1).train(rb)                    # floats pass through
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    upd.train(rb)                                                              # the default: progress_remaining = 1
    assert calls["lr"][-1] == 1.0 and upd.learning_rate == 3e-4 and len(calls["lr"]) == 3


def test_rejections():
    m = _model()
    for kw in (dict(target_kl=0.01), dict(learning_rate=lambda p: 1e-3), dict(clip_range=lambda p: 0.1)):
        with pytest.raises(ValueError, match="graph=False"):
            PPOUpdate(m, backend="torch", graph=True, **kw)
    for kw in (dict(target_kl=0.0), dict(clip_range_vf=-1.0)):
        with pytest.raises(ValueError, match="> 0"):
            PPOUpdate(m, backend="torch", graph=False, **kw)
    assert len(PPOUpdate.LOG_KEYS) == 10
