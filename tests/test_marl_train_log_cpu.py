"""The device-side RLlib training log without a GPU: the ring's reference against hand-written cases, the torch backend
of MarlPPOUpdate(log_stats=True) on the host in float64 against an independent evaluation of the loss's terms, and
MarlEpisodeRing.summary()'s keys over a ring filled from the host (the class allocates on the batch's device: a stand-in
batch on "cpu" never touches the library)."""
import math
import types

import numpy as np
import pytest

import marl_train_log_ref as T


# ---- MarlRingRef against hand-written cases ---------------------------------------------------------------------------
def test_an_agent_that_drops_out_early_has_a_shorter_length():
    ref = T.MarlRingRef(E=2, N=2, W=4)
    f = np.float32
    ref.step([[1, 1], [1, 1]], f([[1.0, 2.0], [0.5, 0.25]]), [0, 0])
    ref.step([[1, 0], [1, 1]], f([[4.0, np.nan], [0.5, 0.25]]), [0, 0])     # agent 1 of env 0 dropped out
    ref.step([[1, 0], [1, 1]], f([[8.0, 1e30], [0.5, 0.25]]), [1, 0])       # env 0 ends
    (ret, length, a_ret, a_len, env), = ref.entries()
    assert (ret, length, env) == (15.0, 3, 0)
    assert a_ret.tolist() == [13.0, 2.0] and a_len.tolist() == [3, 1]
    assert ref.total == 1 and ref.env_steps == 6 and ref.agent_steps.tolist() == [6, 4]
    assert ref.acc_return.tolist() == [[0.0, 0.0], [1.5, 0.75]] and ref.acc_steps.tolist() == [0, 3]
    a = ref.arrays()
    assert a["ep_return"][0] == 15.0 and a["agent_length"][0].tolist() == [3, 1] and a["total"][0] == 1


def test_more_endings_than_slots_keep_the_last_in_env_order():
    E, W = 7, 3
    ref = T.MarlRingRef(E, 1, W)
    rew = np.arange(1, E + 1, dtype=np.float32).reshape(E, 1)
    ref.step(np.ones((E, 1), np.uint8), rew, [1, 1, 0, 1, 1, 1, 1])      # C = 6 > W: envs 0 1 3 4 5 6
    assert ref.total == 6 and ref.max_ended == 6
    assert [e[4] for e in ref.entries()] == [4, 5, 6] and [e[0] for e in ref.entries()] == [5.0, 6.0, 7.0]
    # episode k lives in slot k % W: episodes 3, 4, 5 (envs 4, 5, 6) in slots 0, 1, 2
    assert ref.ep_env.tolist() == [4, 5, 6] and ref.ep_return.tolist() == [5.0, 6.0, 7.0]
    ref.step(np.ones((E, 1), np.uint8), rew, [0, 0, 1, 0, 0, 0, 0])      # env 2: two steps, 3 + 3
    assert ref.total == 7 and [e[4] for e in ref.entries()] == [5, 6, 2]
    assert ref.ep_env.tolist() == [2, 5, 6] and ref.ep_length.tolist() == [2, 1, 1] and ref.ep_return[0] == 6.0


def test_an_episode_open_at_begin_counts_from_zero():
    ref = T.MarlRingRef(1, 2, 2)
    one = np.ones((1, 2), np.uint8)
    ref.step(one, np.float32([[1.0, 1.0]]), [0])
    ref.step(one, np.float32([[1.0, 1.0]]), [0])
    ref.begin()
    assert ref.acc_steps.tolist() == [0] and ref.env_steps == 0 and ref.agent_steps.tolist() == [0, 0]
    ref.step(one, np.float32([[2.0, 3.0]]), [1])
    (ret, length, a_ret, a_len, env), = ref.entries()
    assert (ret, length) == (5.0, 1) and a_len.tolist() == [1, 1] and ref.total == 1


# ---- the torch backend's learner record ---------------------------------------------------------------------------------
def _update(model, **kw):
    from cattleherd.marl_ppo import MarlPPOUpdate
    import marl_ppo_ref as R
    hp = R.hp_for(eps=R.TRAIN_EPS)
    return MarlPPOUpdate(model, lr=hp["lr"], eps=hp["eps"], backend="torch", log_stats=True, seed=5, **kw), hp


@pytest.mark.parametrize("minibatch", [40, 1])
def test_last_log_equals_an_independent_evaluation_of_the_last_minibatch(minibatch):
    import torch
    import marl_ppo_ref as R
    rb = T.cpu_buffer(R.SMALL)
    m0 = R.make_model(R.SMALL, "cpu", torch.float64)
    m, mr = (R.make_model(R.SMALL, "cpu", torch.float64, like=m0) for _ in range(2))
    epochs = 2 if minibatch > 1 else 1
    upd, hp = _update(m, num_epochs=epochs, minibatch_size=minibatch)
    steps = upd.train(rb)
    want_steps, stats, klc, live = T.ref_train_log(mr, rb, hp, upd.kl_target, epochs, minibatch, 5)
    assert steps == want_steps == epochs * math.ceil(live / minibatch) and tuple(upd.stats.shape) == (steps, 8)
    assert list(upd.last_log) == T.LOG_KEYS
    last = stats[-1].numpy()
    want = {"policy_loss": last[0], "vf_loss": last[1], "entropy": last[2], "mean_kl_loss": last[3],
            "gradients_default_optimizer_global_norm": last[4], "vf_loss_unclipped": last[5], "total_loss": last[6],
            "vf_explained_var": last[7], "curr_kl_coeff": float(klc), "curr_entropy_coeff": hp["entropy_coeff"],
            "num_module_steps_trained": live * epochs}
    for k, w in want.items():
        g = upd.last_log[k]
        if k == "vf_explained_var" and minibatch == 1:
            assert math.isnan(g) and math.isnan(w)      # one row: 0 / 0
        else:
            assert g == pytest.approx(w, rel=1e-12, abs=1e-14), k
    assert upd.last_log["curr_kl_coeff"] == float(upd.kl_coeff)
    assert isinstance(upd.last_log["num_module_steps_trained"], int)
    if minibatch > 1:   # every step's row, not only the last
        assert np.allclose(upd.stats.numpy(), stats.numpy(), rtol=1e-12, atol=1e-14)
        assert bool((stats[:, 5] > stats[:, 1]).any()) and last[1] > 0.0      # the value clip is active on some rows


def test_log_stats_off_changes_nothing():
    import torch
    import marl_ppo_ref as R
    from cattleherd.marl_ppo import MarlPPOUpdate
    rb = T.cpu_buffer(R.SMALL)
    m0 = R.make_model(R.SMALL, "cpu", torch.float64)
    ma, mb = (R.make_model(R.SMALL, "cpu", torch.float64, like=m0) for _ in range(2))
    a = MarlPPOUpdate(ma, num_epochs=1, minibatch_size=40, backend="torch", seed=5)
    b = MarlPPOUpdate(mb, num_epochs=1, minibatch_size=40, backend="torch", seed=5, log_stats=True)
    a.train(rb), b.train(rb)
    assert tuple(a.stats.shape) == (3, 5) and a.last_log == {}
    assert torch.equal(a.stats, b.stats[:, :5]) and torch.equal(a.kl_coeff, b.kl_coeff)
    assert all(torch.equal(p, q) for p, q in zip(ma.parameters(), mb.parameters()))


def test_explained_variance_is_floored_at_minus_one_for_a_bad_critic():
    import torch
    import marl_ppo_ref as R
    rb = T.cpu_buffer(R.SMALL)
    m = R.make_model(R.SMALL, "cpu", torch.float64)
    with torch.no_grad():
        m.vf.weight.mul_(200.0)      # values that vary far more than the targets do
    y, v = rb.returns.view(-1), m.values(rb.obs.view(rb.T * rb.rows, -1)).detach()
    raw = 1.0 - float((y - v).var()) / (float(y.var()) + 1e-6)
    assert raw < -1.0
    upd, _ = _update(m, num_epochs=1, minibatch_size=1000)      # one minibatch of every live row
    upd.train(rb)
    assert upd.last_log["vf_explained_var"] == -1.0


# ---- MarlEpisodeRing.summary() over a ring filled from the host -----------------------------------------------------------
def _host_ring(E, N, W):
    import torch
    from cattleherd import _lib as L
    from cattleherd.train_log import MarlEpisodeRing
    batch = types.SimpleNamespace(mode=L.CH_MODE_MARL, torch=torch, device="cpu", n_envs=E, num_drones=N)
    return MarlEpisodeRing(batch, W)


def _fill(ring, ref):
    import torch
    for k, a in ref.arrays().items():
        getattr(ring, k).copy_(torch.as_tensor(a))


def test_summary_keys_and_the_since_last_call_count():
    E, N, W = 5, 3, 4
    live, reward, rh = T.synthetic(E, W, N, S=12)
    live[:, :, 2] = 0      # agent_2 takes part in no episode: it has no return key
    ref = T.MarlRingRef(E, N, W)
    ring = _host_ring(E, N, W)
    for t in range(6):
        ref.step(live[t], reward[t], rh[t])
    _fill(ring, ref)
    T.assert_ring(ring.arrays(), ref.arrays(), "host ring")
    T.assert_entries(ring.entries(), ref.entries())
    s = ring.summary()
    assert ref.total > W
    ent = ref.entries()
    keys = ["episode_return_mean", "episode_return_min", "episode_return_max", "episode_len_mean", "episode_len_min",
            "episode_len_max", "agent_episode_returns_mean/agent_0", "agent_episode_returns_mean/agent_1",
            "module_episode_returns_mean/shared_policy", "num_episodes", "num_env_steps_sampled",
            "num_agent_steps_sampled/agent_0", "num_agent_steps_sampled/agent_1", "num_agent_steps_sampled/agent_2"]
    assert sorted(s) == sorted(keys)
    assert s["episode_return_mean"] == np.mean([e[0] for e in ent]) == s["module_episode_returns_mean/shared_policy"]
    assert s["episode_return_min"] == min(e[0] for e in ent) and s["episode_return_max"] == max(e[0] for e in ent)
    assert s["episode_len_mean"] == np.mean([e[1] for e in ent]) and s["episode_len_max"] == max(e[1] for e in ent)
    took = [e for e in ent if e[3][1] > 0]
    assert 0 < len(took) and s["agent_episode_returns_mean/agent_1"] == np.mean([e[2][1] for e in took])
    assert s["num_episodes"] == ref.total and s["num_env_steps_sampled"] == 6 * E
    assert s["num_agent_steps_sampled/agent_0"] == int(live[:6, :, 0].sum()) and s["num_agent_steps_sampled/agent_2"] == 0
    assert ring.summary()["num_episodes"] == 0      # nothing since the previous call
    before = ref.total
    for t in range(6, 12):
        ref.step(live[t], reward[t], rh[t])
    _fill(ring, ref)
    assert ring.summary()["num_episodes"] == ref.total - before > 0


def test_rllib_result_nests_the_two_records():
    from cattleherd.train_log import rllib_result
    ring = _host_ring(2, 2, 3)
    upd = types.SimpleNamespace(last_log={})
    with pytest.raises(ValueError):
        rllib_result(ring, upd)
    upd.last_log = {k: 0.0 for k in T.LOG_KEYS}
    out = rllib_result(ring, upd)
    assert list(out) == ["env_runners", "learners"] and list(out["learners"]) == ["shared_policy"]
    assert list(out["learners"]["shared_policy"]) == T.LOG_KEYS and out["env_runners"]["num_episodes"] == 0


def test_ring_rejects_a_ctde_batch_and_an_empty_window():
    import torch
    from cattleherd import _lib as L
    from cattleherd.train_log import MarlEpisodeRing
    ctde = types.SimpleNamespace(mode=L.CH_MODE_CTDE, torch=torch, device="cpu", n_envs=2, num_drones=2)
    with pytest.raises(ValueError):
        MarlEpisodeRing(ctde)
    marl = types.SimpleNamespace(mode=L.CH_MODE_MARL, torch=torch, device="cpu", n_envs=2, num_drones=2)
    with pytest.raises(ValueError):
        MarlEpisodeRing(marl, 0)
