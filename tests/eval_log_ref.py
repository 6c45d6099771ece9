"""numpy reference of the device-side evaluator log (cattleherd.eval_log; ch_eval_log_*), for tests.

``reference_rows`` drives a batch (a ``HerdBatch``, or tests/fake_batch.py's ``FakeBatch`` over the CPU oracle) one step
at a time through the only route the library offered before the log existed: mark from ``get_state()``, step with
``autoreset=False``, build each logged env's row from ``get_state()`` / ``eval_distances()`` /
``evaluation.herding_effectiveness`` / ``evaluation.failure_truncation``, reset with ``reset(mask=done)``.  Besides the
rows (the layout of ``DeviceEvalLog.arrays()``) it reports per row the smallest distance of any of the four threshold
comparisons of ``failure_truncation``, and of ep_time vs the episode length, from its threshold: a test asserts that
margin so that a near-tie cannot hide (or cause) a mismatch of the flags.
"""
import numpy as np

from cattleherd.evaluation import failure_truncation, herding_effectiveness

TARGET_ALT, MAX_ALT_ERROR, COLLISION, MAX_FORMATION, MISSION_BOUNDARY = 0.45, 0.27, 0.2, 8.0, 15.0
ROW_ARRAYS = ("time", "effectiveness", "num_drones", "episode", "flags", "drone_xy", "drone_vxy", "drone_dist",
              "cattle_xy", "cattle_vxy")


def threshold_margin(state, e, n, ep_time, episode_len):
    """min |value - threshold| over every comparison that decides the time-out trigger of env ``e``."""
    pos = np.asarray(state["drone_pos"][e, :n], np.float64)
    m = [abs(ep_time - episode_len)]
    m.append(np.min(np.abs(np.abs(pos[:, 2] - TARGET_ALT) - MAX_ALT_ERROR)))
    xy = pos[:, :2]
    d = np.linalg.norm(xy[:, None, :] - xy[None, :, :], axis=-1)[np.triu_indices(n, 1)]
    if d.size:
        m.append(np.min(np.abs(d - COLLISION)))
        m.append(np.min(np.abs(d - MAX_FORMATION)))
    herd = np.asarray(state["cow_pos"][e], np.float64).mean(axis=0)
    m.append(abs(np.linalg.norm(xy.mean(axis=0) - herd) - MISSION_BOUNDARY))
    return float(np.nanmin(m))


def _sliced(state, N, M):
    """The state with exactly N drone and M cow slots per env (the oracle's dicts are padded to its maxima)."""
    out = dict(state)
    for k in ("drone_pos", "drone_vel"):
        out[k] = np.asarray(state[k])[:, :N]
    for k in ("cow_pos", "cow_vel"):
        out[k] = np.asarray(state[k])[:, :M]
    return out


def reference_rows(batch, envs, actions, episode_len, ctrl_freq=60):
    """``actions``: float32 [steps, E, N, 4].  Returns (arrays, margins, done): ``arrays`` as
    ``DeviceEvalLog.arrays()`` gives them (rows = steps, nothing dropped), ``margins`` float64 [S, steps] and ``done``
    bool [steps, E] (terminated | truncated of every env)."""
    torch = batch.torch
    envs = np.asarray(envs, np.int64)
    S, T, E, N, M = len(envs), len(actions), batch.n_envs, batch.num_drones, batch.num_cattle
    a = {"time": np.zeros((S, T)), "effectiveness": np.zeros((S, T)), "num_drones": np.zeros((S, T), np.int32),
         "episode": np.zeros((S, T), np.int32), "flags": np.zeros((S, T), np.uint8),
         "drone_xy": np.zeros((S, T, N, 2)), "drone_vxy": np.zeros((S, T, N, 2)), "drone_dist": np.zeros((S, T, N)),
         "cattle_xy": np.zeros((S, T, M, 2)), "cattle_vxy": np.zeros((S, T, M, 2))}
    margins = np.zeros((S, T))
    done_all = np.zeros((T, E), bool)
    for t in range(T):
        s0 = _sliced(batch.get_state(), N, M)                                      # 1. mark
        batch.step(torch.from_numpy(np.ascontiguousarray(actions[t], np.float32)).to(batch.device), autoreset=False)  # 2.
        s1 = _sliced(batch.get_state(), N, M)                                      # 3. the rows
        dist = np.asarray(batch.eval_distances(), np.float64)
        te = batch.terminated.cpu().numpy()[:, 0] != 0
        tr = batch.truncated.cpu().numpy()[:, 0] != 0
        for s, e in enumerate(envs):
            n = int(s1["n"][e])
            ep_time = int(s0["step_counter"][e]) / ctrl_freq
            a["time"][s, t] = ep_time
            a["effectiveness"][s, t] = herding_effectiveness(s1["cow_pos"][e], s1["drone_pos"][e, :n, :2])
            a["num_drones"][s, t] = n
            a["episode"][s, t] = int(s1["episode"][e])
            timeout = ep_time > episode_len and not failure_truncation(s1, e, n)
            a["flags"][s, t] = (1 if te[e] else 0) | (2 if tr[e] else 0) | (4 if timeout else 0)
            a["drone_xy"][s, t, :n] = s1["drone_pos"][e, :n, :2]
            a["drone_vxy"][s, t, :n] = s1["drone_vel"][e, :n, :2]
            a["drone_dist"][s, t, :n] = dist[e, :n]
            a["cattle_xy"][s, t] = s1["cow_pos"][e]
            a["cattle_vxy"][s, t] = s0["cow_vel"][e]
            margins[s, t] = threshold_margin(s1, e, n, ep_time, episode_len)
        done = te | tr
        done_all[t] = done
        batch.reset(mask=torch.from_numpy(done.astype(np.uint8)))                  # 4.
    a["sel_env"] = envs.astype(np.int32)
    a["rows"] = np.full(S, T, np.int32)
    a["dropped"] = np.zeros(S, np.int32)
    return a, margins, done_all


# ---- directed states: episodes that end inside the logged window -------------------------------------------------------
def _rest(s, n):
    """The first ``n`` drones hovering at rest at the target altitude with a clean PID (tests/directed_states.py)."""
    for k in ("drone_vel", "drone_angv", "pid_last_rpy", "pid_int_pos", "pid_int_rpy", "last_rpm", "rpy_rates"):
        s[k][:, :n] = 0
    for k in ("drone_quat", "drone_qlag"):
        s[k][:, :n] = (0, 0, 0, 1)
    s["drone_pos"][:, :n, 2] = TARGET_ALT


def timeout_state(state, n, m, step_counter):
    """Every env of a freshly reset batch's ``get_state()`` a few steps before its time limit: the ``n`` drones at rest
    in a 1.5 m formation about the centroid of the ``m`` cows (no failure condition near), ``step_counter`` as given
    (not a multiple of ctrl_freq away from the limit: ep_time never equals the episode length)."""
    s = {k: np.array(v) for k, v in state.items()}
    _rest(s, n)
    ang = 2 * np.pi * (np.arange(n) + 0.25) / n
    ring = 1.5 * np.stack([np.cos(ang), np.sin(ang)], -1)
    s["drone_pos"][:, :n, :2] = s["cow_pos"][:, :m].mean(axis=1)[:, None, :] + ring[None]
    s["step_counter"] = np.full_like(s["step_counter"], step_counter)
    return s


def collision_state(state, n, m, gap=0.25):
    """As ``timeout_state`` early in the episode, but drone 1 at rest ``gap`` metres along x from drone 0: with
    ``closing_actions`` the pair closes below the collision threshold within a few steps."""
    s = timeout_state(state, n, m, 40)
    s["drone_pos"][:, 1, :2] = s["drone_pos"][:, 0, :2] + np.array([gap, 0.0])
    return s


def closing_actions(steps, E, N):
    """Drone 0 flies +x and drone 1 flies -x at full speed; the others hover."""
    a = np.zeros((steps, E, N, 4), np.float32)
    a[:, :, 0] = (1, 0, 0, 1)
    a[:, :, 1] = (-1, 0, 0, 1)
    return a


# ---- comparing evaluation_data() dicts --------------------------------------------------------------------------------------
def same(x, y, path=""):
    if isinstance(x, (list, tuple)):
        assert isinstance(y, (list, tuple)) and len(x) == len(y), path
        for i, (p, q) in enumerate(zip(x, y)):
            same(p, q, f"{path}[{i}]")
    else:
        p, q = np.asarray(x), np.asarray(y)
        assert p.shape == q.shape and np.array_equal(p, q), path


def alias_pattern(data):
    """Which distance arrays of the pickle are the same object: every leaf of ``distances`` and
    ``distances_per_step`` numbered by first appearance."""
    seen, out = {}, []

    def walk(x):
        if isinstance(x, list):
            for v in x:
                walk(v)
        else:
            out.append(seen.setdefault(id(x), len(seen)))
    walk(data["distances"])
    walk(data["distances_per_step"])
    return out
