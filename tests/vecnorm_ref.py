"""Float64 numpy restatement of SB3's RunningMeanStd and VecNormalize: the yardstick of the device-side VecNormalize
(cattleherd/vec_normalize.py, csrc/ch_norm.hip).  SB3 is not installed here: written from the formulas of its source,
"parity unpinned".  The env is outside: ``reset`` and ``step`` are fed what the env returned."""
import numpy as np


class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        self.update_from_moments(np.mean(x, axis=0), np.var(x, axis=0), x.shape[0])

    def update_from_moments(self, bm, bv, bn):
        delta = bm - self.mean
        tot = self.count + bn
        m_a = self.var * self.count
        m_b = bv * bn
        m2 = m_a + m_b + np.square(delta) * self.count * bn / tot
        self.mean = self.mean + delta * bn / tot
        self.var = m2 / tot
        self.count = tot


class VecNormalize:
    def __init__(self, n_envs, obs_shape, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0,
                 clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        self.obs_rms, self.ret_rms = RunningMeanStd(obs_shape), RunningMeanStd(())
        self.ret = np.zeros(n_envs, np.float64)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon

    def normalize_obs(self, obs):
        obs = np.asarray(obs, np.float32)
        if not self.norm_obs:
            return obs
        q = (obs.astype(np.float64) - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon)
        return np.clip(q, -self.clip_obs, self.clip_obs).astype(np.float32)

    def normalize_reward(self, reward):
        reward = np.asarray(reward, np.float32)
        if not self.norm_reward:
            return reward
        q = reward.astype(np.float64) / np.sqrt(self.ret_rms.var + self.epsilon)
        return np.clip(q, -self.clip_reward, self.clip_reward).astype(np.float32)

    def reset(self, obs):
        self.ret = np.zeros_like(self.ret)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def step(self, obs, reward, done, terminal_obs=None):
        """After an env step (``obs``: already the auto-reset one where ``done``): returns ``(obs_n, reward_n,
        terminal_obs_n)``, the last one rows of ``terminal_obs[done]`` normalised with the updated statistics."""
        done = np.asarray(done, bool)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)                                    # 1
        obs_n = self.normalize_obs(obs)                                 # 2
        if self.training:
            self.ret = self.ret * self.gamma + np.asarray(reward, np.float32).astype(np.float64)   # 3
            self.ret_rms.update(self.ret)
        reward_n = self.normalize_reward(reward)                        # 4
        term_n = None if terminal_obs is None else self.normalize_obs(np.asarray(terminal_obs)[done])   # 5
        self.ret[done] = 0.0                                            # 6
        return obs_n, reward_n, term_n

    def state_dict(self):
        return {"obs_mean": self.obs_rms.mean.copy(), "obs_var": self.obs_rms.var.copy(), "obs_count": self.obs_rms.count,
                "ret_mean": float(self.ret_rms.mean), "ret_var": float(self.ret_rms.var), "ret_count": self.ret_rms.count,
                "ret": self.ret.copy(), "training": self.training, "norm_obs": self.norm_obs,
                "norm_reward": self.norm_reward, "clip_obs": self.clip_obs, "clip_reward": self.clip_reward,
                "gamma": self.gamma, "epsilon": self.epsilon}

    def load_state_dict(self, s):
        self.obs_rms.mean, self.obs_rms.var = np.array(s["obs_mean"], np.float64), np.array(s["obs_var"], np.float64)
        self.obs_rms.count = float(s["obs_count"])
        self.ret_rms.mean, self.ret_rms.var = np.float64(s["ret_mean"]), np.float64(s["ret_var"])
        self.ret_rms.count = float(s["ret_count"])
        self.ret = np.array(s["ret"], np.float64)
        for k in ("training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon"):
            setattr(self, k, s[k])
        return self


def abs_terms(batches):
    """The derived tolerance's ingredients for the running statistics after ``update`` over ``batches`` (a list of
    float [n_k, ...] arrays) from the initial state: ``(n, sum_abs_mean_terms, sum_abs_var_terms)``.  The running mean
    is the sum of the terms x_i / tot (the prior's mean is 0); the running variance the sum of (x_i - mean)^2 / tot and
    the prior's var * count / tot + mean^2 * count / tot (its deviation from the merged mean), tot = 1e-4 + n: every
    term as the test computes it from the input in float64."""
    x = np.concatenate([np.asarray(b, np.float64) for b in batches], axis=0)
    n = x.shape[0]
    tot = 1e-4 + n
    mean = x.sum(axis=0) / tot
    mean_terms = np.abs(x).sum(axis=0) / tot
    var_terms = (np.square(x - mean).sum(axis=0) + 1e-4 * (1.0 + np.square(mean))) / tot
    return n, mean_terms, var_terms
