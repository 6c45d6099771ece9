"""A literal numpy restatement of stable_baselines3 ``evaluate_policy``'s bookkeeping (targets, counts, append order),
the reference of the device episode table (csrc/ch_eval.hip, cattleherd/eval_policy.py).

SB3 (common/evaluation.py), per ``env.step`` of a VecEnv of ``n_envs`` envs::

    episode_counts = np.zeros(n_envs, dtype="int")
    episode_count_targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")
    while (episode_counts < episode_count_targets).any():
        ... step ...
        for i in range(n_envs):
            if episode_counts[i] < episode_count_targets[i]:
                if dones[i] and "episode" in infos[i]:
                    episode_rewards.append(info["episode"]["r"]); episode_lengths.append(info["episode"]["l"])
                    episode_counts[i] += 1

Here a step is the arrays the device step writes: ``reset_happened`` [E] (the env's episode ended and it auto-reset),
``episode_stats`` [E, 2] (Monitor's "r" and "l"), ``terminated`` / ``truncated`` [E].  Beside SB3's lists the
reference keeps the same episodes in the table's layout ([E, C], slot = the env's count), so a test compares every
device array exactly.
"""
import numpy as np


class EvalRef:
    def __init__(self, n_eval_episodes, n_envs, capacity):
        self.n, self.E, self.C = int(n_eval_episodes), int(n_envs), int(capacity)
        self.counts = np.zeros(self.E, dtype="int")
        self.targets = np.array([(self.n + i) // self.E for i in range(self.E)], dtype="int")
        assert self.targets.max() <= self.C
        # SB3's lists, and with them what the table also keeps of each episode
        self.episode_rewards, self.episode_lengths = [], []
        self.episode_flags, self.episode_env, self.episode_end_step = [], [], []
        self.ep_return = np.zeros((self.E, self.C), np.float64)
        self.ep_length = np.zeros((self.E, self.C), np.int32)
        self.ep_flags = np.zeros((self.E, self.C), np.uint8)
        self.ep_end_step = np.zeros((self.E, self.C), np.int32)
        # episodes SB3 does not count: ended in an env that had reached its target / whose target is 0
        self.ignored_full, self.ignored_zero = 0, 0

    def running(self):
        """SB3's while condition."""
        return bool((self.counts < self.targets).any())

    @property
    def remaining(self):
        return int((self.targets - self.counts).sum())

    def step(self, reset_happened, episode_stats, terminated, truncated, step_index):
        reset_happened = np.asarray(reset_happened).reshape(self.E)
        episode_stats = np.asarray(episode_stats, np.float64).reshape(self.E, 2)
        terminated, truncated = np.asarray(terminated).reshape(self.E), np.asarray(truncated).reshape(self.E)
        for i in range(self.E):
            if self.counts[i] < self.targets[i]:
                if reset_happened[i]:
                    r, n = float(episode_stats[i, 0]), int(episode_stats[i, 1])
                    f = (1 if terminated[i] else 0) | (2 if truncated[i] else 0)
                    self.episode_rewards.append(r)
                    self.episode_lengths.append(n)
                    self.episode_flags.append(f)
                    self.episode_env.append(i)
                    self.episode_end_step.append(int(step_index))
                    k = self.counts[i]
                    self.ep_return[i, k], self.ep_length[i, k] = r, n
                    self.ep_flags[i, k], self.ep_end_step[i, k] = f, step_index
                    self.counts[i] += 1
            elif reset_happened[i]:
                if self.targets[i] > 0:
                    self.ignored_full += 1
                else:
                    self.ignored_zero += 1

    def arrays(self):
        """The table's arrays, in cattleherd.eval_policy.DeviceEvalTable.ARRAYS' names and dtypes."""
        return {"quota": self.targets.astype(np.int32), "count": self.counts.astype(np.int32),
                "ep_return": self.ep_return.copy(), "ep_length": self.ep_length.copy(),
                "ep_flags": self.ep_flags.copy(), "ep_end_step": self.ep_end_step.copy(),
                "remaining": np.array([self.remaining], np.int64)}

    def episodes(self):
        """SB3's lists as DeviceEvalTable.episodes() returns them."""
        return (np.asarray(self.episode_rewards, np.float64), np.asarray(self.episode_lengths, np.int64),
                np.asarray(self.episode_flags, np.uint8), np.asarray(self.episode_env, np.int64),
                np.asarray(self.episode_end_step, np.int64))
