"""A numpy restatement of the per-agent episode table of the DTDE evaluation (csrc/ch_marl_eval.hip,
cattleherd/marl_eval.py), the reference the device table is compared with exactly.

The bookkeeping is RLlibMultiAgentWrapper's (rllib_envs/marl_wrapper.py:77-119) with the CTDE table's quota rule
(tests/eval_ref.py: SB3's ``episode_count_targets``): per env step, every agent live at the start of the step adds its
float32 reward to its float64 return and 1 to its length; where the env ended (every agent has terminated: the step's
``reset_happened``) the episode is filed under the env's quota, or ignored, and the env's accumulators return to 0.  A
truncation ends nothing.  Every float64 add is done one at a time in the order the recorder kernel does it -- step by
step per agent, then over the agents in index order from 0.0 -- so the sums agree to the bit.
"""
import numpy as np


class MarlEvalRef:
    def __init__(self, n_eval_episodes, n_envs, n_agents, capacity):
        self.n, self.E, self.N, self.C = int(n_eval_episodes), int(n_envs), int(n_agents), int(capacity)
        E, N, C = self.E, self.N, self.C
        self.counts = np.zeros(E, dtype="int")
        self.targets = np.array([(self.n + i) // E for i in range(E)], dtype="int")
        assert self.targets.max() <= C
        self.ep_return = np.zeros((E, C), np.float64)
        self.agent_return = np.zeros((E, C, N), np.float64)
        self.ep_length = np.zeros((E, C), np.int32)
        self.agent_length = np.zeros((E, C, N), np.int32)
        self.ep_end_step = np.zeros((E, C), np.int32)
        self.acc_return = np.zeros((E, N), np.float64)
        self.acc_length = np.zeros((E, N), np.int32)
        self.acc_steps = np.zeros(E, np.int32)
        self.live = np.zeros((E, N), np.uint8)
        self._filed = []   # (end step, env, slot) in filing order
        # ended episodes that are not counted: the env had reached its target / its target is 0
        self.ignored_full, self.ignored_zero = 0, 0

    def running(self):
        return bool((self.counts < self.targets).any())

    @property
    def remaining(self):
        return int((self.targets - self.counts).sum())

    def step(self, live, reward_f32, reset_happened, step_index):
        live = np.asarray(live).reshape(self.E, self.N)
        reward = np.asarray(reward_f32)
        assert reward.dtype == np.float32
        reward = reward.reshape(self.E, self.N)
        reset_happened = np.asarray(reset_happened).reshape(self.E)
        self.live = (live != 0).astype(np.uint8)
        for e in range(self.E):
            for i in range(self.N):
                if live[e, i]:   # (a reward of an agent that is not live is never read into a sum)
                    self.acc_return[e, i] = self.acc_return[e, i] + np.float64(reward[e, i])
                    self.acc_length[e, i] += 1
            self.acc_steps[e] += 1
            if not reset_happened[e]:
                continue
            if self.counts[e] < self.targets[e]:
                k = self.counts[e]
                total = np.float64(0.0)
                for i in range(self.N):
                    self.agent_return[e, k, i] = self.acc_return[e, i]
                    self.agent_length[e, k, i] = self.acc_length[e, i]
                    total = total + self.acc_return[e, i]
                self.ep_return[e, k], self.ep_length[e, k] = total, self.acc_steps[e]
                self.ep_end_step[e, k] = step_index
                self._filed.append((int(step_index), e, int(k)))
                self.counts[e] += 1
            elif self.targets[e] > 0:
                self.ignored_full += 1
            else:
                self.ignored_zero += 1
            self.acc_return[e], self.acc_length[e], self.acc_steps[e] = 0.0, 0, 0

    def arrays(self):
        """The table's arrays, in cattleherd.marl_eval.DeviceMarlEvalTable.ARRAYS' names and dtypes."""
        return {"quota": self.targets.astype(np.int32), "count": self.counts.astype(np.int32),
                "ep_return": self.ep_return.copy(), "agent_return": self.agent_return.copy(),
                "ep_length": self.ep_length.copy(), "agent_length": self.agent_length.copy(),
                "ep_end_step": self.ep_end_step.copy(), "remaining": np.array([self.remaining], np.int64),
                "acc_return": self.acc_return.copy(), "acc_length": self.acc_length.copy(),
                "acc_steps": self.acc_steps.copy(), "live": self.live.copy()}

    def episodes(self):
        """The filed episodes as DeviceMarlEvalTable.episodes() returns them: by end step, then env (the filing
        order: steps ascend and a step files its envs in index order)."""
        assert self._filed == sorted(self._filed)
        env = np.array([f[1] for f in self._filed], np.int64)
        slot = np.array([f[2] for f in self._filed], np.int64)
        end = np.array([f[0] for f in self._filed], np.int64)
        return (self.ep_return[env, slot], self.ep_length[env, slot].astype(np.int64), self.agent_return[env, slot],
                self.agent_length[env, slot].astype(np.int64), env, end)
