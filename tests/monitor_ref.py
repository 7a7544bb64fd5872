"""Plain-Python restatement of what usim_monitor_step / monitor.DeviceMonitor / monitor.evaluate_policy / usim_explained_variance compute -- stable-baselines3's
own bookkeeping, written the way SB3 writes it:
  - MonitorRef: `ep_info_buffer = deque(maxlen=window)` fed by `_update_info_buffer(infos)` in environment order, with evaluate_policy's target gating and the
    life-time totals of the device block
  - sb3_evaluate_bookkeeping: the loop body of stable_baselines3.common.evaluation.evaluate_policy over recorded (done, return, length) steps
  - explained_variance: stable_baselines3.common.utils.explained_variance in float64 numpy
No GPU, no library: the tests compare the device results with these."""
from collections import deque

import numpy as np


def eval_targets(n_eval_episodes, n_envs):
    """evaluate_policy: episode_count_targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)])"""
    return [(int(n_eval_episodes) + i) // int(n_envs) for i in range(int(n_envs))]


class MonitorRef:
    def __init__(self, n, window, horizon=0, targets=None):
        self.n, self.window, self.horizon = int(n), int(window), int(horizon)
        self.buffer = deque(maxlen=self.window)                      # rows (return as float32, length, env, launch)
        self.targets = None if targets is None else [int(t) for t in targets]
        self.counts = [0] * self.n
        self.episodes = self.length_sum = self.truncated = self.launches = 0
        self.return_sum = 0.0                                        # float64, environment order
        self.abs_sum_bound = 0.0                                     # sum over launches of 2 n 2^-53 sum |r_i|: the bound of float64 summation in any order

    def step(self, done, ep_return, ep_length):
        """one launch: done [n] (any non-zero byte), ep_return [n] float32, ep_length [n] int32"""
        done, ep_return, ep_length = np.asarray(done), np.asarray(ep_return, dtype=np.float32), np.asarray(ep_length)
        c, abs_sum = 0, 0.0
        for i in range(self.n):
            if done[i] == 0:
                continue
            if self.targets is not None:
                if self.counts[i] >= self.targets[i]:
                    continue
                self.counts[i] += 1
            r, l = np.float32(ep_return[i]), int(ep_length[i])
            self.buffer.append((r, l, i, self.launches & 0xffffffff))
            self.episodes += 1
            self.length_sum += l
            self.return_sum += float(r)
            self.truncated += int(self.horizon > 0 and l >= self.horizon)
            c += 1
            abs_sum += abs(float(r))
        self.abs_sum_bound += 2.0 * self.n * 2.0 ** -53 * abs_sum
        self.launches += 1
        return c

    def rows(self):
        """the live rows, oldest first, as int32 [m][4]: return bits, length, env, launch"""
        out = np.zeros((len(self.buffer), 4), dtype=np.int64)
        for k, (r, l, i, s) in enumerate(self.buffer):
            out[k] = (int(np.array([r], dtype=np.float32).view(np.uint32)[0]), l, i, s)
        return out.astype(np.uint32).view(np.int32)

    def summary(self):
        nan = float("nan")
        r = [float(x[0]) for x in self.buffer]
        l = [float(x[1]) for x in self.buffer]
        return {"rollout/ep_rew_mean": float(np.mean(r)) if r else nan, "rollout/ep_len_mean": float(np.mean(l)) if l else nan,
                "rollout/episodes": self.episodes, "rollout/truncated": self.truncated,
                "rollout/ep_rew_mean_all": self.return_sum / self.episodes if self.episodes else nan,
                "rollout/ep_len_mean_all": self.length_sum / self.episodes if self.episodes else nan}


def sb3_evaluate_bookkeeping(steps, n_envs, n_eval_episodes):
    """evaluate_policy's loop over `steps`, an iterable of (done [n], episode return [n], episode length [n]) per env step (the Monitor's info["episode"] where
    done): `if episode_counts[i] < episode_count_targets[i]: if dones[i]: append; episode_counts[i] += 1`, until the counts reach the targets.
    -> (episode_rewards, episode_lengths) in SB3's append order; raises if the steps run out first."""
    targets = np.array(eval_targets(n_eval_episodes, n_envs), dtype=int)
    counts = np.zeros(n_envs, dtype=int)
    rewards, lengths = [], []
    for done, ret, length in steps:
        if not (counts < targets).any():
            break
        for i in range(n_envs):
            if counts[i] < targets[i] and done[i]:
                rewards.append(float(np.float32(ret[i])))
                lengths.append(int(length[i]))
                counts[i] += 1
    if (counts < targets).any():
        raise RuntimeError(f"the recorded steps hold {int(counts.sum())} of {n_eval_episodes} episodes")
    return rewards, lengths


def explained_variance(values, returns):
    """SB3: var_y = np.var(y_true); np.nan if var_y == 0 else 1 - np.var(y_true - y_pred) / var_y -- on float64 copies"""
    y_pred, y_true = np.asarray(values, dtype=np.float64).ravel(), np.asarray(returns, dtype=np.float64).ravel()
    var_y = np.var(y_true)
    return float("nan") if var_y == 0 else float(1.0 - np.var(y_true - y_pred) / var_y)
