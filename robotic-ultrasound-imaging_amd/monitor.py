"""Episode statistics on the device: what SB3's Monitor wrapper (src/rl.py:39), `ep_info_buffer` and `evaluate_policy` give the reference's training loop --
rollout/ep_rew_mean, the quantity its curves are drawn in (src/utils/plot.py:420-436), and the mean return of n complete deterministic episodes -- for loops
that never leave the GPU.  The step kernels leave done / ep_return / ep_length behind every usim_step; `DeviceMonitor.record()` is one more small launch
(include/usim.h usim_monitor_step; csrc/usim_monitor.hip) that folds them into a block on the device, inside a recorded rollout as well.

    mon = env.attach_monitor(DeviceMonitor(env))           # BEFORE the collector is built: a recorded collector holds the launches of its capture
    collector = FusedRollout(env, policy, vecnorm, buffer)
    ppo = NativePPO(env, policy, vecnorm, buffer, collector); ppo.learn(40)
    write_scalar_csv("ep_rew_mean.csv", ppo.history, "rollout/ep_rew_mean")
    mean, std = evaluate_policy(env, policy, vecnorm, n_eval_episodes=100)
"""
import csv
import ctypes as C

import numpy as np
import torch

from . import _lib

_HEAD = _lib.MONITOR_HEADER_WORDS
_ROW = _lib.MONITOR_ROW_WORDS


class DeviceMonitor:
    """SB3's Monitor + `ep_info_buffer = deque(maxlen=window)` for all environments of `env`, on the device.  window: SB3's stats_window_size (100).
    targets (int [n], optional): environment i is counted at most targets[i] times -- evaluate_policy's bookkeeping; the monitor then owns the count array too.

    record() is called by env.step_tensor while the monitor is attached (env.attach_monitor); nothing here synchronises but summary() / episodes()."""

    def __init__(self, env, window=100, targets=None):
        self.env, self.window = env, int(window)
        self.lib = _lib.load()
        dev = env.device
        self.block = torch.zeros(_lib.monitor_words(self.window), dtype=torch.int32, device=dev)          # all zero: an empty monitor
        self.targets = self.counts = None
        if targets is not None:
            t = torch.as_tensor(targets, device=dev).to(torch.int32).contiguous()
            if tuple(t.shape) != (env.num_envs,):
                raise ValueError(f"targets must have shape {(env.num_envs,)}, got {tuple(t.shape)}")
            self.targets, self.counts = t, torch.zeros(env.num_envs, dtype=torch.int32, device=dev)

    def record(self):
        """one usim_monitor_step on the env's stream, from the env's own step buffers (done, episode_return, episode_length) and horizon.  Capture-safe."""
        env = self.env
        ptr = lambda x: None if x is None else x.data_ptr()
        _lib.check(self.lib, self.lib.usim_monitor_step(C.byref(env._io), env.num_envs, self.window, int(env.horizon), ptr(self.targets), ptr(self.counts),
                                                        self.block.data_ptr(), env._stream()))

    def reset(self):
        """an empty monitor again (and zero counts): in-place zero_(), capturable"""
        self.block.zero_()
        if self.counts is not None:
            self.counts.zero_()

    def _host(self):
        """the block on the host (ONE device-to-host copy) -> (episodes, length_sum, return_sum, truncated, launches, live ring rows [m][4] int32, oldest first)"""
        w = self.block.cpu().numpy()
        head = w[:_HEAD]
        episodes, length_sum, truncated, launches = (int(head[2 * k:2 * k + 2].view(np.int64)[0]) for k in (0, 1, 3, 4))
        return_sum = float(head[4:6].view(np.float64)[0])
        ring = w[_HEAD:].reshape(self.window, _ROW)
        if episodes > self.window:                                   # full: the oldest live row is the one the next episode will take
            ring = np.roll(ring, -(episodes % self.window), axis=0)
        return episodes, length_sum, return_sum, truncated, launches, ring[:min(episodes, self.window)]

    def summary(self):
        """SB3's logger names.  rollout/ep_rew_mean, rollout/ep_len_mean: safe_mean over the ring (the last min(episodes, window) episodes; NaN when there are
        none), in float64; rollout/episodes, rollout/truncated: counted over the monitor's life; rollout/ep_rew_mean_all, rollout/ep_len_mean_all: the life-time
        sums over episodes.  One device-to-host copy (it waits for the stream)."""
        episodes, length_sum, return_sum, truncated, _, rows = self._host()
        nan = float("nan")
        live = len(rows) > 0
        return {"rollout/ep_rew_mean": float(np.mean(rows[:, 0].view(np.float32).astype(np.float64))) if live else nan,
                "rollout/ep_len_mean": float(np.mean(rows[:, 1].astype(np.float64))) if live else nan,
                "rollout/episodes": episodes, "rollout/truncated": truncated,
                "rollout/ep_rew_mean_all": return_sum / episodes if episodes else nan,
                "rollout/ep_len_mean_all": length_sum / episodes if episodes else nan}

    def episodes(self):
        """the live ring rows, oldest first: [{"r": return, "l": length, "env": environment index, "step": number of the record() that counted it}]"""
        rows = self._host()[5]
        r = rows[:, 0].view(np.float32)
        return [{"r": float(r[k]), "l": int(rows[k, 1]), "env": int(rows[k, 2]), "step": int(rows[k, 3]) & 0xffffffff} for k in range(len(rows))]

    def episode_count(self):
        """episodes counted so far (a 8-byte device-to-host copy; waits for the stream)"""
        return int(self.block[:2].cpu().numpy().view(np.int64)[0])


def eval_targets(n_eval_episodes, n_envs):
    """SB3 evaluate_policy's episode_count_targets: (n_eval_episodes + i) // n_envs for environment i -- they sum to n_eval_episodes"""
    return [(int(n_eval_episodes) + i) // int(n_envs) for i in range(int(n_envs))]


def _evaluation_run(env, policy, vecnorm, mon, observers, n_eval, targets, deterministic, seed, check_every, what):
    """The loop of evaluate_policy (and of evaluation.evaluate_episodes): reset, then FusedRollout.act(training=0) and env.step_tensor with `mon` and
    `observers` attached -- and nothing else: the monitor and the observers that were attached before are taken off first and put back afterwards, in their
    order, whatever happens -- until mon has counted n_eval episodes (read every `check_every` steps) or max(targets) * env.horizon steps have run
    (RuntimeError).  -> mon.episodes()"""
    from .policy import DeviceRolloutBuffer, FusedRollout
    n = env.num_envs
    before = env.detach_monitor()                                   # (FusedRollout's constructor does not step, but nothing of this run may reach `before`)
    others = env.detach_observer()
    try:
        fr = FusedRollout(env, policy, vecnorm, DeviceRolloutBuffer(1, n, _lib.OBS_DIM, env.action_dim, device=env.device), seed=seed, graph=False, init_stats=False)
        obs = env.reset_tensor()
        env.attach_monitor(mon)
        for o in observers:
            env.attach_observer(o)
        fr.pack()                                                   # the weights do not change inside the loop
        bound, every, got = max(targets) * int(env.horizon), max(1, int(check_every)), 0
        for k in range(bound):
            act, _ = fr.act(obs, None, counter=k, training=0, deterministic=deterministic, pack=False)
            obs, _, _ = env.step_tensor(act)
            if (k + 1) % every == 0 or k + 1 == bound:
                got = mon.episode_count()
                if got >= n_eval:
                    break
        if got < n_eval:
            raise RuntimeError(f"{what}: {got} of {n_eval} episodes after {bound} steps (max(target) x horizon)")
        return mon.episodes()
    finally:
        env.detach_monitor()
        env.detach_observer()
        if before is not None:
            env.attach_monitor(before)
        for o in others:
            env.attach_observer(o)


def evaluate_policy(env, policy, vecnorm, n_eval_episodes=10, deterministic=True, seed=0, check_every=50, return_episode_rewards=False):
    """stable_baselines3.common.evaluation.evaluate_policy (what EvalCallback and src/rl.py's `training: False` branch run) on the device: n_eval_episodes
    complete episodes, environment i contributing its first (n_eval_episodes + i) // n_envs, their returns the raw Monitor returns.  The env is reset, then an
    eager loop of FusedRollout.act(training=0: the statistics of `vecnorm` are frozen, never updated) and env.step_tensor runs with a fresh DeviceMonitor
    (window = n_eval_episodes: the ring holds every counted episode) attached; the host reads the episode count every `check_every` steps and stops at
    n_eval_episodes.  An episode cannot outlast env.horizon, so the loop is bounded by max(target) * env.horizon steps; RuntimeError if that bound is reached
    short of the count.  A monitor that was attached before is attached again afterwards, its block untouched; so are the env's observers.
    -> (mean, std) = np.mean / np.std of the episode returns in the order SB3 appends them (step by step, ascending environment index); with
    return_episode_rewards=True (episode returns, episode lengths) as two lists instead."""
    n_eval = int(n_eval_episodes)
    if n_eval < 1:
        raise ValueError("n_eval_episodes must be at least 1")
    targets = eval_targets(n_eval, env.num_envs)
    mon = DeviceMonitor(env, window=n_eval, targets=targets)
    eps = _evaluation_run(env, policy, vecnorm, mon, (), n_eval, targets, deterministic, seed, check_every, "evaluate_policy")
    returns, lengths = [e["r"] for e in eps], [e["l"] for e in eps]
    if return_episode_rewards:
        return returns, lengths
    return float(np.mean(returns)), float(np.std(returns))


def write_scalar_csv(path, rows, tag):
    """One scalar of a training log (ppo.NativePPO.history: a list of dicts) as TensorBoard's CSV export -- the columns `Wall time,Step,Value` that
    src/utils/plot.py plot_training_rew_mean reads: one line per row that holds `tag`, Step = the row's time/total_timesteps, Wall time = its time/wall
    (0 where absent).  Returns the number of lines written."""
    lines = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Wall time", "Step", "Value"])
        for row in rows:
            if tag in row:
                w.writerow([repr(float(row.get("time/wall", 0.0))), int(row["time/total_timesteps"]), repr(float(row[tag]))])
                lines += 1
    return lines
