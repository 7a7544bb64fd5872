"""Evaluation runs on the device: the reference evaluates a trained policy with `save_data: True`, dumps 24 CSV files per episode (ultrasound.py:552-614) and
turns them into thirteen error metrics (src/utils/error.py:148-191).  Here both stay on the GPU for every environment of a batch: `DeviceEpisodeMetrics` keeps
the metrics of finished episodes in a ring (include/usim.h usim_metrics_step), `EpisodeRecorder` keeps whole episodes of a few chosen environments
(usim_record_step) and writes the reference's files from them, `evaluate_episodes` is monitor.evaluate_policy with both attached -- returns, lengths and metrics
of exactly the episodes SB3's evaluate_policy counts.  Both classes are observers of an env (env.attach_observer): step_tensor feeds them after every step, inside
a recorded rollout as well; nothing here synchronises but the reads.

    res = evaluate_episodes(env, policy, vecnorm, n_eval_episodes=4096, record_envs=[0, 1])
    res["metrics"]["force_mse"].mean(); res["recorder"].write_csv("eval_run")       # error.py's numbers; the files plot.py and error.py read
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .episode_log import _CHANNELS, _save
from .error_metrics import METRICS
from .monitor import DeviceMonitor, _evaluation_run, eval_targets

_HEAD = _lib.METRICS_HEADER_WORDS
_ROW = _lib.METRICS_ROW_WORDS
_M = _lib.METRICS
assert len(METRICS) == _M


class DeviceEpisodeMetrics:
    """The thirteen metrics of error_metrics.METRICS for every finished episode of every environment of `env`, on the device: a ring of the last `window`
    episodes in the order SB3 walks them (step by step, ascending environment index) and life-time sums.  targets (int [n], optional): environment i is
    counted at most targets[i] times -- evaluate_policy's bookkeeping, with a count array of this object's own.  Turns the step log on.

    record() is called by env.step_tensor while the object is attached (env.attach_observer); nothing here synchronises but the host reads, each of which is
    ONE device-to-host copy of the block."""

    def __init__(self, env, window=100, targets=None):
        self.env, self.window = env, int(window)
        self.lib = _lib.load()
        dev = env.device
        self.block = torch.zeros(_lib.metrics_words(env.num_envs, self.window), dtype=torch.int32, device=dev)          # all zero: an empty block
        self._live = _HEAD + _ROW * self.window                       # header + ring: what the host reads
        self.targets = self.counts = None
        if targets is not None:
            t = torch.as_tensor(targets, device=dev).to(torch.int32).contiguous()
            if tuple(t.shape) != (env.num_envs,):
                raise ValueError(f"targets must have shape {(env.num_envs,)}, got {tuple(t.shape)}")
            self.targets, self.counts = t, torch.zeros(env.num_envs, dtype=torch.int32, device=dev)
        if env.step_log is None:
            env.enable_step_log(True)

    def record(self):
        """one usim_metrics_step on the env's stream, from the env's own step record and done flags.  Capture-safe."""
        env = self.env
        ptr = lambda x: None if x is None else x.data_ptr()
        _lib.check(self.lib, self.lib.usim_metrics_step(C.byref(env._io), env.num_envs, self.window, int(env.horizon), ptr(self.targets), ptr(self.counts),
                                                        self.block.data_ptr(), env._stream()))

    def reset(self):
        """an empty block again (accumulators and counts included): in-place zero_(), capturable"""
        self.block.zero_()
        if self.counts is not None:
            self.counts.zero_()

    def _host(self):
        """header and ring on the host (ONE device-to-host copy) -> (header dict, live ring rows [k][32] int32, oldest first)"""
        w = self.block[:self._live].cpu().numpy()
        i64 = w[:8].view(np.int64)
        f64 = w[8:8 + 4 * _M].view(np.float64)
        head = {"episodes": int(i64[0]), "launches": int(i64[1]), "length_sum": int(i64[2]), "nonfinite": int(i64[3]), "total": f64[:_M].copy(),
                "total_sq": f64[_M:].copy()}
        ring = w[_HEAD:].reshape(self.window, _ROW)
        if head["episodes"] > self.window:                            # full: the oldest live row is the one the next episode will take
            ring = np.roll(ring, -(head["episodes"] % self.window), axis=0)
        return head, ring[:min(head["episodes"], self.window)]

    def episodes(self):
        """the live ring rows, oldest first: [{"env": environment index, "l": episode length, "step": number of the record() that counted it, <13 metrics>}]"""
        rows = self._host()[1]
        vals = np.ascontiguousarray(rows[:, :2 * _M]).view(np.float64).reshape(len(rows), _M)
        return [{"env": int(rows[k, 2 * _M]), "l": int(rows[k, 2 * _M + 1]), "step": int(rows[k, 2 * _M + 2]) & 0xffffffff,
                 **{name: float(vals[k, m]) for m, name in enumerate(METRICS)}} for k in range(len(rows))]

    def summary(self):
        """{"eval/<metric>": mean over the ring (the last min(episodes, window) episodes; NaN when there are none)} and "eval/mean_ep_length" likewise; over the
        block's life "eval/episodes", "eval/nonfinite", "eval/mean_ep_length_all" and "eval/<metric>_all", "eval/<metric>_std_all" -- mean and population
        standard deviation from total / total_sq over the episodes whose metrics are all finite."""
        head, rows = self._host()
        nan = float("nan")
        live = len(rows) > 0
        vals = np.ascontiguousarray(rows[:, :2 * _M]).view(np.float64).reshape(len(rows), _M)
        out = {f"eval/{name}": float(np.mean(vals[:, m])) if live else nan for m, name in enumerate(METRICS)}
        out["eval/mean_ep_length"] = float(np.mean(rows[:, 2 * _M + 1].astype(np.float64))) if live else nan
        out["eval/episodes"], out["eval/nonfinite"] = head["episodes"], head["nonfinite"]
        out["eval/mean_ep_length_all"] = head["length_sum"] / head["episodes"] if head["episodes"] else nan
        good = head["episodes"] - head["nonfinite"]
        for m, name in enumerate(METRICS):
            mean = head["total"][m] / good if good else nan
            out[f"eval/{name}_all"] = float(mean)
            out[f"eval/{name}_std_all"] = float(np.sqrt(max(head["total_sq"][m] / good - mean * mean, 0.0))) if good else nan
        return out

    def episode_count(self):
        """episodes counted so far (an 8-byte device-to-host copy; waits for the stream)"""
        return int(self.block[:2].cpu().numpy().view(np.int64)[0])


class EpisodeRecorder:
    """Whole episodes of the environments `env_indices` (distinct) of `env`, on the device: the first `episodes` episodes of each after attaching (or reset()),
    every step's [53] record at its row, rows an episode never reached left zero -- what episode_log.EpisodeLogger buffers for one environment with a host
    synchronisation per step.  Turns the step log on.  record() is called by env.step_tensor while the object is attached (env.attach_observer)."""

    def __init__(self, env, env_indices, episodes=1):
        idx = [int(i) for i in env_indices]
        if not idx or len(set(idx)) != len(idx) or min(idx) < 0 or max(idx) >= env.num_envs:
            raise ValueError(f"env_indices must be distinct indices in [0, {env.num_envs}), got {list(env_indices)!r}")
        self.env, self.indices, self.n_episodes = env, idx, int(episodes)
        self.horizon, self.action_dim = int(env.horizon), int(env.action_dim)
        self.lib = _lib.load()
        self.block = torch.zeros(_lib.record_words(len(idx), self.n_episodes, self.horizon), dtype=torch.int32, device=env.device)      # all zero: empty
        self._index = torch.tensor(idx, dtype=torch.int32, device=env.device)
        if env.step_log is None:
            env.enable_step_log(True)

    def record(self):
        """one usim_record_step on the env's stream.  Capture-safe."""
        env = self.env
        _lib.check(self.lib, self.lib.usim_record_step(C.byref(env._io), env.num_envs, self.horizon, self._index.data_ptr(), len(self.indices), self.n_episodes,
                                                       self.block.data_ptr(), env._stream()))

    def reset(self):
        """an empty record again: in-place zero_(), capturable"""
        self.block.zero_()

    def complete(self):
        """True when every tracked environment has finished `episodes` episodes (one small device-to-host copy; waits for the stream)"""
        return bool((self.block[:len(self.indices)].cpu().numpy() >= self.n_episodes).all())

    @staticmethod
    def episodes_from_block(words, m, episodes, horizon):
        """the block of usim_record_step as 32-bit words (any 4-byte dtype) -> (filled int32 [m], lengths int32 [m][episodes], rows float32
        [m][episodes][horizon][53]); plain numpy"""
        w = np.ascontiguousarray(words).view(np.int32).ravel()
        m, episodes, horizon = int(m), int(episodes), int(horizon)
        if w.size != _lib.record_words(m, episodes, horizon):
            raise ValueError(f"a record block of {m} x {episodes} episodes of {horizon} rows has {_lib.record_words(m, episodes, horizon)} words, got {w.size}")
        head = (m + m * episodes + 3) // 4 * 4
        return w[:m].copy(), w[m:m + m * episodes].reshape(m, episodes).copy(), w[head:].view(np.float32).reshape(m, episodes, horizon, _lib.LOG_WIDTH).copy()

    def episodes(self):
        """the finished episodes, tracked environment by tracked environment, each in the order they were played:
        [{"env": environment index, "index": number of the episode among that environment's, from 0, "length": steps, "rows": float32 [horizon, 53]}]
        (ONE device-to-host copy of the block)"""
        filled, lengths, rows = self.episodes_from_block(self.block.cpu().numpy(), len(self.indices), self.n_episodes, self.horizon)
        return [{"env": e, "index": k, "length": int(lengths[r, k]), "rows": rows[r, k]}
                for r, e in enumerate(self.indices) for k in range(min(int(filled[r]), self.n_episodes))]

    def write_csv(self, root=".", episodes=None):
        """the reference's files (ultrasound.py:584-612, 890-910) for every finished episode -- or for `episodes`, a list as episodes() returns --, in that order:
        <root>/simulation_data, reward_data, policy_data/<stem>_<idx>.csv, idx the first free integer >= 1, rows as float64 like EpisodeLogger's.  -> the paths"""
        written = []
        for ep in self.episodes() if episodes is None else episodes:
            rows = np.asarray(ep["rows"], dtype=np.float32).astype(np.float64)
            for folder, stem, col, width in _CHANNELS:
                w = self.action_dim if width is None else width
                data = rows[:, col:col + w]
                written.append(_save(data[:, 0] if w == 1 else data, os.path.join(root, folder), stem))
        return written


def evaluate_episodes(env, policy, vecnorm, n_eval_episodes=10, deterministic=True, seed=0, check_every=50, record_envs=None, record_episodes=1):
    """monitor.evaluate_policy's loop with the error metrics in it: the same reset, the same eager loop of FusedRollout.act(training=0: the statistics of
    `vecnorm` are frozen) and env.step_tensor, with a fresh DeviceMonitor, a fresh DeviceEpisodeMetrics (window = n_eval_episodes, the same targets, counts of
    its own) and, with record_envs, an EpisodeRecorder(env, record_envs, record_episodes) attached.  Row k of the metrics ring and row k of the monitor ring
    must name the same (environment, launch): RuntimeError if they do not.  A monitor and observers attached before are put back afterwards, untouched, and
    a step log that was off is turned off again.
    -> {"returns": float64 [n_eval], "lengths": int64 [n_eval], "metrics": {name: float64 [n_eval]} -- one entry per episode in SB3's order --,
        "mean": np.mean(returns), "std": np.std(returns), "recorder": the EpisodeRecorder or None}"""
    n_eval = int(n_eval_episodes)
    if n_eval < 1:
        raise ValueError("n_eval_episodes must be at least 1")
    targets = eval_targets(n_eval, env.num_envs)
    mon = DeviceMonitor(env, window=n_eval, targets=targets)
    had_log = env.step_log is not None
    met = DeviceEpisodeMetrics(env, window=n_eval, targets=targets)
    rec = None if record_envs is None else EpisodeRecorder(env, record_envs, record_episodes)
    try:
        eps = _evaluation_run(env, policy, vecnorm, mon, (met,) if rec is None else (met, rec), n_eval, targets, deterministic, seed, check_every,
                              "evaluate_episodes")
        rows = met._host()[1]                                         # arrays, not episodes(): at 4096 episodes the dicts would cost more than the run's launches
    finally:
        if not had_log:                                               # the step kernels go back to writing no record, as before the call
            env.enable_step_log(False)
    named = np.array([(e["env"], e["step"]) for e in eps], dtype=np.int64).reshape(len(eps), 2)
    if len(rows) != len(eps) or not np.array_equal(named, np.stack([rows[:, 2 * _M], rows[:, 2 * _M + 2]], axis=1).astype(np.int64) & 0xffffffff):
        raise RuntimeError("evaluate_episodes: the metrics ring and the monitor ring do not name the same (environment, launch) row by row")
    vals = np.ascontiguousarray(rows[:, :2 * _M]).view(np.float64).reshape(len(rows), _M)
    returns = np.array([e["r"] for e in eps], dtype=np.float64)
    return {"returns": returns, "lengths": np.array([e["l"] for e in eps], dtype=np.int64),
            "metrics": {name: vals[:, m].copy() for m, name in enumerate(METRICS)},
            "mean": float(np.mean(returns)), "std": float(np.std(returns)), "recorder": rec}
