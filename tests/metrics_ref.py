"""Plain numpy restatement, in float64, of what usim_metrics_step and usim_record_step (include/usim.h; csrc/usim_metrics.hip) do to their blocks: the thirteen
summands of error_metrics.step_terms, the per-environment accumulators, evaluate_policy's target gating, the ring in SB3's append order with its wrap, the
ordered life-time sums, `nonfinite`, and the recorder's slots.  Both classes produce the block word for word (`block()`), so a test compares integers exactly and
float64 words to a relative bound.  No GPU, no library."""
import numpy as np

M = 13
HEADER, ROW, LOG, TIME = 64, 32, 53, 40
NAMES = ("x_pos_mse", "y_pos_mse", "force_mse", "mean_force_mse", "der_force_mse", "velocity_mse", "mean_velocity_mse", "quat_diff_mean",
         "pos_reward_mean", "ori_reward_mean", "force_reward_mean", "der_force_reward_mean", "vel_reward_mean")


def step_terms(log):
    """[n, 53] float32 record of one step -> [n, 13] float64 summands (src/utils/error.py:33-156 row by row)"""
    x = np.asarray(log, dtype=np.float32).astype(np.float64)
    sq = lambda a, b: (a - b) ** 2
    speed = np.sqrt(x[:, 6] * x[:, 6] + x[:, 7] * x[:, 7] + x[:, 8] * x[:, 8])
    return np.stack([sq(x[:, 0], x[:, 3]), sq(x[:, 1], x[:, 4]), sq(x[:, 20], x[:, 21]), sq(x[:, 22], x[:, 21]), sq(x[:, 23], x[:, 24]),
                     sq(speed, x[:, 9]), sq(x[:, 10], x[:, 9]), x[:, 19], x[:, 41], x[:, 42], x[:, 44], x[:, 45], x[:, 43]], axis=1)


def row_time(time_word, horizon):
    """t of a row: round-half-even of float64(time) * horizon / 100 (episode_log.EpisodeLogger.after_step); a float (NaN stays NaN)"""
    return float(np.rint(np.float64(np.float32(time_word)) * horizon / 100.0))


def length_of(td):
    """the episode length a done row with time td stands for: t + 1; 0 where td is no step number"""
    return int(td) + 1 if -1.0 <= td < 2147483647.0 else 0


class MetricsRef:
    def __init__(self, n, window, horizon, targets=None):
        self.n, self.window, self.horizon = int(n), int(window), int(horizon)
        self.targets = None if targets is None else [int(t) for t in targets]
        self.counts = [0] * self.n
        self.acc = np.zeros((self.n, M), dtype=np.float64)
        self.ring = np.zeros((self.window, ROW), dtype=np.int32)       # physical rows: episode e lives in row e mod window
        self.episodes = self.launches = self.length_sum = self.nonfinite = 0
        self.total, self.total_sq = np.zeros(M, dtype=np.float64), np.zeros(M, dtype=np.float64)
        self.history = []                                              # every counted episode over the block's life: (metrics [13], env, length, launch)

    def step(self, log, done):
        """one call: log [n, 53] float32, done [n] (any non-zero byte) -> the number of episodes counted"""
        log, done = np.asarray(log, dtype=np.float32), np.asarray(done)
        with np.errstate(invalid="ignore", over="ignore"):
            self.acc += step_terms(log)
        c = 0
        for i in range(self.n):
            if done[i] == 0:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                fin = self.acc[i] / float(self.horizon)
            self.acc[i] = 0.0                                          # counted or not
            if self.targets is not None:
                if self.counts[i] >= self.targets[i]:
                    continue
                self.counts[i] += 1
            length = length_of(row_time(log[i, TIME], self.horizon))
            row = self.ring[self.episodes % self.window]
            row[:2 * M] = fin.view(np.int32)
            row[2 * M:] = (i, length, np.array([self.launches & 0xffffffff], dtype=np.uint32).view(np.int32)[0], 0, 0, 0)
            self.history.append((fin.copy(), i, length, self.launches))
            self.episodes += 1
            self.length_sum += length
            if np.isfinite(fin).all():
                self.total += fin                                      # one episode after the other, ascending environment index
                self.total_sq += fin * fin
            else:
                self.nonfinite += 1
            c += 1
        self.launches += 1
        return c

    def live(self):
        """the live episodes, oldest first (what DeviceEpisodeMetrics.episodes() lists)"""
        return self.history[-self.window:]

    def block(self):
        """the whole block as int32 words"""
        w = np.zeros(HEADER + ROW * self.window + 2 * M * self.n, dtype=np.int32)
        w[:8] = np.array([self.episodes, self.launches, self.length_sum, self.nonfinite], dtype=np.int64).view(np.int32)
        w[8:8 + 2 * M] = self.total.view(np.int32)
        w[8 + 2 * M:8 + 4 * M] = self.total_sq.view(np.int32)
        w[HEADER:HEADER + ROW * self.window] = self.ring.ravel()
        w[HEADER + ROW * self.window:] = self.acc.ravel().view(np.int32)
        return w


def split_block(words, n, window):
    """int32 words of a metrics block -> (integer words, float64 words): every word of the block is in exactly one of the two"""
    w = np.ascontiguousarray(words).view(np.int32).ravel()
    assert w.size == HEADER + ROW * window + 2 * M * n
    ring = w[HEADER:HEADER + ROW * window].reshape(window, ROW)
    ints = np.concatenate([w[:8], w[8 + 4 * M:HEADER], ring[:, 2 * M:].ravel()])
    floats = np.concatenate([w[8:8 + 4 * M], ring[:, :2 * M].ravel(), w[HEADER + ROW * window:]]).view(np.float64)
    return ints, floats


def compare_blocks(got, want, n, window, rtol=1e-12):
    """every integer word exact; every float64 word within rtol relative (a NaN where the reference has one, an exact zero where it has zero)
    -> the largest relative difference seen"""
    gi, gf = split_block(got, n, window)
    wi, wf = split_block(want, n, window)
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(np.isnan(gf), np.isnan(wf))
    ok = np.isfinite(wf)
    np.testing.assert_array_equal(gf[~ok & ~np.isnan(wf)], wf[~ok & ~np.isnan(wf)])          # infinities
    err = np.abs(gf[ok] - wf[ok])
    bound = rtol * np.abs(wf[ok])
    assert (err <= bound).all(), f"float64 words differ by up to {np.max(err / np.maximum(np.abs(wf[ok]), 1e-300)):.3e} relative (bound {rtol:.1e})"
    nz = wf[ok] != 0
    return float(np.max(err[nz] / np.abs(wf[ok][nz]))) if nz.any() else 0.0


class RecorderRef:
    def __init__(self, n, indices, episodes, horizon):
        self.n, self.indices, self.n_episodes, self.horizon = int(n), [int(i) for i in indices], int(episodes), int(horizon)
        m = len(self.indices)
        self.filled = np.zeros(m, dtype=np.int32)
        self.lengths = np.zeros((m, self.n_episodes), dtype=np.int32)
        self.rows = np.zeros((m, self.n_episodes, self.horizon, LOG), dtype=np.float32)

    def step(self, log, done):
        log, done = np.asarray(log, dtype=np.float32), np.asarray(done)
        for r, e in enumerate(self.indices):
            f = int(self.filled[r])
            if not 0 <= e < self.n or f >= self.n_episodes:
                continue
            td = row_time(log[e, TIME], self.horizon)
            if 0.0 <= td < self.horizon:
                self.rows[r, f, int(td)].view(np.uint32)[:] = log[e].view(np.uint32)          # as its bits
            if done[e] != 0:
                self.lengths[r, f] = length_of(td)
                self.filled[r] = f + 1

    def block(self):
        m = len(self.indices)
        head = (m + m * self.n_episodes + 3) // 4 * 4
        w = np.zeros(head + self.rows.size, dtype=np.int32)
        w[:m] = self.filled
        w[m:m + m * self.n_episodes] = self.lengths.ravel()
        w[head:] = self.rows.ravel().view(np.int32)
        return w


class FakeEnv:
    """the attributes error_metrics.DeviceErrorMetrics / episode_log.EpisodeLogger use of an env (as tests/test_error_metrics.py's stand-in), on the CPU"""
    def __init__(self, n, horizon, adim=6):
        import torch
        self.num_envs, self.horizon, self.action_dim, self.device = n, horizon, adim, torch.device("cpu")
        self.step_log = torch.zeros(n, LOG)

    def enable_step_log(self, enable=True):
        return self.step_log


def synthetic_episodes(n, horizon, steps, seed, p_done=0.15, signed=True):
    """`steps` x (log [n, 53] float32, done [n] uint8): random channels, the time channel the environment's own step counter ((timestep - 1) / horizon * 100 in
    float32), an episode ending at random or at the horizon.  Goal channels are constants as in the simulator."""
    g = np.random.default_rng(seed)
    t = np.zeros(n, dtype=np.int64)
    out = []
    for _ in range(steps):
        log = g.standard_normal((n, LOG)).astype(np.float32)
        if not signed:
            log = np.abs(log)
        log[:, TIME] = (t.astype(np.float64) / horizon * 100.0).astype(np.float32)
        log[:, 9], log[:, 21], log[:, 24] = 0.04, 5.0, 0.0
        t += 1
        done = ((t >= horizon) | (g.random(n) < p_done)).astype(np.uint8)
        t[done != 0] = 0
        out.append((log, done))
    return out
