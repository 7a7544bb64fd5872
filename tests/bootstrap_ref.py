"""Plain float64 restatement of usim_policy_bootstrap (include/usim.h; csrc/usim_policy.hip) -- SB3's time-limit bootstrap
`rewards[idx] += gamma * V(terminal_observation)` where an episode ended at the horizon -- on top of policy_ref.forward / forward_bounds: numpy
only, no torch and no library calls.

    truncated_i = done_i != 0 and ep_length_i >= horizon
    nobs_i      = float32(clip((term_obs_i - obs_mean) / sqrt(obs_var + epsilon), +-clip_obs))     (the float32 word the value network is given)
    out_i       = rew_i + gamma V(nobs_i)   where truncated, rew_i otherwise

The bound of a float32 evaluation is the one policy_ref.forward_bounds gives for the value output on nobs_i with the error units of
tests/test_gpu_policy_kernels.py (UNITS below: the same numbers, for the same operations -- float32 fmaf chains and the exp / rcp tanh), carried
through the last multiply-add: with bV the bound of V and ref = rew + gamma V,
    fused (one fmaf, one rounding)       gamma bV + 2^-24 (|ref| + gamma bV)
    separate product and sum (torch)     ... + 2^-24 gamma (|V| + bV)                               (the product's own rounding)
gamma is the float32 word the kernel receives, taken as exact."""
import numpy as np

import policy_ref as R

U24 = 2.0**-24
UNITS = dict(mm1=1.5e-7 + U24, tanh=2.0**-22, mm2=3 * 2.0**-22 + 1.5e-7 + U24, floor=2.0**-25, head=1.5e-7 + U24)      # tests/test_gpu_policy_kernels.py


PATTERNS = ("none", "all", "last", "alternating", "early", "stale", "mixed")
HORIZON = 37


def orthogonal_params(seed, adim=6):
    """SB3's initialisation (orthogonal rows / columns; gain sqrt 2 for the hidden layers, 0.01 for the action head, 1 for the value head; zero biases)"""
    rng = np.random.default_rng(seed)

    def orth(rows, cols, gain):
        a = rng.normal(size=(max(rows, cols), min(rows, cols)))
        q, r = np.linalg.qr(a)
        q = q * np.sign(np.diag(r))
        return (gain * (q if rows >= cols else q.T)).astype(np.float32)

    p = {}
    for net in ("pi", "vf"):
        p[net + "_w1"], p[net + "_b1"] = orth(256, 19, 2**0.5), np.zeros(256, np.float32)
        p[net + "_w2"], p[net + "_b2"] = orth(128, 256, 2**0.5), np.zeros(128, np.float32)
    p["act_w"], p["act_b"] = orth(adim, 128, 0.01), np.zeros(adim, np.float32)
    p["val_w"], p["val_b"] = orth(1, 128, 1.0), np.zeros(1, np.float32)
    p["log_std"] = np.zeros(adim, np.float32)
    return p


def crafted_stats(rng):
    """observation statistics with variances from 1e-6 to 1e2 (one decade step per two or three channels, shuffled) and means of a few deviations"""
    var = rng.permutation(10.0 ** np.linspace(-6.0, 2.0, 19))
    return rng.normal(size=19) * 3.0 * np.sqrt(var), var


def crafted_obs(rng, n, mean, var):
    """terminal observations whose normalised components spread over +-2 clip_obs: a tenth of them is clipped, on both sides"""
    return (mean + np.sqrt(var + 1e-8) * rng.normal(size=(n, 19)) * 6.0).astype(np.float32)


def crafted_flags(rng, n, pattern, horizon=HORIZON):
    """-> (done uint8 [n], ep_length int32 [n]) of one of PATTERNS: which environments are truncated, and what the others look like --
    not done with a short stale length, done before the horizon (early termination), not done with a stale length at or past the horizon"""
    i = np.arange(n)
    kind = {"none": np.zeros(n, int), "all": np.ones(n, int), "last": (i == n - 1).astype(int), "alternating": (i % 2 == 0).astype(int),
            "early": np.full(n, 2), "stale": np.full(n, 3), "mixed": rng.integers(0, 4, n)}[pattern]
    done = np.where((kind == 1) | (kind == 2), rng.choice(np.array([1, 2, 255]), n), 0).astype(np.uint8)
    ep = np.select([kind == 1, kind == 2, kind == 3], [horizon + (i % 3 == 0), horizon - 1, horizon + 5 * (i % 2)], rng.integers(0, horizon, n)).astype(np.int32)
    return done, ep


def poison(term_obs, tr):
    """a copy with NaN / +inf / -inf in the rows that are not truncated"""
    out = np.array(term_obs, dtype=np.float32)
    rows = np.flatnonzero(~tr)
    out[rows] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[(rows[:, None] + np.arange(19)[None, :]) % 3]
    return out


def truncated(done, ep_length, horizon):
    return (np.asarray(done) != 0) & (np.asarray(ep_length) >= int(horizon))


def normalize(term_obs, obs_mean, obs_var, epsilon=1e-8, clip_obs=10.0):
    """the normalised terminal observation as the value network receives it: float64 arithmetic, one rounding to float32"""
    x = (np.asarray(term_obs, dtype=np.float64) - np.asarray(obs_mean, dtype=np.float64)) / np.sqrt(np.asarray(obs_var, dtype=np.float64) + epsilon)
    return np.clip(x, -clip_obs, clip_obs).astype(np.float32)


def bootstrap(p, obs_mean, obs_var, term_obs, done, ep_length, horizon, gamma, rew, epsilon=1e-8, clip_obs=10.0, fused=True):
    """-> (out [n] float64, bound [n] float64 (0 where not truncated), truncated [n] bool, value [n] float64 (0 where not truncated), value bound [n]).
    Rows that are not truncated are never looked at: they may hold NaN or inf."""
    rew = np.asarray(rew, dtype=np.float64)
    tr = truncated(done, ep_length, horizon)
    out, bound, value, bvalue = rew.copy(), np.zeros(rew.shape), np.zeros(rew.shape), np.zeros(rew.shape)
    if tr.any():
        nobs = normalize(np.asarray(term_obs)[tr], obs_mean, obs_var, epsilon, clip_obs)
        _, v = R.forward(p, nobs)
        _, bv = R.forward_bounds(p, nobs, UNITS)
        g = float(gamma)
        ref = rew[tr] + g * v
        b = g * bv + U24 * (np.abs(ref) + g * bv)
        if not fused:
            b = b + U24 * g * (np.abs(v) + bv)
        out[tr], bound[tr], value[tr], bvalue[tr] = ref, b, v, bv
    return out, bound, tr, value, bvalue
