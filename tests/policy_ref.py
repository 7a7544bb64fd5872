"""Plain float64 restatement of the policy side of a rollout step (csrc/usim_policy.hip; policy.DeviceVecNormalize, MlpActorCritic,
DeviceRolloutBuffer): numpy only, no torch and no library calls, so that it shares no rounding with what it checks.

- philox4x32 / policy_noise: Philox4x32-10 on arrays and the exploration noise of usim_policy_step (Box-Muller in float64 on the same words)
- RunningMeanStd / VecNormalize: stable-baselines3's statistics, two-pass batch moments (population variance) + update_from_moments
- forward / forward_bounds: both MlpPolicy networks in float64, and an absolute-value companion pass (|W| |x| through every layer) that turns
  per-operation error units into a bound per output
- log_prob / clip_action / gae: DiagGaussianDistribution.log_prob, the clip to the action box, SB3's GAE recursion"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)
NOISE_TAG = 0x504F4C59                          # fourth counter word of the policy noise ("POLY")
PARAM_NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "act_w", "act_b", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "val_w", "val_b", "log_std")
_SB3_NAMES = {"pi_w1": "mlp_extractor.policy_net.0.weight", "pi_b1": "mlp_extractor.policy_net.0.bias", "pi_w2": "mlp_extractor.policy_net.2.weight",
              "pi_b2": "mlp_extractor.policy_net.2.bias", "act_w": "action_net.weight", "act_b": "action_net.bias",
              "vf_w1": "mlp_extractor.value_net.0.weight", "vf_b1": "mlp_extractor.value_net.0.bias", "vf_w2": "mlp_extractor.value_net.2.weight",
              "vf_b2": "mlp_extractor.value_net.2.bias", "val_w": "value_net.weight", "val_b": "value_net.bias", "log_std": "log_std"}


def params_from_sb3(sd):
    """{PARAM_NAMES: array} from a state dict under SB3's layer names (tests/golden/*_policy.npz)"""
    return {k: np.asarray(sd[v]) for k, v in _SB3_NAMES.items()}


# ---- Philox4x32-10 (Salmon et al. 2011) ----
def philox4x32(ctr, key):
    """ctr = (c0, c1, c2, c3), key = (k0, k1): integer arrays (broadcast together) -> uint32 array [4, ...]"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & M32 for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2      # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3)).astype(np.uint32)


def policy_noise(seed, n, adim, counter, base=0, env_offset=0):
    """N(0, 1) of usim_policy_step for environments 0 .. n-1: counter (env_offset + env, (counter + base) mod 2^32, component >> 1, NOISE_TAG), key
    (seed low, seed high); u1 = ((a >> 8) + 1) / 2^24 in (0, 1], u2 = (b >> 8) / 2^24; radius sqrt(-2 ln u1), cosine for even components, sine for
    odd ones.  -> (noise, radius), float64 [n, adim]"""
    seed = int(seed)
    env = (int(env_offset) + np.arange(n, dtype=np.int64)) & 0xFFFFFFFF
    comp = np.arange(adim)
    w = philox4x32((env[:, None], (int(counter) + int(base)) % 2**32, comp[None, :] >> 1, NOISE_TAG), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w[0] >> 8).astype(np.float64) + 1.0) / 2.0**24
    u2 = (w[1] >> 8).astype(np.float64) / 2.0**24
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.where(comp % 2 == 0, rad * np.cos(ang), rad * np.sin(ang)), rad


# ---- VecNormalize ----
class RunningMeanStd:
    def __init__(self, shape=(), count=1e-4):
        self.mean, self.var, self.count = np.zeros(shape), np.ones(shape), float(count)

    def update(self, x):
        x = np.asarray(x, dtype=np.float64)
        bm = x.mean(0)
        self.update_from_moments(bm, ((x - bm) ** 2).mean(0), x.shape[0])

    def update_from_moments(self, bm, bv, bn):
        delta, tot = bm - self.mean, self.count + bn
        m2 = self.var * self.count + bv * bn + delta * delta * self.count * bn / tot
        self.mean, self.var, self.count = self.mean + delta * bn / tot, m2 / tot, tot


class VecNormalize:
    """the statistics side of stable_baselines3 VecNormalize, as policy.DeviceVecNormalize implements it"""

    def __init__(self, num_envs, obs_dim=19, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8, training=True, norm_reward=True):
        self.obs_rms, self.ret_rms = RunningMeanStd((obs_dim,)), RunningMeanStd(())
        self.returns = np.zeros(num_envs)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.training, self.norm_reward = training, norm_reward

    def scale_obs(self, obs):
        """(obs - mean) / sqrt(var + eps), clipped; float64 (the statistics are not updated)"""
        x = (np.asarray(obs, dtype=np.float64) - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon)
        return np.clip(x, -self.clip_obs, self.clip_obs)

    def normalize_obs(self, obs):
        if self.training:
            self.obs_rms.update(obs)
        return self.scale_obs(obs)

    def scale_reward(self, rew):
        return np.clip(np.asarray(rew, dtype=np.float64) / np.sqrt(self.ret_rms.var + self.epsilon), -self.clip_reward, self.clip_reward)

    def normalize_reward(self, rew, done):
        rew = np.asarray(rew, dtype=np.float64)
        if self.training:
            self.returns = self.returns * self.gamma + rew
            self.ret_rms.update(self.returns)
            self.returns = np.where(np.asarray(done) != 0, 0.0, self.returns)
        return self.scale_reward(rew) if self.norm_reward else rew


# ---- the two networks ----
def _layers(p, net):
    f = lambda k: np.asarray(p[k], dtype=np.float64)
    return [(f(net + "_w1"), f(net + "_b1")), (f(net + "_w2"), f(net + "_b2"))], (f("act_w"), f("act_b")) if net == "pi" else (f("val_w"), f("val_b"))


def forward(p, x):
    """-> (mean [n, A], value [n]) of both networks on observations x [n, 19], float64 throughout"""
    out = []
    for net in ("pi", "vf"):
        (l1, l2), (wh, bh) = _layers(p, net)
        h = np.asarray(x, dtype=np.float64)
        for w, b in (l1, l2):
            h = np.tanh(h @ w.T + b)
        out.append(h @ wh.T + bh)
    return out[0], out[1][:, 0]


def _tanh_bound(z, ez, et):
    e = np.exp(-2.0 * np.maximum(np.abs(z) - ez, 0.0))              # sech^2 u = 4 e^-2u / (1 + e^-2u)^2
    return ez * 4.0 * e / (1.0 + e) ** 2 + et


def forward_bounds(p, x, u):
    """Error bound per output of a forward pass that rounds as the unit dictionary `u` says, from the absolute-value companion pass:
       layer 1   e_z1 = u["mm1"] (|W1| |x| + |b1|)                                             (float32 products + bias)
       tanh      e_h = e_z sech^2(max(|z| - e_z, 0)) + u["tanh"]                                  (the largest slope within the error interval; absolute error
                                                                                                   of the approximation)
       layer 2   e_z2 = |W2| e_h1 + u["mm2"] (|W2| |h1| + |b2|) + u["floor"] (sum_k |W2| + sum_k |h1|)   (split words: relative part, absolute floor)
       heads     e = |Wh| e_h2 + u["head"] (|Wh| |h2| + |bh|)
    x is taken as exact (the caller passes the observation the kernel normalised).  -> (bound of mean [n, A], bound of value [n])"""
    out = []
    x = np.asarray(x, dtype=np.float64)
    for net in ("pi", "vf"):
        ((w1, b1), (w2, b2)), (wh, bh) = _layers(p, net)
        z1 = x @ w1.T + b1
        h1 = np.tanh(z1)
        e1 = _tanh_bound(z1, u["mm1"] * (np.abs(x) @ np.abs(w1).T + np.abs(b1)), u["tanh"])
        z2 = h1 @ w2.T + b2
        h2 = np.tanh(z2)
        e2 = _tanh_bound(z2, e1 @ np.abs(w2).T + u["mm2"] * (np.abs(h1) @ np.abs(w2).T + np.abs(b2))
                         + u["floor"] * (np.abs(w2).sum(1)[None, :] + np.abs(h1).sum(1, keepdims=True)), u["tanh"])
        out.append(e2 @ np.abs(wh).T + u["head"] * (np.abs(h2) @ np.abs(wh).T + np.abs(bh)))
    return out[0], out[1][:, 0]


# ---- sampling, box, GAE ----
def log_prob(noise, log_std):
    """DiagGaussianDistribution.log_prob of mean + exp(log_std) noise: sum(-noise^2 / 2 - log_std - ln(2 pi) / 2)"""
    return (-0.5 * np.asarray(noise, dtype=np.float64) ** 2 - np.asarray(log_std, dtype=np.float64) - LOG_SQRT_2PI).sum(-1)


def clip_action(a, low, high):
    return np.minimum(np.maximum(np.asarray(a, dtype=np.float64), np.asarray(low, dtype=np.float64)), np.asarray(high, dtype=np.float64))


def gae(rewards, values, starts, last_values, last_done, gamma, lam):
    """RolloutBuffer.compute_returns_and_advantage in float64 on [T, n] arrays -> (advantages, returns, magnitude): `magnitude` is the
    absolute-value companion of the recursion (|r| + gamma |v'| + |v| + gamma lam |...|), the scale of its rounding errors"""
    r, v, s = (np.asarray(a, dtype=np.float64) for a in (rewards, values, starts))
    T = r.shape[0]
    adv, mag = np.zeros_like(r), np.zeros_like(r)
    last, last_mag = np.zeros(r.shape[1]), np.zeros(r.shape[1])
    for t in reversed(range(T)):
        if t == T - 1:
            nnt, nv = 1.0 - (np.asarray(last_done) != 0), np.asarray(last_values, dtype=np.float64)
        else:
            nnt, nv = 1.0 - s[t + 1], v[t + 1]
        last = r[t] + gamma * nv * nnt - v[t] + gamma * lam * nnt * last
        last_mag = np.abs(r[t]) + gamma * np.abs(nv) * nnt + np.abs(v[t]) + gamma * lam * nnt * last_mag
        adv[t], mag[t] = last, last_mag
    return adv, adv + v, mag
