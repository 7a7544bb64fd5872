"""Replay of the reference's trained stable-baselines3 PPO policies on the batched simulator, entirely on the GPU
(SURVEY.md section 8f rank 1).

The reference evaluates a checkpoint with `VecNormalize.load(...)`, `PPO.load(...)`, `model.predict(obs)` (src/rl.py:171-192).
The shipped artefacts are `trained_rl_models/<name>.zip` (SB3 1.1.0a5: json `data` + `policy.pth` state dict of an
ActorCriticPolicy with net_arch [dict(pi=[256,128], vf=[256,128])], tanh activations) and `vec_normalize_<name>.pkl`
(obs_rms / ret_rms, clip 10, gamma 0.99, eps 1e-8).  Neither SB3 nor gym is imported: the zip is read with zipfile +
torch.load(weights_only=True), the pickle with a restricted unpickler that maps the four SB3 / gym classes to local stand-ins
(sys.modules is never touched).  save_sb3_zip / save_vecnormalize_pkl write the same formats (the model.save / env.save step at the
end of src/rl.py's training branch, :157-158)."""
import ctypes as C
import functools
import io
import json
import pickle
import zipfile

import numpy as np
import torch

from . import _lib

# the four classes a VecNormalize pickle of stable-baselines3 refers to (besides numpy's array reconstructors)
_SB3_CLASSES = (("gym.spaces.box", "Box"), ("gym.spaces.space", "Space"),
                ("stable_baselines3.common.running_mean_std", "RunningMeanStd"),
                ("stable_baselines3.common.vec_env.vec_normalize", "VecNormalize"))


def _make_stub(modname, clsname):
    # local stand-in for one SB3 / gym class: carries the original (module, name) for the writer, never registered in sys.modules
    return type(clsname, (), {"__module__": __name__, "_pickle_global": (modname, clsname),
                              "__setstate__": lambda self, st: self.__dict__.update(st)})


_STUBS = {key: _make_stub(*key) for key in _SB3_CLASSES}
# numpy's array / dtype / scalar reconstructors (both spellings of the private multiarray module)
_NUMPY_GLOBALS = {("numpy", "dtype"), ("numpy", "ndarray"), ("numpy.core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"),
                  ("numpy._core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "scalar")}


class _CheckpointUnpickler(pickle.Unpickler):
    """Resolves only the four SB3 / gym classes (to local stubs) and numpy's array reconstructors; everything else is refused, and
    sys.modules is left alone (a later `import stable_baselines3` in the same process finds the real package)."""

    def find_class(self, module, name):
        if (module, name) in _STUBS:
            return _STUBS[(module, name)]
        if (module, name) in _NUMPY_GLOBALS:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refusing to load {module}.{name} from a VecNormalize checkpoint")


class _CheckpointPickler(pickle._Pickler):
    """Writes the stub classes under the (module, name) of the SB3 / gym class they stand for, so that the file loads with
    VecNormalize.load on a machine that has stable-baselines3."""

    def save_global(self, obj, name=None):
        target = getattr(obj, "_pickle_global", None) if isinstance(obj, type) else None
        if target is None:
            return super().save_global(obj, name)
        self.save(target[0]); self.save(target[1])
        self.write(pickle.STACK_GLOBAL)
        self.memoize(obj)

    dispatch = dict(pickle._Pickler.dispatch)
    dispatch[type] = save_global


def load_sb3_zip(path):
    """-> (state_dict of CPU tensors, data dict) of a stable-baselines3 PPO checkpoint"""
    with zipfile.ZipFile(path) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        data = json.loads(z.read("data"))
    return sd, data


def adam_state_dict(sd, step=0, lr=3e-4, eps=1e-5):
    """`policy.optimizer.pth` of an SB3 PPO checkpoint: the state dict of torch.optim.Adam(lr 3e-4, eps 1e-5: SB3's PPO defaults, as stored in
    the reference zips) over the policy parameters in state-dict order.  step == 0 writes a fresh optimizer (empty state)."""
    names = list(sd)
    state = {}
    if step > 0:
        state = {i: {"step": int(step), "exp_avg": torch.zeros_like(sd[k]), "exp_avg_sq": torch.zeros_like(sd[k])} for i, k in enumerate(names)}
    return {"state": state, "param_groups": [{"lr": lr, "betas": (0.9, 0.999), "eps": eps, "weight_decay": 0, "amsgrad": False,
                                               "params": list(range(len(names)))}]}


def save_sb3_zip(path, policy, data=None, optimizer_state=None):
    """Write `policy` (MlpActorCritic) in the on-disk layout of `PPO.save` (src/rl.py:157) -- the five members of the reference zips
    (src/trained_rl_models/*.zip): data json, pytorch_variables.pth, policy.pth (state dict under SB3's layer names), policy.optimizer.pth
    (Adam state dict: PPO.load -> set_parameters(exact_match=True) raises without it), _stable_baselines3_version.  `data` is the json
    dictionary of the checkpoint; pass the one returned by load_sb3_zip for a reference checkpoint (it carries the serialized policy class and
    spaces PPO.load asks for) -- without it only the numeric hyper-parameters of src/rl.py are written, enough for load_sb3_zip /
    policy.load_state_dict.  `optimizer_state`: an Adam state dict (e.g. torch.optim.Adam(policy.parameters()).state_dict() mapped to SB3's
    parameter order); default a fresh optimizer."""
    sd = policy.to_sb3_state_dict()
    if data is None:
        data = {"gamma": 0.99, "gae_lambda": 0.95, "n_steps": 2048, "n_envs": None,
                "policy_kwargs": {"activation_fn": "tanh", "net_arch": [{"pi": list(policy.pi_sizes), "vf": list(policy.vf_sizes)}]}}
    buf, var, opt = io.BytesIO(), io.BytesIO(), io.BytesIO()
    torch.save(sd, buf); torch.save({}, var); torch.save(optimizer_state if optimizer_state is not None else adam_state_dict(sd), opt)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", json.dumps(data, indent=4))
        z.writestr("pytorch_variables.pth", var.getvalue())
        z.writestr("policy.pth", buf.getvalue())
        z.writestr("policy.optimizer.pth", opt.getvalue())
        z.writestr("_stable_baselines3_version", "1.1.0a5")


def load_vecnormalize_pkl(path):
    """-> dict(obs_mean, obs_var, count, ret_mean, ret_var, ret_count, clip_obs, clip_reward, gamma, epsilon)"""
    with open(path, "rb") as f:
        v = _CheckpointUnpickler(f).load().__dict__
    o, r = v["obs_rms"].__dict__, v["ret_rms"].__dict__
    return {"obs_mean": np.asarray(o["mean"], dtype=np.float64), "obs_var": np.asarray(o["var"], dtype=np.float64), "count": float(o["count"]),
            "ret_mean": float(r["mean"]), "ret_var": float(r["var"]), "ret_count": float(r["count"]),
            "clip_obs": float(v["clip_obs"]), "clip_reward": float(v["clip_reward"]),
            "gamma": float(v["gamma"]), "epsilon": float(v["epsilon"])}


def _box(low, high, dtype=np.float32):
    b = _STUBS[("gym.spaces.box", "Box")]()
    low, high = np.asarray(low, dtype=dtype), np.asarray(high, dtype=dtype)
    b.__dict__.update(dtype=np.dtype(dtype), shape=tuple(low.shape), low=low, high=high, bounded_below=np.isfinite(low),
                      bounded_above=np.isfinite(high), _np_random=None)
    return b


def save_vecnormalize_pkl(path, stats, num_envs, action_low, action_high, training=True, norm_reward=True):
    """Write running statistics in the layout of `VecNormalize.save` (src/rl.py:158; the fields VecNormalize.__getstate__ keeps):
    loads with VecNormalize.load where stable-baselines3 is installed, and with load_vecnormalize_pkl here.  `stats` is the
    dictionary load_vecnormalize_pkl returns / DeviceVecNormalize.stats() builds."""
    def rms(mean, var, count):
        r = _STUBS[("stable_baselines3.common.running_mean_std", "RunningMeanStd")]()
        r.__dict__.update(mean=mean, var=var, count=float(count))
        return r
    n_obs = len(stats["obs_mean"])
    v = _STUBS[("stable_baselines3.common.vec_env.vec_normalize", "VecNormalize")]()
    v.__dict__.update(
        num_envs=int(num_envs), observation_space=_box(np.full(n_obs, -np.inf), np.full(n_obs, np.inf)), action_space=_box(action_low, action_high),
        obs_keys=None, obs_spaces=None,
        obs_rms=rms(np.asarray(stats["obs_mean"], dtype=np.float64), np.asarray(stats["obs_var"], dtype=np.float64), stats["count"]),
        ret_rms=rms(np.float64(stats["ret_mean"]), np.float64(stats["ret_var"]), stats.get("ret_count", stats["count"])),
        clip_obs=float(stats["clip_obs"]), clip_reward=float(stats["clip_reward"]), gamma=float(stats["gamma"]), epsilon=float(stats["epsilon"]),
        training=bool(training), norm_obs=True, norm_reward=bool(norm_reward),
        old_obs=np.zeros((int(num_envs), n_obs), dtype=np.float32), old_reward=np.zeros(int(num_envs), dtype=np.float32))
    with open(path, "wb") as f:
        _CheckpointPickler(f, protocol=4).dump(v)


class DeviceVecNormalize:
    """stable_baselines3 VecNormalize on device tensors: running mean/variance of observations and discounted returns
    (parallel-variance update of RunningMeanStd), normalisation with clipping.  `training=False` freezes the statistics
    (src/rl.py:180-181)."""

    def __init__(self, num_envs, obs_dim=19, device="cuda:0", clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8, training=True, norm_reward=True):
        dev = torch.device(device)
        # every statistic is a tensor that is updated IN PLACE (the sample counts too): a captured graph of the rollout loop (GraphedCollector)
        # then reads and writes the same addresses at every replay
        self.obs_mean = torch.zeros(obs_dim, dtype=torch.float64, device=dev)
        self.obs_var = torch.ones(obs_dim, dtype=torch.float64, device=dev)
        self._obs_count = torch.full((), 1e-4, dtype=torch.float64, device=dev)
        self.ret_mean = torch.zeros((), dtype=torch.float64, device=dev)
        self.ret_var = torch.ones((), dtype=torch.float64, device=dev)
        self._ret_count = torch.full((), 1e-4, dtype=torch.float64, device=dev)
        self.returns = torch.zeros(num_envs, dtype=torch.float64, device=dev)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.training, self.norm_reward = training, norm_reward

    obs_count = property(lambda self: float(self._obs_count))          # (a host read: synchronises)
    ret_count = property(lambda self: float(self._ret_count))

    @classmethod
    def from_stats(cls, stats, num_envs, device="cuda:0", training=False, norm_reward=False):
        self = cls(num_envs, len(stats["obs_mean"]), device, stats["clip_obs"], stats["clip_reward"], stats["gamma"], stats["epsilon"], training, norm_reward)
        self.obs_mean.copy_(torch.as_tensor(stats["obs_mean"], dtype=torch.float64))
        self.obs_var.copy_(torch.as_tensor(stats["obs_var"], dtype=torch.float64))
        self._obs_count.fill_(float(stats["count"]))
        self.ret_mean.fill_(float(stats["ret_mean"]))
        self.ret_var.fill_(float(stats["ret_var"]))
        self._ret_count.fill_(float(stats.get("ret_count", stats["count"])))
        return self

    def stats(self):
        """the dictionary load_vecnormalize_pkl returns, for save_vecnormalize_pkl"""
        return {"obs_mean": self.obs_mean.cpu().numpy(), "obs_var": self.obs_var.cpu().numpy(), "count": float(self.obs_count),
                "ret_mean": float(self.ret_mean), "ret_var": float(self.ret_var), "ret_count": float(self.ret_count),
                "clip_obs": self.clip_obs, "clip_reward": self.clip_reward, "gamma": self.gamma, "epsilon": self.epsilon}

    @staticmethod
    def _update(mean, var, count, batch):
        """RunningMeanStd.update_from_moments (parallel-variance update), in place on the three tensors"""
        b = batch.to(torch.float64)
        bm, bv, bn = b.mean(0), b.var(0, unbiased=False), b.shape[0]
        delta, tot = bm - mean, count + bn
        new_mean = mean + delta * bn / tot
        m2 = var * count + bv * bn + delta * delta * count * bn / tot
        mean.copy_(new_mean); var.copy_(m2 / tot); count.copy_(tot)

    def normalize_obs(self, obs, update=None):
        """update: None -- the statistics take `obs` in first when self.training says so; False -- they are only read, whatever self.training says"""
        if self.training if update is None else update:
            self._update(self.obs_mean, self.obs_var, self._obs_count, obs)
        out = (obs.to(torch.float64) - self.obs_mean) / torch.sqrt(self.obs_var + self.epsilon)
        return torch.clamp(out, -self.clip_obs, self.clip_obs).to(torch.float32)

    def normalize_reward(self, rew, done):
        if self.training:
            self.returns.mul_(self.gamma).add_(rew.to(torch.float64))
            self._update(self.ret_mean, self.ret_var, self._ret_count, self.returns)
            self.returns.masked_fill_(done.bool(), 0.0)
        if not self.norm_reward:
            return rew
        return torch.clamp(rew.to(torch.float64) / torch.sqrt(self.ret_var + self.epsilon), -self.clip_reward, self.clip_reward).to(torch.float32)


class MlpActorCritic(torch.nn.Module):
    """SB3 ActorCriticPolicy(MlpPolicy, net_arch=[dict(pi=[256,128], vf=[256,128])]) with tanh activations and a state-independent
    log_std (rl_config.yaml:11-15; layer names as in the checkpoints' policy.pth)."""

    def __init__(self, obs_dim=19, act_dim=6, pi=(256, 128), vf=(256, 128)):
        super().__init__()
        def mlp(sizes):
            layers, d = [], obs_dim
            for h in sizes:
                layers += [torch.nn.Linear(d, h), torch.nn.Tanh()]
                d = h
            return torch.nn.Sequential(*layers)
        self.pi_sizes, self.vf_sizes = tuple(pi), tuple(vf)
        self.policy_net, self.value_net_body = mlp(pi), mlp(vf)
        self.action_net = torch.nn.Linear(pi[-1], act_dim)
        self.value_net = torch.nn.Linear(vf[-1], 1)
        self.log_std = torch.nn.Parameter(torch.zeros(act_dim))

    @classmethod
    def from_sb3_state_dict(cls, sd):
        act_dim, obs_dim = sd["action_net.weight"].shape[0], sd["mlp_extractor.policy_net.0.weight"].shape[1]
        self = cls(obs_dim, act_dim, (sd["mlp_extractor.policy_net.0.weight"].shape[0], sd["mlp_extractor.policy_net.2.weight"].shape[0]),
                   (sd["mlp_extractor.value_net.0.weight"].shape[0], sd["mlp_extractor.value_net.2.weight"].shape[0]))
        mapped = {}
        for k, v in sd.items():
            k2 = k.replace("mlp_extractor.policy_net.", "policy_net.").replace("mlp_extractor.value_net.", "value_net_body.")
            mapped[k2] = torch.as_tensor(v)
        self.load_state_dict(mapped)
        return self

    def to_sb3_state_dict(self):
        """state dict under the layer names of SB3's ActorCriticPolicy (the inverse of from_sb3_state_dict)"""
        out = {}
        for k, v in self.state_dict().items():
            k2 = k.replace("value_net_body.", "mlp_extractor.value_net.")
            if k2.startswith("policy_net."):
                k2 = "mlp_extractor." + k2
            out[k2] = v.detach().cpu().clone()
        return out

    def forward(self, obs):
        return self.action_net(self.policy_net(obs)), self.value_net(self.value_net_body(obs)).squeeze(-1)

    @staticmethod
    def _log_prob(mean, log_std, act):
        var = torch.exp(2.0 * log_std)
        return (-0.5 * ((act - mean) ** 2 / var) - log_std - 0.9189385332046727).sum(-1)       # DiagGaussianDistribution.log_prob

    @torch.no_grad()
    def sample(self, obs, generator=None):
        """ActorCriticPolicy.forward as collect_rollouts uses it: (unclipped action sample, value, log-probability)"""
        mean, value = self.forward(obs)
        act = mean + torch.exp(self.log_std) * torch.randn(mean.shape, device=mean.device, generator=generator)
        return act, value, self._log_prob(mean, self.log_std, act)

    def evaluate_actions(self, obs, act):
        """ActorCriticPolicy.evaluate_actions: (values, log-probabilities, entropy) with gradients, for a PPO update"""
        mean, value = self.forward(obs)
        ent = (0.5 + 0.9189385332046727 + self.log_std).sum(-1).expand(mean.shape[0])
        return value, self._log_prob(mean, self.log_std, act), ent

    @torch.no_grad()
    def predict(self, obs, deterministic=True, low=None, high=None, generator=None):
        """PPO.predict: Gaussian mean (or a sample), clipped to the action box like SB3 does before env.step"""
        mean, _ = self.forward(obs)
        act = mean if deterministic else mean + torch.exp(self.log_std) * torch.randn(mean.shape, device=mean.device, generator=generator)
        if low is not None:
            act = torch.max(torch.min(act, high), low)
        return act


# the header's field order (usim_policy_net) as attribute paths of MlpActorCritic
FIELDS = (("pi_w1", "policy_net.0.weight"), ("pi_b1", "policy_net.0.bias"), ("pi_w2", "policy_net.2.weight"), ("pi_b2", "policy_net.2.bias"),
          ("act_w", "action_net.weight"), ("act_b", "action_net.bias"), ("vf_w1", "value_net_body.0.weight"), ("vf_b1", "value_net_body.0.bias"),
          ("vf_w2", "value_net_body.2.weight"), ("vf_b2", "value_net_body.2.bias"), ("val_w", "value_net.weight"), ("val_b", "value_net.bias"),
          ("log_std", "log_std"))


def policy_net(policy, w2_packed=None):
    """usim_policy_net of a MlpActorCritic: the addresses of its parameters as they are now, in FIELDS order, and of `w2_packed` (a tensor for usim_policy_pack's
    output; None where no kernel reads it: the learners)"""
    params = dict(policy.named_parameters())
    return _lib.UsimPolicyNet(*(params[path].data_ptr() for _, path in FIELDS), None if w2_packed is None else w2_packed.data_ptr())


@torch.no_grad()
def policy_rollout(env, policy, vecnorm, steps, deterministic=False, seed=0, fused=False):
    """Run `steps` env steps of the policy on the device-resident fast path (no host synchronisation inside the loop).
    Returns raw-observation running statistics (mean, var over all visited steps), mean reward per step, and episode stats.
    fused=True: normalisation, both MLPs, sampling and clipping by the library's policy kernel (usim_policy_step) instead of PyTorch modules."""
    dev = env.device
    fr = FusedRollout(env, policy, vecnorm, DeviceRolloutBuffer(1, env.num_envs, 19, env.action_dim, device=dev), seed=seed, graph=False, init_stats=False) if fused else None
    low = torch.as_tensor(env.action_space.low, device=dev)
    high = torch.as_tensor(env.action_space.high, device=dev)
    gen = torch.Generator(device=dev); gen.manual_seed(seed)
    obs = env.reset_tensor()
    n = env.num_envs
    s1 = torch.zeros(obs.shape[1], dtype=torch.float64, device=dev); s2 = torch.zeros_like(s1)
    rew_sum = torch.zeros((), dtype=torch.float64, device=dev)
    ep_n = torch.zeros((), dtype=torch.float64, device=dev); ep_r = torch.zeros_like(ep_n); ep_l = torch.zeros_like(ep_n)
    if fr is not None:
        fr.pack()                                       # the weights do not change inside the loop: one pack launch, not one per step
    for _ in range(steps):
        o = obs.to(torch.float64)
        s1 += o.sum(0); s2 += (o * o).sum(0)
        if fr is not None:
            act, _ = fr.act(obs, None, counter=_, deterministic=deterministic, pack=False)
        else:
            act = policy.predict(vecnorm.normalize_obs(obs), deterministic, low, high, gen)
        obs, rew, done = env.step_tensor(act)
        vecnorm.normalize_reward(rew, done)
        rew_sum += rew.sum()
        d = done.bool()
        ep_n += d.sum(); ep_r += env.episode_return[d].sum(); ep_l += env.episode_length[d].sum()
    tot = steps * n
    mean = s1 / tot
    out = {"obs_mean": mean.cpu().numpy(), "obs_var": (s2 / tot - mean * mean).cpu().numpy(), "reward_per_step": float(rew_sum / tot),
           "episodes": float(ep_n), "mean_episode_return": float(ep_r / ep_n) if ep_n > 0 else float("nan"),
           "mean_episode_length": float(ep_l / ep_n) if ep_n > 0 else float("nan")}
    return out


class DeviceRolloutBuffer:
    """stable_baselines3.common.buffers.RolloutBuffer on the device (src/rl.py:143 builds PPO with SB3's defaults: n_steps 2048,
    gamma 0.99, gae_lambda 0.95): [T, n, ...] tensors filled step by step, GAE(lambda) returns/advantages, flattened minibatches.
    Nothing leaves the GPU between env.step_tensor() and the learner."""

    def __init__(self, buffer_size, num_envs, obs_dim=19, act_dim=6, device="cuda:0", gamma=0.99, gae_lambda=0.95):
        self.buffer_size, self.n_envs, self.gamma, self.gae_lambda = int(buffer_size), int(num_envs), float(gamma), float(gae_lambda)
        self.device = torch.device(device)
        T, n = self.buffer_size, self.n_envs
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.observations, self.actions = z(T, n, obs_dim), z(T, n, act_dim)
        self.rewards, self.episode_starts, self.values, self.log_probs = z(T, n), z(T, n), z(T, n), z(T, n)
        self.advantages, self.returns = z(T, n), z(T, n)
        self.reset()

    def reset(self):
        self.pos, self.full = 0, False

    def write(self, t, obs, action, reward, episode_start, value, log_prob):
        """the six slices of step t (no bookkeeping: a recorded rollout writes the same slices at every replay)"""
        self.observations[t].copy_(obs); self.actions[t].copy_(action); self.rewards[t].copy_(reward)
        self.episode_starts[t].copy_(episode_start.to(torch.float32)); self.values[t].copy_(value); self.log_probs[t].copy_(log_prob)

    def add(self, obs, action, reward, episode_start, value, log_prob):
        if self.pos >= self.buffer_size:
            raise RuntimeError("rollout buffer is full")
        self.write(self.pos, obs, action, reward, episode_start, value, log_prob)
        self.pos += 1
        self.full = self.pos == self.buffer_size

    def compute_returns_and_advantage(self, last_values, dones):
        """GAE exactly as RolloutBuffer.compute_returns_and_advantage: `dones` are the done flags of the last stored step"""
        last_gae = torch.zeros(self.n_envs, dtype=torch.float32, device=self.device)
        for step in reversed(range(self.buffer_size)):
            if step == self.buffer_size - 1:
                next_non_terminal, next_values = 1.0 - dones.to(torch.float32), last_values
            else:
                next_non_terminal, next_values = 1.0 - self.episode_starts[step + 1], self.values[step + 1]
            delta = self.rewards[step] + self.gamma * next_values * next_non_terminal - self.values[step]
            last_gae = delta + self.gamma * self.gae_lambda * next_non_terminal * last_gae
            self.advantages[step] = last_gae
        self.returns = self.advantages + self.values

    def get(self, batch_size=None, generator=None):
        """minibatches of the flattened [T * n] samples (swap_and_flatten order: env-major), shuffled like SB3"""
        if not self.full:
            raise RuntimeError("rollout buffer is not full")
        N = self.buffer_size * self.n_envs
        flat = lambda x: x.transpose(0, 1).reshape(N, *x.shape[2:])
        data = tuple(flat(x) for x in (self.observations, self.actions, self.values, self.log_probs, self.advantages, self.returns))
        perm = torch.randperm(N, device=self.device, generator=generator)
        bs = N if batch_size is None else int(batch_size)
        for i in range(0, N, bs):
            idx = perm[i:i + bs]
            yield tuple(x[idx] for x in data)


@torch.no_grad()
def _rollout_step(env, policy, vecnorm, low, high, obs, episode_start, generator=None, store=None, raw_reward_sum=None, bootstrap_gamma=None):
    """One step of the rollout loop, for collect_rollouts and GraphedCollector alike: normalise the observation, sample, clip the action to the box
    for the env, step, normalise the reward; store(normalised obs, unclipped action, normalised reward, episode_start, value, log-prob) where a store is
    given.  bootstrap_gamma (the buffer's gamma; None: off): SB3's time-limit bootstrap -- where the step ended at the horizon (env.truncated) the
    normalised reward becomes reward + gamma V(terminal observation), the terminal observation normalised with the statistics as they are after this
    step (frozen for that normalisation: VecNormalize.step_wait has already seen the new observation).  A `where` on all environments, not a product with the
    mask (rows of terminal_obs that are not truncated are stale and may hold anything) and no indexing: nothing synchronises, so the step can be captured.
    Returns (next raw obs, next episode_start, done flags of this step); the first two are copies: the env rewrites its buffers."""
    nobs = vecnorm.normalize_obs(obs)
    act, value, logp = policy.sample(nobs, generator)
    obs, rew, done = env.step_tensor(torch.max(torch.min(act, high), low))
    if raw_reward_sum is not None:
        raw_reward_sum.add_(rew.sum())
    nrew = vecnorm.normalize_reward(rew, done)
    if bootstrap_gamma is not None:
        nrew = _bootstrap_truncated(policy, vecnorm, nrew, obs, env.terminal_obs, env.truncated, bootstrap_gamma)
    if store is not None:
        store(nobs, act, nrew, episode_start, value, logp)
    return obs.clone(), done.bool().clone(), done


@torch.no_grad()
def _bootstrap_value(policy, vecnorm, obs):
    """SB3 bootstraps with the value of the stored, already normalised `_last_obs`: the statistics are not updated a second time"""
    return policy.forward(vecnorm.normalize_obs(obs, update=False))[1]


@torch.no_grad()
def _bootstrap_truncated(policy, vecnorm, nrew, next_obs, terminal_obs, truncated, gamma):
    """-> where(truncated, nrew + gamma V(normalize(terminal_obs)), nrew).  This loop updates the observation statistics when an observation is CONSUMED (the
    next step's normalize_obs), SB3's VecNormalize.step_wait when the env RETURNS it and before it normalises the terminal observation: while training, the
    statistics therefore take `next_obs` in for this normalisation and are put back, bit for bit, afterwards."""
    rms = (vecnorm.obs_mean, vecnorm.obs_var, vecnorm._obs_count)
    kept = [t.clone() for t in rms] if vecnorm.training else None
    if kept is not None:
        vecnorm._update(*rms, next_obs)
    value = _bootstrap_value(policy, vecnorm, terminal_obs)
    if kept is not None:
        for t, k in zip(rms, kept):
            t.copy_(k)
    return torch.where(truncated, nrew + float(gamma) * value, nrew)


def _capture(env, record, prologue=None, generator=None):
    """record() as a HIP graph (torch.cuda.CUDAGraph), captured on a side stream.  Library handles, lazy initialisation and the allocator's warm-up must
    happen outside the capture: `prologue` runs eagerly on the side stream first.  The reset bank is refilled before the capture (env.refill_bank)."""
    dev = env.device
    graph = torch.cuda.CUDAGraph()
    if generator is not None:
        graph.register_generator_state(generator)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        if prologue is not None:
            prologue()
        env.refill_bank()
        torch.cuda.current_stream(dev).synchronize()
        with torch.cuda.graph(graph, stream=side):
            record()
    torch.cuda.current_stream(dev).wait_stream(side)
    return graph


@torch.no_grad()
def collect_rollouts(env, policy, vecnorm, buffer, obs=None, episode_start=None, generator=None, bootstrap_truncation=False):
    """OnPolicyAlgorithm.collect_rollouts for one buffer: sample actions from the policy on normalised observations, clip them to
    the action box for the env, store the unclipped sample, normalise rewards, bootstrap with the value of the last observation.
    SB3 also bootstraps time-limit truncations with the terminal observation's value; the reference's GymWrapper does not report
    truncations, so by default no reward is touched.  bootstrap_truncation=True: rewards of steps that ended at the horizon
    (env.truncated) get + gamma V(terminal observation), gamma the buffer's (_rollout_step).
    Returns (next raw obs, next episode_start) to continue from."""
    dev = env.device
    low, high = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
    if obs is None:
        obs = env.reset_tensor()
    if episode_start is None:
        episode_start = torch.ones(env.num_envs, dtype=torch.bool, device=dev)
    buffer.reset()
    done = episode_start
    for _ in range(buffer.buffer_size):
        obs, episode_start, done = _rollout_step(env, policy, vecnorm, low, high, obs, episode_start, generator, buffer.add,
                                                 bootstrap_gamma=buffer.gamma if bootstrap_truncation else None)
    buffer.compute_returns_and_advantage(_bootstrap_value(policy, vecnorm, obs), done.bool())
    return obs, episode_start


class GraphedCollector:
    """collect_rollouts recorded once as a HIP graph (torch.cuda.CUDAGraph) and replayed with one launch per rollout.

    With a policy in the loop a rollout step is ~40 small launches -- observation statistics and normalisation, two MLPs, sampling, clipping, the
    simulator step, return statistics, six buffer writes -- and the simulator kernel is 15 us of it: issued one by one from Python the loop is bound
    by launch overhead (~0.4 ms per step at 2048 environments).  The loop has no host dependency (the simulator resets finished environments on
    the device, the running statistics are tensors updated in place), so the T steps of a rollout, the bootstrap value and the GAE recursion are
    captured into one graph; `collect()` replays it.  Semantics are those of collect_rollouts (same operations in the same order on the same
    tensors): `tests/test_gpu_policy_replay.py` compares the two bit for bit.

    The simulator's reset bank is refilled every 256 steps by a launch that usim_step issues from a HOST counter, which does not advance at replay:
    the recorded sequence therefore starts and ends with an explicit refill (env.refill_bank) and contains the periodic ones in between, so every
    ring is valid at every replay for any T.  Sampling uses the default CUDA generator (graph-safe: the Philox offset advances per replay) or a
    generator registered with the graph.  The policy's parameters are read at their addresses: an optimiser that updates them in place (torch.optim)
    is seen by the next replay."""

    def __init__(self, env, policy, vecnorm, buffer, generator=None, warmup_steps=2, bootstrap_truncation=False):
        self.env, self.policy, self.vecnorm, self.buffer, self.generator = env, policy, vecnorm, buffer, generator
        self.bootstrap_truncation = bool(bootstrap_truncation)                  # collect_rollouts' option: recorded with the rest (no host dependency)
        dev = env.device
        self._low, self._high = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
        self.obs = env.reset_tensor().clone()                                   # raw observation the next rollout starts from
        self.episode_start = torch.ones(env.num_envs, dtype=torch.bool, device=dev)
        self.last_done = torch.zeros(env.num_envs, dtype=torch.bool, device=dev)
        self.raw_reward_sum = torch.zeros((), dtype=torch.float64, device=dev)  # sum of the raw rewards of the last rollout (diagnostics)
        def warm_up():
            # a few eager steps: real ones (the statistics and the environments advance), exactly like the first steps of an eager collect_rollouts
            obs, start = self.obs, self.episode_start
            for _ in range(warmup_steps):
                obs, start, _ = self._step(obs, start, None)
            self.obs.copy_(obs); self.episode_start.copy_(start)
        self.graph = _capture(env, self._record, warm_up, generator)
        buffer.pos, buffer.full = buffer.buffer_size, True

    def _step(self, obs, episode_start, t):
        """_rollout_step; with t, into the buffer slices of step t and the reward sum"""
        store, raw_sum = (None, None) if t is None else (functools.partial(self.buffer.write, t), self.raw_reward_sum)
        return _rollout_step(self.env, self.policy, self.vecnorm, self._low, self._high, obs, episode_start, self.generator, store, raw_sum,
                             bootstrap_gamma=self.buffer.gamma if self.bootstrap_truncation else None)

    @torch.no_grad()
    def _record(self):
        b = self.buffer
        obs, start = self.obs, self.episode_start
        self.env.refill_bank()                 # first node of the recorded sequence as well as the last: a replay does not depend on what ran before it
        self.raw_reward_sum.zero_()
        done = None
        for t in range(b.buffer_size):
            obs, start, done = self._step(obs, start, t)
        last_value = _bootstrap_value(self.policy, self.vecnorm, obs)
        self.last_done.copy_(done.bool())
        b.compute_returns_and_advantage(last_value, self.last_done)
        self.obs.copy_(obs); self.episode_start.copy_(start)
        self.env.refill_bank()

    def collect(self):
        """one rollout of buffer.buffer_size steps into the buffer (returns / advantages included); returns (next raw obs, next episode_start)"""
        self.graph.replay()
        self.buffer.pos, self.buffer.full = self.buffer.buffer_size, True
        return self.obs, self.episode_start


class FusedRollout:
    """The rollout loop with the policy in it on the library's fused kernels (include/usim.h usim_policy_step / usim_policy_reward / usim_policy_gae;
    csrc/usim_policy.hip) instead of ~100 PyTorch launches per step: per step one statistics kernel, one kernel that normalises the observation,
    runs both MLPs on the matrix cores, samples, clips and writes the buffer slices, the simulator step, and one reward kernel; GAE is one more
    kernel per rollout.  The whole rollout is recorded as a HIP graph, as in GraphedCollector.  The parameters stay the torch module's (read at
    their addresses), the statistics stay the DeviceVecNormalize's tensors, the buffer is the DeviceRolloutBuffer: a PPO update written against
    those objects is unchanged.  Differences from collect_rollouts: sums are ordered differently (agreement to rounding, not bit for bit) and the
    Gaussian noise comes from the library's counter-based stream (seed, environment, step), not from a torch generator."""

    def __init__(self, env, policy, vecnorm, buffer, seed=0, graph=True, fused_stats=None, init_stats=True, bootstrap_truncation=False):
        # bootstrap_truncation: SB3's time-limit bootstrap (usim_policy_bootstrap: one more small launch per step; off: the launches are exactly those below).
        # `truncations` counts the truncated environment-steps of the last rollout on the device.
        self.bootstrap_truncation = bool(bootstrap_truncation)
        self.truncations = torch.zeros(1, dtype=torch.int32, device=env.device)
        # fused_stats: VecNormalize's two updates inside the policy launch (usim_policy_step_fused: two launches per step instead of three).  Its workgroups wait
        # for one another, so all of them must be resident: by default only up to 4096 environments (256 workgroups, half of what the device holds -- room
        # for a collective's kernels beside them); fused_stats=True asks for it up to the library's limit of 8192 (a device to itself)
        self.fused_stats = (vecnorm.training and env.num_envs <= 4096) if fused_stats is None else bool(fused_stats)
        if self.fused_stats and not vecnorm.training:
            raise ValueError("fused_stats is the training path (frozen statistics need no update kernels)")
        if policy.pi_sizes != (256, 128) or policy.vf_sizes != (256, 128) or policy.policy_net[0].in_features != 19:
            raise ValueError("the fused kernels implement the MlpPolicy of the shipped checkpoints: 19 -> 256 -> 128 (tanh) for both networks")
        self.env, self.policy, self.vecnorm, self.buffer, self.seed = env, policy, vecnorm, buffer, int(seed)
        self.lib = _lib.load()
        dev = env.device
        for p_ in policy.parameters():
            if p_.device != dev or p_.dtype != torch.float32 or not p_.is_contiguous():
                raise ValueError("policy parameters must be contiguous float32 tensors on the environment's device")
        ptr = lambda t: t.data_ptr()
        # layer-2 weights of both networks in the order the matrix-core operands consume them (usim_policy_pack; include/usim.h): packed again before every eager
        # launch and as the first policy node of a recorded rollout, so a parameter update between rollouts is seen as before
        self._w2_packed = torch.zeros(_lib.POLICY_PACKED, dtype=torch.float32, device=dev)
        self._net = policy_net(policy, self._w2_packed)
        vn = vecnorm
        self._scratch = torch.zeros(_lib.POLICY_SCRATCH, dtype=torch.float64, device=dev)
        self._stats = _lib.UsimNormStats(ptr(vn.obs_mean), ptr(vn.obs_var), ptr(vn._obs_count), ptr(vn.ret_mean), ptr(vn.ret_var), ptr(vn._ret_count), ptr(vn.returns),
                                         ptr(self._scratch), float(vn.clip_obs), float(vn.clip_reward), float(vn.gamma), float(vn.epsilon))
        self._low = torch.as_tensor(env.action_space.low, dtype=torch.float32, device=dev).contiguous()
        self._high = torch.as_tensor(env.action_space.high, dtype=torch.float32, device=dev).contiguous()
        self._act_env = torch.zeros(env.num_envs, env.action_dim, dtype=torch.float32, device=dev)
        self._value = torch.zeros(env.num_envs, dtype=torch.float32, device=dev)
        self.raw_reward_sum = torch.zeros((), dtype=torch.float64, device=dev)
        self.counter = 0                                                                    # rollouts collected
        self._ctr = torch.zeros(1, dtype=torch.int32, device=dev)                           # device part of the noise counter: advanced by every rollout
        self._work = torch.zeros(_lib.policy_fused_work(env.num_envs), dtype=torch.float64, device=dev)
        self.obs = env.reset_tensor()                                                       # the env's own observation buffer: rewritten by every step
        self._prev_done = env._done                                                         # ... and its done flags: read by the policy kernel BEFORE the next step rewrites them
        self._prev_done.fill_(1)                                                            # every environment starts an episode
        if vecnorm.training and init_stats:                                                 # VecNormalize.reset(): the statistics see the reset observation (init_stats=False: the caller's first act(training=1) does)
            self.act(self.obs, self._prev_done, counter=0, training=1, deterministic=True)
        self.graph = _capture(env, self._record) if graph else None

    def _check(self, rc):
        _lib.check(self.lib, rc, None)

    def pack(self):
        """usim_policy_pack: the layer-2 weights as they are now, in operand order (a launch of 64 workgroups)"""
        self._check(self.lib.usim_policy_pack(C.byref(self._net), self._w2_packed.data_ptr(), self.env._stream()))

    def _out(self, t):
        """usim_policy_out: the env's action; with t, the buffer slices of step t; without, only the value (into a tensor of its own)"""
        b = self.buffer
        if t is None:
            return _lib.UsimPolicyOut(self._act_env.data_ptr(), None, None, self._value.data_ptr(), None, None)
        return _lib.UsimPolicyOut(self._act_env.data_ptr(), b.observations[t].data_ptr(), b.actions[t].data_ptr(), b.values[t].data_ptr(), b.log_probs[t].data_ptr(),
                                  b.episode_starts[t].data_ptr())

    def act(self, obs, prev_done, counter, training=None, deterministic=False, t=None, pack=True):
        """usim_policy_step on raw observations [n, 19]: returns (clipped action for the env, value); with t, the buffer slices of step t are written"""
        env, b = self.env, self.buffer
        if pack:
            self.pack()
        training = self.vecnorm.training if training is None else training
        ptr = lambda x: None if x is None else x.data_ptr()
        out = self._out(t)
        self._check(self.lib.usim_policy_step(C.byref(self._net), C.byref(self._stats), ptr(obs), ptr(prev_done), env.num_envs, env.action_dim, ptr(self._low), ptr(self._high),
                                              self.seed, int(counter) & 0xffffffff, ptr(self._ctr), int(env.env_offset), int(training),
                                              int(bool(deterministic)), C.byref(out), env._stream()))
        return self._act_env, (self._value if t is None else b.values[t])

    def _fused(self, t, rewards_out):
        env, vn = self.env, self.vecnorm
        prev = t > 0
        return _lib.UsimPolicyFused(self._work.data_ptr(), env._rew.data_ptr() if prev else None, env._done.data_ptr() if prev else None,
                                    rewards_out.data_ptr() if prev else None, self.raw_reward_sum.data_ptr(), int(prev), int(prev), int(bool(vn.norm_reward)), 0)

    def act_fused(self, obs, prev_done, counter, rewards_out=None, deterministic=False, t=None, pack=True):
        """usim_policy_step_fused: as act(), with RunningMeanStd.update(obs) and the reward side of the step before (normalised into rewards_out) in the same
        launch when counter > 0"""
        env = self.env
        if pack:
            self.pack()
        ptr = lambda x: None if x is None else x.data_ptr()
        out, f = self._out(t), self._fused(counter, rewards_out)
        self._check(self.lib.usim_policy_step_fused(C.byref(self._net), C.byref(self._stats), C.byref(f), ptr(obs), ptr(prev_done), env.num_envs, env.action_dim,
                                                    ptr(self._low), ptr(self._high), self.seed, int(counter) & 0xffffffff, ptr(self._ctr),
                                                    int(env.env_offset), int(bool(deterministic)), C.byref(out), env._stream()))

    def _bootstrap(self, t):
        """usim_policy_bootstrap on the env's buffers of the step just taken, into the (already written) rewards of buffer row t"""
        env, b = self.env, self.buffer
        self._check(self.lib.usim_policy_bootstrap(C.byref(self._net), C.byref(self._stats), env._term.data_ptr(), env._done.data_ptr(), env._ep_len.data_ptr(),
                                                   env.num_envs, int(env.horizon), b.gamma, b.rewards[t].data_ptr(), self.truncations.data_ptr(), env._stream()))

    @property
    def wait_ran_out(self):
        """True if a workgroup of usim_policy_step_fused ever gave up waiting for the others' partial sums (the device was shared; statistics are then wrong)"""
        rows = _lib.policy_fused_rows(self.env.num_envs)
        flags = self._work[rows * _lib.POLICY_FUSED_ROW:].view(torch.int32)                 # two arrival flags per row, then the status word
        return bool(flags[2 * rows].item())

    def _record(self):
        """one rollout: T x (policy, env[, reward]) + bootstrap value + GAE.  The noise of step t is keyed on (seed, environment, t + device counter); the
        recorded sequence advances the device counter by T + 1 at its end, so a replay draws fresh noise.
        fused_stats: two launches per step -- the policy launch also takes the statistics of the observation it reads and the reward side of the step before.
        Otherwise three, and the observation statistics follow VecNormalize's timing: RunningMeanStd.update(obs) when the environment RETURNS the observation
        (reset: once, in __init__; step: in the launch that also does the reward side), so the policy kernel only normalises (training = 2) and the bootstrap
        value sees statistics that include the last observation, as SB3's `_last_obs` does.
        bootstrap_truncation: usim_policy_bootstrap of step t goes where rewards[t] has been written, the statistics contain the observation step t returned and
        the env's buffers of step t are still intact -- right after the reward launch of step t, or (fused_stats: rewards[t] is written by the policy launch of
        step t + 1) between that launch and the env step t + 1; for the last step after the bootstrap-value launch."""
        env, b, vn = self.env, self.buffer, self.vecnorm
        T, n = b.buffer_size, env.num_envs
        boot = self.bootstrap_truncation
        env.refill_bank()                      # first node of the recorded sequence as well as the last: a replay is valid whatever ran on the env since the last one
        self.raw_reward_sum.zero_()
        if boot:
            self.truncations.zero_()
        self.pack()                            # the weights of this rollout (they do not change inside it)
        for t in range(T):
            if self.fused_stats:
                self.act_fused(self.obs, self._prev_done, counter=t, rewards_out=b.rewards[t - 1] if t else None, t=t, pack=False)
                if boot and t:
                    self._bootstrap(t - 1)
                env.step_tensor(self._act_env)
            else:
                self.act(self.obs, self._prev_done, counter=t, training=2 if vn.training else 0, t=t, pack=False)
                o, rew, done = env.step_tensor(self._act_env)
                self._check(self.lib.usim_policy_reward(C.byref(self._stats), rew.data_ptr(), done.data_ptr(), n, int(bool(vn.training)), int(bool(vn.norm_reward)),
                                                        b.rewards[t].data_ptr(), self.raw_reward_sum.data_ptr(), o.data_ptr() if vn.training else None, env._stream()))
                if boot:
                    self._bootstrap(t)
        if self.fused_stats:                   # bootstrap value (+ the last step's reward side)
            self.act_fused(self.obs, self._prev_done, counter=T, rewards_out=b.rewards[T - 1], deterministic=True, pack=False)
            if boot:
                self._bootstrap(T - 1)
        else:
            self.act(self.obs, self._prev_done, counter=T, training=0, deterministic=True, pack=False)
        self._check(self.lib.usim_policy_gae(b.rewards.data_ptr(), b.values.data_ptr(), b.episode_starts.data_ptr(), self._value.data_ptr(), self._prev_done.data_ptr(),
                                             T, n, b.gamma, b.gae_lambda, b.advantages.data_ptr(), b.returns.data_ptr(), env._stream()))
        self._ctr.add_(T + 1)
        env.refill_bank()

    def collect(self, check=True):
        """one rollout of buffer.buffer_size steps into the buffer (returns / advantages included).  With the in-launch statistics exchange
        (fused_stats) the status word of the exchange is read once per rollout (one host synchronisation; check=False leaves it to the caller):
        a workgroup that gave up waiting for the others -- the device was shared with something that took its CUs -- has normalised with
        partial sums, and the rollout must not be used.  (The workgroup that writes the running statistics back skips its stores when its own wait ran out, so the
        caller's VecNormalize is then the one of the step before -- not a corrupted one; the buffer's normalised observations of that step are still wrong.)"""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._record()
        if check and self.fused_stats and self.wait_ran_out:
            raise RuntimeError("usim_policy_step_fused: a workgroup ran out of its bounded wait for the other workgroups' statistics (device shared with "
                               "another kernel?); this rollout's observation / return statistics are incomplete -- use FusedRollout(..., fused_stats=False)")
        self.counter += 1
        self.buffer.pos, self.buffer.full = self.buffer.buffer_size, True
        return self.obs, self._prev_done
