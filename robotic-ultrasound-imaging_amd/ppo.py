"""The PPO learner on the device: stable-baselines3's `PPO.train` (the `model.learn` of src/rl.py:143) as two library calls per minibatch -- usim_ppo_grad (loss,
statistics and the gradient for every parameter of the shipped MlpPolicy) and usim_ppo_adam (clip_grad_norm_ + Adam.step) on ONE flat parameter block
(include/usim.h; csrc/usim_ppo.hip).  The collector (policy.FusedRollout), the running statistics (policy.DeviceVecNormalize), the buffer
(policy.DeviceRolloutBuffer) and the checkpoint writer (policy.save_sb3_zip) are the ones of policy.py: the module's parameters become views into the flat block,
so all of them keep working on the same memory.

    policy = MlpActorCritic(19, env.action_dim).to(env.device)
    theta = flatten_parameters(policy)                     # BEFORE the collector is built: it records the parameters' addresses
    collector = FusedRollout(env, policy, vecnorm, buffer)
    ppo = NativePPO(env, policy, vecnorm, buffer, collector)
    ppo.learn(40); ppo.save("model.zip")
"""
import ctypes as C
import time

import torch

from . import _lib
from .policy import save_sb3_zip

# the header's field order (usim_policy_net) as attribute paths of policy.MlpActorCritic
FIELDS = (("pi_w1", "policy_net.0.weight"), ("pi_b1", "policy_net.0.bias"), ("pi_w2", "policy_net.2.weight"), ("pi_b2", "policy_net.2.bias"),
          ("act_w", "action_net.weight"), ("act_b", "action_net.bias"), ("vf_w1", "value_net_body.0.weight"), ("vf_b1", "value_net_body.0.bias"),
          ("vf_w2", "value_net_body.2.weight"), ("vf_b2", "value_net_body.2.bias"), ("val_w", "value_net.weight"), ("val_b", "value_net.bias"),
          ("log_std", "log_std"))
STAT_NAMES = ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss",
              "train/explained_variance")       # the first six: usim_ppo_grad's statistics of the last minibatch; the seventh: usim_explained_variance on the buffer


def ppo_params(act_dim):
    """usim_ppo_params: floats of the flat parameter / gradient block"""
    return 76032 + 130 * int(act_dim) + 129


def _field_shapes(act_dim):
    A = int(act_dim)
    return ((256, 19), (256,), (128, 256), (128,), (A, 128), (A,), (256, 19), (256,), (128, 256), (128,), (1, 128), (1,), (A,))


def _check_shapes(policy):
    """-> act_dim; ValueError unless the module is the MlpPolicy the kernels implement: 19 -> 256 -> 128 -> A / 1, A <= 8"""
    params = dict(policy.named_parameters())
    if set(params) != {path for _, path in FIELDS}:
        raise ValueError("policy shapes: not a policy.MlpActorCritic with two hidden layers per network")
    A = int(params["log_std"].shape[0])
    if not 1 <= A <= 8:
        raise ValueError(f"policy shapes: act_dim {A} outside 1 .. 8")
    for (name, path), shape in zip(FIELDS, _field_shapes(A)):
        if tuple(params[path].shape) != shape:
            raise ValueError(f"policy shapes: {path} is {tuple(params[path].shape)}, the learner's kernels implement 19 -> 256 -> 128 -> A / 1 ({name}: {shape})")
    return A


def flatten_parameters(policy):
    """Re-seat the parameters of a policy.MlpActorCritic (19 -> 256 -> 128, A <= 8) as views into ONE contiguous float32 tensor in the order of include/usim.h
    (pi_w1 pi_b1 pi_w2 pi_b2 act_w act_b vf_w1 vf_b1 vf_w2 vf_b2 val_w val_b log_std) and return that tensor.  The values are kept; the module, a collector built
    AFTERWARDS and save_sb3_zip read and write the same memory as the learner.  Calling it again on a flattened module returns the same tensor."""
    A = _check_shapes(policy)
    params = dict(policy.named_parameters())
    theta = getattr(policy, "_flat_theta", None)
    if theta is not None and _is_flat(policy, theta):
        return theta
    first = params[FIELDS[0][1]]
    theta = torch.empty(ppo_params(A), dtype=torch.float32, device=first.device)
    o = 0
    with torch.no_grad():
        for (_, path), shape in zip(FIELDS, _field_shapes(A)):
            p, n = params[path], 1
            for s in shape:
                n *= s
            view = theta[o:o + n].view(shape)
            view.copy_(p.detach().to(torch.float32))
            p.data = view
            o += n
    assert o == theta.numel()
    policy._flat_theta = theta
    return theta


def _is_flat(policy, theta):
    params, o = dict(policy.named_parameters()), 0
    for _, path in FIELDS:
        p = params[path]
        if p.device != theta.device or p.dtype != torch.float32 or p.data_ptr() != theta.data_ptr() + 4 * o:
            return False
        o += p.numel()
    return o == theta.numel()


class NativePPO:
    """stable-baselines3's PPO update on the library's learner kernels, with SB3's defaults (what src/rl.py:143 runs with): learning_rate 3e-4, n_epochs 10,
    clip_range 0.2, ent_coef 0, vf_coef 0.5, max_grad_norm 0.5, per-minibatch advantage normalisation, Adam(eps 1e-5).

    batch_size=None means one eighth of the rollout (as tools/ppo_demo.py): SB3's default of 64 is a choice for eight environments x 2048 steps and is
    meaningless at 4096 environments -- 8192 minibatches of 64 per epoch would be 8192 launch pairs for what eight do.  learning_rate may be a callable of the
    remaining progress (1 at the start, 0 at the end of learn(): src/rl.py's linear_schedule); outside learn() the progress is 1.

    The policy must be flattened (flatten_parameters) BEFORE a collector that records parameter addresses (policy.FusedRollout) is built; a policy that is
    not flat yet is flattened here when no collector is given.  Refusals are ValueErrors raised before any library call."""

    def __init__(self, env, policy, vecnorm, buffer, collector=None, *, learning_rate=3e-4, n_epochs=10, batch_size=None, clip_range=0.2, ent_coef=0.0,
                 vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True, adam_eps=1e-5, seed=0):
        A = _check_shapes(policy)
        if A != int(env.action_dim):
            raise ValueError(f"policy shapes: act_dim {A} is not the environment's {env.action_dim}")
        dev = torch.device(env.device)
        if torch.device(buffer.device) != dev:
            raise ValueError(f"buffer is on device {buffer.device}, the environment on {dev}")
        rollout = int(buffer.buffer_size) * int(buffer.n_envs)
        batch_size = rollout // 8 if batch_size is None else int(batch_size)
        if not 1 <= batch_size <= rollout:
            raise ValueError(f"batch_size {batch_size} outside 1 .. the rollout's {rollout} samples")
        if int(n_epochs) < 1:
            raise ValueError("n_epochs must be at least 1")
        for p in policy.parameters():
            if p.device != dev:
                raise ValueError(f"policy is on device {p.device}, the environment on {dev}")
        theta = getattr(policy, "_flat_theta", None)
        if theta is None or not _is_flat(policy, theta):
            if collector is not None:
                raise ValueError("flatten_parameters(policy) must be called before the collector is built: it has recorded the parameters' addresses")
            theta = flatten_parameters(policy)
        self.env, self.policy, self.vecnorm, self.buffer, self.collector = env, policy, vecnorm, buffer, collector
        self.learning_rate, self.n_epochs, self.batch_size, self.rollout = learning_rate, int(n_epochs), batch_size, rollout
        self.clip_range, self.ent_coef, self.vf_coef, self.max_grad_norm = float(clip_range), float(ent_coef), float(vf_coef), float(max_grad_norm)
        self.normalize_advantage, self.adam_eps, self.act_dim = bool(normalize_advantage), float(adam_eps), A
        self.progress_remaining = 1.0
        self.lib = _lib.load()
        self.theta, self.params = theta, theta.numel()
        z = lambda n, dtype=torch.float32: torch.zeros(n, dtype=dtype, device=dev)
        self.grad, self.exp_avg, self.exp_avg_sq = z(self.params), z(self.params), z(self.params)
        self.step_count = z(1, torch.int32)                                   # Adam's step, advanced on the device
        self.stats = z(_lib.PPO_STATS)
        self.first_stats = z(_lib.PPO_STATS)                                  # the statistics of the first minibatch of the last update()
        self._ev = z(1)                                                       # train/explained_variance of the last update() (usim_explained_variance)
        self.history = []                                                     # learn(): one dict of logger scalars per iteration
        self.num_timesteps = 0                                                # environment steps collected by learn() so far
        self._work = z(int(self.lib.usim_ppo_work_floats(A)))
        self._index = torch.zeros(rollout, dtype=torch.int32, device=dev)
        self.generator = torch.Generator(device=dev)
        self.generator.manual_seed(int(seed))
        ptr = {name: dict(policy.named_parameters())[path].data_ptr() for name, path in FIELDS}
        self._net = _lib.UsimPolicyNet(*(ptr[name] for name, _ in FIELDS), None)

    def _check(self, rc):
        _lib.check(self.lib, rc, None)

    def _flat(self, x):
        """a [T, n, ...] buffer tensor in SB3's swap_and_flatten order (environment-major), contiguous"""
        T, n = x.shape[:2]
        return x.transpose(0, 1).reshape(T * n, *x.shape[2:]).contiguous()

    def current_lr(self):
        lr = self.learning_rate
        return float(lr(self.progress_remaining)) if callable(lr) else float(lr)

    def minibatch_step(self, data, index, batch, lr=None):
        """one usim_ppo_grad + one usim_ppo_adam on the rows `index` (an int32 device tensor, or None: rows 0 .. batch - 1) of the flattened slices `data` =
        (obs, act, old_logp, adv, ret)"""
        obs, act, lp, adv, ret = data
        b = _lib.UsimPpoBatch(obs.data_ptr(), act.data_ptr(), lp.data_ptr(), adv.data_ptr(), ret.data_ptr(), None if index is None else index.data_ptr(),
                              obs.shape[0], int(batch), self.act_dim, int(self.normalize_advantage), self.clip_range, self.ent_coef, self.vf_coef, 0.0)
        stream = self.env._stream()
        self._check(self.lib.usim_ppo_grad(C.byref(self._net), C.byref(b), self._work.data_ptr(), self.grad.data_ptr(), self.stats.data_ptr(), stream))
        self._check(self.lib.usim_ppo_adam(self.theta.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                           self.step_count.data_ptr(), self.params, self.current_lr() if lr is None else float(lr), 0.9, 0.999, self.adam_eps,
                                           self.max_grad_norm, self.stats.data_ptr(), stream))

    def update(self):
        """PPO.train on the buffer as it is: n_epochs passes, each a torch.randperm on the device cut into minibatches of batch_size (the trailing partial one
        is used, as in SB3), then the collector's pack().  -> the statistics of the last minibatch under SB3's logger names, and train/explained_variance of the
        buffer's values against its returns as they are BEFORE the first minibatch (SB3's explained_variance; one launch into a device word).  One host read at
        the end brings both."""
        b = self.buffer
        if not b.full:
            raise RuntimeError("rollout buffer is not full")
        values, returns = b.values.contiguous(), b.returns.contiguous()
        self._check(self.lib.usim_explained_variance(values.data_ptr(), returns.data_ptr(), values.numel(), self._ev.data_ptr(), self.env._stream()))
        data = tuple(self._flat(x) for x in (b.observations, b.actions, b.log_probs, b.advantages, b.returns))
        N, lr, first = self.rollout, self.current_lr(), True
        for _ in range(self.n_epochs):
            self._index.copy_(torch.randperm(N, device=self._index.device, generator=self.generator))
            for i in range(0, N, self.batch_size):
                n = min(self.batch_size, N - i)
                self.minibatch_step(data, self._index[i:i + n], n, lr)
                if first:
                    self.first_stats.copy_(self.stats)
                    first = False
        if self.collector is not None and hasattr(self.collector, "pack"):
            self.collector.pack()
        s = torch.cat((self.stats, self._ev)).tolist()                        # one read for both
        return dict(zip(STAT_NAMES, s[:6] + s[_lib.PPO_STATS:]))

    def learn(self, iterations):
        """`iterations` x (collector.collect(), update()); -> the statistics of the last update.  Every iteration appends one dict to self.history -- SB3's logger
        scalars: time/total_timesteps (environment steps collected by learn() so far), time/wall (time.time()), the train/* statistics of update(),
        train/learning_rate and, when the env has a monitor attached (env.attach_monitor, before the collector was built), its summary(): rollout/ep_rew_mean,
        rollout/ep_len_mean, ... -- the series monitor.write_scalar_csv writes out."""
        if self.collector is None:
            raise ValueError("learn() needs a collector")
        out = None
        for it in range(int(iterations)):
            self.progress_remaining = 1.0 - it / float(iterations)
            lr = self.current_lr()
            self.collector.collect()
            out = self.update()
            self.num_timesteps += self.rollout
            row = {"time/total_timesteps": self.num_timesteps, "time/wall": time.time(), **out, "train/learning_rate": lr}
            mon = getattr(self.env, "monitor", None)
            if mon is not None:
                row.update(mon.summary())
            self.history.append(row)
        self.progress_remaining = 1.0
        return out

    def adam_state_dict(self):
        """the learner's Adam state as `policy.optimizer.pth` of an SB3 checkpoint (policy.adam_state_dict shows the layout): moments per parameter in
        state-dict order, CPU tensors"""
        sd = self.policy.to_sb3_state_dict()
        step = int(self.step_count.item())
        mods = dict(self.policy.named_parameters())
        offset, o = {}, 0
        for _, path in FIELDS:
            offset[path] = o
            o += mods[path].numel()
        state = {}
        if step > 0:
            for i, name in enumerate(self.policy.state_dict()):
                o, p = offset[name], mods[name]
                cut = lambda t: t[o:o + p.numel()].view(p.shape).detach().cpu().clone()
                state[i] = {"step": step, "exp_avg": cut(self.exp_avg), "exp_avg_sq": cut(self.exp_avg_sq)}
        return {"state": state, "param_groups": [{"lr": self.current_lr(), "betas": (0.9, 0.999), "eps": self.adam_eps, "weight_decay": 0, "amsgrad": False,
                                                   "params": list(range(len(sd)))}]}

    def save(self, path, data=None):
        """the checkpoint zip of PPO.save (policy.save_sb3_zip) with the Adam moments"""
        save_sb3_zip(path, self.policy, data=data, optimizer_state=self.adam_state_dict())
