"""The PPO learner on the device: stable-baselines3's `PPO.train` (the `model.learn` of src/rl.py:143) as two library calls per minibatch -- usim_ppo_grad (loss,
statistics and the gradient for every parameter of the shipped MlpPolicy) and usim_ppo_adam (clip_grad_norm_ + Adam.step) on ONE flat parameter block
(include/usim.h; csrc/usim_ppo.hip).  The collector (policy.FusedRollout), the running statistics (policy.DeviceVecNormalize), the buffer
(policy.DeviceRolloutBuffer) and the checkpoint writer (policy.save_sb3_zip) are the ones of policy.py: the module's parameters become views into the flat block,
so all of them keep working on the same memory.

    policy = MlpActorCritic(19, env.action_dim).to(env.device)
    theta = flatten_parameters(policy)                     # BEFORE the collector is built: it records the parameters' addresses
    collector = FusedRollout(env, policy, vecnorm, buffer)
    ppo = NativePPO(env, policy, vecnorm, buffer, collector)
    ppo.set_evaluation(1_000_000, eval_env)                # SB3's EvalCallback: eval/mean_reward and the error metrics in ppo.history (evaluation.evaluate_episodes)
    ppo.set_checkpointing(1_000_000); ppo.learn(40); ppo.save_checkpoint("trained_models", "tracking")
    ...
    ppo.load_checkpoint("trained_models", "tracking", reset_num_timesteps=False); ppo.learn(40)      # src/rl.py's continual training

target_kl is a decision taken on the device (the gate words of include/usim.h): update() still reads the device once, at its end.
"""
import ctypes as C
import io
import math
import time
import zipfile
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .policy import load_sb3_zip, load_vecnormalize_pkl, save_sb3_zip, save_vecnormalize_pkl

# the header's field order (usim_policy_net) as attribute paths of policy.MlpActorCritic
FIELDS = (("pi_w1", "policy_net.0.weight"), ("pi_b1", "policy_net.0.bias"), ("pi_w2", "policy_net.2.weight"), ("pi_b2", "policy_net.2.bias"),
          ("act_w", "action_net.weight"), ("act_b", "action_net.bias"), ("vf_w1", "value_net_body.0.weight"), ("vf_b1", "value_net_body.0.bias"),
          ("vf_w2", "value_net_body.2.weight"), ("vf_b2", "value_net_body.2.bias"), ("val_w", "value_net.weight"), ("val_b", "value_net.bias"),
          ("log_std", "log_std"))
STAT_NAMES = ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss",
              "train/explained_variance")       # the first six: usim_ppo_grad's statistics of the last minibatch; the seventh: usim_explained_variance on the buffer
_SB3_PREFIX = (("mlp_extractor.policy_net.", "policy_net."), ("mlp_extractor.value_net.", "value_net_body."))      # policy.pth's names -> the module's


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


def _field_offsets(act_dim):
    """module path -> (offset, shape) in the flat block"""
    out, o = {}, 0
    for (_, path), shape in zip(FIELDS, _field_shapes(act_dim)):
        out[path] = (o, shape)
        o += math.prod(shape)
    return out


def adam_state_from_flat(exp_avg, exp_avg_sq, step, names, act_dim, lr=3e-4, eps=1e-5):
    """flat Adam moments in FIELDS order + the step count -> the state dict of torch.optim.Adam as `policy.optimizer.pth` of an SB3 checkpoint holds it
    (policy.adam_state_dict shows the layout): CPU tensors per parameter, numbered in the order `names` (module paths in state-dict order).  Device-free when its
    inputs are; step 0 writes a fresh optimizer (empty state), as torch does before the first step."""
    off, state = _field_offsets(act_dim), {}
    if int(step) > 0:
        for i, name in enumerate(names):
            o, shape = off[name]
            cut = lambda t: t[o:o + math.prod(shape)].view(shape).detach().cpu().clone()
            state[i] = {"step": int(step), "exp_avg": cut(exp_avg), "exp_avg_sq": cut(exp_avg_sq)}
    return {"state": state, "param_groups": [{"lr": float(lr), "betas": (0.9, 0.999), "eps": float(eps), "weight_decay": 0, "amsgrad": False,
                                               "params": list(range(len(names)))}]}


def adam_state_to_flat(opt, names, act_dim):
    """the inverse of adam_state_from_flat: -> (exp_avg, exp_avg_sq [ppo_params(act_dim)] float32 CPU tensors in FIELDS order, step).  An empty state gives
    zero moments and step 0; `step` may be an int or a 0-d tensor (newer torch writes tensors).  ValueError: a state that is not one entry per parameter, a
    moment whose shape is not the parameter's, per-parameter steps that differ (the learner keeps ONE step count)."""
    off = _field_offsets(act_dim)
    m, v = torch.zeros(ppo_params(act_dim), dtype=torch.float32), torch.zeros(ppo_params(act_dim), dtype=torch.float32)
    state = opt.get("state", {})
    if len(state) == 0:
        return m, v, 0
    if sorted(state) != list(range(len(names))) or set(names) != set(off):
        raise ValueError(f"optimizer state: {len(state)} entries for the learner's {len(names)} parameters")
    steps = set()
    for i, name in enumerate(names):
        o, shape = off[name]
        st = state[i]
        steps.add(int(st["step"].item()) if torch.is_tensor(st["step"]) else int(st["step"]))
        for key, dst in (("exp_avg", m), ("exp_avg_sq", v)):
            t = torch.as_tensor(st[key])
            if tuple(t.shape) != shape:
                raise ValueError(f"optimizer state: {key} of {name} is {tuple(t.shape)}, the learner's parameter {shape}")
            dst[o:o + math.prod(shape)].copy_(t.detach().to(device="cpu", dtype=torch.float32).reshape(-1))
    if len(steps) != 1:
        raise ValueError(f"optimizer state: per-parameter Adam steps differ ({sorted(steps)}); the learner keeps one step count")
    return m, v, steps.pop()


def state_dict_to_flat(sd, act_dim):
    """policy.pth of an SB3 checkpoint (load_sb3_zip) -> the flat parameter block (float32, CPU); ValueError unless its names and shapes are the learner's"""
    mapped = {}
    for k, t in sd.items():
        for a, b in _SB3_PREFIX:
            k = k.replace(a, b)
        mapped[k] = torch.as_tensor(t)
    off = _field_offsets(act_dim)
    if set(mapped) != set(off):
        raise ValueError(f"checkpoint shapes: parameters {sorted(set(mapped) ^ set(off))} do not match the learner's policy")
    theta = torch.empty(ppo_params(act_dim), dtype=torch.float32)
    for name, (o, shape) in off.items():
        if tuple(mapped[name].shape) != shape:
            raise ValueError(f"checkpoint shapes: {name} is {tuple(mapped[name].shape)}, the learner's {shape}")
        theta[o:o + math.prod(shape)].copy_(mapped[name].detach().to(device="cpu", dtype=torch.float32).reshape(-1))
    return theta


def _positive(name, x):
    """SB3's None or a positive finite number (checked again on every value a schedule returns)"""
    if x is None:
        return None
    x = float(x)
    if not (math.isfinite(x) and x > 0.0):
        raise ValueError(f"{name} must be None or a positive finite number, got {x!r}")
    return x


def _scheduled(name, x):
    """a hyper-parameter that may be a callable of the remaining progress: checked at progress 1 here, and at every later evaluation"""
    if callable(x):
        _positive(name, x(1.0))
        return x
    return _positive(name, x)


class NativePPO:
    """stable-baselines3's PPO update on the library's learner kernels, with SB3's defaults (what src/rl.py:143 runs with): learning_rate 3e-4, n_epochs 10,
    clip_range 0.2, ent_coef 0, vf_coef 0.5, max_grad_norm 0.5, per-minibatch advantage normalisation, Adam(eps 1e-5).

    batch_size=None means one eighth of the rollout (as tools/ppo_demo.py): SB3's default of 64 is a choice for eight environments x 2048 steps and is
    meaningless at 4096 environments -- 8192 minibatches of 64 per epoch would be 8192 launch pairs for what eight do.  learning_rate may be a callable of the
    remaining progress (1 at the start, 0 at the end of learn(): src/rl.py's linear_schedule); outside learn() the progress is 1.  clip_range and clip_range_vf
    may be such callables too.  clip_range_vf=None and target_kl=None are SB3's defaults (no value clipping, no early stop); a non-positive or non-finite value
    of either is refused.  With target_kl set, the minibatch whose approx_kl exceeds 1.5 target_kl is evaluated but not stepped and no later minibatch of the
    update is evaluated at all -- decided on the device by the gate of usim_ppo_grad / usim_ppo_adam_gated, so that update() still reads the device once.

    The policy must be flattened (flatten_parameters) BEFORE a collector that records parameter addresses (policy.FusedRollout) is built; a policy that is
    not flat yet is flattened here when no collector is given.  Refusals are ValueErrors raised before any library call."""

    def __init__(self, env, policy, vecnorm, buffer, collector=None, *, learning_rate=3e-4, n_epochs=10, batch_size=None, clip_range=0.2, ent_coef=0.0,
                 vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True, adam_eps=1e-5, seed=0, clip_range_vf=None, target_kl=None):
        A = _check_shapes(policy)
        clip_range_vf, target_kl = _scheduled("clip_range_vf", clip_range_vf), _positive("target_kl", target_kl)
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
        self.clip_range = clip_range if callable(clip_range) else float(clip_range)
        self.ent_coef, self.vf_coef, self.max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
        self.clip_range_vf, self.target_kl = clip_range_vf, target_kl
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
        self.gate = z(_lib.PPO_GATE_WORDS, torch.int32)                       # stop flag, gradient calls, optimizer steps of the current update(), 0
        self._std = z(1)                                                      # train/std of the last update(): mean(exp(log_std))
        self.last_update = {}                                                 # the logger scalars of the last update() beyond its return value
        self.set_checkpointing(None)                                          # learn(): no periodic save until set_checkpointing(every, ...)
        self.set_evaluation(None)                                             # learn(): no periodic evaluation until set_evaluation(every, eval_env, ...)
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

    def current_clip_range(self):
        c = self.clip_range
        return float(c(self.progress_remaining)) if callable(c) else float(c)

    def current_clip_range_vf(self):
        """SB3's clip_range_vf at the current progress, or None"""
        c = self.clip_range_vf
        return _positive("clip_range_vf", c(self.progress_remaining)) if callable(c) else c

    def minibatch_step(self, data, index, batch, lr=None):
        """one usim_ppo_grad + one usim_ppo_adam_gated on the rows `index` (an int32 device tensor, or None: rows 0 .. batch - 1) of the flattened slices `data` =
        (obs, act, old_logp, adv, ret[, old_values]); the old values are required when clip_range_vf is set.  Both calls stand behind self.gate: the caller clears
        it (update() does, once per update); once a minibatch has tripped target_kl, further calls change nothing."""
        obs, act, lp, adv, ret = data[:5]
        cvf = self.current_clip_range_vf()
        if cvf is not None and len(data) < 6:
            raise ValueError("clip_range_vf needs the buffer's values as the sixth slice of `data`")
        b = _lib.UsimPpoBatch(obs.data_ptr(), act.data_ptr(), lp.data_ptr(), adv.data_ptr(), ret.data_ptr(), None if index is None else index.data_ptr(),
                              obs.shape[0], int(batch), self.act_dim, int(self.normalize_advantage), self.current_clip_range(), self.ent_coef, self.vf_coef, 0.0,
                              data[5].data_ptr() if len(data) > 5 else None, self.gate.data_ptr(), cvf or 0.0, self.target_kl or 0.0)
        stream = self.env._stream()
        self._check(self.lib.usim_ppo_grad(C.byref(self._net), C.byref(b), self._work.data_ptr(), self.grad.data_ptr(), self.stats.data_ptr(), stream))
        self._check(self.lib.usim_ppo_adam_gated(self.theta.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                                 self.step_count.data_ptr(), self.params, self.current_lr() if lr is None else float(lr), 0.9, 0.999,
                                                 self.adam_eps, self.max_grad_norm, self.stats.data_ptr(), self.gate.data_ptr(), stream))

    def update(self):
        """PPO.train on the buffer as it is: n_epochs passes, each a torch.randperm on the device cut into minibatches of batch_size (the trailing partial one
        is used, as in SB3), then the collector's pack().  -> the statistics of the last minibatch under SB3's logger names, and train/explained_variance of the
        buffer's values against its returns as they are BEFORE the first minibatch (SB3's explained_variance; one launch into a device word).  With target_kl
        set, the statistics after an early stop are those of the minibatch that tripped it (later calls leave them alone).  One host read at the end brings
        all of it, the gate and train/std included; self.last_update receives SB3's further logger scalars: train/clip_range, train/clip_range_vf (when set),
        train/std, train/optimizer_steps, train/minibatches_evaluated, train/early_stop."""
        b = self.buffer
        if not b.full:
            raise RuntimeError("rollout buffer is not full")
        values, returns = b.values.contiguous(), b.returns.contiguous()
        self._check(self.lib.usim_explained_variance(values.data_ptr(), returns.data_ptr(), values.numel(), self._ev.data_ptr(), self.env._stream()))
        data = tuple(self._flat(x) for x in (b.observations, b.actions, b.log_probs, b.advantages, b.returns, b.values))
        N, lr, first = self.rollout, self.current_lr(), True
        self.gate.zero_()
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
        torch.mean(torch.exp(self.policy.log_std.detach()), dim=0, keepdim=True, out=self._std)
        s = torch.cat((self.stats, self._ev, self._std, self.gate.to(torch.float32))).tolist()       # one read for all (the gate's counts are far below 2^24)
        n = _lib.PPO_STATS
        stop, evaluated, steps = (int(x) for x in s[n + 2:n + 5])
        cvf = self.current_clip_range_vf()
        self.last_update = {"train/clip_range": self.current_clip_range(), **({} if cvf is None else {"train/clip_range_vf": cvf}), "train/std": s[n + 1],
                            "train/optimizer_steps": steps, "train/minibatches_evaluated": evaluated, "train/early_stop": stop}
        return dict(zip(STAT_NAMES, s[:6] + s[n:n + 1]))

    def set_checkpointing(self, checkpoint_every, checkpoint_dir="./checkpoints", name_prefix="rl_model"):
        """SB3's CheckpointCallback (src/rl.py:133-134) for learn(): with checkpoint_every set, in environment timesteps, learn() writes
        save_checkpoint(checkpoint_dir, f"{name_prefix}_{num_timesteps}_steps") after every iteration in which num_timesteps reaches or passes a further multiple
        of it -- the callback's file names (its save_freq counts vectorised steps, this argument timesteps).  None, the state of a new learner: no periodic save.
        Like the callback it is an object of its own beside learn(), whose signature stays (iterations)."""
        if checkpoint_every is not None and int(checkpoint_every) < 1:
            raise ValueError("checkpoint_every must be None or at least 1 timestep")
        self.checkpoint_every = None if checkpoint_every is None else int(checkpoint_every)
        self.checkpoint_dir, self.name_prefix = checkpoint_dir, str(name_prefix)

    def set_evaluation(self, eval_every, eval_env=None, n_eval_episodes=10, deterministic=True):
        """SB3's EvalCallback (imported at src/rl.py:16) for learn(): with eval_every set, in environment timesteps, learn() runs
        evaluation.evaluate_episodes(eval_env, the live policy, the live vecnorm, n_eval_episodes, deterministic) after every iteration in which num_timesteps
        reaches or passes a further multiple of it, and puts eval/mean_reward, eval/mean_ep_length and the thirteen eval/<metric> means into that iteration's
        history row.  The statistics of vecnorm are frozen and only read during an evaluation (EvalCallback's sync_envs_normalization: the evaluation sees the
        training statistics as they are).  eval_env must be an environment other than the training one -- an evaluation resets its env -- with the same
        action_dim, on the same device: ValueError otherwise.  None, the state of a new learner: no evaluation, learn() behaves exactly as before."""
        if eval_every is None:
            self.eval_every, self.eval_env = None, None
            return
        if int(eval_every) < 1:
            raise ValueError("eval_every must be None or at least 1 timestep")
        if int(n_eval_episodes) < 1:
            raise ValueError("n_eval_episodes must be at least 1")
        if eval_env is None or eval_env is self.env:
            raise ValueError("eval_env must be an environment other than the training one: an evaluation resets it")
        if int(eval_env.action_dim) != self.act_dim or torch.device(eval_env.device) != torch.device(self.env.device):
            raise ValueError(f"eval_env has action_dim {eval_env.action_dim} on {eval_env.device}, the training env {self.act_dim} on {self.env.device}")
        self.eval_every, self.eval_env = int(eval_every), eval_env
        self.n_eval_episodes, self.eval_deterministic = int(n_eval_episodes), bool(deterministic)

    def evaluate(self):
        """one evaluation as learn() runs it -> (the eval/* scalars of a history row, the result of evaluation.evaluate_episodes)"""
        from .evaluation import evaluate_episodes
        if self.eval_every is None:
            raise ValueError("set_evaluation(eval_every, eval_env, ...) first")
        res = evaluate_episodes(self.eval_env, self.policy, self.vecnorm, n_eval_episodes=self.n_eval_episodes, deterministic=self.eval_deterministic)
        row = {"eval/mean_reward": res["mean"], "eval/mean_ep_length": float(np.mean(res["lengths"]))}
        row.update({f"eval/{name}": float(np.mean(v)) for name, v in res["metrics"].items()})
        return row, res

    def learn(self, iterations):
        """`iterations` x (collector.collect(), update()); -> the statistics of the last update.  Every iteration appends one dict to self.history -- SB3's logger
        scalars: time/total_timesteps (environment steps collected by learn() so far), time/wall (time.time()), the train/* statistics of update() and of
        self.last_update, train/learning_rate and, when the env has a monitor attached (env.attach_monitor, before the collector was built), its summary():
        rollout/ep_rew_mean, rollout/ep_len_mean, ... -- the series monitor.write_scalar_csv writes out.  After set_checkpointing(every, ...) it also writes
        the periodic checkpoints, after set_evaluation(every, eval_env, ...) it also runs the periodic evaluations (eval/* scalars in the rows of those
        iterations); without, it behaves exactly as before."""
        if self.collector is None:
            raise ValueError("learn() needs a collector")
        every, out = self.checkpoint_every, None
        for it in range(int(iterations)):
            self.progress_remaining = 1.0 - it / float(iterations)
            lr = self.current_lr()
            self.collector.collect()
            out = self.update()
            before = self.num_timesteps
            self.num_timesteps += self.rollout
            row = {"time/total_timesteps": self.num_timesteps, "time/wall": time.time(), **out, "train/learning_rate": lr, **self.last_update}
            mon = getattr(self.env, "monitor", None)
            if mon is not None:
                row.update(mon.summary())
            if self.eval_every is not None and self.num_timesteps // self.eval_every > before // self.eval_every:
                row.update(self.evaluate()[0])
            self.history.append(row)
            if every is not None and self.num_timesteps // every > before // every:
                self.save_checkpoint(self.checkpoint_dir, f"{self.name_prefix}_{self.num_timesteps}_steps")
        self.progress_remaining = 1.0
        return out

    def adam_state_dict(self):
        """the learner's Adam state as `policy.optimizer.pth` of an SB3 checkpoint (policy.adam_state_dict shows the layout): moments per parameter in
        state-dict order, CPU tensors"""
        return adam_state_from_flat(self.exp_avg, self.exp_avg_sq, int(self.step_count.item()), list(self.policy.state_dict()), self.act_dim,
                                    self.current_lr(), self.adam_eps)

    def save(self, path, data=None):
        """the checkpoint zip of PPO.save (policy.save_sb3_zip) with the Adam moments"""
        save_sb3_zip(path, self.policy, data=data, optimizer_state=self.adam_state_dict())

    def checkpoint_data(self):
        """the `data` json of a checkpoint this learner writes: what save_sb3_zip writes by default, num_timesteps and the numeric hyper-parameters in force"""
        b, p = self.buffer, self.policy
        return {"gamma": b.gamma, "gae_lambda": b.gae_lambda, "n_steps": b.buffer_size, "n_envs": b.n_envs,
                "policy_kwargs": {"activation_fn": "tanh", "net_arch": [{"pi": list(p.pi_sizes), "vf": list(p.vf_sizes)}]},
                "num_timesteps": int(self.num_timesteps), "n_epochs": self.n_epochs, "batch_size": self.batch_size, "learning_rate": self.current_lr(),
                "clip_range": self.current_clip_range(), "clip_range_vf": self.current_clip_range_vf(), "target_kl": self.target_kl,
                "ent_coef": self.ent_coef, "vf_coef": self.vf_coef, "max_grad_norm": self.max_grad_norm}

    def save_checkpoint(self, folder, name):
        """folder/name.zip (save(), with checkpoint_data()) and folder/vec_normalize_<name>.pkl (policy.save_vecnormalize_pkl): the pair src/rl.py:119-120
        names and :166-167 writes.  -> (zip path, pkl path)"""
        folder = Path(folder)
        folder.mkdir(parents=True, exist_ok=True)
        zip_path, pkl_path = folder / f"{name}.zip", folder / f"vec_normalize_{name}.pkl"
        self.save(zip_path, data=self.checkpoint_data())
        space = self.env.action_space
        save_vecnormalize_pkl(pkl_path, self.vecnorm.stats(), self.buffer.n_envs, space.low, space.high, training=self.vecnorm.training,
                              norm_reward=self.vecnorm.norm_reward)
        return zip_path, pkl_path

    def load_checkpoint(self, folder, name, reset_num_timesteps=True):
        """PPO.load + VecNormalize.load of src/rl.py:151-160 on a learner that exists: folder/name.zip and folder/vec_normalize_<name>.pkl are restored IN
        PLACE -- the flat parameter block, exp_avg, exp_avg_sq, step_count and every tensor of the DeviceVecNormalize (observation and return statistics, both
        counts) keep their addresses, so a collector or graph recorded earlier goes on working; the collector's pack() runs afterwards.  vecnorm.returns is
        zeroed, as VecNormalize.load -> set_venv does.  num_timesteps is restored only with reset_num_timesteps=False (rl.py:163); the hyper-parameters stay
        the learner's.  ValueError, before anything is written: a checkpoint whose shapes are not the learner's, per-parameter Adam steps that differ,
        VecNormalize constants (clip_obs, clip_reward, gamma, epsilon) that are not the learner's.  A fresh optimizer in the file (step 0) gives zero moments.

        NOT restored, as in the reference: the environments' state (the next collect() goes on from where this process's environments are), the minibatch
        generator, the collector's noise counters.  -> the checkpoint's data dict"""
        folder = Path(folder)
        zip_path = folder / f"{name}.zip"
        sd, data = load_sb3_zip(zip_path)
        with zipfile.ZipFile(zip_path) as z:
            opt = torch.load(io.BytesIO(z.read("policy.optimizer.pth")), map_location="cpu", weights_only=True)
        theta = state_dict_to_flat(sd, self.act_dim)
        m, v, step = adam_state_to_flat(opt, list(self.policy.state_dict()), self.act_dim)
        st, vn = load_vecnormalize_pkl(folder / f"vec_normalize_{name}.pkl"), self.vecnorm
        if len(st["obs_mean"]) != vn.obs_mean.numel() or len(st["obs_var"]) != vn.obs_var.numel():
            raise ValueError(f"checkpoint shapes: VecNormalize statistics of {len(st['obs_mean'])} observations, the learner's {vn.obs_mean.numel()}")
        for key in ("clip_obs", "clip_reward", "gamma", "epsilon"):
            if float(st[key]) != float(getattr(vn, key)):
                raise ValueError(f"checkpoint VecNormalize {key} {st[key]!r} is not the learner's {getattr(vn, key)!r}")
        with torch.no_grad():
            self.theta.copy_(theta); self.exp_avg.copy_(m); self.exp_avg_sq.copy_(v); self.step_count.fill_(step)
            vn.obs_mean.copy_(torch.as_tensor(st["obs_mean"], dtype=torch.float64)); vn.obs_var.copy_(torch.as_tensor(st["obs_var"], dtype=torch.float64))
            vn._obs_count.fill_(float(st["count"])); vn._ret_count.fill_(float(st["ret_count"]))
            vn.ret_mean.fill_(float(st["ret_mean"])); vn.ret_var.fill_(float(st["ret_var"]))
            vn.returns.zero_()
        if self.collector is not None and hasattr(self.collector, "pack"):
            self.collector.pack()
        if not reset_num_timesteps:
            self.num_timesteps = int(data.get("num_timesteps", 0))
        return data
