"""The PPO learner on the device: stable-baselines3's `PPO.train` (the `model.learn` of src/rl.py:143) as two library calls per minibatch -- usim_ppo_grad (loss,
statistics and the gradient for every parameter of the shipped MlpPolicy) and usim_ppo_adam (clip_grad_norm_ + Adam.step) on ONE flat parameter block
(include/usim.h; csrc/usim_ppo.hip).  The block, the Adam call and the epoch loop are learner.py's (FlatLearner, shared with imitation.NativeBC).  The collector
(policy.FusedRollout), the running statistics (policy.DeviceVecNormalize), the buffer (policy.DeviceRolloutBuffer) and the checkpoint writer (policy.save_sb3_zip)
are the ones of policy.py: the module's parameters become views into the flat block, so all of them keep working on the same memory.

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
# (the flat block's functions are learner.py's; they stay available under the names this module has always offered)
from .learner import FIELDS, FlatLearner, _check_shapes, _field_shapes, _is_flat, adam_state_from_flat, adam_state_to_flat  # noqa: F401
from .learner import flatten_parameters, ppo_params, state_dict_to_flat  # noqa: F401
from .policy import load_sb3_zip, load_vecnormalize_pkl, save_sb3_zip, save_vecnormalize_pkl

STAT_NAMES = ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss",
              "train/explained_variance")       # the first six: usim_ppo_grad's statistics of the last minibatch; the seventh: usim_explained_variance on the buffer


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


class NativePPO(FlatLearner):
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
        super().__init__(policy, A, dev, "environment", rollout, n_epochs=n_epochs, max_grad_norm=max_grad_norm, adam_eps=adam_eps, seed=seed, collector=collector)
        self.env, self.vecnorm, self.buffer, self.collector = env, vecnorm, buffer, collector
        self.learning_rate, self.batch_size, self.rollout = learning_rate, batch_size, rollout
        self.clip_range = clip_range if callable(clip_range) else float(clip_range)
        self.ent_coef, self.vf_coef, self.normalize_advantage = float(ent_coef), float(vf_coef), bool(normalize_advantage)
        self.clip_range_vf, self.target_kl, self.progress_remaining = clip_range_vf, target_kl, 1.0
        z = lambda n, dtype=torch.float32: torch.zeros(n, dtype=dtype, device=dev)
        self._ev = z(1)                                                       # train/explained_variance of the last update() (usim_explained_variance)
        self.gate = z(_lib.PPO_GATE_WORDS, torch.int32)                       # stop flag, gradient calls, optimizer steps of the current update(), 0
        self._std = z(1)                                                      # train/std of the last update(): mean(exp(log_std))
        self.last_update = {}                                                 # the logger scalars of the last update() beyond its return value
        self.set_checkpointing(None)                                          # learn(): no periodic save until set_checkpointing(every, ...)
        self.set_evaluation(None)                                             # learn(): no periodic evaluation until set_evaluation(every, eval_env, ...)
        self.history = []                                                     # learn(): one dict of logger scalars per iteration
        self.num_timesteps = 0                                                # environment steps collected by learn() so far

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
        self._check(self.lib.usim_ppo_grad(C.byref(self._net), C.byref(b), self._work.data_ptr(), self.grad.data_ptr(), self.stats.data_ptr(), self._stream()))
        self.adam_step(self.current_lr() if lr is None else lr, self.gate)

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
        self._check(self.lib.usim_explained_variance(values.data_ptr(), returns.data_ptr(), values.numel(), self._ev.data_ptr(), self._stream()))
        data = tuple(self._flat(x) for x in (b.observations, b.actions, b.log_probs, b.advantages, b.returns, b.values))
        lr = self.current_lr()
        self.gate.zero_()
        self.run_epochs(self.rollout, self.batch_size, lambda index, n: self.minibatch_step(data, index, n, lr))
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
