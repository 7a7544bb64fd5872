"""Behaviour cloning and DAgger on the device: what the `imitation` package offers users of stable-baselines3 (bc.BC, dagger.SimpleDAggerTrainer), with the
minibatch loss and gradient as one library call -- usim_bc_grad (include/usim.h; csrc/usim_ppo.hip: further instances of the PPO gradient kernel) -- and the
optimiser step as usim_ppo_adam on the flat parameter block of learner.flatten_parameters; the block, that step and the epoch loop are learner.FlatLearner's, the
core ppo.NativePPO stands on as well.  It connects the pieces that stand beside each other: a planner
(planner.MPPIPlanner) or a shipped checkpoint becomes a network that costs one forward pass per decision, with a critic where the expert has one, and
ppo.NativePPO built afterwards on the same policy continues from the same words.

    student = MlpActorCritic(19, env.action_dim).to(env.device)
    trainer = distill(env, teacher, teacher_vecnorm, student, rounds=4, rollout_steps=64)          # PolicyExpert + NativeBC + DAggerTrainer
    ...
    demos = DemoBuffer(rounds * G * steps, A, dev)
    learner = NativeBC(student, vecnorm, demos, loss="mse")
    trainer = DAggerTrainer(planner.real, PlannerExpert(planner), learner, rollout_steps=steps)
    for _ in range(rounds): trainer.round()

An expert is any object with label(obs_raw [n, 19]) -> (act [n, A], value [n] or None); two optional hooks: check_env(env) (ValueError where the expert cannot
label that environment) and after_step(done) (the done flags of the step the trainer has just taken)."""
import ctypes as C

import torch

from . import _lib
from .learner import FlatLearner, _check_shapes
from .policy import DeviceVecNormalize

LOSSES = {"nll": _lib.BC_NLL, "mse": _lib.BC_MSE}
STAT_NAMES = ("bc/loss", "bc/neglogp", "bc/action_mse", "bc/value_loss", "bc/entropy_loss", "bc/grad_norm", "bc/optimizer_steps")
ROUND_NAMES = ("dagger/round", "dagger/beta", "dagger/rows", "dagger/expert_share")


class DemoBuffer:
    """A ring on the device of raw observations [capacity, obs_dim], expert actions [capacity, act_dim] and optional value targets [capacity].  add() appends
    n rows in environment order and, when the ring is full, overwrites the oldest; the write position is host arithmetic (n is known), so adding never reads the
    device.  `rows`: rows held (at most capacity).  `has_value`: every row since the last clear() came with a value target (None while empty); a buffer takes
    values with all of its rows or with none -- ValueError otherwise.  ordered() returns the rows oldest first."""

    def __init__(self, capacity, act_dim, device, obs_dim=19):
        if int(capacity) < 1 or int(act_dim) < 1 or int(obs_dim) < 1:
            raise ValueError(f"capacity, act_dim and obs_dim must be at least 1, got {capacity!r}, {act_dim!r}, {obs_dim!r}")
        self.capacity, self.act_dim, self.obs_dim, self.device = int(capacity), int(act_dim), int(obs_dim), torch.device(device)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.obs, self.act, self.value = z(self.capacity, self.obs_dim), z(self.capacity, self.act_dim), z(self.capacity)
        self.clear()

    def clear(self):
        self.rows, self.pos, self.total, self.has_value = 0, 0, 0, None

    def add(self, obs, act, value=None):
        n = int(obs.shape[0])
        if tuple(obs.shape) != (n, self.obs_dim) or tuple(act.shape) != (n, self.act_dim) or (value is not None and tuple(value.shape) != (n,)):
            raise ValueError(f"add: obs [n, {self.obs_dim}], act [n, {self.act_dim}] and value [n] or None, got {tuple(obs.shape)}, {tuple(act.shape)}, "
                             f"{None if value is None else tuple(value.shape)}")
        if self.has_value is not None and self.has_value != (value is not None):
            raise ValueError("add: a buffer holds value targets for all of its rows or for none")
        if n == 0:
            return
        self.has_value = value is not None
        skip = max(0, n - self.capacity)                                       # more rows than the ring holds: the last `capacity` of them stay
        pos, cap = (self.pos + skip) % self.capacity, self.capacity
        for dst, src in ((self.obs, obs), (self.act, act)) + (((self.value, value),) if value is not None else ()):
            src = src[skip:]
            head = min(n - skip, cap - pos)
            dst[pos:pos + head].copy_(src[:head])
            if head < n - skip:
                dst[:n - skip - head].copy_(src[head:])
        self.pos, self.total = (self.pos + n) % cap, self.total + n
        self.rows = min(self.total, cap)

    def add_block(self, obs, act, value=None):
        """add() step by step: obs [T, n, obs_dim], act [T, n, act_dim], value [T, n] or None"""
        for t in range(int(obs.shape[0])):
            self.add(obs[t], act[t], None if value is None else value[t])

    def ordered(self):
        """(obs, act, value or None) of the rows held, oldest first (copies when the ring has wrapped)"""
        if self.total <= self.capacity:
            sl = lambda x: x[:self.rows]
        else:
            sl = lambda x: torch.cat((x[self.pos:], x[:self.pos]))
        return sl(self.obs), sl(self.act), (sl(self.value) if self.has_value else None)


class NativeBC(FlatLearner):
    """Behaviour cloning of the rows of a DemoBuffer into a policy.MlpActorCritic (19 -> 256 -> 128, A <= 8): per minibatch one usim_bc_grad and one
    usim_ppo_adam.  loss: "nll" (-log-prob of the expert's action: imitation's BC, trains log_std too) or "mse" (squared error of the mean; log_std then moves
    by the entropy term alone).  vf_coef > 0 with value targets in the buffer also regresses the critic on them; a buffer without value targets has no value
    term, whatever vf_coef says.  batch_size=None: one eighth of the buffer's rows at train() time.

    The policy is flattened (learner.flatten_parameters) if it is not flat yet -- as with ppo.NativePPO, BEFORE any collector that records parameter addresses
    (policy.FusedRollout) is built; a NativePPO constructed afterwards on the same policy trains the same words.  `vecnorm` is only read: train() normalises
    with its statistics as they are and never updates them; fit_normalizer() sets them from the buffer for demonstrations that come without statistics.
    Refusals are ValueErrors raised before any library call."""

    def __init__(self, policy, vecnorm, demos, *, loss="nll", learning_rate=3e-4, batch_size=None, n_epochs=1, ent_coef=1e-3, vf_coef=0.5, max_grad_norm=0.5,
                 adam_eps=1e-5, seed=0):
        A = _check_shapes(policy)
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {sorted(LOSSES)}, got {loss!r}")
        if A != int(demos.act_dim):
            raise ValueError(f"policy shapes: act_dim {A} is not the buffer's {demos.act_dim}")
        if int(demos.obs_dim) != _lib.OBS_DIM:
            raise ValueError(f"the buffer holds observations of {demos.obs_dim} words, the policy reads {_lib.OBS_DIM}")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError(f"batch_size {batch_size} outside 1 .. the buffer's rows")
        super().__init__(policy, A, demos.device, "buffer", demos.capacity, n_epochs=n_epochs, max_grad_norm=max_grad_norm, adam_eps=adam_eps, seed=seed)
        self.vecnorm, self.demos, self.loss = vecnorm, demos, loss
        self.learning_rate, self.batch_size = float(learning_rate), None if batch_size is None else int(batch_size)
        self.ent_coef, self.vf_coef = float(ent_coef), float(vf_coef)
        self.first_minibatch = {}                                             # first_stats under the names of train()'s result
        self.last_extra = []
        self.history = []

    def minibatch_step(self, data, index, batch, lr=None):
        """one usim_bc_grad + one usim_ppo_adam on the rows `index` (an int32 device tensor, or None: rows 0 .. batch - 1) of `data` = (normalised observations
        [rows, 19], expert actions [rows, A][, value targets [rows]]), contiguous float32 device tensors"""
        obs, act = data[:2]
        value = data[2] if len(data) > 2 else None
        b = _lib.UsimBcBatch(obs.data_ptr(), act.data_ptr(), None if value is None else value.data_ptr(), None if index is None else index.data_ptr(),
                             obs.shape[0], int(batch), self.act_dim, LOSSES[self.loss], self.ent_coef, self.vf_coef)
        self._check(self.lib.usim_bc_grad(C.byref(self._net), C.byref(b), self._work.data_ptr(), self.grad.data_ptr(), self.stats.data_ptr(), self._stream()))
        self.adam_step(self.learning_rate if lr is None else lr)

    def _named(self, s, steps):
        return dict(zip(STAT_NAMES, (s[5], -s[4], s[3], s[1], s[2], s[6], steps)))

    def train(self, extra=None):
        """n_epochs passes over the buffer's rows: the observations normalised once with vecnorm's statistics as they are, per pass a torch.randperm on the
        device cut into minibatches (the trailing partial one is used).  One host read at the end brings the statistics of the last minibatch (and of the first,
        into self.first_minibatch; and `extra`, a float device tensor of the caller's, into self.last_extra).  -> bc/loss, bc/neglogp, bc/action_mse,
        bc/value_loss, bc/entropy_loss, bc/grad_norm of the last minibatch and bc/optimizer_steps, the steps of this call; the dict is appended to history."""
        d = self.demos
        N = int(d.rows)
        if N < 1:
            raise ValueError("the demonstration buffer is empty")
        batch = N // 8 if self.batch_size is None else self.batch_size
        if not 1 <= batch <= N:
            raise ValueError(f"batch_size {batch} outside 1 .. the buffer's {N} rows")
        data = (self.vecnorm.normalize_obs(d.obs[:N], update=False).contiguous(), d.act[:N]) + ((d.value[:N],) if d.has_value and self.vf_coef != 0.0 else ())
        steps = self.run_epochs(N, batch, lambda index, n: self.minibatch_step(data, index, n))
        parts = (self.stats, self.first_stats) + (() if extra is None else (extra.reshape(-1).to(torch.float32),))
        s = torch.cat(parts).tolist()                                          # the one read
        n = _lib.PPO_STATS
        out, self.first_minibatch, self.last_extra = self._named(s[:n], steps), self._named(s[n:2 * n], steps), s[2 * n:]
        self.history.append(out)
        return out

    def fit_normalizer(self):
        """set vecnorm's observation mean, variance and count from the buffer's raw observations (float64; the count is the rows), in place"""
        N = int(self.demos.rows)
        if N < 1:
            raise ValueError("the demonstration buffer is empty")
        o = self.demos.obs[:N].to(torch.float64)
        vn = self.vecnorm
        vn.obs_mean.copy_(o.mean(0)); vn.obs_var.copy_(o.var(0, unbiased=False)); vn._obs_count.fill_(float(N))


class PolicyExpert:
    """A trained policy.MlpActorCritic as the expert: the deterministic mean clipped to the action box (what PPO.predict hands the environment) and the critic's
    value, both under the expert's own statistics `vecnorm`, which are only read."""

    def __init__(self, policy, vecnorm, low, high):
        dev = next(policy.parameters()).device
        self.policy, self.vecnorm = policy, vecnorm
        self.low, self.high = (torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous() for x in (low, high))

    @torch.no_grad()
    def label(self, obs_raw):
        mean, value = self.policy.forward(self.vecnorm.normalize_obs(obs_raw, update=False))
        return torch.max(torch.min(mean, self.high), self.low), value


class PlannerExpert:
    """planner.MPPIPlanner as the expert: label() is the first action of planner.plan() -- the plan from the present state of planner.real, whatever
    observations are passed -- so it labels the environment planner.real and no other (check_env).  No value targets.  The trainer steps the environment, not
    the planner; after_step hands the planner the done flags as the restart flags of its next plan, as MPPIPlanner.step does."""

    def __init__(self, planner):
        self.planner = planner

    def check_env(self, env):
        if env is not self.planner.real:
            raise ValueError("a PlannerExpert labels the states of planner.real: the DAgger environment must be that environment")

    def label(self, obs_raw):
        if int(obs_raw.shape[0]) != int(self.planner.groups):
            raise ValueError(f"a PlannerExpert labels the {self.planner.groups} environments of planner.real, got {int(obs_raw.shape[0])} observations")
        return self.planner.plan(), None

    def after_step(self, done):
        self.planner.restart.copy_(done)


def _default_beta(round_index):
    return 1.0 if round_index == 0 else 0.0


class DAggerTrainer:
    """DAgger (Ross et al. 2011) around a NativeBC learner: round() rolls `rollout_steps` steps of env.step_tensor (auto-reset on) in which every environment
    acts with the expert's label with probability beta(round) -- drawn per environment and step from a seeded device generator -- and with the student's action
    under the learner's vecnorm otherwise; EVERY visited observation goes into the learner's DemoBuffer with the expert's label, whoever acted; then
    learner.train().  The first round starts from env.reset_tensor(), later rounds continue where the environments are.  Nothing in a round reads the device but
    train()'s one read.  -> the learner's scalars plus dagger/round, dagger/beta, dagger/rows (the buffer's) and dagger/expert_share (the share of this round's
    environment steps the expert acted in); the dict is appended to history.  ValueError before anything runs: rollout_steps < 1, an expert without label(), an
    environment the expert refuses, an act_dim or device that is not the learner's, a buffer too small for one round, a beta outside [0, 1]."""

    def __init__(self, env, expert, learner, *, rollout_steps, beta=_default_beta, student_deterministic=True, seed=0):
        if int(rollout_steps) < 1:
            raise ValueError("rollout_steps must be at least 1")
        if not callable(getattr(expert, "label", None)):
            raise ValueError("an expert has label(obs_raw [n, 19]) -> (act [n, A], value [n] or None)")
        if not callable(beta):
            raise ValueError("beta must be a callable of the round number")
        if hasattr(expert, "check_env"):
            expert.check_env(env)
        if int(env.action_dim) != int(learner.act_dim):
            raise ValueError(f"the environment has action_dim {env.action_dim}, the learner's policy {learner.act_dim}")
        if torch.device(env.device) != torch.device(learner.device):
            raise ValueError(f"the environment is on device {env.device}, the learner on {learner.device}")
        if int(learner.demos.capacity) < int(env.num_envs) * int(rollout_steps):
            raise ValueError(f"the buffer's capacity {learner.demos.capacity} is below one round's {int(env.num_envs) * int(rollout_steps)} rows")
        self.env, self.expert, self.learner, self.rollout_steps, self.beta = env, expert, learner, int(rollout_steps), beta
        self.student_deterministic, self.round_index, self.history = bool(student_deterministic), 0, []
        dev = torch.device(env.device)
        self.low, self.high = (torch.as_tensor(x, dtype=torch.float32, device=dev) for x in (env.action_space.low, env.action_space.high))
        self.generator = torch.Generator(device=dev)
        self.generator.manual_seed(int(seed))
        self._share = torch.zeros(1, dtype=torch.float32, device=dev)
        self._obs = None

    @torch.no_grad()
    def student_action(self, obs_raw):
        """the student's action on raw observations: the learner's policy under the learner's vecnorm (frozen), clipped to the action box"""
        L = self.learner
        return L.policy.predict(L.vecnorm.normalize_obs(obs_raw, update=False), self.student_deterministic, self.low, self.high, self.generator)

    def round(self):
        beta = float(self.beta(self.round_index))
        if not 0.0 <= beta <= 1.0:
            raise ValueError(f"beta({self.round_index}) = {beta!r} outside [0, 1]")
        env, n = self.env, int(self.env.num_envs)
        obs = env.reset_tensor() if self._obs is None else self._obs
        self._share.zero_()
        for _ in range(self.rollout_steps):
            raw = obs.clone()                                                 # (the environment overwrites its observation tensor with every step)
            e_act, e_val = self.expert.label(raw)
            expert_acts = torch.rand(n, device=raw.device, generator=self.generator) < beta
            act = e_act if beta >= 1.0 else torch.where(expert_acts[:, None], e_act, self.student_action(raw))
            self.learner.demos.add(raw, e_act, e_val)
            self._share.add_(expert_acts.sum())
            obs, _, done = env.step_tensor(act.contiguous())
            if hasattr(self.expert, "after_step"):
                self.expert.after_step(done)
        self._obs = obs
        out = self.learner.train(extra=self._share)
        row = {**out, "dagger/round": self.round_index, "dagger/beta": beta, "dagger/rows": int(self.learner.demos.rows),
               "dagger/expert_share": self.learner.last_extra[0] / (n * self.rollout_steps)}
        self.history.append(row)
        self.round_index += 1
        return row


def distill(env, teacher_policy, teacher_vecnorm, student_policy, rounds, rollout_steps, **bc_kwargs):
    """Distil a trained policy into `student_policy` on `env`: `rounds` DAgger rounds of `rollout_steps` steps with PolicyExpert(teacher) and a NativeBC
    learner whose buffer holds every round.  The student's DeviceVecNormalize is built from the teacher's statistics, frozen (from_stats(training=False)), so
    the student reads what the teacher reads and its critic is regressed on the teacher's values in the teacher's units.  bc_kwargs go to NativeBC, but
    beta, student_deterministic (DAggerTrainer's) and capacity (the buffer's, default rounds x env.num_envs x rollout_steps).  -> the DAggerTrainer (its
    learner, the learner's vecnorm and the history hang on it)."""
    n, dev = int(env.num_envs), torch.device(env.device)
    trainer_kw = {k: bc_kwargs.pop(k) for k in ("beta", "student_deterministic") if k in bc_kwargs}
    capacity = int(bc_kwargs.pop("capacity", int(rounds) * n * int(rollout_steps)))
    vecnorm = DeviceVecNormalize.from_stats(teacher_vecnorm.stats(), n, device=dev, training=False, norm_reward=teacher_vecnorm.norm_reward)
    demos = DemoBuffer(capacity, int(env.action_dim), dev)
    learner = NativeBC(student_policy, vecnorm, demos, **bc_kwargs)
    expert = PolicyExpert(teacher_policy, teacher_vecnorm, env.action_space.low, env.action_space.high)
    trainer = DAggerTrainer(env, expert, learner, rollout_steps=rollout_steps, seed=bc_kwargs.get("seed", 0), **trainer_kw)
    for _ in range(int(rounds)):
        trainer.round()
    return trainer
