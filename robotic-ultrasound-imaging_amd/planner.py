"""A batched MPPI shooting planner on the device: a model-predictive baseline next to the reference's PPO policies.

`MPPIPlanner(real, sim, ...)` controls the G environments of `real` with the n = G K environments of `sim`: environments [g K, (g + 1) K) of `sim` play the K
candidate action sequences of real environment g, candidate 0 being the unperturbed nominal.  A planning step is six launches and no host work in between --
save the real states, load them into their groups, sample the candidates around the nominal (usim_plan_sample), play them (usim_rollout_actions), score them
(usim_score_block), and form the exponentially weighted plan, the action and the shifted nominal of the next step (usim_plan_update; csrc/usim_plan.hip).  Every
buffer is allocated once, so a whole step() -- plan, the real step, the restart flags -- is recordable as one HIP graph.

Three options, all off by default, let a trained network guide the planner (include/usim.h "the guided planner"): `critic` adds the value of the state behind the
horizon to every surviving candidate's return (usim_policy_step on the last observations, usim_score_block_tail); `tail_action` makes the actor's action there the
last step of the next nominal (usim_plan_tail); `iterations` > 1 refines the sampling distribution inside a control step by cross-entropy refits on the elite
candidates (usim_plan_sample_elem, usim_plan_refit).  Still launches only, on buffers allocated once."""
import ctypes as C
import math

import torch

from . import _lib
from .policy import _capture, policy_net


class MPPIPlanner:
    """pl = MPPIPlanner(real, sim, horizon=16, sigma=0.3, temperature=1.0)
       act = pl.plan()              # [G, A] device tensor; real is not modified
       obs, rew, done = pl.step()   # plan(), real.step_tensor(act), done remembered as the restart flags of the next plan
       pl.record(); pl.replay()     # one HIP graph of a whole step()

    real, sim: two UltrasoundVecEnv of one configuration on one device, sim.num_envs a multiple of real.num_envs (the caller resets `real`; the state of `sim` is
    overwritten by every plan).  sigma: the standard deviation of the candidates' noise, a number or one per action component.  temperature: of the exponential
    weights, in units of return; 0 selects the best candidate.  gamma: the discount of the candidates' returns.  smoothing in [0, 1): first-order correlation of the
    noise along the horizon.  seed: key of the noise stream; a draw is keyed (seed, noise counter, candidate, step, component).

    After a plan(): `candidates` [H, n, A], `returns` [n] (each candidate's own episode, up to and including its first done), `lengths` [n], `weights` [n],
    `best` [G] (int32, index inside the group), `plan_actions` [G, H, A], `action` [G, A]; `mean` [G, H, A] already holds the nominal of the NEXT plan (the plan
    shifted by one step); `block` is the rollout block the candidates were played into (obs [H, n, 19], rew and done [H, n]).  All are device tensors that the next
    plan overwrites.  `restart` [G] (uint8) are the flags the next plan reads: where non-zero the group is sampled around zero and its nominal is zeroed.  `noise_counter` (int32 [1], device) is advanced by every plan; set it to repeat a sequence of draws.

    critic=(policy, vecnorm): a policy.MlpActorCritic and its policy.DeviceVecNormalize (statistics read, never updated).  After the candidates are played the
    network is evaluated on their last observations (`tail_value` [n], `tail_policy_action` [n, A]: the clipped mean action) and a candidate that played all H steps
    without a done earns gamma^H * s * value on top, s = sqrt(ret_var + epsilon) where vecnorm.norm_reward (the critic then speaks in normalised returns), else 1.
    `gamma` must be the statistics' gamma: the value is that of a return discounted so.  tail_action=True (needs critic): the last step of the next nominal is the
    weighted mean of the actor's actions behind the horizon (a candidate that ended keeps its own last action) instead of a repeat of the plan's last action.
    iterations=R > 1: R - 1 rounds of load, sample, play, score, refit before the final round that ends in the update; a refit moves `mean` to the mean of the
    `elites` best candidates of each group (default K // 8, at least 1) and `sigma_elem` [G, H, A], which restarts from `sigma` at every plan, to their standard
    deviation, both blended with `momentum` in [0, 1) of the old and with `sigma_min` as sigma's floor; `elite` [G, elites] (int32, -1 padded) is the last
    refit's set.  Every round advances `noise_counter`, so a plan advances it by R."""

    def __init__(self, real, sim, horizon=16, sigma=0.3, temperature=1.0, gamma=1.0, smoothing=0.0, seed=0, critic=None, tail_action=False, iterations=1,
                 elites=None, momentum=0.0, sigma_min=1e-3):
        G, n = int(real.num_envs), int(sim.num_envs)
        if G <= 0 or n <= 0 or n % G != 0:
            raise ValueError(f"sim.num_envs must be a positive multiple of real.num_envs, got {n} and {G}")
        for name in ("snapshot_words", "action_dim"):
            if getattr(real, name) != getattr(sim, name):
                raise ValueError(f"real and sim differ in {name}: {getattr(real, name)} and {getattr(sim, name)}")
        if real._kwargs != sim._kwargs:
            raise ValueError("real and sim must be built with the same robosuite kwargs (a snapshot row is loaded across them)")
        if real.device != sim.device:
            raise ValueError(f"real and sim must be on one device, got {real.device} and {sim.device}")
        A, H = int(real.action_dim), int(horizon)
        sig = [float(sigma)] * A if isinstance(sigma, (int, float)) else [float(s) for s in sigma]
        if len(sig) != A or not all(math.isfinite(s) and s > 0.0 for s in sig):
            raise ValueError(f"sigma must be a positive number or {A} of them, got {sigma!r}")
        if H < 1:
            raise ValueError(f"horizon must be at least 1, got {horizon}")
        if not (math.isfinite(temperature) and temperature >= 0.0):
            raise ValueError(f"temperature must be finite and not negative, got {temperature}")
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"smoothing must lie in [0, 1), got {smoothing}")
        K, R = n // G, int(iterations)
        if tail_action and critic is None:
            raise ValueError("tail_action needs critic=(policy, vecnorm): the actor's action behind the horizon comes from the critic's launch")
        if critic is not None and float(critic[1].gamma) != float(gamma):
            raise ValueError(f"gamma {gamma} differs from the gamma {critic[1].gamma} of the critic's statistics: its value is that of another return")
        if R < 1:
            raise ValueError(f"iterations must be at least 1, got {iterations}")
        E = max(1, K // 8) if elites is None else int(elites)
        if not 1 <= E <= K:
            raise ValueError(f"elites must lie in 1 .. {K} (the candidates of a group), got {elites}")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"momentum must lie in [0, 1), got {momentum}")
        if not (math.isfinite(sigma_min) and sigma_min > 0.0):
            raise ValueError(f"sigma_min must be positive and finite, got {sigma_min}")
        if R > 1 and K > _lib.PLAN_REFIT_MAX_K:
            raise ValueError(f"iterations > 1 needs at most {_lib.PLAN_REFIT_MAX_K} candidates per group (usim_plan_refit), got {K}")
        self.real, self.sim = real, sim
        self.groups, self.per_group, self.horizon, self.action_dim = G, K, H, A
        self.tail_action, self.iterations, self.elites, self.momentum, self.sigma_min = bool(tail_action), R, E, float(momentum), float(sigma_min)
        self.temperature, self.gamma, self.smoothing, self.seed = float(temperature), float(gamma), float(smoothing), int(seed) & (2**64 - 1)
        self.lib = _lib.load()
        dev = self.device = real.device
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.sigma = torch.tensor(sig, dtype=torch.float32, device=dev)
        self._low = torch.as_tensor(real.action_space.low, dtype=torch.float32, device=dev).contiguous()
        self._high = torch.as_tensor(real.action_space.high, dtype=torch.float32, device=dev).contiguous()
        self.mean, self.plan_actions, self.action = f32(G, H, A), f32(G, H, A), f32(G, A)
        self.candidates, self.returns, self.weights = f32(H, n, A), f32(n), f32(n)
        self.lengths = torch.zeros(n, dtype=torch.int32, device=dev)
        self.best = torch.zeros(G, dtype=torch.int32, device=dev)
        self.restart = torch.zeros(G, dtype=torch.uint8, device=dev)
        self.noise_counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self._snap = torch.zeros((G, real.snapshot_words), dtype=torch.float32, device=dev)
        self._rows = (torch.arange(n, dtype=torch.int32, device=dev) // self.per_group).contiguous()       # sim environment i continues from real environment i // K
        self.block = self._block = sim.alloc_block(H, with_actions=False)
        self.graph = None
        self.critic = None
        if critic is not None:
            self._bind_critic(*critic)
        if R > 1:
            self._sigma0 = self.sigma.expand(G, H, A).contiguous()                                         # what sigma_elem restarts from at every plan
            self.sigma_elem = self._sigma0.clone()
            self.elite = torch.full((G, E), -1, dtype=torch.int32, device=dev)
        # both kernels once on the zeroed buffers, `mean` left alone: the library's own argument checks speak here, not in the first plan, and the first launch of
        # the unit's kernels happens outside any capture
        self.sample()
        self.update(shift=False)
        # the same for the kernels an option adds; refit and tail write into `mean`, which is zeroed again
        if self.critic is not None:
            self.evaluate_tail()
            self.score()
            if self.tail_action:
                self.tail()
        if R > 1:
            self.sample_elem()
            self.refit()
            self.sigma_elem.copy_(self._sigma0)
        if self.tail_action or R > 1:
            self.mean.zero_()

    def _bind_critic(self, policy, vecnorm):
        """the argument blocks of usim_policy_step for the n candidates: the network's parameters and the statistics at their addresses, outputs allocated once"""
        dev, n, A = self.device, self.groups * self.per_group, self.action_dim
        if policy.pi_sizes != (256, 128) or policy.vf_sizes != (256, 128) or policy.policy_net[0].in_features != 19 or policy.action_net.out_features != A:
            raise ValueError(f"the critic must be the MlpPolicy of the shipped checkpoints, 19 -> 256 -> 128 (tanh) for both networks, with {A} actions")
        for p_ in policy.parameters():
            if p_.device != dev or p_.dtype != torch.float32 or not p_.is_contiguous():
                raise ValueError("the critic's parameters must be contiguous float32 tensors on the environments' device")
        vn, ptr = vecnorm, lambda t: t.data_ptr()
        self.critic = (policy, vecnorm)
        self._w2_packed = torch.zeros(_lib.POLICY_PACKED, dtype=torch.float32, device=dev)
        self._net = policy_net(policy, self._w2_packed)
        self._stats = _lib.UsimNormStats(ptr(vn.obs_mean), ptr(vn.obs_var), ptr(vn._obs_count), ptr(vn.ret_mean), ptr(vn.ret_var), ptr(vn._ret_count), ptr(vn.returns),
                                         None, float(vn.clip_obs), float(vn.clip_reward), float(vn.gamma), float(vn.epsilon))      # (no scratch: the statistics are never updated)
        self.tail_value = torch.zeros(n, dtype=torch.float32, device=dev)
        self.tail_policy_action = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self._out = _lib.UsimPolicyOut(self.tail_policy_action.data_ptr(), None, None, self.tail_value.data_ptr(), None, None)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def sample(self):
        """usim_plan_sample: `candidates` around `mean` (around zero, and `mean` zeroed, where `restart` is set) with the noise of the present counter"""
        rc = self.lib.usim_plan_sample(self.mean.data_ptr(), self.sigma.data_ptr(), self._low.data_ptr(), self._high.data_ptr(), self.restart.data_ptr(), self.groups,
                                       self.per_group, self.horizon, self.action_dim, self.smoothing, self.seed, 0, self.noise_counter.data_ptr(),
                                       self.candidates.data_ptr(), self._stream())
        _lib.check(self.lib, rc)
        return self.candidates

    def update(self, shift=True):
        """usim_plan_update: `best`, `weights`, `plan_actions`, `action` from `candidates` and `returns`; with `shift` the shifted plan goes into `mean`"""
        rc = self.lib.usim_plan_update(self.candidates.data_ptr(), self.returns.data_ptr(), self._low.data_ptr(), self._high.data_ptr(), self.groups, self.per_group,
                                       self.horizon, self.action_dim, self.temperature, self.plan_actions.data_ptr(), self.mean.data_ptr() if shift else None,
                                       self.action.data_ptr(), self.best.data_ptr(), self.weights.data_ptr(), self._stream())
        _lib.check(self.lib, rc)
        return self.action

    def sample_elem(self, restart=True):
        """usim_plan_sample_elem: sample() with the per-element `sigma_elem`; restart=False leaves the restart flags out (the rounds after the first: the first has
        zeroed the nominal of a restarted group, and the refits since are to be kept)"""
        rc = self.lib.usim_plan_sample_elem(self.mean.data_ptr(), self.sigma_elem.data_ptr(), self._low.data_ptr(), self._high.data_ptr(),
                                            self.restart.data_ptr() if restart else None, self.groups, self.per_group, self.horizon, self.action_dim, self.smoothing,
                                            self.seed, 0, self.noise_counter.data_ptr(), self.candidates.data_ptr(), self._stream())
        _lib.check(self.lib, rc)
        return self.candidates

    def refit(self):
        """usim_plan_refit: `mean` and `sigma_elem` towards the elite candidates' mean and standard deviation, from `candidates` and `returns`; `elite` their indices"""
        rc = self.lib.usim_plan_refit(self.candidates.data_ptr(), self.returns.data_ptr(), self._low.data_ptr(), self._high.data_ptr(), self.groups, self.per_group,
                                      self.horizon, self.action_dim, self.elites, self.momentum, self.sigma_min, self.mean.data_ptr(), self.sigma_elem.data_ptr(),
                                      self.elite.data_ptr(), self._stream())
        _lib.check(self.lib, rc)
        return self.mean

    def evaluate_tail(self, pack=True):
        """usim_policy_step (statistics frozen, deterministic) on the candidates' last observations: `tail_value`, `tail_policy_action`.  pack: usim_policy_pack
        first -- the layer-2 weights as they are now, as policy.FusedRollout packs before every launch that may follow a change of the parameters"""
        if pack:
            _lib.check(self.lib, self.lib.usim_policy_pack(C.byref(self._net), self._w2_packed.data_ptr(), self._stream()))
        rc = self.lib.usim_policy_step(C.byref(self._net), C.byref(self._stats), self._block["obs"][self.horizon - 1].data_ptr(), None, self.groups * self.per_group,
                                       self.action_dim, self._low.data_ptr(), self._high.data_ptr(), self.seed, 0, None, 0, 0, 1, C.byref(self._out), self._stream())
        _lib.check(self.lib, rc)
        return self.tail_value

    def score(self):
        """`returns`, `lengths` of the played candidates: usim_score_block, or with a critic usim_score_block_tail on `tail_value`"""
        if self.critic is None:
            return self.sim.score_block(self._block, gamma=self.gamma, out=(self.returns, self.lengths))
        vn = self.critic[1]
        rc = self.lib.usim_score_block_tail(self._block["rew"].data_ptr(), self._block["done"].data_ptr(), self.horizon, self.groups * self.per_group, self.gamma,
                                            self.tail_value.data_ptr(), vn.ret_var.data_ptr() if vn.norm_reward else None, float(vn.epsilon),
                                            self.returns.data_ptr(), self.lengths.data_ptr(), self._stream())
        _lib.check(self.lib, rc)
        return self.returns, self.lengths

    def tail(self):
        """usim_plan_tail: the last step of `mean` from `weights`, `best`, `lengths`, the last done flags and `tail_policy_action`; after update()"""
        rc = self.lib.usim_plan_tail(self.candidates.data_ptr(), self.weights.data_ptr(), self.best.data_ptr(), self.lengths.data_ptr(),
                                     self._block["done"][self.horizon - 1].data_ptr(), self.tail_policy_action.data_ptr(), self._low.data_ptr(), self._high.data_ptr(),
                                     self.groups, self.per_group, self.horizon, self.action_dim, self.temperature, self.mean.data_ptr(), self._stream())
        _lib.check(self.lib, rc)
        return self.mean

    def _round(self, snap, first):
        """one round of a plan: load the saved real states into their groups, sample the candidates, play them, score them.  first: the round that reads the
        restart flags and packs the critic's weights"""
        self.sim.load_envs(snap, self._rows)
        if self.iterations > 1:
            self.sample_elem(restart=first)
        else:
            self.sample()
        self.sim.rollout_actions(self.candidates, self._block)
        if self.critic is not None:
            self.evaluate_tail(pack=first)
        self.score()

    def plan(self):
        """One planning step from the present state of `real`, which is read and not modified: returns `action` [G, A].  Six launches on the current stream and
        the advance of the noise counter; nothing touches the host.  A critic adds one launch per round and the pack of its weights, tail_action one launch, and
        every round before the last its load, sample, rollout, score, refit and counter advance (and iterations > 1 the copy that restarts `sigma_elem`)."""
        snap = self.real.save_envs(out=self._snap)
        if self.iterations > 1:
            self.sigma_elem.copy_(self._sigma0)
        for r in range(self.iterations - 1):
            self._round(snap, first=r == 0)
            self.refit()
            self.noise_counter.add_(1)
        self._round(snap, first=self.iterations == 1)
        self.update()
        if self.tail_action:
            self.tail()
        self.noise_counter.add_(1)
        return self.action

    def step(self):
        """plan(), then real.step_tensor(action); the done flags become the restart flags of the next plan.  Returns real's (obs, rew, done) tensors."""
        obs, rew, done = self.real.step_tensor(self.plan())
        self.restart.copy_(done)
        return obs, rew, done

    def _recorded(self):
        # the rule of every recorded sequence of steps (policy.GraphedCollector): the reset banks are refilled first and last, so a replay is valid whatever ran before it
        self.real.refill_bank(); self.sim.refill_bank()
        self.step()
        self.real.refill_bank(); self.sim.refill_bank()

    def record(self):
        """Capture one step() as a HIP graph on a side stream (one stream, no parallel branches); replay() launches it.  Nothing runs during the capture: the
        environments and the planner stand where they stood.  The noise counter is a device word, so every replay draws fresh noise."""
        self.graph = _capture(self.real, self._recorded, prologue=self.sim.refill_bank)
        return self.graph

    def replay(self):
        """one recorded step(); returns real's (obs, rew, done) tensors"""
        if self.graph is None:
            raise RuntimeError("replay() before record()")
        self.graph.replay()
        return self.real._obs, self.real._rew, self.real._done
