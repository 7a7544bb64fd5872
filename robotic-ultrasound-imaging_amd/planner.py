"""A batched MPPI shooting planner on the device: a model-predictive baseline next to the reference's PPO policies.

`MPPIPlanner(real, sim, ...)` controls the G environments of `real` with the n = G K environments of `sim`: environments [g K, (g + 1) K) of `sim` play the K
candidate action sequences of real environment g, candidate 0 being the unperturbed nominal.  A planning step is six launches and no host work in between --
save the real states, load them into their groups, sample the candidates around the nominal (usim_plan_sample), play them (usim_rollout_actions), score them
(usim_score_block), and form the exponentially weighted plan, the action and the shifted nominal of the next step (usim_plan_update; csrc/usim_plan.hip).  Every
buffer is allocated once, so a whole step() -- plan, the real step, the restart flags -- is recordable as one HIP graph."""
import ctypes as C
import math

import torch

from . import _lib
from .policy import _capture


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
    shifted by one step).  All are device tensors that the next plan overwrites.  `restart` [G] (uint8) are the flags the next plan reads: where non-zero the group
    is sampled around zero and its nominal is zeroed.  `noise_counter` (int32 [1], device) is advanced by every plan; set it to repeat a sequence of draws."""

    def __init__(self, real, sim, horizon=16, sigma=0.3, temperature=1.0, gamma=1.0, smoothing=0.0, seed=0):
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
        self.real, self.sim = real, sim
        self.groups, self.per_group, self.horizon, self.action_dim = G, n // G, H, A
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
        self._block = sim.alloc_block(H, with_actions=False)
        self.graph = None
        # both kernels once on the zeroed buffers, `mean` left alone: the library's own argument checks speak here, not in the first plan, and the first launch of
        # the unit's kernels happens outside any capture
        self.sample()
        self.update(shift=False)

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

    def plan(self):
        """One planning step from the present state of `real`, which is read and not modified: returns `action` [G, A].  Six launches on the current stream and
        the advance of the noise counter; nothing touches the host."""
        snap = self.real.save_envs(out=self._snap)
        self.sim.load_envs(snap, self._rows)
        self.sample()
        self.sim.rollout_actions(self.candidates, self._block)
        self.sim.score_block(self._block, gamma=self.gamma, out=(self.returns, self.lengths))
        self.update()
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
