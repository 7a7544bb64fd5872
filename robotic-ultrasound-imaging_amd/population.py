"""Policy populations: K networks ("members") in ONE rollout, evaluated and trained side by side (include/usim.h usim_policy_pack_multi / usim_policy_step_multi /
usim_policy_reward_multi; csrc/usim_policy.hip).  n = K G environments, member k owning environments [k G, (k + 1) G): the policy
launch's unit of work is 32 environments x one network, so the member is one more grid axis and the launch count of a rollout step does not grow with K.
Environments do not depend on their neighbours, so a population computes, bit for bit, what K lone runs on shard environments (num_envs = G, env_offset = k G, same
seed) compute -- tests/test_gpu_population_rollout.py, tests/test_gpu_population_ppo.py.

    pop = PolicyPopulation.from_checkpoints(sorted(folder.glob("rl_model_*_steps.zip")), device=env.device)      # K = len(paths)
    vn = PopulationVecNormalize(pop.members, env.num_envs // pop.members, device=env.device, training=False)
    for k, p in enumerate(pkls): vn.load_member(k, p)
    ranking = evaluate_population(env, pop, vn, n_eval_episodes=10)                                              # [(mean, std)] x K

    pop, vn = PolicyPopulation(4, env.action_dim, env.device), PopulationVecNormalize(4, env.num_envs // 4, device=env.device)
    buffer = DeviceRolloutBuffer(T, env.num_envs, 19, env.action_dim, device=env.device)
    collector = PopulationRollout(env, pop, vn, buffer, seed=0)
    ppo = PopulationPPO(env, pop, vn, buffer, collector, seeds=[0, 1, 2, 3], learning_rate=[3e-4, 3e-4, 1e-4, 1e-4]); ppo.learn(40)

    ppo = PopulationPPO(env, pop, vn, buffer, collector, seeds=range(32), learning_rate=list(sweep), concurrent=True)     # one gradient launch for all K members

PopulationPPO(concurrent=True) is the learner's side of the same idea (include/usim.h usim_ppo_grad_multi / usim_ppo_adam_multi): the member is a grid axis of the
learner's kernels, a minibatch step of K members is the launches of one, and every member's words are the bits of its lone update.

Still out: a multi form of usim_policy_step_fused (its cross-workgroup wait would have to become per member) and the time-limit bootstrap (refused)."""
import ctypes as C
import math
import time
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .learner import FIELDS, _check_shapes, _field_shapes, _is_flat, ppo_params, state_dict_to_flat
from .monitor import DeviceMonitor, eval_targets
from .policy import DeviceRolloutBuffer, DeviceVecNormalize, MlpActorCritic, _capture, load_sb3_zip, load_vecnormalize_pkl

_CONSTANTS = ("clip_obs", "clip_reward", "gamma", "epsilon")


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class PolicyPopulation:
    """K policies as ONE tensor: theta [K, stride] float32, row k the flat parameter block of member k in the field order of include/usim.h (learner.ppo_params(A)
    words; stride: that, rounded up to a multiple of 4), and packed [K, USIM_POLICY_PACKED], the layer-2 weights in operand order (pack()).  member(k) is a
    policy.MlpActorCritic whose parameters are views into row k -- learner._is_flat holds for it, learner.flatten_parameters(member(k)) returns the row's first P
    words without copying -- so a learner, save_sb3_zip and the population's kernels work on the same memory.  New members carry torch's default initialisation."""

    def __init__(self, members, act_dim, device="cuda:0", stride=None):
        K, A = int(members), int(act_dim)
        if not 1 <= K <= _lib.POLICY_MAX_MEMBERS:
            raise ValueError(f"members must be 1 .. {_lib.POLICY_MAX_MEMBERS}, got {members!r}")
        if not 1 <= A <= 8:
            raise ValueError(f"act_dim {A} outside 1 .. 8")
        P = ppo_params(A)
        stride = (P + 3) // 4 * 4 if stride is None else int(stride)
        if stride < P or stride % 4:
            raise ValueError(f"stride must be a multiple of 4 of at least {P} words, got {stride}")
        self.members, self.act_dim, self.params, self.stride, self.device = K, A, P, stride, torch.device(device)
        self.theta = torch.zeros(K, stride, dtype=torch.float32, device=self.device)
        self.packed = torch.zeros(K, _lib.POLICY_PACKED, dtype=torch.float32, device=self.device)
        self._members = [self._seat(MlpActorCritic(_lib.OBS_DIM, A), k) for k in range(K)]

    def _seat(self, policy, k):
        """learner.flatten_parameters into row k instead of a tensor of the module's own: the values are kept, the parameters become views"""
        row, o = self.theta[k, :self.params], 0
        params = dict(policy.named_parameters())
        with torch.no_grad():
            for (_, path), shape in zip(FIELDS, _field_shapes(self.act_dim)):
                p, n = params[path], math.prod(shape)
                view = row[o:o + n].view(shape)
                view.copy_(p.detach().to(torch.float32))
                p.data = view
                o += n
        policy._flat_theta = row
        assert _is_flat(policy, row)
        return policy

    def member(self, k):
        return self._members[k]

    def load_member(self, k, source):
        """row k <- a policy.MlpActorCritic of the same shapes, or the path of an SB3 checkpoint zip (policy.load_sb3_zip); in place: addresses are kept"""
        if isinstance(source, torch.nn.Module):
            if _check_shapes(source) != self.act_dim:
                raise ValueError(f"policy shapes: act_dim {source.log_std.shape[0]} is not the population's {self.act_dim}")
            flat = state_dict_to_flat({n: p.detach() for n, p in source.named_parameters()}, self.act_dim)
        else:
            flat = state_dict_to_flat(load_sb3_zip(source)[0], self.act_dim)
        with torch.no_grad():
            self.theta[k, :self.params].copy_(flat)
        return self._members[k]

    @classmethod
    def from_policies(cls, policies, device=None):
        policies = list(policies)
        if not policies:
            raise ValueError("a population needs at least one policy")
        dev = next(policies[0].parameters()).device if device is None else device
        self = cls(len(policies), _check_shapes(policies[0]), dev)
        for k, p in enumerate(policies):
            self.load_member(k, p)
        return self

    @classmethod
    def from_checkpoints(cls, paths, device="cuda:0"):
        paths = list(paths)
        if not paths:
            raise ValueError("a population needs at least one checkpoint")
        self = cls(len(paths), load_sb3_zip(paths[0])[0]["action_net.weight"].shape[0], device)
        for k, p in enumerate(paths):
            self.load_member(k, p)
        return self

    def pack(self):
        """usim_policy_pack_multi: every member's layer-2 weights as they are now, in operand order -- one launch on the current stream"""
        lib = _lib.load()
        _lib.check(lib, lib.usim_policy_pack_multi(self.theta.data_ptr(), self.stride, self.members, self.act_dim, self.packed.data_ptr(), _stream(self.device)))


class _MemberVecNormalize(DeviceVecNormalize):
    """one member of a PopulationVecNormalize: a DeviceVecNormalize on views of the population's tensors; training / norm_reward are the population's"""
    training = property(lambda self: self._population.training)
    norm_reward = property(lambda self: self._population.norm_reward)

    def __init__(self, population, k):
        p, G = population, population.envs_per_member
        self._population = p
        self.obs_mean, self.obs_var, self._obs_count = p.obs_mean[k], p.obs_var[k], p._obs_count[k]
        self.ret_mean, self.ret_var, self._ret_count = p.ret_mean[k], p.ret_var[k], p._ret_count[k]
        self.returns = p.returns[k * G:(k + 1) * G]
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = p.clip_obs, p.clip_reward, p.gamma, p.epsilon


class PopulationVecNormalize:
    """K policy.DeviceVecNormalize in the K-major layout of include/usim.h: obs_mean / obs_var [K, 19], the counts and return moments [K], returns [K G]; the
    four constants, `training` and `norm_reward` are shared.  member(k) is a DeviceVecNormalize on the same memory."""

    def __init__(self, members, envs_per_member, obs_dim=19, device="cuda:0", clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8, training=True,
                 norm_reward=True):
        K, G = int(members), int(envs_per_member)
        if K < 1 or G < 1 or K * G > 2 ** 31 - 1:
            raise ValueError(f"members and envs_per_member must be at least 1 and their product within 2^31 - 1, got {members!r}, {envs_per_member!r}")
        dev = torch.device(device)
        self.members, self.envs_per_member, self.device = K, G, dev
        f = lambda shape, v: torch.full(shape, v, dtype=torch.float64, device=dev)
        self.obs_mean, self.obs_var, self._obs_count = f((K, obs_dim), 0.0), f((K, obs_dim), 1.0), f((K,), 1e-4)
        self.ret_mean, self.ret_var, self._ret_count = f((K,), 0.0), f((K,), 1.0), f((K,), 1e-4)
        self.returns = f((K * G,), 0.0)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), float(epsilon)
        self.training, self.norm_reward = bool(training), bool(norm_reward)
        self._members = [_MemberVecNormalize(self, k) for k in range(K)]

    def member(self, k):
        return self._members[k]

    def load_member(self, k, stats):
        """member k <- the dictionary policy.load_vecnormalize_pkl returns, or the path of such a pickle; its four constants must be the population's"""
        st = stats if isinstance(stats, dict) else load_vecnormalize_pkl(stats)
        if len(st["obs_mean"]) != self.obs_mean.shape[1]:
            raise ValueError(f"statistics of {len(st['obs_mean'])} observations, the population's {self.obs_mean.shape[1]}")
        for key in _CONSTANTS:
            if float(st[key]) != getattr(self, key):
                raise ValueError(f"VecNormalize {key} {st[key]!r} is not the population's {getattr(self, key)!r}: the constants are shared")
        m = self._members[k]
        m.obs_mean.copy_(torch.as_tensor(st["obs_mean"], dtype=torch.float64)); m.obs_var.copy_(torch.as_tensor(st["obs_var"], dtype=torch.float64))
        m._obs_count.fill_(float(st["count"])); m._ret_count.fill_(float(st.get("ret_count", st["count"])))
        m.ret_mean.fill_(float(st["ret_mean"])); m.ret_var.fill_(float(st["ret_var"]))
        return m


def _check_population(env, population, vecnorm, buffer=None, bootstrap_truncation=False):
    """the refusals the population's collectors and learners share (ValueError, before the library is loaded) -> (K, G)"""
    K, G = int(population.members), int(vecnorm.envs_per_member)
    if bootstrap_truncation:
        raise ValueError("bootstrap_truncation: usim_policy_bootstrap has no population form; collect each member with policy.FusedRollout instead")
    if int(vecnorm.members) != K:
        raise ValueError(f"the statistics hold {vecnorm.members} members, the population {K}")
    if int(env.num_envs) != K * G:
        raise ValueError(f"env.num_envs {env.num_envs} is not members x envs_per_member = {K} x {G}")
    if buffer is not None and int(buffer.n_envs) != K * G:
        raise ValueError(f"the buffer holds {buffer.n_envs} environments, the population {K} x {G}")
    if int(env.action_dim) != int(population.act_dim):
        raise ValueError(f"the population's act_dim {population.act_dim} is not the environment's {env.action_dim}")
    dev = torch.device(env.device)
    for what, x in (("population", population), ("statistics", vecnorm), ("buffer", buffer)):
        if x is not None and torch.device(x.device) != dev:
            raise ValueError(f"the {what} is on device {x.device}, the environment on {dev}")
    return K, G


class PopulationRollout:
    """policy.FusedRollout(fused_stats=False) for a population: the same recorded sequence -- refill, pack, T x (policy launch with training = 2 or 0, env step,
    reward launch with the returned observation), the bootstrap-value launch, GAE, the counter advance, refill -- with the population's calls, so a rollout of K
    members is as many launches as a rollout of one.  The buffer is ONE policy.DeviceRolloutBuffer over all K G environments (member k's samples are its
    [:, k G:(k + 1) G] slices); raw_reward_sum [K].  The noise of environment i is keyed (seed, env.env_offset + i, step), whichever member i belongs to."""

    def __init__(self, env, population, vecnorm, buffer, seed=0, graph=True, init_stats=True, bootstrap_truncation=False):
        K, G = _check_population(env, population, vecnorm, buffer, bootstrap_truncation)
        self.env, self.population, self.vecnorm, self.buffer, self.seed = env, population, vecnorm, buffer, int(seed)
        self.members, self.envs_per_member = K, G
        self.lib = _lib.load()
        dev, vn, ptr = env.device, vecnorm, (lambda t: t.data_ptr())
        self._scratch = torch.zeros(K * _lib.POLICY_SCRATCH, dtype=torch.float64, device=dev)
        self._stats = _lib.UsimNormStats(ptr(vn.obs_mean), ptr(vn.obs_var), ptr(vn._obs_count), ptr(vn.ret_mean), ptr(vn.ret_var), ptr(vn._ret_count), ptr(vn.returns),
                                         ptr(self._scratch), vn.clip_obs, vn.clip_reward, vn.gamma, vn.epsilon)
        self._low = torch.as_tensor(env.action_space.low, dtype=torch.float32, device=dev).contiguous()
        self._high = torch.as_tensor(env.action_space.high, dtype=torch.float32, device=dev).contiguous()
        self._act_env = torch.zeros(env.num_envs, env.action_dim, dtype=torch.float32, device=dev)
        self._value = torch.zeros(env.num_envs, dtype=torch.float32, device=dev)
        self.raw_reward_sum = torch.zeros(K, dtype=torch.float64, device=dev)
        self.counter = 0                                                                    # rollouts collected
        self._ctr = torch.zeros(1, dtype=torch.int32, device=dev)                           # device part of the noise counter: advanced by every rollout
        self.obs = env.reset_tensor()                                                       # the env's own observation buffer: rewritten by every step
        self._prev_done = env._done
        self._prev_done.fill_(1)                                                            # every environment starts an episode
        if vn.training and init_stats:                                                      # VecNormalize.reset(): every member's statistics see its reset observations
            self.act(self.obs, self._prev_done, counter=0, training=1, deterministic=True)
        self.graph = _capture(env, self._record) if graph else None

    def _check(self, rc):
        _lib.check(self.lib, rc, None)

    def pack(self):
        self.population.pack()

    def act(self, obs, prev_done, counter, training=None, deterministic=False, t=None, pack=True):
        """usim_policy_step_multi on raw observations [K G, 19]: returns (clipped actions for the env, values); with t, the buffer slices of step t are written"""
        env, b, pop = self.env, self.buffer, self.population
        if pack:
            self.pack()
        training = self.vecnorm.training if training is None else training
        ptr = lambda x: None if x is None else x.data_ptr()
        if t is None:
            out = _lib.UsimPolicyOut(ptr(self._act_env), None, None, ptr(self._value), None, None)
        else:
            out = _lib.UsimPolicyOut(ptr(self._act_env), ptr(b.observations[t]), ptr(b.actions[t]), ptr(b.values[t]), ptr(b.log_probs[t]), ptr(b.episode_starts[t]))
        self._check(self.lib.usim_policy_step_multi(ptr(pop.theta), pop.stride, ptr(pop.packed), C.byref(self._stats), ptr(obs), ptr(prev_done), self.members,
                                                    self.envs_per_member, env.action_dim, ptr(self._low), ptr(self._high), self.seed, int(counter) & 0xffffffff,
                                                    ptr(self._ctr), int(env.env_offset), int(training), int(bool(deterministic)), C.byref(out), env._stream()))
        return self._act_env, (self._value if t is None else b.values[t])

    def _record(self):
        env, b, vn = self.env, self.buffer, self.vecnorm
        T, n = b.buffer_size, env.num_envs
        env.refill_bank()
        self.raw_reward_sum.zero_()
        self.pack()
        for t in range(T):
            self.act(self.obs, self._prev_done, counter=t, training=2 if vn.training else 0, t=t, pack=False)
            o, rew, done = env.step_tensor(self._act_env)
            self._check(self.lib.usim_policy_reward_multi(C.byref(self._stats), rew.data_ptr(), done.data_ptr(), self.members, self.envs_per_member, int(bool(vn.training)),
                                                          int(bool(vn.norm_reward)), b.rewards[t].data_ptr(), self.raw_reward_sum.data_ptr(),
                                                          o.data_ptr() if vn.training else None, env._stream()))
        self.act(self.obs, self._prev_done, counter=T, training=0, deterministic=True, pack=False)
        self._check(self.lib.usim_policy_gae(b.rewards.data_ptr(), b.values.data_ptr(), b.episode_starts.data_ptr(), self._value.data_ptr(), self._prev_done.data_ptr(),
                                             T, n, b.gamma, b.gae_lambda, b.advantages.data_ptr(), b.returns.data_ptr(), env._stream()))
        self._ctr.add_(T + 1)
        env.refill_bank()

    def collect(self):
        """one rollout of buffer.buffer_size steps of all members into the buffer (returns / advantages included)"""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._record()
        self.counter += 1
        self.buffer.pos, self.buffer.full = self.buffer.buffer_size, True
        return self.obs, self._prev_done


def evaluate_population(env, population, vecnorm, n_eval_episodes=10, deterministic=True, seed=0, check_every=50, return_episode_rewards=False):
    """monitor.evaluate_policy for every member in one run: member k plays n_eval_episodes complete episodes on its environments [k G, (k + 1) G), environment i of
    a member contributing its first (n_eval_episodes + i) // G.  ONE DeviceMonitor (window K n_eval_episodes: the ring holds every counted episode; targets
    eval_targets(n_eval_episodes, G) tiled K times) is attached for the run, its episodes are grouped by env // G, and the loop stops when it has counted all
    K n_eval_episodes.  The statistics are frozen (training = 0).  The monitor and observers attached before are taken off first and put back afterwards, as in
    evaluate_policy.  -> a list of K (mean, std); with return_episode_rewards=True a list of K (episode returns, episode lengths), each what evaluate_policy gives
    for that member on a shard environment (num_envs = G, env_offset = k G)."""
    n_eval = int(n_eval_episodes)
    if n_eval < 1:
        raise ValueError("n_eval_episodes must be at least 1")
    K, G = _check_population(env, population, vecnorm)
    targets = eval_targets(n_eval, G) * K
    total = K * n_eval
    before = env.detach_monitor()
    others = env.detach_observer()
    try:
        mon = DeviceMonitor(env, window=total, targets=targets)
        buf = DeviceRolloutBuffer(1, env.num_envs, _lib.OBS_DIM, env.action_dim, device=env.device)
        pr = PopulationRollout(env, population, vecnorm, buf, seed=seed, graph=False, init_stats=False)
        obs = env.reset_tensor()
        env.attach_monitor(mon)
        pr.pack()
        bound, every, got = max(targets) * int(env.horizon), max(1, int(check_every)), 0
        for k in range(bound):
            act, _ = pr.act(obs, None, counter=k, training=0, deterministic=deterministic, pack=False)
            obs, _, _ = env.step_tensor(act)
            if (k + 1) % every == 0 or k + 1 == bound:
                got = mon.episode_count()
                if got >= total:
                    break
        if got < total:
            raise RuntimeError(f"evaluate_population: {got} of {total} episodes after {bound} steps (max(target) x horizon)")
        eps = mon.episodes()
    finally:
        env.detach_monitor()
        env.detach_observer()
        if before is not None:
            env.attach_monitor(before)
        for o in others:
            env.attach_observer(o)
    out = []
    for k in range(K):
        mine = [e for e in eps if e["env"] // G == k]
        returns, lengths = [e["r"] for e in mine], [e["l"] for e in mine]
        out.append((returns, lengths) if return_episode_rewards else (float(np.mean(returns)), float(np.std(returns))))
    return out


class _BufferSlice(DeviceRolloutBuffer):
    """member k's columns of a shared DeviceRolloutBuffer: the [:, k G:(k + 1) G] views of its tensors, n_envs = G; pos / full are the shared buffer's"""
    pos = property(lambda self: self._shared.pos)
    full = property(lambda self: self._shared.full)

    def __init__(self, shared, k, G):
        self._shared, self.buffer_size, self.n_envs, self.gamma, self.gae_lambda, self.device = shared, shared.buffer_size, int(G), shared.gamma, shared.gae_lambda, shared.device
        for name in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            setattr(self, name, getattr(shared, name)[:, k * G:(k + 1) * G])


def _per_member(name, value, K):
    """a hyper-parameter as K values: a list / tuple / array of length K, or one value (a callable schedule included) for all"""
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != K:
            raise ValueError(f"{name}: {len(value)} values for {K} members")
        return list(value)
    return [value] * K


_SHARED = ("n_epochs", "batch_size", "normalize_advantage", "adam_eps")      # one value for all members of a concurrent population: they shape the launches


def _check_concurrent(per):
    """the refusals of PopulationPPO(concurrent=True) (ValueError, before the library is loaded); `per`: keyword -> its K values"""
    for name in _SHARED:
        v = per.get(name)
        for k in range(1, len(v) if v else 0):
            if v[k] != v[0]:
                raise ValueError(f"concurrent=True: {name} must be the same for all members, member 0 has {v[0]!r} and member {k} has {v[k]!r}; the members of "
                                 f"one launch share it (learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, target_kl and the value of clip_range_vf may differ)")
    v = per.get("clip_range_vf")
    if v:
        for k in range(1, len(v)):
            if (v[k] is None) != (v[0] is None):
                raise ValueError(f"concurrent=True: clip_range_vf must be set for all members or for none (value clipping is an instance of the gradient kernel), "
                                 f"member 0 has {v[0]!r} and member {k} has {v[k]!r}")


class PopulationPPO:
    """K ppo.NativePPO learners over one PopulationRollout: member k's learner sees population.member(k), vecnorm.member(k) and its columns of the shared buffer
    (n_envs = G), and computes what a lone NativePPO computes on a shard.  `seeds` (K minibatch-shuffle seeds) and every keyword of NativePPO, each one value for
    all members or a sequence of K: several seeds of one configuration, or a sweep.  update() runs the K updates one after the other, then collector.pack() once.
    history[k]: member k's rows as NativePPO.learn() writes them (time/*, train/*); with a monitor attached to the env (before the collector was built) also
    rollout/ep_rew_mean and rollout/ep_len_mean over member k's rows of the monitor's ring.  The ring is SHARED: its `window` last episodes of ALL members, so a
    member's mean runs over roughly window / K episodes -- size the window K times SB3's 100 for the same smoothing.

    concurrent=True runs the K updates as ONE chain of launches (usim_ppo_grad_multi / usim_ppo_adam_multi: the member is a grid axis), bit for bit the updates of
    the sequential path.  n_epochs, batch_size, normalize_advantage and adam_eps must then be one value for all members, and clip_range_vf set for all or for none
    (ValueError before the library is loaded); learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, target_kl, the value of clip_range_vf (callables
    included) and the seeds stay per member.  The population then owns grad, exp_avg, exp_avg_sq [K, stride], step_count [K], stats / first_stats [K, 8], gate
    [K, 4], index [K, rollout], the hyper-parameter table and the workspace; every learner's attributes of those names are views of its row, so adam_state_dict,
    save_checkpoint, load_checkpoint, history and a member's lone update() keep working on the same memory.  It is meant for many small members, where a lone
    update is launch-bound and leaves most of its 256 gradient workgroups without a tile; with few large members (each minibatch already of 4096 rows or more) a
    lone gradient launch fills the device and the gain is smaller (1.15 times at 4 x 4096 environments); with ONE member leave it off: the concurrent update is 1.9 %
    slower than the lone one there (27.2 against 26.7 ms) -- profiles/population_learner/cost.txt has the measured points."""

    def __init__(self, env, population, vecnorm, buffer, collector, *, seeds, concurrent=False, **hyper):
        from .ppo import NativePPO
        K, G = _check_population(env, population, vecnorm, buffer)
        seeds = _per_member("seeds", seeds, K)
        per = {name: _per_member(name, v, K) for name, v in hyper.items()}
        if concurrent:
            _check_concurrent(per)
        self.env, self.population, self.vecnorm, self.buffer, self.collector = env, population, vecnorm, buffer, collector
        self.members, self.envs_per_member, self.concurrent = K, G, bool(concurrent)
        self.learners = []
        for k in range(K):
            self.learners.append(NativePPO(env, population.member(k), vecnorm.member(k), _BufferSlice(buffer, k, G), None, seed=seeds[k],
                                           **{name: v[k] for name, v in per.items()}))
            if concurrent:
                self._seat_learner(k)
        self.history = [[] for _ in range(K)]

    def _seat_learner(self, k):
        """concurrent=True: learner k's gradient, moments, step count, statistics, gate and index list become views of row k of the population's tensors (built with
        learner 0), and all learners share learner 0's lone workspace -- a member's lone update() stays valid on the same memory, K workspaces are not kept"""
        l, pop, K = self.learners[k], self.population, self.members
        if k == 0:
            dev, P = l.device, pop.params
            z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
            self.lib, self.device = l.lib, dev
            self.grad, self.exp_avg, self.exp_avg_sq = z(K, pop.stride), z(K, pop.stride), z(K, pop.stride)
            self.step_count, self.gate = z(K, dtype=torch.int32), z(K, _lib.PPO_GATE_WORDS, dtype=torch.int32)
            self.stats, self.first_stats = z(K, _lib.PPO_STATS), z(K, _lib.PPO_STATS)
            self.index, self.hyper = z(K, l.rollout, dtype=torch.int32), z(K, _lib.PPO_HYPER_WORDS)
            self._hyper_host = torch.zeros(K, _lib.PPO_HYPER_WORDS, dtype=torch.float32).pin_memory()
            self._ev, self._std = z(K), z(K)                                 # train/explained_variance and train/std of the last update(), per member
            floats = int(self.lib.usim_ppo_work_floats_multi(pop.act_dim, K, l.batch_size))
            if floats < 0:
                _lib.check(self.lib, floats, None)
            self._work = z(floats)
        P = pop.params
        l.grad, l.exp_avg, l.exp_avg_sq = self.grad[k, :P], self.exp_avg[k, :P], self.exp_avg_sq[k, :P]
        l.step_count, l.stats, l.first_stats, l.gate, l._index = self.step_count[k:k + 1], self.stats[k], self.first_stats[k], self.gate[k], self.index[k]
        l._work = self.learners[0]._work

    def update(self):
        """the K updates, then the collector's pack(); -> the K statistics dictionaries.  concurrent=False: NativePPO.update of every member, one after the other.
        concurrent=True: the same updates with the member as a grid axis -- the shared buffer is flattened once (environment-major: member k's rows are
        contiguous and are the rows of its lone flatten), the hyper-parameter table is written and the gates are cleared once, every epoch draws the K
        torch.randperm from the members' own generators (the draws of the sequential path, so the two paths and a member's lone update() are interchangeable
        mid-run), every minibatch is ONE usim_ppo_grad_multi and ONE usim_ppo_adam_multi, and one host read at the end brings all members' statistics, gates,
        explained variances and train/std.  Return value, every learner's last_update and every word of the members' state are those of the sequential path."""
        if self.concurrent:
            return self._update_concurrent()
        out = [l.update() for l in self.learners]
        self.collector.pack()
        return out

    def _update_concurrent(self):
        from .ppo import STAT_NAMES
        b, ls, K, G, lib, pop = self.buffer, self.learners, self.members, self.envs_per_member, self.lib, self.population
        if not b.full:
            raise RuntimeError("rollout buffer is not full")
        check = lambda rc: _lib.check(lib, rc, None)
        T, l0 = int(b.buffer_size), ls[0]
        N, batch, A, P = l0.rollout, l0.batch_size, pop.act_dim, pop.params
        # usim_explained_variance per member on its [T, G] block in the order of its lone update (K launches into K words)
        values, returns = (x.reshape(T, K, G).transpose(0, 1).contiguous() for x in (b.values, b.returns))
        for k in range(K):
            check(lib.usim_explained_variance(values[k].data_ptr(), returns[k].data_ptr(), T * G, self._ev.data_ptr() + 4 * k, _stream(self.device)))
        cvf = [l.current_clip_range_vf() for l in ls]
        value_clip = cvf[0] is not None
        obs, act, lp, adv, ret = (l0._flat(x) for x in (b.observations, b.actions, b.log_probs, b.advantages, b.returns))
        old = l0._flat(b.values) if value_clip else None
        self._hyper_host.copy_(torch.tensor([[l.current_lr(), l.current_clip_range(), l.ent_coef, l.vf_coef, l.max_grad_norm, cvf[k] or 0.0, l.target_kl or 0.0, 0.0]
                                             for k, l in enumerate(ls)], dtype=torch.float32))
        self.hyper.copy_(self._hyper_host, non_blocking=True)                # from pinned memory, in stream order: the host does not wait (update() ends with a read)
        self.gate.zero_()
        ptr = lambda t: t.data_ptr()
        steps = 0
        for _ in range(l0.n_epochs):
            for k, l in enumerate(ls):
                self.index[k].copy_(torch.randperm(N, device=self.device, generator=l.generator))
            for i in range(0, N, batch):
                n = min(batch, N - i)
                mb = _lib.UsimPpoBatchMulti(ptr(obs), ptr(act), ptr(lp), ptr(adv), ptr(ret), None if old is None else ptr(old), ptr(self.index) + 4 * i, ptr(self.hyper),
                                            ptr(self.gate), N, N, n, A, int(l0.normalize_advantage), int(value_clip))
                check(lib.usim_ppo_grad_multi(ptr(pop.theta), pop.stride, K, C.byref(mb), ptr(self._work), ptr(self.grad), ptr(self.stats), _stream(self.device)))
                check(lib.usim_ppo_adam_multi(ptr(pop.theta), ptr(self.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.step_count), pop.stride, K, P,
                                              ptr(self.hyper), 0.9, 0.999, l0.adam_eps, ptr(self.stats), ptr(self.gate), _stream(self.device)))
                if steps == 0:
                    self.first_stats.copy_(self.stats)
                steps += 1
        self.collector.pack()
        std = torch.exp(pop.theta[:, P - A:P])
        for k in range(K):                                                   # the lone update's reduction, member by member: the same bits
            torch.mean(std[k], dim=0, keepdim=True, out=self._std[k:k + 1])
        s = torch.cat((self.stats.reshape(-1), self._ev, self._std, self.gate.to(torch.float32).reshape(-1))).tolist()      # one read for all members
        n, out = _lib.PPO_STATS, []
        for k, l in enumerate(ls):
            stop, evaluated, done = (int(x) for x in s[(n + 2) * K + 4 * k:(n + 2) * K + 4 * k + 3])
            l.last_update = {"train/clip_range": l.current_clip_range(), **({} if cvf[k] is None else {"train/clip_range_vf": cvf[k]}), "train/std": s[(n + 1) * K + k],
                             "train/optimizer_steps": done, "train/minibatches_evaluated": evaluated, "train/early_stop": stop}
            out.append(dict(zip(STAT_NAMES, s[n * k:n * k + 6] + [s[n * K + k]])))
        return out

    def learn(self, iterations):
        """`iterations` x (collector.collect(), update()); -> the statistics of the last update, per member"""
        out = None
        for it in range(int(iterations)):
            for l in self.learners:
                l.progress_remaining = 1.0 - it / float(iterations)
            lrs = [l.current_lr() for l in self.learners]
            self.collector.collect()
            out = self.update()
            mon = getattr(self.env, "monitor", None)
            eps = mon.episodes() if mon is not None else None
            now = time.time()
            for k, l in enumerate(self.learners):
                l.num_timesteps += l.rollout
                row = {"time/total_timesteps": l.num_timesteps, "time/wall": now, **out[k], "train/learning_rate": lrs[k], **l.last_update}
                if eps is not None:
                    mine = [e for e in eps if e["env"] // self.envs_per_member == k]
                    row["rollout/ep_rew_mean"] = float(np.mean([e["r"] for e in mine])) if mine else float("nan")
                    row["rollout/ep_len_mean"] = float(np.mean([e["l"] for e in mine])) if mine else float("nan")
                self.history[k].append(row)
        for l in self.learners:
            l.progress_remaining = 1.0
        return out

    def save_checkpoint(self, folder, names):
        """one SB3 zip + VecNormalize pkl per member (NativePPO.save_checkpoint): folder/names[k].zip, folder/vec_normalize_<names[k]>.pkl -> the K path pairs"""
        names = _per_member("names", list(names), self.members)
        Path(folder).mkdir(parents=True, exist_ok=True)
        return [l.save_checkpoint(folder, str(names[k])) for k, l in enumerate(self.learners)]
