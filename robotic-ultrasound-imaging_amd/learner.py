"""What the learners on the device share, stated once: the ONE flat parameter block of include/usim.h (flatten_parameters and its conversions to and from the
files of an SB3 checkpoint) and FlatLearner, the core of ppo.NativePPO and imitation.NativeBC -- the block with its gradient, Adam moments, step count,
statistics and workspace, the clip_grad_norm_ + Adam.step call (usim_ppo_adam / usim_ppo_adam_gated) and the epoch loop over shuffled minibatches.  A learner adds
its own gradient call (usim_ppo_grad, usim_bc_grad) as minibatch_step."""
import ctypes as C
import math

import torch

from . import _lib
from .policy import FIELDS, policy_net

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
            p, n = params[path], math.prod(shape)
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


class FlatLearner:
    """The flat block of `policy` (flattened here if it is not flat yet) with what every learner keeps beside it.  A subclass checks its own arguments first, then
    calls this constructor, whose refusals are ValueErrors too and come before the library is loaded; `where` names what `device` is the device of in the
    message about a policy elsewhere ("environment", "buffer"); `index_rows` is the largest number of rows one pass shuffles.  A `collector` has recorded the
    parameters' addresses: a policy that is not flat yet is then refused, not re-seated."""

    def __init__(self, policy, act_dim, device, where, index_rows, *, n_epochs, max_grad_norm, adam_eps, seed, collector=None):
        dev = torch.device(device)
        if int(n_epochs) < 1:
            raise ValueError("n_epochs must be at least 1")
        for p in policy.parameters():
            if p.device != dev:
                raise ValueError(f"policy is on device {p.device}, the {where} on {dev}")
        theta = getattr(policy, "_flat_theta", None)
        if theta is None or not _is_flat(policy, theta):
            if collector is not None:
                raise ValueError("flatten_parameters(policy) must be called before the collector is built: it has recorded the parameters' addresses")
            theta = flatten_parameters(policy)
        self.policy, self.act_dim, self.device, self.n_epochs = policy, int(act_dim), dev, int(n_epochs)
        self.max_grad_norm, self.adam_eps = float(max_grad_norm), float(adam_eps)
        self.lib = _lib.load()
        self.theta, self.params = theta, theta.numel()
        z = lambda n, dtype=torch.float32: torch.zeros(n, dtype=dtype, device=dev)
        self.grad, self.exp_avg, self.exp_avg_sq = z(self.params), z(self.params), z(self.params)
        self.step_count = z(1, torch.int32)                                   # Adam's step, advanced on the device
        self.stats, self.first_stats = z(_lib.PPO_STATS), z(_lib.PPO_STATS)   # of the last minibatch; of the first minibatch of the last run_epochs()
        self._work = z(int(self.lib.usim_ppo_work_floats(self.act_dim)))
        self._index = z(int(index_rows), torch.int32)
        self.generator = torch.Generator(device=dev)
        self.generator.manual_seed(int(seed))
        self._net = policy_net(policy)

    def _check(self, rc):
        _lib.check(self.lib, rc, None)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def adam_step(self, lr, gate=None):
        """clip_grad_norm_ + Adam.step on the flat block with the gradient as it stands: usim_ppo_adam, or usim_ppo_adam_gated behind the gate words `gate`"""
        args = (self.theta.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.step_count.data_ptr(), self.params,
                float(lr), 0.9, 0.999, self.adam_eps, self.max_grad_norm, self.stats.data_ptr())
        if gate is None:
            self._check(self.lib.usim_ppo_adam(*args, self._stream()))
        else:
            self._check(self.lib.usim_ppo_adam_gated(*args, gate.data_ptr(), self._stream()))

    def run_epochs(self, N, batch, step):
        """n_epochs passes over rows 0 .. N - 1, each a torch.randperm on the device cut into minibatches of `batch` (the trailing partial one is used, as in
        SB3): step(index, n) per minibatch, first_stats after the first one.  -> the minibatches stepped"""
        steps = 0
        for _ in range(self.n_epochs):
            self._index[:N].copy_(torch.randperm(N, device=self.device, generator=self.generator))
            for i in range(0, N, batch):
                n = min(batch, N - i)
                step(self._index[i:i + n], n)
                if steps == 0:
                    self.first_stats.copy_(self.stats)
                steps += 1
        return steps
