"""usim_ppo_params / usim_ppo_work_floats / usim_ppo_grad / usim_ppo_adam on the host side: declared in include/usim.h, bound by _lib.SYMBOLS and exported by the
library built here; their argument checks answer USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up pointers that no kernel may
ever see, and run without a GPU.  The refusals of ppo.NativePPO's constructor come before any library call and are tested with stand-in objects;
ppo.flatten_parameters is tested on a CPU module."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
NAMES = ("usim_ppo_params", "usim_ppo_work_floats", "usim_ppo_grad", "usim_ppo_adam")
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments (16-byte aligned)


def _declaration(name, ret="int"):
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declared_and_bound(usim):
    assert _declaration("usim_ppo_params") == ["int act_dim"]
    assert _declaration("usim_ppo_work_floats", "int64_t") == ["int act_dim"]
    assert _declaration("usim_ppo_grad") == ["const usim_policy_net* net", "const usim_ppo_batch* b", "float* work_dev", "float* grad_dev", "float* stats_dev",
                                             "void* stream"]
    assert _declaration("usim_ppo_adam") == ["float* theta_dev", "const float* grad_dev", "float* m_dev", "float* v_dev", "int32_t* step_dev", "int params",
                                             "float lr", "float beta1", "float beta2", "float eps", "float max_grad_norm", "float* stats_dev", "void* stream"]
    L = usim._lib
    S, v, i, f = L.SYMBOLS, C.c_void_p, C.c_int, C.c_float
    assert S["usim_ppo_params"] == (C.c_int, [i]) and S["usim_ppo_work_floats"] == (C.c_int64, [i])
    assert S["usim_ppo_grad"] == (C.c_int, [C.POINTER(L.UsimPolicyNet), C.POINTER(L.UsimPpoBatch), v, v, v, v])
    assert S["usim_ppo_adam"] == (C.c_int, [v, v, v, v, v, i, f, f, f, f, f, v, v])
    for name, value in (("USIM_PPO_STATS", L.PPO_STATS), ("USIM_PPO_WORKGROUPS", L.PPO_WORKGROUPS)):
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", HEADER, flags=re.M)
        assert m and int(m.group(1)) == value, name


def test_batch_struct_matches_the_header(usim, tmp_path):
    src = ('#include "usim.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(usim_ppo_batch), '
           'offsetof(usim_ppo_batch, index_dev), offsetof(usim_ppo_batch, rows), offsetof(usim_ppo_batch, normalize_advantage), offsetof(usim_ppo_batch, clip_range));return 0;}')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    B = usim._lib.UsimPpoBatch
    assert out == [C.sizeof(B), B.index_dev.offset, B.rows.offset, B.normalize_advantage.offset, B.clip_range.offset]


def test_library_exports_them(usim):
    lib = usim._lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(usim._lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    for name in NAMES:
        assert name in exported and getattr(lib, name) is not None
    assert usim.ppo.NativePPO is not None and callable(usim.ppo.flatten_parameters) and "ppo" in usim.__all__
    for method in ("update", "learn", "save", "minibatch_step"):
        assert callable(getattr(usim.ppo.NativePPO, method))


def test_parameter_and_workspace_counts(usim):
    lib = usim._lib.load()
    assert lib.usim_ppo_params(6) == 76941 and lib.usim_ppo_params(7) == 77071
    for A in range(1, 9):
        assert lib.usim_ppo_params(A) == 76032 + 130 * A + 129 == usim.ppo.ppo_params(A)
        assert lib.usim_ppo_work_floats(A) >= usim._lib.PPO_WORKGROUPS * lib.usim_ppo_params(A)
    for bad in (0, -1, 9, 64):
        assert lib.usim_ppo_params(bad) < 0 and lib.usim_ppo_work_floats(bad) < 0


def _net(usim, **kw):
    f = dict({n: P for n, _ in usim._lib.UsimPolicyNet._fields_}, w2_packed=None)
    f.update(kw)
    return usim._lib.UsimPolicyNet(**f)


def _batch(usim, **kw):
    f = dict(obs_dev=P, act_dev=P, old_logp_dev=P, adv_dev=P, ret_dev=P, index_dev=None, rows=64, batch=64, act_dim=6, normalize_advantage=1, clip_range=0.2,
             ent_coef=0.0, vf_coef=0.5, reserved_=0.0)
    f.update(kw)
    return usim._lib.UsimPpoBatch(**f)


def _grad(lib, net, b, work=P, grad=P, stats=P):
    return lib.usim_ppo_grad(None if net is None else C.byref(net), None if b is None else C.byref(b), work, grad, stats, None)


def test_grad_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    net, b = _net(usim), _batch(usim)
    assert _grad(lib, None, b) == INVALID and _grad(lib, net, None) == INVALID
    for name in ("work", "grad", "stats"):
        assert _grad(lib, net, b, **{name: None}) == INVALID, name
    assert _grad(lib, net, b, work=P + 4) == INVALID                      # the workspace off the 16-byte grid
    for name, _ in usim._lib.UsimPolicyNet._fields_:
        if name != "w2_packed":                                           # (ignored by the learner)
            assert _grad(lib, _net(usim, **{name: None}), b) == INVALID, name
    for name in ("obs_dev", "act_dev", "old_logp_dev", "adv_dev", "ret_dev"):
        assert _grad(lib, net, _batch(usim, **{name: None})) == INVALID, name
    for bad in (0, -1, 9, 64):
        assert _grad(lib, net, _batch(usim, act_dim=bad)) == INVALID, bad
    for bad in (0, -5):
        assert _grad(lib, net, _batch(usim, batch=bad)) == INVALID, bad
    assert _grad(lib, net, _batch(usim, rows=63, batch=64)) == INVALID    # rows < batch without an index list
    assert _grad(lib, net, _batch(usim, rows=0, batch=64, index_dev=P)) == INVALID
    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        assert _grad(lib, net, _batch(usim, clip_range=bad)) == INVALID, bad
    for name in ("ent_coef", "vf_coef"):
        for bad in (float("nan"), float("inf")):
            assert _grad(lib, net, _batch(usim, **{name: bad})) == INVALID, (name, bad)


def _adam(lib, theta=P, grad=P, m=P, v=P, step=P, params=1000, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5):
    return lib.usim_ppo_adam(theta, grad, m, v, step, params, lr, beta1, beta2, eps, max_grad_norm, None, None)


def test_adam_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("theta", "grad", "m", "v", "step"):
        assert _adam(lib, **{name: None}) == INVALID, name
    for bad in (0, -7):
        assert _adam(lib, params=bad) == INVALID, bad
    for name in ("lr", "eps"):
        for bad in (-1e-9, float("nan"), float("inf"), float("-inf")):
            assert _adam(lib, **{name: bad}) == INVALID, (name, bad)
    for name in ("beta1", "beta2"):
        for bad in (-0.1, 1.0, float("nan")):
            assert _adam(lib, **{name: bad}) == INVALID, (name, bad)
    assert _adam(lib, max_grad_norm=float("nan")) == INVALID


# ---- the constructor of ppo.NativePPO: every refusal is a ValueError raised before the library (or a device) is touched ----
def _env(action_dim=6, device="cuda:0"):
    return SimpleNamespace(action_dim=action_dim, device=device, num_envs=64)


def _buffer(device="cuda:0", T=32, n=64):
    return SimpleNamespace(device=device, buffer_size=T, n_envs=n, full=True)


def _policy(usim, A=6, pi=(256, 128), vf=(256, 128), obs=19):
    return usim.policy.MlpActorCritic(obs, A, pi, vf)


@pytest.mark.parametrize("make, kw, what", [
    (lambda u: (_env(), _policy(u, pi=(64, 64)), _buffer()), {}, "policy shapes"),
    (lambda u: (_env(), _policy(u, vf=(256, 64)), _buffer()), {}, "policy shapes"),
    (lambda u: (_env(), _policy(u, obs=20), _buffer()), {}, "policy shapes"),
    (lambda u: (_env(), _policy(u, pi=(256,), vf=(256,)), _buffer()), {}, "policy shapes"),
    (lambda u: (_env(), _policy(u, A=9), _buffer()), {}, "policy shapes"),
    (lambda u: (_env(action_dim=7), _policy(u, A=6), _buffer()), {}, "policy shapes"),
    (lambda u: (_env(), _policy(u), _buffer(device="cuda:1")), {}, "buffer is on device"),
    (lambda u: (_env(), _policy(u), _buffer(device="cpu")), {}, "buffer is on device"),
    (lambda u: (_env(), _policy(u), _buffer()), dict(batch_size=32 * 64 + 1), "batch_size"),
    (lambda u: (_env(), _policy(u), _buffer()), dict(batch_size=0), "batch_size"),
    (lambda u: (_env(), _policy(u), _buffer()), dict(n_epochs=0), "n_epochs"),
    (lambda u: (_env(), _policy(u), _buffer()), {}, "policy is on device"),                 # (a CPU module for a cuda:0 environment)
])
def test_constructor_refusals(usim, monkeypatch, make, kw, what):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(usim._lib, "load", no_library)
    env, policy, buffer = make(usim)
    with pytest.raises(ValueError, match=what):
        usim.ppo.NativePPO(env, policy, None, buffer, **kw)


def test_a_collector_built_before_flattening_is_refused(usim, monkeypatch):
    monkeypatch.setattr(usim._lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    with pytest.raises(ValueError, match="flatten_parameters"):
        usim.ppo.NativePPO(_env(device="cpu"), _policy(usim), None, _buffer(device="cpu"), collector=SimpleNamespace(pack=lambda: None))


def test_flatten_parameters_on_a_cpu_module(usim):
    torch.manual_seed(3)
    for A in (6, 7):
        m = _policy(usim, A)
        with torch.no_grad():
            m.log_std.uniform_(-0.5, 0.3)
        before = {k: v.detach().clone() for k, v in m.named_parameters()}
        obs = torch.randn(37, 19)
        out_before = [t.detach().clone() for t in m(obs)]
        theta = usim.ppo.flatten_parameters(m)
        assert theta.dtype == torch.float32 and theta.is_contiguous() and theta.numel() == 76032 + 130 * A + 129
        params, o = dict(m.named_parameters()), 0
        assert len(params) == 13 and all(isinstance(p, torch.nn.Parameter) and p.requires_grad for p in params.values())
        for name, path in usim.ppo.FIELDS:                                # the header's order, every view where the order puts it
            p = params[path]
            assert p.data_ptr() == theta.data_ptr() + 4 * o and p.is_contiguous(), name
            assert torch.equal(p.detach(), before[path]) and torch.equal(theta[o:o + p.numel()].view(p.shape), before[path]), name
            o += p.numel()
        assert o == theta.numel()
        assert [n for n, _ in usim.ppo.FIELDS] == [n for n, _ in usim._lib.UsimPolicyNet._fields_][:13]
        out_after = m(obs)
        assert all(torch.equal(a, b) for a, b in zip(out_before, out_after))          # bit for bit
        with torch.no_grad():
            theta.mul_(0.5)                                               # a write through the block is a write to the module ...
        assert torch.equal(m.action_net.weight.detach(), 0.5 * before["action_net.weight"])
        with torch.no_grad():
            m.value_net.bias.fill_(0.25)                                  # ... and the other way round
        assert theta[-A - 1] == 0.25
        assert usim.ppo.flatten_parameters(m) is theta                    # idempotent
        sd = m.to_sb3_state_dict()                                        # the checkpoint writer reads the same memory
        assert torch.equal(sd["mlp_extractor.value_net.2.weight"], m.value_net_body[2].weight.detach())


# ---- one construction of usim_policy_net, one learner core ----
@pytest.mark.parametrize("A", [6, 7])
def test_policy_net_holds_the_addresses_of_the_parameters_in_the_headers_order(usim, A):
    m = _policy(usim, A)
    packed = torch.zeros(8)
    for flat in (False, True):                                            # before and after flatten_parameters (which re-seats every parameter)
        if flat:
            usim.ppo.flatten_parameters(m)
        net, params = usim.policy.policy_net(m), dict(m.named_parameters())
        for name, path in usim.ppo.FIELDS:
            assert getattr(net, name) == params[path].data_ptr(), (flat, name)
        ptr = lambda t: t.data_ptr()                                      # the construction FusedRollout spelled out attribute by attribute until now
        pn, vb = m.policy_net, m.value_net_body
        want = (ptr(pn[0].weight), ptr(pn[0].bias), ptr(pn[2].weight), ptr(pn[2].bias), ptr(m.action_net.weight), ptr(m.action_net.bias),
                ptr(vb[0].weight), ptr(vb[0].bias), ptr(vb[2].weight), ptr(vb[2].bias), ptr(m.value_net.weight), ptr(m.value_net.bias), ptr(m.log_std))
        names = [n for n, _ in usim._lib.UsimPolicyNet._fields_]
        assert names[13:] == ["w2_packed"] and tuple(getattr(net, n) for n in names[:13]) == want and len(set(want)) == 13
        assert net.w2_packed is None and usim.policy.policy_net(m, packed).w2_packed == packed.data_ptr()
        assert tuple(getattr(usim.policy.policy_net(m, packed), n) for n in names[:13]) == want
    assert usim.policy.FIELDS is usim.ppo.FIELDS is usim.learner.FIELDS


class _NoCalls:
    """stands where the library stands: any call is a failure of the test"""

    def usim_ppo_work_floats(self, A):
        return 16

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called by a constructor")


def test_native_ppo_and_native_bc_stand_on_one_core_and_one_block(usim, monkeypatch):
    monkeypatch.setattr(usim._lib, "load", lambda: _NoCalls())
    A, policy = 6, _policy(usim)
    bc = usim.NativeBC(policy, usim.policy.DeviceVecNormalize(1, 19, device="cpu", training=False), usim.DemoBuffer(40, A, "cpu"), seed=3)
    env = SimpleNamespace(action_dim=A, device="cpu", num_envs=8)
    ppo = usim.ppo.NativePPO(env, policy, usim.policy.DeviceVecNormalize(8, 19, device="cpu"), usim.policy.DeviceRolloutBuffer(4, 8, 19, A, device="cpu"), seed=3)
    core = usim.learner.FlatLearner
    assert isinstance(bc, core) and isinstance(ppo, core) and usim.ppo.NativePPO.__mro__[1] is core and usim.NativeBC.__mro__[1] is core
    assert ppo.theta is bc.theta and usim.ppo._is_flat(policy, ppo.theta) and ppo.params == bc.params == usim.ppo.ppo_params(A)
    names = [n for n, _ in usim._lib.UsimPolicyNet._fields_]
    assert [getattr(ppo._net, n) for n in names] == [getattr(bc._net, n) for n in names] and ppo._net.pi_w1 == ppo.theta.data_ptr()
    for ln, rows in ((ppo, 32), (bc, 40)):                                # what the core allocates, under the names the tools and tests read
        assert all(getattr(ln, k).shape == (ln.params,) and getattr(ln, k).dtype == torch.float32 and not getattr(ln, k).any() for k in ("grad", "exp_avg", "exp_avg_sq"))
        assert ln.step_count.dtype == torch.int32 and ln.step_count.tolist() == [0] and ln._index.dtype == torch.int32 and ln._index.numel() == rows
        assert ln.stats.numel() == ln.first_stats.numel() == usim._lib.PPO_STATS and ln._work.numel() == 16 and ln.act_dim == A and ln.device == torch.device("cpu")
        assert ln.generator.initial_seed() == 3 and all(k in vars(ln) for k in ("theta", "params", "lib", "_net", "policy", "n_epochs", "adam_eps", "max_grad_norm"))
