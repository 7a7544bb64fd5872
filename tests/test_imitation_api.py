"""usim_bc_grad on the host side -- declared in include/usim.h, bound by _lib.SYMBOLS, exported by the library built here, its argument checks answering
USIM_ERR_INVALID before anything is enqueued (NULL or made-up pointers that no kernel may ever see) -- and the device-free side of imitation.py: DemoBuffer's
ring on CPU tensors, every ValueError of NativeBC, PlannerExpert and DAggerTrainer with stand-in objects.  Runs without a GPU."""
import copy
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
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments (16-byte aligned)


def test_declared_and_bound(usim):
    m = re.search(r"\bint\s+usim_bc_grad\s*\(([^;]*)\)\s*;", HEADER)
    assert m, "usim_bc_grad is not declared in include/usim.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ["const usim_policy_net* net", "const usim_bc_batch* b", "float* work_dev",
                                                                              "float* grad_dev", "float* stats_dev", "void* stream"]
    L, v = usim._lib, C.c_void_p
    assert L.SYMBOLS["usim_bc_grad"] == (C.c_int, [C.POINTER(L.UsimPolicyNet), C.POINTER(L.UsimBcBatch), v, v, v, v])
    for name, value in (("USIM_BC_NLL", L.BC_NLL), ("USIM_BC_MSE", L.BC_MSE)):
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", HEADER, flags=re.M)
        assert m and int(m.group(1)) == value, name
    assert (L.BC_NLL, L.BC_MSE) == (0, 1) and usim.imitation.LOSSES == {"nll": 0, "mse": 1}
    nm = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "usim_bc_grad" in set(re.findall(r" T (usim_[a-z_]+)", nm)) and L.load().usim_bc_grad is not None
    for name in ("imitation", "DemoBuffer", "NativeBC", "PolicyExpert", "PlannerExpert", "DAggerTrainer", "distill"):
        assert name in usim.__all__ and getattr(usim, name) is not None, name
    for method in ("train", "minibatch_step", "fit_normalizer"):
        assert callable(getattr(usim.NativeBC, method))


def test_batch_struct_matches_the_header(usim, tmp_path):
    fields = ("obs_dev", "act_dev", "value_dev", "index_dev", "rows", "batch", "act_dim", "loss", "ent_coef", "vf_coef", "reserved_")
    src = ('#include "usim.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(usim_bc_batch));'
           + "".join(f'printf(" %zu", offsetof(usim_bc_batch, {f}));' for f in fields) + 'printf("\\n");return 0;}')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    B = usim._lib.UsimBcBatch
    assert out == [C.sizeof(B)] + [getattr(B, f).offset for f in fields]
    assert [n for n, _ in B._fields_] == list(fields)


def _net(usim, **kw):
    f = dict({n: P for n, _ in usim._lib.UsimPolicyNet._fields_}, w2_packed=None)
    f.update(kw)
    return usim._lib.UsimPolicyNet(**f)


def _batch(usim, **kw):
    f = dict(obs_dev=P, act_dev=P, value_dev=P, index_dev=None, rows=64, batch=64, act_dim=6, loss=0, ent_coef=1e-3, vf_coef=0.5)
    f.update(kw)
    return usim._lib.UsimBcBatch(**f)


def _grad(lib, net, b, work=P, grad=P, stats=P):
    return lib.usim_bc_grad(None if net is None else C.byref(net), None if b is None else C.byref(b), work, grad, stats, None)


def test_grad_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    net, b = _net(usim), _batch(usim)
    assert _grad(lib, None, b) == INVALID and _grad(lib, net, None) == INVALID
    for name in ("work", "grad", "stats"):
        assert _grad(lib, net, b, **{name: None}) == INVALID, name
    assert _grad(lib, net, b, work=P + 4) == INVALID and _grad(lib, net, b, work=P + 8) == INVALID      # the workspace off the 16-byte grid
    for name, _ in usim._lib.UsimPolicyNet._fields_:
        if name != "w2_packed":
            assert _grad(lib, _net(usim, **{name: None}), b) == INVALID, name
    for name in ("obs_dev", "act_dev"):
        assert _grad(lib, net, _batch(usim, **{name: None})) == INVALID, name
    for bad in (0, -1, 9, 64):
        assert _grad(lib, net, _batch(usim, act_dim=bad)) == INVALID, bad
    for bad in (0, -5):
        assert _grad(lib, net, _batch(usim, batch=bad)) == INVALID, bad
    assert _grad(lib, net, _batch(usim, rows=63, batch=64)) == INVALID    # rows < batch without an index list
    assert _grad(lib, net, _batch(usim, rows=0, batch=64, index_dev=P)) == INVALID
    for bad in (-1, 2, 7):
        assert _grad(lib, net, _batch(usim, loss=bad)) == INVALID, bad
    for name in ("ent_coef", "vf_coef"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert _grad(lib, net, _batch(usim, **{name: bad})) == INVALID, (name, bad)
    # (a NULL value_dev is no refusal: it means no value term -- that call would launch, so it is the GPU tests')


# ---- DemoBuffer on CPU tensors ----
def _rows(lo, hi, A=3):
    i = torch.arange(lo, hi, dtype=torch.float32)
    return i[:, None] + torch.arange(19, dtype=torch.float32) / 100, -i[:, None] - torch.arange(A, dtype=torch.float32) / 10, 0.5 * i


def test_demo_buffer_ring_order_and_wrap_around(usim):
    buf = usim.DemoBuffer(10, 3, "cpu")
    assert buf.rows == 0 and buf.has_value is None and buf.capacity == 10
    obs, act, val = _rows(0, 4)
    buf.add(obs, act, val)
    assert buf.rows == 4 and buf.has_value is True
    buf.add(*_rows(4, 8))
    o, a, v = buf.ordered()
    assert buf.rows == 8 and all(torch.equal(x, y) for x, y in zip((o, a, v), _rows(0, 8)))
    assert torch.equal(buf.obs[:8], o)                                       # not wrapped: the storage is in order
    buf.add(*_rows(8, 14))                                                    # wraps: rows 0 .. 3 are overwritten
    assert buf.rows == 10 and buf.pos == 4 and buf.total == 14
    assert all(torch.equal(x, y) for x, y in zip(buf.ordered(), _rows(4, 14)))
    assert torch.equal(buf.obs[:4], _rows(10, 14)[0]) and torch.equal(buf.obs[4:], _rows(4, 10)[0])
    buf.add(*_rows(14, 39))                                                   # more rows than the ring holds: the last ten stay, oldest first from `pos`
    assert buf.rows == 10 and buf.pos == 39 % 10 and all(torch.equal(x, y) for x, y in zip(buf.ordered(), _rows(29, 39)))
    buf.add(*_rows(39, 49))                                                   # exactly one ring
    assert all(torch.equal(x, y) for x, y in zip(buf.ordered(), _rows(39, 49)))
    buf.clear()
    assert buf.rows == 0 and buf.pos == 0 and buf.has_value is None
    obs, act, _ = _rows(0, 6)
    buf.add_block(obs.view(3, 2, 19), act.view(3, 2, 3))                      # step-major, environment-minor; no values
    o, a, v = buf.ordered()
    assert buf.rows == 6 and buf.has_value is False and v is None and torch.equal(o, obs) and torch.equal(a, act)
    buf.clear()
    blk = _rows(0, 6)
    buf.add_block(blk[0].view(3, 2, 19), blk[1].view(3, 2, 3), blk[2].view(3, 2))
    assert all(torch.equal(x, y) for x, y in zip(buf.ordered(), blk))


def test_demo_buffer_refusals(usim):
    for bad in ((0, 3), (4, 0)):
        with pytest.raises(ValueError, match="at least 1"):
            usim.DemoBuffer(*bad, "cpu")
    buf = usim.DemoBuffer(8, 3, "cpu")
    obs, act, val = _rows(0, 4)
    for args in ((obs[:, :18], act, val), (obs, act[:, :2], val), (obs, act, val[:3]), (obs[:3], act, None)):
        with pytest.raises(ValueError, match="add:"):
            buf.add(*args)
    buf.add(obs, act, val)
    with pytest.raises(ValueError, match="for all of its rows or for none"):
        buf.add(obs, act)
    assert buf.rows == 4


# ---- NativeBC: every refusal is a ValueError raised before the library is touched ----
def _policy(usim, A=6, pi=(256, 128), vf=(256, 128), obs=19):
    return usim.policy.MlpActorCritic(obs, A, pi, vf)


def _demos(A=6, device="cpu", rows=0, capacity=64, obs_dim=19):
    return SimpleNamespace(act_dim=A, device=device, rows=rows, capacity=capacity, obs_dim=obs_dim, has_value=None)


@pytest.mark.parametrize("make, kw, what", [
    (lambda u: (_policy(u, pi=(64, 64)), _demos()), {}, "policy shapes"),
    (lambda u: (_policy(u, vf=(256, 64)), _demos()), {}, "policy shapes"),
    (lambda u: (_policy(u, obs=20), _demos()), {}, "policy shapes"),
    (lambda u: (_policy(u, A=9), _demos(A=9)), {}, "policy shapes"),
    (lambda u: (_policy(u, A=6), _demos(A=7)), {}, "is not the buffer's"),
    (lambda u: (_policy(u), _demos(device="cuda:0")), {}, "policy is on device"),
    (lambda u: (_policy(u), _demos(obs_dim=20)), {}, "observations of 20 words"),
    (lambda u: (_policy(u), _demos()), dict(loss="huber"), "loss must be one of"),
    (lambda u: (_policy(u), _demos()), dict(batch_size=0), "batch_size"),
    (lambda u: (_policy(u), _demos()), dict(n_epochs=0), "n_epochs"),
])
def test_native_bc_constructor_refusals(usim, monkeypatch, make, kw, what):
    monkeypatch.setattr(usim._lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded before the arguments were checked")))
    policy, demos = make(usim)
    with pytest.raises(ValueError, match=what):
        usim.NativeBC(policy, None, demos, **kw)


class _NoCalls:
    """stands where the library stands: any call is a failure of the test"""

    def usim_ppo_work_floats(self, A):
        return 16

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called before the arguments were checked")


def test_native_bc_train_refusals(usim, monkeypatch):
    monkeypatch.setattr(usim._lib, "load", lambda: _NoCalls())
    buf = usim.DemoBuffer(64, 6, "cpu")
    vn = usim.policy.DeviceVecNormalize(1, 19, device="cpu", training=False)
    bc = usim.NativeBC(_policy(usim), vn, buf, batch_size=9)
    with pytest.raises(ValueError, match="buffer is empty"):
        bc.train()
    with pytest.raises(ValueError, match="buffer is empty"):
        bc.fit_normalizer()
    buf.add(torch.zeros(8, 19), torch.zeros(8, 6))
    with pytest.raises(ValueError, match="batch_size 9 outside 1 .. the buffer's 8 rows"):
        bc.train()
    assert bc.history == []
    usim.NativeBC(_policy(usim), vn, buf, vf_coef=0.5)                        # vf_coef > 0 over a buffer without value targets is no refusal


def test_native_bc_flattens_and_fit_normalizer_sets_the_statistics(usim, monkeypatch):
    monkeypatch.setattr(usim._lib, "load", lambda: _NoCalls())
    torch.manual_seed(1)
    buf = usim.DemoBuffer(50, 6, "cpu")
    obs = torch.randn(40, 19) * 3 + 1
    buf.add(obs, torch.zeros(40, 6))
    vn = usim.policy.DeviceVecNormalize(1, 19, device="cpu", training=True)
    policy = _policy(usim)
    bc = usim.NativeBC(policy, vn, buf)
    assert usim.ppo._is_flat(policy, bc.theta) and usim.ppo.flatten_parameters(policy) is bc.theta and bc.theta.numel() == usim.ppo.ppo_params(6)
    bc.fit_normalizer()
    o = obs.double()
    assert torch.equal(vn.obs_mean, o.mean(0)) and torch.equal(vn.obs_var, o.var(0, unbiased=False)) and float(vn._obs_count) == 40.0
    before = vn.obs_mean.clone()
    out = vn.normalize_obs(obs, update=False)                                 # normalising for train() reads the statistics and leaves them alone
    assert torch.equal(vn.obs_mean, before) and float(vn._obs_count) == 40.0 and vn.training is True
    assert out.dtype == torch.float32 and float(out.abs().max()) <= 10.0


def test_normalize_obs_update_false_only_reads_the_statistics(usim):
    torch.manual_seed(5)
    vn = usim.policy.DeviceVecNormalize(4, 19, device="cpu", training=True)
    vn.normalize_obs(torch.randn(32, 19) * 2 + 0.5)                           # statistics that are not the identity
    obs = torch.randn(8, 19) * 30                                             # (wide enough for the clip to act)
    kept = (vn.obs_mean.clone(), vn.obs_var.clone(), vn._obs_count.clone())
    frozen = copy.deepcopy(vn)
    frozen.training = False
    out = vn.normalize_obs(obs, update=False)
    assert all(torch.equal(a, b) for a, b in zip((vn.obs_mean, vn.obs_var, vn._obs_count), kept)) and vn.training is True
    assert out.dtype == torch.float32 and torch.equal(out, frozen.normalize_obs(obs)) and float(out.abs().max()) == 10.0
    assert all(torch.equal(a, b) for a, b in zip((frozen.obs_mean, frozen.obs_var, frozen._obs_count), kept))
    twin = copy.deepcopy(vn)
    out_none, out_default = vn.normalize_obs(obs, update=None), twin.normalize_obs(obs)     # None: as self.training says -- today's call, which updates first
    assert float(vn._obs_count) == float(kept[2]) + 8 and not torch.equal(vn.obs_mean, kept[0]) and not torch.equal(vn.obs_var, kept[1])
    assert torch.equal(out_none, out_default) and torch.equal(vn.obs_mean, twin.obs_mean) and not torch.equal(out_none, out)
    count = float(frozen._obs_count)
    frozen.normalize_obs(obs, update=None)                                    # ... and leaves a frozen object alone
    assert float(frozen._obs_count) == count and torch.equal(frozen.obs_mean, kept[0])


# ---- PlannerExpert and DAggerTrainer with stand-ins ----
def _env(A=6, device="cpu", n=4):
    return SimpleNamespace(action_dim=A, device=device, num_envs=n, action_space=SimpleNamespace(low=-np.ones(A, np.float32), high=np.ones(A, np.float32)))


def _learner(A=6, device="cpu", capacity=64):
    return SimpleNamespace(act_dim=A, device=device, demos=SimpleNamespace(capacity=capacity, rows=0))


def test_planner_expert_refuses_another_environment(usim):
    real, other = _env(), _env()
    planner = SimpleNamespace(real=real, groups=4, plan=lambda: torch.zeros(4, 6), restart=torch.zeros(4, dtype=torch.uint8))
    expert = usim.PlannerExpert(planner)
    expert.check_env(real)
    with pytest.raises(ValueError, match="must be that environment"):
        expert.check_env(other)
    with pytest.raises(ValueError, match="must be that environment"):
        usim.DAggerTrainer(other, expert, _learner(), rollout_steps=4)
    with pytest.raises(ValueError, match="labels the 4 environments"):
        expert.label(torch.zeros(5, 19))
    act, value = expert.label(torch.zeros(4, 19))
    assert tuple(act.shape) == (4, 6) and value is None
    expert.after_step(torch.tensor([0, 1, 0, 1], dtype=torch.uint8))
    assert planner.restart.tolist() == [0, 1, 0, 1]
    assert usim.DAggerTrainer(real, expert, _learner(), rollout_steps=4).round_index == 0


@pytest.mark.parametrize("make, kw, what", [
    (lambda: (_env(), SimpleNamespace(label=lambda o: None), _learner()), dict(rollout_steps=0), "rollout_steps"),
    (lambda: (_env(), SimpleNamespace(), _learner()), dict(rollout_steps=4), "an expert has label"),
    (lambda: (_env(), SimpleNamespace(label=lambda o: None), _learner()), dict(rollout_steps=4, beta=0.5), "beta must be a callable"),
    (lambda: (_env(A=7), SimpleNamespace(label=lambda o: None), _learner()), dict(rollout_steps=4), "action_dim 7"),
    (lambda: (_env(device="cuda:0"), SimpleNamespace(label=lambda o: None), _learner()), dict(rollout_steps=4), "is on device"),
    (lambda: (_env(), SimpleNamespace(label=lambda o: None), _learner(capacity=15)), dict(rollout_steps=4), "below one round's 16 rows"),
])
def test_dagger_trainer_refusals(usim, make, kw, what):
    env, expert, learner = make()
    with pytest.raises(ValueError, match=what):
        usim.DAggerTrainer(env, expert, learner, **kw)


def test_dagger_round_refuses_a_beta_outside_the_unit_interval(usim):
    env = _env()
    env.reset_tensor = lambda: (_ for _ in ()).throw(AssertionError("the environment was touched before beta was checked"))
    for bad in (-0.1, 1.5, float("nan")):
        tr = usim.DAggerTrainer(env, SimpleNamespace(label=lambda o: None), _learner(), rollout_steps=4, beta=lambda r, b=bad: b)
        with pytest.raises(ValueError, match="outside \\[0, 1\\]"):
            tr.round()
    assert usim.imitation._default_beta(0) == 1.0 and usim.imitation._default_beta(1) == 0.0 and usim.imitation._default_beta(7) == 0.0
