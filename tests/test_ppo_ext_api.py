"""What clip_range_vf, target_kl and resume add on the host side: the four fields appended to usim_ppo_batch and usim_ppo_adam_gated are declared in
include/usim.h, mirrored by _lib and exported; the new refusals answer USIM_ERR_INVALID before anything is enqueued (made-up pointers that no kernel may ever
see); ppo.NativePPO refuses bad values before any library call; the Adam-state conversion is device-free and round-trips bit for bit; a checkpoint written by
one learner is restored in place by another -- here on CPU tensors, which the learner's host side never distinguishes from device tensors (no kernel runs)."""
import ctypes as C
import io
import re
import shutil
import subprocess
import zipfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
P = 0x1000                                                                # never dereferenced (16-byte aligned)
NEW_FIELDS = ("old_value_dev", "gate_dev", "clip_range_vf", "target_kl")


# ================================================================ the C ABI ================================================================
def test_new_batch_fields_match_the_header(usim, tmp_path):
    fields = ", ".join(f"offsetof(usim_ppo_batch, {n})" for n in ("reserved_",) + NEW_FIELDS)
    src = ('#include "usim.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(usim_ppo_batch), '
           + fields + ', (int)USIM_PPO_GATE_WORDS);return 0;}')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    B = usim._lib.UsimPpoBatch
    assert out == [C.sizeof(B), B.reserved_.offset] + [getattr(B, n).offset for n in NEW_FIELDS] + [usim._lib.PPO_GATE_WORDS]
    names = [n for n, _ in B._fields_]
    assert tuple(names[-4:]) == NEW_FIELDS and names[-5] == "reserved_"    # appended, in the header's order
    assert out[1] == 76 and out[0] == 104                                  # every earlier field where it was: reserved_ is the last of the old 80 bytes
    b = B(P, P, P, P, P, None, 64, 64, 6, 1, 0.2, 0.0, 0.5, 0.0)           # an existing caller: the new fields are zero-filled, that is "off"
    assert b.old_value_dev is None and b.gate_dev is None and b.clip_range_vf == 0.0 and b.target_kl == 0.0


def test_adam_gated_is_declared_bound_and_exported(usim):
    m = re.search(r"\bint\s+usim_ppo_adam_gated\s*\(([^;]*)\)\s*;", HEADER)
    assert m, "usim_ppo_adam_gated is not declared in include/usim.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["float* theta_dev", "const float* grad_dev", "float* m_dev", "float* v_dev", "int32_t* step_dev", "int params", "float lr", "float beta1",
                    "float beta2", "float eps", "float max_grad_norm", "float* stats_dev", "int32_t* gate_dev", "void* stream"]      # gate_dev in front of stream
    v, i, f = C.c_void_p, C.c_int, C.c_float
    assert usim._lib.SYMBOLS["usim_ppo_adam_gated"] == (C.c_int, [v, v, v, v, v, i, f, f, f, f, f, v, v, v])
    nm = subprocess.run(["nm", "-D", "--defined-only", str(usim._lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "usim_ppo_adam_gated" in set(re.findall(r" T (usim_[a-z_]+)", nm)) and usim._lib.load().usim_ppo_adam_gated is not None
    for method in ("save_checkpoint", "load_checkpoint", "set_checkpointing", "current_clip_range", "current_clip_range_vf"):
        assert callable(getattr(usim.ppo.NativePPO, method))


def _grad(usim, **kw):
    L = usim._lib
    net = L.UsimPolicyNet(**dict({n: P for n, _ in L.UsimPolicyNet._fields_}, w2_packed=None))
    f = dict(obs_dev=P, act_dev=P, old_logp_dev=P, adv_dev=P, ret_dev=P, index_dev=None, rows=64, batch=64, act_dim=6, normalize_advantage=1, clip_range=0.2,
             ent_coef=0.0, vf_coef=0.5, reserved_=0.0, old_value_dev=P, gate_dev=P, clip_range_vf=0.2, target_kl=0.01)
    f.update(kw)
    work = f.pop("work", P)
    return L.load().usim_ppo_grad(C.byref(net), C.byref(L.UsimPpoBatch(**f)), work, P, P, None)


def test_grad_refuses_the_new_fields_before_it_launches(usim):
    """(a valid set of the new fields cannot be shown here: that call would launch.  Each refusal below differs from it in one field; the last line shows that
    the helper's other arguments are refused for their own reason only)"""
    for name in ("clip_range_vf", "target_kl"):
        for bad in (-0.1, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert _grad(usim, **{name: bad}) == INVALID, (name, bad)
    assert _grad(usim, old_value_dev=None) == INVALID                      # clip_range_vf > 0 without the old values
    assert _grad(usim, gate_dev=None) == INVALID                           # target_kl > 0 without a gate
    assert _grad(usim, old_value_dev=None, gate_dev=None) == INVALID
    assert _grad(usim, work=P + 4) == INVALID


def test_adam_gated_refuses_like_adam(usim):
    lib = usim._lib.load()
    ok = dict(theta=P, grad=P, m=P, v=P, step=P, params=1000, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5)

    def call(gate, **kw):
        a = dict(ok, **kw)
        return lib.usim_ppo_adam_gated(a["theta"], a["grad"], a["m"], a["v"], a["step"], a["params"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["max_grad_norm"],
                                       None, gate, None)
    for gate in (None, P):
        for name in ("theta", "grad", "m", "v", "step"):
            assert call(gate, **{name: None}) == INVALID, name
        assert call(gate, params=0) == INVALID and call(gate, lr=float("nan")) == INVALID and call(gate, beta2=1.0) == INVALID and call(gate, eps=-1.0) == INVALID


# ================================================================ ppo.NativePPO: refusals ================================================================
def _cpu_learner(usim, A=6, seed=0, T=4, n=8, **kw):
    """a NativePPO whose tensors live on the CPU: the host side (checkpoints, conversions, argument checks) without a device"""
    torch.manual_seed(seed)
    policy = usim.policy.MlpActorCritic(19, A)
    with torch.no_grad():
        policy.log_std.uniform_(-0.5, 0.3)
    env = SimpleNamespace(action_dim=A, device="cpu", num_envs=n, action_space=SimpleNamespace(low=-np.ones(A, np.float32), high=np.ones(A, np.float32)))
    vn = usim.policy.DeviceVecNormalize(n, 19, device="cpu")
    buf = usim.policy.DeviceRolloutBuffer(T, n, 19, A, device="cpu")
    return usim.ppo.NativePPO(env, policy, vn, buf, None, seed=seed, **kw)


@pytest.mark.parametrize("kw, what", [
    (dict(clip_range_vf=0.0), "clip_range_vf"), (dict(clip_range_vf=-0.2), "clip_range_vf"), (dict(clip_range_vf=float("nan")), "clip_range_vf"),
    (dict(clip_range_vf=float("inf")), "clip_range_vf"), (dict(clip_range_vf=lambda progress: -0.1 * progress), "clip_range_vf"),
    (dict(target_kl=0.0), "target_kl"), (dict(target_kl=-0.01), "target_kl"), (dict(target_kl=float("nan")), "target_kl"), (dict(target_kl=float("inf")), "target_kl"),
])
def test_constructor_refuses_bad_values_before_the_library(usim, monkeypatch, kw, what):
    monkeypatch.setattr(usim._lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded before the arguments were checked")))
    with pytest.raises(ValueError, match=what):
        _cpu_learner(usim, **kw)


def test_schedules_and_defaults(usim):
    plain = _cpu_learner(usim)
    assert plain.clip_range_vf is None and plain.target_kl is None and plain.current_clip_range_vf() is None and plain.current_clip_range() == 0.2
    assert plain.gate.dtype == torch.int32 and plain.gate.numel() == usim._lib.PPO_GATE_WORDS and not plain.gate.any() and plain.last_update == {}
    ln = _cpu_learner(usim, clip_range=lambda p: 0.2 * p, clip_range_vf=lambda p: 0.4 * p, target_kl=0.03)
    ln.progress_remaining = 0.5
    assert ln.current_clip_range() == pytest.approx(0.1) and ln.current_clip_range_vf() == pytest.approx(0.2) and ln.target_kl == 0.03
    ln.progress_remaining = 0.0                                           # a schedule that reaches zero is refused where it does, before the library call
    with pytest.raises(ValueError, match="clip_range_vf"):
        ln.current_clip_range_vf()
    data = _cpu_learner(usim, clip_range_vf=0.3, target_kl=0.02, n_epochs=3, batch_size=16).checkpoint_data()
    assert data["clip_range_vf"] == 0.3 and data["target_kl"] == 0.02 and data["n_epochs"] == 3 and data["batch_size"] == 16 and data["learning_rate"] == 3e-4
    assert data["num_timesteps"] == 0 and data["n_steps"] == 4 and data["n_envs"] == 8
    assert (plain.checkpoint_every, plain.checkpoint_dir, plain.name_prefix) == (None, "./checkpoints", "rl_model")      # a new learner: no periodic save
    plain.set_checkpointing(512, "ck", name_prefix="tracking")
    assert (plain.checkpoint_every, plain.checkpoint_dir, plain.name_prefix) == (512, "ck", "tracking")
    for bad in (0, -64):
        with pytest.raises(ValueError, match="checkpoint_every"):
            plain.set_checkpointing(bad)


# ================================================================ Adam state <-> flat block ================================================================
@pytest.mark.parametrize("A", [6, 7])
def test_adam_state_round_trips_bit_for_bit(usim, A):
    ppo = usim.ppo
    names = list(usim.policy.MlpActorCritic(19, A).state_dict())
    n = ppo.ppo_params(A)
    g = torch.Generator().manual_seed(A)
    m, v = torch.randn(n, generator=g), torch.rand(n, generator=g)
    opt = ppo.adam_state_from_flat(m, v, 41, names, A, lr=1e-4, eps=1e-5)
    assert sorted(opt["state"]) == list(range(13)) and opt["param_groups"][0]["params"] == list(range(13)) and opt["param_groups"][0]["lr"] == 1e-4
    shapes = dict(zip((path for _, path in ppo.FIELDS), ppo._field_shapes(A)))
    assert all(tuple(opt["state"][i]["exp_avg"].shape) == shapes[name] and opt["state"][i]["step"] == 41 for i, name in enumerate(names))
    m2, v2, step = ppo.adam_state_to_flat(opt, names, A)
    assert step == 41 and torch.equal(m2.view(torch.int32), m.view(torch.int32)) and torch.equal(v2.view(torch.int32), v.view(torch.int32))
    o = 0                                                                 # FIELDS order in the flat block, state-dict order in the optimizer
    for _, path in ppo.FIELDS:
        e = opt["state"][names.index(path)]["exp_avg"]
        assert torch.equal(e.reshape(-1), m[o:o + e.numel()])
        o += e.numel()
    assert o == n
    # the file format: through torch.save / torch.load(weights_only=True), and with `step` as newer torch writes it -- a 0-d tensor
    buf = io.BytesIO()
    torch.save(opt, buf)
    back = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=True)
    for st in back["state"].values():
        st["step"] = torch.tensor(41.0)
    m3, v3, step3 = ppo.adam_state_to_flat(back, names, A)
    assert step3 == 41 and isinstance(step3, int) and torch.equal(m3, m) and torch.equal(v3, v)
    # step 0: a fresh optimizer has no state; it comes back as zero moments
    fresh = ppo.adam_state_from_flat(m, v, 0, names, A)
    assert fresh["state"] == {}
    m0, v0, step0 = ppo.adam_state_to_flat(fresh, names, A)
    assert step0 == 0 and not m0.any() and not v0.any() and m0.numel() == n
    # refusals
    uneven = ppo.adam_state_from_flat(m, v, 41, names, A)
    uneven["state"][5]["step"] = 40
    with pytest.raises(ValueError, match="steps differ"):
        ppo.adam_state_to_flat(uneven, names, A)
    with pytest.raises(ValueError, match="optimizer state"):
        ppo.adam_state_to_flat(opt, names, A + 1)                         # another action dimension: the moments' shapes are not the parameters'
    short = ppo.adam_state_from_flat(m, v, 41, names, A)
    del short["state"][12]
    with pytest.raises(ValueError, match="optimizer state"):
        ppo.adam_state_to_flat(short, names, A)


# ================================================================ save_checkpoint / load_checkpoint ================================================================
def _fill(ln, seed):
    """a learner in the middle of a run: moments, a step count, statistics and running returns that are nobody's initial values"""
    g = torch.Generator().manual_seed(seed)
    ln.exp_avg.copy_(torch.randn(ln.params, generator=g)); ln.exp_avg_sq.copy_(torch.rand(ln.params, generator=g)); ln.step_count.fill_(17)
    vn = ln.vecnorm
    vn.obs_mean.copy_(torch.randn(19, generator=g, dtype=torch.float64)); vn.obs_var.copy_(torch.rand(19, generator=g, dtype=torch.float64) + 0.5)
    vn._obs_count.fill_(4096.0001); vn.ret_mean.fill_(0.37); vn.ret_var.fill_(2.5); vn._ret_count.fill_(4032.0001)
    vn.returns.copy_(torch.randn(vn.returns.numel(), generator=g, dtype=torch.float64))
    ln.num_timesteps = 12345


VN_TENSORS = ("obs_mean", "obs_var", "_obs_count", "ret_mean", "ret_var", "_ret_count")


def test_checkpoint_round_trip_in_place(usim, tmp_path):
    a, b = _cpu_learner(usim, seed=1, clip_range_vf=0.2, target_kl=0.05), _cpu_learner(usim, seed=2)
    _fill(a, 1)
    assert not torch.equal(a.theta, b.theta)
    paths = a.save_checkpoint(tmp_path / "models", "tracking")
    assert [p.name for p in paths] == ["tracking.zip", "vec_normalize_tracking.pkl"] and all(p.exists() for p in paths)      # src/rl.py:119-120's names
    sd, data = usim.policy.load_sb3_zip(paths[0])
    assert data["num_timesteps"] == 12345 and data["clip_range_vf"] == pytest.approx(0.2) and data["target_kl"] == 0.05 and "policy_kwargs" in data
    assert all(torch.equal(sd[k], v) for k, v in a.policy.to_sb3_state_dict().items())
    with zipfile.ZipFile(paths[0]) as z:
        opt = torch.load(io.BytesIO(z.read("policy.optimizer.pth")), map_location="cpu", weights_only=True)
    assert len(opt["state"]) == 13 and opt["state"][0]["step"] == 17
    ptrs = [t.data_ptr() for t in (b.theta, b.exp_avg, b.exp_avg_sq, b.step_count, b.vecnorm.returns)] + [getattr(b.vecnorm, k).data_ptr() for k in VN_TENSORS] + \
           [p.data_ptr() for p in b.policy.parameters()]
    b.vecnorm.returns.fill_(3.0)
    out = b.load_checkpoint(tmp_path / "models", "tracking")
    assert out == data and b.num_timesteps == 0                            # reset_num_timesteps=True: the counter starts again, as PPO.learn's default
    for k in ("theta", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(b, k).view(torch.int32), getattr(a, k).view(torch.int32)), k
    assert int(b.step_count) == 17
    for k in VN_TENSORS:
        assert torch.equal(getattr(b.vecnorm, k), getattr(a.vecnorm, k)) and getattr(b.vecnorm, k).dtype == torch.float64, k
    assert not b.vecnorm.returns.any() and a.vecnorm.returns.any()          # zeroed, as VecNormalize.load -> set_venv does
    assert ptrs == [t.data_ptr() for t in (b.theta, b.exp_avg, b.exp_avg_sq, b.step_count, b.vecnorm.returns)] + [getattr(b.vecnorm, k).data_ptr() for k in VN_TENSORS] + \
           [p.data_ptr() for p in b.policy.parameters()]                   # in place: every address is the one a recorded graph holds
    assert usim.ppo._is_flat(b.policy, b.theta) and torch.equal(b.policy.action_net.weight.detach(), a.policy.action_net.weight.detach())
    b.load_checkpoint(tmp_path / "models", "tracking", reset_num_timesteps=False)
    assert b.num_timesteps == 12345
    # a fresh optimizer in the file: zero moments, step 0
    a.step_count.fill_(0)
    a.save_checkpoint(tmp_path / "models", "fresh")
    b.load_checkpoint(tmp_path / "models", "fresh")
    assert int(b.step_count) == 0 and not b.exp_avg.any() and not b.exp_avg_sq.any() and torch.equal(b.theta, a.theta)


def test_load_checkpoint_refusals_leave_the_learner_alone(usim, tmp_path):
    a, b = _cpu_learner(usim, seed=1), _cpu_learner(usim, seed=2)
    _fill(a, 1); _fill(b, 2)
    zip_path, pkl_path = a.save_checkpoint(tmp_path, "good")
    before = [t.clone() for t in (b.theta, b.exp_avg, b.exp_avg_sq, b.step_count, b.vecnorm.obs_mean, b.vecnorm.returns)]
    opt = a.adam_state_dict()
    opt["state"][3]["step"] = 16                                          # per-parameter steps that differ
    usim.policy.save_sb3_zip(tmp_path / "uneven.zip", a.policy, data=a.checkpoint_data(), optimizer_state=opt)
    shutil.copy(pkl_path, tmp_path / "vec_normalize_uneven.pkl")
    with pytest.raises(ValueError, match="steps differ"):
        b.load_checkpoint(tmp_path, "uneven")
    seven = _cpu_learner(usim, A=7, seed=3)                                # another action dimension: shapes that are not the learner's
    _fill(seven, 3)
    seven.save_checkpoint(tmp_path, "seven")
    with pytest.raises(ValueError, match="checkpoint shapes"):
        b.load_checkpoint(tmp_path, "seven")
    other = _cpu_learner(usim, seed=4)
    other.vecnorm.gamma = 0.9                                             # a VecNormalize constant that a recorded collector does not share
    other.save_checkpoint(tmp_path, "gamma")
    with pytest.raises(ValueError, match="gamma"):
        b.load_checkpoint(tmp_path, "gamma")
    after = (b.theta, b.exp_avg, b.exp_avg_sq, b.step_count, b.vecnorm.obs_mean, b.vecnorm.returns)
    assert all(torch.equal(x, y) for x, y in zip(before, after))           # every refusal came before the first write
    b.load_checkpoint(tmp_path, "good")
    assert torch.equal(b.theta, a.theta)
