"""usim_policy_pack_multi / usim_policy_step_multi / usim_policy_reward_multi on the host side: declared in include/usim.h, bound by _lib.SYMBOLS and exported by
the library built here; their argument checks answer USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up pointers that no kernel
may ever see, and run without a GPU.  population.PolicyPopulation is tested on the CPU device; the refusals of the population's Python constructors come before
the library is loaded and are tested with stand-in objects."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
NAMES = ("usim_policy_pack_multi", "usim_policy_step_multi", "usim_policy_reward_multi")
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments (16-byte aligned)
INT_MAX = 2**31 - 1


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declared_bound_and_exported(usim):
    assert _declaration("usim_policy_pack_multi") == ["const float* theta_dev", "int stride", "int members", "int act_dim", "float* packed_dev", "void* stream"]
    assert _declaration("usim_policy_step_multi") == [
        "const float* theta_dev", "int stride", "const float* packed_dev", "const usim_norm_stats* st", "const float* obs_dev", "const uint8_t* prev_done_dev",
        "int members", "int envs_per_member", "int act_dim", "const float* act_low_dev", "const float* act_high_dev", "uint64_t seed", "uint32_t counter",
        "const uint32_t* counter_base_dev", "int env_offset", "int training", "int deterministic", "const usim_policy_out* out", "void* stream"]
    assert _declaration("usim_policy_reward_multi") == [
        "const usim_norm_stats* st", "const float* rew_dev", "const uint8_t* done_dev", "int members", "int envs_per_member", "int training", "int norm_reward",
        "float* nrew_dev", "double* raw_sum_dev", "const float* next_obs_dev", "void* stream"]
    L = usim._lib
    S, v, i = L.SYMBOLS, C.c_void_p, C.c_int
    assert S["usim_policy_pack_multi"] == (C.c_int, [v, i, i, i, v, v])
    assert S["usim_policy_step_multi"] == (C.c_int, [v, i, v, C.POINTER(L.UsimNormStats), v, v, i, i, i, v, v, C.c_uint64, C.c_uint32, v, i, i, i,
                                                     C.POINTER(L.UsimPolicyOut), v])
    assert S["usim_policy_reward_multi"] == (C.c_int, [C.POINTER(L.UsimNormStats), v, v, i, i, i, i, v, v, v, v])
    m = re.search(r"^#define\s+USIM_POLICY_MAX_MEMBERS\s+(\d+)\b", HEADER, flags=re.M)
    assert m and int(m.group(1)) == L.POLICY_MAX_MEMBERS
    lib = L.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    for name in NAMES:
        assert name in exported and getattr(lib, name) is not None
    for name in ("population", "PolicyPopulation", "PopulationVecNormalize", "PopulationRollout", "PopulationPPO", "evaluate_population"):
        assert name in usim.__all__ and getattr(usim, name) is getattr(usim.population, name, usim.population)


def _stats(usim, **kw):
    f = dict({n: P for n, _ in usim._lib.UsimNormStats._fields_[:8]}, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
    f.update(kw)
    return usim._lib.UsimNormStats(**f)


def _out(usim, **kw):
    f = {n: P for n, _ in usim._lib.UsimPolicyOut._fields_}
    f.update(kw)
    return usim._lib.UsimPolicyOut(**f)


def _params(A):
    return 76032 + 130 * A + 129


def _stride(A):
    return (_params(A) + 3) // 4 * 4


def _pack(lib, theta=P, stride=None, members=3, act_dim=6, packed=P):
    return lib.usim_policy_pack_multi(theta, _stride(act_dim if 1 <= act_dim <= 8 else 6) if stride is None else stride, members, act_dim, packed, None)


def _step(lib, usim, theta=P, stride=None, packed=P, st="default", obs=P, prev_done=P, members=3, envs=33, act_dim=6, low=P, high=P, training=0, out="default"):
    st = _stats(usim) if st == "default" else st
    out = _out(usim) if out == "default" else out
    return lib.usim_policy_step_multi(theta, _stride(act_dim if 1 <= act_dim <= 8 else 6) if stride is None else stride, packed, None if st is None else C.byref(st), obs,
                                      prev_done, members, envs, act_dim, low, high, 7, 0, None, 0, training, 0, None if out is None else C.byref(out), None)


def _reward(lib, usim, st="default", rew=P, done=P, members=3, envs=33, training=1, nrew=P, raw=P, next_obs=P):
    st = _stats(usim) if st == "default" else st
    return lib.usim_policy_reward_multi(None if st is None else C.byref(st), rew, done, members, envs, training, 1, nrew, raw, next_obs, None)


BAD_SIZES = ((0, 32), (-1, 32), (3, 0), (3, -7), (2, 2**30), (65536, 32768), (INT_MAX, 2), (65536, 1))      # <= 0, K G beyond INT_MAX, K beyond a grid axis


def test_pack_multi_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    assert _pack(lib, theta=None) == INVALID and _pack(lib, packed=None) == INVALID
    assert _pack(lib, packed=P + 4) == INVALID                             # off the 16-byte grid
    for bad in (0, -1, 65536):
        assert _pack(lib, members=bad) == INVALID, bad
    for bad in (0, -1, 9, 64):
        assert _pack(lib, act_dim=bad) == INVALID, bad
    for A in (1, 6, 7, 8):
        assert lib.usim_ppo_params(A) == _params(A)
        for bad in (_params(A) - 1, _stride(A) - 4, _stride(A) + 1, _stride(A) + 2, 0, -4):
            assert _pack(lib, stride=bad, act_dim=A) == INVALID, (A, bad)


def test_step_multi_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("theta", "packed", "st", "obs", "low", "high", "out"):
        assert _step(lib, usim, **{name: None}) == INVALID, name
    assert _step(lib, usim, out=_out(usim, act_env_dev=None)) == INVALID
    assert _step(lib, usim, packed=P + 8) == INVALID
    for name in ("obs_mean", "obs_var"):
        assert _step(lib, usim, st=_stats(usim, **{name: None})) == INVALID, name
    for name in ("scratch", "obs_count"):                                  # required by the statistics launch only
        assert _step(lib, usim, training=1, st=_stats(usim, **{name: None})) == INVALID, name
    for K, G in BAD_SIZES:
        assert _step(lib, usim, members=K, envs=G) == INVALID, (K, G)
    for bad in (0, -1, 9, 64):
        assert _step(lib, usim, act_dim=bad) == INVALID, bad
    for A in (6, 7):
        for bad in (_params(A) - 1, _stride(A) - 4, _stride(A) + 2, 0):
            assert _step(lib, usim, stride=bad, act_dim=A) == INVALID, (A, bad)


def test_reward_multi_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("st", "rew", "done", "nrew"):
        assert _reward(lib, usim, **{name: None}) == INVALID, name
    for K, G in BAD_SIZES:
        assert _reward(lib, usim, members=K, envs=G) == INVALID, (K, G)
    assert _reward(lib, usim, training=0, next_obs=None, st=_stats(usim, ret_var=None)) == INVALID
    for name in ("ret_mean", "ret_var", "ret_count", "returns"):
        assert _reward(lib, usim, next_obs=None, st=_stats(usim, **{name: None})) == INVALID, name
    for name in ("scratch", "obs_mean", "obs_var", "obs_count"):            # required with next_obs_dev while training
        assert _reward(lib, usim, st=_stats(usim, **{name: None})) == INVALID, name


@pytest.mark.parametrize("A", [6, 7])
def test_members_alias_their_rows(usim, A):
    pop_mod, learner = usim.population, usim.learner
    torch.manual_seed(5)
    pop = pop_mod.PolicyPopulation(3, A, device="cpu")
    Pw = learner.ppo_params(A)
    assert pop.theta.shape == (3, pop.stride) and pop.stride >= Pw and pop.stride % 4 == 0 and pop.packed.shape == (3, usim._lib.POLICY_PACKED)
    for k in range(3):
        m = pop.member(k)
        assert isinstance(m, usim.policy.MlpActorCritic) and m is pop.member(k)
        row = pop.theta[k, :Pw]
        assert learner._is_flat(m, row)
        flat = learner.flatten_parameters(m)
        assert flat.data_ptr() == pop.theta.data_ptr() + 4 * k * pop.stride and flat.numel() == Pw      # the row itself: nothing was copied
        o = 0
        for _, path in learner.FIELDS:
            p = dict(m.named_parameters())[path]
            assert p.data_ptr() == row.data_ptr() + 4 * o and torch.equal(p.detach().reshape(-1), row[o:o + p.numel()])
            o += p.numel()
        assert o == Pw
    assert not torch.equal(pop.theta[0], pop.theta[1])                     # members are initialised independently
    # writing a member changes its row and no other word
    before = pop.theta.clone()
    with torch.no_grad():
        pop.member(1).action_net.bias.add_(1.0)
        pop.member(1).log_std.fill_(-0.5)
    changed = (pop.theta != before)
    assert changed[1].sum().item() == 2 * A and not changed[0].any() and not changed[2].any()
    assert torch.equal(pop.theta[1, Pw - A:Pw], torch.full((A,), -0.5))
    # ... and writing the row is seen by the member
    with torch.no_grad():
        pop.theta[2, :Pw].zero_()
    assert all(float(p.detach().abs().sum()) == 0.0 for p in pop.member(2).parameters()) and torch.equal(pop.theta[0], before[0])


def test_load_member_and_from_policies(usim, tmp_path):
    pop_mod, policy = usim.population, usim.policy
    torch.manual_seed(9)
    src = [policy.MlpActorCritic(19, 6) for _ in range(2)]
    pop = pop_mod.PolicyPopulation.from_policies(src)
    Pw = usim.learner.ppo_params(6)
    for k in range(2):
        assert torch.equal(pop.theta[k, :Pw], usim.learner.state_dict_to_flat(src[k].to_sb3_state_dict(), 6))
        assert src[k].log_std.data_ptr() != pop.member(k).log_std.data_ptr()       # the sources are read, not re-seated
    policy.save_sb3_zip(tmp_path / "a.zip", src[1])
    ptr = pop.member(0).log_std.data_ptr()
    pop.load_member(0, tmp_path / "a.zip")
    assert torch.equal(pop.theta[0], pop.theta[1]) and pop.member(0).log_std.data_ptr() == ptr
    again = pop_mod.PolicyPopulation.from_checkpoints([tmp_path / "a.zip"] * 3, device="cpu")
    assert again.members == 3 and all(torch.equal(again.theta[k], pop.theta[1]) for k in range(3))
    with pytest.raises(ValueError):
        pop.load_member(0, policy.MlpActorCritic(19, 7))
    for bad in (dict(members=0, act_dim=6), dict(members=2, act_dim=9), dict(members=2, act_dim=6, stride=usim.learner.ppo_params(6) + 1)):
        with pytest.raises(ValueError):
            pop_mod.PolicyPopulation(device="cpu", **bad)


def test_vecnormalize_members_share_memory(usim):
    vn = usim.population.PopulationVecNormalize(3, 5, device="cpu")
    assert vn.obs_mean.shape == (3, 19) and vn._obs_count.shape == (3,) and vn.returns.shape == (15,)
    m = vn.member(1)
    assert isinstance(m, usim.policy.DeviceVecNormalize) and m.obs_mean.data_ptr() == vn.obs_mean[1].data_ptr() and m.returns.data_ptr() == vn.returns[5:].data_ptr()
    st = dict(obs_mean=[0.5] * 19, obs_var=[2.0] * 19, count=100.0, ret_mean=1.5, ret_var=4.0, ret_count=90.0, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
    vn.load_member(1, st)
    assert vn.obs_mean[1].eq(0.5).all() and vn.obs_mean[0].eq(0).all() and vn.obs_mean[2].eq(0).all()
    assert vn._obs_count.tolist() == [1e-4, 100.0, 1e-4] and vn._ret_count.tolist() == [1e-4, 90.0, 1e-4] and vn.ret_var.tolist() == [1.0, 4.0, 1.0]
    assert m.obs_count == 100.0 and m.stats()["ret_mean"] == 1.5
    vn.training = False
    assert m.training is False and m.norm_reward is True
    with pytest.raises(ValueError):
        vn.load_member(0, dict(st, gamma=0.9))                             # the constants are shared


def _standins(usim, K=3, G=32, n=96, A=6, buf_n=None):
    box = SimpleNamespace(low=[-1.0] * A, high=[1.0] * A)
    env = SimpleNamespace(num_envs=n, action_dim=A, device=torch.device("cpu"), action_space=box, env_offset=0)
    pop = usim.population.PolicyPopulation(K, A, device="cpu")
    vn = usim.population.PopulationVecNormalize(K, G, device="cpu")
    buf = usim.policy.DeviceRolloutBuffer(4, n if buf_n is None else buf_n, 19, A, device="cpu")
    return env, pop, vn, buf


def test_constructors_refuse_before_the_library_is_loaded(usim, monkeypatch):
    L, pm = usim._lib, usim.population

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_load)
    env, pop, vn, buf = _standins(usim)
    with pytest.raises(ValueError, match="num_envs"):
        pm.PopulationRollout(SimpleNamespace(**{**vars(env), "num_envs": 97}), pop, vn, buf)
    with pytest.raises(ValueError, match="buffer"):
        pm.PopulationRollout(*_standins(usim, buf_n=64))
    with pytest.raises(ValueError, match="bootstrap_truncation"):
        pm.PopulationRollout(env, pop, vn, buf, bootstrap_truncation=True)
    with pytest.raises(ValueError, match="act_dim"):
        pm.PopulationRollout(SimpleNamespace(**{**vars(env), "action_dim": 7}), pop, vn, buf)
    with pytest.raises(ValueError, match="num_envs"):
        pm.evaluate_population(SimpleNamespace(**{**vars(env), "num_envs": 64}), pop, vn)
    with pytest.raises(ValueError, match="num_envs"):
        pm.PopulationPPO(SimpleNamespace(**{**vars(env), "num_envs": 95}), pop, vn, buf, None, seeds=[0, 1, 2])
    with pytest.raises(ValueError, match="learning_rate"):
        pm.PopulationPPO(env, pop, vn, buf, None, seeds=[0, 1, 2], learning_rate=[3e-4, 1e-4])
    with pytest.raises(ValueError, match="seeds"):
        pm.PopulationPPO(env, pop, vn, buf, None, seeds=[0, 1])
    with pytest.raises(AssertionError, match="library was loaded"):       # ... and with good arguments the constructor does go on to the library
        pm.PopulationRollout(env, pop, vn, buf)
