"""usim_ppo_work_floats_multi / usim_ppo_grad_multi / usim_ppo_adam_multi on the host side: declared in include/usim.h, bound by _lib.SYMBOLS and exported by the
library built here; their argument checks answer USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up pointers that no kernel may
ever see, and run without a GPU.  The refusals of population.PopulationPPO(concurrent=True) come before the library is loaded and are tested with stand-in objects."""
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
NAMES = ("usim_ppo_work_floats_multi", "usim_ppo_grad_multi", "usim_ppo_adam_multi")
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments (16-byte aligned)
INT_MAX = 2**31 - 1
W, TILE, W2 = 128, 32, 128 * 256


def _declaration(name, ret="int"):
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def _params(A):
    return 76032 + 130 * A + 129


def _stride(A):
    return (_params(A) + 3) // 4 * 4


def test_declared_bound_and_exported(usim):
    assert _declaration("usim_ppo_work_floats_multi", "int64_t") == ["int act_dim", "int members", "int batch"]
    assert _declaration("usim_ppo_grad_multi") == ["const float* theta_dev", "int stride", "int members", "const usim_ppo_batch_multi* b", "float* work_dev",
                                                   "float* grad_dev", "float* stats_dev", "void* stream"]
    assert _declaration("usim_ppo_adam_multi") == ["float* theta_dev", "const float* grad_dev", "float* m_dev", "float* v_dev", "int32_t* step_dev", "int stride",
                                                   "int members", "int params", "const float* hyper_dev", "float beta1", "float beta2", "float eps",
                                                   "float* stats_dev", "int32_t* gate_dev", "void* stream"]
    L = usim._lib
    S, v, i, f = L.SYMBOLS, C.c_void_p, C.c_int, C.c_float
    assert S["usim_ppo_work_floats_multi"] == (C.c_int64, [i, i, i])
    assert S["usim_ppo_grad_multi"] == (C.c_int, [v, i, i, C.POINTER(L.UsimPpoBatchMulti), v, v, v, v])
    assert S["usim_ppo_adam_multi"] == (C.c_int, [v, v, v, v, v, i, i, i, v, f, f, f, v, v, v])
    m = re.search(r"^#define\s+USIM_PPO_HYPER_WORDS\s+(\d+)\b", HEADER, flags=re.M)
    assert m and int(m.group(1)) == L.PPO_HYPER_WORDS == 8
    lib = L.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    for name in NAMES:
        assert name in exported and getattr(lib, name) is not None


def test_struct_layout_matches_the_header(usim, tmp_path):
    L = usim._lib
    fields = [n for n, _ in L.UsimPpoBatchMulti._fields_]
    src = ('#include "usim.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(usim_ppo_batch_multi));'
           + "".join(f'printf(" %zu", offsetof(usim_ppo_batch_multi, {n}));' for n in fields) + 'printf("\\n");return 0;}')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(L.UsimPpoBatchMulti)] + [getattr(L.UsimPpoBatchMulti, n).offset for n in fields]


def _batch(usim, **kw):
    f = dict({n: P for n, t in usim._lib.UsimPpoBatchMulti._fields_ if t is C.c_void_p}, index_stride=4200, rows=4200, batch=70, act_dim=6, normalize_advantage=1,
             value_clip=0)
    f.update(kw)
    return usim._lib.UsimPpoBatchMulti(**f)


def _grad(lib, usim, theta=P, stride=None, members=3, b="default", work=P, grad=P, stats=P, **kw):
    b = _batch(usim, **kw) if b == "default" else b
    A = kw.get("act_dim", 6)
    stride = _stride(A if 1 <= A <= 8 else 6) if stride is None else stride
    return lib.usim_ppo_grad_multi(theta, stride, members, None if b is None else C.byref(b), work, grad, stats, None)


def _adam(lib, theta=P, grad=P, m=P, v=P, step=P, stride=None, members=3, params=None, hyper=P, beta1=0.9, beta2=0.999, eps=1e-5, stats=P, gate=P):
    params = _params(6) if params is None else params
    return lib.usim_ppo_adam_multi(theta, grad, m, v, step, _stride(6) if stride is None else stride, members, params, hyper, beta1, beta2, eps, stats, gate, None)


def test_grad_multi_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    # what usim_ppo_grad refuses
    for name in ("theta", "b", "work", "grad", "stats"):
        assert _grad(lib, usim, **{name: None}) == INVALID, name
    for name in ("obs_dev", "act_dev", "old_logp_dev", "adv_dev", "ret_dev"):
        assert _grad(lib, usim, **{name: None}) == INVALID, name
    for bad in (0, -1, 9, 64):
        assert _grad(lib, usim, act_dim=bad) == INVALID, bad
    for bad in (0, -5, INT_MAX):
        assert _grad(lib, usim, batch=bad, index_stride=INT_MAX) == INVALID, bad
    assert _grad(lib, usim, rows=0) == INVALID
    assert _grad(lib, usim, index_dev=None, rows=69) == INVALID             # rows < batch without an index list
    for off in (4, 8, 12):
        assert _grad(lib, usim, work=P + off) == INVALID, off               # off the 16-byte grid
    # the population's own
    for bad in (0, -1, 65536, INT_MAX):
        assert _grad(lib, usim, members=bad) == INVALID, bad
    for A in (1, 6, 8):
        for bad in (_params(A) - 1, _stride(A) - 4, _stride(A) + 1, _stride(A) + 2, 0, -4):
            assert _grad(lib, usim, stride=bad, act_dim=A) == INVALID, (A, bad)
    assert _grad(lib, usim, members=65535, rows=32769, index_stride=32769) == INVALID           # members x rows beyond INT_MAX
    assert _grad(lib, usim, members=2, rows=2**30) == INVALID
    assert _grad(lib, usim, index_stride=69) == INVALID                     # index_stride < batch with an index list
    assert _grad(lib, usim, hyper_dev=None) == INVALID
    assert _grad(lib, usim, value_clip=1, old_value_dev=None) == INVALID


def test_adam_multi_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("theta", "grad", "m", "v", "step", "hyper"):
        assert _adam(lib, **{name: None}) == INVALID, name
    assert _adam(lib, params=0) == INVALID and _adam(lib, params=-3) == INVALID
    for bad in (-1e-5, float("inf"), float("nan")):
        assert _adam(lib, eps=bad) == INVALID, bad
    for bad in (-0.1, 1.0, float("nan")):
        assert _adam(lib, beta1=bad) == INVALID and _adam(lib, beta2=bad) == INVALID, bad
    for bad in (0, -1, 65536):
        assert _adam(lib, members=bad) == INVALID, bad
    for bad in (_params(6) - 1, _stride(6) - 4, _stride(6) + 1, _stride(6) + 2, 0, -4):
        assert _adam(lib, stride=bad) == INVALID, bad
    assert _adam(lib, params=_stride(6) + 1) == INVALID                     # stride < params


def _blocks(batch):
    return min(W, -(-batch // TILE))


def _region(A, batch):
    """a member's region as include/usim.h states it: nb partial blocks | four packed matrices on the 16-byte grid | nb rows of 8 float64 | two float64"""
    nb = _blocks(batch)
    return (nb * _params(A) + 3) // 4 * 4 + 4 * W2 + 16 * nb + 4


def test_work_floats_multi(usim):
    lib = usim._lib.load()
    for bad in ((0, 3, 70), (9, 3, 70), (6, 0, 70), (6, 65536, 70), (6, 3, 0), (6, -1, 70), (6, 3, -70)):
        assert lib.usim_ppo_work_floats_multi(*bad) == INVALID, bad
    for A in (1, 6, 7, 8):
        for batch in (1, 32, 33, 70, 4095, 4096, 4097, 4133, 65536, INT_MAX - 8192):
            one = lib.usim_ppo_work_floats_multi(A, 1, batch)
            assert one == _region(A, batch) and one % 4 == 0                 # every member's region starts on the 16-byte grid
            for K in (3, 128, 65535):
                assert lib.usim_ppo_work_floats_multi(A, K, batch) == K * one
    f = lambda batch: lib.usim_ppo_work_floats_multi(6, 1, batch)
    assert f(1) == f(32) < f(33) == f(64) < f(65) and f(4064) < f(4065) == f(4096) == f(4097) == f(10**6)      # grows with min(128, ceil(batch / 32)) and no further
    assert f(4096) == lib.usim_ppo_work_floats(6)                            # at 128 blocks a member's region is the lone workspace
    assert f(70) * 16 < lib.usim_ppo_work_floats(6)                          # 16 members at batch 70 in less than one lone workspace


def _standins(usim, K=3, G=32, A=6):
    box = SimpleNamespace(low=[-1.0] * A, high=[1.0] * A)
    env = SimpleNamespace(num_envs=K * G, action_dim=A, device=torch.device("cpu"), action_space=box, env_offset=0)
    pop = usim.population.PolicyPopulation(K, A, device="cpu")
    vn = usim.population.PopulationVecNormalize(K, G, device="cpu")
    buf = usim.policy.DeviceRolloutBuffer(4, K * G, 19, A, device="cpu")
    return env, pop, vn, buf


def test_concurrent_refuses_before_the_library_is_loaded(usim, monkeypatch):
    L, pm = usim._lib, usim.population

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_load)
    args = _standins(usim)
    new = lambda **kw: pm.PopulationPPO(*args, None, seeds=[0, 1, 2], concurrent=True, **kw)
    for name, values in (("n_epochs", [2, 2, 3]), ("batch_size", [32, 64, 32]), ("normalize_advantage", [True, False, True]), ("adam_eps", [1e-5, 1e-5, 1e-8])):
        with pytest.raises(ValueError, match=name) as e:
            new(**{name: values})
        k = 1 if values[1] != values[0] else 2
        assert f"member 0 has {values[0]!r}" in str(e.value) and f"member {k} has {values[k]!r}" in str(e.value)      # the first differing pair
    with pytest.raises(ValueError, match="clip_range_vf"):
        new(clip_range_vf=[0.2, None, 0.2])
    with pytest.raises(ValueError, match="clip_range_vf"):
        new(clip_range_vf=[None, None, lambda p: 0.2])
    with pytest.raises(ValueError, match="learning_rate"):                 # the refusals every population shares still come first
        new(learning_rate=[3e-4, 1e-4])
    # what may differ per member passes the checks and goes on to the library, and so does the sequential path with differing shared values
    for kw in (dict(learning_rate=[3e-4, 1e-3, 1e-4], clip_range=[0.1, 0.2, 0.3], ent_coef=[0, 1e-3, 0], vf_coef=[0.5, 0.25, 1.0], max_grad_norm=[0.5, 0, 1e-3],
                    target_kl=[None, 1e-9, None], clip_range_vf=[0.1, 0.2, lambda p: 0.3], n_epochs=[2, 2, 2], batch_size=32),):
        with pytest.raises(AssertionError, match="library was loaded"):
            new(**kw)
    with pytest.raises(AssertionError, match="library was loaded"):
        pm.PopulationPPO(*args, None, seeds=[0, 1, 2], n_epochs=[2, 2, 3])
