"""usim_plan_sample / usim_plan_update on the host side: both are declared in include/usim.h, bound by _lib.SYMBOLS and exported by the library built here, and
their argument checks answer USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up pointers that no kernel may ever see, and run
without a GPU.  The refusals of planner.MPPIPlanner's constructor come before any library call and are tested with stand-in environment objects."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
NAMES = ("usim_plan_sample", "usim_plan_update")
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declared_and_bound(usim):
    assert _declaration("usim_plan_sample") == ["float* mean_dev", "const float* sigma_dev", "const float* act_low_dev", "const float* act_high_dev",
                                                "const uint8_t* restart_dev", "int groups", "int per_group", "int horizon", "int act_dim", "float smoothing",
                                                "uint64_t seed", "uint32_t counter", "const uint32_t* counter_base_dev", "float* cand_dev", "void* stream"]
    assert _declaration("usim_plan_update") == ["const float* cand_dev", "const float* ret_dev", "const float* act_low_dev", "const float* act_high_dev", "int groups",
                                                "int per_group", "int horizon", "int act_dim", "float temperature", "float* plan_dev", "float* next_mean_dev",
                                                "float* act_dev", "int32_t* best_dev", "float* weight_dev", "void* stream"]
    S, v, i = usim._lib.SYMBOLS, C.c_void_p, C.c_int
    assert S["usim_plan_sample"] == (C.c_int, [v, v, v, v, v, i, i, i, i, C.c_float, C.c_uint64, C.c_uint32, v, v, v])
    assert S["usim_plan_update"] == (C.c_int, [v, v, v, v, i, i, i, i, C.c_float, v, v, v, v, v, v])


def test_library_exports_them(usim):
    lib = usim._lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(usim._lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    for name in NAMES:
        assert name in exported and getattr(lib, name) is not None


def test_class_is_exported(usim):
    assert usim.planner.MPPIPlanner is not None and "planner" in usim.__all__
    for method in ("plan", "step", "record", "replay"):
        assert callable(getattr(usim.planner.MPPIPlanner, method))


def _sample(lib, mean=P, sigma=P, low=P, high=P, restart=None, G=2, K=4, H=3, A=6, smoothing=0.0, base=None, cand=P):
    return lib.usim_plan_sample(mean, sigma, low, high, restart, G, K, H, A, smoothing, 7, 0, base, cand, None)


def _update(lib, cand=P, ret=P, low=P, high=P, G=2, K=4, H=3, A=6, temperature=1.0, act=P):
    return lib.usim_plan_update(cand, ret, low, high, G, K, H, A, temperature, None, None, act, None, None, None)


def test_sample_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("mean", "sigma", "low", "high", "cand"):
        assert _sample(lib, **{name: None}) == INVALID, name
    for name in ("G", "K", "H"):
        for bad in (0, -3):
            assert _sample(lib, **{name: bad}) == INVALID, (name, bad)
    for bad in (0, -1, 9, 64):
        assert _sample(lib, A=bad) == INVALID, bad
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert _sample(lib, smoothing=bad) == INVALID, bad
    assert _sample(lib, G=2**20, K=2**12) == INVALID                      # G K beyond the int the library counts environments with


def test_update_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("cand", "ret", "low", "high", "act"):
        assert _update(lib, **{name: None}) == INVALID, name
    for name in ("G", "K", "H"):
        for bad in (0, -3):
            assert _update(lib, **{name: bad}) == INVALID, (name, bad)
    for bad in (0, -1, 9, 64):
        assert _update(lib, A=bad) == INVALID, bad
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert _update(lib, temperature=bad) == INVALID, bad
    assert _update(lib, G=2**20, K=2**12) == INVALID


# ---- the constructor of planner.MPPIPlanner: every refusal is a ValueError raised before the library (or a device) is touched ----
KW = dict(horizon=37, torso="soft")


def _stand_in(num_envs, snapshot_words=240, action_dim=6, kwargs=KW, device="cuda:0"):
    return SimpleNamespace(num_envs=num_envs, snapshot_words=snapshot_words, action_dim=action_dim, _kwargs=dict(kwargs), device=device)


@pytest.mark.parametrize("real, sim, kw, what", [
    (_stand_in(2), _stand_in(15), {}, "multiple"),
    (_stand_in(2), _stand_in(0), {}, "multiple"),
    (_stand_in(0), _stand_in(0), {}, "multiple"),
    (_stand_in(4), _stand_in(2), {}, "multiple"),
    (_stand_in(2), _stand_in(16, snapshot_words=312), {}, "snapshot_words"),
    (_stand_in(2), _stand_in(16, action_dim=7), {}, "action_dim"),
    (_stand_in(2), _stand_in(16, kwargs=dict(KW, horizon=38)), {}, "kwargs"),
    (_stand_in(2), _stand_in(16, device="cuda:1"), {}, "device"),
    (_stand_in(2), _stand_in(16), dict(sigma=0.0), "sigma"),
    (_stand_in(2), _stand_in(16), dict(sigma=-0.5), "sigma"),
    (_stand_in(2), _stand_in(16), dict(sigma=[0.3] * 5), "sigma"),
    (_stand_in(2), _stand_in(16), dict(sigma=[0.3] * 5 + [0.0]), "sigma"),
    (_stand_in(2), _stand_in(16), dict(sigma=float("nan")), "sigma"),
    (_stand_in(2), _stand_in(16), dict(horizon=0), "horizon"),
    (_stand_in(2), _stand_in(16), dict(temperature=-1.0), "temperature"),
    (_stand_in(2), _stand_in(16), dict(smoothing=1.0), "smoothing"),
])
def test_constructor_refusals(usim, monkeypatch, real, sim, kw, what):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(usim._lib, "load", no_library)
    args = dict(horizon=4, sigma=0.3, temperature=1.0)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        usim.planner.MPPIPlanner(real, sim, **args)
