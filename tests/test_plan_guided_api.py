"""usim_score_block_tail / usim_plan_sample_elem / usim_plan_refit / usim_plan_tail on the host side, in the manner of test_plan_api.py: declared in include/usim.h,
bound by _lib.SYMBOLS, exported by the library built here, and every refusal answered with USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL
or made-up pointers that no kernel may ever see, and run without a GPU.  The refusals that planner.MPPIPlanner's new arguments add come before any library call and
are tested with stand-in objects."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
NAMES = ("usim_score_block_tail", "usim_plan_sample_elem", "usim_plan_refit", "usim_plan_tail")
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments
NAN, INF = float("nan"), float("inf")


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declared_and_bound(usim):
    assert _declaration("usim_score_block_tail") == ["const float* rew_block_dev", "const uint8_t* done_block_dev", "int nsteps", "int n", "float gamma",
                                                     "const float* tail_dev", "const double* ret_var_dev", "double epsilon", "float* return_dev", "int32_t* length_dev",
                                                     "void* stream"]
    assert _declaration("usim_plan_sample_elem") == [a.replace("sigma_dev", "sigma_elem_dev") for a in _declaration("usim_plan_sample")]
    assert _declaration("usim_plan_refit") == ["const float* cand_dev", "const float* ret_dev", "const float* act_low_dev", "const float* act_high_dev", "int groups",
                                               "int per_group", "int horizon", "int act_dim", "int elites", "float momentum", "float sigma_min", "float* mean_dev",
                                               "float* sigma_elem_dev", "int32_t* elite_dev", "void* stream"]
    assert _declaration("usim_plan_tail") == ["const float* cand_dev", "const float* weight_dev", "const int32_t* best_dev", "const int32_t* length_dev",
                                              "const uint8_t* done_last_dev", "const float* pol_act_dev", "const float* act_low_dev", "const float* act_high_dev",
                                              "int groups", "int per_group", "int horizon", "int act_dim", "float temperature", "float* next_mean_dev", "void* stream"]
    S, v, i, f = usim._lib.SYMBOLS, C.c_void_p, C.c_int, C.c_float
    assert S["usim_score_block_tail"] == (C.c_int, [v, v, i, i, f, v, v, C.c_double, v, v, v])
    assert S["usim_plan_sample_elem"] == S["usim_plan_sample"]
    assert S["usim_plan_refit"] == (C.c_int, [v, v, v, v, i, i, i, i, i, f, f, v, v, v, v])
    assert S["usim_plan_tail"] == (C.c_int, [v, v, v, v, v, v, v, v, i, i, i, i, f, v, v])
    assert re.search(r"#define\s+USIM_PLAN_REFIT_MAX_K\s+(\d+)", HEADER).group(1) == str(usim._lib.PLAN_REFIT_MAX_K)
    assert usim._lib.PLAN_REFIT_MAX_K >= 1024


def test_library_exports_them(usim):
    lib = usim._lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(usim._lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    for name in NAMES:
        assert name in exported and getattr(lib, name) is not None


def test_planner_methods_are_exported(usim):
    assert "planner" in usim.__all__
    for method in ("sample_elem", "refit", "evaluate_tail", "score", "tail", "plan", "step", "record", "replay"):
        assert callable(getattr(usim.planner.MPPIPlanner, method))


def _score(lib, rew=P, done=P, T=3, n=5, gamma=0.99, tail=P, ret_var=P, epsilon=1e-8, ret=P, length=P):
    return lib.usim_score_block_tail(rew, done, T, n, gamma, tail, ret_var, epsilon, ret, length, None)


def _sample(lib, mean=P, sigma=P, low=P, high=P, restart=None, G=2, K=4, H=3, A=6, smoothing=0.0, base=None, cand=P):
    return lib.usim_plan_sample_elem(mean, sigma, low, high, restart, G, K, H, A, smoothing, 7, 0, base, cand, None)


def _refit(lib, cand=P, ret=P, low=P, high=P, G=2, K=4, H=3, A=6, elites=2, momentum=0.1, sigma_min=1e-3, mean=P, sigma=P, elite=P):
    return lib.usim_plan_refit(cand, ret, low, high, G, K, H, A, elites, momentum, sigma_min, mean, sigma, elite, None)


def _tail(lib, cand=P, weight=P, best=P, length=P, done_last=P, pol=P, low=P, high=P, G=2, K=4, H=3, A=6, temperature=1.0, mean=P):
    return lib.usim_plan_tail(cand, weight, best, length, done_last, pol, low, high, G, K, H, A, temperature, mean, None)


def test_score_block_tail_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("rew", "done", "ret"):
        assert _score(lib, **{name: None}) == INVALID, name
    for name in ("T", "n"):
        for bad in (0, -3):
            assert _score(lib, **{name: bad}) == INVALID, (name, bad)
    for bad in (NAN, INF, -INF):
        assert _score(lib, gamma=bad) == INVALID, bad
    for bad in (NAN, INF, -INF, -1e-8):
        assert _score(lib, epsilon=bad) == INVALID, bad


def test_sample_elem_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("mean", "sigma", "low", "high", "cand"):
        assert _sample(lib, **{name: None}) == INVALID, name
    for name in ("G", "K", "H"):
        for bad in (0, -3):
            assert _sample(lib, **{name: bad}) == INVALID, (name, bad)
    for bad in (0, -1, 9, 64):
        assert _sample(lib, A=bad) == INVALID, bad
    for bad in (-0.1, 1.0, 1.5, NAN, INF):
        assert _sample(lib, smoothing=bad) == INVALID, bad
    assert _sample(lib, G=2**20, K=2**12) == INVALID


def test_refit_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("cand", "ret", "low", "high", "mean", "sigma"):
        assert _refit(lib, **{name: None}) == INVALID, name
    for name in ("G", "K", "H"):
        for bad in (0, -3):
            assert _refit(lib, **{name: bad}) == INVALID, (name, bad)
    for bad in (0, -1, 9, 64):
        assert _refit(lib, A=bad) == INVALID, bad
    for bad in (0, -1, 5, 2**30):                                         # elites in 1 .. K
        assert _refit(lib, elites=bad) == INVALID, bad
    for bad in (-0.1, 1.0, 1.5, NAN, INF):
        assert _refit(lib, momentum=bad) == INVALID, bad
    for bad in (0.0, -1e-3, NAN, INF):
        assert _refit(lib, sigma_min=bad) == INVALID, bad
    assert _refit(lib, K=usim._lib.PLAN_REFIT_MAX_K + 1) == INVALID       # the largest group a workgroup ranks
    assert _refit(lib, G=2**20, K=2**12) == INVALID


def test_tail_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    for name in ("cand", "weight", "best", "length", "done_last", "pol", "low", "high", "mean"):
        assert _tail(lib, **{name: None}) == INVALID, name
    for name in ("G", "K", "H"):
        for bad in (0, -3):
            assert _tail(lib, **{name: bad}) == INVALID, (name, bad)
    for bad in (0, -1, 9, 64):
        assert _tail(lib, A=bad) == INVALID, bad
    for bad in (-1.0, -1e-30, NAN, INF, -INF):
        assert _tail(lib, temperature=bad) == INVALID, bad
    assert _tail(lib, G=2**20, K=2**12) == INVALID


# ---- the constructor of planner.MPPIPlanner: the refusals of the new arguments are ValueErrors raised before the library (or a device) is touched ----
KW = dict(horizon=37, torso="soft")


def _stand_in(num_envs):
    return SimpleNamespace(num_envs=num_envs, snapshot_words=240, action_dim=6, _kwargs=dict(KW), device="cuda:0")


def _critic(gamma=0.99):
    return (SimpleNamespace(), SimpleNamespace(gamma=gamma, epsilon=1e-8, norm_reward=True))


@pytest.mark.parametrize("kw, what", [
    (dict(tail_action=True), "tail_action"),
    (dict(critic=_critic(0.99), gamma=1.0), "gamma"),
    (dict(critic=_critic(0.99)), "gamma"),                               # the planner's default gamma is 1
    (dict(critic=_critic(0.95), gamma=0.99, tail_action=True), "gamma"),
    (dict(iterations=2, elites=9), "elites"),                            # K = 8
    (dict(iterations=2, elites=0), "elites"),
    (dict(elites=9), "elites"),
    (dict(iterations=0), "iterations"),
    (dict(iterations=-2), "iterations"),
    (dict(iterations=2, momentum=1.0), "momentum"),
    (dict(iterations=2, momentum=-0.1), "momentum"),
    (dict(iterations=2, sigma_min=0.0), "sigma_min"),
    (dict(iterations=2, sigma_min=float("nan")), "sigma_min"),
])
def test_constructor_refusals(usim, monkeypatch, kw, what):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(usim._lib, "load", no_library)
    args = dict(horizon=4, sigma=0.3, temperature=1.0)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        usim.planner.MPPIPlanner(_stand_in(2), _stand_in(16), **args)


def test_refit_limit_is_checked_by_the_constructor(usim, monkeypatch):
    monkeypatch.setattr(usim._lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded before the arguments were checked")))
    big = usim._lib.PLAN_REFIT_MAX_K + 1
    with pytest.raises(ValueError, match="candidates per group"):
        usim.planner.MPPIPlanner(_stand_in(1), _stand_in(big), horizon=4, iterations=2)
