"""usim_policy_bootstrap on the host side: declared in include/usim.h, bound by _lib.SYMBOLS, exported by the library; every refusal is answered with
USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up pointers that no kernel may ever see, and run without a GPU.  The
collectors accept the keyword that switches it on, last in their signatures and off by default."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments
VALUE_SIDE = ("vf_w1", "vf_b1", "vf_w2", "vf_b2", "val_w", "val_b")


def test_declared_bound_and_exported(usim):
    m = re.search(r"\bint\s+usim_policy_bootstrap\s*\(([^;]*)\)\s*;", HEADER)
    assert m, "usim_policy_bootstrap is not declared in include/usim.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == [
        "const usim_policy_net* net", "const usim_norm_stats* st", "const float* term_obs_dev", "const uint8_t* done_dev", "const int32_t* ep_length_dev",
        "int n", "int horizon", "float gamma", "float* rew_dev", "int32_t* count_dev", "void* stream"]
    L = usim._lib
    v, i = C.c_void_p, C.c_int
    assert L.SYMBOLS["usim_policy_bootstrap"] == (C.c_int, [C.POINTER(L.UsimPolicyNet), C.POINTER(L.UsimNormStats), v, v, v, i, i, C.c_float, v, v, v])
    nm = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "usim_policy_bootstrap" in set(re.findall(r" T (usim_[a-z_]+)", nm)) and L.load().usim_policy_bootstrap is not None


def _net(usim, **kw):
    f = {n: None for n, _ in usim._lib.UsimPolicyNet._fields_}            # the policy side, log_std and w2_packed are ignored: NULL throughout
    f.update({n: P for n in VALUE_SIDE})
    f.update(kw)
    return usim._lib.UsimPolicyNet(**f)


def _stats(usim, **kw):
    f = dict(obs_mean=P, obs_var=P, obs_count=None, ret_mean=None, ret_var=None, ret_count=None, returns=None, scratch=None, clip_obs=10.0, clip_reward=10.0,
             gamma=0.99, epsilon=1e-8)
    f.update(kw)
    return usim._lib.UsimNormStats(**f)


def _call(lib, net, st, term=P, done=P, ep=P, n=64, horizon=1000, gamma=0.99, rew=P, count=P):
    return lib.usim_policy_bootstrap(None if net is None else C.byref(net), None if st is None else C.byref(st), term, done, ep, n, horizon, gamma, rew, count, None)


def test_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    net, st = _net(usim), _stats(usim)
    assert _call(lib, None, st) == INVALID and _call(lib, net, None) == INVALID
    for name in ("term", "done", "ep", "rew"):
        assert _call(lib, net, st, **{name: None}) == INVALID, name
    for name in VALUE_SIDE:
        assert _call(lib, _net(usim, **{name: None}), st) == INVALID, name
    for name in ("obs_mean", "obs_var"):
        assert _call(lib, net, _stats(usim, **{name: None})) == INVALID, name
    for bad in (0, -1, -4096):
        assert _call(lib, net, st, n=bad) == INVALID, bad
        assert _call(lib, net, st, horizon=bad) == INVALID, bad
    for bad in (float("nan"), float("inf"), float("-inf"), -1e-6, 1.0 + 1e-6, -1.0, 2.0):
        assert _call(lib, net, st, gamma=bad) == INVALID, bad
    # (count_dev = NULL and the ends of [0, 1] are accepted: with a GPU, tests/test_gpu_bootstrap.py)


def test_collectors_accept_the_keyword(usim):
    pol = usim.policy
    for fn in (pol.FusedRollout.__init__, pol.collect_rollouts, pol.GraphedCollector.__init__):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "bootstrap_truncation" and params[-1].default is False, fn.__qualname__
    assert inspect.signature(pol._rollout_step).parameters["bootstrap_gamma"].default is None
    assert isinstance(usim.UltrasoundVecEnv.truncated, property)
