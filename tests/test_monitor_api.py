"""usim_monitor_words / usim_monitor_step / usim_explained_variance on the host side: declared in include/usim.h with the stated argument lists, bound by
_lib.SYMBOLS, exported by the library; every refusal is answered with USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up
pointers that no kernel may ever see, and run without a GPU.  The constants of _lib.py are the header's (a compiled probe), the Python surface is exported, and
write_scalar_csv writes TensorBoard's CSV export."""
import csv
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments (16-byte aligned)


def _args(name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declared_bound_and_exported(usim):
    assert _args("usim_monitor_words") == ["int window"]
    assert _args("usim_monitor_step") == ["const usim_step_io* io", "int n", "int window", "int horizon", "const int32_t* target_dev", "int32_t* count_dev",
                                          "uint32_t* monitor_dev", "void* stream"]
    assert _args("usim_explained_variance") == ["const float* values_dev", "const float* returns_dev", "int64_t count", "float* out_dev", "void* stream"]
    L = usim._lib
    v, i = C.c_void_p, C.c_int
    assert L.SYMBOLS["usim_monitor_words"] == (C.c_int, [i])
    assert L.SYMBOLS["usim_monitor_step"] == (C.c_int, [C.POINTER(L.UsimStepIO), i, i, i, v, v, v, v])
    assert L.SYMBOLS["usim_explained_variance"] == (C.c_int, [v, v, C.c_int64, v, v])
    nm = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    lib = L.load()
    for name in ("usim_monitor_words", "usim_monitor_step", "usim_explained_variance"):
        assert name in exported and getattr(lib, name) is not None


def test_python_surface(usim):
    mon = usim.monitor
    assert "monitor" in usim.__all__
    for name in ("DeviceMonitor", "evaluate_policy", "write_scalar_csv"):
        assert name in usim.__all__ and getattr(usim, name) is getattr(mon, name)
    sig = inspect.signature(mon.DeviceMonitor.__init__).parameters
    assert list(sig) == ["self", "env", "window", "targets"] and sig["window"].default == 100 and sig["targets"].default is None
    ev = inspect.signature(mon.evaluate_policy).parameters
    assert list(ev) == ["env", "policy", "vecnorm", "n_eval_episodes", "deterministic", "seed", "check_every", "return_episode_rewards"]
    assert [ev[k].default for k in list(ev)[3:]] == [10, True, 0, 50, False]
    assert list(inspect.signature(mon.write_scalar_csv).parameters) == ["path", "rows", "tag"]
    env = usim.UltrasoundVecEnv
    assert callable(env.attach_monitor) and callable(env.detach_monitor)
    assert "rollout_random" in env.attach_monitor.__doc__ and "before" in env.attach_monitor.__doc__.lower()
    assert list(inspect.signature(usim.ppo.NativePPO.learn).parameters) == ["self", "iterations"]
    assert usim.ppo.STAT_NAMES[-1] == "train/explained_variance"


def test_monitor_words(usim):
    lib, L = usim._lib.load(), usim._lib
    assert lib.usim_monitor_words(100) == 416 and L.monitor_words(100) == 416
    assert lib.usim_monitor_words(1) == 20 and lib.usim_monitor_words(1 << 20) == 16 + 4 * (1 << 20)
    for bad in (0, -1, (1 << 20) + 1, 2 ** 31 - 1):
        assert lib.usim_monitor_words(bad) == INVALID, bad
        with pytest.raises(ValueError):
            L.monitor_words(bad)


def test_constants_match_header(usim):
    """as test_struct_layouts_match_header: a probe compiled with the system compiler prints the header's values"""
    src = ('#include "usim.h"\n#include <stdio.h>\nint main(){printf("%d %d %d\\n", (int)USIM_MONITOR_HEADER_WORDS, (int)USIM_MONITOR_ROW_WORDS, '
           '(int)USIM_MONITOR_MAX_WINDOW);return 0;}')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        out = subprocess.run([f"{d}/p"], capture_output=True, text=True, check=True).stdout.split()
    L = usim._lib
    assert [int(v) for v in out] == [L.MONITOR_HEADER_WORDS, L.MONITOR_ROW_WORDS, L.MONITOR_MAX_WINDOW] == [16, 4, 1 << 20]


def _io(usim, **kw):
    f = {n: None for n, _ in usim._lib.UsimStepIO._fields_}               # only done, ep_return and ep_length are looked at
    f.update(done_dev=P, ep_return_dev=P, ep_length_dev=P)
    f.update(kw)
    return usim._lib.UsimStepIO(**f)


def _step(lib, io, n=64, window=100, horizon=1000, target=None, count=None, monitor=P):
    return lib.usim_monitor_step(None if io is None else C.byref(io), n, window, horizon, target, count, monitor, None)


def test_monitor_step_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    assert _step(lib, None) == INVALID
    for name in ("done_dev", "ep_return_dev", "ep_length_dev"):
        assert _step(lib, _io(usim, **{name: None})) == INVALID, name
    io = _io(usim)
    assert _step(lib, io, monitor=None) == INVALID
    for off in (1, 4, 8, 12):
        assert _step(lib, io, monitor=P + off) == INVALID, off              # off the 16-byte grid
    for bad in (0, -1, -4096):
        assert _step(lib, io, n=bad) == INVALID, bad
    for bad in (0, -1, (1 << 20) + 1):
        assert _step(lib, io, window=bad) == INVALID, bad
    assert _step(lib, io, target=P, count=None) == INVALID                  # targets without counts


def test_explained_variance_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    assert lib.usim_explained_variance(None, P, 8, P, None) == INVALID
    assert lib.usim_explained_variance(P, None, 8, P, None) == INVALID
    assert lib.usim_explained_variance(P, P, 8, None, None) == INVALID
    for bad in (0, -1, -2 ** 40):
        assert lib.usim_explained_variance(P, P, bad, P, None) == INVALID, bad


def test_write_scalar_csv_round_trip(usim, tmp_path):
    rows = [{"time/total_timesteps": 1024, "time/wall": 1700000000.25, "rollout/ep_rew_mean": 5.5, "train/loss": 0.1},
            {"time/total_timesteps": 2048, "time/wall": 1700000001.5, "train/loss": 0.2},                             # no monitor summary in this row: no line
            {"time/total_timesteps": 3072, "time/wall": 1700000002.75, "rollout/ep_rew_mean": 0.1 + 0.2, "train/loss": 0.3}]
    path = tmp_path / "ep_rew_mean.csv"
    assert usim.write_scalar_csv(path, rows, "rollout/ep_rew_mean") == 2
    with open(path, newline="") as f:
        read = list(csv.DictReader(f))
    assert list(read[0]) == ["Wall time", "Step", "Value"]
    assert [(float(r["Wall time"]), int(r["Step"]), float(r["Value"])) for r in read] == [(1700000000.25, 1024, 5.5), (1700000002.75, 3072, 0.1 + 0.2)]
    assert usim.write_scalar_csv(path, rows, "train/loss") == 3 and usim.write_scalar_csv(path, rows, "absent") == 0
