"""usim_rollout_actions / usim_score_block on the host side: both are declared in include/usim.h, bound by _lib.SYMBOLS and exported by the library built here, and
their argument checks answer USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up pointers that no kernel may ever see, and run
without a GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
NAMES = ("usim_rollout_actions", "usim_score_block")


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declared_and_bound(usim):
    assert _declaration("usim_rollout_actions") == ["usim_handle* h", "int nsteps", "const usim_step_io* io", "int block_advance", "void* stream"]
    assert _declaration("usim_score_block") == ["const float* rew_block_dev", "const uint8_t* done_block_dev", "int nsteps", "int n", "float gamma",
                                                "float* return_dev", "int32_t* length_dev", "void* stream"]
    S = usim._lib.SYMBOLS
    assert S["usim_rollout_actions"] == (C.c_int, [C.c_void_p, C.c_int, C.POINTER(usim._lib.UsimStepIO), C.c_int, C.c_void_p])
    assert S["usim_score_block"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p])


def test_library_exports_them(usim):
    lib = usim._lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(usim._lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    for name in NAMES:
        assert name in exported and getattr(lib, name) is not None


def test_methods_exist(usim):
    assert callable(usim.UltrasoundVecEnv.rollout_actions) and callable(usim.UltrasoundVecEnv.score_block)


def test_score_block_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    p = 0x1000                                                            # never dereferenced: every call below is refused on its arguments
    assert lib.usim_score_block(None, p, 4, 8, 1.0, p, p, None) == INVALID
    assert lib.usim_score_block(p, None, 4, 8, 1.0, p, p, None) == INVALID
    assert lib.usim_score_block(p, p, 4, 8, 1.0, None, p, None) == INVALID
    assert lib.usim_score_block(p, p, 4, 0, 1.0, p, p, None) == INVALID
    assert lib.usim_score_block(p, p, 4, -8, 1.0, p, p, None) == INVALID
    assert lib.usim_score_block(p, p, 0, 8, 1.0, p, p, None) == INVALID
    assert lib.usim_score_block(p, p, -4, 8, 1.0, p, None, None) == INVALID


def test_rollout_actions_refuses_a_null_handle(usim):
    lib = usim._lib.load()
    io = usim._lib.UsimStepIO()
    assert lib.usim_rollout_actions(None, 4, C.byref(io), 1, None) == INVALID
    assert lib.usim_rollout_actions(None, 0, C.byref(io), 0, None) == INVALID
    assert lib.usim_rollout_actions(None, 4, None, 0, None) == INVALID
