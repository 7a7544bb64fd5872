"""usim_metrics_words / usim_metrics_step / usim_record_words / usim_record_step on the host side: declared in include/usim.h with the stated argument lists,
bound by _lib.SYMBOLS, exported by the library; the word formulas; the constants of _lib.py are the header's (a compiled probe); every refusal is answered with
USIM_ERR_INVALID before anything is enqueued -- the calls below hold NULL or made-up pointers that no kernel may ever see, and run without a GPU.  Then the Python
surface, and EpisodeRecorder's decoding and CSV writing on a synthetic block."""
import ctypes as C
import inspect
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import metrics_ref as ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "usim.h").read_text(), flags=re.S)
INVALID = -1                                                              # USIM_ERR_INVALID
P = 0x1000                                                                # never dereferenced: every call below is refused on its arguments (16-byte aligned)
NAMES = ("usim_metrics_words", "usim_metrics_step", "usim_record_words", "usim_record_step")


def _args(name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), HEADER)
    assert m, f"{name} is not declared in include/usim.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_declared_bound_and_exported(usim):
    assert _args("usim_metrics_words") == ["int n", "int window"]
    assert _args("usim_metrics_step") == ["const usim_step_io* io", "int n", "int window", "int horizon", "const int32_t* target_dev", "int32_t* count_dev",
                                          "uint32_t* metrics_dev", "void* stream"]
    assert _args("usim_record_words") == ["int m", "int episodes", "int horizon"]
    assert _args("usim_record_step") == ["const usim_step_io* io", "int n", "int horizon", "const int32_t* env_index_dev", "int m", "int episodes",
                                         "float* record_dev", "void* stream"]
    L = usim._lib
    v, i = C.c_void_p, C.c_int
    assert L.SYMBOLS["usim_metrics_words"] == (C.c_int, [i, i])
    assert L.SYMBOLS["usim_metrics_step"] == (C.c_int, [C.POINTER(L.UsimStepIO), i, i, i, v, v, v, v])
    assert L.SYMBOLS["usim_record_words"] == (C.c_int, [i, i, i])
    assert L.SYMBOLS["usim_record_step"] == (C.c_int, [C.POINTER(L.UsimStepIO), i, i, v, i, i, v, v])
    nm = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (usim_[a-z_]+)", nm))
    lib = L.load()
    for name in NAMES:
        assert name in exported and getattr(lib, name) is not None


def test_word_formulas(usim):
    lib, L = usim._lib.load(), usim._lib
    assert lib.usim_metrics_words(64, 100) == 64 + 3200 + 1664 == L.metrics_words(64, 100)
    assert lib.usim_metrics_words(1, 1) == 64 + 32 + 26 == L.metrics_words(1, 1)
    assert lib.usim_metrics_words(4096, 1 << 20) == 64 + 32 * (1 << 20) + 26 * 4096 == L.metrics_words(4096, 1 << 20)
    for n, window in ((0, 100), (-1, 100), (64, 0), (64, -1), (64, (1 << 20) + 1), (2 ** 31 - 1, 100)):          # the last: beyond 2^31 - 1 words
        assert lib.usim_metrics_words(n, window) == INVALID, (n, window)
        with pytest.raises(ValueError):
            L.metrics_words(n, window)
    assert lib.usim_record_words(3, 2, 10) == 12 + 3180 == L.record_words(3, 2, 10)
    assert lib.usim_record_words(1, 1, 1) == 4 + 53 == L.record_words(1, 1, 1)
    assert lib.usim_record_words(16, 1, 1000) == 32 + 16 * 1000 * 53 == L.record_words(16, 1, 1000)
    for m, episodes, horizon in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 2, 10), (4096, 100, 1000)):               # the last: beyond 2^31 - 1 words
        assert lib.usim_record_words(m, episodes, horizon) == INVALID, (m, episodes, horizon)
        with pytest.raises(ValueError):
            L.record_words(m, episodes, horizon)


def test_constants_match_header(usim):
    """as test_struct_layouts_match_header: a probe compiled with the system compiler prints the header's values"""
    src = ('#include "usim.h"\n#include <stdio.h>\nint main(){printf("%d %d %d %d\\n", (int)USIM_METRICS, (int)USIM_METRICS_HEADER_WORDS, '
           '(int)USIM_METRICS_ROW_WORDS, (int)USIM_LOG_WIDTH);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        out = subprocess.run([f"{d}/p"], capture_output=True, text=True, check=True).stdout.split()
    L = usim._lib
    assert [int(v) for v in out] == [L.METRICS, L.METRICS_HEADER_WORDS, L.METRICS_ROW_WORDS, L.LOG_WIDTH] == [13, 64, 32, 53]
    assert (ref.M, ref.HEADER, ref.ROW, ref.LOG) == (13, 64, 32, 53) and L.METRICS == len(usim.error_metrics.METRICS)


def _io(usim, **kw):
    f = {n: None for n, _ in usim._lib.UsimStepIO._fields_}               # only log_dev and done_dev are looked at
    f.update(log_dev=P, done_dev=P)
    f.update(kw)
    return usim._lib.UsimStepIO(**f)


def _metrics(lib, io, n=64, window=100, horizon=1000, target=None, count=None, block=P):
    return lib.usim_metrics_step(None if io is None else C.byref(io), n, window, horizon, target, count, block, None)


def _record(lib, io, n=64, horizon=1000, index=P, m=2, episodes=1, block=P):
    return lib.usim_record_step(None if io is None else C.byref(io), n, horizon, index, m, episodes, block, None)


def test_metrics_step_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    assert _metrics(lib, None) == INVALID
    for name in ("log_dev", "done_dev"):
        assert _metrics(lib, _io(usim, **{name: None})) == INVALID, name
    io = _io(usim)
    assert _metrics(lib, io, block=None) == INVALID
    for off in (1, 4, 8, 12):
        assert _metrics(lib, io, block=P + off) == INVALID, off             # off the 16-byte grid
    for bad in (0, -1, -4096):
        assert _metrics(lib, io, n=bad) == INVALID, bad
        assert _metrics(lib, io, horizon=bad) == INVALID, bad
    for bad in (0, -1, (1 << 20) + 1):
        assert _metrics(lib, io, window=bad) == INVALID, bad
    assert _metrics(lib, io, target=P, count=None) == INVALID               # targets without counts


def test_record_step_refuses_before_it_launches(usim):
    lib = usim._lib.load()
    assert _record(lib, None) == INVALID
    for name in ("log_dev", "done_dev"):
        assert _record(lib, _io(usim, **{name: None})) == INVALID, name
    io = _io(usim)
    assert _record(lib, io, index=None) == INVALID
    assert _record(lib, io, block=None) == INVALID
    for off in (1, 4, 8, 12):
        assert _record(lib, io, block=P + off) == INVALID, off
    for bad in (0, -1, -4096):
        for key in ("n", "m", "episodes", "horizon"):
            assert _record(lib, io, **{key: bad}) == INVALID, (key, bad)


def test_python_surface(usim):
    ev = usim.evaluation
    assert "evaluation" in usim.__all__
    for name in ("DeviceEpisodeMetrics", "EpisodeRecorder", "evaluate_episodes"):
        assert name in usim.__all__ and getattr(usim, name) is getattr(ev, name)
    sig = inspect.signature(ev.DeviceEpisodeMetrics.__init__).parameters
    assert list(sig) == ["self", "env", "window", "targets"] and sig["window"].default == 100 and sig["targets"].default is None
    for name in ("record", "reset", "episode_count", "episodes", "summary"):
        assert callable(getattr(ev.DeviceEpisodeMetrics, name))
    sig = inspect.signature(ev.EpisodeRecorder.__init__).parameters
    assert list(sig) == ["self", "env", "env_indices", "episodes"] and sig["episodes"].default == 1
    for name in ("record", "reset", "complete", "episodes", "write_csv", "episodes_from_block"):
        assert callable(getattr(ev.EpisodeRecorder, name))
    assert list(inspect.signature(ev.EpisodeRecorder.write_csv).parameters)[:2] == ["self", "root"]
    assert list(inspect.signature(ev.EpisodeRecorder.episodes_from_block).parameters) == ["words", "m", "episodes", "horizon"]
    sig = inspect.signature(ev.evaluate_episodes).parameters
    assert list(sig) == ["env", "policy", "vecnorm", "n_eval_episodes", "deterministic", "seed", "check_every", "record_envs", "record_episodes"]
    assert [sig[k].default for k in list(sig)[3:]] == [10, True, 0, 50, None, 1]
    env = usim.UltrasoundVecEnv
    assert callable(env.attach_observer) and callable(env.detach_observer) and isinstance(env.observers, property)
    assert "before a collector is built" in env.attach_observer.__doc__.lower()
    sig = inspect.signature(usim.ppo.NativePPO.set_evaluation).parameters
    assert list(sig) == ["self", "eval_every", "eval_env", "n_eval_episodes", "deterministic"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, 10, True]
    # what existing callers rely on stays
    assert list(inspect.signature(usim.ppo.NativePPO.learn).parameters) == ["self", "iterations"]
    assert list(inspect.signature(usim.monitor.evaluate_policy).parameters) == ["env", "policy", "vecnorm", "n_eval_episodes", "deterministic", "seed", "check_every",
                                                                               "return_episode_rewards"]


def test_recorder_block_decodes_and_writes_the_reference_files(usim, tmp_path):
    """a block built by the restatement from synthetic episodes -> episodes_from_block -> write_csv: the reference's folders and file stems with the first free
    index, readable by metrics_from_csv, whose numbers are the restatement's metrics of those episodes"""
    n, H, eps = 4, 12, 2
    rec = ref.RecorderRef(n, [2, 0], episodes=eps, horizon=H)
    m = ref.MetricsRef(n, 100, H)
    for log, done in ref.synthetic_episodes(n, H, 60, seed=8):
        rec.step(log, done)
        m.step(log, done)
    assert rec.filled.tolist() == [eps, eps]
    R = usim.evaluation.EpisodeRecorder
    filled, lengths, rows = R.episodes_from_block(rec.block(), 2, eps, H)
    np.testing.assert_array_equal(filled, rec.filled)
    np.testing.assert_array_equal(lengths, rec.lengths)
    np.testing.assert_array_equal(rows.view(np.uint32), rec.rows.view(np.uint32))
    np.testing.assert_array_equal(R.episodes_from_block(rec.block().view(np.float32), 2, eps, H)[2].view(np.uint32), rec.rows.view(np.uint32))       # any 4-byte dtype
    with pytest.raises(ValueError):
        R.episodes_from_block(rec.block()[:-1], 2, eps, H)
    # write_csv needs of `self` only the action width: a stand-in carries it
    stand_in = type("Stand", (), {"action_dim": 6})()
    episodes = [{"env": e, "index": k, "length": int(lengths[r, k]), "rows": rows[r, k]} for r, e in enumerate((2, 0)) for k in range(eps)]
    written = R.write_csv(stand_in, root=str(tmp_path), episodes=episodes)
    chans = usim.episode_log._CHANNELS
    assert len(chans) == 23 and len(written) == len(chans) * 4             # (the reference's 24th file, the reward sum, is not a channel of the record)
    for folder, stem, _, _ in chans:
        assert sorted(p.name for p in (tmp_path / folder).glob(f"{stem}_*.csv")) == [f"{stem}_{i}.csv" for i in (1, 2, 3, 4)]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["policy_data", "reward_data", "simulation_data"]
    assert np.loadtxt(tmp_path / "policy_data" / "action_1.csv", delimiter=",").shape == (H, 6)
    for idx, ep in enumerate(episodes, start=1):
        fin = [h[0] for h in m.history if h[1] == ep["env"]][ep["index"]]
        want = usim.error_metrics.metrics_from_csv(str(tmp_path), idx)
        np.testing.assert_allclose(fin, [want[k] for k in ref.NAMES], rtol=1e-12, atol=1e-13)        # (bounds: tests/test_metrics_ref.py)
    written = R.write_csv(stand_in, root=str(tmp_path), episodes=episodes[:1])                        # the first free index
    assert all(p.endswith("_5.csv") for p in written)
