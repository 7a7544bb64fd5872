"""The C ABI used directly, without the Python host classes: the stand-alone ctypes stub of INTEGRATION.md section 4 must work
as printed (it is extracted from the document and executed), and the error conventions must hold on a real device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_integration_md_stub_runs_as_printed(monkeypatch):
    text = (ROOT / "INTEGRATION.md").read_text()
    blocks = re.findall(r"```python\n(.*?)```", text, flags=re.S)
    stub = next(b for b in blocks if "class UsimStepIO(C.Structure)" in b)
    monkeypatch.chdir(ROOT)                                  # the stub uses the in-tree library path
    ns = {}
    exec(compile(stub, "INTEGRATION.md:stub", "exec"), ns)
    torch.cuda.synchronize()
    obs, rew, done = ns["obs"], ns["rew"], ns["done"]
    assert obs.shape == (4096, 19) and torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert (rew > 0).all() and (rew <= 12.0001).all() and done.dtype == torch.uint8


def test_error_conventions_on_device(usim):
    lib = usim._lib.load()
    cfg = usim.make_config()
    h = C.c_void_p()
    assert lib.usim_create(C.byref(cfg), 8, 99, C.byref(h)) == -2 and not h            # device index out of range
    for lanes in (1, 5, 8):
        cfg.lanes_per_env = lanes
        assert lib.usim_create(C.byref(cfg), 8, 0, C.byref(h)) == -1, lanes             # invalid mapping
        if h:
            lib.usim_destroy(h); h = C.c_void_p()
    cfg.lanes_per_env = 0
    assert lib.usim_create(C.byref(cfg), 8, 0, C.byref(h)) == 0 and h
    assert lib.usim_num_envs(h) == 8 and lib.usim_action_dim(h) == 6 and lib.usim_num_elements(h) == 99
    io = usim._lib.UsimStepIO()                                                          # all-NULL io block
    assert lib.usim_step(h, C.byref(io), 1, None) == -1
    assert lib.usim_reset_explicit(h, None, None, None, None) == -1
    assert lib.usim_last_hip_error(h).decode() == ""
    # state round trip through the raw entry points
    assert lib.usim_reset(h, None, None, None) == 0
    sc = np.zeros((8, 40), dtype=np.float32); lat = np.zeros((8, 99, 2), dtype=np.float32)
    assert lib.usim_get_state(h, sc.ctypes.data, lat.ctypes.data) == 0
    assert np.all(sc[:, 37] == 1) and np.all(sc[:, 35] == 0) and np.isfinite(sc).all()   # episode 1, t = 0
    assert lib.usim_set_state(h, sc.ctypes.data, lat.ctypes.data) == 0
    sc2 = np.zeros_like(sc)
    assert lib.usim_get_state(h, sc2.ctypes.data, None) == 0 and np.array_equal(sc, sc2)
    lib.usim_destroy(h)


def test_mapping_refusal_matrix(usim):
    """which kernel mappings usim_create and usim_set_mapping accept (include/usim.h lanes_per_env, waves_per_simd): the rigid torso takes
    lanes_per_env 0 or 16, the soft and full torsos 0, 16, 32 or 64 (the full torso ignores it), every torso waves_per_simd 0 .. 2;
    usim_set_mapping switches soft-torso handles only, between lanes_per_env 16, 32 and 64"""
    lib = usim._lib.load()
    lanes_ok = {0: (0, 16), 1: (0, 16, 32, 64), 2: (0, 16, 32, 64)}
    got, want = {}, {}
    for torso in (0, 1, 2):
        for lanes in (0, 1, 5, 8, 16, 32, 64):
            for waves in (0, 1, 2, 3):
                cfg = usim._lib.UsimConfig()
                cfg.struct_size = C.sizeof(cfg)
                assert lib.usim_default_config(C.byref(cfg)) == 0
                cfg.torso, cfg.lanes_per_env, cfg.waves_per_simd = torso, lanes, waves
                h = C.c_void_p()
                got[torso, lanes, waves] = lib.usim_create(C.byref(cfg), 8, 0, C.byref(h))
                want[torso, lanes, waves] = 0 if lanes in lanes_ok[torso] and waves <= 2 else -1
                if h:
                    lib.usim_destroy(h)
    assert got == want
    assert lib.usim_set_mapping(None, 32, 0) == -1
    for torso in (0, 1, 2):
        cfg = usim._lib.UsimConfig()
        cfg.struct_size = C.sizeof(cfg)
        assert lib.usim_default_config(C.byref(cfg)) == 0
        cfg.torso = torso
        h = C.c_void_p()
        assert lib.usim_create(C.byref(cfg), 8, 0, C.byref(h)) == 0
        got, want = {}, {}
        for lanes in (0, 1, 5, 8, 16, 32, 64):
            for waves in (-1, 0, 1, 2, 3):
                got[lanes, waves] = lib.usim_set_mapping(h, lanes, waves)
                want[lanes, waves] = 0 if torso == 1 and lanes in (16, 32, 64) and 0 <= waves <= 2 else -1
        assert got == want, torso
        assert lib.usim_set_mapping(h, 32, 0) == (0 if torso == 1 else -1)
        lib.usim_destroy(h)


def test_profile_step_needs_the_profiling_build(usim):
    """the phase stamps are compiled into libusim_prof.so only (make -C csrc prof); the production library says so instead of
    returning zeros"""
    env = usim.UltrasoundVecEnv(64, device="cuda:0", seed=1, **usim.default_robosuite_kwargs())
    env.reset_tensor()
    with pytest.raises(RuntimeError, match="(?i)unsupported|profiling build"):
        env.profile_step(0)
    obs, rew, done = env.step_tensor(env.random_actions_tensor(0))      # the handle is still usable
    assert torch.isfinite(obs).all()
    env.close()


def test_plain_c_client_matches_the_python_host_class(usim, tmp_path):
    """examples/usim_client.c: the ABI from plain C (gcc, HIP runtime for device memory; no Python, no PyTorch in the process) gives, bit for bit, the
    observations the Python host class gives when driven with the same seed and actions"""
    import subprocess
    exe = tmp_path / "usim_client"
    libdir = ROOT / "robotic-ultrasound-imaging_amd" / "lib"
    subprocess.run(["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include", str(ROOT / "examples" / "usim_client.c"), "-o", str(exe),
                    "-L", str(libdir), "-lusim", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    n, steps, seed = 256, 60, 5
    out = subprocess.run([str(exe), str(n), str(steps), str(seed)], capture_output=True, text=True, check=True, timeout=300).stdout.split()
    rec = dict(zip(out[0::2], out[1::2]))
    env = usim.UltrasoundVecEnv(n, device="cuda:0", seed=seed, **usim.default_robosuite_kwargs())
    A = env.action_dim
    env.reset_tensor()
    total, ended = 0.0, 0
    idx = np.arange(n * A, dtype=np.int64)
    for t in range(steps):
        act = (((idx * 7 + t * 13) % 21 - 10).astype(np.float32) * np.float32(0.05)).reshape(n, A)
        obs, rew, done = env.step_tensor(torch.from_numpy(act).to("cuda:0"))
        total += float(rew.double().sum()); ended += int(done.sum())
    h = 1469598103934665603
    for byte in obs.cpu().numpy().astype(np.float32).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert int(rec["n"]) == n and int(rec["steps"]) == steps and int(rec["ended"]) == ended
    assert rec["obs_hash"] == f"{h:016x}"
    assert abs(float(rec["mean_reward"]) - total / (n * steps)) < 1e-5
    env.close()


@pytest.mark.parametrize("torso, n, kw", [("rigid", 70, {}), ("soft", 70, {}), ("soft", 70, {"warm_start": 1}), ("full", 8, {})],
                         ids=["rigid", "soft", "soft-warm", "full"])
def test_checkpoint_moves_a_state_between_handles(usim, torso, n, kw):
    """get_state of one handle, set_state on another of the same configuration, for every kind of state block and a number of environments that leaves padding
    environments in it: the second handle hands out the same state bit for bit in every key (scalars, lattice, the full torso's body, the kept contact lists) and
    computes the same next step"""
    opts = dict(usim.default_robosuite_kwargs(), **kw)
    a, b = (usim.UltrasoundVecEnv(n, device="cuda:0", seed=3, torso=torso, **opts) for _ in range(2))
    a.reset_tensor(); b.reset_tensor()
    a.rollout_random(0, 30)
    st = a.get_state()
    assert ("solver_warm_start" in st) == (torso == "full" or bool(kw)) and ("body" in st) == (torso == "full")
    b.set_state(st)
    st2 = b.get_state()
    assert set(st2) == set(st)
    for k in st:
        assert st[k].dtype == st2[k].dtype and st[k].shape == st2[k].shape and np.ascontiguousarray(st[k]).tobytes() == np.ascontiguousarray(st2[k]).tobytes(), k
    act = a.random_actions_tensor(30).clone()
    oa = [t.clone() for t in a.step_tensor(act)]
    ob = [t.clone() for t in b.step_tensor(act)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    a.close(); b.close()
