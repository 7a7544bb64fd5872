"""usim_config.warm_start: the top-face contact solve started from the forces of the previous physics step (MuJoCo's semantics; oracle: uso_config.warm_start).
Parity with the oracle at 18 warm iterations, mapping / launch invariance bit for bit, cold episode starts, the checkpoint round trip, and what stopping at 18 costs
against a converged solve."""
import os

import numpy as np
import pytest
import torch

from oracle_lib import deep_spawn_params
from test_gpu_parity import _mk, _razor_edge, _run_parity

pytestmark = pytest.mark.gpu

WARM = dict(warm_start=1, pgs_iters=18)
MODES = ["tracking", "fixed", "variable_z", "wrench"]


def _env(usim, n, torso="soft", **kw):
    opts = dict(usim.default_robosuite_kwargs())
    seed = kw.pop("seed", 3)
    opts.update(kw)
    return usim.UltrasoundVecEnv(n, device="cuda:0", seed=seed, torso=torso, **opts)


def _state_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 1. parity with the oracle (same iteration count, same warm start on both sides), the existing bars ----
@pytest.mark.parametrize("mode", MODES)
def test_warm_start_parity_200_steps(usim, mode):
    _run_parity(usim, 256, 200, "soft", mode, **WARM)


@pytest.mark.parametrize("case", ["merged_pair", "one_probe_geom", "substeps", "randomised", "ur5e", "single_env", "ragged"])
def test_warm_start_parity_other_configurations(usim, case):
    if case == "merged_pair":
        _run_parity(usim, 256, 200, "soft", "tracking", pair_model=0, **WARM)
    elif case == "one_probe_geom":
        _run_parity(usim, 256, 200, "soft", "tracking", probe_geoms=1, **WARM)
    elif case == "substeps":          # four physics substeps per control step: the forces carry from substep to substep
        _run_parity(usim, 67, 50, "soft", "variable_z", gpu_extra=dict(control_freq=125), ora_extra=dict(substeps=4, control_dt=1 / 125), **WARM)
    elif case == "randomised":
        _run_parity(usim, 256, 200, "soft", "tracking", friction_randomization=1, elem_friction=0.0, probe_friction=0.3, **WARM)
    elif case == "ur5e":
        _run_parity(usim, 256, 200, "soft", "tracking", robot="UR5e", **WARM)
    elif case == "single_env":
        _run_parity(usim, 1, 200, "soft", "tracking", **WARM)
    else:
        _run_parity(usim, 67, 200, "soft", "tracking", **WARM)


# ---- 2. one size up: the automatic mappings of 4096 (lanes_per_env 32) and 8192 environments (64) ----
@pytest.mark.parametrize("n", [4096, 8192])
def test_warm_start_parity_full_size(usim, n):
    os.environ.setdefault("OMP_NUM_THREADS", str(min(os.cpu_count() or 1, 64)))
    _run_parity(usim, n, 200, "soft", "tracking", omp=True, **WARM)


# ---- 3. mapping and launch invariance, bit for bit ----
def _rollout(env, steps, chunks=None, mappings=None):
    env.reset_tensor()
    blk = env.alloc_block(steps)
    if chunks is None:
        env.rollout_random(0, steps, blk)
    else:
        for i, k0 in enumerate(range(0, steps, chunks)):
            if mappings:
                env.set_mapping(*mappings[i % len(mappings)])
            kk = min(chunks, steps - k0)
            env.rollout_random(k0, kk, {k: t[k0:k0 + kk] for k, t in blk.items()})
    torch.cuda.synchronize()
    return blk, env.contacts.clone(), env.get_state()


def _same_rollout(ref, other):
    for key in ("obs", "rew", "done", "act"):
        assert torch.equal(ref[0][key], other[0][key]), key
    assert torch.equal(ref[1], other[1])
    _state_equal(ref[2], other[2])


def test_warm_start_mappings_and_launch_lengths_compute_the_same_bits(usim):
    n, steps = 500, 300

    def run(lanes, spl=256, **kw):                                        # (a fresh handle per rollout: a reset draws with the handle's episode counter)
        env = _env(usim, n, lanes_per_env=lanes, **WARM)
        env.set_steps_per_launch(spl)
        out = _rollout(env, steps, **kw)
        env.close()
        return out

    ref = run(32)
    assert int(ref[0]["done"].sum()) > 100                               # episodes end and restart cold inside the launches
    assert "solver_warm_start" in ref[2] and (ref[2]["solver_warm_start"][:, :8] >= 0).any()
    for lanes in (16, 32, 64):
        for spl in (256, 7, 1):
            if (lanes, spl) != (32, 256):
                _same_rollout(ref, run(lanes, spl))
    # a mapping switch every 16 steps
    _same_rollout(ref, run(32, chunks=16, mappings=[(32, 0), (16, 1), (64, 0), (16, 2)]))
    # Python-driven usim_step, one launch per step
    e = _env(usim, n, lanes_per_env=32, **WARM)
    e.reset_tensor()
    for k in range(steps):
        act = e.random_actions_tensor(k)
        obs, rew, done = e.step_tensor(act)
        torch.cuda.synchronize()
        assert torch.equal(ref[0]["obs"][k], obs) and torch.equal(ref[0]["rew"][k], rew) and torch.equal(ref[0]["done"][k], done), k
    _state_equal(ref[2], e.get_state())
    e.close()


def test_warm_start_resolves_a_slot_overflow_to_the_same_bits_in_every_mapping(usim):
    """the warm twin of test_gpu_properties.test_every_mapping_resolves_a_slot_overflow_to_the_same_bits: probes spawned 1.2-3 cm deep, so that waves carry more than four
    contacts (the Delassus product summed by halves, the A s0 product of the kept forces included) and the slot rule runs, under a warm start in the three mappings --
    observations, rewards, done flags, contact lists and the final state with its kept list are the same bits"""
    n = 256
    envs = [_env(usim, n, lanes_per_env=lanes, **WARM) for lanes in (16, 32, 64)]
    for e in envs:
        e.reset_tensor()
    p = deep_spawn_params(envs[0].get_state(), n)
    obs0 = [e.reset_explicit_tensor(p).clone() for e in envs]
    assert all(torch.equal(obs0[0], o) for o in obs0[1:])
    status = [e.get_state()["status"].astype(int) & 1 for e in envs]
    assert status[0].sum() > 20 and all(np.array_equal(status[0], s) for s in status[1:])
    act = torch.full((n, 6), 0.5, dtype=torch.float32, device=envs[0].device)
    most = 0
    for k in range(25):
        res = [[x.clone() for x in e.step_tensor(act, auto_reset=False)] for e in envs]
        most = max(most, int(envs[0].contacts[:, 0].max()))
        for r, e in zip(res[1:], envs[1:]):
            assert all(torch.equal(a, b) for a, b in zip(res[0], r)) and torch.equal(envs[0].contacts, e.contacts), k
    assert most > 4
    s0 = envs[0].get_state()
    assert "solver_warm_start" in s0 and (s0["solver_warm_start"][:, :8] >= 0).any()
    for e in envs[1:]:
        _state_equal(s0, e.get_state())
    for e in envs:
        e.close()


# ---- 4. it does something, and only when asked ----
def _fifty_steps(env):
    env.reset_tensor()
    out = []
    for k in range(50):
        act = env.random_actions_tensor(k)
        out.append([t.clone() for t in env.step_tensor(act)])
    torch.cuda.synchronize()
    return out


def _all_equal(a, b):
    return all(torch.equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def test_warm_start_acts_only_when_asked(usim):
    plain, off, on = _env(usim, 300), _env(usim, 300, warm_start=0), _env(usim, 300, warm_start=1)
    rp, r0, r1 = _fifty_steps(plain), _fifty_steps(off), _fifty_steps(on)
    assert _all_equal(rp, r0)
    assert "solver_warm_start" not in off.get_state() and "solver_warm_start" in on.get_state()
    assert any(not torch.equal(a[0][:, :3], b[0][:, :3]) for a, b in zip(r0, r1))          # some contact-force channel
    for e in (plain, off, on):
        e.close()
    for torso, n in (("rigid", 300), ("full", 32)):
        a, b = _env(usim, n, torso, warm_start=0), _env(usim, n, torso, warm_start=1)
        assert _all_equal(_fifty_steps(a), _fifty_steps(b)), torso
        assert a.lib.usim_get_warm_start(a._handle, np.zeros((n, 72), np.float32).ctypes.data) == -1     # USIM_ERR_INVALID: no top-face warm start on this handle
        assert a.lib.usim_has_warm_start(a._handle) == 0 and b.lib.usim_has_warm_start(b._handle) == 0
        a.close(); b.close()
    with pytest.raises(RuntimeError):
        _env(usim, 16, warm_start=2)


# ---- 5. episode starts are cold ----
def test_warm_start_episode_starts_are_cold(usim):
    n = 256
    env = _env(usim, n, **WARM)
    env.reset_tensor()
    env.rollout_random(0, 30)
    torch.cuda.synchronize()
    w = env.get_state()["solver_warm_start"]
    assert w.shape == (n, 72) and (w[:, :8] >= 0).any() and (w[:, :8] < 99).all()
    mask = np.zeros(n, np.uint8); mask[::2] = 1
    env.reset_tensor(mask)
    torch.cuda.synchronize()
    w2 = env.get_state()["solver_warm_start"]
    assert (w2[::2, :8] == -1).all() and (w2[::2, 8:] == 0).all()
    assert np.array_equal(w2[1::2], w[1::2]) and (w2[1::2, :8] >= 0).any()
    env.close()
    # an environment auto-reset in a step == a handle given the same episode by usim_reset_explicit and nothing else (position noise off, so that the explicit
    # parameters say everything the bank's draw did); b comes with a kept list of its own, which the explicit reset must drop
    kw = dict(WARM, initial_probe_pos_randomization=False)
    a = _env(usim, n, **kw)
    a.reset_tensor()
    k, done = 0, None
    while done is None or not done.any():
        _, _, d = a.step_tensor(a.random_actions_tensor(k))
        torch.cuda.synchronize()
        done = d.cpu().numpy().astype(bool); k += 1
        assert k < 400
    st = a.get_state()
    assert (st["solver_warm_start"][done, :8] == -1).all() and (st["solver_warm_start"][~done, :8] >= 0).any()
    b = _env(usim, n, **kw)
    b.reset_tensor()
    b.rollout_random(0, 30)
    assert (b.get_state()["solver_warm_start"][done, :8] >= 0).any()
    params = np.concatenate([st["traj_start"], st["traj_end"], st["u0"][:, None], np.zeros((n, 3), np.float32), st["stiffness"][:, None], st["damping"][:, None],
                             st["mu"][:, None]], axis=1).astype(np.float32)
    b.reset_explicit_tensor(params, mask=done.astype(np.uint8))
    torch.cuda.synchronize()
    sb = b.get_state()
    assert (sb["solver_warm_start"][done, :8] == -1).all() and (sb["solver_warm_start"][done, 8:] == 0).all()
    for key in ("q", "q0", "qd", "s", "sd", "fzbar", "t"):
        assert np.array_equal(sb[key][done], st[key][done]), key
    act = a.random_actions_tensor(k).clone()
    oa = [t.clone() for t in a.step_tensor(act, auto_reset=False)]
    ob = [t.clone() for t in b.step_tensor(act, auto_reset=False)]
    torch.cuda.synchronize()
    idx = torch.as_tensor(done, device=oa[0].device)
    assert all(torch.equal(x[idx], y[idx]) for x, y in zip(oa, ob))
    assert np.array_equal(a.get_state()["solver_warm_start"][done], b.get_state()["solver_warm_start"][done])
    a.close(); b.close()


# ---- 6. checkpoint round trip: with the kept list the state is complete ----
def test_warm_start_checkpoint_round_trip(usim):
    """get_state() after 40 steps, set_state() into other handles, 40 more steps.
    The FIRST step after the restore is bit for bit the step of the handle that never left the device (d against b: observations, rewards, done flags, contact lists and
    the new kept list) -- the statement that the checkpoint is complete: a handle restored WITHOUT the kept list (c) differs in that very step.
    From the SECOND step on the two differ in the last bit whatever the solver does: usim_get_state hands out q = q0 + dq in float32 while the device integrates dq
    (usim_device.h), q0 + dq' reproduces q for the step that reads it and dq' itself is off by up to 2.4e-7 rad afterwards (measured on the cold default as well: no
    environment of 300 differs in the first step after the restore, 260 differ in some observation bit in the second).  Over the 40 steps the bit-for-bit statement is
    therefore made between handles that took the checkpoint through the same interface -- the checkpointing handle itself (restored in place) and a second one, with
    auto-reset --, the restored state, kept list included, reads back as it was written, and c and d stay within the float bars of the restored handle."""
    n = 300
    a, b, c, d = (_env(usim, n, **WARM) for _ in range(4))
    for e in (a, b, c, d):
        e.reset_tensor()
    a.rollout_random(0, 40); d.rollout_random(0, 40)
    st = a.get_state()
    assert (st["solver_warm_start"][:, :8] >= 0).any()
    a.set_state(st); b.set_state(st)
    _state_equal(st, b.get_state())
    _state_equal(st, a.get_state())
    c.set_state({k: v for k, v in st.items() if k != "solver_warm_start"})
    assert (c.get_state()["solver_warm_start"][:, :8] == -1).all()
    with pytest.raises(ValueError):
        b.set_state(dict(st, solver_warm_start=st["solver_warm_start"][:, :8]))
    _state_equal(st, b.get_state())                                      # (refused before anything was written)
    blk = [e.alloc_block(39) for e in (a, b, c, d)]
    first = []
    for e, bk in zip((a, b, c, d), blk):
        out = [t.clone() for t in e.step_tensor(e.random_actions_tensor(40))]                 # step 40 through the handle's own buffers (contact lists included)
        torch.cuda.synchronize()
        first.append(dict(obs=out[0], rew=out[1], done=out[2], contacts=e.contacts.clone(), warm=e.get_state()["solver_warm_start"]))
        e.rollout_random(41, 39, bk)
    torch.cuda.synchronize()
    # the first step after the restore: the restored handle against the one that never left the device, bit for bit
    assert int(first[3]["contacts"][:, 0].sum()) > 0 and (first[3]["warm"][:, :8] >= 0).any()
    for key in ("obs", "rew", "done", "contacts"):
        assert torch.equal(first[3][key], first[1][key]), key
    assert np.array_equal(first[3]["warm"], first[1]["warm"])
    # ... and without the kept list that step starts cold: other bits
    assert not torch.equal(first[1]["obs"], first[2]["obs"])
    assert int(blk[0]["done"].sum()) > 0
    for key in ("obs", "rew", "done"):
        assert torch.equal(blk[0][key], blk[1][key]), key
    _state_equal(a.get_state(), b.get_state())
    sb = b.get_state()
    for other, ob in ((c, blk[2]), (d, blk[3])):
        same = (blk[1]["done"] == ob["done"]).all(0).cpu().numpy()
        assert same.mean() >= 0.99
        so = other.get_state()
        for key in ("q", "qd", "s", "sd"):
            x, y = np.asarray(sb[key], np.float64)[same], np.asarray(so[key], np.float64)[same]
            assert np.abs(x - y).max() / max(np.abs(x).max(), 1e-12) < 1e-3, key
    # a checkpoint of a warm run loads into a handle without a warm start (which does not use the list)
    cold = _env(usim, n)
    cold.reset_tensor()
    cold.set_state(st)
    assert "solver_warm_start" not in cold.get_state()
    for e in (a, b, c, d, cold):
        e.close()


# ---- 7. what stopping at 18 warm iterations costs ----
def converged_comparison(usim, mode, n, steps=200, gpu_extra=None):
    """the body of test_gpu_parity.test_default_solver_against_a_converged_solve: environments that left the converged run's decisions, razor edges among them, worst state error"""
    env, ora = _mk(usim, n, "soft", mode, gpu_extra=gpu_extra, ora_extra=dict(cone_solver=1, pgs_iters=30), omp=n > 256)
    env.reset(); ora.reset()
    same = np.ones(n, dtype=bool)
    razor = 0
    worst = {k: 0.0 for k in ("q", "qd", "s", "sd")}
    for k in range(steps):
        a = ora.random_actions(k)
        _, _, done_o, _, con_o = ora.step(a)
        _, _, done_g, _ = env.step(a.astype(np.float32))
        con_g = env.contacts.cpu().numpy()
        mism = ((done_g != done_o) | (con_g != con_o).any(1)) & same
        if mism.any():
            inf = ora.last_info()
            razor += sum(1 for i in np.nonzero(mism)[0] if _razor_edge(inf, i))
        same &= ~mism
        if k % 10 == 9 or k == steps - 1:
            sg, so = env.get_state(), ora.get_state()
            for key in worst:
                a_, b_ = np.asarray(sg[key], dtype=np.float64)[same], so[key][same]
                worst[key] = max(worst[key], float(np.abs(a_ - b_).max() / max(np.abs(so[key]).max(), 1e-12)))
    env.close()
    return int((~same).sum()), razor, worst


@pytest.mark.parametrize("mode", MODES)
def test_warm_18_against_a_converged_solve(usim, mode):
    """18 warm iterations against the converged Gauss-Seidel (30 sweeps), 1024 environments x 200 steps: at most 1 % leave the converged decisions beyond razor edges, razor
    edges at most 2 %, every state field within 1e-3 while they agree (the rule of test_default_solver_against_a_converged_solve)."""
    os.environ.setdefault("OMP_NUM_THREADS", str(min(os.cpu_count() or 1, 64)))
    n = 1024
    left, razor, worst = converged_comparison(usim, mode, n, gpu_extra=dict(WARM))
    print(f"warm 18 vs converged, {mode}, n = {n}: {left} left ({razor} on a razor edge), worst state error {max(worst.values()):.2e}")
    assert razor <= max(5, 0.02 * n) and left - razor <= 0.01 * n, f"{left} of {n} environments left the converged trajectory's decisions ({razor} of them on a razor edge)"
    assert max(worst.values()) < 1e-3, worst
