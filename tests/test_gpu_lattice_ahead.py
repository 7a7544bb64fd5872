"""The split kernel with 16-lane groups in multi-step launches lets its lattice wave run from the integration of pass k straight into the right-hand side and the
matrix-core solve of pass k + 1 (csrc/usim_step16.h lattice_ahead): it assumes that no episode of its wave ended, meets the arm wave at hand-off (1) only, and
runs the two phases again where the arm wave reports a new episode.  Hand-off (4) and the barrier between the passes exist on the last pass of a launch only.
None of that may show: the single-step launches (steps_per_launch 1) and the single-wave kernel (lanes_per_env 16) keep the code they had, and every launch
length must give their bits -- obs, act, rew, done of every step and the state a rollout leaves behind (save_envs: scalars, lattice, warm rows).

Soft torso, 21 environments (one full workgroup of 16 and a ragged one), at most 37 control steps."""
import os
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N, SEED, OFFSET = 21, 3, 4096
SPLS = [2, 5, 14, 64]                                  # 64: every rollout call is a single launch
LAT0, LAT1 = 40, 240                                   # lattice words of a snapshot row (csrc/usim_device.h: F_NSCALAR scalars, then LAT_ENV_WORDS; warm words behind)

# the long case: default horizon, 37 steps (launches of 2 / 5 / 14 leave a last launch of 1 / 2 / 9 steps)
T_LONG = 37
# the episode case: horizon 6, 18 steps; every other environment is reset by mask after step 3, so that the two halves of every quad (the four environments of a
# wave pair) end at different steps -- 5, 11, 17 and 9, 15 where nothing terminates early -- and the rollout ends on a step at which episodes end
HORIZON, T_EP, MASK_AT = 6, 18, 4
MASK = (np.arange(N) % 2 == 1)


def _env(usim, lanes=32, mode="tracking", **kw):
    opts = dict(usim.default_robosuite_kwargs())
    opts["controller_configs"] = dict(opts["controller_configs"], impedance_mode=mode)
    opts.update(kw)
    return usim.UltrasoundVecEnv(N, device="cuda:0", seed=SEED, env_offset=OFFSET, torso="soft", lanes_per_env=lanes, **opts)


def _segments(T, mask_at):
    return [(0, T)] if mask_at is None else [(0, mask_at), (mask_at, T)]


def _rollout(usim, spl, T, mask_at=None, actions=None, **kw):
    """T steps from a fresh reset with steps_per_launch = spl (random actions, or the caller's block `actions` [T, n, A]); with mask_at the environments of MASK are
    reset before step mask_at.  Returns the blocks and the snapshot of the final state as host arrays."""
    env = _env(usim, **kw)
    env.set_steps_per_launch(spl)
    env.reset_tensor()
    blk = env.alloc_block(T, with_actions=actions is None)
    for a, b in _segments(T, mask_at):
        if a:
            env.reset_tensor(torch.as_tensor(MASK))
        part = {k: v[a:b] for k, v in blk.items()}
        if actions is None:
            env.rollout_random(a, b - a, part)
        else:
            env.rollout_actions(actions[a:b].contiguous(), part)
    snap = env.save_envs()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().copy() for k, v in blk.items()}
    out["snap"] = snap.cpu().numpy().copy()
    env.close()
    return out


def _assert_same(got, ref, what):
    assert got.keys() == ref.keys()
    for name in got:
        if name == "snap":
            continue
        T = ref[name].shape[0]
        same = (got[name].view(np.uint8) == ref[name].view(np.uint8)).reshape(T, -1).all(1)
        assert same.all(), f"{what}: {name} differs first at step {int(np.nonzero(~same)[0][0])}"
    same = (got["snap"].view(np.uint8) == ref["snap"].view(np.uint8)).reshape(N, -1).all(1)
    assert same.all(), f"{what}: the saved state differs for environments {np.nonzero(~same)[0].tolist()}"


_REF = {}


def _reference(usim, key, T, mask_at=None, **kw):
    """steps_per_launch = 1: the single-step kernels; computed once per case and left unchanged"""
    if key not in _REF:
        _REF[key] = _rollout(usim, 1, T, mask_at, **kw)
    return _REF[key]


def _launch_ends(T, mask_at, spl):
    """(last steps of the launches, steps that are neither first nor last of theirs) of a rollout in launches of spl steps"""
    last, middle = set(), set()
    for a, b in _segments(T, mask_at):
        for k0 in range(a, b, spl):
            k1 = min(k0 + spl, b)
            last.add(k1 - 1)
            middle.update(range(k0 + 1, k1 - 1))
    return last, middle


# ---- launch length does not show ----
@pytest.mark.parametrize("spl", SPLS)
def test_launch_length_does_not_show(usim, spl):
    ref = _reference(usim, "long", T_LONG)
    _assert_same(_rollout(usim, spl, T_LONG), ref, f"steps_per_launch {spl}")


def test_single_wave_kernel_agrees(usim):
    ref = _reference(usim, "long", T_LONG)
    for spl in (1, 14):
        _assert_same(_rollout(usim, spl, T_LONG, lanes=16), ref, f"lanes_per_env 16 steps_per_launch {spl}")


# ---- episodes ending inside a launch ----
def _episode_case(usim, key, **kw):
    ref = _reference(usim, key, T_EP, MASK_AT, horizon=HORIZON, **kw)
    done = ref["done"].astype(bool)                                      # [T, n]
    seen_partial = seen_last = seen_middle = False
    quads = [np.arange(q, min(q + 4, N)) for q in range(0, N, 4)]
    for k in range(T_EP):
        seen_partial |= any(0 < done[k, q].sum() < len(q) for q in quads)
    for spl in SPLS:
        last, middle = _launch_ends(T_EP, MASK_AT, spl)
        seen_last |= any(done[k].any() for k in last)
        seen_middle |= any(done[k].any() for k in middle)
        _assert_same(_rollout(usim, spl, T_EP, MASK_AT, horizon=HORIZON, **kw), ref, f"{key} steps_per_launch {spl}")
    assert seen_partial, "no step at which some but not all environments of a quad ended"
    assert seen_last, "no episode ended on the last step of a launch"
    assert seen_middle, "no episode ended on a middle step of a launch"
    return ref, done


def test_episodes_end_inside_a_launch(usim):
    ref, done = _episode_case(usim, "episodes")
    # the rollout stops right after a step at which episodes ended: their lattice is at rest in the saved state (every launch length was compared with it above),
    # the lattice of the others is not
    ended = done[T_EP - 1]
    assert ended.any() and not ended.all()
    lat = ref["snap"][:, LAT0:LAT1]
    assert not lat[ended].any(), "an episode that has just begun must have its lattice at rest"
    assert all(lat[i].any() for i in np.nonzero(~ended)[0])


def test_single_wave_kernel_agrees_on_the_episode_case(usim):
    ref = _reference(usim, "episodes", T_EP, MASK_AT, horizon=HORIZON)
    _assert_same(_rollout(usim, 14, T_EP, MASK_AT, horizon=HORIZON, lanes=16), ref, "lanes_per_env 16 steps_per_launch 14")


# ---- warm-start handle, then physics substeps ----
def test_warm_start_handle(usim):
    ref, done = _episode_case(usim, "warm", warm_start=1, pgs_iters=18)
    ended = done[T_EP - 1]
    assert ended.any()
    assert ref["snap"].shape[1] > LAT1                                   # the rows carry the warm words
    warm = ref["snap"][:, LAT1:]
    assert (warm[ended][:, :8].view(np.int32) == -1).all() and not warm[ended][:, 8:].any(), "an episode starts cold"


@pytest.mark.parametrize("mode", ["tracking", "fixed"])
def test_physics_substeps(usim, mode):
    """control_freq 250: two physics passes per control step -- t advances on the first one only, also where the lattice wave has advanced it ahead"""
    _episode_case(usim, f"substeps-{mode}", mode=mode, control_freq=250)


# ---- caller-supplied action blocks ----
def test_rollout_actions(usim):
    rnd = _reference(usim, "long", T_LONG)
    acts = torch.as_tensor(rnd["act"], device="cuda:0")
    ref = _rollout(usim, 1, T_LONG, actions=acts)
    for name in ("obs", "rew", "done"):                                  # the same actions: the same bits as the rollout that drew them
        assert np.array_equal(ref[name].view(np.uint8), rnd[name].view(np.uint8)), name
    assert np.array_equal(ref["snap"].view(np.uint8), rnd["snap"].view(np.uint8))
    for spl in SPLS:
        _assert_same(_rollout(usim, spl, T_LONG, actions=acts), ref, f"rollout_actions steps_per_launch {spl}")
    _assert_same(_rollout(usim, 14, T_LONG, actions=acts, lanes=16), ref, "rollout_actions lanes_per_env 16 steps_per_launch 14")


# ---- barrier count ----
def test_both_roles_execute_the_barriers_of_the_table(usim):
    """BARRIER INVARIANT at usim_step32_kernel: a multi-step launch of n passes executes 3 n + 2 workgroup barriers in each role (table copy, hand-offs (1)-(3) of
    every pass, hand-off (4) of the last).  The profiling build counts them per role: a launch of four passes right after a reset (contact slots overflow), then two
    more, on the ragged batch."""
    nsub = 4
    csrc = ROOT / "robotic-ultrasound-imaging_amd" / "csrc"
    prof = ROOT / "robotic-ultrasound-imaging_amd" / "lib" / "libusim_prof.so"
    subprocess.run(["make", "-s", "-C", str(csrc), "prof"], check=True)
    code = textwrap.dedent(f"""
        import importlib, sys
        sys.path.insert(0, {str(ROOT)!r})
        usim = importlib.import_module("robotic-ultrasound-imaging_amd")
        env = usim.UltrasoundVecEnv({N}, device="cuda:0", seed=3, lanes_per_env=32, **usim.default_robosuite_kwargs())
        env.reset_tensor()
        for k in range(3):
            t = env.profile_step_raw({nsub} * k, n=48)
            print(k, t[46], t[47])
        env.close()
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, USIM_LIB=str(prof), USIM_PROFILE_NSUB=str(nsub)))
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines() if line[:1].isdigit()]
    assert len(rows) == 3
    for k, arm, lat in rows:
        assert arm == lat == 3 * nsub + 2, (k, arm, lat)
