"""The random action of usim_rollout_random does not depend on where in a launch it is drawn.  In resident multi-step launches the arm wave of the split kernel
draws the NEXT pass's action while it waits for the contact solve (csrc/usim_step16.h step16_one AHEAD); the first pass of a launch, single-step launches and the
single-wave kernels draw in place.  So the rollout blocks must not depend on steps_per_launch, and the `act` rows must be the oracle's random_actions(k) for the same
seed, environment offset and step index (which pins the counter against an off-by-one).

Soft torso, 40 environments (two and a half workgroups of 16-lane groups: ragged), 14 steps, horizon 6 so that auto-resets fall inside the launches,
env_offset 4096.  Launch lengths 2, 3, 5 and 14 put a launch boundary before, at and after the steps that follow an episode end."""
import numpy as np
import pytest
import torch

from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

N, T, HORIZON, OFFSET, SEED = 40, 14, 6, 4096, 3
MODES = ["tracking", "fixed", "variable_z", "wrench"]


def _env(usim, mode="tracking", **kw):
    opts = dict(usim.default_robosuite_kwargs())
    opts["controller_configs"] = dict(opts["controller_configs"], impedance_mode=mode)
    opts.update(kw, horizon=HORIZON)
    return usim.UltrasoundVecEnv(N, device="cuda:0", seed=SEED, env_offset=OFFSET, torso="soft", **opts)


def _rollout(usim, spl, mode="tracking", **kw):
    """the blocks of T steps from a fresh reset, steps_per_launch = spl, as host arrays"""
    env = _env(usim, mode, **kw)
    env.set_steps_per_launch(spl)
    env.reset_tensor()
    blk = env.alloc_block(T)
    blk["act"].fill_(-7.0)
    env.rollout_random(0, T, blk)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().copy() for k, v in blk.items()}
    env.close()
    return out


def _assert_same(got, ref, what):
    assert got.keys() == ref.keys()
    for name in ("obs", "act", "rew", "done"):
        same = (got[name].view(np.uint8) == ref[name].view(np.uint8)).reshape(T, -1).all(1)
        assert same.all(), f"{what}: {name} differs first at step {int(np.nonzero(~same)[0][0])}"


def _oracle_actions(mode, **ora_kw):
    ora = Oracle(N, precision="f64", mode=mode, torso="top", seed=SEED, env_offset=OFFSET, **ora_kw)
    return np.stack([ora.random_actions(k).astype(np.float32) for k in range(T)])


_REF = {}


def _reference(usim, lanes):
    """steps_per_launch = 1 (every action drawn in place), computed once per mapping"""
    if lanes not in _REF:
        _REF[lanes] = _rollout(usim, 1, lanes_per_env=lanes)
    return _REF[lanes]


@pytest.mark.parametrize("lanes", [32, 64, 16])
@pytest.mark.parametrize("spl", [2, 3, 5, 14])
def test_launch_length_does_not_show(usim, lanes, spl):
    ref = _reference(usim, lanes)
    assert int(ref["done"].sum()) >= 2 * N                                # episodes end inside the block
    _assert_same(_rollout(usim, spl, lanes_per_env=lanes), ref, f"lanes {lanes} steps_per_launch {spl}")


@pytest.mark.parametrize("lanes", [32, 64, 16])
def test_actions_are_the_oracles_for_the_step_index(usim, lanes):
    want = _oracle_actions("tracking")
    for spl in (1, 5):
        got = _reference(usim, lanes) if spl == 1 else _rollout(usim, spl, lanes_per_env=lanes)
        assert np.array_equal(got["act"], want), f"lanes {lanes} steps_per_launch {spl}"


@pytest.mark.parametrize("lanes", [32, 64, 16])
@pytest.mark.parametrize("mode", ["tracking", "fixed"])
def test_action_is_held_over_physics_substeps(usim, lanes, mode):
    """control_freq 250: two physics substeps per control step; the action (and the goal of the `fixed` mode, anchored at the first substep) is that of the control step"""
    ref = _rollout(usim, 1, mode, lanes_per_env=lanes, control_freq=250)
    assert np.array_equal(ref["act"], _oracle_actions(mode, substeps=2, control_dt=1.0 / 250))
    for spl in (2, 3, 14):
        _assert_same(_rollout(usim, spl, mode, lanes_per_env=lanes, control_freq=250), ref, f"{mode} lanes {lanes} substeps 2 steps_per_launch {spl}")


@pytest.mark.parametrize("mode", MODES)
def test_every_controller_mode(usim, mode):
    ref = _rollout(usim, 1, mode)
    assert np.array_equal(ref["act"], _oracle_actions(mode))
    _assert_same(_rollout(usim, 3, mode), ref, f"mode {mode} steps_per_launch 3")
