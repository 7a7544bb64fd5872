"""The split step kernel sets the contact solve up behind hand-off (2) -- the wave's largest contact count, the operands Lambda^-1 / alpha / vs from the mailbox, the
rows and the Delassus blocks -- and hands the wrench, the count, the overflow flag and the contacts' element ids over at hand-off (3); the arm wave maps the
elements to shell ids only where a launch reports contacts (csrc/usim_step16.h, csrc/usim_contact.h).  None of that may show: every launch length of the split
kernel gives the bits of the single-wave 16-lane kernel stepping one step at a time -- obs, rew, done, act of every step and the state the rollout leaves behind --
and env.contacts (count and shell ids) of every step is that kernel's, byte for byte.

Soft torso, seed 3, the default configuration, 40 steps from a reset (the first steps overflow the eight contact slots).  16-lane groups (lanes_per_env 32): 20
environments, one full workgroup of 16 and a ragged one; 8-lane groups (lanes_per_env 64): 24 environments, a ragged workgroup of its 32.  Cold and with the warm
start (warm_start 1, pgs_iters 18); the default horizon and one of 7 steps, at which every launch length has episodes ending inside a launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, T = 3, 40
SPLS = [1, 3, 14]
HORIZON = 7                                            # episodes end at steps 6, 13, 20, 27, 34: middle steps of the launches of 3 (13, 34) and of 14 (6, 20, 34)
CASES = {"cold": {}, "cold-short": {"horizon": HORIZON}, "warm": {"warm_start": 1, "pgs_iters": 18}, "warm-short": {"warm_start": 1, "pgs_iters": 18, "horizon": HORIZON}}
GROUPS = {32: 20, 64: 24}                              # lanes_per_env of the split kernel -> environments


def _env(usim, n, lanes, **kw):
    opts = dict(usim.default_robosuite_kwargs())
    opts.update(kw)
    return usim.UltrasoundVecEnv(n, device="cuda:0", seed=SEED, torso="soft", lanes_per_env=lanes, **opts)


def _rollout(usim, n, lanes, spl, **kw):
    """T steps from a fresh reset in launches of spl steps: the blocks and the snapshot of the final state, as host arrays"""
    env = _env(usim, n, lanes, **kw)
    env.set_steps_per_launch(spl)
    env.reset_tensor()
    blk = env.alloc_block(T)
    env.rollout_random(0, T, blk)
    snap = env.save_envs()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().copy() for k, v in blk.items()}
    out["snap"] = snap.cpu().numpy().copy()
    env.close()
    return out


def _contacts(usim, n, lanes, **kw):
    """env.contacts of T single steps through step_tensor (the path that passes contacts_dev): int32 [T, n, 1 + MAXC]"""
    env = _env(usim, n, lanes, **kw)
    env.reset_tensor()
    rows = []
    for k in range(T):
        env.step_tensor(env.random_actions_tensor(k))
        rows.append(env.contacts.clone())
    torch.cuda.synchronize()
    out = torch.stack(rows).cpu().numpy()
    env.close()
    return out


_REF = {}


def _reference(usim, kind, n, case):
    """the single-wave 16-lane kernel, one step per launch: computed once per case and batch size and left unchanged"""
    key = (kind, n, case)
    if key not in _REF:
        _REF[key] = _rollout(usim, n, 16, 1, **CASES[case]) if kind == "rollout" else _contacts(usim, n, 16, **CASES[case])
    return _REF[key]


def _middle_steps(spl):
    """steps that are neither the first nor the last of their launch"""
    return {k for k0 in range(0, T, spl) for k in range(k0 + 1, min(k0 + spl, T) - 1)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("lanes", list(GROUPS))
def test_same_bits_across_mappings_and_launch_lengths(usim, lanes, case):
    n = GROUPS[lanes]
    ref = _reference(usim, "rollout", n, case)
    done = ref["done"].astype(bool)
    if "horizon" in CASES[case]:
        for spl in SPLS[1:]:
            assert any(done[k].any() for k in _middle_steps(spl)), f"no episode ends inside a launch of {spl} steps"
    for spl in SPLS:
        got = _rollout(usim, n, lanes, spl, **CASES[case])
        assert got.keys() == ref.keys() and {"obs", "rew", "done", "act", "snap"} <= got.keys()
        for name in ("obs", "rew", "done", "act"):
            same = (got[name].view(np.uint8) == ref[name].view(np.uint8)).reshape(T, -1).all(1)
            assert same.all(), f"lanes_per_env {lanes} steps_per_launch {spl} {case}: {name} differs first at step {int(np.nonzero(~same)[0][0])}"
        same = (got["snap"].view(np.uint8) == ref["snap"].view(np.uint8)).reshape(n, -1).all(1)
        assert same.all(), f"lanes_per_env {lanes} steps_per_launch {spl} {case}: the saved state differs for environments {np.nonzero(~same)[0].tolist()}"


@pytest.mark.parametrize("case", ["cold", "warm"])
@pytest.mark.parametrize("lanes", list(GROUPS))
def test_contacts_output(usim, lanes, case):
    n = GROUPS[lanes]
    ref = _reference(usim, "contacts", n, case)
    cnt = ref[:, :, 0]
    assert ((0 <= cnt) & (cnt <= 8)).all()
    # seed 3 gives both ends at either batch size in every one of the 40 steps: an environment with eight contacts (six to eight from step 24 on) and one with none;
    # asserted for step 0, right after the reset, where the slots overflow
    assert (cnt[0] > 4).any(), "step 0 reports no environment with more than four contacts"
    assert (cnt[0] == 0).any(), "step 0 reports no environment without a contact"
    shell = ref[:, :, 1:]
    k = np.arange(shell.shape[2])
    assert ((shell >= 0) == (k < cnt[:, :, None])).all(), "shell ids fill exactly the first `count` slots, -1 behind them"
    got = _contacts(usim, n, lanes, **CASES[case])
    same = (got.view(np.uint8) == ref.view(np.uint8)).reshape(T, -1).all(1)
    assert same.all(), f"lanes_per_env {lanes} {case}: env.contacts differs first at step {int(np.nonzero(~same)[0][0])}"
