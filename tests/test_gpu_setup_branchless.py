"""The split step kernel with 16-lane groups (lanes_per_env 32) sets the rows of the contact solve up without a divergent region: a lane whose contact slot is
empty runs the owning lanes' code on a zero frame, and when the wave holds four or more contacts the four Delassus blocks of a half are formed in one straight
line (csrc/usim_contact.h contact_row_geometry<true>, contact_row_residual<true>, delassus_blocks<.., true>; DESIGN.md section 4.1: finite everywhere, exact
zeros where they are summed).  The single-wave 16-lane kernels (lanes_per_env 16) keep the set-up with the branches, instruction for instruction, so they are
the reference here: every output of every step and the state afterwards must have their bits, and be finite, in the cases the new form could break --

  * a ragged batch: 19 environments = one full workgroup of 16 and one with 3 live and 13 absent environments, so that a wave holds absent environments
    beside live ones; and the same 19 environments inside a full batch of 32;
  * the steps right after a reset, where more than eight elements penetrate: eight filled slots, the `upper` halves of the blocks;
  * empty slots beside full ones in one wave (counts 0, 1-4 and 5-8 among its four environments) and a wave without any contact, reached with `fixed`-mode action
    sequences that lift some probes of a quad off the torso while the others press (chosen with the CPU oracle: seed 18, the lift mask below; the float32 and
    the float64 oracle report the same counts at every step);
  * the warm start, whose matching and whose product A s0 read the same rows.

Shapes: 16 to 32 environments, at most 64 steps; a reference is computed once per case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WARM = {"warm_start": 1, "pgs_iters": 18}


def _env(usim, n, lanes, seed=3, mode=None, **kw):
    opts = dict(usim.default_robosuite_kwargs())
    if mode is not None:
        opts["controller_configs"] = dict(opts["controller_configs"], impedance_mode=mode)
    opts.update(kw)
    return usim.UltrasoundVecEnv(n, device="cuda:0", seed=seed, torso="soft", lanes_per_env=lanes, **opts)


def _host(env, blk, snap):
    out = {k: v.cpu().numpy().copy() for k, v in blk.items()}
    out["snap"] = snap.cpu().numpy().copy()
    st = env.get_state()
    out["state"] = np.concatenate([np.asarray(st[k], dtype=np.float64).reshape(env.num_envs, -1) for k in ("q", "qd", "s", "sd", "vbar", "fzbar", "fzprev", "dfz")], axis=1)
    return out


def _random_rollout(usim, n, lanes, launches, **kw):
    """steps with the in-kernel actions from a fresh reset, `launches` = [(steps, steps_per_launch), ...]: the blocks of all steps and the state afterwards"""
    env = _env(usim, n, lanes, **kw)
    env.reset_tensor()
    total = sum(s for s, _ in launches)
    blk = env.alloc_block(total)
    first = 0
    for steps, spl in launches:
        env.set_steps_per_launch(spl)
        part = {k: v[first:first + steps] for k, v in blk.items()}
        env.rollout_random(first, steps, part)
        first += steps
    snap = env.save_envs()
    torch.cuda.synchronize()
    out = _host(env, blk, snap)
    env.close()
    return out


def _assert_same(got, ref, live, what):
    """bits of obs / rew / done / act of every step and of the saved state, for the first `live` environments; all of it finite"""
    for name in ("obs", "rew", "done", "act"):
        g, r = got[name][:, :live], ref[name][:, :live]
        if g.dtype.kind == "f":
            assert np.isfinite(g).all(), f"{what}: {name} is not finite"
        same = (np.ascontiguousarray(g).view(np.uint8) == np.ascontiguousarray(r).view(np.uint8)).reshape(g.shape[0], -1).all(1)
        assert same.all(), f"{what}: {name} differs first at step {int(np.nonzero(~same)[0][0])}"
    assert np.isfinite(got["state"][:live]).all(), f"{what}: the arm or lattice state is not finite"
    g, r = got["snap"][:live], ref["snap"][:live]                              # (opaque rows that hold integer words too: compared, not tested for finiteness)
    same = (np.ascontiguousarray(g).view(np.uint8) == np.ascontiguousarray(r).view(np.uint8)).reshape(live, -1).all(1)
    assert same.all(), f"{what}: the saved state differs for environments {np.nonzero(~same)[0].tolist()}"


_REF = {}


def _ragged_reference(usim, case):
    """19 environments on the single-wave 16-lane mapping, 16 steps one launch each: once per case"""
    if case not in _REF:
        _REF[case] = _random_rollout(usim, 19, 16, [(16, 1)], **(WARM if case == "warm" else {}))
    return _REF[case]


# ---- 1. ragged batch, cold and with the warm start: 8 steps from the reset in one launch, 8 more in launches of 4 ------------------------------------------
@pytest.mark.parametrize("case", ["cold", "warm"])
def test_ragged_batch(usim, case):
    kw = WARM if case == "warm" else {}
    ref = _ragged_reference(usim, case)
    assert np.isfinite(ref["obs"]).all() and np.isfinite(ref["rew"]).all()
    got = _random_rollout(usim, 19, 32, [(8, 8), (8, 4)], **kw)
    _assert_same(got, ref, 19, f"19 environments, {case}")
    # the same environments with live neighbours in place of the absent ones
    full = _random_rollout(usim, 32, 32, [(8, 8), (8, 4)], **kw)
    _assert_same(full, ref, 19, f"the first 19 of 32 environments, {case}")


# ---- 2. right after a reset: eight filled slots, more elements penetrate than there are slots ------------------------------------------------------------------
def test_full_slots_after_reset(usim):
    n, T = 16, 4
    ref_env = _env(usim, n, 16)
    ref_env.reset_tensor()
    blk = ref_env.alloc_block(T)
    counts = []
    for k in range(T):
        act = ref_env.random_actions_tensor(k)
        obs, rew, done = ref_env.step_tensor(act)
        blk["obs"][k].copy_(obs); blk["rew"][k].copy_(rew); blk["done"][k].copy_(done); blk["act"][k].copy_(act)
        counts.append(ref_env.contacts[:, 0].clone())
    snap = ref_env.save_envs()
    torch.cuda.synchronize()
    ref = _host(ref_env, blk, snap)
    cnt = torch.stack(counts).cpu().numpy()
    ref_env.close()
    assert (cnt[0] == 8).any(), "no environment fills its eight slots at the first step"
    assert (cnt[0].reshape(4, 4).max(1) > 4).any() and (cnt[0] == 0).any()
    got = _random_rollout(usim, n, 32, [(T, T)])
    _assert_same(got, ref, n, "first steps after the reset")


# ---- 3. empty slots beside full ones in one wave, and a wave without a contact -----------------------------------------------------------------------------------
LIFT_SEED, LIFT_T = 18, 64
LIFT = np.array([0, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1], dtype=bool)       # environments whose probe is lifted (+z); the others press (-z)


def test_empty_slots_beside_full_ones(usim):
    n = LIFT.size
    acts = torch.zeros((LIFT_T, n, 6), dtype=torch.float32)
    acts[:, :, 2] = torch.where(torch.from_numpy(LIFT), 1.0, -1.0)
    ref_env = _env(usim, n, 16, seed=LIFT_SEED, mode="fixed")
    assert ref_env.action_dim == 6
    acts = acts.to(ref_env.device).contiguous()
    ref_env.reset_tensor()
    blk = ref_env.alloc_block(LIFT_T, with_actions=False)
    counts = []
    for k in range(LIFT_T):
        obs, rew, done = ref_env.step_tensor(acts[k])
        blk["obs"][k].copy_(obs); blk["rew"][k].copy_(rew); blk["done"][k].copy_(done)
        counts.append(ref_env.contacts[:, 0].clone())
    snap = ref_env.save_envs()
    torch.cuda.synchronize()
    ref = _host(ref_env, blk, snap)
    cnt = torch.stack(counts).cpu().numpy().reshape(LIFT_T, n // 4, 4)             # [step, wave of the split kernel, environment of the wave]
    ref_env.close()
    mixed = (cnt == 0).any(2) & ((cnt >= 1) & (cnt <= 4)).any(2) & (cnt >= 5).any(2)
    assert mixed.any(), "no wave holds environments with 0, 1-4 and 5-8 contacts at one step"
    assert (cnt.max(2) == 0).any(), "no wave is without a contact at some step"
    assert (cnt == 8).any() and ref["done"].astype(bool).any()

    env = _env(usim, n, 32, seed=LIFT_SEED, mode="fixed")
    env.reset_tensor()
    got_blk = env.alloc_block(LIFT_T, with_actions=False)
    env.rollout_actions(acts, got_blk)
    got_snap = env.save_envs()
    torch.cuda.synchronize()
    got = _host(env, got_blk, got_snap)
    env.close()
    ref["act"] = got["act"] = np.zeros(1, dtype=np.float32).reshape(1, 1)          # (the actions are the caller's: nothing to compare)
    _assert_same(got, ref, n, "lifted and pressed probes")
