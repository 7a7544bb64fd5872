"""The arm wave of the split kernel with 16-lane groups writes the REPORT of a pass -- probe torque sensor, observation row, every output row of the transition,
the state words -- one pass late where another pass of the launch follows (csrc/usim_step16.h arm_report_late): in its wait between hand-offs (2) and (3) of the
next pass, from words it parked in its own area of the environment's mailbox block.  The last pass of a launch writes the pending report and then its own.
None of that may show: the single-step launches (steps_per_launch 1) and the single-wave kernel (lanes_per_env 16) keep the code they had, and every launch
length must give their bits -- obs, act, rew, done of every step, the optional outputs and the state a rollout leaves behind (save_envs).

Soft torso, 21 environments (one full workgroup of 16 and a ragged one), lanes_per_env 32, at most 37 control steps.
Launch lengths 2 (one deferred report and the flush), 3 and 5 (middle passes; the last launches of 37 steps are 1 and 2 steps long).

Optional outputs: terminal_obs, contacts, episode_return, episode_length, status and the step log are written by multi-step launches into the environment's own
buffers (rollout_random without a block); act is the block's own entry.  All of DevIO's outputs can be reached from Python."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, SEED, OFFSET = 21, 3, 4096
SPLS = [2, 3, 5]
T_LONG = 37
# the episode case of tests/test_gpu_lattice_ahead.py: horizon 6, 18 steps; every other environment is reset by mask before step 4
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
        g, r = np.ascontiguousarray(got[name]), np.ascontiguousarray(ref[name])
        assert g.shape == r.shape and g.dtype == r.dtype, f"{what}: {name}"
        same = (g.view(np.uint8) == r.view(np.uint8)).reshape(g.shape[0], -1).all(1)
        assert same.all(), f"{what}: {name} differs first at row {int(np.nonzero(~same)[0][0])}"


_REF = {}


def _reference(usim, key, T, mask_at=None, **kw):
    """steps_per_launch = 1: the single-step kernels; computed once per case and left unchanged"""
    if key not in _REF:
        _REF[key] = _rollout(usim, 1, T, mask_at, **kw)
    return _REF[key]


def _pass_kinds(T, mask_at, spl):
    """steps that are the first, a middle and the last pass of their launch when a rollout runs in launches of spl steps"""
    first, middle, last = set(), set(), set()
    for a, b in _segments(T, mask_at):
        for k0 in range(a, b, spl):
            k1 = min(k0 + spl, b)
            first.add(k0)
            last.add(k1 - 1)
            middle.update(range(k0 + 1, k1 - 1))
    return first, middle, last


# ---- launch lengths ----
@pytest.mark.parametrize("spl", SPLS)
def test_launch_length_does_not_show(usim, spl):
    ref = _reference(usim, "long", T_LONG)
    _assert_same(_rollout(usim, spl, T_LONG), ref, f"steps_per_launch {spl}")


def test_single_wave_kernel_agrees(usim):
    ref = _reference(usim, "long", T_LONG)
    _assert_same(_rollout(usim, 1, T_LONG, lanes=16), ref, "lanes_per_env 16 steps_per_launch 1")


# ---- episodes that end on a first, a middle and the last pass of a launch ----
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm_start"])
def test_episodes_end_on_every_kind_of_pass(usim, warm):
    kw = dict(horizon=HORIZON, early_termination=True)
    if warm:
        kw.update(warm_start=1, pgs_iters=18)
    ref = _reference(usim, "episodes-warm" if warm else "episodes", T_EP, MASK_AT, **kw)
    done = ref["done"].astype(bool)                                      # [T, n]
    seen = {"first": False, "middle": False, "last": False}
    for spl in SPLS:
        first, middle, last = _pass_kinds(T_EP, MASK_AT, spl)
        seen["first"] |= any(done[k].any() for k in first)
        seen["middle"] |= any(done[k].any() for k in middle)
        seen["last"] |= any(done[k].any() for k in last)
        _assert_same(_rollout(usim, spl, T_EP, MASK_AT, **kw), ref, f"steps_per_launch {spl}")
    for kind, ok in seen.items():
        assert ok, f"the reference has no episode that ends on a {kind} pass of a launch"
    # the row of a step at which an episode ended holds the observation the reset bank prepared for the next one (arm at rest: no hand velocity, no mean velocity yet),
    # the row of the step behind it is an ordinary one
    obs = ref["obs"]
    ks, es = np.nonzero(done)
    assert len(ks)
    assert not obs[ks, es, 6:9].any() and (obs[ks, es, 11] == np.float32(0.0) - np.float32(0.04)).all(), "the row of an ending step holds the bank's observation"
    later = ks + 1 < T_EP
    assert obs[ks[later] + 1, es[later], 6:9].any(1).all(), "the row behind a reset is the step's own"


def test_terminal_rows_and_optional_outputs(usim):
    """Without a block every pass writes the environment's own buffers, the episode-end rows (terminal_obs, episode_return, episode_length) only where an episode
    ended: what remains after a rollout is the last step's rows and, per environment, the rows of its last ending -- wherever in a launch that step fell.
    Stops after 6, 10, 12 and 18 steps (horizon 6; episodes end on first, middle and last passes of the launches of 2, 3 and 5 steps)."""
    stops = [6, 10, 12, 18]

    def run(spl):
        env = _env(usim, horizon=HORIZON, early_termination=True)
        env.set_steps_per_launch(spl)
        env.enable_step_log(True)
        env.reset_tensor()
        out, a = {}, 0
        for b in stops:
            env.rollout_random(a, b - a)
            a = b
            torch.cuda.synchronize()
            for name, t in (("obs", env._obs), ("rew", env._rew), ("done", env._done), ("terminal_obs", env.terminal_obs), ("contacts", env.contacts),
                            ("episode_return", env.episode_return), ("episode_length", env.episode_length), ("status", env.status), ("log", env.step_log)):
                out[f"{name}@{b}"] = t.cpu().numpy().copy()
        out["snap"] = env.save_envs().cpu().numpy().copy()
        env.close()
        return out

    ref = run(1)
    assert ref["episode_length@18"].max() == HORIZON and ref["terminal_obs@18"].any()
    for spl in SPLS:
        _assert_same(run(spl), ref, f"own buffers, steps_per_launch {spl}")


# ---- the rollout block's rows ----
def test_rollout_block_rows(usim):
    """A row is written by the pass after its own: T = 7 steps in launches of 3 + 3 + 1, as one call over the block and as three calls into slices of it; the rows
    around the block keep what they held."""
    T = 7
    ref = _reference(usim, "rows", T)

    def run(calls):
        env = _env(usim)
        env.set_steps_per_launch(3)
        env.reset_tensor()
        blk = env.alloc_block(T + 2)
        for v in blk.values():
            v.fill_(77)
        for a, b in calls:
            env.rollout_random(a, b - a, {k: v[1 + a:1 + b] for k, v in blk.items()})
        snap = env.save_envs()
        torch.cuda.synchronize()
        for name, v in blk.items():
            h = v.cpu().numpy()
            assert (h[0] == 77).all() and (h[T + 1] == 77).all(), f"{name}: a row outside the block was written"
        out = {k: v[1:T + 1].cpu().numpy().copy() for k, v in blk.items()}
        out["snap"] = snap.cpu().numpy().copy()
        env.close()
        return out

    _assert_same(run([(0, 7)]), ref, "one call, launches of 3 + 3 + 1")
    _assert_same(run([(0, 3), (3, 6), (6, 7)]), ref, "three calls into slices of one block")


# ---- caller-supplied action blocks ----
def test_rollout_actions(usim):
    rnd = _reference(usim, "long", T_LONG)
    acts = torch.as_tensor(rnd["act"], device="cuda:0")
    ref = _rollout(usim, 1, T_LONG, actions=acts)
    for name in ("obs", "rew", "done", "snap"):                          # the same actions: the same bits as the rollout that drew them
        assert np.array_equal(ref[name].view(np.uint8), rnd[name].view(np.uint8)), name
    for spl in SPLS:
        _assert_same(_rollout(usim, spl, T_LONG, actions=acts), ref, f"rollout_actions steps_per_launch {spl}")


# ---- physics substeps ----
@pytest.mark.parametrize("mode", ["tracking", "fixed"])
def test_physics_substeps(usim, mode):
    """control_freq 250: two physics passes per control step; the transition is written by the second one's report only, the state words by both"""
    kw = dict(mode=mode, control_freq=250, horizon=HORIZON, early_termination=True)
    ref = _reference(usim, f"substeps-{mode}", T_EP, MASK_AT, **kw)
    assert ref["done"].any()
    for spl in (2, 3):
        _assert_same(_rollout(usim, spl, T_EP, MASK_AT, **kw), ref, f"{mode} substeps 2 steps_per_launch {spl}")
