"""usim_rollout_actions (include/usim.h) and its host side UltrasoundVecEnv.rollout_actions / score_block: a block of caller-supplied actions played in multi-step
launches computes the bits of the same steps one usim_step each -- every output and the state afterwards --, in every mapping, for every steps_per_launch, across
the refill period of the reset bank, with the warm start and with physics substeps.  100 environments: a ragged last workgroup in every mapping and a padded state
block of 128 (tests/test_gpu_snapshot.py).  Episodes end by the configuration: with horizon 37 every environment finishes at least 8 episodes in 300 steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 100
CASES = {"rigid": dict(torso="rigid"), "soft16": dict(lanes_per_env=16), "soft32": dict(lanes_per_env=32), "soft64": dict(lanes_per_env=64),
         "warm32": dict(lanes_per_env=32, warm_start=1), "warm64": dict(lanes_per_env=64, warm_start=1), "full": dict(torso="full", n=8),
         # the single-wave kernels the cases above do not reach: lanes 16 at 100 environments is one wave per SIMD without the warm start
         "warm16": dict(lanes_per_env=16, warm_start=1), "soft16w2": dict(lanes_per_env=16, waves_per_simd=2),
         "warm16w2": dict(lanes_per_env=16, waves_per_simd=2, warm_start=1)}


def _env(usim, n=N, torso="soft", seed=3, **kw):
    opts = dict(usim.default_robosuite_kwargs())
    opts.update(kw)
    return usim.UltrasoundVecEnv(n, device="cuda:0", seed=seed, torso=torso, **opts)


def _actions(env, steps, seed, n=None):
    """[steps, n, A] uniform in the action box, the same for the same seed"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.as_tensor(env.action_space.low, dtype=torch.float32)
    hi = torch.as_tensor(env.action_space.high, dtype=torch.float32)
    u = torch.rand((steps, n or env.num_envs, env.action_dim), generator=g)
    return (lo + u * (hi - lo)).to(env.device)


def _arange(env):
    return torch.arange(env.num_envs, dtype=torch.int32, device=env.device)


def _loop(env, acts):
    """the same steps one launch each: a block filled from step_tensor's buffers"""
    blk = env.alloc_block(acts.shape[0], with_actions=False)
    for k, a in enumerate(acts):
        obs, rew, done = env.step_tensor(a)
        blk["obs"][k].copy_(obs); blk["rew"][k].copy_(rew); blk["done"][k].copy_(done)
    return blk


def _same_block(x, y):
    for name in ("obs", "rew", "done"):
        same = (x[name].view(torch.int32) == y[name].view(torch.int32)) if x[name].dtype == torch.float32 else (x[name] == y[name])
        steps = same.reshape(same.shape[0], -1).all(dim=1)
        assert bool(steps.all()), (name, "first step that differs", int((~steps).nonzero()[0]))


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    assert sa.keys() == sb.keys()
    for key in sa:
        assert np.array_equal(np.asarray(sa[key]).view(np.uint8), np.asarray(sb[key]).view(np.uint8)), key


def _start(env, steps=25, seed=11):
    env.reset_tensor()
    for a in _actions(env, steps, seed):
        env.step_tensor(a)


# ---- 1. a block equals the same steps one launch each ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_block_equals_single_step_launches(usim, case):
    kw = CASES[case]
    T, horizon, ends = (12, 5, 2 * 8) if case == "full" else (300, 37, 800)      # (from a fresh reset the 300 steps are cut at the refill period: 256 + 44)
    a, b = _env(usim, horizon=horizon, **kw), _env(usim, horizon=horizon, **kw)
    a.reset_tensor(); b.reset_tensor()
    acts = _actions(a, T, 21)
    blk = a.alloc_block(T)
    blk["act"].fill_(-7.0)
    a.rollout_actions(acts, blk)
    ref = _loop(b, acts)
    _same_block(blk, ref)
    assert int(blk["done"].sum()) >= ends
    assert bool((blk["act"] == -7.0).all())                               # the block's own action entry is not written
    _same_state(a, b)
    a.close(); b.close()


# ---- 2. the launch length does not show ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [32, 64])
def test_steps_per_launch_gives_the_same_block(usim, lanes):
    T = 40
    blocks = []
    for spl in (1, 7, 256):
        env = _env(usim, horizon=37, lanes_per_env=lanes)
        env.set_steps_per_launch(spl)
        env.reset_tensor()
        blk = env.alloc_block(T, with_actions=False)
        env.rollout_actions(_actions(env, T, 22), blk)
        blocks.append((blk, env.get_state()))
        env.close()
    assert int(blocks[0][0]["done"].sum()) >= N                           # every environment passed an episode end
    for blk, st in blocks[1:]:
        _same_block(blocks[0][0], blk)
        for key in st:
            assert np.array_equal(st[key], blocks[0][1][key]), key


# ---- 3. physics substeps: one action per control step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["soft32", "rigid"])
@pytest.mark.parametrize("control_freq", [250, 100])
def test_substeps(usim, case, control_freq):
    T = 12
    a, b = (_env(usim, horizon=5, control_freq=control_freq, **CASES[case]) for _ in range(2))
    a.reset_tensor(); b.reset_tensor()
    acts = _actions(a, T, 23)
    blk = a.alloc_block(T, with_actions=False)
    a.rollout_actions(acts, blk)
    _same_block(blk, _loop(b, acts))
    assert int(blk["done"].sum()) >= 2 * N
    _same_state(a, b)
    a.close(); b.close()


# ---- 4. without a block the handle's own buffers hold the last step -------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [16, 32])
def test_without_a_block(usim, lanes):
    T = 40
    a, b = _env(usim, horizon=37, lanes_per_env=lanes), _env(usim, horizon=37, lanes_per_env=lanes)
    a.reset_tensor(); b.reset_tensor()
    acts = _actions(a, T, 24)
    a.rollout_actions(acts)
    for act in acts:
        b.step_tensor(act)
    for name in ("_obs", "_rew", "_done", "_term", "_contacts", "_ep_ret", "_ep_len", "_status"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert int(a.episode_length.max()) == 37                              # (an episode ended on the way: the statistics were written)
    _same_state(a, b)
    a.close(); b.close()


# ---- 5. non-finite action components count as zero ------------------------------------------------------------------------------------------
def test_non_finite_actions_count_as_zero(usim):
    T = 12
    a, b = _env(usim, horizon=5), _env(usim, horizon=5)
    a.reset_tensor(); b.reset_tensor()
    zeros = _actions(a, T, 25)
    g = torch.Generator().manual_seed(26)
    hit = (torch.rand(zeros.shape, generator=g) < 0.2).to(a.device)
    kind = torch.randint(0, 3, zeros.shape, generator=g).to(a.device)
    bad = torch.where(kind == 0, torch.full_like(zeros, float("nan")), torch.where(kind == 1, torch.full_like(zeros, float("inf")), torch.full_like(zeros, float("-inf"))))
    planted = torch.where(hit, bad, zeros).contiguous()
    zeros = torch.where(hit, torch.zeros_like(zeros), zeros).contiguous()
    assert int(hit.sum()) > T * N and not bool(torch.isfinite(planted).all())
    ba, bb = a.alloc_block(T, with_actions=False), b.alloc_block(T, with_actions=False)
    a.rollout_actions(planted, ba); b.rollout_actions(zeros, bb)
    _same_block(ba, bb)
    assert bool(torch.isfinite(ba["obs"]).all()) and bool(torch.isfinite(ba["rew"]).all())
    _same_state(a, b)
    a.close(); b.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone(usim):
    env = _env(usim)
    _start(env, 5)
    before = env.get_state()
    good = _actions(env, 4, 27)
    A = env.action_dim
    bad = {"shape n": good[:, : N - 1].contiguous(), "shape A": good[:, :, : A - 1].contiguous(), "two dimensions": good[0], "dtype": good.double(),
           "device": good.cpu(), "not contiguous": good.transpose(0, 1).contiguous().transpose(0, 1), "not a tensor": good.cpu().numpy()}
    assert not bad["not contiguous"].is_contiguous() and bad["not contiguous"].shape == good.shape
    for name, x in bad.items():
        with pytest.raises(ValueError):
            env.rollout_actions(x)
        with pytest.raises(ValueError):
            env.rollout_actions(x, env.alloc_block(4))
    with pytest.raises(ValueError):
        env.rollout_actions(good, env.alloc_block(3))                     # a block shorter than the actions
    with pytest.raises(ValueError):
        env.score_block(torch.zeros((4, N), device=env.device), torch.zeros((4, N), dtype=torch.bool, device=env.device))
    with pytest.raises(ValueError):
        env.score_block(torch.zeros((4, N), device=env.device), torch.zeros((3, N), dtype=torch.uint8, device=env.device))
    lib, io = env.lib, env._io
    keep, io.act_dev = io.act_dev, None
    assert lib.usim_rollout_actions(env._handle, 4, io, 0, env._stream()) == -1          # USIM_ERR_INVALID: no action block
    io.act_dev = keep
    assert lib.usim_rollout_actions(env._handle, -1, io, 0, env._stream()) == -1
    assert lib.usim_rollout_actions(env._handle, 4, None, 0, env._stream()) == -1
    assert lib.usim_rollout_actions(env._handle, 0, io, 0, env._stream()) == 0           # nothing to do
    after = env.get_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    env.close()


# ---- 7. the shooting planner of INTEGRATION.md section 4c ------------------------------------------------------------------------------------
def test_planner_scores_equal_the_alive_loop(usim):
    H = 16
    env, twin = _env(usim, horizon=37, early_termination=False), _env(usim, horizon=37, early_termination=False)
    _start(env); _start(twin)                                             # 25 steps: every episode ends at its horizon, step 12 of the 16 planned ones
    home = env.save_envs().clone()
    src = torch.full((N,), 7, dtype=torch.int64, device=env.device)
    cands = _actions(env, N, 28, n=H)                                     # [candidate, step, A]
    plan = cands.transpose(0, 1).contiguous()                             # [step, candidate, A]
    env.fork(src)
    blk = env.alloc_block(H, with_actions=False)
    env.rollout_actions(plan, blk)
    ret, length = env.score_block(blk, gamma=1.0)
    ret2, length2 = env.score_block(blk["rew"], blk["done"], gamma=1.0)
    assert torch.equal(ret, ret2) and torch.equal(length, length2)
    env.load_envs(home, _arange(env))
    env.fork(src)
    loop_ret = torch.zeros(N, dtype=torch.float32, device=env.device)
    loop_len = torch.zeros(N, dtype=torch.int32, device=env.device)
    alive = torch.ones(N, dtype=torch.bool, device=env.device)
    for t in range(H):
        obs, rew, done = env.step_tensor(cands[:, t].contiguous())
        loop_ret += rew * alive
        loop_len += alive.to(torch.int32)
        alive &= ~done.bool()
    assert torch.equal(length, loop_len)
    assert torch.equal(ret.view(torch.int32), loop_ret.view(torch.int32))
    assert int(length.min()) < H and not bool(alive.any())                # every candidate's episode ended inside the plan
    assert len(torch.unique(ret)) > N // 2                                # the candidates differ
    # home again: every environment's next step is the one it would have taken without the planning
    env.load_envs(home, _arange(env))
    act = _actions(env, 1, 29)[0]
    env.step_tensor(act); twin.step_tensor(act)
    for name in ("_rew", "_done", "_contacts"):
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    fin_e = torch.where(env._done.bool()[:, None], env.terminal_obs, env._obs)
    fin_t = torch.where(twin._done.bool()[:, None], twin.terminal_obs, twin._obs)
    assert torch.equal(fin_e, fin_t)
    env.close(); twin.close()


# ---- 8. capture ------------------------------------------------------------------------------------------------------------------------------
def test_plan_and_score_replay_from_a_graph(usim):
    H = 16
    env = _env(usim, horizon=37, early_termination=False)                # (25 steps in: the episodes end inside the plan)
    _start(env)
    home, rows = env.save_envs().clone(), _arange(env)
    plan = _actions(env, H, 30)
    blk = env.alloc_block(H, with_actions=False)
    out = (torch.zeros(N, dtype=torch.float32, device=env.device), torch.zeros(N, dtype=torch.int32, device=env.device))

    def sequence():                                                       # (the order of policy.GraphedCollector: a recorded sequence starts and ends with a refill)
        env.refill_bank()
        env.rollout_actions(plan, blk)
        env.score_block(blk, gamma=0.99, out=out)
        env.refill_bank()

    sequence()
    eager = [t.clone() for t in out]
    assert int(eager[1].min()) < H
    dev = env.device
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        env.load_envs(home, rows)
        sequence()                                                        # (a first eager pass on the side stream)
        torch.cuda.current_stream(dev).synchronize()
        with torch.cuda.graph(graph, stream=side):
            sequence()
    torch.cuda.current_stream(dev).wait_stream(side)
    replays = []
    for _ in range(2):
        env.load_envs(home, rows)
        for t in out:
            t.zero_()
        graph.replay()
        replays.append([t.clone() for t in out])
    torch.cuda.synchronize()
    for got in replays:
        assert torch.equal(got[0].view(torch.int32), eager[0].view(torch.int32)) and torch.equal(got[1], eager[1])
    env.close()
