"""usim_save_envs / usim_load_envs (include/usim.h "snapshots") and their host side UltrasoundVecEnv.save_envs / load_envs / fork: a loaded environment computes the
same bits as the one that was saved, under its own episode counter; indices and row numbers out of range are skipped; a save does not modify the handle; both calls
can be recorded in a graph.  100 environments: a ragged last workgroup in every mapping, and a padded block (128) larger than n.  Actions are explicit tensors -- the
synthetic ones of rollout_random are keyed by environment."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 100
SENTINEL = 12345.0


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


def _outputs(env):
    return [t.clone() for t in (env._obs, env._rew, env._done, env.contacts)]


def _start(env, steps=20, seed=11):
    env.reset_tensor()
    for a in _actions(env, steps, seed):
        env.step_tensor(a)


# ---- 1. rewind --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rigid", "soft16", "soft32", "soft64", "warm32", "warm64", "full"])
def test_rewind_repeats_the_same_bits(usim, case):
    kw = {"rigid": dict(torso="rigid"), "soft16": dict(lanes_per_env=16), "soft32": dict(lanes_per_env=32), "soft64": dict(lanes_per_env=64),
          "warm32": dict(lanes_per_env=32, warm_start=1), "warm64": dict(lanes_per_env=64, warm_start=1), "full": dict(torso="full", n=8)}[case]
    before, after = (5, 5) if case == "full" else (20, 25)
    env = _env(usim, early_termination=False, **kw)
    assert env.snapshot_words == usim._lib.snapshot_words(kw.get("torso", "soft"), kw.get("warm_start", 0))
    _start(env, before)
    snap = env.save_envs()
    assert snap.shape == (env.num_envs, env.snapshot_words) and snap.dtype == torch.float32 and snap.is_cuda
    acts = _actions(env, after, 12)
    first = []
    for a in acts:
        env.step_tensor(a)
        first.append(_outputs(env))
    assert not any(bool(o[2].any()) for o in first)                       # no episode ends in these steps: horizon 1000, no early termination
    assert not torch.equal(first[0][0], first[-1][0])
    env.load_envs(snap, _arange(env))
    for k, a in enumerate(acts):
        env.step_tensor(a)
        for name, x, y in zip(("obs", "rew", "done", "contacts"), first[k], _outputs(env)):
            assert torch.equal(x, y), (k, name)
    env.close()


# ---- 2. fork across indices, 3. the counter rule -----------------------------------------------------------------------------------
def _fork_from_7(usim, **kw):
    """default configuration (early termination on): 20 steps, every environment forked from environment 7, then env 7's action row for all until env 7's episode ends.
    Returns the env, the states before / after the fork and the per-step outputs up to and including the step of the first done."""
    env = _env(usim, **kw)
    _start(env)
    st0 = env.get_state()
    obs_before = env._obs.clone()
    obs = env.fork(torch.full((N,), 7, dtype=torch.int64, device=env.device))
    assert obs is env._obs and torch.equal(obs, obs_before[7].expand(N, -1))
    st1 = env.get_state()
    rows = _actions(env, env.horizon, 13, n=1)
    steps = []
    for k in range(env.horizon):                                         # (the episode ends at its horizon at the latest)
        env.step_tensor(rows[k].expand(N, -1).contiguous())
        steps.append(_outputs(env) + [env.terminal_obs.clone()])
        if bool(env._done.any()):
            break
    return env, st0, st1, steps


@pytest.mark.parametrize("lanes", [32, 64])
def test_forked_environments_follow_their_source(usim, lanes):
    env, _, _, steps = _fork_from_7(usim, lanes_per_env=lanes)
    last = len(steps) - 1
    for k, (obs, rew, done, contacts, term) in enumerate(steps):
        assert torch.equal(rew, rew[7].expand(N)), k
        assert torch.equal(done, done[7].expand(N)), k
        assert torch.equal(contacts, contacts[7].expand(N, -1)), k
        if k < last:
            assert torch.equal(obs, obs[7].expand(N, -1)), k
    obs, rew, done, contacts, term = steps[last]
    assert bool(done[7])                                                  # the step where env 7's episode ended (and with it everybody's)
    assert torch.equal(term, term[7].expand(N, -1))
    assert not torch.equal(obs, obs[7].expand(N, -1))                     # every environment went on with an episode of its own: its own reset observation
    env.close()


def test_a_load_keeps_the_episode_counter(usim):
    env, st0, st1, steps = _fork_from_7(usim)
    others = np.arange(N) != 7
    for key in st1:
        if key == "episode":
            assert np.array_equal(st1[key], st0[key])                     # nobody's counter moved
        else:
            assert np.array_equal(st1[key][7], st0[key][7]), key          # the source is untouched
            assert np.array_equal(st1[key][others], np.broadcast_to(st1[key][7], st1[key].shape)[others]), key
    assert bool(steps[-1][2].all())                                       # the first done of every environment is this step
    st2 = env.get_state()
    assert np.array_equal(st2["episode"], st0["episode"] + 1)             # ... and each went on with ITS next episode
    # the bank rings and the outstanding refill orders are intact: 300 more auto-reset steps (a refill launch among them) without a fault
    finite = torch.ones((), dtype=torch.bool, device=env.device)
    fault = torch.zeros((), dtype=torch.int32, device=env.device)
    ended = torch.zeros((), dtype=torch.int64, device=env.device)
    for a in _actions(env, 300, 14):
        obs, rew, done = env.step_tensor(a)
        finite &= torch.isfinite(obs).all() & torch.isfinite(rew).all()
        fault |= (env.status & 4).max()
        ended += done.sum()
    assert bool(finite) and int(fault) == 0
    assert int(ended) > 0
    env.close()


# ---- 4. selective load ---------------------------------------------------------------------------------------------------------------
def test_selective_load(usim):
    a, b = _env(usim), _env(usim)                                         # twins: b is never loaded
    _start(a); _start(b)
    m = 10
    src = torch.arange(40, 40 + m, dtype=torch.int32, device=a.device)    # row r holds environment 40 + r
    snap = a.save_envs(src)
    i = torch.arange(N, device=a.device)
    rows = torch.where(i % 2 == 1, i % m, torch.full_like(i, -1)).to(torch.int32)
    a.load_envs(snap, rows)
    sa, sb = a.get_state(), b.get_state()
    even, odd = np.arange(N) % 2 == 0, np.arange(N) % 2 == 1
    source = 40 + np.arange(N) % m
    for key in sa:
        assert np.array_equal(sa[key][even], sb[key][even]), key
        if key == "episode":
            assert np.array_equal(sa[key], sb[key])
        else:
            assert np.array_equal(sa[key][odd], sb[key][source][odd]), key
    act_b = _actions(b, 1, 15)[0]
    act_a = act_b.clone()
    src_t = torch.as_tensor(source, device=a.device)
    odd_t = torch.as_tensor(odd, device=a.device)
    act_a[odd_t] = act_b[src_t][odd_t]
    a.step_tensor(act_a); b.step_tensor(act_b)
    ev = ~odd_t
    for x, y in zip(_outputs(a), _outputs(b)):
        assert torch.equal(x[ev], y[ev])
    assert torch.equal(a._rew[odd_t], b._rew[src_t][odd_t]) and torch.equal(a._done[odd_t], b._done[src_t][odd_t])
    assert torch.equal(a.contacts[odd_t], b.contacts[src_t][odd_t])
    # the observation a step returns where an episode ended is the reset observation of the environment's own next episode: compare the terminal one there
    fin_a = torch.where(a._done.bool()[:, None], a.terminal_obs, a._obs)
    fin_b = torch.where(b._done.bool()[:, None], b.terminal_obs, b._obs)
    assert torch.equal(fin_a[odd_t], fin_b[src_t][odd_t])
    a.close(); b.close()


# ---- 5. guards (a missing one would still stay inside an allocation: index n lies in the padded block, row m in the buffer) ---------------
def test_out_of_range_indices_and_rows_are_skipped(usim):
    env = _env(usim)
    _start(env)
    w = env.snapshot_words
    whole = env.save_envs()
    m = 4
    buf = torch.full((m + 4, w), SENTINEL, dtype=torch.float32, device=env.device)
    out = env.save_envs(torch.tensor([3, N, 5, N], dtype=torch.int32, device=env.device), out=buf)
    assert out.data_ptr() == buf.data_ptr() and tuple(out.shape) == (m, w)
    assert torch.equal(buf[0], whole[3]) and torch.equal(buf[2], whole[5])
    for r in (1, 3, 4, 5, 6, 7):
        assert bool((buf[r] == SENTINEL).all()), r
    buf.fill_(SENTINEL)
    env.load_envs(buf[:m], torch.full((N,), m, dtype=torch.int32, device=env.device))      # row m exists in the allocation and holds the sentinel
    assert torch.equal(env.save_envs(), whole)
    env.close()


# ---- 6. rows of one handle loaded into another ----------------------------------------------------------------------------------------
def test_rows_load_into_another_handle(usim):
    small, big = _env(usim, n=8, early_termination=False), _env(usim, early_termination=False)
    assert small.snapshot_words == big.snapshot_words
    _start(small)
    big.reset_tensor()
    snap = small.save_envs()
    big.load_envs(snap, torch.zeros(N, dtype=torch.int32, device=big.device))
    rows = _actions(small, 20, 16, n=1)
    for k in range(20):
        small.step_tensor(rows[k].expand(8, -1).contiguous())
        big.step_tensor(rows[k].expand(N, -1).contiguous())
        for x, y in zip(_outputs(small), _outputs(big)):
            assert torch.equal(x[0].expand_as(y), y), k
        assert not bool(small._done.any())
    small.close(); big.close()


# ---- 7. a save does not modify the handle ----------------------------------------------------------------------------------------------
def test_save_does_not_modify_the_handle(usim):
    a, b = _env(usim), _env(usim)
    a.reset_tensor(); b.reset_tensor()
    buf = None
    for k, act in enumerate(_actions(a, 30, 17)):
        buf = a.save_envs(out=buf)
        a.step_tensor(act); b.step_tensor(act)
        for x, y in zip(_outputs(a) + [a.terminal_obs], _outputs(b) + [b.terminal_obs]):
            assert torch.equal(x, y), k
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    a.close(); b.close()


# ---- 8. capture --------------------------------------------------------------------------------------------------------------------------
def test_load_and_step_replay_from_a_graph(usim):
    env = _env(usim, early_termination=False)
    _start(env)
    snap, rows = env.save_envs(), _arange(env)
    act = _actions(env, 1, 18)[0]
    other = _actions(env, 6, 19)
    env.load_envs(snap, rows)
    env.step_tensor(act)
    eager = _outputs(env)
    for a in other[:3]:
        env.step_tensor(a)
    dev = env.device
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        env.load_envs(snap, rows)                                         # (a first eager pass on the side stream, as policy.GraphedCollector does)
        env.step_tensor(act)
        torch.cuda.current_stream(dev).synchronize()
        with torch.cuda.graph(graph, stream=side):                        # one linear sequence: load, step
            env.load_envs(snap, rows)
            env.step_tensor(act)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph.replay()
    first = _outputs(env)
    for a in other[3:]:
        env.step_tensor(a)
    assert not torch.equal(env._obs, first[0])
    graph.replay()
    second = _outputs(env)
    torch.cuda.synchronize()
    for name, e, x, y in zip(("obs", "rew", "done", "contacts"), eager, first, second):
        assert torch.equal(e, x) and torch.equal(e, y), name
    env.close()


# ---- 9. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors(usim):
    env = _env(usim)
    env.reset_tensor()
    lib, h, s = env.lib, env._handle, env._stream()
    INVALID = -1                                                          # USIM_ERR_INVALID
    w = env.snapshot_words
    buf = torch.full((N + 1, w), SENTINEL, dtype=torch.float32, device=env.device)
    rows = _arange(env)
    p = buf.data_ptr()
    assert p % 16 == 0
    assert lib.usim_snapshot_words(None) == INVALID
    assert lib.usim_save_envs(None, None, N, p, s) == INVALID
    assert lib.usim_save_envs(h, None, N, None, s) == INVALID
    assert lib.usim_save_envs(h, None, 0, p, s) == INVALID
    assert lib.usim_save_envs(h, None, -3, p, s) == INVALID
    assert lib.usim_save_envs(h, None, N, p + 4, s) == INVALID            # off the 16-byte grid
    assert lib.usim_save_envs(h, None, N + 1, p, s) == INVALID            # no index list: environments 0 .. m - 1 must exist
    assert lib.usim_load_envs(None, p, N, rows.data_ptr(), s) == INVALID
    assert lib.usim_load_envs(h, None, N, rows.data_ptr(), s) == INVALID
    assert lib.usim_load_envs(h, p, N, None, s) == INVALID
    assert lib.usim_load_envs(h, p, 0, rows.data_ptr(), s) == INVALID
    assert lib.usim_load_envs(h, p + 4, N, rows.data_ptr(), s) == INVALID
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())                                  # nothing was enqueued
    assert lib.usim_save_envs(h, None, N, p, s) == 0
    assert torch.equal(buf[:N], env.save_envs())
    assert bool((buf[N] == SENTINEL).all())
    with pytest.raises(ValueError):
        env.load_envs(buf[:, : w - 4].contiguous(), rows)                 # rows of another size
    with pytest.raises(ValueError):
        env.load_envs(buf[:N], rows[:-1])
    env.close()
