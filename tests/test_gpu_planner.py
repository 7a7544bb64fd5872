"""planner.MPPIPlanner end to end: two controlled soft-torso environments (`real`), 2 x 8 = 16 simulated ones (`sim`), a plan of 4 steps.  What plan() must equal is
stated with the library's own pieces -- load_envs + rollout_actions + score_block on a third handle -- and tests/plan_ref.py; where the contract says so, bit for
bit.  The `short` set-up has episodes of 6 steps and `real` stepped 3 times first, so every candidate's episode ends inside the plan."""
import numpy as np
import pytest
import torch

import plan_ref as R

pytestmark = pytest.mark.gpu
G, K, H = 2, 8, 4
N = G * K


def _env(usim, n, seed=3, **kw):
    opts = dict(usim.default_robosuite_kwargs())
    opts.update(kw)
    return usim.UltrasoundVecEnv(n, device="cuda:0", seed=seed, torso="soft", **opts)


def _i32(t):
    return t.contiguous().view(torch.int32)


def _setup(usim, short, temperature, sim_seed=5, **kw):
    """(real, sim, planner); real is reset and, in the short set-up, 3 steps into its 6-step episodes"""
    env_kw = dict(horizon=6) if short else {}
    real, sim = _env(usim, G, **env_kw), _env(usim, N, seed=sim_seed, **env_kw)
    real.reset_tensor(); sim.reset_tensor()
    if short:
        g = torch.Generator().manual_seed(1)
        for _ in range(3):
            real.step_tensor((torch.rand((G, real.action_dim), generator=g) * 0.3).to(real.device))
        assert not bool(real._done.any())
    pl = usim.planner.MPPIPlanner(real, sim, horizon=H, sigma=0.3, temperature=temperature, seed=17, **kw)
    return real, sim, pl


def _rows(env):
    return torch.arange(env.num_envs, dtype=torch.int32, device=env.device)


# ---- 1. plan() reads real and leaves it as it is ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [False, True])
def test_plan_leaves_real_bit_for_bit(usim, short):
    real, sim, pl = _setup(usim, short, temperature=0.5)
    before, obs = real.save_envs().clone(), real._obs.clone()
    others = [t.clone() for t in (real._rew, real._done, real._ep_ret, real._ep_len)]
    act = pl.plan()
    assert tuple(act.shape) == (G, real.action_dim) and act.device == real.device
    assert torch.equal(_i32(real.save_envs()), _i32(before))
    assert torch.equal(_i32(real._obs), _i32(obs))
    for t, was in zip((real._rew, real._done, real._ep_ret, real._ep_len), others):
        assert torch.equal(t, was)
    real.close(); sim.close()


# ---- 2. what plan() equals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short, temperature, gamma, smoothing", [(False, 0.5, 1.0, 0.0), (True, 0.05, 0.99, 0.7), (True, 0.0, 1.0, 0.0)])
def test_plan_equals_its_parts(usim, short, temperature, gamma, smoothing):
    real, sim, pl = _setup(usim, short, temperature, gamma=gamma, smoothing=smoothing)
    third = _env(usim, N, seed=9, **(dict(horizon=6) if short else {}))   # another seed: a loaded row carries everything the plan depends on
    third.reset_tensor()
    low, high = real.action_space.low, real.action_space.high
    mean0 = pl.mean.cpu().numpy()
    pl.plan()
    cand = pl.candidates.clone()
    # the candidates are the reference's sample around the nominal the planner held, at noise counter 0
    ref_s = R.sample(mean0, pl.sigma.cpu().numpy(), low, high, None, K, smoothing, seed=17, counter=0)
    err = np.abs(cand.cpu().numpy().astype(np.float64) - ref_s["cand"])
    print("candidates: worst error / bound", float(np.max(np.where(err == 0, 0, err / np.maximum(ref_s["bound"], 1e-300)))))
    assert np.all(err <= ref_s["bound"])
    assert int(pl.noise_counter.item()) == 1
    # returns and lengths: the same rows played on a third handle
    third.load_envs(real.save_envs(), _rows(third) // K)
    blk = third.alloc_block(H, with_actions=False)
    third.rollout_actions(cand, blk)
    ret, length = third.score_block(blk, gamma=gamma)
    assert torch.equal(_i32(pl.returns), _i32(ret)) and torch.equal(pl.lengths, length)
    assert (int(length.min()) < H) == short                               # short: the candidates' episodes end inside the plan
    assert len(torch.unique(ret)) > N // 2
    # best, weights, plan, action, next nominal: the reference's update on these candidates and returns
    ref = R.update(cand.cpu().numpy(), ret.cpu().numpy(), low, high, K, temperature)
    assert np.array_equal(pl.best.cpu().numpy(), ref["best"])
    w, plan = pl.weights.cpu().numpy().astype(np.float64), pl.plan_actions.cpu().numpy().astype(np.float64)
    ew, ep = np.abs(w - ref["weights"]), np.abs(plan - ref["plan"])
    for name, e, b in (("weights", ew, ref["b_weights"]), ("plan", ep, ref["b_plan"])):
        print(name, "worst error / bound", float(np.max(np.where(e == 0, 0, e / np.maximum(b, 1e-300)))))
        assert np.all(e <= b), name
    assert torch.equal(_i32(pl.action), _i32(pl.plan_actions[:, 0]))
    shifted = torch.cat([pl.plan_actions[:, 1:], pl.plan_actions[:, -1:]], dim=1)
    assert torch.equal(_i32(pl.mean), _i32(shifted))
    for e in (real, sim, third):
        e.close()


# ---- 3. at temperature 0 the plan is realised exactly ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [False, True])
def test_selected_plan_is_realised_on_real(usim, short):
    real, sim, pl = _setup(usim, short, temperature=0.0)
    pl.plan()
    best = pl.best.long()
    chosen = torch.arange(G, device=real.device) * K + best
    for g in range(G):
        assert torch.equal(_i32(pl.plan_actions[g]), _i32(pl.candidates[:, int(chosen[g])]))
    # played open loop on real -- a handle of 2 environments, the candidates ran on one of 16 -- the chosen sequence earns the return it was chosen for
    acts = pl.plan_actions.transpose(0, 1).contiguous()
    blk = real.alloc_block(H, with_actions=False)
    real.rollout_actions(acts, blk)
    ret, length = real.score_block(blk, gamma=1.0)
    assert torch.equal(_i32(ret), _i32(pl.returns[chosen])) and torch.equal(length, pl.lengths[chosen])
    assert bool((pl.returns[chosen] >= pl.returns[torch.arange(G, device=real.device) * K]).all())      # no worse than the nominal, candidate 0
    assert (int(length.min()) < H) == short
    real.close(); sim.close()


# ---- 4. an episode end restarts that group's nominal, and only that one ------------------------------------------------------------------------
def test_restart_after_an_episode_end(usim):
    real, sim = _env(usim, G, horizon=6, early_termination=False), _env(usim, N, seed=5, horizon=6, early_termination=False)
    real.reset_tensor(); sim.reset_tensor()
    zero = torch.zeros((G, real.action_dim), device=real.device)
    real.step_tensor(zero); real.step_tensor(zero)
    real.reset_tensor(mask=[0, 1])                                        # environment 0 is 2 steps into its episode, environment 1 starts one
    pl = usim.planner.MPPIPlanner(real, sim, horizon=H, sigma=0.3, temperature=0.5, seed=17)
    for k in range(4):
        obs, rew, done = pl.step()
        assert done.tolist() == ([1, 0] if k == 3 else [0, 0]), k        # the 6th step of environment 0
        assert pl.restart.tolist() == done.tolist()
    assert bool((pl.mean[1] != 0).any())
    nominal = pl.mean.cpu().numpy()                                       # what the last update left: both groups' shifted plans
    counter = int(pl.noise_counter.item())
    pl.plan()
    cand = pl.candidates.cpu().numpy()
    low, high = real.action_space.low, real.action_space.high
    assert not cand[:, 0, :].any()                                        # group 0 is sampled around zero ...
    assert np.array_equal(cand[:, K, :].view(np.uint32), np.clip(nominal[1], low, high).astype(np.float32).view(np.uint32))     # ... group 1 around its shifted nominal
    ref = R.sample(nominal, pl.sigma.cpu().numpy(), low, high, [1, 0], K, 0.0, seed=17, counter=counter)
    assert np.all(np.abs(cand.astype(np.float64) - ref["cand"]) <= ref["bound"])
    real.close(); sim.close()


# ---- 5. a recorded step replays the eager one ----------------------------------------------------------------------------------------------
def test_record_and_replay_equal_eager_steps(usim):
    real, sim, pl = _setup(usim, short=False, temperature=0.5, smoothing=0.7)
    pl.step()                                                             # (a nominal that is not zero)
    rows = _rows(real)
    start = dict(state=real.save_envs().clone(), mean=pl.mean.clone(), restart=pl.restart.clone(), counter=pl.noise_counter.clone())

    def three(step):
        real.load_envs(start["state"], rows)
        pl.mean.copy_(start["mean"]); pl.restart.copy_(start["restart"]); pl.noise_counter.copy_(start["counter"])
        seen = []
        for _ in range(3):
            obs, rew, done = step()
            seen.append([t.clone() for t in (pl.action, pl.returns, pl.best, pl.mean, obs, rew, done, real.save_envs())])
        return seen

    eager = three(pl.step)
    assert not any(bool(s[6].any()) for s in eager)                       # (no episode of real ends: load_envs brings everything back but the episode counter)
    pl.record()
    replayed = three(pl.replay)
    torch.cuda.synchronize()
    assert int(pl.noise_counter.item()) == int(start["counter"].item()) + 3
    for k, (a, b) in enumerate(zip(eager, replayed)):
        for x, y in zip(a, b):
            assert torch.equal(_i32(x) if x.dtype == torch.float32 else x, _i32(y) if y.dtype == torch.float32 else y), k
    assert not torch.equal(eager[0][0], eager[1][0])                      # the steps differ from one another
    real.close(); sim.close()
