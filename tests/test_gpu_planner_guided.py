"""planner.MPPIPlanner with its guiding options end to end: 4 controlled soft-torso environments (`real`), 4 x 16 = 64 simulated ones (`sim`), a plan of 4 steps,
the critic built from the golden `tracking` weights and statistics.  Episodes last 6 steps, end at that limit alone (no early termination), and the four real
environments stand 3, 1, 2 and 1 steps into theirs, so the candidates of group 0 end inside the plan, those of group 2 end ON its last step and those of groups 1
and 3 play all four steps: every case of the bootstrap and of the tail action occurs.  What a plan must equal is stated with the planner's public pieces, tests/cem_ref.py and
tests/policy_ref.py; bit for bit wherever the contract says so."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import cem_ref as Q
import policy_ref as P
from test_gpu_policy_kernels import UNITS                                # the rounding units of the policy kernels, derived there

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
G, K, H = 4, 16, 4
N = G * K
GAMMA = 0.99
U24 = 2.0**-24
ALL = dict(tail_action=True, iterations=3, elites=4, momentum=0.2, sigma_min=0.02, smoothing=0.5)


def _i32(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _env(usim, n, seed, **kw):
    opts = dict(usim.default_robosuite_kwargs())
    opts.update(kw)
    return usim.UltrasoundVecEnv(n, device=DEV, seed=seed, torso="soft", **opts)


def _critic(usim, pins, norm_reward=True, constant=None):
    """(policy, vecnorm) of the golden tracking checkpoint; constant: the value head replaced by weights 0 and this bias"""
    meta = json.loads((ROOT / "tests/golden/reference_pins.json").read_text())["tracking"]
    sd = {k: torch.from_numpy(v) for k, v in np.load(ROOT / "tests/golden/tracking_policy.npz").items()}
    stats = {"obs_mean": pins["tracking_obs_rms_mean"], "obs_var": pins["tracking_obs_rms_var"], "count": meta["obs_rms_count"], "ret_mean": meta["ret_rms_mean"],
             "ret_var": meta["ret_rms_var"], "clip_obs": meta["clip_obs"], "clip_reward": meta["clip_reward"], "gamma": meta["gamma"], "epsilon": meta["epsilon"]}
    assert meta["gamma"] == GAMMA
    policy = usim.policy.MlpActorCritic.from_sb3_state_dict(sd).to(DEV)
    if constant is not None:
        with torch.no_grad():
            policy.value_net.weight.zero_(); policy.value_net.bias.fill_(constant)
    return policy, usim.policy.DeviceVecNormalize.from_stats(stats, N, device=DEV, training=False, norm_reward=norm_reward)


def _setup(usim, short=True, **kw):
    """(real, sim, planner); short: 6-step episodes, real 3 / 1 / 2 / 1 steps into them"""
    env_kw = dict(horizon=6, early_termination=False) if short else {}
    real, sim = _env(usim, G, 3, **env_kw), _env(usim, N, 5, **env_kw)
    real.reset_tensor(); sim.reset_tensor()
    if short:
        g = torch.Generator().manual_seed(1)
        act = lambda: (torch.rand((G, real.action_dim), generator=g) * 0.3).to(DEV)
        real.step_tensor(act()); real.reset_tensor(mask=[0, 0, 1, 0])
        real.step_tensor(act()); real.reset_tensor(mask=[0, 1, 0, 1])
        real.step_tensor(act())
        assert not bool(real._done.any())
    args = dict(horizon=H, sigma=0.3, temperature=0.5, gamma=GAMMA, seed=17)
    args.update(kw)
    return real, sim, usim.planner.MPPIPlanner(real, sim, **args)


def _base(pl):
    """usim_score_block of the block the planner's last round played, and who survived it"""
    base, length = pl.sim.score_block(pl.block, gamma=GAMMA)
    last = pl.block["done"][H - 1]
    return base.cpu().numpy(), length.cpu().numpy(), last.cpu().numpy(), ((length == H) & (last == 0)).cpu().numpy()


def _disc():
    d = np.float32(1)
    for _ in range(H):
        d = np.float32(d * np.float32(GAMMA))
    return d


# ---- 1. a constant critic: the bootstrap is one stated fmaf on top of usim_score_block ------------------------------------------------------
@pytest.mark.parametrize("norm_reward", [True, False])
def test_constant_critic_adds_exactly_its_discounted_value_to_survivors(usim, pins, norm_reward):
    c = 2.5
    policy, vn = _critic(usim, pins, norm_reward, constant=c)
    real, sim, pl = _setup(usim, critic=(policy, vn))
    pl.plan()
    base, length, last, alive = _base(pl)
    assert alive[K:2 * K].all() and alive[3 * K:].all() and not alive[:K].any() and not alive[2 * K:3 * K].any()
    assert (length[:K] == 3).all() and (length[2 * K:3 * K] == H).all() and (last[2 * K:3 * K] != 0).all()       # ended inside the plan; ended on its last step
    assert bool((pl.tail_value == c).all())
    s = Q.tail_scale(float(vn.ret_var), vn.epsilon) if norm_reward else np.float32(1)
    assert (s > 200) == norm_reward                                       # sqrt(66170): the critic's unit is hundreds of reward
    want = np.where(alive, Q.fmaf32(_disc(), np.float32(s * np.float32(c)), base), base)
    got = pl.returns.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(pl.lengths.cpu().numpy(), length)
    real.close(); sim.close()


def test_zero_critic_is_the_plain_planner_bit_for_bit(usim, pins):
    policy, vn = _critic(usim, pins, True, constant=0.0)
    real_a, sim_a, a = _setup(usim, critic=(policy, vn))
    real_b, sim_b, b = _setup(usim)
    for _ in range(2):
        for pl in (a, b):
            pl.step()
    for name in ("candidates", "returns", "lengths", "weights", "best", "plan_actions", "action", "mean", "noise_counter"):
        assert torch.equal(_i32(getattr(a, name)), _i32(getattr(b, name))), name
    assert torch.equal(_i32(real_a.save_envs()), _i32(real_b.save_envs()))
    for e in (real_a, sim_a, real_b, sim_b):
        e.close()


# ---- 2. a plan with every option -----------------------------------------------------------------------------------------------------------
NAMES = ("candidates", "returns", "lengths", "weights", "best", "plan_actions", "action", "mean", "sigma_elem", "elite", "tail_value", "tail_policy_action",
         "noise_counter")


@pytest.fixture(scope="module")
def guided(usim, pins):
    """one plan() with every option from the stated start, and what it left (clones)"""
    policy, vn = _critic(usim, pins, True)
    real, sim, pl = _setup(usim, critic=(policy, vn), **ALL)
    before = [t.clone() for t in (real.save_envs(), real._obs, real._rew, real._done, real._ep_ret, real._ep_len)]
    pl.restart.copy_(torch.tensor([0, 1, 0, 0], dtype=torch.uint8))       # group 1 starts from a fresh nominal
    pl.mean.uniform_(-0.2, 0.2, generator=torch.Generator(device=DEV).manual_seed(2))
    mean0 = pl.mean.clone()
    act = pl.plan()
    after = [t.clone() for t in (real.save_envs(), real._obs, real._rew, real._done, real._ep_ret, real._ep_len)]
    out = {k: getattr(pl, k).clone() for k in NAMES}
    out.update(act=act, before=before, after=after, mean0=mean0, block={k: v.clone() for k, v in pl.block.items()}, pl=pl, policy=policy, vn=vn, real=real, sim=sim)
    yield out
    real.close(); sim.close()


def test_plan_leaves_real_untouched_and_advances_the_counter_once_per_round(guided):
    for was, now in zip(guided["before"], guided["after"]):
        assert torch.equal(_i32(was), _i32(now))
    assert int(guided["noise_counter"].item()) == ALL["iterations"]
    assert guided["act"] is guided["pl"].action and tuple(guided["action"].shape) == (G, guided["real"].action_dim)


def test_plan_equals_the_sequence_of_its_public_calls(usim, pins, guided):
    policy, vn = _critic(usim, pins, True)
    real, sim, pl = _setup(usim, critic=(policy, vn), **ALL)
    pl.restart.copy_(torch.tensor([0, 1, 0, 0], dtype=torch.uint8))
    pl.mean.copy_(guided["mean0"])
    rows = torch.arange(N, dtype=torch.int32, device=DEV) // K
    snap = real.save_envs()
    pl.sigma_elem.copy_(pl.sigma.expand(G, H, real.action_dim))
    R_ = ALL["iterations"]
    for r in range(R_):
        sim.load_envs(snap, rows)
        pl.sample_elem(restart=r == 0)
        sim.rollout_actions(pl.candidates, pl.block)
        pl.evaluate_tail(pack=r == 0)
        pl.score()
        if r < R_ - 1:
            pl.refit()
        else:
            pl.update()
            pl.tail()
        pl.noise_counter.add_(1)
    for name in NAMES:
        assert torch.equal(_i32(getattr(pl, name)), _i32(guided[name])), name
    for k, v in guided["block"].items():
        assert torch.equal(_i32(pl.block[k]), _i32(v)), k
    real.close(); sim.close()


def test_the_refits_moved_the_distribution(guided):
    mean0, sigma = guided["mean0"], guided["sigma_elem"]
    assert bool((guided["elite"] >= 0).all()) and bool((guided["elite"][:, 1:] > guided["elite"][:, :-1]).all())       # four finite elites per group, ascending
    assert bool((sigma >= np.float32(ALL["sigma_min"])).all()) and bool((sigma != np.float32(0.3)).all())
    assert float(sigma.mean()) < 0.3                                      # elites lie closer together than the candidates they were chosen from
    assert not torch.equal(guided["candidates"][:, K], mean0[1])          # group 1 was restarted: its nominal (candidate 0) comes from the refits alone
    assert int(guided["pl"].restart.sum()) == 1                           # the flags are the caller's: a plan reads them, it does not clear them


def test_tail_word_of_the_nominal_matches_the_reference(guided):
    low, high = guided["real"].action_space.low, guided["real"].action_space.high
    cpu = lambda t: t.cpu().numpy()
    done_last = cpu(guided["block"]["done"][H - 1])
    ref = Q.plan_tail(cpu(guided["candidates"]), cpu(guided["weights"]), cpu(guided["best"]), cpu(guided["lengths"]), done_last, cpu(guided["tail_policy_action"]),
                      low, high, K, 0.5)
    mean, plan = cpu(guided["mean"]), cpu(guided["plan_actions"])
    err = np.abs(mean[:, H - 1].astype(np.float64) - ref["tail"])
    print("tail word: worst error", err.max(), "worst error / bound", float(np.max(err / np.maximum(ref["b_tail"], 1e-300))))
    assert np.all(err <= ref["b_tail"])
    assert np.array_equal(mean[:, :H - 1].view(np.int32), plan[:, 1:].view(np.int32))                     # the rest is usim_plan_update's shift
    x, alive = Q.tail_rows(cpu(guided["candidates"]), cpu(guided["lengths"]), done_last, cpu(guided["tail_policy_action"]))
    assert alive[K:2 * K].all() and not alive[:K].any() and not alive[2 * K:3 * K].any()
    assert np.array_equal(mean[0, H - 1].view(np.int32), plan[0, H - 1].view(np.int32))                   # no survivor in group 0: the plan's own last action, same order
    assert not np.array_equal(mean[1, H - 1], plan[1, H - 1])


def test_the_critics_value_enters_the_score_within_the_policy_kernels_bound(usim, guided):
    """the network on the candidates' last observations against policy_ref's float64 forward pass on the observation the kernel normalised, under
    policy_ref.forward_bounds; the return of a survivor is fmaf(disc_H, s v, base): the value's bound scaled by disc_H s, the product s v rounded once (U24 of
    it, scaled by disc_H) and the fmaf rounded once (U24 of the result)"""
    pl, lib = guided["pl"], usim._lib.load()
    A = guided["real"].action_dim
    obs = guided["block"]["obs"][H - 1].contiguous()
    nobs = torch.zeros((N, 19), dtype=torch.float32, device=DEV)
    value, act = torch.zeros(N, dtype=torch.float32, device=DEV), torch.zeros((N, A), dtype=torch.float32, device=DEV)
    out = usim._lib.UsimPolicyOut(act.data_ptr(), nobs.data_ptr(), None, value.data_ptr(), None, None)
    rc = lib.usim_policy_step(C.byref(pl._net), C.byref(pl._stats), obs.data_ptr(), None, N, A, pl._low.data_ptr(), pl._high.data_ptr(), 17, 0, None, 0, 0, 1,
                              C.byref(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(_i32(value), _i32(guided["tail_value"])) and torch.equal(_i32(act), _i32(guided["tail_policy_action"]))    # the launch plan() made
    p = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in P.params_from_sb3(dict(np.load(ROOT / "tests/golden/tracking_policy.npz"))).items()}
    x = nobs.cpu().numpy().astype(np.float64)
    mean64, v64 = P.forward(p, x)
    bmean, bvalue = P.forward_bounds(p, x, UNITS)
    ev = np.abs(value.cpu().numpy().astype(np.float64) - v64)
    print("value: worst error", ev.max(), "worst error / bound", float(np.max(ev / bvalue)))
    assert np.all(ev <= bvalue)
    low, high = guided["real"].action_space.low.astype(np.float64), guided["real"].action_space.high.astype(np.float64)
    assert np.all(np.abs(act.cpu().numpy() - np.clip(mean64, low, high)) <= bmean)
    # ... and from there into the returns
    sim = guided["sim"]
    base, length = sim.score_block(guided["block"], gamma=GAMMA)
    base, length = base.cpu().numpy().astype(np.float64), length.cpu().numpy()
    alive = (length == H) & (guided["block"]["done"][H - 1].cpu().numpy() == 0)
    got = guided["returns"].cpu().numpy().astype(np.float64)
    assert np.array_equal(got[~alive], base[~alive]) and alive.any() and (~alive).any()
    ds = float(_disc()) * float(Q.tail_scale(float(guided["vn"].ret_var), guided["vn"].epsilon))
    want = base + ds * v64
    bound = ds * bvalue + 1.01 * U24 * (ds * np.abs(v64) + np.abs(got))
    err = np.abs(got - want)
    print("returns of survivors: worst error", err[alive].max(), "worst error / bound", float(np.max(err[alive] / bound[alive])), "value term", ds * np.abs(v64[alive]).mean())
    assert np.all(err[alive] <= bound[alive])


def test_planner_expert_labels_with_the_guided_plan(usim, guided):
    pl, real = guided["pl"], guided["real"]
    counter = int(pl.noise_counter.item())
    expert = usim.PlannerExpert(pl)
    expert.check_env(real)
    act, value = expert.label(real._obs)
    assert act is pl.action and value is None and int(pl.noise_counter.item()) == counter + ALL["iterations"]
    assert torch.equal(_i32(real.save_envs()), _i32(guided["after"][0]))


# ---- 3. a recorded step replays the eager one, with every option ----------------------------------------------------------------------------
def test_record_and_replay_equal_eager_steps(usim, pins):
    policy, vn = _critic(usim, pins, True)
    real, sim, pl = _setup(usim, short=False, critic=(policy, vn), **ALL)
    pl.step()
    rows = torch.arange(G, dtype=torch.int32, device=DEV)
    start = dict(state=real.save_envs().clone(), mean=pl.mean.clone(), restart=pl.restart.clone(), counter=pl.noise_counter.clone())

    def three(step):
        real.load_envs(start["state"], rows)
        pl.mean.copy_(start["mean"]); pl.restart.copy_(start["restart"]); pl.noise_counter.copy_(start["counter"])
        seen = []
        for _ in range(3):
            obs, rew, done = step()
            seen.append([t.clone() for t in (pl.action, pl.returns, pl.best, pl.mean, pl.sigma_elem, pl.elite, pl.tail_value, obs, rew, done, real.save_envs())])
        return seen

    eager = three(pl.step)
    assert not any(bool(s[9].any()) for s in eager)
    pl.record()
    replayed = three(pl.replay)
    torch.cuda.synchronize()
    assert int(pl.noise_counter.item()) == int(start["counter"].item()) + 3 * ALL["iterations"]
    for k, (a, b) in enumerate(zip(eager, replayed)):
        for x, y in zip(a, b):
            assert torch.equal(_i32(x), _i32(y)), k
    assert not torch.equal(eager[0][0], eager[1][0])
    real.close(); sim.close()
