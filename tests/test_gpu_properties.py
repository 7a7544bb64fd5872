"""Size-independent properties of the HIP path at BASELINE's full size (4096 / 8192 envs per GPU) and the VecEnv protocol."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle_lib import deep_spawn_params

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _env(usim, n, torso="soft", **kw):
    opts = dict(usim.default_robosuite_kwargs())
    seed = kw.pop("seed", 3)
    opts.update(kw)
    return usim.UltrasoundVecEnv(n, device="cuda:0", seed=seed, torso=torso, **opts)


def _rollout_hash(env, steps):
    env.reset_tensor()
    acc = []
    for k in range(steps):
        a = env.random_actions_tensor(k)
        obs, rew, done = env.step_tensor(a)
        acc.append((obs.clone(), rew.clone(), done.clone()))
    torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize("torso", ["rigid", "soft"])
def test_determinism_bit_exact_at_4096(usim, torso):
    a, b = _env(usim, 4096, torso), _env(usim, 4096, torso)
    ra, rb = _rollout_hash(a, 60), _rollout_hash(b, 60)
    for (o1, r1, d1), (o2, r2, d2) in zip(ra, rb):
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    assert not torch.isnan(ra[-1][0]).any()
    a.close(); b.close()


def test_lane_independence_and_env_offset_sharding(usim):
    """env i of a 4096 batch == env i of a 64 batch == env (i - 4000) of a shard created with env_offset 4000"""
    big, small, shard = _env(usim, 4096), _env(usim, 64), _env(usim, 96, env_offset=4000)
    rb, rs, rh = _rollout_hash(big, 40), _rollout_hash(small, 40), _rollout_hash(shard, 40)
    for (ob, rwb, db), (os_, rws, ds), (oh, rwh, dh) in zip(rb, rs, rh):
        assert torch.equal(ob[:64], os_) and torch.equal(rwb[:64], rws) and torch.equal(db[:64], ds)
        assert torch.equal(ob[4000:4096], oh) and torch.equal(db[4000:4096], dh)
    for e in (big, small, shard):
        e.close()


def test_rollout_random_equals_explicit_actions(usim):
    """one launch of many steps (up to 256 since round 4; the rollout below is cut at the reset bank's refill period: 256 + 44) == the same steps one launch each"""
    a, b = _env(usim, 512), _env(usim, 512)
    a.reset_tensor(); b.reset_tensor()
    blk = a.alloc_block(300)
    a.rollout_random(0, 300, blk)
    assert int(blk["done"].sum()) > 100                                  # (episodes end and restart inside the launches)
    for k in range(300):
        act = b.random_actions_tensor(k)
        obs, rew, done = b.step_tensor(act)
        torch.cuda.synchronize()
        assert torch.equal(blk["obs"][k], obs) and torch.equal(blk["rew"][k], rew) and torch.equal(blk["done"][k], done)
        assert torch.equal(blk["act"][k], act)
    a.close(); b.close()


@pytest.mark.parametrize("torso", ["rigid", "soft"])
def test_substeps_are_the_same_physics_as_single_steps(usim, torso):
    """control_freq 100 = five 2 ms physics substeps per env.step().  In the open-loop `wrench` mode nothing in the physics depends on the control-step
    counter, so q, qd and the lattice after k steps at 100 Hz are, bit for bit, those after 5 k steps at 500 Hz with every action held for five
    steps; the bookkeeping differs as the reference's does (t counts control steps, dF/dt is taken over 10 ms).  Also: every kernel mapping
    computes the same bits with substeps, and a multi-step rollout equals stepping one control step at a time."""
    cc = dict(usim.default_robosuite_kwargs()["controller_configs"], impedance_mode="wrench")
    slow, fast = _env(usim, 300, torso, controller_configs=cc, control_freq=100, early_termination=False), _env(usim, 300, torso, controller_configs=cc, early_termination=False)
    slow.reset_tensor(); fast.reset_tensor()
    for k in range(30):
        act = slow.random_actions_tensor(k).clone()
        slow.step_tensor(act)
        for _ in range(5):
            fast.step_tensor(act)
    a, b = slow.get_state(), fast.get_state()
    for key in ("q", "qd", "s", "sd"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["t"], np.full(300, 30)) and np.array_equal(b["t"], np.full(300, 150))
    slow.close(); fast.close()
    if torso == "soft":
        kw = dict(control_freq=125, early_termination=True)
        envs = [_env(usim, 500, lanes_per_env=32, **kw), _env(usim, 500, lanes_per_env=16, **kw), _env(usim, 500, lanes_per_env=64, **kw)]
        for e in envs:
            e.reset_tensor()
        blk = [e.alloc_block(40) for e in envs]
        envs[0].rollout_random(0, 40, blk[0]); envs[2].rollout_random(0, 40, blk[2])
        for k in range(40):                                                  # one control step (four substeps) per launch
            act = envs[1].random_actions_tensor(k)
            obs, rew, done = envs[1].step_tensor(act)
            blk[1]["obs"][k], blk[1]["rew"][k], blk[1]["done"][k] = obs, rew, done
        torch.cuda.synchronize()
        for key in ("obs", "rew", "done"):
            assert torch.equal(blk[0][key], blk[1][key]) and torch.equal(blk[0][key], blk[2][key]), key
        assert int(blk[0]["done"].sum()) >= 10                               # episodes ended and restarted from the bank on the way
        for e in envs:
            e.close()
    # `fixed` mode: the goal anchored at the policy step is held across the substeps; every mapping holds it the same way
    fx = dict(controller_configs=dict(cc, impedance_mode="fixed"), control_freq=100, early_termination=True)
    fenvs = [_env(usim, 200, torso, **fx)] + ([_env(usim, 200, torso, lanes_per_env=16, **fx), _env(usim, 200, torso, lanes_per_env=64, **fx)] if torso == "soft" else [])
    for e in fenvs:
        e.reset_tensor()
    for k in range(40):
        act = fenvs[0].random_actions_tensor(k).clone()
        res = [[x.clone() for x in e.step_tensor(act)] for e in fenvs]
        for r in res[1:]:
            assert all(torch.equal(a, b) for a, b in zip(res[0], r)), k
    for e in fenvs:
        e.close()


def test_state_roundtrip_checkpoint(usim):
    a, b = _env(usim, 300), _env(usim, 300)
    a.reset_tensor(); b.reset_tensor()
    a.rollout_random(0, 25)
    st = a.get_state()
    b.set_state(st)
    st2 = b.get_state()
    for k in st:
        assert np.array_equal(st[k], st2[k]), k
    act = a.random_actions_tensor(25).clone()
    oa = [t.clone() for t in a.step_tensor(act, auto_reset=False)]
    ob = [t.clone() for t in b.step_tensor(act, auto_reset=False)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    a.close(); b.close()


def test_full_torso_checkpoint_determinism_and_auto_reset(usim):
    """torso="full" (csrc/usim_full.h; ultrasound.py:426-431 free joint, soft_box.xml:9 all 270 elements): the state that usim_get_state / usim_get_body_state hand out
    restores the simulation bit for bit on another handle; two handles run identically; an episode that ends re-spawns the torso (body at its spawn pose, sliders at
    rest) inside the step kernel; the body comes to rest on the table within a millimetre of the height the top-face model pins its base at."""
    def mk():
        return usim.UltrasoundVecEnv(192, device="cuda:0", seed=5, torso="full", **usim.default_robosuite_kwargs())
    a, b = mk(), mk()
    assert a.num_elements == 270
    a.reset_tensor(); b.reset_tensor()
    spawn = a.get_state()["body"].copy()
    assert np.allclose(spawn[:, 3:7], [1, 0, 0, 0]) and np.all(spawn[:, 7:] == 0) and np.ptp(spawn[:, 2]) == 0
    a.rollout_random(0, 30)
    st = a.get_state()
    assert np.isfinite(st["body"]).all() and np.isfinite(st["s"]).all() and np.abs(st["body"][:, 3:7]).max() <= 1.0 + 1e-6
    assert np.all(np.abs(st["body"][:, 2] - spawn[:, 2]) < 1e-3) and np.abs(st["s"]).max() < 0.04        # resting on its rim capsules; dents of centimetres at most
    b.set_state(st)
    st2 = b.get_state()
    for k in st:
        assert np.array_equal(st[k], st2[k]), k
    # the step after the restore: bit for bit (the joint words travel as q = q0 + dq, which is exact for this step and within rounding afterwards, as for every torso)
    act = a.random_actions_tensor(30).clone()
    oa = [t.clone() for t in a.step_tensor(act)]
    ob = [t.clone() for t in b.step_tensor(act)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    # two handles from the same seed: identical, step after step
    c, d = mk(), mk()
    c.reset_tensor(); d.reset_tensor()
    for k in range(8):
        act = c.random_actions_tensor(k).clone()
        oc = [t.clone() for t in c.step_tensor(act)]
        od = [t.clone() for t in d.step_tensor(act)]
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(oc, od)), k
    c.close(); d.close()
    a.close(); b.close()
    # auto-reset at a KNOWN step (horizon 12, no early termination: every episode ends at step 12): the step that ends an episode leaves the free body at its spawn
    # pose, the sliders at rest and no warm start -- read right after it, asserted for every environment
    kw = usim.default_robosuite_kwargs(); kw["horizon"] = 12; kw["early_termination"] = False
    e = usim.UltrasoundVecEnv(64, device="cuda:0", seed=5, torso="full", **kw)
    e.reset_tensor()
    spawn = e.get_state()["body"].copy()
    for k in range(11):
        _, _, done = e.step_tensor(e.random_actions_tensor(k))
    assert not done.any()
    mid = e.get_state()
    assert np.abs(mid["s"]).max() > 1e-4 and np.abs(mid["solver_warm_start"][:, :4 * 270]).max() > 0          # the torso has moved and carries contact forces
    _, _, done = e.step_tensor(e.random_actions_tensor(11))
    assert done.all()
    se = e.get_state()
    assert np.all(se["t"] == 0) and np.all(se["episode"] == mid["episode"] + 1)
    assert np.array_equal(se["body"], spawn) and np.all(se["s"] == 0) and np.all(se["sd"] == 0)
    ws = se["solver_warm_start"]
    assert np.all(ws[:, :4 * 270] == 0) and np.all(ws[:, 4 * 270:4 * 270 + 8] == -1) and np.all(ws[:, 4 * 270 + 8:] == 0)
    e.close()


def test_full_torso_banked_reset_equals_live_reset(usim):
    """torso="full": an episode adopted from the reset bank (computed ahead by a refill launch, parked in the bank, adopted inside the step that ends the episode
    before it) is bit for bit the episode that a live reset of the same environment and episode index computes: reset draws, initial-pose IK, zero-torque forward
    pass, park and adopt.  Horizon 12 without early termination: every episode of handle A ends at step 12; handle B gets to the same episode index by resets only."""
    kw = usim.default_robosuite_kwargs(); kw["horizon"] = 12; kw["early_termination"] = False
    def mk():
        return usim.UltrasoundVecEnv(64, device="cuda:0", seed=5, torso="full", **kw)
    a, b = mk(), mk()
    a.reset_tensor()
    for k in range(12):
        obs_a, _, done = a.step_tensor(a.random_actions_tensor(k))
    assert done.all()
    obs_a = obs_a.clone()
    b.reset_tensor()
    obs_b = b.reset_tensor().clone()
    torch.cuda.synchronize()
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa["episode"], sb["episode"])
    assert torch.equal(obs_a, obs_b)
    assert set(sa) == set(sb) and {"q", "qd", "body", "s", "sd", "solver_warm_start"} <= set(sa)
    for k in sa:                                       # q, qd, q0 and every per-episode scalar; body, s, sd, solver_warm_start
        assert np.array_equal(sa[k], sb[k]), k
    a.close(); b.close()


def test_full_torso_rejects_the_configurations_it_does_not_run(usim):
    """torso="full" runs the Panda at control_freq 500 (the reference's callers: rl_config.yaml:26, robots Panda); the UR5e (ultrasound.py:137) and control_freq below
    500 (ultrasound.py:119: physics substeps) are refused at creation with USIM_ERR_UNSUPPORTED and a message, not run as something else; the top-face model runs both."""
    kw = usim.default_robosuite_kwargs()
    for bad in (dict(robots="UR5e"), dict(control_freq=20), dict(control_freq=100)):
        with pytest.raises(RuntimeError, match="(?i)unsupported.*USIM_TORSO_FULL|USIM_TORSO_FULL.*Panda"):
            usim.UltrasoundVecEnv(32, device="cuda:0", seed=1, torso="full", **dict(kw, **bad))
        usim.UltrasoundVecEnv(32, device="cuda:0", seed=1, torso="soft", **dict(kw, **bad)).close()
    usim.UltrasoundVecEnv(32, device="cuda:0", seed=1, torso="full", **kw).close()


def test_full_torso_numerical_fault_guard(usim):
    """The fault guard sees the torso: a non-finite word in the free body's state or in a slider ends the episode with status bit 2 and the environment restarts clean
    (free body at the spawn pose, sliders at rest, no warm start), its neighbours untouched.  (Until round 6 the guard looked at the arm only: a torso gone NaN fails
    every comparison of the forward pass, its contacts vanish silently and the arm stays finite.)"""
    n = 64
    def mk():
        return usim.UltrasoundVecEnv(n, device="cuda:0", seed=9, torso="full", **usim.default_robosuite_kwargs())
    env, ref = mk(), mk()
    env.reset_tensor(); ref.reset_tensor()
    spawn = env.get_state()["body"].copy()
    for k in range(4):
        a = env.random_actions_tensor(k).clone()
        env.step_tensor(a); ref.step_tensor(a)
    st = env.get_state()
    st["body"][5, 0] = np.nan          # position
    st["s"][9, 131] = np.nan           # one slider
    st["body"][11, 11] = np.inf        # angular velocity
    st["body"][13, 4] = np.nan         # quaternion
    env.set_state(st); ref.set_state(ref.get_state())
    bad = [5, 9, 11, 13]
    a = env.random_actions_tensor(4).clone()
    obs, rew, done = [t.clone() for t in env.step_tensor(a)]
    obs_r, rew_r, done_r = [t.clone() for t in ref.step_tensor(a)]
    torch.cuda.synchronize()
    status = env.status.cpu().numpy()
    ok = np.ones(n, bool); ok[bad] = False
    assert done[bad].all() and (status[bad] & 4).all() and not (status[ok] & 4).any()
    assert torch.equal(obs[ok], obs_r[ok]) and torch.equal(rew[ok], rew_r[ok]) and torch.equal(done[ok], done_r[ok])
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and (rew[bad] == 0).all()
    s2 = env.get_state()
    assert all(np.isfinite(s2[k]).all() for k in ("q", "qd", "s", "sd", "body", "solver_warm_start"))
    assert np.array_equal(s2["body"][bad], spawn[bad]) and np.all(s2["s"][bad] == 0) and np.all(s2["t"][bad] == 0)
    ws = s2["solver_warm_start"][bad]
    assert np.all(ws[:, :4 * 270] == 0) and np.all(ws[:, 4 * 270:4 * 270 + 8] == -1) and np.all(ws[:, 4 * 270 + 8:] == 0)
    # and the restarted environments run on
    for k in range(5, 10):
        obs, rew, done = env.step_tensor(env.random_actions_tensor(k))
    assert torch.isfinite(obs).all() and np.isfinite(env.get_state()["body"]).all()
    env.close(); ref.close()


def test_vecenv_protocol_and_auto_reset(usim):
    n = 128
    # horizon also sets the trajectory speed (ultrasound.py:528-529), so a short horizon needs early termination off
    kw = usim.default_robosuite_kwargs(); kw["horizon"] = 20; kw["early_termination"] = False
    env = usim.UltrasoundVecEnv(n, device="cuda:0", seed=11, torso="soft", **kw)
    assert env.num_envs == n and env.observation_space.shape == (19,) and env.action_space.shape == (6,)
    assert env.action_space.low.min() == 0.0 and env.action_space.high.max() == 1.0
    obs = env.reset()
    assert obs.shape == (n, 19) and obs.dtype == np.float32 and np.isfinite(obs).all()
    assert np.all(obs[:, 6:9] == 0) and np.allclose(obs[:, 11], -0.04)
    rng = np.random.default_rng(0)
    total_done = 0
    for k in range(45):
        actions = np.stack([env.action_space.sample(rng) for _ in range(n)])
        obs, rew, done, infos = env.step(actions)
        assert obs.shape == (n, 19) and rew.shape == (n,) and done.shape == (n,) and done.dtype == bool and len(infos) == n
        assert np.isfinite(obs).all() and np.isfinite(rew).all() and (rew >= 0).all() and (rew <= 12.0001).all()
        for i in np.nonzero(done)[0]:
            assert infos[i]["terminal_observation"].shape == (19,)
            ep = infos[i]["episode"]
            assert 1 <= ep["l"] <= 20 and 0 <= ep["r"] <= 12.0001 * ep["l"] and ep["t"] >= 0
            assert np.all(obs[i, 6:9] == 0) and obs[i, 10] == 0 and abs(obs[i, 11] + 0.04) < 1e-7    # reset observation returned
            assert "TimeLimit.truncated" not in infos[i]          # the reference stack never emits it (src/rl.py:36-40); opt-in below
        for i in np.nonzero(~done)[0][:4]:
            assert infos[i] == {}
        total_done += int(done.sum())
        assert done.all() == (k in (19, 39))      # the horizon ends every episode together
    assert total_done == 2 * n
    env_t = usim.UltrasoundVecEnv(4, device="cuda:0", seed=11, torso="soft", report_truncation=True, **kw)
    env_t.reset()
    for k in range(20):
        _, _, done_t, infos_t = env_t.step(np.stack([env_t.action_space.sample(rng) for _ in range(4)]))
        for i in np.nonzero(done_t)[0]:
            assert infos_t[i]["TimeLimit.truncated"] == (infos_t[i]["episode"]["l"] == 20)
    assert done_t.all()
    env_t.close()
    assert env.get_attr("horizon") == [20] * n and env.env_is_wrapped(object) == [False] * n
    with pytest.raises(ValueError):
        env.step(np.zeros((n, 5), dtype=np.float32))
    env.seed(5)
    o1 = env.reset(); env.seed(5); o2 = env.reset()
    assert np.array_equal(o1, o2)
    env.seed(6)
    assert not np.array_equal(o1, env.reset())
    env.close()


def test_single_env_view_follows_gym_semantics(usim):
    kw = usim.default_robosuite_kwargs(); kw["horizon"] = 10; kw["early_termination"] = False
    kw["controller_configs"] = dict(kw["controller_configs"], impedance_mode="fixed")
    env = usim.UltrasoundEnv(device="cuda:0", seed=1, torso="rigid", **kw)
    lo, hi = env.action_spec
    assert np.array_equal(lo, -np.ones(6)) and np.array_equal(hi, np.ones(6)) and env.horizon == 10
    with pytest.raises(ValueError):
        env.step(np.zeros(6))                      # step before reset / after done (robosuite MujocoEnv.step)
    obs = env.reset()
    assert obs.shape == (19,)
    ret = 0.0
    for t in range(10):                            # src/main.py:67-70: zero-action rollout
        obs, r, done, info = env.step([0.0] * 6)
        ret += r
        assert done == (t == 9) and info == {}
    assert ret > 0 and env.reward() == r
    with pytest.raises(ValueError):
        env.step(np.zeros(6))
    env.close()


def test_reset_distribution_matches_reference_fixtures(usim, pins):
    """Reset observations of 8192 GPU envs against the decoded reference rows: same structural pins as
    tests/test_oracle_env_formulas.py, evaluated on the HIP path."""
    env = _env(usim, 8192)
    obs = env.reset()
    ref = np.concatenate([pins[m + "_reset_obs"] for m in ("tracking", "variable_z", "wrench")])
    assert np.all(obs[:, 6:9] == 0) and np.all(obs[:, 10] == 0) and np.allclose(obs[:, 11], -0.04)
    assert np.allclose(obs[:, 9], obs[:, 2] - 5.0, atol=1e-5)
    assert np.allclose(obs[:, 15], -1.0, atol=1e-3) and np.abs(obs[:, 16:19]).max() < 1e-3
    assert np.allclose(obs[:, 12:15].mean(0), [0.0028, 0.0008, 0.0066], atol=4e-4)
    assert np.allclose(obs[:, 12:15].std(0), [0.0025, 0.0025, 0.010], rtol=0.05)
    # the six force / torque channels against the reference rows: the same bands as the oracle's test (onset, force-depth bins incl. the deep
    # rows, spread of Fx / Fz / torque x / torque y within 30 %, the known gaps of Fy and torque z at their measured size)
    from test_oracle_env_formulas import check_reset_rows_against_reference
    assert np.all(obs[:, 2] >= 0)
    check_reset_rows_against_reference(obs.astype(np.float64), ref)
    env.close()


def test_long_random_rollout_stays_finite_at_full_size(usim):
    """2000 steps x 4096 envs with auto-reset: nothing diverges, rewards bounded by 12/step, episodes end and restart."""
    env = _env(usim, 4096)
    env.reset_tensor()
    blk = env.alloc_block(250)
    ndone = 0
    for b in range(8):
        env.rollout_random(b * 250, 250, blk)
        torch.cuda.synchronize()
        assert torch.isfinite(blk["obs"]).all() and torch.isfinite(blk["rew"]).all()
        assert blk["rew"].min() >= 0 and blk["rew"].max() <= 12.0001
        # contact force sane: a glancing contact on the flank of a cap can have a downward normal, but it stays rare and bounded
        fz = blk["obs"][..., 2]
        assert fz.min() > -100 and fz.max() < 500 and (fz < -1.0).float().mean() < 1e-3
        ndone += int(blk["done"].sum())
    st = env.get_state()
    assert ndone > 4096 and st["episode"].min() >= 1 and st["t"].max() <= 1000
    assert np.isfinite(st["q"]).all() and np.abs(st["s"]).max() < 0.03
    # contact-slot overflow (bit 0, sticky for the episode): 15 % of the episodes START with more than eight penetrating elements (the blade
    # spawned up to 3 cm deep), 2 % of the steps run with all eight slots taken (profiles/r03/soak.txt)
    assert (st["status"] != 0).mean() < 0.3
    env.close()


def test_episode_csv_dump_matches_reference_wire_format(usim, tmp_path, monkeypatch):
    """save_data=True (ultrasound.py:479-509, 552-614, 890-910): 23 files in three folders, `horizon` rows, no header, `_<idx>` suffix,
    channels consistent with the step outputs."""
    monkeypatch.chdir(tmp_path)
    kw = usim.default_robosuite_kwargs(); kw["horizon"] = 40; kw["early_termination"] = False; kw["save_data"] = True
    env = usim.UltrasoundEnv(device="cuda:0", seed=5, **kw)
    for ep in range(2):
        obs = env.reset()
        rewards, forces = [], []
        for t in range(40):
            obs, r, done, _ = env.step(np.full(6, 0.6, dtype=np.float32))
            rewards.append(r); forces.append(obs[2])
        assert done
    sim, rew, pol = tmp_path / "simulation_data", tmp_path / "reward_data", tmp_path / "policy_data"
    assert len(list(sim.glob("*_1.csv"))) == 17 and len(list(rew.glob("*_2.csv"))) == 5 and (pol / "action_2.csv").exists()
    load = lambda p: np.loadtxt(p, delimiter=",", ndmin=2)
    ee_pos, goal = load(sim / "ee_pos_2.csv"), load(sim / "ee_goal_pos_2.csv")
    assert ee_pos.shape == (40, 3) and goal.shape == (40, 3) and load(sim / "q_pos_2.csv").shape == (40, 7)
    assert load(sim / "ee_quat_2.csv").shape == (40, 4) and load(pol / "action_2.csv").shape == (40, 6)
    terms = sum(load(rew / f"{n}_2.csv")[:, 0] for n in ("pos", "ori", "vel", "force", "derivative_force"))
    assert np.allclose(terms, rewards, atol=1e-5)                                   # the five shaped terms add up to the step reward
    assert np.allclose(load(sim / "ee_z_contact_force_2.csv")[:, 0], forces, atol=1e-5)
    assert np.allclose(load(sim / "time_2.csv")[:, 0], np.arange(40) / 40 * 100, atol=1e-4)
    assert np.all(np.abs(load(sim / "q_torques_2.csv")) <= np.array([80, 80, 80, 80, 12, 12, 12]) + 1e-4)
    assert np.allclose(load(sim / "ee_goal_vel_2.csv"), 0.04) and np.allclose(load(sim / "ee_z_goal_contact_force_2.csv"), 5.0)
    assert np.allclose(np.linalg.norm(load(sim / "ee_quat_2.csv"), axis=1), 1.0, atol=1e-5)
    assert np.allclose(goal[:, 2], 0.8572 + 0.039, atol=1e-5)                       # trajectory height (ultrasound.py:807)
    assert np.allclose(load(pol / "action_2.csv"), 0.6)
    assert set(np.unique(load(sim / "is_contact_2.csv"))) <= {0.0, 1.0}
    env.close()


def test_numerical_fault_guard_and_action_sanitising(usim):
    """Non-finite action components are treated as 0; a non-finite / run-away state ends the episode, sets status bit 2 and the
    environment restarts from its next prepared episode while its neighbours are untouched."""
    from oracle_lib import Oracle
    n = 64
    env, ref = _env(usim, n, "soft"), _env(usim, n, "soft")
    env.reset_tensor(); ref.reset_tensor()
    act = env.random_actions_tensor(0).clone()
    bad = act.clone(); bad[3, 2] = float("nan"); bad[7, 0] = float("inf")
    clean = act.clone(); clean[3, 2] = 0.0; clean[7, 0] = 0.0
    o1 = [t.clone() for t in env.step_tensor(bad)]; o2 = [t.clone() for t in ref.step_tensor(clean)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(o1, o2)) and torch.isfinite(o1[0]).all()
    st = env.get_state()
    st["q"][5, :] = np.nan; st["qd"][9, :] = 1e9
    env.set_state(st); ref.set_state(ref.get_state())
    a1 = env.random_actions_tensor(1).clone()
    obs, rew, done = [t.clone() for t in env.step_tensor(a1)]
    obs_r, rew_r, done_r = [t.clone() for t in ref.step_tensor(a1)]
    torch.cuda.synchronize()
    status = env.status.cpu().numpy()
    assert done[5] and done[9] and (status[5] & 4) and (status[9] & 4)
    ok = np.ones(n, bool); ok[[5, 9]] = False
    assert torch.equal(obs[ok], obs_r[ok]) and torch.equal(done[ok], done_r[ok]) and not (status[ok] & 4).any()
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and rew[5] == 0     # faulted envs: reset observation, zero reward
    st2 = env.get_state()
    assert np.isfinite(st2["q"]).all() and st2["t"][5] == 0 and st2["episode"][5] == st["episode"][5] + 1
    # the oracle applies the same rule
    ora = Oracle(4, torso="top"); ora.reset(); so = ora.get_state(); so["q"][1, :] = np.nan; ora.set_state(so)
    _, _, d, _, _ = ora.step(ora.random_actions(0))
    assert d[1] and int(ora.get_state()["episode"][1]) == int(so["episode"][1]) + 1
    env.close(); ref.close()


@pytest.mark.parametrize("lanes", [0, 64])
def test_config3_global_batch_equals_its_shards(usim, lanes):
    """BASELINE configs[3]: 32768 environments sharded 8 x 4096.  The first and the last 4096-env shard (env_offset = 0 / 28672)
    reproduce their slice of one 32768-env handle bit for bit -- no state is shared between environments.  (lanes = 64: one fixed
    mapping, the split kernel with 8-lane groups, for the whole batch and its shards; lanes = 0: the automatic choice, i.e. that kernel
    at 32768 envs and the split kernel with 16-lane groups in the shards: two mappings give the same bits)"""
    kw = dict(usim.default_robosuite_kwargs(), lanes_per_env=lanes)
    whole = usim.UltrasoundVecEnv(32768, device="cuda:0", seed=3, torso="soft", **kw)
    first = usim.UltrasoundVecEnv(4096, device="cuda:0", seed=3, torso="soft", env_offset=0, **kw)
    last = usim.UltrasoundVecEnv(4096, device="cuda:0", seed=3, torso="soft", env_offset=28672, **kw)
    rw, rf, rl = _rollout_hash(whole, 24), _rollout_hash(first, 24), _rollout_hash(last, 24)
    for (ow, rww, dw), (of, rwf, df), (ol, rwl, dl) in zip(rw, rf, rl):
        assert torch.equal(ow[:4096], of) and torch.equal(rww[:4096], rwf) and torch.equal(dw[:4096], df)
        assert torch.equal(ow[28672:], ol) and torch.equal(rww[28672:], rwl) and torch.equal(dw[28672:], dl)
    assert not torch.isnan(rw[-1][0]).any()
    for e in (whole, first, last):
        e.close()


def test_two_live_handles_with_different_torso_shapes_do_not_share_tables(usim):
    """The lattice tables (element positions / axes, lattice inverse, shell ids) belong to the handle: a box-torso env steps the same
    whether or not a cylinder-torso env was created after it on the same GPU (and vice versa)."""
    def run(env, steps=40):
        out = _rollout_hash(env, steps)
        return torch.stack([o for o, _, _ in out]), env.contacts.clone()
    box_alone = _env(usim, 128, use_box_torso=True)
    ref_box, ref_box_con = run(box_alone)
    ref_box2, _ = run(box_alone)                         # the following episodes of the same handle
    box_alone.close()
    cyl_alone = _env(usim, 128, use_box_torso=False)
    ref_cyl, ref_cyl_con = run(cyl_alone); cyl_alone.close()
    assert not torch.equal(ref_box, ref_cyl)
    box = _env(usim, 128, use_box_torso=True)
    cyl = _env(usim, 128, use_box_torso=False)          # created while `box` is alive
    got_box, got_box_con = run(box)
    got_cyl, got_cyl_con = run(cyl)
    got_box2, _ = run(box)                               # box again after the cylinder env has stepped
    assert torch.equal(got_box, ref_box) and torch.equal(got_box_con, ref_box_con) and torch.equal(got_box2, ref_box2)
    assert torch.equal(got_cyl, ref_cyl) and torch.equal(got_cyl_con, ref_cyl_con)
    box.close(); cyl.close()


def test_split_kernel_equals_the_single_wave_kernel_bit_for_bit(usim):
    """lanes_per_env = 32 (arm side and lattice / contact side of a quad of environments in two waves, mailboxes in LDS; the automatic choice
    up to 4096 envs) and lanes_per_env = 16 (one wave does both) are the same arithmetic: identical bits over 300 steps with auto-resets,
    both register budgets of the 16-lane kernel included"""
    envs = [_env(usim, 1000, lanes_per_env=32), _env(usim, 1000, lanes_per_env=16, waves_per_simd=1), _env(usim, 1000, lanes_per_env=16, waves_per_simd=2),
            _env(usim, 1000, lanes_per_env=64)]        # 64: the split kernel with 8-lane groups (two environments per DPP row)
    obs0 = [e.reset_tensor().clone() for e in envs]
    assert all(torch.equal(obs0[0], o) for o in obs0[1:])
    ended = 0
    for k in range(300):
        act = envs[0].random_actions_tensor(k).clone()
        res = [[x.clone() for x in e.step_tensor(act)] for e in envs]
        for r, e in zip(res[1:], envs[1:]):
            assert all(torch.equal(a, b) for a, b in zip(res[0], r)) and torch.equal(envs[0].contacts, e.contacts), k
        ended += int(res[0][2].sum())
    assert ended > 100
    s0 = envs[0].get_state()
    for e in envs[1:]:
        s = e.get_state()
        assert all(np.array_equal(s0[key], s[key]) for key in s0)
    for e in envs:
        e.close()


def test_every_mapping_resolves_a_slot_overflow_to_the_same_bits(usim):
    """probes spawned 1.2-3 cm deep (the reset of test_contact_slot_overflow_parity, which checks it against the oracle): more elements penetrate than there are
    contact slots in every workgroup, so the slot rule of the single-wave kernel (lanes_per_env 16), of the split kernel with 16-lane groups (32; after hand-off
    (2)) and with 8-lane groups (64; before it) all run -- same bits at the reset and over the 25 steps that follow"""
    n = 256
    envs = [_env(usim, n, lanes_per_env=lanes) for lanes in (16, 32, 64)]
    for e in envs:
        e.reset_tensor()
    p = deep_spawn_params(envs[0].get_state(), n)
    obs0 = [e.reset_explicit_tensor(p).clone() for e in envs]
    assert all(torch.equal(obs0[0], o) for o in obs0[1:])
    status = [e.get_state()["status"].astype(int) & 1 for e in envs]
    assert status[0].sum() > 20 and all(np.array_equal(status[0], s) for s in status[1:])
    act = torch.full((n, 6), 0.5, dtype=torch.float32, device=envs[0].device)
    for k in range(25):
        res = [[x.clone() for x in e.step_tensor(act, auto_reset=False)] for e in envs]
        for r, e in zip(res[1:], envs[1:]):
            assert all(torch.equal(a, b) for a, b in zip(res[0], r)) and torch.equal(envs[0].contacts, e.contacts), k
    s0 = envs[0].get_state()
    for e in envs[1:]:
        s = e.get_state()
        assert all(np.array_equal(s0[key], s[key]) for key in s0)
    for e in envs:
        e.close()


def test_mapping_can_change_in_the_middle_of_a_rollout(usim):
    """usim_set_mapping: a rollout that alternates between the split kernel and the 16-lane kernel (both register budgets) every few
    steps is bit for bit the rollout of an env that never switches (what bench.py does around the all-gather for N > 1)"""
    a, b = _env(usim, 512), _env(usim, 512)
    a.reset_tensor(); b.reset_tensor()
    blk_a, blk_b = a.alloc_block(96), b.alloc_block(96)
    a.rollout_random(0, 96, blk_a)
    maps = [(16, 2), (32, 0), (16, 1), (32, 0), (16, 0), (32, 0)]
    for i, (lanes, waves) in enumerate(maps):
        b.set_mapping(lanes, waves)
        b.rollout_random(16 * i, 16, {k: t[16 * i:16 * (i + 1)] for k, t in blk_b.items()})
    torch.cuda.synchronize()
    for k in blk_a:
        assert torch.equal(blk_a[k], blk_b[k]), k
    with pytest.raises(RuntimeError):
        b.set_mapping(8, 0)
    rigid = _env(usim, 64, torso="rigid")
    with pytest.raises(RuntimeError):
        rigid.set_mapping(32, 0)
    for e in (a, b, rigid):
        e.close()


def test_split_kernel_roles_execute_the_same_number_of_barriers(usim, tmp_path):
    """The two roles of usim_step32_kernel meet at workgroup barriers placed at different program points (outside the HIP programming model; the
    invariant is stated at the kernel): the profiling build counts the barriers each role executes -- table copy + four hand-offs per step --
    and they must agree, also for a ragged last workgroup and right after a reset that overflows the contact slots."""
    import subprocess, sys, textwrap
    csrc = ROOT / "robotic-ultrasound-imaging_amd" / "csrc"
    prof = ROOT / "robotic-ultrasound-imaging_amd" / "lib" / "libusim_prof.so"
    subprocess.run(["make", "-s", "-C", str(csrc), "prof"], check=True)
    code = textwrap.dedent(f"""
        import importlib, sys
        sys.path.insert(0, {str(ROOT)!r})
        usim = importlib.import_module("robotic-ultrasound-imaging_amd")
        for n in (16, 1000, 37):
            env = usim.UltrasoundVecEnv(n, device="cuda:0", seed=3, lanes_per_env=32, **usim.default_robosuite_kwargs())
            env.reset_tensor()
            for k in range(3):
                t = env.profile_step_raw(k, n=48)
                print(n, k, t[46], t[47])
            env.close()
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, USIM_LIB=str(prof)))
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines() if line[:1].isdigit()]
    assert len(rows) == 9
    for n, k, arm, lat in rows:
        assert arm == lat == 5, (n, k, arm, lat)                  # table copy + hand-offs (1)-(4)


def test_kernel_contact_forces_rest_at_the_optimum_of_the_convex_problem(usim):
    """The kernels' contact solve AT ITS DEFAULT (block Jacobi with a line search, 24 iterations, the two coincident contacts of a pair explicit) against the
    optimum of the convex contact problem computed by the independent solver of tests/cone_qp.py from the dual problem the oracle exports at the same state: the
    round-4 review's bar for a converged solve -- 99 % of the environments within 1e-2 N, the worst within 5e-2 N, on net forces of up to 100 N -- holds in float32
    (MuJoCo's Newton solver converges to this optimum); 60 iterations sit on the float32 floor of the kinematics (~1e-3 N)."""
    from oracle_lib import Oracle
    from cone_qp import dual_problem, solve_exact, net_force
    n, pre = 128, 8
    ora = Oracle(n); ora.reset()
    for k in range(pre):
        ora.step(ora.random_actions(k))
    st, act = ora.get_state(), ora.random_actions(pre)
    probs = [dual_problem(ora, i, act[i]) for i in range(n)]
    live = [i for i, p in enumerate(probs) if p is not None]
    assert max(probs[i]["pairs"] for i in live) >= 6
    want = np.array([net_force(probs[i], solve_exact(probs[i])) for i in live])
    errs = {}
    for iters in (0, 60):
        env = _env(usim, n, **({"pgs_iters": iters} if iters else {}))
        env.reset()
        g = env.get_state()
        for key in ("q", "qd", "q0", "traj_start", "traj_end", "u0", "vbar", "fzbar", "fzprev", "dfz", "stiffness", "damping", "mu", "t", "has_touched", "episode", "ep_return", "status", "s", "sd"):
            g[key] = st[key]
        env.set_state(g)
        obs, *_ = env.step(act.astype(np.float32))
        errs[iters] = np.abs(obs[live, :3] - want).max(1)
        env.close()
    assert len(live) > 60 and np.abs(want).max() > 30
    assert np.quantile(errs[0], 0.99) < 1e-2 and errs[0].max() < 5e-2, (np.median(errs[0]), np.quantile(errs[0], 0.99), errs[0].max())        # the default
    assert np.quantile(errs[60], 0.99) < 5e-3 and errs[60].max() < 2e-2, (np.quantile(errs[60], 0.99), errs[60].max())       # float32 kinematics: ~1e-3 N on forces of up to 100 N
