"""imitation.DAggerTrainer end to end on small problems.  With imitation.PolicyExpert on the golden `tracking` weights: 32 rigid-torso environments, 2 rounds
of 16 steps (round 0 with beta = 1, round 1 with beta = 0: the default schedule) -- what the buffer holds and in which order, that every stored label is the
expert's, who acted, and that the student's action error falls.  With imitation.PlannerExpert: 4 soft-torso environments planned with 4 x 16 candidates over a
horizon of 4 -- the labels are planner.plan()'s first actions and the trainer steps planner.real as planner.step() would."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
N, T, ROUNDS = 32, 16, 2


def _i32(t):
    return t.contiguous().view(torch.int32)


def _env(usim, n=N, torso="rigid", seed=3):
    return usim.UltrasoundVecEnv(n, device=DEV, seed=seed, torso=torso, **usim.default_robosuite_kwargs())


def _teacher(usim, pins, n=N):
    meta = json.loads((ROOT / "tests/golden/reference_pins.json").read_text())["tracking"]
    sd = {k: torch.from_numpy(v) for k, v in np.load(ROOT / "tests/golden/tracking_policy.npz").items()}
    stats = {"obs_mean": pins["tracking_obs_rms_mean"], "obs_var": pins["tracking_obs_rms_var"], "count": meta["obs_rms_count"],
             "ret_mean": meta["ret_rms_mean"], "ret_var": meta["ret_rms_var"], "clip_obs": meta["clip_obs"], "clip_reward": meta["clip_reward"],
             "gamma": meta["gamma"], "epsilon": meta["epsilon"]}
    policy = usim.policy.MlpActorCritic.from_sb3_state_dict(sd).to(DEV)
    return policy, usim.policy.DeviceVecNormalize.from_stats(stats, n, device=DEV, training=False, norm_reward=False)


def _student(usim, A, seed=0):
    torch.manual_seed(seed)
    policy = usim.policy.MlpActorCritic(19, A).to(DEV)
    for m in policy.modules():                                             # SB3's initialisation, as tools/ppo_demo.py
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.orthogonal_(m.weight, gain=2 ** 0.5); torch.nn.init.zeros_(m.bias)
    torch.nn.init.orthogonal_(policy.action_net.weight, gain=0.01); torch.nn.init.orthogonal_(policy.value_net.weight, gain=1.0)
    return policy


def _tap(env, trainer):
    """record what reaches the environment and what the student proposed: (visited observations, actions stepped, student actions) as lists of clones"""
    visited, stepped, proposed = [], [], []
    step, student = env.step_tensor, trainer.student_action

    def step_tensor(a, auto_reset=True):
        visited.append(env._obs.clone()); stepped.append(a.clone())
        return step(a, auto_reset)

    def student_action(obs):
        proposed.append(student(obs).clone())
        return proposed[-1]

    env.step_tensor, trainer.student_action = step_tensor, student_action
    return visited, stepped, proposed


@pytest.fixture(scope="module")
def run(usim, pins):
    """the two rounds, with what the tests below look at"""
    im = usim.imitation
    env = _env(usim)
    teacher, teacher_vn = _teacher(usim, pins)
    expert = im.PolicyExpert(teacher, teacher_vn, env.action_space.low, env.action_space.high)
    vn = usim.policy.DeviceVecNormalize.from_stats(teacher_vn.stats(), N, device=DEV, training=False)
    demos = im.DemoBuffer(ROUNDS * N * T, env.action_dim, DEV)
    learner = im.NativeBC(_student(usim, env.action_dim), vn, demos, learning_rate=1e-3, n_epochs=8, batch_size=128, seed=5)
    trainer = im.DAggerTrainer(env, expert, learner, rollout_steps=T, seed=5)
    visited, stepped, proposed = _tap(env, trainer)
    rows, firsts = [], []
    for _ in range(ROUNDS):
        trainer.round()
        rows.append(demos.rows); firsts.append(dict(learner.first_minibatch))
    torch.cuda.synchronize()
    yield dict(env=env, expert=expert, learner=learner, trainer=trainer, demos=demos, visited=torch.stack(visited), stepped=torch.stack(stepped),
               proposed=proposed, rows=rows, firsts=firsts)
    env.close()


def test_the_buffer_holds_every_visited_observation_in_step_major_order(run):
    demos = run["demos"]
    assert run["rows"] == [N * T, 2 * N * T] and demos.rows == 2 * N * T and demos.has_value is True
    obs, act, value = demos.ordered()
    assert tuple(obs.shape) == (2 * N * T, 19) and tuple(act.shape) == (2 * N * T, run["env"].action_dim) and tuple(value.shape) == (2 * N * T,)
    assert torch.equal(_i32(obs.view(ROUNDS * T, N, 19)), _i32(run["visited"]))          # row (step, env): step-major, environment-minor, round after round


def test_every_stored_label_is_the_experts(run):
    obs, act, value = run["demos"].ordered()
    A = run["env"].action_dim
    for t in range(ROUNDS * T):                                            # the same function on the same 32 rows: the same bits
        a, v = run["expert"].label(obs[t * N:(t + 1) * N])
        assert torch.equal(_i32(a), _i32(act[t * N:(t + 1) * N])) and torch.equal(_i32(v), _i32(value[t * N:(t + 1) * N])), t
    low, high = (torch.as_tensor(x, device=DEV) for x in (run["env"].action_space.low, run["env"].action_space.high))
    assert bool((act >= low).all()) and bool((act <= high).all()) and float(act.abs().max()) > 0
    assert tuple(act.shape) == (ROUNDS * N * T, A)


def test_with_beta_one_the_expert_drives(usim, pins, run):
    obs, act, _ = run["demos"].ordered()
    assert torch.equal(_i32(run["stepped"][:T]), _i32(act[:N * T].view(T, N, -1)))       # round 0: the labels themselves reached the environment
    env = _env(usim)                                                       # the expert alone, same seed, same reset
    teacher, teacher_vn = _teacher(usim, pins)
    expert = usim.PolicyExpert(teacher, teacher_vn, env.action_space.low, env.action_space.high)
    o, seen = env.reset_tensor(), []
    for _ in range(T):
        seen.append(o.clone())
        o, _, _ = env.step_tensor(expert.label(seen[-1])[0])
    assert torch.equal(_i32(torch.stack(seen)), _i32(obs[:N * T].view(T, N, 19)))
    env.close()
    assert run["trainer"].history[0]["dagger/expert_share"] == 1.0 and run["trainer"].history[0]["dagger/beta"] == 1.0


def test_with_beta_zero_no_expert_action_reaches_the_environment(run):
    _, act, _ = run["demos"].ordered()
    stepped, labels = run["stepped"][T:], act[N * T:].view(T, N, -1)
    assert len(run["proposed"]) == T                                       # the student was asked in round 1 only
    assert torch.equal(_i32(stepped), _i32(torch.stack(run["proposed"])))  # what reached the environment is what the student proposed
    assert bool((stepped != labels).any(dim=2).all())                      # and in no environment at no step the expert's label
    assert run["trainer"].history[1]["dagger/expert_share"] == 0.0 and run["trainer"].history[1]["dagger/beta"] == 0.0


def test_the_action_error_falls_and_the_history_is_as_specified(usim, run):
    im, hist = usim.imitation, run["trainer"].history
    first, last = run["firsts"][0]["bc/action_mse"], hist[-1]["bc/action_mse"]
    print(f"bc/action_mse: first minibatch of round 0 {first:.6f}, last minibatch of round 1 {last:.6f}")
    assert last < first
    assert len(hist) == ROUNDS and all(tuple(row) == im.STAT_NAMES + im.ROUND_NAMES for row in hist)
    assert [row["dagger/round"] for row in hist] == [0, 1] and [row["dagger/rows"] for row in hist] == [N * T, 2 * N * T]
    assert [row["bc/optimizer_steps"] for row in hist] == [8 * 4, 8 * 8]  # 512 and 1024 rows in minibatches of 128, eight passes
    assert run["learner"].history == [{k: row[k] for k in im.STAT_NAMES} for row in hist]
    assert all(np.isfinite(v) for row in hist for v in row.values()) and hist[-1]["bc/value_loss"] > 0
    assert int(run["learner"].step_count.item()) == 96


# ================================================================ the planner as the expert ================================================================
G, K, H, STEPS = 4, 16, 4, 3


def _planner(usim):
    real, sim = _env(usim, G, torso="soft"), _env(usim, G * K, torso="soft", seed=5)
    real.reset_tensor(); sim.reset_tensor()
    return real, sim, usim.planner.MPPIPlanner(real, sim, horizon=H, sigma=0.3, temperature=0.5, seed=17)


def test_planner_expert_labels_with_the_plans_first_actions(usim):
    im = usim.imitation
    real, sim, pl = _planner(usim)
    expert = im.PlannerExpert(pl)
    demos = im.DemoBuffer(G * STEPS, real.action_dim, DEV)
    vn = usim.policy.DeviceVecNormalize(G, 19, device=DEV, training=False)
    learner = im.NativeBC(_student(usim, real.action_dim), vn, demos, loss="mse")
    with pytest.raises(ValueError, match="must be that environment"):
        im.DAggerTrainer(sim, expert, learner, rollout_steps=STEPS)            # a second environment is refused
    trainer = im.DAggerTrainer(real, expert, learner, rollout_steps=STEPS)
    visited, stepped, _ = _tap(real, trainer)
    row = trainer.round()
    obs, act, value = demos.ordered()
    assert demos.rows == G * STEPS and demos.has_value is False and value is None and row["bc/value_loss"] == 0.0 and row["dagger/expert_share"] == 1.0
    assert torch.equal(_i32(obs.view(STEPS, G, 19)), _i32(torch.stack(visited))) and torch.equal(_i32(act.view(STEPS, G, -1)), _i32(torch.stack(stepped)))
    # the planner driving its own pair of environments from the same seeds: planner.step() = plan(), real.step_tensor(first action), restart flags
    real2, sim2, pl2 = _planner(usim)
    real2.reset_tensor()                                                   # (the trainer's first round resets its environment once more)
    seen, acted = [], []
    for _ in range(STEPS):
        seen.append(real2._obs.clone())
        pl2.step()
        acted.append(pl2.action.clone())
    assert torch.equal(_i32(torch.stack(acted)), _i32(act.view(STEPS, G, -1)))           # the labels are plan()'s first actions
    assert torch.equal(_i32(torch.stack(seen)), _i32(obs.view(STEPS, G, 19)))            # and the trainer stepped planner.real with them
    assert torch.equal(pl.restart, pl2.restart) and int(pl.noise_counter.item()) == int(pl2.noise_counter.item()) == STEPS
    assert float(act.abs().max()) > 0
    for e in (real, sim, real2, sim2):
        e.close()
