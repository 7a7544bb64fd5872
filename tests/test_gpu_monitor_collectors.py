"""A monitor attached to the env (UltrasoundVecEnv.attach_monitor) is fed by everything that steps through step_tensor: the three device collectors -- the fused
one recorded as a graph and eager, and GraphedCollector -- and the SB3 numpy path.  64 environments, rigid torso, horizon 8 without early termination, a 16-step
buffer: every episode lasts exactly 8 steps and ends at the time limit, so the counts are known in advance.  The monitor does not touch the rollout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T, HORIZON = 64, 16, 8
KINDS = ["fused_graph", "fused_eager", "graphed"]
BUFFERS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


def _env(usim, horizon, seed=3):
    kw = usim.default_robosuite_kwargs()
    kw["horizon"], kw["early_termination"] = horizon, False
    return usim.UltrasoundVecEnv(N, device=DEV, seed=seed, torso="rigid", **kw)


def _collect_twice(usim, kind, monitored):
    """-> dict: the monitor (or None), its block, the buffer after the second collect(), and the episode ends counted from the buffer per rollout"""
    pol = usim.policy
    env = _env(usim, HORIZON)
    torch.manual_seed(0)
    policy = pol.MlpActorCritic(19, env.action_dim).to(env.device)
    vn = pol.DeviceVecNormalize(N, 19, device=env.device, training=True, norm_reward=True)
    buf = pol.DeviceRolloutBuffer(T, N, 19, env.action_dim, device=env.device)
    mon = env.attach_monitor(usim.DeviceMonitor(env)) if monitored else None          # before the collector is built
    if kind == "graphed":
        gen = torch.Generator(device=env.device); gen.manual_seed(0)
        coll = pol.GraphedCollector(env, policy, vn, buf, generator=gen)
    else:
        coll = pol.FusedRollout(env, policy, vn, buf, seed=0, graph=kind == "fused_graph")
    ends = []
    for _ in range(2):
        coll.collect()
        last = coll.last_done if kind == "graphed" else coll._prev_done
        ends.append(int(buf.episode_starts[1:].sum()) + int(last.bool().sum()))
    torch.cuda.synchronize()
    out = dict(mon=mon, attached=env.monitor, ends=ends, buffer={k: getattr(buf, k).clone() for k in BUFFERS},
               block=None if mon is None else mon.block.cpu().numpy().copy(), summary=None if mon is None else mon.summary(),
               episodes=None if mon is None else mon.episodes())
    env.close()
    return out


@pytest.fixture(scope="module")
def runs(usim):
    out = {(kind, True): _collect_twice(usim, kind, True) for kind in KINDS}
    out[("fused_graph", False)] = _collect_twice(usim, "fused_graph", False)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_every_collector_feeds_the_monitor(runs, kind):
    r = runs[(kind, True)]
    s, eps = r["summary"], r["episodes"]
    assert s["rollout/episodes"] == N * 2 * T // HORIZON == 256
    assert s["rollout/truncated"] == s["rollout/episodes"]                        # every episode ended at the time limit
    assert len(eps) == 100 and all(e["l"] == HORIZON for e in eps)                # the window of the last 100
    assert s["rollout/ep_len_mean"] == HORIZON == s["rollout/ep_len_mean_all"]
    assert s["rollout/episodes"] == sum(r["ends"]) and r["ends"] == [N * T // HORIZON] * 2          # counted independently from the buffer, per rollout
    assert s["rollout/ep_rew_mean"] == np.mean([np.float64(e["r"]) for e in eps]) and np.isfinite(s["rollout/ep_rew_mean_all"])
    assert [e["env"] for e in eps[-N:]] == list(range(N))                         # one launch's episodes in ascending environment index


def test_graphed_and_eager_fused_collectors_leave_the_same_block(runs):
    a, b = runs[("fused_graph", True)], runs[("fused_eager", True)]
    np.testing.assert_array_equal(a["block"], b["block"])
    for k in BUFFERS:
        assert torch.equal(a["buffer"][k], b["buffer"][k]), k


def test_without_a_monitor_nothing_is_attached_and_the_rollout_is_the_same(runs):
    plain, monitored = runs[("fused_graph", False)], runs[("fused_graph", True)]
    assert plain["attached"] is None and monitored["attached"] is monitored["mon"]
    for k in BUFFERS:
        assert torch.equal(plain["buffer"][k], monitored["buffer"][k]), k         # the monitor does not touch the rollout
    assert plain["ends"] == monitored["ends"]


def test_numpy_path_feeds_the_same_monitor(usim):
    """a short deterministic action sequence once through step() -- info["episode"] -- and once through step_tensor on a second env with the same seed"""
    steps, horizon = 30, 12
    a_env, b_env = _env(usim, horizon), _env(usim, horizon)
    mon_a = a_env.attach_monitor(usim.DeviceMonitor(a_env, window=1000))          # the numpy path steps through step_tensor: it feeds a monitor as well
    mon_b = b_env.attach_monitor(usim.DeviceMonitor(b_env, window=1000))
    g = np.random.default_rng(5)
    low, high = a_env.action_space.low, a_env.action_space.high
    actions = (low + (high - low) * g.random((steps, N, a_env.action_dim))).astype(np.float32)
    a_env.reset(); b_env.reset_tensor()
    infos_eps = []
    for k in range(steps):
        _, _, done, infos = a_env.step(actions[k])
        infos_eps += [(infos[i]["episode"]["r"], infos[i]["episode"]["l"], i, k) for i in range(N) if done[i]]
        b_env.step_tensor(torch.from_numpy(actions[k]).to(DEV))
    assert len(infos_eps) == N * (steps // horizon) and all(l == horizon for _, l, _, _ in infos_eps)
    for mon in (mon_a, mon_b):
        assert [(e["r"], e["l"], e["env"], e["step"]) for e in mon.episodes()] == infos_eps
        assert mon.summary()["rollout/episodes"] == len(infos_eps)
    assert a_env.detach_monitor() is mon_a and a_env.monitor is None and a_env.detach_monitor() is None
    with pytest.raises(ValueError):
        a_env.attach_monitor(mon_b)                                               # a monitor of another env
    a_env.close(); b_env.close()
