"""What an attached monitor.DeviceMonitor costs, and what monitor.evaluate_policy costs against the loop it replaces.
usage: python tools/monitor_cost.py [n_envs] [n_steps] [repeats] [trace]
(a) FusedRollout.collect() without and with a monitor attached (before the collector was built: the launch is part of the recorded rollout), alternating in one
    process, on twin environments; the difference per step is the usim_monitor_step launch inside the graph.
(b) evaluate_policy against policy.policy_rollout(fused=True) -- the loop the README's replay numbers came from, whose episode sums use boolean-mask indexing
    (one host synchronisation per step) -- for the same number of env steps: an evaluation of n_envs episodes with horizon = n_steps and no early termination is
    exactly n_steps steps.
Prints median (fastest .. slowest) milliseconds; profiles/monitor/cost.txt."""
import importlib, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
usim = importlib.import_module("robotic-ultrasound-imaging_amd")
pol = importlib.import_module("robotic-ultrasound-imaging_amd.policy")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 128
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 15
fmt = lambda t: f"{statistics.median(t):8.3f}   ({min(t):8.3f} .. {max(t):8.3f})"


def make(monitored, **kw_over):
    torch.manual_seed(0)
    env = usim.UltrasoundVecEnv(n, device="cuda:0", seed=3, **dict(usim.default_robosuite_kwargs(), **kw_over))
    policy = pol.MlpActorCritic(19, env.action_dim).to(env.device)
    vn = pol.DeviceVecNormalize(n, 19, device=env.device, training=True, norm_reward=True)
    if monitored:
        env.attach_monitor(usim.DeviceMonitor(env))
    return env, policy, vn


print(f"{usim._lib.load().usim_version().decode()}  {torch.cuda.get_device_name(0)}")

if len(sys.argv) > 4 and sys.argv[4] == "trace":
    # for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/monitor_cost.py 4096 128 3 trace): the monitored collector alone, with the
    # three-launch step (fused_stats=False) so that usim_policy_reward -- the yardstick launch of the same loop -- is in the trace next to usim_monitor_step
    env, policy, vn = make(True)
    c = pol.FusedRollout(env, policy, vn, pol.DeviceRolloutBuffer(T, n, 19, env.action_dim, device=env.device), seed=0, fused_stats=False)
    for _ in range(repeats):
        c.collect()
    torch.cuda.synchronize()
    print(f"trace run: {repeats} x collect() of {n} x {T}, fused_stats False, monitor attached: {env.monitor.summary()['rollout/episodes']} episodes")
    env.close()
    sys.exit(0)

# ---- (a) the collector
colls = {}
for name in ("off", "on"):
    env, policy, vn = make(name == "on")
    colls[name] = pol.FusedRollout(env, policy, vn, pol.DeviceRolloutBuffer(T, n, 19, env.action_dim, device=env.device), seed=0)
print(f"(a) FusedRollout.collect(), {n} environments x {T} steps, fused_stats {colls['off'].fused_stats}; {repeats} repeats after 3; ms per collect(): median (fastest .. slowest)")
times = {name: [] for name in colls}
for rep in range(repeats + 3):
    for name, c in colls.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        c.collect()
        torch.cuda.synchronize()
        if rep >= 3:
            times[name].append((time.perf_counter() - t0) * 1e3)
for name, t in times.items():
    print(f"    monitor {name:3s}  {fmt(t)}   {n * T / statistics.median(t) / 1e3:7.1f} M env-steps/s")
d = statistics.median(times["on"]) - statistics.median(times["off"])
spread = (max(times["on"]) - min(times["on"])) + (max(times["off"]) - min(times["off"]))
print(f"    on - off: {d:+.3f} ms per collect() = {d / T * 1e3:+.2f} us per step; the two spreads together are {spread:.3f} ms")
s = colls["on"].env.monitor.summary()
print(f"    the monitor after {repeats + 3} rollouts: {s['rollout/episodes']} episodes, ep_rew_mean {s['rollout/ep_rew_mean']:.2f}, ep_len_mean {s['rollout/ep_len_mean']:.1f}")
for c in colls.values():
    c.env.close()

# ---- (b) evaluation: n episodes of exactly T steps each
env, policy, vn = make(False, horizon=T, early_termination=False)
vn.training = False
print(f"(b) {n} episodes of {T} steps (horizon {T}, no early termination) = {T} env steps of {n} environments; {repeats} repeats after 2; ms per call")
te, tr = [], []
for rep in range(repeats + 2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    mean, std = usim.evaluate_policy(env, policy, vn, n_eval_episodes=n)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    out = pol.policy_rollout(env, policy, vn, T, deterministic=True, fused=True)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    if rep >= 2:
        te.append((t1 - t0) * 1e3); tr.append((t2 - t1) * 1e3)
print(f"    evaluate_policy        {fmt(te)}   mean return {mean:.3f} +- {std:.3f}")
print(f"    policy_rollout(fused)  {fmt(tr)}   mean episode return {out['mean_episode_return']:.3f} over {out['episodes']:.0f} episodes")
env.close()
