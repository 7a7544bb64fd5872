"""What FusedRollout(bootstrap_truncation=True) costs: collect() with the option off and on, alternating in one process, on twin environments.
usage: python tools/bootstrap_cost.py [n_envs] [n_steps] [horizon] [repeats] [only]
horizon: the env's (default 1000, the shipped one: no truncation inside a short rollout; 1 with early termination off makes EVERY step of every
environment a truncation -- the all-truncated case); only: `off` or `on` runs one collector alone (for a kernel trace of its own).
Prints median (fastest .. slowest) milliseconds per collect() and the difference per step; profiles/truncation/cost.txt."""
import importlib, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
usim = importlib.import_module("robotic-ultrasound-imaging_amd")
pol = importlib.import_module("robotic-ultrasound-imaging_amd.policy")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 128
horizon = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 15
only = sys.argv[5] if len(sys.argv) > 5 else None
kw = usim.default_robosuite_kwargs()
kw["horizon"] = horizon
if horizon < 1000:
    kw["early_termination"] = False


def make(boot):
    torch.manual_seed(0)
    env = usim.UltrasoundVecEnv(n, device="cuda:0", seed=3, **kw)
    policy = pol.MlpActorCritic(19, env.action_dim).to(env.device)
    vn = pol.DeviceVecNormalize(n, 19, device=env.device, training=True, norm_reward=True)
    buf = pol.DeviceRolloutBuffer(T, n, 19, env.action_dim, device=env.device)
    return pol.FusedRollout(env, policy, vn, buf, seed=0, bootstrap_truncation=boot)


colls = {name: make(name == "on") for name in ("off", "on") if only in (None, name)}
print(f"{usim._lib.load().usim_version().decode()}  {torch.cuda.get_device_name(0)}")
print(f"{n} environments x {T} steps, horizon {horizon}, fused_stats {next(iter(colls.values())).fused_stats}; {repeats} repeats after 3; ms per collect(): median (fastest .. slowest)")
times = {name: [] for name in colls}
for rep in range(repeats + 3):
    for name, c in colls.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        c.collect()
        torch.cuda.synchronize()
        if rep >= 3:
            times[name].append((time.perf_counter() - t0) * 1e3)
for name, t in times.items():
    extra = f"   truncated env-steps of the last rollout: {int(colls[name].truncations)} of {n * T}" if name == "on" else ""
    print(f"    bootstrap_truncation {name:3s}  {statistics.median(t):8.3f}   ({min(t):8.3f} .. {max(t):8.3f})   {n * T / statistics.median(t) / 1e3:7.1f} M env-steps/s{extra}")
if len(times) == 2:
    d = statistics.median(times["on"]) - statistics.median(times["off"])
    spread = (max(times["on"]) - min(times["on"])) + (max(times["off"]) - min(times["off"]))
    print(f"    on - off: {d:+.3f} ms per collect() = {d / T * 1e3:+.2f} us per step; the two spreads together are {spread:.3f} ms")
for c in colls.values():
    c.env.close()
