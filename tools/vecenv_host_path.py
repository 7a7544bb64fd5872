"""What stable-baselines3 sees around the step kernel: the numpy path of UltrasoundVecEnv (step_async + step_wait, numpy actions in, numpy arrays and the
infos list out) timed against the tensor path (step_tensor + one torch.cuda.synchronize() per step), soft torso, shipped configuration.

Only the public step_async / step_wait / step_tensor are used, so the same file times any version of the package: --root names the checkout to import
(default: the one this file lies in).  To compare two versions, run them alternately in one session on one machine and take the larger of the two spreads
as the margin.

Per path and size: `warmup` untimed steps, then `repeats` windows of `steps` steps, host clock around each window (every step of both paths ends with the
host waiting for the device, so the window contains finished work only).  Reported: the median window in us per step and env-steps/s, the fastest and
slowest window, and spread = (slowest - fastest) / median.  The actions come from a pool drawn before the clock starts.

usage: python tools/vecenv_host_path.py [--envs 4096 8192] [--steps 1000] [--repeats 7] [--warmup 200] [--label TEXT] [--root DIR]"""
import argparse
import importlib
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 8192])
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--label", default="", help="printed with every line (e.g. the commit the checkout is at)")
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="checkout whose package is imported")
args = ap.parse_args()
sys.path.insert(0, str(Path(args.root).resolve()))
import torch

usim = importlib.import_module("robotic-ultrasound-imaging_amd")
if not torch.cuda.is_available():
    raise SystemExit("vecenv_host_path.py needs the GPU: a host-path time taken without one says nothing")
POOL = 16


def windows(step, warmup, steps, repeats):
    for k in range(warmup):
        step(k)
    torch.cuda.synchronize()
    out = []
    for r in range(repeats):
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e6)
    return out


def report(path, n, us):
    med = statistics.median(us)
    print(f"{args.label:>12s} envs {n:5d}  {path:28s} median {med:8.1f} us/step  {n / med * 1e6:12.0f} env-steps/s   fastest {min(us):8.1f}  slowest {max(us):8.1f}  "
          f"spread {(max(us) - min(us)) / med * 100:5.1f} %  ({len(us)} windows of {args.steps} steps)", flush=True)
    return med


print(f"{args.label:>12s} {usim._lib.load().usim_version().decode()}  {torch.cuda.get_device_name(0)}  package {Path(usim.__file__).resolve().parent}", flush=True)
for n in args.envs:
    g = np.random.default_rng(0)
    env = usim.UltrasoundVecEnv(n, device="cuda:0", seed=3, torso="soft", **usim.default_robosuite_kwargs())
    lo, hi = env.action_space.low.astype(np.float32), env.action_space.high.astype(np.float32)
    pool_np = [(lo + (hi - lo) * g.random((n, env.action_dim), dtype=np.float32)).astype(np.float32) for _ in range(POOL)]
    pool_dev = [torch.from_numpy(a).to(env.device) for a in pool_np]
    ended = [0]

    def numpy_step(k):
        env.step_async(pool_np[k % POOL])
        _, _, done, _ = env.step_wait()
        ended[0] += int(done.sum())

    def tensor_step(k):
        env.step_tensor(pool_dev[k % POOL])
        torch.cuda.synchronize()

    env.reset()
    a = report("step_async + step_wait", n, windows(numpy_step, args.warmup, args.steps, args.repeats))
    env.reset()
    b = report("step_tensor + synchronize", n, windows(tensor_step, args.warmup, args.steps, args.repeats))
    print(f"{args.label:>12s} envs {n:5d}  numpy path / tensor path {a / b:6.2f}   episodes ended on the numpy path: {ended[0]} in {args.warmup + args.steps * args.repeats} steps", flush=True)
    env.close()
