#!/usr/bin/env python
"""What one PPO update of a population costs (profiles/population_learner/cost.txt): n environments split into K members of n / K, a rollout buffer of T steps
filled with synthetic samples (no simulator: the update does not care where its rows came from), `--epochs` epochs of `--minibatches` minibatches, timed as
  concurrent   PopulationPPO(concurrent=True).update(): one usim_ppo_grad_multi + one usim_ppo_adam_multi per minibatch for all K members
  sequential   PopulationPPO(concurrent=False).update(): K lone NativePPO.update() one after the other
  lone(parent) at K = 1 with --parent-lib: NativePPO.update() + the population's pack() with the learner's calls going through a library built from the parent
               commit -- the bar: the concurrent update at K = 1 may not be slower than this by more than the spread of these timings
Each figure is the device time (events) from the first launch of update() to the end of its host read; the variants alternate within a round; the table gives
the median over the rounds and the spread (min .. max).  All variants step the same parameters (the figures do not depend on their values).  Needs a GPU.

    python tools/population_learner_cost.py --n 4096 --members 1 4 32 128 --parent-lib /path/to/parent/libusim.so
    python tools/population_learner_cost.py --n 16384 --members 4                                                     # the demo's 4 x 4096 point"""
import argparse
import ctypes as C
import importlib
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
usim = importlib.import_module("robotic-ultrasound-imaging_amd")
L, P, M = usim._lib, usim.policy, usim.population
DEV = torch.device("cuda:0")
A = 6


def bind(path):
    lib = C.CDLL(str(path))
    for name in ("usim_ppo_grad", "usim_ppo_adam", "usim_ppo_adam_gated", "usim_explained_variance", "usim_ppo_work_floats", "usim_strerror", "usim_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SYMBOLS[name]
    return lib


def build(n, K, T, epochs, minibatches):
    """-> (the two PopulationPPO on the same population and buffer, the population)"""
    G = n // K
    box = SimpleNamespace(low=[-1.0] * A, high=[1.0] * A)
    env = SimpleNamespace(num_envs=n, action_dim=A, device=DEV, action_space=box, env_offset=0)
    torch.manual_seed(0)
    pop = M.PolicyPopulation(K, A, device=DEV)
    vn = M.PopulationVecNormalize(K, G, device=DEV)
    buf = P.DeviceRolloutBuffer(T, n, 19, A, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    buf.observations.copy_(r(T, n, 19)); buf.actions.copy_(0.5 * r(T, n, A)); buf.log_probs.copy_(-5.0 + 0.05 * r(T, n))
    buf.advantages.copy_(r(T, n)); buf.returns.copy_(r(T, n)); buf.values.copy_(r(T, n))
    buf.pos, buf.full = T, True
    coll = SimpleNamespace(pack=pop.pack)
    kw = dict(seeds=list(range(K)), n_epochs=epochs, batch_size=T * G // minibatches)
    return {c: M.PopulationPPO(env, pop, vn, buf, coll, concurrent=c, **kw) for c in (True, False)}, pop


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128, help="T: rollout steps in the buffer")
    ap.add_argument("--members", type=int, nargs="+", default=[1, 4, 32, 128])
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("population_learner_cost.py measures on a GPU; there is none")
    lib = L.load()
    parent = bind(a.parent_lib) if a.parent_lib else None
    print(f"# {torch.cuda.get_device_name(0)}; library {lib.usim_version().decode()}" + (f"; parent {parent.usim_version().decode()}" if parent else "; parent: not given"))
    print(f"# n = {a.n} environments, T = {a.steps}, act_dim {A}, {a.epochs} epochs x {a.minibatches} minibatches; ms per update(): median [min .. max] over {a.rounds} "
          f"rounds after {a.warmup} warm-up rounds, the variants alternating within a round")
    for K in a.members:
        if a.n % K or (a.steps * (a.n // K)) % a.minibatches:
            raise SystemExit(f"n {a.n} is not a multiple of K {K}, or a member's rollout not a multiple of {a.minibatches} minibatches")
        ppo, pop = build(a.n, K, a.steps, a.epochs, a.minibatches)
        variants = {"concurrent": ppo[True].update, "sequential": ppo[False].update}
        if parent is not None and K == 1:
            lone = ppo[False].learners[0]

            def lone_parent():
                lone.lib = parent
                try:
                    lone.update()
                    pop.pack()
                finally:
                    lone.lib = lib
            variants["lone(parent)"] = lone_parent
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        res = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                res[name].append(timed(fn))
        l0 = ppo[True].learners[0]
        print(f"K = {K:4d}  G = {a.n // K:5d}  rows per member {l0.rollout:7d}  minibatch {l0.batch_size:6d}  multi workspace {ppo[True]._work.numel() * 4 / 2 ** 20:8.1f} MiB "
              f"(lone workspaces of the sequential path: {K} x {l0._work.numel() * 4 / 2 ** 20:.1f} MiB)")
        for name, v in res.items():
            print(f"K = {K:4d}  {name:13s} {statistics.median(v):9.3f}  [{min(v):9.3f} .. {max(v):9.3f}]")
        med = {name: statistics.median(v) for name, v in res.items()}
        print(f"K = {K:4d}  sequential / concurrent = {med['sequential'] / med['concurrent']:.2f}")
        if "lone(parent)" in res:
            spread = max(res["lone(parent)"]) - min(res["lone(parent)"])
            over = med["concurrent"] - med["lone(parent)"]
            print(f"K =    1  the bar: concurrent - lone(parent) = {over:+.3f} ms against the parent's own spread of {spread:.3f} ms: {'PASS' if over <= spread else 'FAIL'}")
        finite = bool(torch.isfinite(pop.theta[:, :pop.params]).all())
        print(f"K = {K:4d}  parameters finite after the run: {finite}")
        del ppo, pop, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
