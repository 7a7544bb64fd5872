#!/usr/bin/env python
"""What a policy step costs with K networks in it (profiles/population/cost.txt): n environments split into K members of n / K, timed as
  multi    one usim_policy_step_multi
  slices   K usim_policy_step launches on the members' slices (what a population cost before)
  single   one usim_policy_step over all n with ONE network -- with --parent-lib also the same call through a library built from the parent commit, and the
           two libraries' outputs compared word for word on the same inputs
Every variant is recorded as a HIP graph of `--steps` policy steps (statistics frozen: training = 0, sampled actions, all buffer outputs written) and replayed;
a figure is the replay's device time (events) over the steps.  The variants alternate within a round; the table gives the median over the rounds and the
spread (min .. max).  Needs a GPU.

    python tools/population_cost.py --n 4096 --members 1 4 32 128 --parent-lib /path/to/parent/libusim.so"""
import argparse
import ctypes as C
import importlib
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
usim = importlib.import_module("robotic-ultrasound-imaging_amd")
L = usim._lib
DEV = torch.device("cuda:0")
A = 6


def bind(path):
    lib = C.CDLL(str(path))
    for name in ("usim_policy_step", "usim_policy_pack", "usim_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SYMBOLS[name]
    return lib


class Problem:
    def __init__(self, lib, n, K):
        self.lib, self.n, self.K, self.G = lib, n, K, n // K
        g = torch.Generator().manual_seed(7)
        self.P = usim.learner.ppo_params(A)
        self.stride = (self.P + 3) // 4 * 4
        self.sizes = [s[0] * (s[1] if len(s) > 1 else 1) for s in usim.learner._field_shapes(A)]
        self.theta = (0.1 * torch.randn(K, self.stride, generator=g)).to(DEV)
        self.packed = torch.zeros(K, L.POLICY_PACKED, device=DEV)
        d = lambda t: t.to(device=DEV, dtype=torch.float64)
        self.st = [d(0.1 * torch.randn(K, 19, generator=g)), d(0.5 + torch.rand(K, 19, generator=g)), d(torch.full((K,), 100.0)), d(torch.zeros(K)), d(torch.ones(K)),
                   d(torch.full((K,), 100.0)), d(torch.zeros(n)), torch.zeros(K * L.POLICY_SCRATCH, dtype=torch.float64, device=DEV)]
        self.obs = torch.randn(n, 19, generator=g).to(DEV)
        self.done = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.low, self.high = torch.full((A,), -1.0, device=DEV), torch.full((A,), 1.0, device=DEV)
        self.out = [torch.zeros(n * w, device=DEV) for w in (A, 19, A, 1, 1, 1)]
        self.widths = (A, 19, A, 1, 1, 1)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def stats(self, k=0):
        off = (19, 19, 1, 1, 1, 1, self.G, L.POLICY_SCRATCH)
        return L.UsimNormStats(*[t.data_ptr() + 8 * k * o for t, o in zip(self.st, off)], 10.0, 10.0, 0.99, 1e-8)

    def policy_out(self, k=0):
        return L.UsimPolicyOut(*[t.data_ptr() + 4 * k * self.G * w for t, w in zip(self.out, self.widths)])

    def net(self, k):
        base, ptrs = self.theta.data_ptr() + 4 * k * self.stride, []
        for s in self.sizes:
            ptrs.append(base)
            base += 4 * s
        return L.UsimPolicyNet(*ptrs, self.packed.data_ptr() + 4 * k * L.POLICY_PACKED)

    def pack(self):
        assert self.lib.usim_policy_pack_multi(self.theta.data_ptr(), self.stride, self.K, A, self.packed.data_ptr(), self.stream()) == 0

    def multi(self, counter):
        S, o = self.stats(), self.policy_out()
        assert self.lib.usim_policy_step_multi(self.theta.data_ptr(), self.stride, self.packed.data_ptr(), C.byref(S), self.obs.data_ptr(), self.done.data_ptr(), self.K, self.G, A,
                                               self.low.data_ptr(), self.high.data_ptr(), 1, counter, None, 0, 0, 0, C.byref(o), self.stream()) == 0

    def slices(self, counter, lib=None, members=None, n=None):
        lib, G = lib or self.lib, n or self.G
        for k in range(self.K if members is None else members):
            net, S, o = self.net(k), self.stats(k), self.policy_out(k)
            assert lib.usim_policy_step(C.byref(net), C.byref(S), self.obs.data_ptr() + 4 * 19 * k * self.G, self.done.data_ptr() + k * self.G, G, A, self.low.data_ptr(),
                                        self.high.data_ptr(), 1, counter, None, k * self.G, 0, 0, C.byref(o), self.stream()) == 0

    def single(self, counter, lib=None):
        """ONE network (member 0's) over all n environments: the single-network launch as it was before populations"""
        self.slices(counter, lib, members=1, n=self.n)


def graph_of(fn, steps):
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fn(0)
        torch.cuda.current_stream(DEV).synchronize()
        with torch.cuda.graph(g, stream=side):
            for t in range(steps):
                fn(t)
    torch.cuda.current_stream(DEV).wait_stream(side)
    return g


def time_replays(graphs, steps, rounds, warmup):
    """graphs: {name: (graph, steps in it)} -> {name: [us per policy step, one figure per round]}, the variants alternating within a round"""
    for g, _ in graphs.values():
        for _ in range(warmup):
            g.replay()
    torch.cuda.synchronize()
    out = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, (g, s) in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / s)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 4, 32, 128])
    ap.add_argument("--steps", type=int, default=200, help="policy steps per graph (the K-slice graph holds min(steps, 4096 / K) so that it stays a few thousand nodes)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("population_cost.py measures on a GPU; there is none")
    lib = L.load()
    parent = bind(a.parent_lib) if a.parent_lib else None
    print(f"# {torch.cuda.get_device_name(0)}; library {lib.usim_version().decode()}" + (f"; parent {parent.usim_version().decode()}" if parent else "; parent: not given"))
    print(f"# n = {a.n}, act_dim {A}, training 0, sampled; us per policy step: median [min .. max] over {a.rounds} rounds of one graph replay each ({a.steps} steps per graph)")
    for K in a.members:
        if a.n % K:
            raise SystemExit(f"n {a.n} is not a multiple of K {K}")
        p = Problem(lib, a.n, K)
        p.pack()
        ss = max(1, min(a.steps, 4096 // K))
        graphs = {"multi": (graph_of(p.multi, a.steps), a.steps), "slices": (graph_of(p.slices, ss), ss), "single": (graph_of(p.single, a.steps), a.steps)}
        if parent is not None:
            graphs["single(parent)"] = (graph_of(lambda t: p.single(t, parent), a.steps), a.steps)
            p.single(5, lib); torch.cuda.synchronize(); mine = [t.clone() for t in p.out]
            for t in p.out:
                t.zero_()
            p.single(5, parent); torch.cuda.synchronize()
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(mine, p.out))
            print(f"# K = {K}: single-network outputs of the two libraries on the same inputs: {'bit-equal' if same else 'DIFFERENT'}")
        res = time_replays(graphs, a.steps, a.rounds, a.warmup)
        for name, v in res.items():
            print(f"K = {K:4d}  G = {p.G:5d}  {name:15s} {statistics.median(v):9.2f}  [{min(v):8.2f} .. {max(v):8.2f}]")
        del graphs, p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
