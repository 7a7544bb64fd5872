"""What one behaviour-cloning minibatch step costs (imitation.NativeBC.minibatch_step: usim_bc_grad + usim_ppo_adam), at the minibatch of tools/ppo_demo.py --
one eighth of 4096 environments x 128 steps = 65536 rows drawn through an index list from 524288 -- against two other measurements in the same process:
  torch   the same step in PyTorch on a copy of the same policy: the gather, MlpActorCritic.evaluate_actions, the loss, backward, clip_grad_norm_ and
          torch.optim.Adam.step -- what a learner without usim_bc_grad would run, so it is the yardstick
  ppo     usim_ppo_grad + usim_ppo_adam on the same rows, for scale
The three are alternated inside every repeat; a repeat times `--inner` consecutive steps between two events on the current stream; the figures are per step, in
ms: the median over the repeats with the fastest and the slowest.  Seeded random data: the cost does not depend on the values.

usage: python tools/bc_cost.py [--out FILE] [--repeats 11] [--warmup 3] [--inner 10] [--envs 4096] [--steps 128]"""
import argparse
import copy
import ctypes as C
import importlib
import statistics
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=128)
args = ap.parse_args()
if args.repeats < 5:
    raise SystemExit("at least five repeats: the record states medians and spreads")
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

usim = importlib.import_module("robotic-ultrasound-imaging_amd")
if not torch.cuda.is_available():
    raise SystemExit("bc_cost.py needs the GPU: a time taken without one says nothing")
L, dev, A = usim._lib, torch.device("cuda:0"), 6
rows, batch = args.envs * args.steps, args.envs * args.steps // 8
g = torch.Generator(device=dev); g.manual_seed(0)
rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)
obs, act, value = rnd(rows, 19).clamp_(-10, 10), rnd(rows, A).mul_(0.3).clamp_(-1, 1), rnd(rows)
old_logp, adv = rnd(rows).mul_(0.1).sub_(5.0), rnd(rows)
index = torch.randperm(rows, device=dev, generator=g)[:batch].to(torch.int32).contiguous()
index64 = index.to(torch.int64)

torch.manual_seed(0)
policy = usim.policy.MlpActorCritic(19, A).to(dev)
for m in policy.modules():
    if isinstance(m, torch.nn.Linear):
        torch.nn.init.orthogonal_(m.weight, gain=2 ** 0.5); torch.nn.init.zeros_(m.bias)
torch.nn.init.orthogonal_(policy.action_net.weight, gain=0.01); torch.nn.init.orthogonal_(policy.value_net.weight, gain=1.0)
twin = copy.deepcopy(policy)                                              # the torch learner's copy, before the original is flattened
demos = usim.DemoBuffer(8, A, dev)                                        # (minibatch_step takes its rows as arguments; the buffer only names the shapes)
vn = usim.policy.DeviceVecNormalize(1, 19, device=dev, training=False)
variants = {}
for loss in ("nll", "mse"):
    bc = usim.NativeBC(copy.deepcopy(policy), vn, demos, loss=loss)
    variants[f"native {loss}, value targets"] = lambda bc=bc: bc.minibatch_step((obs, act, value), index, batch)
    variants[f"native {loss}, no value term"] = lambda bc=bc: bc.minibatch_step((obs, act), index, batch)

opt = torch.optim.Adam(twin.parameters(), lr=3e-4, eps=1e-5)


def torch_step(valued=True):
    o, a = obs[index64], act[index64]
    values, logp, ent = twin.evaluate_actions(o, a)
    loss = -logp.mean() - 1e-3 * ent.mean()
    if valued:
        loss = loss + 0.5 * torch.nn.functional.mse_loss(values, value[index64])
    opt.zero_grad(); loss.backward(); torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.5); opt.step()


variants["torch nll, value targets"] = torch_step
variants["torch nll, no value term"] = lambda: torch_step(False)

ref = usim.NativeBC(copy.deepcopy(policy), vn, demos)                     # its flat block, moments and workspace serve the PPO pair
pb = L.UsimPpoBatch(obs.data_ptr(), act.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), value.data_ptr(), index.data_ptr(), rows, batch, A, 1, 0.2, 0.0, 0.5, 0.0)


def ppo_step():
    s = ref._stream()
    L.check(ref.lib, ref.lib.usim_ppo_grad(C.byref(ref._net), C.byref(pb), ref._work.data_ptr(), ref.grad.data_ptr(), ref.stats.data_ptr(), s))
    ref.adam_step(3e-4)                                                   # (NativeBC's defaults: eps 1e-5, max_grad_norm 0.5)


variants["usim_ppo_grad + usim_ppo_adam"] = ppo_step

times = {k: [] for k in variants}
for r in range(args.warmup + args.repeats):
    for name, body in variants.items():                                   # alternated: every repeat visits every variant
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            body()
        e1.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            times[name].append(e0.elapsed_time(e1) / args.inner)
lines = [f"{ref.lib.usim_version().decode()}  {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
         f"one minibatch step, {batch} rows through an index list from {rows}, act_dim {A}; {args.repeats} repeats of {args.inner} steps after {args.warmup}, alternated; "
         f"ms per step: median (fastest .. slowest)"]
for name, t in times.items():
    lines.append(f"    {name:36s} {statistics.median(t):8.3f}   ({min(t):7.3f} .. {max(t):7.3f})")
med = {k: statistics.median(t) for k, t in times.items()}
for kind in ("value targets", "no value term"):
    lines.append(f"    torch / native nll, {kind}: {med['torch nll, ' + kind] / med['native nll, ' + kind]:.2f}")
print("\n".join(lines))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
