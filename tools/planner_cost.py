"""What a planning step of planner.MPPIPlanner costs: 16 controlled soft-torso environments, 256 candidates each (4096 simulated environments), horizons 16 and
64.  Every figure is the median of event-bracketed repeats on the current stream, in us:
  - plan() eager (six launches and the counter advance, issued from Python) and a recorded step() replayed as one graph (plan + the real step + both bank refills)
  - the two planner kernels alone, usim_plan_sample and usim_plan_update, next to a torch restatement of the same work (randn, the clamp, softmax, einsum, roll)
    on the same buffers -- what a user without the kernels would write between the simulator launches
  - the rest of a plan: save_envs + load_envs, rollout_actions, score_block
Then, not a time: the mean reward per step of a closed loop of planner steps next to the same environments (same seed) driven with zero actions.

usage: python tools/planner_cost.py [--out FILE] [--repeats 30] [--warmup 5] [--groups 16] [--per-group 256] [--loop-steps 300]"""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--groups", type=int, default=16)
ap.add_argument("--per-group", type=int, default=256)
ap.add_argument("--loop-steps", type=int, default=300)
ap.add_argument("--sigma", type=float, default=0.3)
ap.add_argument("--temperature", type=float, default=0.05)
args = ap.parse_args()
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

usim = importlib.import_module("robotic-ultrasound-imaging_amd")
if not torch.cuda.is_available():
    raise SystemExit("planner_cost.py needs the GPU: a time taken without one says nothing")

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(body, setup=lambda: None):
    """median / fastest / slowest event time of body() in us; setup() runs before every repeat, outside the events"""
    out = []
    for r in range(args.warmup + args.repeats):
        setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); body(); e1.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out), min(out), max(out)


def row(name, res):
    say(f"    {name:72s} {res[0]:9.1f}   ({res[1]:8.1f} .. {res[2]:8.1f})")


G, K = args.groups, args.per_group
n = G * K
kw = usim.default_robosuite_kwargs()
say(f"{usim._lib.load().usim_version().decode()}  {torch.cuda.get_device_name(0)}")
say(f"real {G} environments, sim {G} x {K} = {n}, soft torso; sigma {args.sigma}, temperature {args.temperature}; {args.repeats} repeats after {args.warmup}; "
    f"us: median (fastest .. slowest)")
real = usim.UltrasoundVecEnv(G, device="cuda:0", seed=3, torso="soft", **kw)
sim = usim.UltrasoundVecEnv(n, device="cuda:0", seed=4, torso="soft", **kw)
dev = real.device
for H in (16, 64):
    real.reset_tensor(); sim.reset_tensor()
    pl = usim.planner.MPPIPlanner(real, sim, horizon=H, sigma=args.sigma, temperature=args.temperature, seed=1)
    for _ in range(20):
        pl.step()
    A = pl.action_dim
    say(f"H = {H}")
    row("plan(), eager", timed(pl.plan))
    row("  usim_plan_sample", timed(pl.sample))
    row("  usim_plan_update", timed(pl.update))
    row("  save_envs + load_envs", timed(lambda: sim.load_envs(real.save_envs(out=pl._snap), pl._rows)))
    row("  rollout_actions", timed(lambda: sim.rollout_actions(pl.candidates, pl._block)))
    row("  score_block", timed(lambda: sim.score_block(pl._block, gamma=pl.gamma, out=(pl.returns, pl.lengths))))

    # ---- the torch restatement of sampler + update on the same buffers (no smoothing, no restart flags: the least it has to do)
    low, high, sigma = pl._low, pl._high, pl.sigma
    mean_t = pl.mean.clone()
    cand_t = torch.empty_like(pl.candidates)
    keep = torch.ones((1, 1, K, 1), device=dev)
    keep[:, :, 0] = 0                                                      # candidate 0 is the nominal

    def torch_sample():
        noise = torch.randn((H, G, K, A), device=dev) * keep
        c = (mean_t.transpose(0, 1).unsqueeze(2) + sigma * noise).clamp(low, high)
        cand_t.copy_(c.reshape(H, n, A))

    def torch_update():
        r = pl.returns.view(G, K)
        w = torch.softmax(torch.where(torch.isfinite(r), r, torch.full_like(r, -torch.inf)) / args.temperature, dim=1)
        plan = torch.einsum("gk,hgka->gha", w, cand_t.view(H, G, K, A)).clamp(low, high)
        mean_t.copy_(torch.roll(plan, -1, dims=1))
        mean_t[:, -1] = plan[:, -1]
        return plan[:, 0]

    ks = timed(lambda: (pl.sample(), pl.update()))
    ts = timed(lambda: (torch_sample(), torch_update()))
    row("usim_plan_sample + usim_plan_update (two launches)", ks)
    row("torch restatement of both (randn, clamp, softmax, einsum, roll)", ts)
    say(f"    the two kernels take {ks[0] / ts[0]:.2f} x the time of the torch restatement" + ("" if ks[0] < ts[0] else "  -- they do NOT beat it"))
    w_ref =torch.softmax(pl.returns.view(G, K).double() / args.temperature, dim=1)
    plan_ref = torch.einsum("gk,hgka->gha", w_ref, pl.candidates.view(H, G, K, A).double()).clamp(low.double(), high.double())
    pl.update(shift=False)
    say(f"    largest |plan - float64 softmax / einsum of the same candidates and returns|: {float((pl.plan_actions.double() - plan_ref).abs().max()):.3g}")

    pl.record()
    row("step() replayed from its graph (plan + real step + 2 x 2 bank refills)", timed(pl.replay))
    torch.cuda.synchronize()
    del pl

# ---- closed loop: mean reward per step, planner against zero actions on the same environments (same seed, same episodes as long as none ends early)
H = 16
real.reset_tensor(); sim.reset_tensor()
twin = usim.UltrasoundVecEnv(G, device="cuda:0", seed=3, torso="soft", **kw)
twin.reset_tensor()
pl = usim.planner.MPPIPlanner(real, sim, horizon=H, sigma=args.sigma, temperature=args.temperature, seed=1)
zero = torch.zeros((G, pl.action_dim), device=dev)
tot = torch.zeros(2, dtype=torch.float64, device=dev)
ends = torch.zeros(2, dtype=torch.int64, device=dev)
for _ in range(args.loop_steps):
    _, rew, done = pl.step()
    tot[0] += rew.double().sum(); ends[0] += done.sum()
    _, rew, done = twin.step_tensor(zero)
    tot[1] += rew.double().sum(); ends[1] += done.sum()
torch.cuda.synchronize()
per = (tot / (args.loop_steps * G)).tolist()
say(f"closed loop, {args.loop_steps} steps x {G} environments, H = {H}, K = {K} (not a time; recorded, not asserted):")
say(f"    mean reward per step: planner {per[0]:.5f} ({int(ends[0])} episode ends), zero actions {per[1]:.5f} ({int(ends[1])} episode ends)")
for e in (real, sim, twin):
    e.close()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
