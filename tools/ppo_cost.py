"""What a PPO update costs, native learner (ppo.NativePPO: usim_ppo_grad + usim_ppo_adam per minibatch) against the torch learner of tools/ppo_demo.py (autograd +
clip_grad_norm_ + torch.optim.Adam), both in this run on this device, on the same collected rollout: n environments x 128 steps, eight minibatches per epoch.
Every figure is the median of event-bracketed repeats on the current stream, in ms, with the fastest and slowest repeat:
  - one minibatch step (gather by index, loss, gradient, clip, Adam)
  - one update of four epochs (a randperm and eight minibatch steps each; the native one ends with the collector's pack() and the read of its statistics)
The two learners start from the same parameters and move their own copies; nothing is asserted but the comparison the record is for.

usage: python tools/ppo_cost.py [--out FILE] [--repeats 7] [--warmup 2] [--envs 2048 4096] [--steps 128]"""
import argparse
import importlib
import statistics
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--envs", type=int, nargs="+", default=[2048, 4096])
ap.add_argument("--steps", type=int, default=128)
args = ap.parse_args()
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

usim = importlib.import_module("robotic-ultrasound-imaging_amd")
pol, ppo = usim.policy, usim.ppo
if not torch.cuda.is_available():
    raise SystemExit("ppo_cost.py needs the GPU: a time taken without one says nothing")
if args.repeats < 5:
    raise SystemExit("at least five repeats: the record states medians and spreads")

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(body):
    """median / fastest / slowest event time of body() in ms"""
    out = []
    for r in range(args.warmup + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); body(); e1.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def row(name, res):
    say(f"    {name:64s} {res[0]:9.3f}   ({res[1]:8.3f} .. {res[2]:8.3f})")


def compare(what, nat, tor):
    gap, spreads = tor[0] - nat[0], (tor[2] - tor[1]) + (nat[2] - nat[1])
    say(f"    {what}: torch / native = {tor[0] / nat[0]:.2f}; the medians differ by {gap:.3f} ms, the two spreads together are {spreads:.3f} ms"
        + ("" if gap > spreads else "  -- the native learner is NOT faster by more than the spreads"))


say(f"{usim._lib.load().usim_version().decode()}  {torch.cuda.get_device_name(0)}")
say(f"{args.steps} steps, eight minibatches per epoch, {args.repeats} repeats after {args.warmup}; ms: median (fastest .. slowest)")
T = args.steps
for n in args.envs:
    env = usim.UltrasoundVecEnv(n, device="cuda:0", seed=3, **usim.default_robosuite_kwargs())
    dev = env.device
    torch.manual_seed(0)
    policy = pol.MlpActorCritic(19, env.action_dim).to(dev)
    for m in policy.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.orthogonal_(m.weight, gain=2 ** 0.5); torch.nn.init.zeros_(m.bias)
    torch.nn.init.orthogonal_(policy.action_net.weight, gain=0.01); torch.nn.init.orthogonal_(policy.value_net.weight, gain=1.0)
    ppo.flatten_parameters(policy)
    twin = pol.MlpActorCritic(19, env.action_dim).to(dev)                  # the torch learner's own copy of the same parameters
    twin.load_state_dict(policy.state_dict())
    vn = pol.DeviceVecNormalize(n, 19, device=dev, training=True, norm_reward=True)
    buf = pol.DeviceRolloutBuffer(T, n, 19, env.action_dim, device=dev)
    coll = pol.FusedRollout(env, policy, vn, buf, seed=0)
    coll.collect()
    native = ppo.NativePPO(env, policy, vn, buf, coll, n_epochs=4, seed=0)
    opt = torch.optim.Adam(twin.parameters(), lr=3e-4, eps=1e-5)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    N, bs = n * T, n * T // 8
    data = tuple(native._flat(x) for x in (buf.observations, buf.actions, buf.log_probs, buf.advantages, buf.returns))
    index = torch.randperm(N, device=dev, generator=gen)[:bs].to(torch.int32)
    index64 = index.long()

    def torch_step(ob, ac, lp, adv, ret):
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        values, logp, ent = twin.evaluate_actions(ob, ac)
        ratio = torch.exp(logp - lp)
        pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 0.8, 1.2)).mean()
        vf = torch.nn.functional.mse_loss(values, ret)
        loss = pg + 0.5 * vf - 0.0 * ent.mean()
        opt.zero_grad(); loss.backward(); torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.5); opt.step()

    def torch_update():
        for epoch in range(4):
            for ob, ac, val, lp, adv, ret in buf.get(batch_size=bs, generator=gen):
                torch_step(ob, ac, lp, adv, ret)

    say(f"{n} environments x {T} steps = {N} samples, minibatch {bs}, {native.params} parameters")
    ns = timed(lambda: native.minibatch_step(data, index, bs))
    ts = timed(lambda: torch_step(*(x[index64] for x in data)))
    row("one minibatch step, native (usim_ppo_grad + usim_ppo_adam)", ns)
    row("one minibatch step, torch (autograd + clip_grad_norm_ + Adam)", ts)
    compare("minibatch step", ns, ts)
    nu = timed(native.update)
    tu = timed(torch_update)
    row("one update of four epochs, native", nu)
    row("one update of four epochs, torch", tu)
    compare("update", nu, tu)
    say(f"    last native statistics: " + ", ".join(f"{k.split('/')[1]} {v:.4g}" for k, v in native.update().items()))
    env.close()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
