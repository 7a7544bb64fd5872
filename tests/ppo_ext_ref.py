"""Float64 restatement of what clip_range_vf and target_kl add to the learner's minibatch step (csrc/usim_ppo.hip; include/usim.h states the contract), on top of
tests/ppo_ref.py, which it imports and does not copy: the networks, the backward pass and the absolute-value companion passes are ppo_ref's.

- loss_and_grad_vf: ppo_ref.loss_and_grad with SB3's clipped value term  Vp = old + clamp(V - old, -c, c),  value_loss = mean((ret - Vp)^2): a row with
  |V - old| <= c (the closed interval: torch's clamp passes its gradient there) is the unclipped row, gradient 2 vf_coef (V - ret) / B; any other row
  contributes ((old +- c) - ret)^2 to the loss and exactly nothing to the gradient
- grad_bounds_vf: the bound per gradient entry and per statistic, derived as ppo_ref.grad_bounds derives its own.  The policy network's entries keep their
  bound.  For the value network, inside-band rows keep ppo_ref's e_dV (the kernel uses V itself there: no new rounding); outside-band rows have an upstream
  gradient of exactly 0 on both sides, so e_dV = 0.  The loss row outside the band is three float32 roundings: vp = fl(old +- c) (u |vp|), dc = fl(vp - ret)
  (u |dc|, plus vp's error), fl(dc dc) -- and no forward-pass error at all, since V enters only through the side it is on.  As everywhere in ppo_ref the
  reference's decisions (here: which side of a band edge) are taken for the kernel's: make_problem_vf keeps every row EDGE_MARGIN from an edge, and
  grad_bounds_vf returns the largest bound on V - old so that a test can see it is far below that margin
- gate_rule: the stop flag as a pure function of the float32 approx_kl the call has written: float32 product 1.5f * target_kl, float32 compare
- make_problem_vf: ppo_ref.make_problem plus old_values with about a third of the rows below the band, a third inside, a third above"""
import numpy as np

import policy_ref as PR
import ppo_ref as R

EDGE_MARGIN = R.EDGE_MARGIN
# the cases of tests/test_gpu_ppo_vf_clip.py (A, batch, rows, index): a lone row, two, a tile edge, more tiles than workgroups, and one gather with repeats
CASES = [(A, batch, None, False) for A in (6, 7) for batch in (1, 2, 33, 32 * R.W + 5)] + [(7, 33, 99, True)]


def gate_rule(approx_kl, target_kl):
    """usim_ppo_grad's stop flag (0 or 1) from the float32 word stats[3] and the float32 target_kl"""
    kl, t = np.float32(approx_kl), np.float32(target_kl)
    return int(bool(t > np.float32(0) and kl > np.float32(1.5) * t))


def _vf_segment(A):
    """[lo, hi) of the value network's six fields in the flat block"""
    lo = 38016 + 129 * A
    return lo, R.n_params(A) - A


def loss_and_grad_vf(p, obs, act, old_logp, adv, ret, old_values, clip_range_vf, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, keep=False):
    """ppo_ref.loss_and_grad with the value term clipped around old_values; the same dictionary (keep=True: with `inside`, `vp`, `old_values`, `cvf`)"""
    out = R.loss_and_grad(p, obs, act, old_logp, adv, ret, clip_range, ent_coef, vf_coef, normalize_advantage, keep=True)
    c, old = R.f32(clip_range_vf), np.asarray(old_values, dtype=np.float64)
    V, ret64, x, B = out["V"], out["ret"], out["x"], len(out["V"])
    dvo = V - old
    inside = np.abs(dvo) <= c
    vp = np.where(inside, V, old + np.sign(dvo) * c)
    dV = np.where(inside, 2.0 * out["vf_coef"] * (V - ret64) / B, 0.0)
    gp, _ = R._back(out["pi"], x, out["dmean"])
    gv, iv = R._back(out["vf"], x, dV[:, None])
    grad = R._assemble(gp, gv, out["dls_rows"].sum(0) - out["ent_coef"])
    stats = out["stats"].copy()
    stats[1] = np.mean((ret64 - vp) ** 2)
    stats[5] = stats[0] + out["vf_coef"] * stats[1] + out["ent_coef"] * stats[2]
    stats[6] = np.sqrt((grad ** 2).sum())
    res = dict(out, grad=grad, stats=stats, dV=dV, iv=iv, inside=inside, vp=vp, old_values=old, cvf=c)
    if not keep:
        res = {k: res[k] for k in ("grad", "stats", "ratio", "adv", "inside")}
    return res


def grad_bounds_vf(p, obs, act, old_logp, adv, ret, old_values, clip_range_vf, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, u=R.UNITS):
    """-> (reference dict of loss_and_grad_vf with `e_dvo`, the bound on the kernel's V - old; bound per gradient entry; bound per statistic [7])"""
    _, e_grad0, e_stats0 = R.grad_bounds(p, obs, act, old_logp, adv, ret, clip_range, ent_coef, vf_coef, normalize_advantage, u)
    Rv = loss_and_grad_vf(p, obs, act, old_logp, adv, ret, old_values, clip_range_vf, clip_range, ent_coef, vf_coef, normalize_advantage, keep=True)
    a, uu, x = np.abs, u["u"], Rv["x"]
    B, A = Rv["act"].shape
    gd = R.gam(R.depth(B), uu)
    fv = R._fwd_bounds(Rv["vf"], x, u)
    e_V, inside = fv["e_out"][:, 0], Rv["inside"]
    # ---- d loss / d value: ppo_ref's e_dV inside the band, exactly zero outside ----
    dv = Rv["V"] - Rv["ret"]
    e_dv = e_V + uu * (a(dv) + e_V)
    k = 2.0 * Rv["vf_coef"] / B
    e_dV = np.where(inside, k * e_dv + 2.0 * uu * k * (a(dv) + e_dv), 0.0)
    ev = R._back_bounds(Rv["vf"], fv, Rv["iv"], x, Rv["dV"][:, None], e_dV[:, None], gd, u)
    lo, hi = _vf_segment(A)
    e_grad = e_grad0.copy()
    e_grad[lo:hi] = np.concatenate([ev["w1"].ravel(), ev["b1"], ev["w2"].ravel(), ev["b2"], ev["wh"].ravel(), ev["bh"]]) * R.SLACK
    # ---- the value-loss rows ----
    vp = Rv["vp"]
    dc = vp - Rv["ret"]
    e_dc_out = uu * a(vp) + uu * (a(dc) + uu * a(vp))                     # fl(old +- c), then fl(vp - ret)
    e_dc = np.where(inside, e_dv, e_dc_out)
    e_vl_rows = 2.0 * a(dc) * e_dc + e_dc ** 2 + uu * (a(dc) + e_dc) ** 2
    s = Rv["stats"]
    e_vl = e_vl_rows.mean() + uu * a(s[1])
    e_stats = e_stats0.copy()                                             # (policy_loss, entropy_loss, approx_kl, clip_fraction: untouched by the value term)
    f64 = u["f64"]
    e_stats[1] = e_vl * R.SLACK + f64 * (1.0 + a(s[1]))
    # e_stats0[0] and [2] are upper bounds of ppo_ref's e_pl and e_el (they carry SLACK and the float64 term already)
    e_stats[5] = (e_stats0[0] + Rv["vf_coef"] * e_vl + a(Rv["ent_coef"]) * e_stats0[2] + uu * a(s[5])) * R.SLACK + f64 * (1.0 + a(s[5]))
    e_stats[6] = (np.sqrt((e_grad ** 2).sum()) + uu * s[6]) * R.SLACK + f64 * (1.0 + a(s[6]))
    Rv["e_dvo"] = float((e_V + uu * (a(Rv["V"] - Rv["old_values"]) + e_V)).max())
    return Rv, e_grad, e_stats


def vf_margin(ref):
    """smallest distance of a row's |V - old| from the band edge, of a loss_and_grad_vf(keep=True) result"""
    return float(np.abs(np.abs(ref["V"] - ref["old_values"]) - ref["cvf"]).min())


def make_problem_vf(A, batch, seed, rows=None, index=False, clip_range=0.2, clip_range_vf=0.2):
    """ppo_ref.make_problem's dictionary with `old_values` [rows] float32 and `clip_range_vf`.  V - old is drawn from three bands -- below -c, inside, above c --
    each at least 0.01 from an edge; a draw in which a row of the buffer has ||V - old| - c| < EDGE_MARGIN after the rounding of old to float32 is drawn again
    (deterministically: the seed sequence is fixed)."""
    pr = R.make_problem(A, batch, seed, rows=rows, index=index, clip_range=clip_range)
    c = R.f32(clip_range_vf)
    _, V = PR.forward(pr["p"], pr["obs"])
    n = pr["rows"]
    for attempt in range(64):
        rng = np.random.default_rng([seed, attempt, 0x7666])
        band = rng.integers(0, 3, n)
        delta = np.where(band == 0, rng.uniform(-2 * c, -c - 0.01, n), np.where(band == 1, rng.uniform(-c + 0.01, c - 0.01, n), rng.uniform(c + 0.01, 2 * c, n)))
        old = (V - delta).astype(np.float32)
        if np.abs(np.abs(V - old.astype(np.float64)) - c).min() > EDGE_MARGIN:
            return dict(pr, old_values=old, clip_range_vf=clip_range_vf)
    raise RuntimeError("no draw without a row near a band edge")


def minibatch_vf(pr):
    """ppo_ref.minibatch's five arrays and the gathered old values"""
    sel = pr["index"] if pr["index"] is not None else np.arange(pr["batch"])
    return R.minibatch(pr) + (pr["old_values"][sel],)


def case_problem(A, batch, rows, index, clip_range_vf=0.2):
    """the make_problem_vf dictionary of one of CASES (its seed is a function of the case)"""
    return make_problem_vf(A, batch, seed=batch + A + (1000 if index else 0), rows=rows, index=index, clip_range_vf=clip_range_vf)
