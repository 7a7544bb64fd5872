"""Plain float64 restatement of the learner's two entry points (csrc/usim_ppo.hip: usim_ppo_grad, usim_ppo_adam; include/usim.h states the contract): numpy
only, built on policy_ref.forward's networks, no torch and no library calls, so that it shares no rounding with what it checks.

- flatten / unflatten / n_params: the flat parameter block in the header's field order (policy_ref.PARAM_NAMES)
- loss_and_grad: the loss of stable-baselines3's PPO.train on one minibatch, its seven statistics and a manual backward pass through both networks
- grad_bounds: an error bound per gradient entry and per statistic for a kernel that rounds as the unit dictionary UNITS says -- the absolute-value companion
  pass of policy_ref.forward_bounds carried on through the loss and the backward pass: every quantity q travels with a bound e_q of |kernel - reference| and its
  magnitude Q = |q| + e_q; a product picks up sum_i e_i prod_{j != i} Q_j plus its own roundings, a sum of n fused multiply-adds gam(n) sum |terms|
- adam / adam_bounds: clip_grad_norm_ + torch.optim.Adam.step on the flat block
- make_problem: the test inputs shared by the CPU and GPU tests -- ratios on both sides of both clip edges, advantages of both signs, nothing near a kink

The units (nothing here is fitted to the kernel's output):
  u        2^-24    one rounding to float32: a fused multiply-add, an add, a product, the conversion of a float64 result
  gam(n)   min(n, 2 sqrt(n)) u / (1 - n u): a chain of n fused multiply-adds or adds, times the sum of the terms' magnitudes.  SQUARE-ROOT growth (Higham and
           Mary 2019, "A new approach to probabilistic rounding error analysis", with lambda = 2): the error of the chain is sum_i delta_i s_i over its partial
           sums s_i with independent roundings |delta_i| <= u of standard deviation u / sqrt(3); at worst (all terms of one sign and size) sqrt(sum s_i^2) =
           sum |terms| sqrt(n / 3), a standard deviation of sqrt(n) u sum |terms| / 3 -- the bar is then six of them, and many more for terms of mixed signs.
           Linear growth n u, which needs no such argument, is used where it is the smaller
  tanh     2^-22 absolute: tanh_ = 1 - 2 rcp(exp2(2 x log2 e) + 1), as tests/test_gpu_policy_kernels.py derives it for the forward kernel
  exp      2^-23 relative: expf of the device library, 1 ulp (HIP's table of device math functions)
  depth(B) terms in the longest chain of a sum over samples: the 32 rows of each of a workgroup's ceil(ceil(B / 32) / W) tiles in one accumulator, then the
           W partial blocks in block order
  f64      2^-49: the float64 parts (advantage statistics, loss sums, Adam's arithmetic) -- a few dozen float64 roundings, relative to the magnitudes involved
Second-order terms (products of two errors) are kept where they are written and otherwise covered by the factor SLACK = 1 + 1e-5 on every bound."""
import numpy as np

import policy_ref as PR

U = 2.0 ** -24
UNITS = dict(u=U, tanh=2.0 ** -22, exp=2.0 ** -23, f64=2.0 ** -49)
SLACK = 1.0 + 1e-5
LAMBDA = 2.0
W = 128                                        # USIM_PPO_WORKGROUPS
TILE = 32
FIELDS = PR.PARAM_NAMES
STAT_NAMES = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss", "grad_norm")
HALF_LOG_2PI = PR.LOG_SQRT_2PI


def shapes(A):
    return {"pi_w1": (256, 19), "pi_b1": (256,), "pi_w2": (128, 256), "pi_b2": (128,), "act_w": (A, 128), "act_b": (A,),
            "vf_w1": (256, 19), "vf_b1": (256,), "vf_w2": (128, 256), "vf_b2": (128,), "val_w": (1, 128), "val_b": (1,), "log_std": (A,)}


def n_params(A):
    return 76032 + 130 * A + 129


def flatten(p):
    return np.concatenate([np.asarray(p[k]).reshape(-1) for k in FIELDS])


def unflatten(theta, A):
    out, o = {}, 0
    for k, s in shapes(A).items():
        n = int(np.prod(s))
        out[k] = np.asarray(theta[o:o + n]).reshape(s)
        o += n
    assert o == len(theta) == n_params(A)
    return out


def f32(x):
    """a host float as the ABI carries it"""
    return float(np.float32(x))


def gam(n, u=U):
    return min(n, LAMBDA * np.sqrt(n)) * u / (1.0 - n * u)


def depth(B):
    return TILE * -(-(-(-B // TILE)) // W) + W


# ---------------------------------------------------------------- loss and gradient ----------------------------------------------------------------
def _net(p, net, x):
    (l1, l2), (wh, bh) = PR._layers(p, net)
    z1 = x @ l1[0].T + l1[1]
    h1 = np.tanh(z1)
    z2 = h1 @ l2[0].T + l2[1]
    h2 = np.tanh(z2)
    return dict(w1=l1[0], b1=l1[1], w2=l2[0], b2=l2[1], wh=wh, bh=bh, z1=z1, h1=h1, z2=z2, h2=h2, out=h2 @ wh.T + bh)


def _back(n, x, dout):
    g = {"wh": dout.T @ n["h2"], "bh": dout.sum(0)}
    dh2 = dout @ n["wh"]
    d2 = dh2 * (1.0 - n["h2"] ** 2)
    g["w2"], g["b2"] = d2.T @ n["h1"], d2.sum(0)
    dh1 = d2 @ n["w2"]
    d1 = dh1 * (1.0 - n["h1"] ** 2)
    g["w1"], g["b1"] = d1.T @ x, d1.sum(0)
    return g, dict(dh2=dh2, d2=d2, dh1=dh1, d1=d1)


def _assemble(gp, gv, dls):
    return np.concatenate([gp["w1"].ravel(), gp["b1"], gp["w2"].ravel(), gp["b2"], gp["wh"].ravel(), gp["bh"],
                           gv["w1"].ravel(), gv["b1"], gv["w2"].ravel(), gv["b2"], gv["wh"].ravel(), gv["bh"], dls])


def loss_and_grad(p, obs, act, old_logp, adv, ret, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, keep=False):
    """the minibatch is what is passed (gather with the index list first).  -> dict(grad [n_params], stats [7] in STAT_NAMES order, ratio, adv (after the
    normalisation)); keep=True adds every intermediate for grad_bounds"""
    x, act, old, adv, ret = (np.asarray(a, dtype=np.float64) for a in (obs, act, old_logp, adv, ret))
    B, A = act.shape
    c, ent_coef, vf_coef = f32(clip_range), f32(ent_coef), f32(vf_coef)
    pi, vf = _net(p, "pi", x), _net(p, "vf", x)
    mean, V = pi["out"], vf["out"][:, 0]
    ls = np.asarray(p["log_std"], dtype=np.float64)
    inv = np.exp(-ls)
    y = (act - mean) * inv
    logp = (-0.5 * y * y - ls - HALF_LOG_2PI).sum(1)
    adv_inv = 1.0 / (adv.std(ddof=1) + 1e-8) if (normalize_advantage and B > 1) else 0.0
    ad = (adv - adv.mean()) * adv_inv if adv_inv else adv
    lr = logp - old
    r = np.exp(lr)
    lo, hi = 1.0 - c, 1.0 + c
    passes = ~(((ad > 0) & (r > hi)) | ((ad < 0) & (r < lo)))
    g = np.where(passes, -ad * r / B, 0.0)
    dmean = g[:, None] * y * inv
    dls_rows = g[:, None] * (y * y - 1.0)
    dV = 2.0 * vf_coef * (V - ret) / B
    gp, ip = _back(pi, x, dmean)
    gv, iv = _back(vf, x, dV[:, None])
    grad = _assemble(gp, gv, dls_rows.sum(0) - ent_coef)
    rc = np.clip(r, lo, hi)
    pl, vl = np.mean(-np.minimum(ad * r, ad * rc)), np.mean((ret - V) ** 2)
    el = -(ls.sum() + A * (0.5 + HALF_LOG_2PI))
    kl, cf = np.mean((r - 1.0) - lr), np.mean(np.abs(r - 1.0) > c)
    stats = np.array([pl, vl, el, kl, cf, pl + vf_coef * vl + ent_coef * el, np.sqrt((grad ** 2).sum())])
    out = dict(grad=grad, stats=stats, ratio=r, adv=ad)
    if keep:
        out.update(x=x, act=act, old=old, ret=ret, pi=pi, vf=vf, ip=ip, iv=iv, ls=ls, inv=inv, y=y, logp=logp, lr=lr, passes=passes, g=g, dmean=dmean,
                   dls_rows=dls_rows, dV=dV, V=V, mean=mean, c=c, ent_coef=ent_coef, vf_coef=vf_coef, rc=rc, raw_adv=adv, adv_inv=adv_inv)
    return out


# ---------------------------------------------------------------- the bound ----------------------------------------------------------------
def _fwd_bounds(n, x, u):
    a = np.abs
    e_z1 = gam(19, u["u"]) * (a(x) @ a(n["w1"]).T + a(n["b1"]))
    e_h1 = PR._tanh_bound(n["z1"], e_z1, u["tanh"])
    H1 = a(n["h1"]) + e_h1
    e_z2 = e_h1 @ a(n["w2"]).T + gam(256, u["u"]) * (H1 @ a(n["w2"]).T + a(n["b2"]))
    e_h2 = PR._tanh_bound(n["z2"], e_z2, u["tanh"])
    H2 = a(n["h2"]) + e_h2
    e_out = e_h2 @ a(n["wh"]).T + gam(128, u["u"]) * (H2 @ a(n["wh"]).T + a(n["bh"]))
    return dict(e_h1=e_h1, H1=H1, e_h2=e_h2, H2=H2, e_out=e_out)


def _back_bounds(n, f, i, x, dout, e_dout, gd, u):
    """errors of one network's six gradients from the error of its head's upstream gradient; gd = gam(depth(B))"""
    a, uu = np.abs, u["u"]
    D = a(dout) + e_dout
    e = {"wh": e_dout.T @ f["H2"] + a(dout).T @ f["e_h2"] + gd * (D.T @ f["H2"]), "bh": e_dout.sum(0) + gd * D.sum(0)}
    e_dh2 = e_dout @ a(n["wh"]) + gam(8, uu) * (D @ a(n["wh"]))
    DH2 = a(i["dh2"]) + e_dh2
    q2, e_q2 = a(1.0 - n["h2"] ** 2), 2.0 * a(n["h2"]) * f["e_h2"] + f["e_h2"] ** 2 + uu * (1.0 + f["H2"] ** 2)
    e_d2 = e_dh2 * (q2 + e_q2) + a(i["dh2"]) * e_q2 + uu * DH2 * (q2 + e_q2)
    D2 = a(i["d2"]) + e_d2
    e["w2"], e["b2"] = e_d2.T @ f["H1"] + a(i["d2"]).T @ f["e_h1"] + gd * (D2.T @ f["H1"]), e_d2.sum(0) + gd * D2.sum(0)
    e_dh1 = e_d2 @ a(n["w2"]) + gam(128, uu) * (D2 @ a(n["w2"]))
    DH1 = a(i["dh1"]) + e_dh1
    q1, e_q1 = a(1.0 - n["h1"] ** 2), 2.0 * a(n["h1"]) * f["e_h1"] + f["e_h1"] ** 2 + uu * (1.0 + f["H1"] ** 2)
    e_d1 = e_dh1 * (q1 + e_q1) + a(i["dh1"]) * e_q1 + uu * DH1 * (q1 + e_q1)
    D1 = a(i["d1"]) + e_d1
    e["w1"], e["b1"] = e_d1.T @ a(x) + gd * (D1.T @ a(x)), e_d1.sum(0) + gd * D1.sum(0)
    return e


def grad_bounds(p, obs, act, old_logp, adv, ret, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, u=UNITS):
    """-> (reference dict of loss_and_grad, bound per gradient entry [n_params], bound per statistic [7])"""
    R = loss_and_grad(p, obs, act, old_logp, adv, ret, clip_range, ent_coef, vf_coef, normalize_advantage, keep=True)
    a, uu, ux, x = np.abs, u["u"], u["exp"], R["x"]
    B, A = R["act"].shape
    gd = gam(depth(B), uu)
    fp, fv = _fwd_bounds(R["pi"], x, u), _fwd_bounds(R["vf"], x, u)
    # ---- log-probability, ratio, advantage ----
    inv, y, ls = R["inv"], R["y"], R["ls"]
    d = R["act"] - R["mean"]
    e_d = fp["e_out"] + uu * (a(d) + fp["e_out"])
    e_y = e_d * inv * (1.0 + ux) + a(y) * (ux + uu)
    Y = a(y) + e_y
    t = a(-0.5 * y * y - ls - HALF_LOG_2PI)
    e_t = Y * e_y + 2.0 * uu * (a(ls) + HALF_LOG_2PI) + uu * (0.5 * Y * Y + a(ls) + HALF_LOG_2PI)
    e_logp = e_t.sum(1) + 3.0 * uu * (t + e_t).sum(1)                     # the eight lanes' butterfly: three additions
    e_lr = e_logp + uu * (a(R["lr"]) + e_logp)
    r = R["ratio"]
    e_r = r * (np.expm1(e_lr) + ux * np.exp(e_lr))
    ad = R["adv"]
    e_ad = uu * a(ad) + u["f64"] * (a(R["raw_adv"]) + a(R["raw_adv"]).mean()) * R["adv_inv"]       # (adv - mean) inv in float64 on both sides, rounded once
    c = R["c"]
    # (everything below takes the reference's decisions -- which side of a clip edge, which sign of the advantage -- for the kernel's: make_problem keeps every
    #  sample 1e-3 from a kink, and the clip_fraction statistic, exact up to its one rounding, shows that the kernel decided alike)
    # ---- d loss / d log-prob, d mean, d log_std, d value ----
    G = (a(ad) + e_ad) * (r + e_r) / B
    e_g = np.where(R["passes"], (a(ad) * e_r + r * e_ad + e_ad * e_r) / B + 3.0 * uu * G, 0.0)
    Gm = (a(R["g"]) + e_g)[:, None]
    e_dmean = e_g[:, None] * Y * inv + a(R["g"])[:, None] * e_y * inv + (2.0 * uu + ux) * Gm * Y * inv
    q = a(y * y - 1.0)
    e_q = 2.0 * Y * e_y + uu * (Y * Y + 1.0)
    e_dls = e_g[:, None] * (q + e_q) + a(R["g"])[:, None] * e_q + uu * Gm * (q + e_q)
    dv = R["V"] - R["ret"]
    e_dv = fv["e_out"][:, 0] + uu * (a(dv) + fv["e_out"][:, 0])
    k = 2.0 * R["vf_coef"] / B
    e_dV = k * e_dv + 2.0 * uu * k * (a(dv) + e_dv)
    # ---- the backward pass ----
    ep = _back_bounds(R["pi"], fp, R["ip"], x, R["dmean"], e_dmean, gd, u)
    ev = _back_bounds(R["vf"], fv, R["iv"], x, R["dV"][:, None], e_dV[:, None], gd, u)
    dls = R["dls_rows"].sum(0)
    e_ls = e_dls.sum(0) + gd * (a(R["dls_rows"]) + e_dls).sum(0) + uu * (a(dls) + a(R["ent_coef"]))
    e_grad = _assemble(ep, ev, e_ls) * SLACK
    # ---- the statistics: float64 sums of float32 row terms, rounded once ----
    AD = a(ad) + e_ad
    e_pl_rows = AD * e_r + np.maximum(r, R["rc"]) * e_ad + uu * AD * (np.maximum(r, 1.0 + c) + e_r) + uu * (1.0 + c) * AD
    e_vl_rows = 2.0 * a(dv) * e_dv + e_dv ** 2 + uu * (a(dv) + e_dv) ** 2
    e_kl_rows = e_r + uu * (a(r - 1.0) + e_r) + e_lr + uu * (a(r - 1.0) + a(R["lr"]) + e_r + e_lr)
    s = R["stats"]
    e_pl, e_vl, e_el = e_pl_rows.mean() + uu * a(s[0]), e_vl_rows.mean() + uu * a(s[1]), uu * a(s[2])
    e_stats = np.array([e_pl, e_vl, e_el, e_kl_rows.mean() + uu * a(s[3]), uu * s[4], e_pl + R["vf_coef"] * e_vl + a(R["ent_coef"]) * e_el + uu * a(s[5]),
                        np.sqrt((e_grad ** 2).sum()) + uu * s[6]]) * SLACK + u["f64"] * (1.0 + a(s))
    return R, e_grad, e_stats


# ---------------------------------------------------------------- clip + Adam ----------------------------------------------------------------
def adam(theta, grad, m, v, step, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step on flat float64 arrays; `step` is the count BEFORE the call.
    -> (theta, m, v, step + 1, the norm used)"""
    theta, grad, m, v = (np.asarray(t, dtype=np.float64) for t in (theta, grad, m, v))
    lr, b1, b2, eps, mx = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(max_grad_norm)
    norm = np.sqrt((grad * grad).sum())
    g = grad * (min(1.0, mx / (norm + 1e-6)) if mx > 0 else 1.0)
    t = int(step) + 1
    m, v = b1 * m + (1.0 - b1) * g, b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
    return theta - lr / (1.0 - b1 ** t) * m / denom, m, v, t, norm


def adam_bounds(theta0, theta, m, v, norm, u=UNITS):
    """the kernel does the same arithmetic in float64 and rounds every result once: (theta, m, v, norm) bounds"""
    a = np.abs
    f = 64.0 * u["f64"]
    return (u["u"] * a(theta) + f * (a(theta0) + a(theta - theta0)), (u["u"] + f) * a(m), (u["u"] + f) * a(v), (u["u"] + f) * norm)


# ---------------------------------------------------------------- test inputs ----------------------------------------------------------------
def make_params(A, seed):
    """float32 parameters with pre-activations of a few units (tanh neither linear nor saturated everywhere)"""
    rng = np.random.default_rng(seed)
    p = {}
    for k, s in shapes(A).items():
        if k == "log_std":
            p[k] = rng.uniform(-0.5, 0.3, s)
        elif len(s) == 1:
            p[k] = rng.normal(0, 0.1, s)
        else:
            p[k] = rng.normal(0, (0.3 if k in ("act_w",) else 1.4) / np.sqrt(s[1]), s)
    return {k: v.astype(np.float32) for k, v in p.items()}


EDGE_MARGIN, ADV_MARGIN = 1e-3, 1e-3


def margins(ref, clip_range=0.2):
    """(smallest distance of a ratio from a clip edge, smallest |advantage|) of a loss_and_grad result"""
    c, r = f32(clip_range), ref["ratio"]
    return float(np.minimum(np.abs(r - (1.0 - c)), np.abs(r - (1.0 + c))).min()), float(np.abs(ref["adv"]).min())


def make_problem(A, batch, seed, rows=None, index=False, clip_range=0.2):
    """-> dict(p, obs [rows, 19], act [rows, A], old_logp, adv, ret [rows] float32, index int32 [batch] or None).  rows: the buffer's rows (default batch);
    index=True: a shuffled index list WITH REPEATS into the buffer.  Target ratios are drawn from three bands -- below 1 - c, inside, above 1 + c -- each at least
    0.01 from an edge, advantage magnitudes from [0.3, 2] with random signs; a draw whose minibatch, with or without advantage normalisation, has a ratio within
    EDGE_MARGIN of an edge or an |advantage| below ADV_MARGIN is drawn again (deterministically: the seed sequence is fixed)."""
    rows = batch if rows is None else rows
    p = make_params(A, seed)
    for attempt in range(64):
        rng = np.random.default_rng([seed, attempt])
        obs = np.clip(rng.normal(0, 1.5, (rows, 19)), -10, 10).astype(np.float32)
        if rows > 3:
            obs[1, :] = 10.0; obs[2, ::2] = -10.0                                    # clipped observations, as VecNormalize leaves them
        mean, _ = PR.forward(p, obs)
        sigma = np.exp(p["log_std"].astype(np.float64))
        act = (mean + sigma * rng.normal(0, 1, (rows, A))).astype(np.float32)
        y = (act.astype(np.float64) - mean) / sigma
        logp = PR.log_prob(y, p["log_std"])
        c = f32(clip_range)
        band = rng.integers(0, 3, rows)
        target = np.where(band == 0, rng.uniform(1 - 2 * c, 1 - c - 0.01, rows), np.where(band == 1, rng.uniform(1 - c + 0.01, 1 + c - 0.01, rows),
                                                                                         rng.uniform(1 + c + 0.01, 1 + 2 * c, rows)))
        old = (logp - np.log(target)).astype(np.float32)
        adv = (rng.choice([-1.0, 1.0], rows) * rng.uniform(0.3, 2.0, rows)).astype(np.float32)
        ret = rng.normal(0, 1, rows).astype(np.float32)
        idx = None
        if index:
            idx = rng.integers(0, rows, batch).astype(np.int32)
            idx[: batch // 8] = idx[batch // 8: 2 * (batch // 8)]                   # repeats for certain
            rng.shuffle(idx)
        sel = idx if idx is not None else np.arange(batch)
        ok = True
        for norm in (False, True):
            e, a_ = margins(loss_and_grad(p, obs[sel], act[sel], old[sel], adv[sel], ret[sel], clip_range, 0.0, 0.5, norm), clip_range)
            ok = ok and e > EDGE_MARGIN and a_ > ADV_MARGIN
        if ok:
            return dict(p=p, obs=obs, act=act, old_logp=old, adv=adv, ret=ret, index=idx, batch=batch, rows=rows, A=A)
    raise RuntimeError("no draw without a sample near a kink")


def minibatch(pr):
    """the six arrays of the minibatch of a make_problem dict, gathered"""
    sel = pr["index"] if pr["index"] is not None else np.arange(pr["batch"])
    return pr["obs"][sel], pr["act"][sel], pr["old_logp"][sel], pr["adv"][sel], pr["ret"][sel]
