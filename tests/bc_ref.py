"""Plain float64 restatement of usim_bc_grad (csrc/usim_ppo.hip; include/usim.h states the contract): the behaviour-cloning minibatch loss in its two forms, the
optional value regression, the entropy term, the eight statistics and the full gradient.  numpy only; the networks' forward and backward passes, the parameter
order, the Adam reference and the error-bound machinery are the ones of tests/ppo_ref.py (its module docstring states the units: u, gam(n), tanh, exp, depth(B),
f64, SLACK) -- the kernel shares every stage but the tile's loads and the heads' loss with usim_ppo_grad, and so does the bound.

What is new in the bound is stage 3 (with d = act - mean, one float32 subtraction; inv = expf(-log_std); y = d inv):
  NLL   the row's d loss / d log-prob is the constant -float32(1 / batch): relative error u, nothing else.  d mean = (g y) inv and d log_std = g (y^2 - 1) are
        the products usim_ppo_grad forms, so their error terms are ppo_ref's with e_g = u / batch
  MSE   d mean = (-2 float32(1 / batch)) d: the factor is exact but for the u of 1 / batch, the product is one rounding; log_std receives -ent_coef only
  value d V = float32(2 vf_coef / batch) (V - value): ppo_ref's value row
  statistics: float64 sums of float32 row terms (-log-prob, or sum_a d^2 -- a product and the three additions of the eight lanes' butterfly), rounded once
Nothing here is fitted to the kernel's output."""
import numpy as np

import policy_ref as PR
import ppo_ref as R

NLL, MSE = 0, 1                                # USIM_BC_NLL, USIM_BC_MSE
STAT_NAMES = ("policy_loss", "value_loss", "entropy_loss", "action_mse", "mean_logp", "loss", "grad_norm")
VF_FIELDS = ("vf_w1", "vf_b1", "vf_w2", "vf_b2", "val_w", "val_b")


def field_slices(A):
    """field name -> slice of the flat block"""
    out, o = {}, 0
    for k, s in R.shapes(A).items():
        n = int(np.prod(s))
        out[k] = slice(o, o + n)
        o += n
    return out


def _zero_net():
    return {"w1": np.zeros((256, 19)), "b1": np.zeros(256), "w2": np.zeros((128, 256)), "b2": np.zeros(128), "wh": np.zeros((1, 128)), "bh": np.zeros(1)}


def loss_and_grad(p, obs, act, value=None, loss=NLL, ent_coef=1e-3, vf_coef=0.5, keep=False):
    """the minibatch is what is passed (gather with the clamped index list first).  value None or vf_coef == 0: no value term, the value network is not
    evaluated and its gradient is zero.  -> dict(grad [n_params], stats [7] in STAT_NAMES order); keep=True adds every intermediate for grad_bounds"""
    assert loss in (NLL, MSE)
    x, act = np.asarray(obs, dtype=np.float64), np.asarray(act, dtype=np.float64)
    B, A = act.shape
    ent_coef, vf_coef = R.f32(ent_coef), R.f32(vf_coef)
    valued = value is not None and vf_coef != 0.0
    pi = R._net(p, "pi", x)
    mean = pi["out"]
    ls = np.asarray(p["log_std"], dtype=np.float64)
    inv = np.exp(-ls)
    d = act - mean
    y = d * inv
    logp = (-0.5 * y * y - ls - R.HALF_LOG_2PI).sum(1)
    sq = (d * d).sum(1)
    if loss == NLL:
        g = np.full(B, -1.0 / B)
        dmean, dls_rows, rows = g[:, None] * y * inv, g[:, None] * (y * y - 1.0), -logp
    else:
        g = np.zeros(B)
        dmean, dls_rows, rows = -2.0 * d / B, np.zeros_like(d), sq
    gp, ip = R._back(pi, x, dmean)
    vf = iv = dV = V = val = None
    gv, vl = _zero_net(), 0.0
    if valued:
        val = np.asarray(value, dtype=np.float64)
        vf = R._net(p, "vf", x)
        V = vf["out"][:, 0]
        dV = 2.0 * vf_coef * (V - val) / B
        gv, iv = R._back(vf, x, dV[:, None])
        vl = np.mean((val - V) ** 2)
    else:
        vf_coef = 0.0
    grad = R._assemble(gp, gv, dls_rows.sum(0) - ent_coef)
    pl = rows.mean()
    el = -(ls.sum() + A * (0.5 + R.HALF_LOG_2PI))
    stats = np.array([pl, vl, el, sq.mean(), logp.mean(), pl + vf_coef * vl + ent_coef * el, np.sqrt((grad ** 2).sum())])
    out = dict(grad=grad, stats=stats)
    if keep:
        out.update(x=x, act=act, value=val, pi=pi, vf=vf, ip=ip, iv=iv, ls=ls, inv=inv, d=d, y=y, logp=logp, sq=sq, g=g, dmean=dmean, dls_rows=dls_rows, dV=dV, V=V,
                   ent_coef=ent_coef, vf_coef=vf_coef, valued=valued, loss=loss)
    return out


def grad_bounds(p, obs, act, value=None, loss=NLL, ent_coef=1e-3, vf_coef=0.5, u=R.UNITS):
    """-> (reference dict of loss_and_grad, bound per gradient entry [n_params], bound per statistic [7])"""
    Q = loss_and_grad(p, obs, act, value, loss, ent_coef, vf_coef, keep=True)
    a, uu, ux, x = np.abs, u["u"], u["exp"], Q["x"]
    B, A = Q["act"].shape
    gd = R.gam(R.depth(B), uu)
    fp = R._fwd_bounds(Q["pi"], x, u)
    inv, y, ls, d = Q["inv"], Q["y"], Q["ls"], Q["d"]
    # ---- d = act - mean, y = d inv, the lanes' log-prob terms and squares, their butterflies ----
    e_d = fp["e_out"] + uu * (a(d) + fp["e_out"])
    e_y = e_d * inv * (1.0 + ux) + a(y) * (ux + uu)
    Y = a(y) + e_y
    t = a(-0.5 * y * y - ls - R.HALF_LOG_2PI)
    e_t = Y * e_y + 2.0 * uu * (a(ls) + R.HALF_LOG_2PI) + uu * (0.5 * Y * Y + a(ls) + R.HALF_LOG_2PI)
    e_logp = e_t.sum(1) + 3.0 * uu * (t + e_t).sum(1)
    e_sqa = 2.0 * a(d) * e_d + e_d ** 2 + uu * (a(d) + e_d) ** 2
    e_sq = e_sqa.sum(1) + 3.0 * uu * (d * d + e_sqa).sum(1)
    # ---- d loss / d mean, d log_std ----
    if loss == NLL:
        e_g = np.full(B, uu / B)                                              # float32(1 / batch)
        Gm = (a(Q["g"]) + e_g)[:, None]
        e_dmean = e_g[:, None] * Y * inv + a(Q["g"])[:, None] * e_y * inv + (2.0 * uu + ux) * Gm * Y * inv
        q = a(y * y - 1.0)
        e_q = 2.0 * Y * e_y + uu * (Y * Y + 1.0)
        e_dls = e_g[:, None] * (q + e_q) + a(Q["g"])[:, None] * e_q + uu * Gm * (q + e_q)
        e_rows = e_logp
    else:
        k = 2.0 / B
        e_dmean = k * e_d + 2.0 * uu * k * (a(d) + e_d)                      # the u of 1 / batch and the product's
        e_dls = np.zeros_like(d)
        e_rows = e_sq
    ep = R._back_bounds(Q["pi"], fp, Q["ip"], x, Q["dmean"], e_dmean, gd, u)
    dls = Q["dls_rows"].sum(0)
    e_ls = e_dls.sum(0) + gd * (a(Q["dls_rows"]) + e_dls).sum(0) + uu * (a(dls) + a(Q["ent_coef"]))
    # ---- the value term ----
    if Q["valued"]:
        fv = R._fwd_bounds(Q["vf"], x, u)
        dv = Q["V"] - Q["value"]
        e_dv = fv["e_out"][:, 0] + uu * (a(dv) + fv["e_out"][:, 0])
        k = 2.0 * Q["vf_coef"] / B
        e_dV = k * e_dv + 2.0 * uu * k * (a(dv) + e_dv)
        ev = R._back_bounds(Q["vf"], fv, Q["iv"], x, Q["dV"][:, None], e_dV[:, None], gd, u)
        e_vl_rows = 2.0 * a(dv) * e_dv + e_dv ** 2 + uu * (a(dv) + e_dv) ** 2
    else:
        ev, e_vl_rows = _zero_net(), np.zeros(B)                             # not evaluated: exact zeros
    e_grad = R._assemble(ep, ev, e_ls) * R.SLACK
    s = Q["stats"]
    e_pl, e_vl, e_el = e_rows.mean() + uu * a(s[0]), e_vl_rows.mean() + uu * a(s[1]), uu * a(s[2])
    e_stats = np.array([e_pl, e_vl, e_el, e_sq.mean() + uu * a(s[3]), e_logp.mean() + uu * a(s[4]),
                        e_pl + Q["vf_coef"] * e_vl + a(Q["ent_coef"]) * e_el + uu * a(s[5]), np.sqrt((e_grad ** 2).sum()) + uu * s[6]]) * R.SLACK \
        + u["f64"] * (1.0 + a(s))
    return Q, e_grad, e_stats


def clamp_index(index, rows):
    """what the kernel reads for an index list: an entry outside [0, rows) is moved to its nearest row"""
    return np.clip(np.asarray(index, dtype=np.int64), 0, rows - 1)


def make_problem(A, batch, seed, rows=None, index=False):
    """-> dict(p, obs [rows, 19], act [rows, A], value [rows] float32, index int32 [batch] or None).  index=True: a shuffled index list WITH REPEATS and with
    entries on both sides outside [0, rows).  The expert actions lie in the action box, a noisy copy of what another seeded network would do."""
    rows = batch if rows is None else rows
    p = R.make_params(A, seed)
    rng = np.random.default_rng([seed, 77])
    obs = np.clip(rng.normal(0, 1.5, (rows, 19)), -10, 10).astype(np.float32)
    if rows > 3:
        obs[1, :] = 10.0; obs[2, ::2] = -10.0                                 # clipped observations, as VecNormalize leaves them
    expert, _ = PR.forward(R.make_params(A, seed + 1000), obs)
    act = np.clip(expert + rng.normal(0, 0.2, (rows, A)), -1.0, 1.0).astype(np.float32)
    value = rng.normal(0, 1, rows).astype(np.float32)
    idx = None
    if index:
        idx = rng.integers(0, rows, batch).astype(np.int32)
        idx[: batch // 8] = idx[batch // 8: 2 * (batch // 8)]               # repeats for certain
        idx[-1], idx[-2] = -3, rows + 5                                       # out of range on both sides
        if batch > 4:
            idx[-3], idx[-4] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
        rng.shuffle(idx)
    return dict(p=p, obs=obs, act=act, value=value, index=idx, batch=batch, rows=rows, A=A)


def minibatch(pr):
    """the three arrays of the minibatch of a make_problem dict, gathered through the clamped index list"""
    sel = clamp_index(pr["index"], pr["rows"]) if pr["index"] is not None else np.arange(pr["batch"])
    return pr["obs"][sel], pr["act"][sel], pr["value"][sel]
