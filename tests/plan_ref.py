"""Plain float64 restatement of the two planner kernels (csrc/usim_plan.hip: usim_plan_sample, usim_plan_update; include/usim.h states the contract): numpy only,
built on policy_ref.philox4x32, no torch and no library calls, so that it shares no rounding with what it checks.  Every function that returns a value the kernels
round also returns a BOUND per output, from an absolute-value companion pass in the manner of policy_ref.forward_bounds.  U24 = 2^-24 is the relative rounding of
one float32 operation.

- plan_noise: xi ~ N(0, 1) for (candidate, step, component), Box-Muller in float64 on the Philox words the kernel uses: counter words (candidate, (counter + base)
  mod 2^32, 4 t + (a >> 1), PLAN_TAG), key (seed low, seed high); u1 = ((word 0 >> 8) + 1) / 2^24, u2 = (word 1 >> 8) / 2^24.
- sample / sample_bound: cand[t][g K + k][a] = clip(m + sigma e), e[0] = xi[0], e[t] = s e[t - 1] + sqrt(1 - s^2) xi[t], e = 0 for k = 0.
- update: best, weights, plan, action, next nominal, and the bounds of weights and plan.

Error units of the sampler.  The draw is made of the operations of the policy sampler (tests/test_gpu_policy_kernels.py derives them):
  radius  2^-21 relative    sqrt(-2 ln u1): v_log at 1 ulp, the root built without the IEEE fix-up at <= 2.5 ulp
  trig    1.5e-6 absolute   the angle 2 PI_F u2, the 1 / 2 pi product inside __sinf / __cosf, v_sin / v_cos
  so      b_xi = |xi| (2^-21 + U24) + radius 1.5e-6           (the product radius x trig rounds once more)
  The smoothing recursion in the kernel is  e[t] = fmaf(s, e[t - 1], c xi[t])  with c = sqrt(1 - s^2) rounded once from float64 (U24 relative), the product c xi
  rounded (U24) and the fmaf rounded (U24 of the result):
      b_e[0] = b_xi[0]        b_e[t] = s b_e[t - 1] + c b_xi[t] + 2 U24 c |xi[t]| + U24 |e[t]|
  The sample is fmaf(sigma, e, m) -- one rounding -- and the clip is 1-Lipschitz:   b_cand = sigma b_e + U24 |m + sigma e|.
  Candidate 0 (e = 0) is fmaf(sigma, 0, m) = m: exact, bound 0.  Second-order products of these units are covered by the factor 1.01.

Error units of the weights, from the kernel's operation sequence  x = (ret_k - ret_best) / temperature;  e_k = expf(x);  S = sum e_k;  w_k = e_k / S:
  x       6 U24 |x|         the subtraction rounds once (U24); the library is built without the IEEE division fix-up, a quotient is within 2.5 ulp = 5 U24
  e_k     relative  rho_k = expm1(6 U24 |x|) + 2^-23: the argument's error amplified by exp, and expf at its documented 1 ulp (HIP math API); absolute floor 2^-126
          where the float32 result is subnormal or flushed      b_e = e_k rho_k + 2^-126
  S       the fixed tree: thread j adds its ceil(K / 256) terms in order, six butterfly stages in the wave, three adds over the four waves -- at most
          D = ceil(K / 256) + 9 roundings on any path, each of at most U24 of a partial sum of non-negative terms <= S:     b_S = sum b_e + D U24 S
  w_k     a quotient again:  b_w = b_e / S + e_k b_S / S^2 + 5 U24 w_k
  plan    acc = fmaf(w_k, cand, acc) along the same tree, every partial sum bounded by M = sum_k w_k |cand|:     b_plan = sum_k b_w |cand| + D U24 M;  the clip is
          1-Lipschitz.  At temperature 0 nothing is rounded: weights exactly 0 / 1, plan the chosen candidate's words.
No bound is fitted to what the kernels return."""
import numpy as np

import policy_ref as P

PLAN_TAG = 0x504C414E                           # fourth counter word of the planner's noise ("PLAN")
U24 = 2.0**-24
REL_RAD, TRIG = 2.0**-21, 1.5e-6
WG = 256                                        # threads of a workgroup of usim_plan_update
SECOND_ORDER = 1.01


def plan_noise(seed, candidates, horizon, adim, counter, base=0):
    """N(0, 1) of usim_plan_sample for the global candidate indices `candidates` (g K + k): -> (xi, radius), float64 [len(candidates), horizon, adim]"""
    seed = int(seed)
    c = np.asarray(candidates, dtype=np.int64).reshape(-1, 1, 1)
    t = np.arange(horizon, dtype=np.int64).reshape(1, -1, 1)
    a = np.arange(adim, dtype=np.int64).reshape(1, 1, -1)
    w = P.philox4x32((c, (int(counter) + int(base)) % 2**32, 4 * t + (a >> 1), PLAN_TAG), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w[0] >> 8).astype(np.float64) + 1.0) / 2.0**24
    u2 = (w[1] >> 8).astype(np.float64) / 2.0**24
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.where(a % 2 == 0, rad * np.cos(ang), rad * np.sin(ang)), rad


def sample(mean, sigma, low, high, restart, per_group, smoothing, seed, counter, base=0):
    """usim_plan_sample on mean [G, H, A] (float32 words, non-finite ones count as 0): -> dict
       cand [H, n, A] float64, bound [H, n, A], mean_after [G, H, A] (the float32 words of mean_dev after the call: zeros where restart[g] != 0)"""
    mean = np.asarray(mean, dtype=np.float32)
    G, H, A = mean.shape
    K, n = int(per_group), G * int(per_group)
    sigma, low, high = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (sigma, low, high))
    fresh = np.zeros(G, dtype=bool) if restart is None else np.asarray(restart) != 0
    mean_after = mean.copy()
    mean_after[fresh] = 0.0
    m = np.where(np.isfinite(mean_after), mean_after, np.float32(0)).astype(np.float64)               # [G, H, A]
    s = float(np.float32(smoothing))
    c = np.sqrt(1.0 - s * s)
    xi, rad = plan_noise(seed, np.arange(n), H, A, counter, base)                                      # [n, H, A]
    b_xi = np.abs(xi) * (REL_RAD + U24) + rad * TRIG
    e, b_e = np.zeros_like(xi), np.zeros_like(xi)
    for t in range(H):
        if t == 0:
            e[:, 0], b_e[:, 0] = xi[:, 0], b_xi[:, 0]
        else:
            e[:, t] = s * e[:, t - 1] + c * xi[:, t]
            b_e[:, t] = s * b_e[:, t - 1] + c * b_xi[:, t] + SECOND_ORDER * (2 * U24 * c * np.abs(xi[:, t]) + U24 * np.abs(e[:, t]))
    nominal = np.arange(n) % K == 0
    e[nominal], b_e[nominal] = 0.0, 0.0
    mm = np.repeat(m, K, axis=0)                                                                       # [n, H, A]: candidate g K + k reads group g
    raw = mm + sigma * e
    bound = sigma * b_e + SECOND_ORDER * U24 * np.abs(raw)
    bound[nominal] = 0.0
    cand = np.minimum(np.maximum(raw, low), high)
    return dict(cand=cand.transpose(1, 0, 2).copy(), bound=bound.transpose(1, 0, 2).copy(), mean_after=mean_after)


def tree_depth(per_group):
    """roundings on the longest path of the kernel's three-stage reduction over per_group terms"""
    return -(-int(per_group) // WG) + 9


def update(cand, ret, low, high, per_group, temperature):
    """usim_plan_update on cand [H, n, A] and ret [n] (float32 words): -> dict
       best [G] int, weights [n], b_weights [n], plan [G, H, A], b_plan [G, H, A], act [G, A], next_mean [G, H, A], exact (bool: temperature 0, nothing rounds)"""
    cand = np.asarray(cand, dtype=np.float32).astype(np.float64)
    H, n, A = cand.shape
    K = int(per_group)
    G = n // K
    assert G * K == n
    low, high = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (low, high))
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.asarray(ret, dtype=np.float32).astype(np.float64).reshape(G, K)
    fin = np.isfinite(r)
    none = ~fin.any(axis=1)
    best = np.argmax(np.where(fin, r, -np.inf), axis=1)                    # (the first maximum: ties to the lowest index)
    best[none] = 0
    c = cand.reshape(H, G, K, A)
    rows = np.arange(G)
    onehot = np.zeros((G, K))
    onehot[rows, best] = 1.0
    T = float(np.float32(temperature))
    if T == 0.0:
        w, b_w = onehot, np.zeros((G, K))
        plan = c[:, rows, best, :].transpose(1, 0, 2).copy()
        b_plan = np.zeros_like(plan)
    else:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            x = np.where(fin, (r - r[rows, best][:, None]) / T, -np.inf)
            e = np.exp(x)
            rho = np.expm1(np.minimum(6 * U24 * np.abs(x), 1.0)) + 2.0**-23
        b_e = np.where(fin, e * rho + 2.0**-126, 0.0)
        e[none], b_e[none] = onehot[none], 0.0
        D = tree_depth(K)
        S = e.sum(axis=1, keepdims=True)
        b_S = b_e.sum(axis=1, keepdims=True) + D * U24 * S
        w = e / S
        b_w = SECOND_ORDER * (b_e / S + e * b_S / S**2 + 5 * U24 * w)
        raw = np.einsum("gk,hgka->gha", w, c)
        b_plan = np.einsum("gk,hgka->gha", b_w, np.abs(c)) + SECOND_ORDER * D * U24 * np.einsum("gk,hgka->gha", w, np.abs(c))
        plan = np.minimum(np.maximum(raw, low), high)
    next_mean = np.concatenate([plan[:, 1:], plan[:, -1:]], axis=1)
    return dict(best=best, weights=w.reshape(n), b_weights=b_w.reshape(n), plan=plan, b_plan=b_plan, act=plan[:, 0].copy(), next_mean=next_mean, exact=T == 0.0)
