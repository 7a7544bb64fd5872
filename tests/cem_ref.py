"""Plain numpy restatement of the four calls that guide the planner (csrc/usim_score.hip: usim_score_block_tail; csrc/usim_plan.hip: usim_plan_sample_elem,
usim_plan_refit, usim_plan_tail; include/usim.h states the contracts), in the manner of plan_ref.py: no torch and no library calls.

Where the header states every float32 operation and its order the restatement is BITWISE:
- score_block_tail: the loop  ret = fmaf(disc, r, ret); disc *= gamma  and the bootstrap  ret = fmaf(disc_T, s tail, ret)  in float32 (fmaf32 below is an exactly
  rounded float32 fused multiply-add); s = (float)sqrt(ret_var + epsilon) from float64.
- refit: the elite set and its order are integers -- exact.
- plan_tail at temperature 0 is a selection -- exact.
Everything else is float64 with a BOUND per output, derived from the term count and M = max(|low|, |high|) (every candidate word is clipped to the box, so |x| <= M).
U24 = 2^-24 is the relative rounding of one float32 operation; the library's float32 division and square root are within 2.5 ulp = 5 U24 (it is built without the
IEEE fix-up sequences, csrc/Makefile).  Second-order products of these units are covered by the factor 1.01.  No bound is fitted to what the kernels return.

Error units of refit, per word (t, a) with E elites x_1 .. x_E taken in ascending candidate index:
  s    s += x from 0: E - 1 rounded additions (the first is exact), each of at most U24 of a partial sum <= E M           b_s = (E - 1) E M U24
  m    s / E, a quotient                                                                                                 b_m = b_s / E + 5 U24 M  = (E + 4) M U24
  d    x - m: the float32 m is off by b_m, the subtraction rounds once, |d| <= 2 M                                        b_d = b_m + 2 M U24
  q    q = fmaf(d, d, q) from 0: each square is off by 2 |d| b_d (+ b_d^2), E roundings of a partial sum <= E (2 M)^2       b_q = E 4 M b_d + E^2 4 M^2 U24
  v    q / E                                                                                                             b_v = b_q / E + 5 U24 v
  sd   sqrtf(v): |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= min(sqrt|a - b|, |a - b| / sqrt(b))                 b_sd = min(sqrt(b_v), b_v / sd) + 5 U24 sd
  out  fmaf(momentum, old, (1 - momentum) new): 1 - momentum rounds once, the product once, the fmaf once; clip and max are 1-Lipschitz
                                                                                                                         b = (1 - momentum) b_new + 3 U24 max(|raw|, |new|)
Error units of plan_tail: the weights are inputs (float32 words, exact); acc = fmaf(w, x, acc) along usim_plan_update's three-stage tree, every partial sum bounded
by S = sum_k w_k |x_k|, at most D = plan_ref.tree_depth(K) roundings on a path:  b = D U24 S."""
import numpy as np

import plan_ref as R

U24 = R.U24
SECOND_ORDER = R.SECOND_ORDER
REFIT_MAX_K = 4096                              # USIM_PLAN_REFIT_MAX_K


def fmaf32(a, b, c):
    """float32 fmaf(a, b, c), exactly rounded: the product of two float32 is exact in float64; the float64 sum is brought to ROUND-TO-ODD with the error term of
    TwoSum, after which the rounding to float32 (29 bits narrower) is the rounding of the exact value"""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(np.isfinite(s) & (err != 0) & even, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def tail_scale(ret_var, epsilon):
    """s of usim_score_block_tail: (float)sqrt(ret_var + epsilon) in float64; 1 without ret_var"""
    return np.float32(1.0) if ret_var is None else np.float32(np.sqrt(np.float64(ret_var) + np.float64(epsilon)))


def score_block(rew, done, gamma):
    """usim_score_block bit for bit: -> (return float32 [n], length int32 [n], disc float32 [n]: the running discount after the environment's last counted step,
    alive bool [n]: no done inside the block)"""
    rew = np.asarray(rew, dtype=np.float32)
    done = np.asarray(done) != 0
    T, n = rew.shape
    g = np.float32(gamma)
    ret, disc = np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)
    alive = np.ones(n, dtype=bool)
    length = np.full(n, T, dtype=np.int32)
    for k in range(T):
        ret = np.where(alive, fmaf32(disc, np.where(alive, rew[k], np.float32(0)), ret), ret)
        disc = np.where(alive, disc * g, disc).astype(np.float32)
        ended = alive & done[k]
        length[ended] = k + 1
        alive &= ~ended
    return ret, length, disc, alive


def score_block_tail(rew, done, gamma, tail=None, ret_var=None, epsilon=0.0):
    """usim_score_block_tail bit for bit: -> (return float32 [n], length int32 [n]).  tail None: score_block."""
    ret, length, disc, alive = score_block(rew, done, gamma)
    if tail is not None:
        s = tail_scale(ret_var, epsilon)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (s * np.where(alive, np.asarray(tail, dtype=np.float32), np.float32(0))).astype(np.float32)     # (the tail of an ended environment is never read)
            ret = np.where(alive, fmaf32(disc, t, ret), ret)
    return ret, length


def sample_elem(mean, sigma_elem, low, high, restart, per_group, smoothing, seed, counter, base=0):
    """usim_plan_sample_elem: plan_ref.sample with sigma_elem [G, H, A] in place of sigma [A] (every candidate of group g reads sigma_elem[g]); same dict"""
    sig = np.repeat(np.asarray(sigma_elem, dtype=np.float32), int(per_group), axis=0)                           # [n, H, A], the shape of the noise in plan_ref.sample
    return R.sample(mean, sig, low, high, restart, per_group, smoothing, seed, counter, base)


def elite_set(ret, per_group, elites):
    """the elite indices of usim_plan_refit: ret [n] -> int32 [G, elites], per group the min(elites, finite returns) candidates with the largest finite returns under
    "larger return, then lower index", listed in ascending candidate index and padded with -1"""
    K, E = int(per_group), int(elites)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.asarray(ret, dtype=np.float32).astype(np.float64).reshape(-1, K)
    out = np.full((r.shape[0], E), -1, dtype=np.int32)
    for g, row in enumerate(r):
        fin = np.flatnonzero(np.isfinite(row))
        order = fin[np.argsort(-row[fin], kind="stable")]                  # descending return; a stable sort keeps the lower index first among equals
        chosen = np.sort(order[:E])
        out[g, :len(chosen)] = chosen
    return out


def refit(cand, ret, low, high, per_group, elites, momentum, sigma_min, mean, sigma_elem):
    """usim_plan_refit on cand [H, n, A], ret [n], mean / sigma_elem [G, H, A] (float32 words): -> dict
       elite [G, elites] int32 (exact), mean, b_mean, sigma, b_sigma [G, H, A] float64"""
    cand = np.asarray(cand, dtype=np.float32).astype(np.float64)
    H, n, A = cand.shape
    K = int(per_group)
    G = n // K
    assert G * K == n
    low, high = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (low, high))
    M = float(max(np.abs(low).max(), np.abs(high).max()))
    mom = float(np.float32(momentum))
    smin = float(np.float32(sigma_min))
    m_old = np.asarray(mean, dtype=np.float32)
    m_old = np.where(np.isfinite(m_old), m_old, np.float32(0)).astype(np.float64)      # a non-finite word of the nominal counts as 0, as in the sampler
    s_old = np.asarray(sigma_elem, dtype=np.float32).astype(np.float64)
    elite = elite_set(ret, K, elites)
    new_mean, new_sigma = m_old.copy(), s_old.copy()
    b_mean, b_sigma = np.zeros_like(m_old), np.zeros_like(s_old)
    for g in range(G):
        idx = elite[g][elite[g] >= 0]
        E = len(idx)
        if E == 0:
            continue                                                       # no finite return: mean and sigma stay as they are, bit for bit
        x = cand[:, g * K + idx, :]                                        # [H, E, A]
        m = x.mean(axis=1)
        v = ((x - m[:, None, :]) ** 2).mean(axis=1)
        sd = np.sqrt(v)
        b_m = (E + 4) * M * U24
        b_d = b_m + 2 * M * U24
        b_q = SECOND_ORDER * E * 4 * M * b_d + E * E * 4 * M * M * U24
        b_v = b_q / E + 5 * U24 * v
        with np.errstate(divide="ignore", invalid="ignore"):
            b_sd = np.minimum(np.sqrt(b_v), np.where(sd > 0, b_v / sd, np.inf)) + 5 * U24 * sd
        raw_m = mom * m_old[g] + (1.0 - mom) * m
        raw_s = mom * s_old[g] + (1.0 - mom) * sd
        new_mean[g] = np.minimum(np.maximum(raw_m, low), high)
        new_sigma[g] = np.maximum(raw_s, smin)
        b_mean[g] = SECOND_ORDER * ((1.0 - mom) * b_m + 3 * U24 * np.maximum(np.abs(raw_m), np.abs(m)))
        b_sigma[g] = SECOND_ORDER * ((1.0 - mom) * b_sd + 3 * U24 * np.maximum(np.abs(raw_s), sd))
    return dict(elite=elite, mean=new_mean, b_mean=b_mean, sigma=new_sigma, b_sigma=b_sigma)


def tail_rows(cand, lengths, done_last, pol_act):
    """x of usim_plan_tail: the actor's action where the candidate survived all H steps (length == H and done[H - 1] == 0), else its own last action: [n, A]"""
    cand = np.asarray(cand, dtype=np.float32)
    H = cand.shape[0]
    alive = (np.asarray(lengths) == H) & (np.asarray(done_last) == 0)
    return np.where(alive[:, None], np.asarray(pol_act, dtype=np.float32), cand[H - 1]), alive


def plan_tail(cand, weights, best, lengths, done_last, pol_act, low, high, per_group, temperature):
    """usim_plan_tail: -> dict  tail [G, A] float64 (the words of next_mean[g][H - 1]), b_tail [G, A], exact (temperature 0: the best candidate's x, bit for bit)"""
    x32, _ = tail_rows(cand, lengths, done_last, pol_act)
    n, A = x32.shape
    K = int(per_group)
    G = n // K
    low, high = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (low, high))
    x = x32.astype(np.float64).reshape(G, K, A)
    if float(np.float32(temperature)) == 0.0:
        tail = x[np.arange(G), np.asarray(best, dtype=np.int64)]
        return dict(tail=tail, b_tail=np.zeros_like(tail), exact=True)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(G, K)
    with np.errstate(invalid="ignore"):
        term = np.where(w[:, :, None] != 0, w[:, :, None] * x, 0.0)        # a candidate of weight 0 adds nothing, whatever its x
        mag = np.where(w[:, :, None] != 0, w[:, :, None] * np.abs(x), 0.0)
    raw = term.sum(axis=1)
    b = SECOND_ORDER * R.tree_depth(K) * U24 * mag.sum(axis=1)
    return dict(tail=np.minimum(np.maximum(raw, low), high), b_tail=b, exact=False)
