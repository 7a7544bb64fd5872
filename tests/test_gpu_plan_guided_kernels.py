"""usim_score_block_tail, usim_plan_sample_elem, usim_plan_refit and usim_plan_tail (csrc/usim_score.hip, csrc/usim_plan.hip) through their C ABI against
tests/cem_ref.py: caller buffers only, no simulator.  Bit for bit where the header states every operation (the score, the elite set, the selection at temperature
0, the sampler against usim_plan_sample); otherwise within the bounds cem_ref derives from the term count and the action box.

Shapes (G, K, H, A): (1, 1, 1, 6) the smallest, (3, 5, 4, 7) odd everywhere, (2, 257, 3, 6) with K one past a workgroup's 256 threads.  The returns are drawn from
a few values, so ties are everywhere, with NaN and both infinities planted; the last group of a shape with more than one has no finite return at all.  Every output
buffer carries guard words behind its end."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cem_ref as Q
import plan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1, 6), (3, 5, 4, 7), (2, 257, 3, 6)]
GUARD = 32
SENT = -12345.0


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)                       # (a copy: the shared problems are read-only)


def _guarded(x):
    """device copy of x with GUARD sentinel words behind it -> (tensor, check() that the guard is untouched)"""
    flat = np.ascontiguousarray(x).reshape(-1)
    sent = np.full(GUARD, SENT if flat.dtype.kind == "f" else -777, dtype=flat.dtype)
    t = _dev(np.concatenate([flat, sent]))
    return t, lambda: bool((t[flat.size:].cpu() == torch.from_numpy(sent)).all())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _box(A):
    low = -np.linspace(0.5, 1.0, A).astype(np.float32)
    return low, (-low * 0.9).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _problem(G, K, H, A):
    """candidates inside the box, returns with ties / NaN / infinities, a nominal and per-element deviations; the last of several groups has no finite return"""
    rng = np.random.default_rng(100 * G + K + 7 * H)
    low, high = _box(A)
    n = G * K
    cand = rng.uniform(low, high, (H, n, A)).astype(np.float32)
    ret = rng.choice(np.array([-2.0, 0.0, -0.0, 1.5, 1.5000001, 3.0], dtype=np.float32), n)
    if K >= 5:
        for g in range(G):
            ret[g * K + np.array([1, 2, 3]) * (K // 5)] = [np.nan, np.inf, -np.inf]
    if G > 1:
        ret[(G - 1) * K:] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), K)
    mean = rng.uniform(low, high, (G, H, A)).astype(np.float32)
    sigma = rng.uniform(0.05, 0.4, (G, H, A)).astype(np.float32)
    for x in (cand, ret, mean, sigma, low, high):
        x.setflags(write=False)
    return cand, ret, mean, sigma, low, high


# ---- usim_plan_refit ------------------------------------------------------------------------------------------------------------------------
def _refit(usim, cand, ret, mean, sigma, low, high, G, K, H, A, elites, momentum=0.25, sigma_min=0.05):
    lib = usim._lib.load()
    m, m_ok = _guarded(mean)
    s, s_ok = _guarded(sigma)
    e, e_ok = _guarded(np.full((G, elites), -5, dtype=np.int32))
    c, r, lo, hi = _dev(cand), _dev(ret), _dev(low), _dev(high)
    rc = lib.usim_plan_refit(c.data_ptr(), r.data_ptr(), lo.data_ptr(), hi.data_ptr(), G, K, H, A, elites, momentum, sigma_min, m.data_ptr(), s.data_ptr(), e.data_ptr(),
                             _stream())
    torch.cuda.synchronize()
    assert rc == 0 and m_ok() and s_ok() and e_ok()
    w = G * H * A
    return m[:w].cpu().numpy().reshape(G, H, A), s[:w].cpu().numpy().reshape(G, H, A), e[:G * elites].cpu().numpy().reshape(G, elites)


@pytest.mark.parametrize("elites", [1, 2, "K"])
@pytest.mark.parametrize("G,K,H,A", SHAPES)
def test_refit_against_the_reference(usim, G, K, H, A, elites):
    E = K if elites == "K" else min(elites, K)
    cand, ret, mean, sigma, low, high = _problem(G, K, H, A)
    ref = Q.refit(cand, ret, low, high, K, E, 0.25, 0.05, mean, sigma)
    got_m, got_s, got_e = _refit(usim, cand, ret, mean, sigma, low, high, G, K, H, A, E)
    assert np.array_equal(got_e, ref["elite"])                            # the set and its order are integers: exact
    em, es = np.abs(got_m.astype(np.float64) - ref["mean"]), np.abs(got_s.astype(np.float64) - ref["sigma"])
    for name, err, b in (("mean", em, ref["b_mean"]), ("sigma", es, ref["b_sigma"])):
        print(f"{name}: worst error {err.max():.3e}, worst error / bound {float(np.max(np.where(err == 0, 0, err / np.maximum(b, 1e-300)))):.3f}")
        assert np.all(err <= b), name
    assert np.all(got_s >= np.float32(0.05)) and np.all(got_m >= low) and np.all(got_m <= high)
    if G > 1:                                                             # no finite return: all -1, mean and sigma bit for bit as they were
        assert (got_e[G - 1] == -1).all()
        assert np.array_equal(_bits(got_m[G - 1]), _bits(mean[G - 1])) and np.array_equal(_bits(got_s[G - 1]), _bits(sigma[G - 1]))
        assert not np.array_equal(_bits(got_m[0]), _bits(mean[0]))
    # the same call again: the same bits
    again = _refit(usim, cand, ret, mean, sigma, low, high, G, K, H, A, E)
    assert np.array_equal(_bits(again[0]), _bits(got_m)) and np.array_equal(_bits(again[1]), _bits(got_s)) and np.array_equal(again[2], got_e)


def test_refit_of_a_lone_candidate_without_a_finite_return(usim):
    cand, _, mean, sigma, low, high = _problem(1, 1, 1, 6)
    for bad in (np.nan, np.inf, -np.inf):
        got_m, got_s, got_e = _refit(usim, cand, np.array([bad], dtype=np.float32), mean, sigma, low, high, 1, 1, 1, 6, 1)
        assert got_e.tolist() == [[-1]] and np.array_equal(_bits(got_m), _bits(mean)) and np.array_equal(_bits(got_s), _bits(sigma))


def test_refit_without_momentum_takes_the_elites_moments_and_reads_a_bad_nominal_as_zero(usim):
    G, K, H, A = 3, 5, 4, 7
    cand, ret, mean, sigma, low, high = _problem(G, K, H, A)
    bad = mean.copy()
    bad[0, 1, 2], bad[1, 0, 0] = np.nan, np.inf
    ref = Q.refit(cand, ret, low, high, K, 2, 0.0, 1e-3, bad, sigma)
    got_m, got_s, got_e = _refit(usim, cand, ret, bad, sigma, low, high, G, K, H, A, 2, momentum=0.0, sigma_min=1e-3)
    assert np.isfinite(got_m[:2]).all() and np.array_equal(got_e, ref["elite"])
    assert np.all(np.abs(got_m - ref["mean"]) <= ref["b_mean"]) and np.all(np.abs(got_s - ref["sigma"]) <= ref["b_sigma"])
    half = Q.refit(cand, ret, low, high, K, 2, 0.5, 1e-3, bad, sigma)       # with momentum the bad words count as 0
    got_m, got_s, _ = _refit(usim, cand, ret, bad, sigma, low, high, G, K, H, A, 2, momentum=0.5, sigma_min=1e-3)
    assert np.isfinite(got_m[:2]).all() and np.all(np.abs(got_m - half["mean"]) <= half["b_mean"]) and np.all(np.abs(got_s - half["sigma"]) <= half["b_sigma"])


@pytest.mark.parametrize("G,K,H,A", SHAPES[1:])
def test_refit_of_a_group_does_not_depend_on_the_others(usim, G, K, H, A):
    cand, ret, mean, sigma, low, high = _problem(G, K, H, A)
    base = _refit(usim, cand, ret, mean, sigma, low, high, G, K, H, A, 2)
    rng = np.random.default_rng(1)
    c2, r2, m2, s2 = cand.copy(), ret.copy(), mean.copy(), sigma.copy()
    c2[:, K:], r2[K:] = rng.uniform(low, high, (H, (G - 1) * K, A)).astype(np.float32), rng.standard_normal((G - 1) * K).astype(np.float32)
    m2[1:], s2[1:] = 0.0, 0.3
    other = _refit(usim, c2, r2, m2, s2, low, high, G, K, H, A, 2)
    for a, b in zip(base, other):
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
    assert not np.array_equal(base[2][1], other[2][1]) or not np.array_equal(_bits(base[0][1]), _bits(other[0][1]))


def test_refit_at_the_largest_group(usim):
    """K = USIM_PLAN_REFIT_MAX_K: the whole of the LDS the ranking declares is in use; elites at both ends of the range"""
    G, H, A = 2, 2, 6
    K = usim._lib.PLAN_REFIT_MAX_K
    rng = np.random.default_rng(8)
    low, high = _box(A)
    cand = rng.uniform(low, high, (H, G * K, A)).astype(np.float32)
    ret = rng.integers(-50, 50, G * K).astype(np.float32)                 # ~40 candidates per value
    ret[rng.integers(0, G * K, 100)] = np.nan
    mean, sigma = np.zeros((G, H, A), dtype=np.float32), np.full((G, H, A), 0.3, dtype=np.float32)
    for E in (64, K):
        ref = Q.refit(cand, ret, low, high, K, E, 0.1, 1e-3, mean, sigma)
        got_m, got_s, got_e = _refit(usim, cand, ret, mean, sigma, low, high, G, K, H, A, E, momentum=0.1, sigma_min=1e-3)
        assert np.array_equal(got_e, ref["elite"])
        assert np.all(np.abs(got_m - ref["mean"]) <= ref["b_mean"]) and np.all(np.abs(got_s - ref["sigma"]) <= ref["b_sigma"])


# ---- usim_plan_sample_elem ----------------------------------------------------------------------------------------------------------------------
def _sample(usim, elem, mean, sigma, low, high, restart, G, K, H, A, smoothing, counter, base):
    lib = usim._lib.load()
    m, m_ok = _guarded(mean)
    cand, c_ok = _guarded(np.full((H, G * K, A), SENT, dtype=np.float32))
    s, lo, hi = _dev(sigma), _dev(low), _dev(high)
    rs = None if restart is None else _dev(np.asarray(restart, dtype=np.uint8))
    b = None if base is None else _dev(np.array([base], dtype=np.int32))
    fn = lib.usim_plan_sample_elem if elem else lib.usim_plan_sample
    rc = fn(m.data_ptr(), s.data_ptr(), lo.data_ptr(), hi.data_ptr(), None if rs is None else rs.data_ptr(), G, K, H, A, smoothing, 0x1234567890, counter,
            None if b is None else b.data_ptr(), cand.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and m_ok() and c_ok()
    return cand[:H * G * K * A].cpu().numpy().reshape(H, G * K, A), m[:G * H * A].cpu().numpy().reshape(G, H, A)


@pytest.mark.parametrize("smoothing, restart", [(0.0, False), (0.6, True)])
@pytest.mark.parametrize("G,K,H,A", SHAPES)
def test_sample_elem_with_a_broadcast_sigma_is_the_sampler_bit_for_bit(usim, G, K, H, A, smoothing, restart):
    _, _, mean, _, low, high = _problem(G, K, H, A)
    sigma = np.linspace(0.1, 0.4, A).astype(np.float32)
    flags = ([1] + [0] * (G - 1)) if restart else None
    a_c, a_m = _sample(usim, False, mean, sigma, low, high, flags, G, K, H, A, smoothing, 3, 5 if restart else None)
    b_c, b_m = _sample(usim, True, mean, np.broadcast_to(sigma, (G, H, A)), low, high, flags, G, K, H, A, smoothing, 3, 5 if restart else None)
    assert np.array_equal(_bits(a_c), _bits(b_c)) and np.array_equal(_bits(a_m), _bits(b_m))
    if restart:
        assert not b_m[0].any() and np.array_equal(_bits(b_m[1:]), _bits(mean[1:]))


@pytest.mark.parametrize("G,K,H,A", SHAPES)
def test_sample_elem_against_the_reference(usim, G, K, H, A):
    _, _, mean, sigma, low, high = _problem(G, K, H, A)
    flags = [0] * (G - 1) + [1]
    ref = Q.sample_elem(mean, sigma, low, high, flags, K, 0.6, 0x1234567890, 3, 5)
    got, got_mean = _sample(usim, True, mean, sigma, low, high, flags, G, K, H, A, 0.6, 3, 5)
    err = np.abs(got.astype(np.float64) - ref["cand"])
    print("worst error / bound", float(np.max(np.where(err == 0, 0, err / np.maximum(ref["bound"], 1e-300)))))
    assert np.all(err <= ref["bound"]) and np.array_equal(_bits(got_mean), _bits(ref["mean_after"]))
    again, _ = _sample(usim, True, mean, sigma, low, high, flags, G, K, H, A, 0.6, 3, 5)
    assert np.array_equal(_bits(again), _bits(got))
    if G > 1:                                                             # group 0 is a function of its own nominal and deviations
        m2, s2 = mean.copy(), sigma.copy()
        m2[1:], s2[1:] = 0.1, 0.2
        other, _ = _sample(usim, True, m2, s2, low, high, flags, G, K, H, A, 0.6, 3, 5)
        assert np.array_equal(_bits(other[:, :K]), _bits(got[:, :K]))
        if K > 1:
            assert not np.array_equal(_bits(other[:, K:2 * K]), _bits(got[:, K:2 * K])) or G == 2   # (the last group is restarted: sampled around zero in both)


# ---- usim_score_block_tail -----------------------------------------------------------------------------------------------------------------------
GAMMA = float(np.float32(0.97))
RET_VAR, EPS = 66170.04861747491, 1e-8


def _block(T, n, shift=0):
    """environment i: (i + shift) % 3 == 0 never ends, 1 ends on the first step, 2 ends on the last step; NaN tails under the ended ones"""
    rng = np.random.default_rng(10 * T + n + shift)
    rew = rng.standard_normal((T, n)).astype(np.float32)
    done = np.zeros((T, n), dtype=np.uint8)
    kind = (np.arange(n) + shift) % 3
    done[0, kind == 1] = 1
    done[T - 1, kind == 2] = 255
    tail = (rng.standard_normal(n) * 3).astype(np.float32)
    tail[kind != 0] = np.nan
    if T > 1:
        rew[1:, kind == 1] = np.nan                                       # behind a first done: not read
    return rew, done, tail, kind


def _score(usim, rew, done, gamma, tail, ret_var, epsilon=EPS, plain=False):
    lib = usim._lib.load()
    T, n = rew.shape
    r, d = _dev(rew), _dev(done)
    ret, r_ok = _guarded(np.full(n, SENT, dtype=np.float32))
    ln, l_ok = _guarded(np.full(n, -5, dtype=np.int32))
    tl = None if tail is None else _dev(tail)
    rv = None if ret_var is None else _dev(np.array([ret_var], dtype=np.float64))
    if plain:
        rc = lib.usim_score_block(r.data_ptr(), d.data_ptr(), T, n, gamma, ret.data_ptr(), ln.data_ptr(), _stream())
    else:
        rc = lib.usim_score_block_tail(r.data_ptr(), d.data_ptr(), T, n, gamma, None if tl is None else tl.data_ptr(), None if rv is None else rv.data_ptr(),
                                       epsilon, ret.data_ptr(), ln.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and r_ok() and l_ok()
    return ret[:n].cpu().numpy(), ln[:n].cpu().numpy()


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("T", [1, 3])
def test_score_block_tail_bit_for_bit(usim, T, n):
    for shift in ((0, 1, 2) if n == 1 else (0,)):
        rew, done, tail, kind = _block(T, n, shift)
        base, base_len = _score(usim, rew, done, GAMMA, None, None, plain=True)
        for ret_var in (RET_VAR, None):
            want, want_len = Q.score_block_tail(rew, done, GAMMA, tail, ret_var, EPS)
            got, got_len = _score(usim, rew, done, GAMMA, tail, ret_var)
            assert np.array_equal(got_len, want_len) and np.array_equal(got_len, base_len)
            assert np.array_equal(_bits(got), _bits(want))
            assert np.isfinite(got).all()                                 # the NaN tails lie under ended environments
            assert np.array_equal(_bits(got[kind != 0]), _bits(base[kind != 0]))
            if (kind == 0).any() and T == 3:
                assert not np.array_equal(_bits(got[kind == 0]), _bits(base[kind == 0]))
            again, _ = _score(usim, rew, done, GAMMA, tail, ret_var)
            assert np.array_equal(_bits(again), _bits(got))
        # without a tail: usim_score_block, bit for bit, whatever ret_var says
        for ret_var in (RET_VAR, None):
            none, none_len = _score(usim, rew, done, GAMMA, None, ret_var)
            assert np.array_equal(_bits(none), _bits(base)) and np.array_equal(none_len, base_len)
        # an environment's result is its own: every other column replaced
        if n > 1:
            i = int(np.flatnonzero(kind == 0)[-1])
            rew2, done2, tail2, _ = _block(T, n, shift + 1)
            rew2[:, i], done2[:, i], tail2[i] = rew[:, i], done[:, i], tail[i]
            got, _ = _score(usim, rew, done, GAMMA, tail, RET_VAR)
            other, _ = _score(usim, rew2, done2, GAMMA, tail2, RET_VAR)
            assert _bits(got)[i] == _bits(other)[i]


def test_a_survivors_bad_tail_is_a_bad_return(usim):
    rew, done, tail, kind = _block(3, 65)
    tail = tail.copy()
    tail[0], tail[3] = np.inf, np.nan
    got, _ = _score(usim, rew, done, GAMMA, tail, RET_VAR)
    assert not np.isfinite(got[0]) and not np.isfinite(got[3]) and np.isfinite(got[1:3]).all() and np.isfinite(got[4:]).all()


# ---- usim_plan_tail --------------------------------------------------------------------------------------------------------------------------
def _tail_problem(G, K, H, A):
    cand, ret, _, _, low, high = _problem(G, K, H, A)
    rng = np.random.default_rng(3 * G + K)
    n = G * K
    pol = rng.uniform(low, high, (n, A)).astype(np.float32)
    lengths = np.full(n, H, dtype=np.int32)
    done_last = np.zeros(n, dtype=np.uint8)
    kind = np.arange(n) % 4                                               # 0, 3: survived; 1: ended early (H > 1); 2: ended on step H
    lengths[kind == 1] = max(H - 1, 1)
    done_last[kind == 2] = 1
    if H == 1:
        done_last[kind == 1] = 1                                          # (a one-step plan: every end is on step H)
    pol[kind == 1], pol[kind == 2] = np.nan, np.nan                       # never read
    upd = R.update(cand, ret, low, high, K, 0.7)
    return cand, pol, lengths, done_last, upd["weights"].astype(np.float32), upd["best"].astype(np.int32), low, high


def _tail(usim, cand, w, best, lengths, done_last, pol, low, high, G, K, H, A, temperature):
    lib = usim._lib.load()
    mean, ok = _guarded(np.full((G, H, A), 7.0, dtype=np.float32))
    t = [_dev(x) for x in (cand, w, best, lengths, done_last, pol, low, high)]
    rc = lib.usim_plan_tail(*(x.data_ptr() for x in t), G, K, H, A, temperature, mean.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and ok()
    out = mean[:G * H * A].cpu().numpy().reshape(G, H, A)
    assert (out[:, :H - 1] == 7.0).all()                                  # no other word of the nominal is written
    return out[:, H - 1]


@pytest.mark.parametrize("G,K,H,A", SHAPES)
def test_tail_against_the_reference(usim, G, K, H, A):
    cand, pol, lengths, done_last, w, best, low, high = _tail_problem(G, K, H, A)
    ref = Q.plan_tail(cand, w, best, lengths, done_last, pol, low, high, K, 0.7)
    got = _tail(usim, cand, w, best, lengths, done_last, pol, low, high, G, K, H, A, 0.7)
    err = np.abs(got.astype(np.float64) - ref["tail"])
    print("worst error", err.max(), "worst error / bound", float(np.max(np.where(err == 0, 0, err / np.maximum(ref["b_tail"], 1e-300)))))
    assert np.isfinite(got).all() and np.all(err <= ref["b_tail"])
    again = _tail(usim, cand, w, best, lengths, done_last, pol, low, high, G, K, H, A, 0.7)
    assert np.array_equal(_bits(again), _bits(got))
    # temperature 0: the best candidate's x, bit for bit -- for every candidate of the group as "best", so both sources of x are selected
    for k in sorted({0, K // 2, K - 1, min(1, K - 1), min(2, K - 1), min(3, K - 1)}):
        pick = np.full(G, k, dtype=np.int32)
        sel = Q.plan_tail(cand, w, pick, lengths, done_last, pol, low, high, K, 0.0)
        got0 = _tail(usim, cand, w, pick, lengths, done_last, pol, low, high, G, K, H, A, 0.0)
        assert sel["exact"] and np.array_equal(_bits(got0), _bits(sel["tail"].astype(np.float32)))
    if G > 1:                                                             # group 0 is a function of its own candidates
        rng = np.random.default_rng(2)
        c2, p2, w2 = cand.copy(), pol.copy(), w.copy()
        c2[:, K:], p2[K:] = rng.uniform(low, high, (H, (G - 1) * K, A)).astype(np.float32), 0.25
        w2[K:] = np.float32(1.0 / K)
        other = _tail(usim, c2, w2, best, lengths, done_last, p2, low, high, G, K, H, A, 0.7)
        assert np.array_equal(_bits(other[0]), _bits(got[0])) and not np.array_equal(_bits(other[1]), _bits(got[1]))


def test_tail_skips_a_candidate_without_weight(usim):
    G, K, H, A = 3, 5, 4, 7
    cand, pol, lengths, done_last, w, best, low, high = _tail_problem(G, K, H, A)
    assert lengths[0] == H and done_last[0] == 0 and lengths[4] == H and done_last[4] == 0
    w, pol = w.copy(), pol.copy()
    w[:K] = [0.0, 0.25, 0.25, 0.0, 0.5]
    pol[0], pol[3] = np.nan, np.inf                                       # survivors that carry no weight
    ref = Q.plan_tail(cand, w, best, lengths, done_last, pol, low, high, K, 0.7)
    got = _tail(usim, cand, w, best, lengths, done_last, pol, low, high, G, K, H, A, 0.7)
    assert np.isfinite(got).all() and np.all(np.abs(got - ref["tail"]) <= ref["b_tail"])
    assert (_tail(usim, cand, w, np.array([-1, K, 2], dtype=np.int32), lengths, done_last, pol, low, high, G, K, H, A, 0.0)[:2] == 7.0).all()   # a best outside the group
