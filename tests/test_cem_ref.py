"""The numpy reference of the guided planner's kernels (tests/cem_ref.py) checked on its own, without a GPU: what the GPU tests compare the kernels with must
itself be the stated arithmetic."""
from fractions import Fraction

import numpy as np

import cem_ref as Q
import plan_ref as R

LOW, HIGH = np.full(6, -1.0, dtype=np.float32), np.full(6, 1.0, dtype=np.float32)


def _problem(G=3, K=7, H=4, A=6, seed=0):
    rng = np.random.default_rng(seed)
    cand = rng.uniform(-1, 1, (H, G * K, A)).astype(np.float32)
    ret = rng.normal(0, 3, G * K).astype(np.float32)
    mean = rng.uniform(-0.5, 0.5, (G, H, A)).astype(np.float32)
    sigma = rng.uniform(0.1, 0.4, (G, H, A)).astype(np.float32)
    return cand, ret, mean, sigma


def test_fmaf32_is_the_rounding_of_the_exact_value():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(2000).astype(np.float32), rng.standard_normal(2000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.choice([0.0, 2.0**-25, 2.0**-30, 1.0], 2000))).astype(np.float32)   # cancellation and near-ties
    a[:3], b[:3], c[:3] = [1.0, 1.0, 3.0], [1.0 + 2.0**-23, 1.0 + 2.0**-23, 1.0 / 3.0], [2.0**-24, 2.0**-60, 2.0**-24]
    got = Q.fmaf32(a, b, c)
    for x, y, z, r in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        d = abs(Fraction(float(r)) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact)
        if d == abs(Fraction(float(lo)) - exact) or d == abs(Fraction(float(hi)) - exact):
            assert (np.float32(r).view(np.int32) & 1) == 0                 # a tie goes to the even neighbour


def test_all_elites_without_momentum_is_the_plain_mean_and_deviation():
    cand, ret, mean, sigma = _problem()
    o = Q.refit(cand, ret, LOW, HIGH, 7, 7, 0.0, 1e-6, mean, sigma)
    c = cand.astype(np.float64).reshape(4, 3, 7, 6)
    assert np.array_equal(o["elite"], np.tile(np.arange(7, dtype=np.int32), (3, 1)))
    assert np.allclose(o["mean"], c.mean(axis=2).transpose(1, 0, 2), rtol=0, atol=1e-15)
    assert np.allclose(o["sigma"], c.std(axis=2).transpose(1, 0, 2), rtol=0, atol=1e-15)
    assert np.all(o["b_mean"] > 0) and np.all(o["b_mean"] < 1e-5) and np.all(o["b_sigma"] > 0) and np.all(o["b_sigma"] < 1e-4)


def test_momentum_and_floor():
    cand, ret, mean, sigma = _problem()
    o0 = Q.refit(cand, ret, LOW, HIGH, 7, 3, 0.0, 1e-6, mean, sigma)
    o = Q.refit(cand, ret, LOW, HIGH, 7, 3, 0.25, 1e-6, mean, sigma)
    assert np.allclose(o["mean"], np.clip(0.25 * mean + 0.75 * o0["mean"], -1, 1), rtol=0, atol=1e-15)
    assert np.allclose(o["sigma"], 0.25 * sigma + 0.75 * o0["sigma"], rtol=0, atol=1e-15)
    one = Q.refit(cand, ret, LOW, HIGH, 7, 1, 0.0, 0.05, mean, sigma)      # one elite: no spread, sigma is the floor; the mean is that candidate
    assert np.all(one["sigma"] == float(np.float32(0.05)))
    for g in range(3):
        k = one["elite"][g, 0]
        assert k == np.argmax(ret[7 * g:7 * g + 7]) and np.array_equal(one["mean"][g], cand[:, 7 * g + k, :].astype(np.float64))


def test_ties_go_to_the_lower_index_and_the_list_ascends():
    ret = np.array([1.0, 5.0, 5.0, 2.0, 5.0, 5.0, -1.0], dtype=np.float32)
    assert Q.elite_set(ret, 7, 1).tolist() == [[1]]
    assert Q.elite_set(ret, 7, 3).tolist() == [[1, 2, 4]]
    assert Q.elite_set(ret, 7, 5).tolist() == [[1, 2, 3, 4, 5]]            # the fifth is the 2.0 at index 3: listed by index, not by rank
    assert Q.elite_set(np.array([0.0, -0.0, 0.0], dtype=np.float32), 3, 2).tolist() == [[0, 1]]          # -0 == 0: a tie


def test_non_finite_returns_are_never_elite():
    ret = np.array([np.inf, 3.0, np.nan, -np.inf, 1.0, 2.0, np.nan], dtype=np.float32)
    assert Q.elite_set(ret, 7, 2).tolist() == [[1, 5]]
    assert Q.elite_set(ret, 7, 7).tolist() == [[1, 4, 5, -1, -1, -1, -1]]  # min(elites, finite returns) of them, padded with -1


def test_a_group_without_a_finite_return_keeps_mean_and_sigma():
    cand, ret, mean, sigma = _problem()
    ret[7:14] = [np.nan, np.inf, -np.inf, np.nan, np.nan, np.inf, np.nan]
    o = Q.refit(cand, ret, LOW, HIGH, 7, 3, 0.5, 1e-3, mean, sigma)
    assert (o["elite"][1] == -1).all() and (o["elite"][[0, 2]] >= 0).all()
    assert np.array_equal(o["mean"][1], mean[1].astype(np.float64)) and np.array_equal(o["sigma"][1], sigma[1].astype(np.float64))
    assert not np.array_equal(o["mean"][0], mean[0].astype(np.float64))
    assert (o["b_mean"][1] == 0).all() and (o["b_sigma"][1] == 0).all()


def test_a_zero_tail_is_score_block():
    rng = np.random.default_rng(2)
    T, n = 5, 40
    rew = rng.standard_normal((T, n)).astype(np.float32)
    done = (rng.uniform(size=(T, n)) < 0.1).astype(np.uint8)
    base, length, disc, alive = Q.score_block(rew, done, 0.99)
    assert alive.any() and (~alive).any()
    for tail in (None, np.zeros(n, dtype=np.float32)):
        ret, ln = Q.score_block_tail(rew, done, 0.99, tail, ret_var=4.0, epsilon=1e-8)
        assert np.array_equal(ret.view(np.int32), base.view(np.int32)) and np.array_equal(ln, length)
    any_done = done.any(axis=0)
    assert np.array_equal(length, np.where(any_done, done.argmax(axis=0) + 1, T))
    live = np.arange(T)[:, None] < length[None, :]
    ret64 = (np.where(live, rew, 0).astype(np.float64) * (float(np.float32(0.99)) ** np.arange(T))[:, None]).sum(axis=0)
    assert np.allclose(base, ret64, rtol=0, atol=2 * T * 2.0**-24 * np.abs(rew).sum(axis=0).max())


def test_the_tail_reaches_survivors_only_and_in_raw_reward_units():
    rng = np.random.default_rng(3)
    T, n = 3, 16
    rew = rng.standard_normal((T, n)).astype(np.float32)
    done = np.zeros((T, n), dtype=np.uint8)
    done[0, 0], done[T - 1, 1] = 1, 1
    tail = rng.standard_normal(n).astype(np.float32)
    tail[0], tail[1] = np.nan, np.nan                                      # under ended environments: never read
    base, _, disc, alive = Q.score_block(rew, done, 0.9)
    ret, _ = Q.score_block_tail(rew, done, 0.9, tail, ret_var=8.999999, epsilon=1e-6)
    assert Q.tail_scale(8.999999, 1e-6) == np.float32(3.0) and Q.tail_scale(None, 5.0) == np.float32(1.0)
    assert np.array_equal(ret[:2].view(np.int32), base[:2].view(np.int32)) and np.isfinite(ret).all()
    g = np.float32(0.9)
    assert (disc[2:] == g * g * g).all()                                   # the loop's own running discount, ((1 g) g) g in float32
    want = base[2:].astype(np.float64) + float(g * g * g) * 3.0 * tail[2:].astype(np.float64)
    assert np.allclose(ret[2:], want, rtol=0, atol=2.0**-22 * (np.abs(want) + 3 * np.abs(tail[2:])))
    tail[5] = np.inf
    assert not np.isfinite(Q.score_block_tail(rew, done, 0.9, tail)[0][5])   # a survivor's non-finite tail is a non-finite return


def test_sample_elem_with_a_broadcast_sigma_is_the_sampler():
    rng = np.random.default_rng(4)
    G, K, H, A = 2, 5, 3, 6
    mean = rng.uniform(-0.5, 0.5, (G, H, A)).astype(np.float32)
    sigma = rng.uniform(0.1, 0.4, A).astype(np.float32)
    a = R.sample(mean, sigma, LOW, HIGH, [0, 1], K, 0.5, 9, 2)
    b = Q.sample_elem(mean, np.broadcast_to(sigma, (G, H, A)), LOW, HIGH, [0, 1], K, 0.5, 9, 2)
    for key in ("cand", "bound", "mean_after"):
        assert np.array_equal(a[key], b[key])
    wide = np.broadcast_to(sigma, (G, H, A)).copy()
    wide[1, 2] *= 2                                                        # one element: only (group 1, step 2) moves
    c = Q.sample_elem(mean, wide, LOW, HIGH, [0, 1], K, 0.5, 9, 2)
    diff = c["cand"] != a["cand"]
    assert diff[2, K:].any() and not diff[:2].any() and not diff[:, :K].any()


def test_plan_tail_takes_the_actor_where_the_candidate_survived():
    rng = np.random.default_rng(6)
    G, K, H, A = 2, 5, 3, 6
    cand = rng.uniform(-1, 1, (H, G * K, A)).astype(np.float32)
    pol = rng.uniform(-1, 1, (G * K, A)).astype(np.float32)
    lengths = np.full(G * K, H, dtype=np.int32)
    done_last = np.zeros(G * K, dtype=np.uint8)
    lengths[1], done_last[2] = 2, 1                                        # ended early; ended on step H (length == H all the same)
    pol[1], pol[2] = np.nan, np.nan
    x, alive = Q.tail_rows(cand, lengths, done_last, pol)
    assert not alive[1] and not alive[2] and alive.sum() == G * K - 2
    assert np.array_equal(x[1], cand[H - 1, 1]) and np.array_equal(x[2], cand[H - 1, 2]) and np.array_equal(x[3], pol[3])
    w = rng.uniform(size=(G, K)).astype(np.float32)
    w /= w.sum(axis=1, keepdims=True)
    o = Q.plan_tail(cand, w.reshape(-1), [0, 0], lengths, done_last, pol, LOW, HIGH, K, 1.0)
    assert np.allclose(o["tail"], np.einsum("gk,gka->ga", w.astype(np.float64), x.astype(np.float64).reshape(G, K, A)), rtol=0, atol=1e-15)
    assert np.all(o["b_tail"] > 0) and np.all(o["b_tail"] < 1e-5) and not o["exact"]
    sel = Q.plan_tail(cand, w.reshape(-1), [2, 4], lengths, done_last, pol, LOW, HIGH, K, 0.0)
    assert sel["exact"] and np.array_equal(sel["tail"][0], cand[H - 1, 2].astype(np.float64)) and np.array_equal(sel["tail"][1], pol[K + 4].astype(np.float64))
    pol[3] = np.nan                                                        # a survivor without weight adds nothing, whatever its action
    w0 = w.copy()
    w0[0, 3] = 0
    assert np.isfinite(Q.plan_tail(cand, w0.reshape(-1), [0, 0], lengths, done_last, pol, LOW, HIGH, K, 1.0)["tail"]).all()
