"""The float64 reference of the planner kernels (tests/plan_ref.py) checked on its own, without a GPU: what the GPU tests compare the kernels with must itself
be the stated planner."""
import numpy as np

import plan_ref as R

LOW, HIGH = np.full(6, -1.0, dtype=np.float32), np.full(6, 1.0, dtype=np.float32)


def _problem(G=3, K=7, H=4, A=6, seed=0):
    rng = np.random.default_rng(seed)
    cand = rng.uniform(-1, 1, (H, G * K, A)).astype(np.float32)
    ret = rng.normal(0, 3, G * K).astype(np.float32)
    return cand, ret


def test_weights_sum_to_one_and_are_bounded():
    cand, ret = _problem()
    ret[3], ret[9], ret[10] = np.nan, np.inf, -np.inf
    for T in (1e-2, 1.0, 1e3):
        o = R.update(cand, ret, LOW, HIGH, 7, T)
        w = o["weights"].reshape(3, 7)
        assert np.allclose(w.sum(1), 1.0, rtol=0, atol=1e-12)
        assert w[0, 3] == 0 and w[1, 2] == 0 and w[1, 3] == 0          # non-finite returns carry no weight
        assert np.all(o["b_weights"] >= 0) and np.all(o["b_weights"] < 1e-4) and np.all(o["b_plan"] < 1e-4)
        assert np.all(o["plan"] >= -1) and np.all(o["plan"] <= 1)
        assert np.array_equal(o["act"], o["plan"][:, 0])
        assert np.array_equal(o["next_mean"][:, :-1], o["plan"][:, 1:]) and np.array_equal(o["next_mean"][:, -1], o["plan"][:, -1])


def test_temperature_zero_is_the_argmax_with_the_lowest_index_tie():
    cand, ret = _problem()
    ret[7:14] = [1.0, 5.0, np.inf, 5.0, np.nan, 5.0, -2.0]                 # group 1: three equal best returns, an infinite one that does not count
    ret[14:21] = np.nan                                                    # group 2: nothing finite
    o = R.update(cand, ret, LOW, HIGH, 7, 0.0)
    assert o["exact"]
    assert o["best"][0] == int(np.argmax(ret[:7])) and o["best"][1] == 1 and o["best"][2] == 0
    w = o["weights"].reshape(3, 7)
    for g in range(3):
        assert w[g].sum() == 1.0 and w[g, o["best"][g]] == 1.0
        assert np.array_equal(o["plan"][g], cand[:, g * 7 + o["best"][g], :].astype(np.float64))
    assert not o["b_weights"].any() and not o["b_plan"].any()
    o1 = R.update(cand, ret, LOW, HIGH, 7, 1.0)                            # with a temperature the dead group still puts everything on candidate 0
    assert np.array_equal(o1["weights"][14:21], [1, 0, 0, 0, 0, 0, 0])


def test_candidate_zero_is_the_clipped_nominal():
    rng = np.random.default_rng(1)
    mean = rng.uniform(-2, 2, (2, 5, 6)).astype(np.float32)                # some words outside the box
    mean[1, 2, 3] = np.nan
    o = R.sample(mean, np.full(6, 0.5), LOW, HIGH, None, 4, 0.7, seed=9, counter=2)
    want = np.clip(np.where(np.isfinite(mean), mean, 0).astype(np.float64), -1, 1)
    for g in range(2):
        assert np.array_equal(o["cand"][:, g * 4, :], want[g])
        assert not o["bound"][:, g * 4, :].any()
    assert np.any(o["cand"][:, 1, :] != o["cand"][:, 0, :])
    assert np.array_equal(o["mean_after"].view(np.uint32), mean.view(np.uint32))          # without restart flags the nominal is not written
    r = R.sample(mean, np.full(6, 0.5), LOW, HIGH, [0, 1], 4, 0.7, seed=9, counter=2)
    assert not r["mean_after"][1].any() and np.array_equal(r["mean_after"][0].view(np.uint32), mean[0].view(np.uint32))
    assert not r["cand"][:, 4, :].any()                                                   # the restarted group's nominal candidate is zero
    assert np.array_equal(r["cand"][:, :4], o["cand"][:, :4])


def test_a_huge_temperature_gives_the_plain_mean():
    cand, ret = _problem()
    o = R.update(cand, ret, np.full(6, -9), np.full(6, 9), 7, 1e30)
    plain = cand.astype(np.float64).reshape(4, 3, 7, 6).mean(axis=2).transpose(1, 0, 2)
    assert np.allclose(o["plan"], plain, rtol=0, atol=1e-12)
    assert np.allclose(o["weights"], 1 / 7, rtol=0, atol=1e-12)


def test_the_first_two_moments_of_the_noise():
    """N = 2^16 draws of xi: the mean of N(0, 1) has standard error 1 / sqrt(N); xi^2 has variance 2, so the second moment has standard error sqrt(2 / N).  Both
    within 5 standard errors."""
    xi, rad = R.plan_noise(seed=0x1234567890abcdef, candidates=np.arange(1, 1 + 2**16 // (8 * 8)), horizon=8, adim=8, counter=3)
    assert xi.size == 2**16
    assert abs(xi.mean()) <= 5 / np.sqrt(xi.size)
    assert abs((xi**2).mean() - 1.0) <= 5 * np.sqrt(2.0 / xi.size)
    even, odd = xi[..., 0::2], xi[..., 1::2]                               # the two components of a pair share a radius: cosine and sine of one angle
    assert np.allclose(even**2 + odd**2, rad[..., 0::2] ** 2, rtol=1e-12)
    again, _ = R.plan_noise(seed=0x1234567890abcdef, candidates=[5], horizon=3, adim=5, counter=1, base=2)
    assert np.array_equal(again[0], xi[4, :3, :5])                         # a draw depends on (seed, counter + base, candidate, t, a) alone


def test_smoothing_keeps_unit_variance_and_correlates_neighbours():
    mean = np.zeros((1, 6, 8), dtype=np.float32)
    big = np.full(8, 1e9, dtype=np.float32)
    o = R.sample(mean, np.ones(8), -big, big, None, 4097, 0.7, seed=5, counter=0)
    e = o["cand"][:, 1:, :]                                                # [H, K - 1, A] = the smoothed noise itself
    n = e[0].size
    assert abs((e[5] ** 2).mean() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert abs((e[5] * e[4]).mean() - 0.7) <= 5 * np.sqrt((1 + 0.49) / n)  # Var(x y) = 1 + rho^2 for unit normals of correlation rho
