"""The planner kernels (csrc/usim_plan.hip) through their C ABI, against the float64 restatement in tests/plan_ref.py: crafted tensors, no env handle.  Every bar
is the bound plan_ref derives from the kernels' operation sequence (its module docstring); integers, selections and everything the contract calls "bit for bit"
are compared exactly.  GUARD sentinel words stand behind every output: a write past its end shows up as a changed guard.  The worst observed margin
(error / bound) of every bar is printed at the end of the module (pytest -s).  Measured on one MI355X over the whole module:
  candidates 0.49 (smoothing 0 and 0.7), 0.46 with restart flags, 0.015 at sigma 100; a bare draw 0.27
  weights 0.17 / 0.15 / 0.14 and plan 0.082 / 0.10 / 0.080 at temperatures 1e-2 / 1 / 1e3
No bar needed loosening beyond its derivation."""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25e33
GUARD = 64
MARGINS = {}


def _margin(name, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))      # (an exact word under a zero bound is margin 0)
    m = float(ratio.max())
    MARGINS[name] = max(MARGINS.get(name, 0.0), m)
    assert np.all(err <= bound), f"{name}: worst error / bound {m:.3g} at {np.unravel_index(np.argmax(ratio), err.shape)}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst error / bound per bar:")
    for k in sorted(MARGINS):
        print(f"  {k:28s} {MARGINS[k]:.3g}")


@pytest.fixture(scope="module")
def lib(usim):
    return usim._lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _guarded(a=None, words=None, dtype=torch.float32):
    """a device buffer of the words of `a` (or `words` sentinel words) with GUARD sentinel words behind"""
    fill = SENTINEL if dtype == torch.float32 else -77
    n = int(np.asarray(a).size) if a is not None else int(words)
    t = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    if a is not None:
        t[:n] = _dev(np.asarray(a).reshape(-1), dtype)
    return t


def _read(t, shape, name):
    a = t.cpu().numpy()
    n = int(np.prod(shape))
    assert np.all(a[n:] == a.dtype.type(SENTINEL if a.dtype == np.float32 else -77)), f"{name}: a word behind its end was written"
    return a[:n].reshape(shape).copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


BOX6 = (np.array([0, 0, 0, 0, 0, 0], dtype=np.float32), np.array([1, 1, 1, 1, 1, 1], dtype=np.float32))
BOX7 = (np.array([0, 0, 0, 0, 0, 0, -1], dtype=np.float32), np.array([1, 1, 1, 1, 1, 1, 1], dtype=np.float32))
BOX = {6: BOX6, 7: BOX7}


def run_sample(lib, mean, sigma, low, high, restart, K, smoothing, seed, counter, base=None):
    """-> (cand [H, n, A], mean afterwards [G, H, A]) float32"""
    G, H, A = mean.shape
    n = G * K
    mean_t, cand_t = _guarded(mean), _guarded(words=H * n * A)
    sig_t, lo_t, hi_t = _dev(sigma), _dev(low), _dev(high)
    rs_t = None if restart is None else _dev(restart, torch.uint8)
    base_t = None if base is None else torch.tensor([base], dtype=torch.int64, device=DEV).to(torch.int32)
    rc = lib.usim_plan_sample(mean_t.data_ptr(), sig_t.data_ptr(), lo_t.data_ptr(), hi_t.data_ptr(), None if rs_t is None else rs_t.data_ptr(), G, K, H, A,
                              float(smoothing), int(seed), int(counter), None if base_t is None else base_t.data_ptr(), cand_t.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _read(cand_t, (H, n, A), "cand"), _read(mean_t, (G, H, A), "mean")


def run_update(lib, cand, ret, low, high, K, temperature, outputs=("plan", "next_mean", "best", "weights")):
    """-> dict of float32 / int32 arrays: plan, next_mean [G, H, A], act [G, A], best [G], weights [n] (those asked for)"""
    H, n, A = cand.shape
    G = n // K
    cand_t, ret_t, lo_t, hi_t = _dev(cand), _dev(ret), _dev(low), _dev(high)
    shapes = dict(plan=(G, H, A), next_mean=(G, H, A), act=(G, A), best=(G,), weights=(n,))
    buf = {k: _guarded(words=int(np.prod(shapes[k])), dtype=torch.int32 if k == "best" else torch.float32) for k in ("act",) + tuple(outputs)}
    p = lambda k: buf[k].data_ptr() if k in buf else None
    rc = lib.usim_plan_update(cand_t.data_ptr(), ret_t.data_ptr(), lo_t.data_ptr(), hi_t.data_ptr(), G, K, H, A, float(temperature), p("plan"), p("next_mean"),
                              p("act"), p("best"), p("weights"), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {k: _read(t, shapes[k], k) for k, t in buf.items()}


# ================================================================ the sampler ================================================================
def _mean(G, H, A, seed):
    rng = np.random.default_rng(seed)
    lo, hi = BOX[A]
    return (lo + rng.uniform(-0.2, 1.2, (G, H, A)) * (hi - lo)).astype(np.float32)          # some words outside the box


def check_sample(cand, ref, K, tag):
    nominal = np.arange(cand.shape[1]) % K == 0
    assert np.array_equal(_bits(cand[:, nominal]), _bits(ref["cand"][:, nominal])), "candidate 0 is not the clipped nominal " + tag
    _margin("candidates " + tag, np.abs(cand.astype(np.float64) - ref["cand"]), ref["bound"])


@pytest.mark.parametrize("smoothing", [0.0, 0.7])
@pytest.mark.parametrize("G, K, H, A", [(1, 1, 1, 6), (3, 5, 4, 7), (2, 257, 3, 6)])
def test_sample_against_the_reference(lib, G, K, H, A, smoothing):
    mean = _mean(G, H, A, seed=G * K)
    low, high = BOX[A]
    sigma = np.linspace(0.05, 0.6, A).astype(np.float32)
    cand, after = run_sample(lib, mean, sigma, low, high, None, K, smoothing, seed=0x9e3779b97f4a7c15, counter=11)
    ref = R.sample(mean, sigma, low, high, None, K, smoothing, seed=0x9e3779b97f4a7c15, counter=11)
    check_sample(cand, ref, K, f"s={smoothing}")
    assert np.array_equal(_bits(after), _bits(mean))                      # without restart flags the nominal is not written
    assert np.all(cand >= low) and np.all(cand <= high)
    if K > 1:
        inside = (cand > low) & (cand < high)
        assert inside[:, np.arange(G * K) % K != 0].mean() > 0.3          # (the comparison is not one of clipped words only)


def test_sample_large_sigma_leaves_the_box_on_both_sides(lib):
    G, K, H, A = 3, 5, 4, 7
    mean = _mean(G, H, A, seed=2)
    low, high = BOX[A]
    sigma = np.full(A, 100.0, dtype=np.float32)
    cand, _ = run_sample(lib, mean, sigma, low, high, None, K, 0.7, seed=5, counter=0)
    ref = R.sample(mean, sigma, low, high, None, K, 0.7, seed=5, counter=0)
    check_sample(cand, ref, K, "large sigma")
    for a in range(A):
        assert np.any(cand[..., a] == low[a]) and np.any(cand[..., a] == high[a]), a
    assert np.isin(cand[:, np.arange(G * K) % K != 0], np.concatenate([low, high])).mean() > 0.95


def test_sample_restart_and_nan(lib):
    G, K, H, A = 3, 5, 4, 6
    mean = _mean(G, H, A, seed=3)
    mean[0, 1, 2], mean[2, 3, 5], mean[2, 0, 0] = np.nan, np.inf, -np.inf
    low, high = BOX[A]
    sigma = np.full(A, 0.25, dtype=np.float32)
    restart = np.array([0, 7, 0], dtype=np.uint8)                         # any non-zero byte
    cand, after = run_sample(lib, mean, sigma, low, high, restart, K, 0.0, seed=5, counter=1)
    ref = R.sample(mean, sigma, low, high, restart, K, 0.0, seed=5, counter=1)
    check_sample(cand, ref, K, "restart")
    assert not _bits(after[1]).any()                                      # the restarted group's nominal reads back as zeros (+0.0)
    assert np.array_equal(_bits(after[0]), _bits(mean[0])) and np.array_equal(_bits(after[2]), _bits(mean[2]))      # the others unchanged, the NaN included
    assert np.array_equal(_bits(after), _bits(ref["mean_after"]))
    assert not cand[:, K, :].any()                                        # its candidate 0 is clip(0) = 0
    assert cand[1, 0, 2] == 0.0 and np.isfinite(cand).all()               # a non-finite word of the nominal counts as 0


def test_sample_counter_base(lib):
    G, K, H, A = 2, 5, 3, 6
    mean = _mean(G, H, A, seed=4)
    low, high = BOX[A]
    sigma = np.full(A, 0.25, dtype=np.float32)
    args = (lib, mean, sigma, low, high, None, K, 0.7)
    a, _ = run_sample(*args, seed=8, counter=3, base=5)
    b, _ = run_sample(*args, seed=8, counter=8, base=0)
    c, _ = run_sample(*args, seed=8, counter=8)
    d, _ = run_sample(*args, seed=8, counter=3, base=0)
    w, _ = run_sample(*args, seed=8, counter=2**32 - 2, base=10)          # the sum wraps modulo 2^32
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)) and np.array_equal(_bits(a), _bits(w))
    assert not np.array_equal(_bits(a), _bits(d))
    e, _ = run_sample(*args, seed=8 + 2**32, counter=8)                   # the high word of the seed is part of the key
    assert not np.array_equal(_bits(a), _bits(e))


def test_a_draw_does_not_depend_on_the_shape_around_it(lib):
    """mean 0, sigma 1, a box nobody reaches, no smoothing: cand[t][c][a] IS the draw xi(c, t, a), for every candidate that is not a group's nominal"""
    A = 6
    big = np.full(A, 1e9, dtype=np.float32)
    one = np.ones(A, dtype=np.float32)
    runs = {}
    for G, K, H in ((3, 5, 4), (1, 15, 2), (5, 3, 6), (1, 300, 4)):
        runs[(G, K, H)] = run_sample(lib, np.zeros((G, H, A), dtype=np.float32), one, -big, big, None, K, 0.0, seed=21, counter=4)[0]
    base = runs[(1, 300, 4)]
    xi, rad = R.plan_noise(21, np.arange(300), 4, A, 4)
    _margin("draw", np.abs(base[:, 1:].transpose(1, 0, 2) - xi[1:]), (np.abs(xi) * (R.REL_RAD + R.U24) + rad * R.TRIG)[1:])
    assert abs(base[:, 1:].std() - 1.0) < 0.05
    compared = 0
    for (G, K, H), c in runs.items():
        T = min(H, 4)
        for cand in range(G * K):
            if cand % K and cand % 300:
                assert np.array_equal(_bits(c[:T, cand]), _bits(base[:T, cand])), (G, K, H, cand)
                compared += 1
    assert compared > 300


# ================================================================ the update ================================================================
def _update_problem(K, H, A, seed):
    """three groups: group 0 carries ties, +-inf and a NaN (where K allows), group 1 is plain, group 2 has no finite return"""
    rng = np.random.default_rng(seed)
    low, high = BOX[A]
    n = 3 * K
    cand = (low + rng.uniform(0, 1, (H, n, A)) * (high - low)).astype(np.float32)
    ret = rng.normal(0, 3, n).astype(np.float32)
    if K >= 5:
        top = np.float32(ret[:K].max() + 1)
        ret[K - 1], ret[2], ret[K // 2] = top, top, top                   # a three-way tie for the best: index 2 wins
        ret[0], ret[1], ret[3] = np.inf, np.nan, -np.inf
        ret[K + 3] = ret[K + 1]                                           # a tie below the best of group 1
    ret[2 * K:] = np.nan
    if K > 1:
        ret[2 * K + 1] = np.inf
    return cand, ret, low, high


@pytest.mark.parametrize("A", [6, 7])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("K", [1, 5, 257, 1000])
def test_update_against_the_reference(lib, K, H, A):
    cand, ret, low, high = _update_problem(K, H, A, seed=K + H)
    for T in (0.0, 1e-2, 1.0, 1e3):
        out = run_update(lib, cand, ret, low, high, K, T)
        ref = R.update(cand, ret, low, high, K, T)
        tag = f"T={T:g}"
        assert np.array_equal(out["best"], ref["best"]), tag
        if K >= 5:
            assert out["best"][0] == 2 and out["best"][2] == 0
        w = out["weights"].astype(np.float64)
        dead = ~np.isfinite(ret)
        dead[2 * K] = False
        assert not w[dead].any()                                          # a non-finite return has weight 0 (but candidate 0 of a group without a finite one)
        assert w[2 * K] == 1.0 and not w[2 * K + 1:].any()                # the group without a finite return: everything on candidate 0
        if T == 0.0:
            assert ref["exact"]
            assert np.array_equal(w, ref["weights"]), tag                 # exactly 0 / 1
            for g in range(3):
                assert np.array_equal(_bits(out["plan"][g]), _bits(cand[:, g * K + out["best"][g], :])), (tag, g)      # the chosen candidate's bits
        else:
            _margin("weights " + tag, np.abs(w - ref["weights"]), ref["b_weights"])
            _margin("plan " + tag, np.abs(out["plan"].astype(np.float64) - ref["plan"]), ref["b_plan"])
            assert abs(w[:K].sum() - 1) < 1e-5 and abs(w[K:2 * K].sum() - 1) < 1e-5
            assert np.all(out["plan"] >= low) and np.all(out["plan"] <= high)
        assert np.array_equal(_bits(out["act"]), _bits(out["plan"][:, 0])), tag
        shifted = np.concatenate([out["plan"][:, 1:], out["plan"][:, -1:]], axis=1)
        assert np.array_equal(_bits(out["next_mean"]), _bits(shifted)), tag
        # two runs give the same bits; the optional outputs may be left out
        again = run_update(lib, cand, ret, low, high, K, T, outputs=("plan",))
        assert np.array_equal(_bits(again["plan"]), _bits(out["plan"])) and np.array_equal(_bits(again["act"]), _bits(out["act"])), tag
        # group 1 of 3 equals the same group run alone
        alone = run_update(lib, cand[:, K:2 * K], ret[K:2 * K], low, high, K, T)
        assert alone["best"][0] == out["best"][1], tag
        for k, sl in (("plan", slice(1, 2)), ("next_mean", slice(1, 2)), ("act", slice(1, 2)), ("weights", slice(K, 2 * K))):
            assert np.array_equal(_bits(alone[k]), _bits(out[k][sl])), (tag, k)


def test_update_temperature_spreads_or_selects(lib):
    """between the limits: at 1e3 the weights are near 1 / (finite candidates), at 1e-2 near a selection of the best"""
    K, H, A = 257, 3, 6
    cand, ret, low, high = _update_problem(K, H, A, seed=1)
    ret[:K] = np.random.default_rng(0).normal(0, 3, K).astype(np.float32)                  # group 0 plain as well
    hot = run_update(lib, cand, ret, low, high, K, 1e3)["weights"][:K]
    assert np.abs(hot * K - 1).max() < 0.05
    cold = run_update(lib, cand, ret, low, high, K, 1e-2)
    sel = run_update(lib, cand, ret, low, high, K, 0.0)
    assert cold["weights"][:K].max() > 0.99 and np.argmax(cold["weights"][:K]) == sel["best"][0]
    assert np.abs(cold["plan"][0] - sel["plan"][0]).max() < 0.02
