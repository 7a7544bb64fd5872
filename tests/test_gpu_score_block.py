"""usim_score_block (csrc/usim_score.hip) through its C ABI: caller buffers only, so the blocks are synthetic -- no simulator -- and the expected result is put
together with numpy.

Sizes: one environment and one step; 7 x 100 (a ragged wave); 300 x 257 (a second workgroup that holds one environment); 256 x 4096 (the planner's size).  The done
bytes are planted at step 0, at the last step, nowhere, several per environment (the first counts) and as a byte of 255 (any non-zero byte counts); "mixed" gives
neighbouring environments different patterns, so that the lanes of a wave stop at different steps.  Behind every first done the rewards are NaN: the sum must not see
them.  The output buffers carry guard words behind the last environment."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (7, 100), (300, 257), (256, 4096)]
PATTERNS = ["step0", "last", "none", "several", "byte255", "mixed"]
GUARD = 64
SENT_F, SENT_I = -12345.0, -777
GAMMA = float(np.float32(0.99))                                          # the float32 the kernel receives, as a double


def _done(T, n, pattern, g):
    d = np.zeros((T, n), dtype=np.uint8)
    env = np.arange(n)
    if pattern == "step0":
        d[0] = 1
    elif pattern == "last":
        d[T - 1] = 1
    elif pattern == "several":
        for _ in range(3):
            d[g.integers(0, T, n), env] = 1
    elif pattern == "byte255":
        d[g.integers(0, T, n), env] = 255
        d[g.integers(0, T, n), env] |= 128                              # (a later or earlier byte with only the top bit set)
    elif pattern == "mixed":
        for k, p in enumerate(PATTERNS[:5]):
            d[:, k::5] = _done(T, n, p, g)[:, k::5]
    return d


@functools.lru_cache(maxsize=None)
def _case(T, n, pattern):
    """host block and its expected results, computed once: rew (NaN behind every first done), done, lengths, float32 sequential returns at gamma 1,
    float64 returns at GAMMA and the sum of |gamma^k r_k| that scales their bound"""
    g = np.random.default_rng(1000 * T + n + 17 * PATTERNS.index(pattern))
    rew = g.standard_normal((T, n)).astype(np.float32)
    done = _done(T, n, pattern, g)
    any_done = (done != 0).any(axis=0)
    length = np.where(any_done, (done != 0).argmax(axis=0) + 1, T).astype(np.int32)
    live = np.arange(T)[:, None] < length[None, :]
    rew[~live] = np.nan
    ret1 = np.zeros(n, dtype=np.float32)
    for k in range(T):
        ret1 = np.where(live[k], ret1 + np.where(live[k], rew[k], np.float32(0)), ret1).astype(np.float32)
    terms = np.where(live, rew.astype(np.float64), 0.0) * (GAMMA ** np.arange(T, dtype=np.float64))[:, None]
    return rew, done, length, ret1, terms.sum(axis=0), np.abs(terms).sum(axis=0)


def _score(usim, rew, done, gamma, with_length=True):
    """device call on fresh guarded output buffers -> (returns, lengths or None) as numpy"""
    lib = usim._lib.load()
    T, n = rew.shape
    r = torch.from_numpy(rew).to(DEV)
    d = torch.from_numpy(done).to(DEV)
    ret = torch.full((n + GUARD,), SENT_F, dtype=torch.float32, device=DEV)
    length = torch.full((n + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    rc = lib.usim_score_block(r.data_ptr(), d.data_ptr(), T, n, gamma, ret.data_ptr(), length.data_ptr() if with_length else None,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((ret[n:] == SENT_F).all()) and bool((length[n:] == SENT_I).all())        # nothing behind the last environment
    if not with_length:
        assert bool((length == SENT_I).all())
    return ret[:n].cpu().numpy(), length[:n].cpu().numpy() if with_length else None


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T,n", SIZES)
def test_lengths_and_undiscounted_returns_are_exact(usim, T, n, pattern):
    rew, done, length, ret1, _, _ = _case(T, n, pattern)
    got, got_len = _score(usim, rew, done, 1.0)
    assert np.isfinite(got).all()                                        # no NaN from behind a first done
    assert np.array_equal(got_len, length)
    assert np.array_equal(got.view(np.int32), ret1.view(np.int32))       # fmaf(1, r, ret) is one rounded addition: the float32 loop, bit for bit


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T,n", SIZES)
def test_discounted_returns_within_the_rounding_bound(usim, T, n, pattern):
    """T multiply-adds, each rounded once (2^-24 relative to a partial sum that is at most the sum of the absolute terms), with a discount that carries at most k
    roundings at step k (k <= T, 2^-24 each, relative to its term): to first order 2 T 2^-24 sum |gamma^k r_k|"""
    rew, done, length, _, ret64, scale = _case(T, n, pattern)
    got, got_len = _score(usim, rew, done, GAMMA)
    assert np.isfinite(got).all()
    assert np.array_equal(got_len, length)
    bound = 2.0 * T * 2.0 ** -24 * scale
    err = np.abs(got.astype(np.float64) - ret64)
    print(f"T {T} n {n} {pattern}: max err {err.max():.3e}, bound there {bound[err.argmax()]:.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()


def test_length_output_is_optional(usim):
    rew, done, length, ret1, _, _ = _case(7, 100, "mixed")
    got, _ = _score(usim, rew, done, 1.0, with_length=False)
    assert np.array_equal(got.view(np.int32), ret1.view(np.int32))


def test_recorded_in_a_graph(usim):
    lib = usim._lib.load()
    rew, done, length, _, _, _ = _case(300, 257, "mixed")
    T, n = rew.shape
    eager, eager_len = _score(usim, rew, done, GAMMA)
    r, d = torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV)
    ret = torch.zeros(n, dtype=torch.float32, device=DEV)
    ln = torch.zeros(n, dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc = lib.usim_score_block(r.data_ptr(), d.data_ptr(), T, n, GAMMA, ret.data_ptr(), ln.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 0
    torch.cuda.synchronize()
    assert not bool(ret.any())                                           # recorded, not run
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ret.cpu().numpy().view(np.int32), eager.view(np.int32)) and np.array_equal(ln.cpu().numpy(), eager_len)
