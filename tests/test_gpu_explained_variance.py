"""usim_explained_variance (csrc/usim_monitor.hip) through its C ABI against the float64 numpy restatement of SB3's explained_variance (tests/monitor_ref.py).

Counts: one and two elements; the edge of a wave (63, 64, 65); past the 1024 threads of the workgroup (1025, 16 * 64 + 7); 262144 = a 2048 x 128 rollout.  Returns
have mean 100 and standard deviation 1 -- the case the shift by the first element exists for: sum(y^2) / N - mean^2 in float64 without it loses mean^2 / var =
1e4 of its precision.
Bound: 1e-6 * max(1, |ev|) -- float32 rounding of the result (6e-8 relative) plus the float64 accumulation error amplified by at most mean^2 / var = 1e4, ~1e-9."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import monitor_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = [1, 2, 63, 64, 65, 1025, 16 * 64 + 7, 262144]
SENTINEL = 12345.0


def _ev(usim, values, returns):
    lib = usim._lib.load()
    v, r = torch.from_numpy(values).to(DEV), torch.from_numpy(returns).to(DEV)
    out = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    rc = lib.usim_explained_variance(v.data_ptr(), r.data_ptr(), v.numel(), out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[1:] == SENTINEL).all()                                 # one word is written
    return float(o[0])


def _data(count, noise):
    g = np.random.default_rng(count)
    returns = (100.0 + g.standard_normal(count)).astype(np.float32)
    values = (returns + noise * g.standard_normal(count) + 0.25).astype(np.float32)
    return values, returns


@pytest.mark.parametrize("noise", [0.1, 1.0, 3.0])
@pytest.mark.parametrize("count", COUNTS)
def test_against_float64(usim, count, noise):
    values, returns = _data(count, noise)
    want, got = ref.explained_variance(values, returns), _ev(usim, values, returns)
    print(f"count {count} noise {noise}: device {got!r} float64 {want!r}")
    if math.isnan(want):
        assert count == 1 and math.isnan(got)                        # one element has no variance
    else:
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (got, want)


@pytest.mark.parametrize("count", COUNTS)
def test_constant_returns_give_nan(usim, count):
    values, _ = _data(count, 1.0)
    assert math.isnan(_ev(usim, values, np.full(count, 100.125, dtype=np.float32)))


@pytest.mark.parametrize("count", COUNTS[1:])
def test_values_equal_returns_give_exactly_one(usim, count):
    _, returns = _data(count, 1.0)
    assert _ev(usim, returns.copy(), returns) == 1.0


def test_twice_the_same_bits(usim):
    values, returns = _data(262144, 1.0)
    a, b = _ev(usim, values, returns), _ev(usim, values, returns)
    assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)
