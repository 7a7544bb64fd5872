"""usim_pack_step (csrc/usim_pack.hip) through its C ABI: the entry point takes caller buffers, so the inputs are synthetic tensors with known contents -- no
simulator -- and the expected block is put together with numpy.  Everything is compared as int32 bits.

Sizes sit where the compaction can go wrong: one environment; the edge of a wave (63, 64, 65) and a ragged one (67); the edge of a workgroup (256, 257); several
workgroups with a ragged last one (300, 1500), where a workgroup's first slot is the count of the flags of the workgroups before it.  The block is pre-filled with
a sentinel: episode rows at and beyond the count, and guard words behind the block, must still hold it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5AA5A5
GUARD = 64
SIZES = [1, 63, 64, 65, 67, 256, 257, 300, 1500]
PATTERNS = ["none", "all", "first", "last", "alternating", "random"]


def _done(n, pattern):
    d = np.zeros(n, dtype=np.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "first":
        d[0] = 1
    elif pattern == "last":
        d[-1] = 1
    elif pattern == "alternating":
        d[::2] = 1
    elif pattern == "random":
        d[np.random.default_rng(1000 + n).random(n) < 0.03] = 1
    return d


def _inputs(n, pattern, seed=0):
    """host arrays of one step's buffers; the float ones are kept as the int32 view of their bits"""
    g = np.random.default_rng(seed * 7919 + n)
    return {"obs": g.standard_normal((n, 19)).astype(np.float32).view(np.int32), "rew": g.standard_normal(n).astype(np.float32).view(np.int32),
            "done": _done(n, pattern), "term": g.standard_normal((n, 19)).astype(np.float32).view(np.int32),
            "ep_return": (100.0 * g.standard_normal(n)).astype(np.float32).view(np.int32), "ep_length": g.integers(1, 1001, n).astype(np.int32),
            "status": g.integers(0, 8, n).astype(np.int32)}


def _expected(h, optional=True):
    """(count, head [n][21], rows [count][23]) as int32, from the host arrays"""
    n = h["done"].shape[0]
    one = np.array([0.0, 1.0], dtype=np.float32).view(np.int32)
    head = np.concatenate([h["obs"], h["rew"][:, None], one[h["done"].astype(np.int64)][:, None]], axis=1)
    idx = np.nonzero(h["done"])[0]
    rows = np.zeros((len(idx), 23), dtype=np.int32)
    rows[:, 0] = idx
    if optional:
        rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4:] = h["ep_length"][idx], h["ep_return"][idx], h["status"][idx], h["term"][idx]
    assert head.shape == (n, 21)
    return int(h["done"].sum()), head, rows


class Packer:
    def __init__(self, usim):
        self.L = usim._lib
        self.lib = usim._lib.load()

    def device(self, h):
        return {k: torch.from_numpy(v).to(DEV) for k, v in h.items()}

    def buffer(self, n):
        return torch.full((self.L.pack_words(n) + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)

    def io(self, d, optional=True):
        p = lambda k: d[k].data_ptr() if (optional or k in ("obs", "rew", "done")) else None
        return self.L.UsimStepIO(None, p("obs"), p("rew"), p("done"), p("term"), None, p("ep_return"), p("ep_length"), None, p("status"), None)

    def pack(self, d, n, buf, optional=True, offset_bytes=0):
        io = self.io(d, optional)
        rc = self.lib.usim_pack_step(C.byref(io), n, buf.data_ptr() + offset_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc


@pytest.fixture(scope="module")
def packer(usim):
    return Packer(usim)


def _check_block(buf, h, optional=True):
    n = h["done"].shape[0]
    count, head, rows = _expected(h, optional)
    out = buf.cpu().numpy()
    assert out[0] == count and not out[1:4].any()
    assert np.array_equal(out[4 : 4 + 21 * n].reshape(n, 21), head)
    lst = out[4 + 21 * n : 4 + 44 * n].reshape(n, 23)
    assert np.array_equal(lst[:count], rows)                      # ascending environment index, integer words as int32
    assert (lst[count:] == SENTINEL).all() and (out[4 + 44 * n :] == SENTINEL).all()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_block_equals_numpy(packer, n, pattern):
    h = _inputs(n, pattern)
    assert pattern not in ("all", "first", "last", "alternating") or h["done"].any()
    buf = packer.buffer(n)
    assert packer.pack(packer.device(h), n, buf) == 0
    _check_block(buf, h)


def test_random_pattern_reaches_later_workgroups():
    """(a property of the inputs above, not of the kernel) the 3 % pattern has finished environments behind the first workgroup at 300 and 1500"""
    assert _done(300, "random")[256:].any() and _done(1500, "random")[:256].any() and _done(1500, "random")[1280:].any()


def test_non_finite_values_travel_as_bits(packer):
    n = 67
    h = _inputs(n, "alternating")
    special = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F812345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], dtype=np.uint32).view(np.int32)
    for key in ("obs", "term"):
        flat = h[key].reshape(-1)
        flat[:: 5] = np.resize(special, flat[::5].shape)          # quiet / signalling NaNs with payloads, +-inf, -0, a subnormal
    h["rew"][:8], h["ep_return"][:8] = special, special
    d = packer.device(h)
    assert torch.equal(d["obs"].cpu(), torch.from_numpy(h["obs"]))
    buf = packer.buffer(n)
    assert packer.pack(d, n, buf) == 0
    _check_block(buf, h)


@pytest.mark.parametrize("n", [67, 300])
def test_null_optional_pointers_give_zero_words(packer, n):
    h = _inputs(n, "alternating")
    buf = packer.buffer(n)
    assert packer.pack(packer.device(h), n, buf, optional=False) == 0
    _check_block(buf, h, optional=False)


def test_invalid_arguments_write_nothing(packer):
    n = 67
    h = _inputs(n, "all")
    d = packer.device(h)
    buf = packer.buffer(n)
    INVALID = -1                                                  # USIM_ERR_INVALID
    assert packer.pack(d, 0, buf) == INVALID
    assert packer.pack(d, -3, buf) == INVALID
    io = packer.io(d)
    io.obs_dev = None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert packer.lib.usim_pack_step(C.byref(io), n, buf.data_ptr(), stream) == INVALID
    for key in ("rew_dev", "done_dev"):
        io = packer.io(d)
        setattr(io, key, None)
        assert packer.lib.usim_pack_step(C.byref(io), n, buf.data_ptr(), stream) == INVALID
    assert packer.lib.usim_pack_step(None, n, buf.data_ptr(), stream) == INVALID
    assert packer.lib.usim_pack_step(C.byref(packer.io(d)), n, None, stream) == INVALID
    assert packer.pack(d, n, buf, offset_bytes=4) == INVALID      # off the 16-byte grid
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("n", [300, 1500])
def test_two_calls_give_the_same_block(packer, n):
    h = _inputs(n, "random", seed=3)
    h["done"] = (np.random.default_rng(n).random(n) < 0.4).astype(np.uint8)
    d = packer.device(h)
    a, b = packer.buffer(n), packer.buffer(n)
    assert packer.pack(d, n, a) == 0 and packer.pack(d, n, b) == 0
    assert torch.equal(a, b)
    _check_block(a, h)


def test_done_array_off_the_16_byte_grid(packer):
    """a caller's done array that is not 16-byte aligned takes the byte-wise count of the preceding workgroups"""
    n = 600
    h = _inputs(n, "random", seed=5)
    h["done"] = (np.random.default_rng(5).random(n) < 0.3).astype(np.uint8)
    d = packer.device(h)
    shifted = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
    shifted[3 : 3 + n] = d["done"]
    d["done"] = shifted[3 : 3 + n]
    assert d["done"].data_ptr() % 16 == 3
    buf = packer.buffer(n)
    assert packer.pack(d, n, buf) == 0
    _check_block(buf, h)
