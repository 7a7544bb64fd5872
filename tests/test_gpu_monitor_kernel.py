"""usim_monitor_step (csrc/usim_monitor.hip) through its C ABI against tests/monitor_ref.py: caller buffers only, so the inputs are synthetic arrays -- no simulator
(but for the capture test, which needs an env for policy._capture).

Sizes sit where the ranking can go wrong: one environment; the edge of a wave (63, 64, 65); several waves (256, 257); the edge of the 1024-environment chunk
(1023, 1024, 1025) and several chunks with a ragged last one (4097).  Windows: 1 and 3 (every launch with more than a few episodes overflows the ring inside the
launch), 100 (SB3's), 5000 (never full here), and windows of n and n - 1 (an all-done launch counts exactly the window, or one more).  Every sequence is 6 launches
whose done patterns are none / all / only the first / only the last environment / random 30 %, with flag bytes from {1, 2, 0x80, 0xff}, NaN and 1e30 in ep_return
where not done, and the done pointer one byte off the 16-byte grid in every second launch.  Integers and ring rows are compared exactly (floats by their bits)."""
import ctypes as C

import numpy as np
import pytest
import torch

import monitor_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5AA5A5
GUARD = 64
SIZES = [1, 63, 64, 65, 256, 257, 1023, 1024, 1025, 4097]
WINDOWS = [1, 3, 100, 5000]
EDGE = [(65, 65), (65, 64), (257, 256), (1025, 1024), (1025, 1025), (4097, 4096)]          # (n, window): all done counts window, or window + 1
PATTERNS = ["random", "all", "none", "first", "last", "all"]
HORIZON = 500


def _launch_inputs(n, pattern, g, nan_at_done=False):
    """host arrays of one launch: done bytes, ep_return (float32), ep_length (int32)"""
    d = np.zeros(n, dtype=np.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "first":
        d[0] = 1
    elif pattern == "last":
        d[-1] = 1
    elif pattern == "random":
        d[g.random(n) < 0.3] = 1
    d = np.where(d != 0, g.choice(np.array([1, 2, 0x80, 0xff], dtype=np.uint8), n), 0).astype(np.uint8)
    r = (100.0 * g.standard_normal(n)).astype(np.float32)
    idx = np.nonzero(d)[0]
    if len(idx):
        r[idx[len(idx) // 2]] = np.float32(-0.0)                     # a negative zero where done: its bits reach the ring
        if nan_at_done:
            r.view(np.uint32)[idx[-1]] = 0x7fc12345                  # a NaN with a payload, in the last done environment
    stale = np.nonzero(d == 0)[0]
    r[stale[0::2]] = np.float32("nan")                               # stale words: never read into anything
    r[stale[1::2]] = np.float32(1e30)
    l = g.integers(1, 1001, n).astype(np.int32)                      # about half are >= HORIZON: truncated
    return d, r, l


def _sequence(n, seed, patterns=PATTERNS, nan_at_done=False):
    g = np.random.default_rng(seed)
    return [_launch_inputs(n, p, g, nan_at_done) for p in patterns]


class Monitor:
    """the device side of one test: the block (+ guard words), optional targets / counts (+ guard words), and the launches"""

    def __init__(self, usim, n, window, targets=None):
        self.L, self.lib, self.n, self.window = usim._lib, usim._lib.load(), n, window
        self.words = self.L.monitor_words(window)
        assert self.lib.usim_monitor_words(window) == self.words
        self.buf = torch.cat([torch.zeros(self.words, dtype=torch.int32), torch.full((GUARD,), SENTINEL, dtype=torch.int32)]).to(DEV)
        self.targets = self.counts = None
        if targets is not None:
            self.targets = torch.tensor(targets, dtype=torch.int32, device=DEV)
            self.counts = torch.cat([torch.zeros(n, dtype=torch.int32), torch.full((GUARD,), SENTINEL, dtype=torch.int32)]).to(DEV)
        self.keep = []

    def upload(self, seq):
        """[(done, ret, len)] -> device tensors; every second launch reads its flags one byte off the 16-byte grid"""
        out = []
        for k, (d, r, l) in enumerate(seq):
            off = k & 1
            dd = torch.zeros(self.n + 16, dtype=torch.uint8, device=DEV)
            dd[off:off + self.n] = torch.from_numpy(d).to(DEV)
            assert dd.data_ptr() % 16 == 0
            out.append((dd, off, torch.from_numpy(r).to(DEV), torch.from_numpy(l).to(DEV)))
        self.keep.append(out)
        return out

    def launch(self, dev_inputs):
        dd, off, r, l = dev_inputs
        io = self.L.UsimStepIO(None, None, None, dd.data_ptr() + off, None, None, r.data_ptr(), l.data_ptr(), None, None, None)
        ptr = lambda x: None if x is None else x.data_ptr()
        rc = self.lib.usim_monitor_step(C.byref(io), self.n, self.window, HORIZON, ptr(self.targets), ptr(self.counts), self.buf.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def host(self):
        torch.cuda.synchronize()
        w = self.buf.cpu().numpy()
        assert (w[self.words:].view(np.uint32) == SENTINEL).all(), "words behind the block were written"
        if self.counts is not None:
            assert (self.counts[self.n:].cpu().numpy().view(np.uint32) == SENTINEL).all(), "words behind count_dev were written"
        return w[:self.words].copy()


def _check(block, m, window, check_return_sum=True):
    """the block against the reference monitor m"""
    head = block[:16]
    episodes, length_sum, truncated, launches = (int(head[2 * k:2 * k + 2].view(np.int64)[0]) for k in (0, 1, 3, 4))
    assert (episodes, length_sum, truncated, launches) == (m.episodes, m.length_sum, m.truncated, m.launches)
    assert (head[10:16] == 0).all()
    ring = block[16:].reshape(window, 4)
    live = min(episodes, window)
    rows = np.roll(ring, -(episodes % window), axis=0)[:live] if episodes >= window else ring[:live]
    np.testing.assert_array_equal(rows, m.rows())
    assert (ring[live:] == 0).all()                                  # rows that no episode has reached yet
    return_sum = float(head[4:6].view(np.float64)[0])
    if check_return_sum:
        err = abs(return_sum - m.return_sum)
        print(f"return_sum {return_sum!r} reference {m.return_sum!r} |difference| {err:.3e} bound {m.abs_sum_bound:.3e}")
        assert err <= m.abs_sum_bound
    return return_sum


def _run(usim, n, window, seed, targets=None, nan_at_done=False, patterns=PATTERNS):
    seq = _sequence(n, seed, patterns, nan_at_done)
    m = ref.MonitorRef(n, window, HORIZON, targets)
    mon = Monitor(usim, n, window, targets)
    dev = mon.upload(seq)
    for k, (d, r, l) in enumerate(seq):
        mon.launch(dev[k])
        m.step(d, r, l)
        _check(mon.host(), m, window, check_return_sum=not nan_at_done)          # after every launch
    block = mon.host()
    if targets is not None:
        assert mon.counts[:n].cpu().tolist() == m.counts
    # again from the same start: the same block, bit for bit
    again = Monitor(usim, n, window, targets)
    for x in again.upload(seq):
        again.launch(x)
    np.testing.assert_array_equal(again.host(), block)
    return block, m


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_sequences_match_the_reference(usim, n, window):
    shift = (SIZES.index(n) + WINDOWS.index(window)) % len(PATTERNS)           # the patterns meet the aligned and the offset flag pointer in turn
    _run(usim, n, window, seed=1000 * window + n, patterns=PATTERNS[shift:] + PATTERNS[:shift])


@pytest.mark.parametrize("n,window", EDGE)
def test_all_done_counts_exactly_the_window_or_one_more(usim, n, window):
    block, m = _run(usim, n, window, seed=7 * n + window)
    assert m.episodes > 2 * window                                   # two all-done launches alone


@pytest.mark.parametrize("n,window", [(65, 3), (1025, 100), (4097, 5000)])
def test_nan_return_where_done_keeps_its_bits(usim, n, window):
    block, m = _run(usim, n, window, seed=31 * n, nan_at_done=True)
    bits = block[16:].reshape(window, 4)[:, 0].view(np.uint32)
    assert (bits == 0x7fc12345).any()                                # the last counted environment of the last launch: in the ring whatever the window
    assert np.isnan(block[4:6].view(np.float64)[0]) and np.isnan(m.return_sum)


@pytest.mark.parametrize("n,window", [(65, 100), (1025, 3), (4097, 5000)])
def test_target_gating(usim, n, window):
    """targets with zeros; environments reach their target in the middle of the sequence and finish again afterwards without being counted"""
    g = np.random.default_rng(n)
    targets = g.integers(0, 4, n).astype(np.int32)
    targets[0], targets[-1] = 0, 2
    block, m = _run(usim, n, window, seed=n + 5, targets=targets.tolist(), patterns=["all", "random", "all", "all", "random", "all"])
    assert m.counts == targets.tolist() and m.episodes == int(targets.sum())     # four all-done launches and targets <= 3: every environment has reached its own


def test_recorded_launches_equal_eager_ones(usim):
    """the 6 launches recorded with policy._capture and replayed equal the eager launches; two replays equal twelve eager launches"""
    n, window = 1025, 100
    env = usim.UltrasoundVecEnv(64, device=DEV, seed=3, torso="rigid", **usim.default_robosuite_kwargs())
    env.reset_tensor()
    seq = _sequence(n, 77)
    eager, graphed = Monitor(usim, n, window), Monitor(usim, n, window)
    dev_e, dev_g = eager.upload(seq), graphed.upload(seq)
    graph = usim.policy._capture(env, lambda: [graphed.launch(x) for x in dev_g])
    np.testing.assert_array_equal(graphed.host()[:16], 0)            # recording runs nothing
    m = ref.MonitorRef(n, window, HORIZON)
    for rounds in (1, 2):
        graph.replay()
        for k, x in enumerate(dev_e):
            eager.launch(x)
            m.step(*seq[k])
        block = graphed.host()
        np.testing.assert_array_equal(block, eager.host())
        _check(block, m, window)
    assert m.launches == 12
    env.close()
