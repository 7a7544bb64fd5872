"""usim_metrics_step (csrc/usim_metrics.hip) through its C ABI against tests/metrics_ref.py: caller buffers only, so the inputs are synthetic log / done arrays -- no
simulator.  horizon 7; every sequence is 10 calls of random records whose time channel is each environment's own step counter, episodes ending at random, at the
horizon, and -- in calls 3 and 7 -- everywhere at once, with flag bytes from {1, 2, 0x80, 0xff}.

Sizes sit where the ranking and the grid can go wrong: one environment; the edge of a wave (63, 64, 65); 300, above the accumulate kernel's workgroup of 256
(environment, metric) items -- 20 environments -- and above the 256 episodes the append kernel stages per round of its ordered walk (an all-done call takes two
rounds); the edge of the append kernel's 1024-environment chunk (1025: a second chunk of one environment) and 2100 (three chunks, the last ragged, nine rounds
in an all-done call).  Windows 4 (every all-done call overflows the ring inside the call) and 100.

Every integer word is compared exactly.  Every float64 word -- totals, ring metrics, accumulators -- within 1e-12 relative of the restatement: the restatement
adds the same float64 terms in the same order (accumulators step by step, totals episode by episode in ascending environment index), so the kernel may differ
only by fused multiply-adds inside a term, its square and the division -- an ulp or two (2.2e-16) per term on sums of at most `horizon` = 7 non-negative terms per
accumulator; 1e-12 leaves a margin of well over 1000.  The columns that are their own summand are signed here and agree exactly.  The measured maximum is printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5AA5A5
GUARD = 64
HORIZON = 7
SIZES = [1, 63, 64, 65, 300, 1025, 2100]
CALLS = 10


def _sequence(n, seed, nan_at=None):
    g = np.random.default_rng(seed)
    seq = ref.synthetic_episodes(n, HORIZON, CALLS, seed, p_done=0.2)
    t = np.zeros(n, dtype=np.int64)
    out = []
    for k, (log, done) in enumerate(seq):
        if k in (3, 7):                                               # everywhere at once
            done = np.ones(n, dtype=np.uint8)
        log[:, ref.TIME] = (t.astype(np.float64) / HORIZON * 100.0).astype(np.float32)          # the step counter under the done flags actually used
        t += 1
        done = np.where((done != 0) | (t >= HORIZON), g.choice(np.array([1, 2, 0x80, 0xff], dtype=np.uint8), n), 0).astype(np.uint8)
        t[done != 0] = 0
        if nan_at is not None and k == nan_at[0]:
            log[nan_at[1], 19] = np.float32("nan")
        out.append((log, done))
    return out


class Block:
    """the device side of one test: the block (+ guard words), optional targets / counts (+ guard words), and the calls"""

    def __init__(self, usim, n, window, targets=None):
        self.L, self.lib, self.n, self.window = usim._lib, usim._lib.load(), n, window
        self.words = self.L.metrics_words(n, window)
        assert self.lib.usim_metrics_words(n, window) == self.words
        self.buf = torch.cat([torch.zeros(self.words, dtype=torch.int32), torch.full((GUARD,), SENTINEL, dtype=torch.int32)]).to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.targets = self.counts = None
        if targets is not None:
            self.targets = torch.tensor(targets, dtype=torch.int32, device=DEV)
            self.counts = torch.cat([torch.zeros(n, dtype=torch.int32), torch.full((GUARD,), SENTINEL, dtype=torch.int32)]).to(DEV)
        self.keep = []

    def upload(self, seq):
        out = [(torch.from_numpy(log).to(DEV).contiguous(), torch.from_numpy(done).to(DEV)) for log, done in seq]
        self.keep.append(out)
        return out

    def call(self, dev_inputs):
        log, done = dev_inputs
        io = self.L.UsimStepIO(None, None, None, done.data_ptr(), None, None, None, None, None, None, log.data_ptr())
        ptr = lambda x: None if x is None else x.data_ptr()
        rc = self.lib.usim_metrics_step(C.byref(io), self.n, self.window, HORIZON, ptr(self.targets), ptr(self.counts), self.buf.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def host(self):
        torch.cuda.synchronize()
        w = self.buf.cpu().numpy()
        assert (w[self.words:].view(np.uint32) == SENTINEL).all(), "words behind the block were written"
        if self.counts is not None:
            assert (self.counts[self.n:].cpu().numpy().view(np.uint32) == SENTINEL).all(), "words behind count_dev were written"
        return w[:self.words].copy()


def _run(usim, n, window, seed, targets=None, nan_at=None, check_every_call=True):
    seq = _sequence(n, seed, nan_at)
    m = ref.MetricsRef(n, window, HORIZON, targets)
    blk = Block(usim, n, window, targets)
    dev = blk.upload(seq)
    worst = 0.0
    for k, (log, done) in enumerate(seq):
        blk.call(dev[k])
        m.step(log, done)
        if check_every_call or k == len(seq) - 1:
            worst = max(worst, ref.compare_blocks(blk.host(), m.block(), n, window, rtol=1e-12))
    block = blk.host()
    print(f"n {n} window {window}: {m.episodes} episodes, largest relative difference of a float64 word {worst:.3e} (bound 1e-12)")
    if targets is not None:
        assert blk.counts[:n].cpu().tolist() == m.counts
    # again from a zero block: the same block, bit for bit
    again = Block(usim, n, window, targets)
    for x in again.upload(seq):
        again.call(x)
    np.testing.assert_array_equal(again.host(), block)
    return block, m


@pytest.mark.parametrize("window", [4, 100])
@pytest.mark.parametrize("n", SIZES)
def test_sequences_match_the_restatement(usim, n, window):
    block, m = _run(usim, n, window, seed=100 * window + n)
    assert m.episodes >= 2 * n and m.launches == CALLS and m.nonfinite == 0


def test_all_65_done_in_one_call_keeps_the_last_four_in_ascending_index(usim):
    n, window = 65, 4
    g = np.random.default_rng(9)
    log = g.standard_normal((n, 53)).astype(np.float32)
    log[:, ref.TIME] = np.float32(2 / 7 * 100.0)
    seq = [(log, np.ones(n, dtype=np.uint8))]
    m = ref.MetricsRef(n, window, HORIZON)
    blk = Block(usim, n, window)
    blk.call(blk.upload(seq)[0])
    m.step(*seq[0])
    block = blk.host()
    ref.compare_blocks(block, m.block(), n, window)
    ring = block[ref.HEADER:ref.HEADER + ref.ROW * window].reshape(window, ref.ROW)
    assert ring[:, 26].tolist() == [64, 61, 62, 63]                  # episodes 61 .. 64 in rows e mod 4
    assert (ring[:, 27] == 3).all() and (ring[:, 28:] == 0).all()
    assert int(block[:2].view(np.int64)[0]) == 65 and int(block[4:6].view(np.int64)[0]) == 65 * 3
    np.testing.assert_allclose(ring[1, :26].view(np.float64), ref.step_terms(log)[61] / 7.0, rtol=1e-12, atol=0)          # row 1 is episode 61: environment 61's one row


@pytest.mark.parametrize("n,window", [(65, 100), (300, 4), (1025, 100)])
def test_target_gating(usim, n, window):
    """targets {0, 1, 2}: environments that are done but not counted are zeroed and enter nothing; two all-done calls bring every environment to its target"""
    targets = np.random.default_rng(n).integers(0, 3, n).astype(np.int32)
    targets[0], targets[-1] = 0, 2
    block, m = _run(usim, n, window, seed=n + 5, targets=targets.tolist())
    assert m.counts == targets.tolist() and m.episodes == int(targets.sum())


def test_one_nan_row_counts_as_nonfinite_and_leaves_the_totals(usim):
    n, window = 65, 100
    block, m = _run(usim, n, window, seed=77, nan_at=(1, 40))        # a NaN in the quaternion-distance channel of environment 40 in call 1
    assert m.nonfinite == 1 and int(block[6:8].view(np.int64)[0]) == 1
    totals = block[8:60].view(np.float64)
    assert np.isfinite(totals).all()
    bad = [h for h in m.history if not np.isfinite(h[0]).all()]
    assert len(bad) == 1 and bad[0][1] == 40 and np.isnan(bad[0][0][7]) and np.isfinite(np.delete(bad[0][0], 7)).all()
    clean = ref.MetricsRef(n, window, HORIZON)                        # the same sequence without that episode's row in the sums
    for h in m.history:
        if np.isfinite(h[0]).all():
            clean.total += h[0]
            clean.total_sq += h[0] * h[0]
    np.testing.assert_allclose(totals[:13], clean.total, rtol=1e-12, atol=0)
    np.testing.assert_allclose(totals[13:], clean.total_sq, rtol=1e-12, atol=0)


def test_recorded_calls_equal_eager_ones(usim):
    """the 10 calls (20 launches) recorded with policy._capture and replayed equal the eager calls"""
    n, window = 300, 100
    env = usim.UltrasoundVecEnv(64, device=DEV, seed=3, torso="rigid", **usim.default_robosuite_kwargs())
    env.reset_tensor()
    seq = _sequence(n, 55)
    eager, graphed = Block(usim, n, window), Block(usim, n, window)
    dev_e, dev_g = eager.upload(seq), graphed.upload(seq)
    graph = usim.policy._capture(env, lambda: [graphed.call(x) for x in dev_g])
    np.testing.assert_array_equal(graphed.host(), 0)                 # recording runs nothing
    m = ref.MetricsRef(n, window, HORIZON)
    for rounds in (1, 2):
        graph.replay()
        for k, x in enumerate(dev_e):
            eager.call(x)
            m.step(*seq[k])
        block = graphed.host()
        np.testing.assert_array_equal(block, eager.host())
        ref.compare_blocks(block, m.block(), n, window)
    assert m.launches == 2 * CALLS
    env.close()
