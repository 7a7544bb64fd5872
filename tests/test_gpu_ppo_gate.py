"""The gate of usim_ppo_grad / usim_ppo_adam_gated (include/usim.h: target_kl's early stop as a decision taken on the device), through the C ABI at A = 6,
batch 33: an open gate changes no bit and counts; a minibatch whose approx_kl exceeds 1.5 target_kl is evaluated, not stepped, and shuts the gate for every
later call; the decision is ppo_ext_ref.gate_rule of the float32 statistic the call wrote, and -- with target_kl a factor of two away from the edge on either
side -- of the float64 reference alone; a captured chain of three gated pairs that trips at the second replays bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_ext_ref as X
import ppo_ref as R
from test_gpu_ppo_kernels import DEV, GUARD, SENTINEL, Problem, _dev, _stream, new_work

pytestmark = pytest.mark.gpu
A, BATCH = 6, 33
ADAM = (3e-4, 0.9, 0.999, 1e-5, 0.5)                                      # lr, beta1, beta2, eps, max_grad_norm


@pytest.fixture(scope="module")
def lib(usim):
    return usim._lib.load()


@pytest.fixture(scope="module")
def problem():
    pr = R.make_problem(A, BATCH, seed=BATCH + A)
    return pr, float(R.loss_and_grad(pr["p"], *R.minibatch(pr), 0.2, 0.01, 0.5, True)["stats"][3])


class State:
    """one learner's device words around a Problem: guarded outputs, Adam's state with moments that are not zero, the gate"""

    def __init__(self, usim, lib, pr, gate=True):
        self.pb = Problem(usim, pr)
        P = self.pb.P
        rng = np.random.default_rng(11)
        self.theta = self.pb.theta
        self.grad = torch.full((P + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.stats = torch.full((8 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.m, self.v = _dev(rng.normal(0, 1e-3, P)), _dev(rng.uniform(1e-7, 1e-5, P))
        self.step = torch.full((1,), 5, dtype=torch.int32, device=DEV)
        self.gate = torch.zeros(4, dtype=torch.int32, device=DEV) if gate else None
        self.work = new_work(lib, A)

    def grad_call(self, lib, target_kl=0.0, pb=None):
        pb = self.pb if pb is None else pb
        b = pb.batch
        b.gate_dev, b.target_kl = (None if self.gate is None else self.gate.data_ptr()), target_kl
        assert lib.usim_ppo_grad(C.byref(self.pb.net), C.byref(b), self.work.data_ptr(), self.grad.data_ptr(), self.stats.data_ptr(), _stream()) == 0

    def adam_call(self, lib, lr=ADAM[0]):
        args = (self.theta.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), self.pb.P, lr) + ADAM[1:] + \
               (self.stats.data_ptr(),)
        if self.gate is None:
            assert lib.usim_ppo_adam(*args, _stream()) == 0
        else:
            assert lib.usim_ppo_adam_gated(*args, self.gate.data_ptr(), _stream()) == 0

    def words(self):
        torch.cuda.synchronize()
        out = {k: getattr(self, k).view(torch.int32).cpu().numpy().copy() for k in ("grad", "stats", "theta", "m", "v", "step")}
        out["gate"] = None if self.gate is None else self.gate.cpu().numpy().copy()
        return out


def _same(a, b, keys=("grad", "stats", "theta", "m", "v", "step")):
    return [k for k in keys if not np.array_equal(a[k], b[k])] == []


def _guards_intact(w, P):
    sent = np.float32(SENTINEL).view(np.int32)
    return np.all(w["grad"][P:] == sent) and np.all(w["stats"][8:] == sent)


@pytest.mark.parametrize("factor", [0.0, 2.0])
def test_an_open_gate_changes_no_bit_and_counts(usim, lib, problem, factor):
    """target_kl 0 (off) and target_kl at twice the reference's approx_kl (1.5 target_kl = 3 approx_kl: no stop): usim_ppo_grad + usim_ppo_adam's bits"""
    pr, kl = problem
    plain, gated = State(usim, lib, pr, gate=False), State(usim, lib, pr)
    plain.grad_call(lib); plain.adam_call(lib)
    gated.grad_call(lib, factor * kl); gated.adam_call(lib)
    a, b = plain.words(), gated.words()
    assert _same(a, b) and _guards_intact(b, gated.pb.P)
    assert b["gate"].tolist() == [0, 1, 1, 0] and int(b["step"][0]) == 6
    assert not np.array_equal(b["theta"], _dev(R.flatten(pr["p"])).view(torch.int32).cpu().numpy())      # (a step was taken)
    assert X.gate_rule(b["stats"][3:4].view(np.float32)[0], factor * kl) == 0
    gated.grad_call(lib, factor * kl); gated.adam_call(lib)               # the counts go on until the caller clears the words
    assert gated.words()["gate"].tolist() == [0, 2, 2, 0]


def test_a_tripping_minibatch_is_evaluated_not_stepped_and_shuts_the_gate(usim, lib, problem):
    pr, kl = problem
    target = 0.5 * kl                                                      # 1.5 target_kl = 0.75 approx_kl: the reference alone decides
    plain, gated = State(usim, lib, pr, gate=False), State(usim, lib, pr)
    plain.grad_call(lib)
    before = gated.words()
    gated.grad_call(lib, target)
    a, b = plain.words(), gated.words()
    assert b["gate"].tolist() == [1, 1, 0, 0]
    assert _same(a, b, ("grad", "stats")) and _guards_intact(b, gated.pb.P)  # the statistics (and the gradient) of the tripping minibatch
    written = b["stats"][3:4].view(np.float32)[0]
    assert abs(float(written) - kl) < 0.05 * kl and X.gate_rule(written, target) == 1 and X.gate_rule(written, 2.0 * kl) == 0
    gated.adam_call(lib)
    c = gated.words()
    assert _same(before, c, ("theta", "m", "v", "step")) and _same(b, c, ("grad", "stats")) and c["gate"].tolist() == [1, 1, 0, 0]      # stats[6] included
    # a second minibatch with other data: nothing is written, not even over a sentinel pattern
    other = Problem(usim, R.make_problem(A, BATCH, seed=1234))
    pattern = torch.arange(gated.pb.P, dtype=torch.float32, device=DEV) * 0.5 - 3.0
    gated.grad[:gated.pb.P].copy_(pattern); gated.stats[:8].copy_(pattern[:8])
    marked = gated.words()
    gated.grad_call(lib, target, pb=other); gated.adam_call(lib)
    d = gated.words()
    assert _same(marked, d) and d["gate"].tolist() == [1, 1, 0, 0]
    # the caller clears the words: the same call now computes (the other data's gradient, in place of the pattern)
    gated.gate.zero_()
    gated.grad_call(lib, 0.0, pb=other)
    e = gated.words()
    assert e["gate"].tolist() == [0, 1, 0, 0] and not np.array_equal(e["grad"][:gated.pb.P], marked["grad"][:gated.pb.P]) and _guards_intact(e, gated.pb.P)


def test_a_captured_chain_that_trips_at_its_second_pair_replays_bit_for_bit(usim, lib, problem):
    """three gated pairs as one captured chain.  Pair 1 sees the samples with old_logp at the reference's own log-probabilities (ratio 1, approx_kl ~ 0) and steps;
    pair 2 sees the problem as drawn (approx_kl: the reference's, moved a little by one Adam step at lr 1e-5) against 1.5 target_kl = 0.375 of it, and trips;
    pair 3 does nothing.  Replayed after the caller has cleared the gate = the eager calls, bit for bit, the second time round too."""
    pr, kl = problem
    ref = R.loss_and_grad(pr["p"], *R.minibatch(pr), 0.2, 0.01, 0.5, True, keep=True)
    calm = dict(pr, old_logp=ref["logp"].astype(np.float32))
    target, lr = 0.25 * kl, 1e-5

    def make():
        s = State(usim, lib, pr)
        s.calm = Problem(usim, calm)
        return s

    def chain(s):
        s.grad_call(lib, target, pb=s.calm); s.adam_call(lib, lr)
        s.grad_call(lib, target); s.adam_call(lib, lr)
        s.grad_call(lib, target, pb=s.calm); s.adam_call(lib, lr)

    eager, rec = make(), make()
    chain(eager)
    first = eager.words()
    assert first["gate"].tolist() == [1, 2, 1, 0] and int(first["step"][0]) == 6
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(graph, stream=side):
            chain(rec)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(rec.step.item()) == 5 and not rec.gate.any()                # recording ran nothing
    graph.replay()
    got = rec.words()
    assert _same(first, got) and got["gate"].tolist() == [1, 2, 1, 0]
    for s in (eager, rec):                                                 # the next update: the caller clears the words, the chain runs again
        s.gate.zero_()
    chain(eager); graph.replay()
    second, got = eager.words(), rec.words()
    assert _same(second, got) and np.array_equal(second["gate"], got["gate"]) and int(second["step"][0]) == 6 + int(second["gate"][2])
    assert not np.array_equal(second["theta"], first["theta"])
