"""usim_ppo_grad_multi / usim_ppo_adam_multi (csrc/usim_ppo.hip) through their C ABI against their contract: member k's words of grad, stats, theta, m, v, step and
gate after the multi calls are, bit for bit, what usim_ppo_grad / usim_ppo_adam_gated write for that member alone.  K = 3 members, 4200 rows each, problems from
ppo_ref.make_problem with a seed per member; theta is [3][stride] with stride = P rounded up to 4 words (A = 6: P = 76941, stride 76944), so the rows of members 1
and 2 start where a lone flat block never starts.  Every comparison is of int32 words over the WHOLE K-major tensors -- both sides start from the same sentinel
fill, so a word behind P in a row, or a word of another member, that either side touched shows.  One gradient is also held to ppo_ref's float64 reference within
ppo_ref.grad_bounds (the reference's own bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, ROWS = 3, 4200
SENTINEL = -7.25e33
HYPER = np.array([[3e-4, 0.2, 0.01, 0.5, 0.5, 0.0, 0.0, 0.0],               # lr, clip_range, ent_coef, vf_coef, max_grad_norm, clip_range_vf, target_kl, 0
                  [1e-3, 0.1, 0.0, 0.25, 0.0, 0.0, 0.0, 0.0],
                  [1e-4, 0.3, 0.003, 1.0, 1e-3, 0.0, 0.0, 0.0]], dtype=np.float32)
_PROBLEMS = {}


@pytest.fixture(scope="module")
def lib(usim):
    return usim._lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _problems(A, batch):
    """the K problems of a case (index lists with repeats into 4200 rows; clip_range per member), made once and shared"""
    if (A, batch) not in _PROBLEMS:
        _PROBLEMS[A, batch] = [R.make_problem(A, batch, seed=1000 * k + batch + A, rows=ROWS, index=True, clip_range=float(HYPER[k, 1])) for k in range(K)]
    return _PROBLEMS[A, batch]


def _i32(t):
    return t.contiguous().view(torch.int32)


class State:
    """the K-major tensors of a population on the device (every output starts as sentinel words) and, for the lone side, the per-member structs pointing into them"""

    def __init__(self, usim, A, batch, index=True, hyper=HYPER, value_clip=False, steps=(0, 0, 0)):
        self.L, self.A, self.batch, self.P = usim._lib, A, batch, R.n_params(A)
        self.stride = (self.P + 3) // 4 * 4
        prs = _problems(A, batch)
        dev = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()
        fill = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)
        self.theta = fill(K, self.stride)
        for k, pr in enumerate(prs):
            self.theta[k, :self.P] = dev(R.flatten(pr["p"]))
        self.data = {name: dev(np.concatenate([pr[name] for pr in prs])) for name in ("obs", "act", "old_logp", "adv", "ret")}
        rng = np.random.default_rng(batch)
        self.data["oldv"] = dev(np.concatenate([pr["ret"] + rng.normal(0, 0.5, ROWS) for pr in prs]).astype(np.float32))
        self.index = dev(np.stack([pr["index"] for pr in prs]), torch.int32) if index else None
        self.hyper, self.value_clip = dev(hyper), value_clip
        self.hyper_host = np.asarray(hyper, dtype=np.float32)
        self.grad, self.m, self.v, self.stats = fill(K, self.stride), fill(K, self.stride), fill(K, self.stride), fill(K, 8)
        self.m[:, :self.P] = 0.0; self.v[:, :self.P] = 0.0
        self.step = torch.tensor(list(steps), dtype=torch.int32, device=DEV)
        self.gate = torch.zeros(K, 4, dtype=torch.int32, device=DEV)

    def words(self):
        return dict(grad=_i32(self.grad), stats=_i32(self.stats), gate=self.gate, theta=_i32(self.theta), m=_i32(self.m), v=_i32(self.v), step=self.step)

    def multi_batch(self):
        d, p = self.data, (lambda t: t.data_ptr())
        return self.L.UsimPpoBatchMulti(p(d["obs"]), p(d["act"]), p(d["old_logp"]), p(d["adv"]), p(d["ret"]), p(d["oldv"]) if self.value_clip else None,
                                        None if self.index is None else p(self.index), p(self.hyper), p(self.gate), self.batch, ROWS, self.batch, self.A, 1,
                                        int(self.value_clip))

    def multi_work(self, lib, fill=0.0):
        return torch.full((int(lib.usim_ppo_work_floats_multi(self.A, K, self.batch)),), fill, dtype=torch.float32, device=DEV)

    def grad_multi(self, lib, work=None):
        self._work = self.multi_work(lib) if work is None else work
        b = self.multi_batch()
        assert lib.usim_ppo_grad_multi(self.theta.data_ptr(), self.stride, K, C.byref(b), self._work.data_ptr(), self.grad.data_ptr(), self.stats.data_ptr(), _stream()) == 0

    def adam_multi(self, lib):
        assert lib.usim_ppo_adam_multi(self.theta.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), self.stride, K, self.P,
                                       self.hyper.data_ptr(), 0.9, 0.999, 1e-5, self.stats.data_ptr(), self.gate.data_ptr(), _stream()) == 0

    def grad_lone(self, lib, k):
        """usim_ppo_grad for member k alone: its row of theta, its rows of the data, its index list, its hyper-parameters as the values of the table, its gate"""
        d, h = self.data, [float(x) for x in self.hyper_host[k]]
        base, o, ptr = self.theta.data_ptr() + 4 * k * self.stride, 0, {}
        for name, s in R.shapes(self.A).items():
            ptr[name] = base + 4 * o
            o += int(np.prod(s))
        net = self.L.UsimPolicyNet(*(ptr[name] for name in R.FIELDS), None)
        at = lambda t, width=1: t.data_ptr() + 4 * k * ROWS * width
        b = self.L.UsimPpoBatch(at(d["obs"], 19), at(d["act"], self.A), at(d["old_logp"]), at(d["adv"]), at(d["ret"]),
                                None if self.index is None else self.index.data_ptr() + 4 * k * self.batch, ROWS, self.batch, self.A, 1, h[1], h[2], h[3], 0.0,
                                at(d["oldv"]) if self.value_clip else None, self.gate.data_ptr() + 16 * k, h[5] if self.value_clip else 0.0, h[6])
        work = torch.zeros(int(lib.usim_ppo_work_floats(self.A)), dtype=torch.float32, device=DEV)
        assert lib.usim_ppo_grad(C.byref(net), C.byref(b), work.data_ptr(), self.grad.data_ptr() + 4 * k * self.stride, self.stats.data_ptr() + 32 * k, _stream()) == 0

    def adam_lone(self, lib, k):
        h, row = [float(x) for x in self.hyper_host[k]], 4 * k * self.stride
        assert lib.usim_ppo_adam_gated(self.theta.data_ptr() + row, self.grad.data_ptr() + row, self.m.data_ptr() + row, self.v.data_ptr() + row,
                                       self.step.data_ptr() + 4 * k, self.P, h[0], 0.9, 0.999, 1e-5, h[4], self.stats.data_ptr() + 32 * k, self.gate.data_ptr() + 16 * k,
                                       _stream()) == 0


def _same(a, b, names=None, members=range(K)):
    torch.cuda.synchronize()
    wa, wb = a.words(), b.words()
    for name in names or wa:
        for k in members:
            assert torch.equal(wa[name][k], wb[name][k]), f"{name} of member {k} differs"


# ================================================================ usim_ppo_grad_multi ================================================================
# 4133 rows: 130 tiles -- blocks 0 and 1 take two tiles, the last tile is partial; 70: three blocks where the lone call has 125 without a tile; 1: no normalisation
@pytest.mark.parametrize("index", [True, False])
@pytest.mark.parametrize("A, batch", [(6, 4133), (6, 70), (6, 1), (1, 70), (8, 70)])
def test_gradient_equals_three_lone_calls(usim, lib, A, batch, index):
    multi, lone = State(usim, A, batch, index), State(usim, A, batch, index)
    multi.grad_multi(lib)
    for k in range(K):
        lone.grad_lone(lib, k)
    _same(multi, lone)
    g = multi.grad[:, :multi.P]
    assert torch.isfinite(g).all() and torch.isfinite(multi.stats).all() and (multi.gate.cpu() == torch.tensor([0, 1, 0, 0])).all()
    assert not torch.equal(g[0], g[1]) and (multi.grad[:, multi.P:] == SENTINEL).all()      # members differ; words behind P are never touched


def test_a_dirty_workspace_changes_nothing(usim, lib):
    """the multi call rewrites every word it reads: NaN bit patterns in the workspace, or the words another batch size left there, change no bit"""
    clean, nan, reused, big = (State(usim, 6, b) for b in (70, 70, 70, 4133))
    clean.grad_multi(lib)
    nan.grad_multi(lib, nan.multi_work(lib, fill=float("nan")))
    work = big.multi_work(lib, fill=float("nan"))
    big.grad_multi(lib, work)
    reused.grad_multi(lib, work)
    _same(nan, clean)
    _same(reused, clean)


def test_gradient_against_the_float64_reference(usim, lib):
    """member 1 at batch 70 within ppo_ref.grad_bounds of ppo_ref.loss_and_grad with ITS clip_range, ent_coef and vf_coef"""
    s = State(usim, 6, 70)
    s.grad_multi(lib)
    torch.cuda.synchronize()
    pr, h = _problems(6, 70)[1], HYPER[1]
    ref, e_grad, e_stats = R.grad_bounds(pr["p"], *R.minibatch(pr), float(h[1]), float(h[2]), float(h[3]), True)
    grad, stats = s.grad[1, :s.P].cpu().numpy().astype(np.float64), s.stats[1].cpu().numpy().astype(np.float64)
    err, serr = np.abs(grad - ref["grad"]), np.abs(stats[:7] - ref["stats"])
    print(f"\nmember 1, batch 70: worst gradient error / bound {np.max(err / np.maximum(e_grad, 1e-300)):.3g}, statistics {np.max(serr / np.maximum(e_stats, 1e-300)):.3g}")
    assert np.all(err <= e_grad) and np.all(serr <= e_stats)
    assert np.abs(ref["grad"]).max() > 100 * e_grad.max()                    # (the bound tells a gradient from none)


def test_value_clip_instance(usim, lib):
    hyper = HYPER.copy()
    hyper[:, 5] = [0.2, 0.05, 1.0]
    multi, lone = State(usim, 6, 70, hyper=hyper, value_clip=True), State(usim, 6, 70, hyper=hyper, value_clip=True)
    plain = State(usim, 6, 70)
    multi.grad_multi(lib); plain.grad_multi(lib)
    for k in range(K):
        lone.grad_lone(lib, k)
    _same(multi, lone)
    assert not torch.equal(multi.stats[:, 1], plain.stats[:, 1])             # (the clip is active: the value loss is another)


# ================================================================ usim_ppo_adam_multi ================================================================
def test_adam_equals_three_lone_calls(usim, lib):
    """steps at entry 0, 5, 1000; three learning rates; max_grad_norm 0.5 (clipping), 0 (none), 1e-3 (clipping hard)"""
    def state():
        s = State(usim, 6, 70, steps=(0, 5, 1000))
        rng = np.random.default_rng(7)
        s.grad[:, :s.P] = torch.as_tensor(rng.normal(0, 0.1, (K, s.P)).astype(np.float32)).to(DEV)
        s.m[1:, :s.P] = torch.as_tensor(rng.normal(0, 0.1, (K - 1, s.P)).astype(np.float32)).to(DEV)
        s.v[1:, :s.P] = torch.as_tensor((rng.uniform(0.2, 2.0, (K - 1, s.P)) * 0.01).astype(np.float32)).to(DEV)
        return s
    multi, lone, before = state(), state(), state()
    multi.adam_multi(lib)
    for k in range(K):
        lone.adam_lone(lib, k)
    _same(multi, lone)
    assert multi.step.tolist() == [1, 6, 1001] and multi.gate[:, 2].tolist() == [1, 1, 1]
    st = multi.stats.cpu().numpy()
    assert np.all(st[:, [0, 1, 2, 3, 4, 5, 7]] == np.float32(SENTINEL)) and np.all(st[:, 6] > 1.0)      # only slot 6 is written: the norm (0.1 sqrt(P) = 27.7)
    moved = (multi.theta[:, :multi.P] - before.theta[:, :multi.P]).abs().amax(dim=1).tolist()
    assert all(x > 0 for x in moved) and (multi.theta[:, multi.P:] == SENTINEL).all()


def test_the_gate_is_per_member(usim, lib):
    """target_kl 0 (off), 1e-12 (trips on the first minibatch), 1e6 (never trips): after two grad + adam pairs member 1 has evaluated one gradient and stepped
    nothing, members 0 and 2 carry the bits of their lone gated runs"""
    hyper = HYPER.copy()
    hyper[:, 6] = [0.0, 1e-12, 1e6]
    multi, lone, before = (State(usim, 6, 70, hyper=hyper, steps=(0, 5, 1000)) for _ in range(3))
    for _ in range(2):
        multi.grad_multi(lib); multi.adam_multi(lib)
    for k in range(K):
        for _ in range(2):
            lone.grad_lone(lib, k); lone.adam_lone(lib, k)
    _same(multi, lone)
    assert multi.gate.tolist() == [[0, 2, 2, 0], [1, 1, 0, 0], [0, 2, 2, 0]] and multi.step.tolist() == [2, 5, 1002]
    _same(multi, before, names=("theta", "m", "v", "step"), members=[1])     # the stopped member's parameters, moments and step are untouched
    assert float(multi.stats[1, 3]) > 1.5e-12 and not torch.equal(multi.theta[0], before.theta[0]) and not torch.equal(multi.theta[2], before.theta[2])


def test_a_nan_stays_inside_its_member(usim, lib):
    clean, dirty = State(usim, 6, 70), State(usim, 6, 70)
    dirty.theta[0, :dirty.P] = float("nan")
    dirty.data["obs"][:ROWS] = float("nan")
    for s in (clean, dirty):
        s.grad_multi(lib); s.adam_multi(lib)
    _same(dirty, clean, members=[1, 2])
    assert torch.isnan(dirty.grad[0, :dirty.P]).any() and torch.isfinite(dirty.theta[1:, :dirty.P]).all()


def test_a_captured_pair_replays_bit_for_bit(usim, lib):
    """one grad + adam multi pair captured as a single chain and replayed twice = two eager pairs"""
    eager, rec = State(usim, 6, 70), State(usim, 6, 70)
    for _ in range(2):
        eager.grad_multi(lib); eager.adam_multi(lib)
    torch.cuda.synchronize()
    work = rec.multi_work(lib)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(graph, stream=side):
            rec.grad_multi(lib, work); rec.adam_multi(lib)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert rec.step.tolist() == [0, 0, 0] and (rec.grad == SENTINEL).all()    # recording ran nothing
    graph.replay(); graph.replay()
    _same(rec, eager)
    assert rec.step.tolist() == [2, 2, 2]
