"""The learner kernels (csrc/usim_ppo.hip) through their C ABI, against the float64 restatement in tests/ppo_ref.py: crafted tensors, no env handle.  Every
gradient entry and statistic is held to the bound ppo_ref.grad_bounds derives from the kernels' operation sequence (its module docstring); what the contract calls
"bit for bit" is compared exactly.  GUARD sentinel words stand behind every output.  The parameters sit in ONE flat block in the header's order, as
ppo.flatten_parameters leaves them (most fields then start off the 16-byte grid).  The worst error / bound per case is printed at the end of the module (pytest -s)
and, where USIM_PPO_ACCURACY_OUT names a file, written there (profiles/ppo/accuracy.txt is such a record).  Measured on one MI355X over the whole module:
  gradient    0.34 / 0.16 at batch 1 / 2, 1.5e-3 at 31 .. 33 rows, 5e-4 at 4101 and 4199 (the bound adds the rows' error bounds coherently and carries the forward
              pass's worst case through the ratio: loose by orders of magnitude from a few dozen rows on; it is about 1e-3 of the largest entry, a thirtieth of what a dropped row is at 33 rows)
  statistics  0.19 .. 0.71 (clip_fraction exact in every case: the kernel takes the reference's side of every clip edge)
  Adam        up to 1.0: its bound IS the half-ulp of the one rounding of a float64 result
No bar was changed after seeing these."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ppo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25e33
GUARD = 64
MARGINS = {}
W = R.W
BATCHES = [(1, None, False), (2, None, False), (31, None, False), (32, None, False), (33, None, False), (32 * W + 5, None, False),
           (32 * (W + 3) + 7, 3 * (32 * (W + 3) + 7), True)]


def _margin(name, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    m = float(ratio.max())
    MARGINS[name] = max(MARGINS.get(name, 0.0), m)
    assert np.all(err <= bound), f"{name}: worst error / bound {m:.3g} at {np.unravel_index(np.argmax(ratio), err.shape)}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["worst error / bound per case (tests/test_gpu_ppo_kernels.py; the bar is 1):"] + [f"  {k:44s} {MARGINS[k]:.3g}" for k in sorted(MARGINS)]
    print("\n" + "\n".join(lines))
    out = os.environ.get("USIM_PPO_ACCURACY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def lib(usim):
    assert usim._lib.PPO_WORKGROUPS == W
    return usim._lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _guarded(n):
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)


def _read(t, n, name):
    a = t.cpu().numpy()
    assert np.all(a[n:] == np.float32(SENTINEL)), f"{name}: a word behind its end was written"
    return a[:n].copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Problem:
    """a make_problem dict on the device: the flat parameter block, the net struct pointing into it, the batch struct"""

    def __init__(self, usim, pr, clip=0.2, ent=0.01, vf=0.5, normalize=True):
        L = usim._lib
        self.pr, self.A, self.const = pr, pr["A"], (clip, ent, vf, normalize)
        self.P = R.n_params(self.A)
        self.theta = _dev(R.flatten(pr["p"]))
        ptr, o = {}, 0
        for k, s in R.shapes(self.A).items():
            ptr[k] = self.theta.data_ptr() + 4 * o
            o += int(np.prod(s))
        self.net = L.UsimPolicyNet(*(ptr[k] for k in R.FIELDS), None)
        self.t = {k: _dev(pr[k]) for k in ("obs", "act", "old_logp", "adv", "ret")}
        self.index = None if pr["index"] is None else _dev(pr["index"], torch.int32)
        self.batch = L.UsimPpoBatch(self.t["obs"].data_ptr(), self.t["act"].data_ptr(), self.t["old_logp"].data_ptr(), self.t["adv"].data_ptr(),
                                    self.t["ret"].data_ptr(), None if self.index is None else self.index.data_ptr(), pr["rows"], pr["batch"], self.A,
                                    int(normalize), clip, ent, vf, 0.0)

    def reference(self):
        clip, ent, vf, normalize = self.const
        return R.grad_bounds(self.pr["p"], *R.minibatch(self.pr), clip, ent, vf, normalize)


def new_work(lib, A, fill=0.0):
    return torch.full((int(lib.usim_ppo_work_floats(A)),), fill, dtype=torch.float32, device=DEV)


def run_grad(lib, pb, work=None):
    """-> (grad [P], stats [8]) float32"""
    work = new_work(lib, pb.A) if work is None else work
    grad, stats = _guarded(pb.P), _guarded(8)
    rc = lib.usim_ppo_grad(C.byref(pb.net), C.byref(pb.batch), work.data_ptr(), grad.data_ptr(), stats.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _read(grad, pb.P, "grad"), _read(stats, 8, "stats")


_CASES = {}


def _case(usim, A, batch, rows, index, **const):
    key = (A, batch, tuple(sorted(const.items())))
    if key not in _CASES:                                                  # the reference of a case is computed once and shared
        pb = Problem(usim, R.make_problem(A, batch, seed=batch + A, rows=rows, index=index), **const)
        _CASES[key] = (pb, pb.reference())
    return _CASES[key]


def _check(tag, grad, stats, ref, e_grad, e_stats):
    assert np.isfinite(grad).all() and np.isfinite(stats).all()
    _margin("gradient " + tag, np.abs(grad.astype(np.float64) - ref["grad"]), e_grad)
    _margin("statistics " + tag, np.abs(stats[:7].astype(np.float64) - ref["stats"]), e_stats)
    assert stats[7] == 0.0


# ================================================================ usim_ppo_grad ================================================================
@pytest.mark.parametrize("A", [6, 7])
@pytest.mark.parametrize("batch, rows, index", BATCHES)
def test_gradient_and_statistics_against_the_reference(usim, lib, A, batch, rows, index):
    pb, (ref, e_grad, e_stats) = _case(usim, A, batch, rows, index)
    grad, stats = run_grad(lib, pb)
    _check(f"A={A} batch={batch}", grad, stats, ref, e_grad, e_stats)
    if batch >= 31:
        assert 0.0 < ref["stats"][4] < 1.0                                 # clipped and unclipped samples in the comparison
    again = run_grad(lib, pb)                                              # the same inputs: the same bits
    assert np.array_equal(_bits(again[0]), _bits(grad)) and np.array_equal(_bits(again[1]), _bits(stats))


@pytest.mark.parametrize("A, batch", [(6, 33), (7, 32 * W + 5)])
def test_without_normalisation_and_entropy_term(usim, lib, A, batch):
    pb, (ref, e_grad, e_stats) = _case(usim, A, batch, None, False, normalize=False, ent=0.0, vf=0.25, clip=0.1)
    _check(f"A={A} batch={batch} raw advantages", *run_grad(lib, pb), ref, e_grad, e_stats)


def test_a_dirty_workspace_changes_nothing(usim, lib):
    """'zero-initialised once': the call rewrites every word of the workspace it reads -- after another batch size, after garbage"""
    big, _ = _case(usim, 6, 32 * W + 5, None, False)
    small, _ = _case(usim, 6, 33, None, False)
    clean = run_grad(lib, small)
    work = new_work(lib, 6)
    run_grad(lib, big, work)
    after_big = run_grad(lib, small, work)
    after_garbage = run_grad(lib, small, new_work(lib, 6, fill=float("nan")))
    for other in (after_big, after_garbage):
        assert np.array_equal(_bits(other[0]), _bits(clean[0])) and np.array_equal(_bits(other[1]), _bits(clean[1]))


def test_an_index_list_is_a_gather(usim, lib):
    """the minibatch through its index list equals the same samples laid out as rows 0 .. batch - 1, bit for bit"""
    pb, _ = _case(usim, 7, 32 * (W + 3) + 7, 3 * (32 * (W + 3) + 7), True)
    pr = pb.pr
    obs, act, old, adv, ret = R.minibatch(pr)
    flat = Problem(usim, dict(pr, obs=obs, act=act, old_logp=old, adv=adv, ret=ret, index=None, rows=pr["batch"]))
    a, b = run_grad(lib, pb), run_grad(lib, flat)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


# ================================================================ usim_ppo_adam ================================================================
def run_adam(lib, theta, grad, m, v, step, lr, eps, max_norm, with_stats=True):
    n = len(theta)
    t, mm, vv = (_guarded(n) for _ in range(3))
    for dst, src in ((t, theta), (mm, m), (vv, v)):
        dst[:n] = _dev(src)
    g = _dev(grad)
    st = torch.tensor([step], dtype=torch.int32, device=DEV)
    stats = _guarded(8)
    rc = lib.usim_ppo_adam(t.data_ptr(), g.data_ptr(), mm.data_ptr(), vv.data_ptr(), st.data_ptr(), n, lr, 0.9, 0.999, eps, max_norm,
                           stats.data_ptr() if with_stats else None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    assert np.all(s[np.arange(8 + GUARD) != 6] == np.float32(SENTINEL))    # only slot 6 is written
    return _read(t, n, "theta"), _read(mm, n, "m"), _read(vv, n, "v"), int(st.item()), float(s[6])


@pytest.mark.parametrize("n", [1000 + 37, R.n_params(6), 1])
@pytest.mark.parametrize("step", [0, 999])
@pytest.mark.parametrize("gscale, max_norm", [(0.1, 0.5), (1e-4, 0.5), (0.1, 0.0)])        # clip active, inactive, none
def test_adam_against_the_reference(lib, n, step, gscale, max_norm):
    rng = np.random.default_rng(n + step)
    theta = rng.normal(0, 0.3, n).astype(np.float32)
    grad = rng.normal(0, gscale, n).astype(np.float32)
    fresh = step == 0
    m = np.zeros(n, dtype=np.float32) if fresh else rng.normal(0, gscale, n).astype(np.float32)
    v = np.zeros(n, dtype=np.float32) if fresh else (rng.uniform(0.2, 2.0, n) * gscale ** 2).astype(np.float32)
    lr, eps = 3e-4, 1e-5
    t1, m1, v1, s1, norm = run_adam(lib, theta, grad, m, v, step, lr, eps, max_norm)
    rt, rm, rv, rs, rnorm = R.adam(theta, grad, m, v, step, lr, 0.9, 0.999, eps, max_norm)
    if n > 1 and max_norm > 0:
        assert (rnorm > max_norm) == (gscale == 0.1)                       # the case is what its name says
    et, em, ev, en = R.adam_bounds(theta, rt, rm, rv, rnorm)
    tag = f"adam n={n} step={step} g={gscale:g} max={max_norm:g}"
    assert s1 == rs == step + 1
    _margin(tag + " theta", np.abs(t1 - rt), et); _margin(tag + " m", np.abs(m1 - rm), em); _margin(tag + " v", np.abs(v1 - rv), ev)
    _margin(tag + " norm", abs(norm - rnorm), en)
    assert np.abs(t1 - theta).max() > 0                                    # (a step was taken)
    t2, m2, v2, s2, _ = run_adam(lib, theta, grad, m, v, step, lr, eps, max_norm, with_stats=False)         # stats_dev may be NULL; the same bits
    assert s2 == s1 and all(np.array_equal(_bits(x), _bits(y)) for x, y in ((t1, t2), (m1, m2), (v1, v2)))


# ================================================================ a recorded pair ================================================================
def test_a_captured_pair_replays_bit_for_bit(usim, lib):
    """usim_ppo_grad + usim_ppo_adam captured as one chain and replayed twice = two eager pairs (the step count lives on the device)"""
    pb0, _ = _case(usim, 6, 32 * W + 5, None, False)

    def state():
        pb = Problem(usim, pb0.pr)
        z = lambda: torch.zeros(pb.P, dtype=torch.float32, device=DEV)
        return dict(pb=pb, grad=z(), m=z(), v=z(), step=torch.zeros(1, dtype=torch.int32, device=DEV), stats=torch.zeros(8, dtype=torch.float32, device=DEV),
                    work=new_work(lib, pb.A))

    def pair(s):
        stream = _stream()
        assert lib.usim_ppo_grad(C.byref(s["pb"].net), C.byref(s["pb"].batch), s["work"].data_ptr(), s["grad"].data_ptr(), s["stats"].data_ptr(), stream) == 0
        assert lib.usim_ppo_adam(s["pb"].theta.data_ptr(), s["grad"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["step"].data_ptr(), s["pb"].P, 3e-4, 0.9, 0.999,
                                 1e-5, 0.5, s["stats"].data_ptr(), stream) == 0

    eager = state()
    pair(eager); pair(eager)
    torch.cuda.synchronize()
    rec = state()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(graph, stream=side):
            pair(rec)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(rec["step"].item()) == 0 and not rec["grad"].any()          # recording ran nothing
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    assert int(rec["step"].item()) == int(eager["step"].item()) == 2
    for k in ("grad", "m", "v", "stats"):
        assert torch.equal(rec[k].view(torch.int32), eager[k].view(torch.int32)), k
    assert torch.equal(rec["pb"].theta.view(torch.int32), eager["pb"].theta.view(torch.int32))
    assert not torch.equal(rec["pb"].theta, _dev(R.flatten(pb0.pr["p"])))  # (the parameters moved)
