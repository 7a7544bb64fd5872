"""usim_bc_grad (csrc/usim_ppo.hip: the behaviour-cloning instances of the gradient kernel) through its C ABI, against the float64 restatement in
tests/bc_ref.py: crafted tensors, no env handle.  Every gradient entry and statistic is held to the bound bc_ref.grad_bounds derives from the kernel's operation
sequence; what the contract calls exact is compared by bit pattern.  GUARD sentinel words stand behind grad_dev and stats_dev.  The parameters sit in ONE flat
block in the header's order, as ppo.flatten_parameters leaves them.  Batch sizes around the tile of 32 rows and the 128 workgroups per network: 1, 31, 32, 33,
and 4129 = 32 x 129 + 1 (130 tiles: workgroups 0 and 1 take two, the last tile holds one row).  The worst error / bound per case is printed at the end of the
module (pytest -s).  Measured on one MI355X over the whole module: gradient 0.37 at batch 1 (0.11 .. 0.37 over act_dim and form), 0.0049 at 31 .. 33 rows,
0.0039 at 4129 (the bound adds the rows' error bounds coherently, as ppo_ref's does: loose from a few dozen rows on); statistics 0.04 .. 0.60.  No bar was
changed after seeing these."""
import ctypes as C

import numpy as np
import pytest
import torch

import bc_ref as B
import ppo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25e33
GUARD = 64
MARGINS = {}
W = R.W
BATCHES = [1, 31, 32, 33, 32 * (W + 1) + 1]
assert BATCHES[-1] == 4129


def _margin(name, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    m = float(ratio.max())
    MARGINS[name] = max(MARGINS.get(name, 0.0), m)
    assert np.all(err <= bound), f"{name}: worst error / bound {m:.3g} at {np.unravel_index(np.argmax(ratio), err.shape)}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n" + "\n".join(["worst error / bound per case (tests/test_gpu_bc_kernels.py; the bar is 1):"] + [f"  {k:52s} {MARGINS[k]:.3g}" for k in sorted(MARGINS)]))


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


def _net(usim, theta, A):
    ptr, o = {}, 0
    for k, s in R.shapes(A).items():
        ptr[k] = theta.data_ptr() + 4 * o
        o += int(np.prod(s))
    return usim._lib.UsimPolicyNet(*(ptr[k] for k in R.FIELDS), None)


class Problem:
    """a bc_ref.make_problem dict on the device: the flat parameter block, the net struct pointing into it, the batch struct"""

    def __init__(self, usim, pr, loss, valued, ent=1e-3, vf=0.5):
        self.pr, self.A, self.const, self.valued = pr, pr["A"], (loss, ent, vf), valued
        self.P = R.n_params(self.A)
        self.theta = _dev(R.flatten(pr["p"]))
        self.net = _net(usim, self.theta, self.A)
        self.t = {k: _dev(pr[k]) for k in ("obs", "act", "value")}
        self.index = None if pr["index"] is None else _dev(pr["index"], torch.int32)
        self.batch = usim._lib.UsimBcBatch(self.t["obs"].data_ptr(), self.t["act"].data_ptr(), self.t["value"].data_ptr() if valued else None,
                                           None if self.index is None else self.index.data_ptr(), pr["rows"], pr["batch"], self.A, loss, ent, vf)

    def reference(self):
        loss, ent, vf = self.const
        obs, act, value = B.minibatch(self.pr)
        return B.grad_bounds(self.pr["p"], obs, act, value if self.valued else None, loss, ent, vf)


def new_work(lib, A, fill=0.0):
    return torch.full((int(lib.usim_ppo_work_floats(A)),), fill, dtype=torch.float32, device=DEV)


def run_grad(lib, pb, work=None):
    """-> (grad [P], stats [8]) float32"""
    work = new_work(lib, pb.A) if work is None else work
    grad, stats = _guarded(pb.P), _guarded(8)
    rc = lib.usim_bc_grad(C.byref(pb.net), C.byref(pb.batch), work.data_ptr(), grad.data_ptr(), stats.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _read(grad, pb.P, "grad"), _read(stats, 8, "stats")


_PROBLEMS = {}


def _problem(A, batch, rows=None, index=False):
    key = (A, batch, rows, index)
    if key not in _PROBLEMS:                                                # the inputs of a case are drawn once and shared by both forms
        _PROBLEMS[key] = B.make_problem(A, batch, seed=batch + A, rows=rows, index=index)
    return _PROBLEMS[key]


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _vf_words(A):
    sl = B.field_slices(A)
    return slice(sl["vf_w1"].start, sl["val_b"].stop)


# ================================================================ against the reference ================================================================
@pytest.mark.parametrize("valued", [True, False], ids=["value", "novalue"])
@pytest.mark.parametrize("loss", [B.NLL, B.MSE], ids=["nll", "mse"])
@pytest.mark.parametrize("A", [1, 6, 8])
@pytest.mark.parametrize("batch", BATCHES)
def test_gradient_and_statistics_against_the_reference(usim, lib, batch, A, loss, valued):
    pb = Problem(usim, _problem(A, batch), loss, valued)
    ref, e_grad, e_stats = pb.reference()
    grad, stats = run_grad(lib, pb)
    tag = f"{'nll' if loss == B.NLL else 'mse'} {'value' if valued else 'novalue'} A={A} batch={batch}"
    assert np.isfinite(grad).all() and np.isfinite(stats).all()
    _margin("gradient " + tag, np.abs(grad.astype(np.float64) - ref["grad"]), e_grad)
    _margin("statistics " + tag, np.abs(stats[:7].astype(np.float64) - ref["stats"]), e_stats)
    assert _bits(stats[7:8])[0] == 0
    vf = _vf_words(A)
    if valued:
        assert np.abs(grad[vf]).max() > 0 and stats[1] > 0
    else:
        assert not _bits(grad[vf]).any() and _bits(stats[1:2])[0] == 0      # +0.0f by bit pattern: the value network was not evaluated
    sl = B.field_slices(A)
    if loss == B.MSE:
        assert np.array_equal(grad[sl["log_std"]], np.full(A, -np.float32(1e-3)))       # the entropy term alone
        assert stats[0] == stats[3]
    assert np.abs(grad[sl["pi_w1"]]).max() > 0 and stats[3] > 0 and stats[6] > 0
    assert _same(run_grad(lib, pb), (grad, stats))                          # the same inputs: the same bits


def test_a_zero_value_coefficient_is_no_value_term(usim, lib):
    pr = _problem(6, 33)
    a, b = run_grad(lib, Problem(usim, pr, B.NLL, True, vf=0.0)), run_grad(lib, Problem(usim, pr, B.NLL, False, vf=0.5))
    assert _same(a, b) and not _bits(a[0][_vf_words(6)]).any()


# ================================================================ the index list ================================================================
@pytest.mark.parametrize("loss", [B.NLL, B.MSE], ids=["nll", "mse"])
@pytest.mark.parametrize("A, batch", [(6, 33), (8, BATCHES[-1])])
def test_an_index_list_with_repeats_and_strays_is_the_clamped_gather(usim, lib, loss, A, batch):
    pr = _problem(A, batch, rows=3 * batch, index=True)
    idx = pr["index"]
    assert (idx < 0).any() and (idx >= pr["rows"]).any() and len(np.unique(idx)) < len(idx)
    clamped = B.clamp_index(idx, pr["rows"]).astype(np.int32)
    obs, act, value = B.minibatch(pr)
    pb = Problem(usim, pr, loss, True)
    ref, e_grad, e_stats = pb.reference()
    got = run_grad(lib, pb)
    _margin(f"gradient index list loss={loss} A={A} batch={batch}", np.abs(got[0].astype(np.float64) - ref["grad"]), e_grad)
    _margin(f"statistics index list loss={loss} A={A} batch={batch}", np.abs(got[1][:7].astype(np.float64) - ref["stats"]), e_stats)
    assert _same(got, run_grad(lib, Problem(usim, dict(pr, index=clamped), loss, True)))                                  # the clamped list: the same bits
    assert _same(got, run_grad(lib, Problem(usim, dict(pr, obs=obs, act=act, value=value, index=None, rows=batch), loss, True)))      # and the rows laid out


# ================================================================ the workspace ================================================================
@pytest.mark.parametrize("loss", [B.NLL, B.MSE], ids=["nll", "mse"])
def test_same_bits_after_usim_ppo_grad_used_the_workspace(usim, lib, loss):
    """one workspace serves both calls in turn: usim_bc_grad rewrites every word it reads -- after a PPO call of another batch size, after a behaviour-cloning
    call of the other kind, after garbage"""
    A = 6
    small, big = Problem(usim, _problem(A, 33), loss, False), Problem(usim, _problem(A, BATCHES[-1]), loss, True)
    clean_small, clean_big = run_grad(lib, small), run_grad(lib, big)
    work = new_work(lib, A)
    ppo = R.make_problem(A, 32 * W + 5, seed=3)
    t = {k: _dev(ppo[k]) for k in ("obs", "act", "old_logp", "adv", "ret")}
    theta = _dev(R.flatten(ppo["p"]))
    pbatch = usim._lib.UsimPpoBatch(t["obs"].data_ptr(), t["act"].data_ptr(), t["old_logp"].data_ptr(), t["adv"].data_ptr(), t["ret"].data_ptr(), None, ppo["rows"],
                                    ppo["batch"], A, 1, 0.2, 0.01, 0.5, 0.0)
    g, s = _guarded(small.P), _guarded(8)

    def ppo_call(w):
        assert lib.usim_ppo_grad(C.byref(_net(usim, theta, A)), C.byref(pbatch), w.data_ptr(), g.data_ptr(), s.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        return _read(g, small.P, "grad"), _read(s, 8, "stats")

    ppo_clean = ppo_call(new_work(lib, A))
    assert _same(run_grad(lib, small, work), clean_small)
    ppo_call(work)
    assert _same(run_grad(lib, small, work), clean_small)                   # value-network blocks full of PPO's partial sums: written over with zeros
    assert _same(run_grad(lib, big, work), clean_big)
    assert _same(ppo_call(work), ppo_clean)                                 # and the other way round
    assert _same(run_grad(lib, small, new_work(lib, A, fill=float("nan"))), clean_small)
    assert not _bits(clean_small[0][_vf_words(A)]).any()
