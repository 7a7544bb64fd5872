"""clip_range_vf in usim_ppo_grad (csrc/usim_ppo.hip, stage 3 of the gradient kernel) against the float64 restatement in tests/ppo_ext_ref.py, through the C ABI
on crafted tensors.  The cases (ppo_ext_ref.CASES) are the smallest at which the kernel can go wrong: a lone row, two, one row past a tile of 32, more tiles than
workgroups (32 W + 5), and a gather with repeats; about a third of the rows lie below the band, a third inside, a third above, none within 1e-3 of an edge
(asserted on the reference alone).  c = 0.2.  Every gradient entry and statistic is held to the bound ppo_ext_ref.grad_bounds_vf derives -- for a minibatch
without a row inside the band that bound is exactly zero over the whole value network.  Sentinel words stand behind grad and stats.  The worst error / bound per
case is printed at the end of the module (pytest -s) and, where USIM_PPO_VF_ACCURACY_OUT names a file, written there (profiles/ppo/accuracy_vf.txt is such a
record)."""
import os

import numpy as np
import pytest
import torch

import ppo_ext_ref as X
import ppo_ref as R
from test_gpu_ppo_kernels import Problem, _bits, _dev, run_grad

pytestmark = pytest.mark.gpu
CVF = 0.2
MARGINS = {}


def _margin(name, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    m = float(ratio.max())
    MARGINS[name] = max(MARGINS.get(name, 0.0), m)
    print(f"{name}: worst error / bound {m:.3g}")
    assert np.all(err <= bound), f"{name}: worst error / bound {m:.3g} at {np.unravel_index(np.argmax(ratio), err.shape)}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["worst error / bound per case (tests/test_gpu_ppo_vf_clip.py, clip_range_vf 0.2; the bar is 1):"] + [f"  {k:52s} {MARGINS[k]:.3g}" for k in sorted(MARGINS)]
    print("\n" + "\n".join(lines))
    out = os.environ.get("USIM_PPO_VF_ACCURACY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def lib(usim):
    assert usim._lib.PPO_WORKGROUPS == R.W
    return usim._lib.load()


class VfProblem(Problem):
    """test_gpu_ppo_kernels.Problem with the old values on the device and the two fields of the batch struct set"""

    def __init__(self, usim, pr, cvf=CVF, **const):
        super().__init__(usim, pr, **const)
        self.cvf = cvf
        self.old = _dev(pr["old_values"])
        self.batch.old_value_dev, self.batch.clip_range_vf = self.old.data_ptr(), cvf

    def reference(self):
        clip, ent, vf, normalize = self.const
        return X.grad_bounds_vf(self.pr["p"], *X.minibatch_vf(self.pr), self.cvf, clip, ent, vf, normalize)


_CASES = {}


def _case(usim, A, batch, rows, index):
    key = (A, batch, rows, index)
    if key not in _CASES:                                                  # the reference of a case is computed once and shared
        pb = VfProblem(usim, X.case_problem(A, batch, rows, index, CVF))
        _CASES[key] = (pb, pb.reference())
    return _CASES[key]


@pytest.mark.parametrize("A, batch, rows, index", X.CASES)
def test_value_clipped_gradient_and_statistics_against_the_reference(usim, lib, A, batch, rows, index):
    pb, (ref, e_grad, e_stats) = _case(usim, A, batch, rows, index)
    assert X.vf_margin(ref) > X.EDGE_MARGIN > ref["e_dvo"]                  # the reference alone: no row near an edge, and the kernel's V - old cannot cross one
    grad, stats = run_grad(lib, pb)
    tag = f"A={A} batch={batch}" + (" indexed" if index else "")
    assert np.isfinite(grad).all() and np.isfinite(stats).all() and stats[7] == 0.0
    _margin("gradient " + tag, np.abs(grad.astype(np.float64) - ref["grad"]), e_grad)
    _margin("statistics " + tag, np.abs(stats[:7].astype(np.float64) - ref["stats"]), e_stats)
    lo, hi = X._vf_segment(A)
    if batch >= 33:
        assert ref["inside"].any() and not ref["inside"].all() and np.abs(grad[lo:hi]).max() > 0
    if not ref["inside"].any():
        assert not grad[lo:hi].any()                                      # exactly zero: no row passes a gradient to the value network
    again = run_grad(lib, pb)                                              # the same inputs: the same bits
    assert np.array_equal(_bits(again[0]), _bits(grad)) and np.array_equal(_bits(again[1]), _bits(stats))


@pytest.mark.parametrize("A, batch, rows, index", [(6, 33, None, False), (7, 33, 99, True), (6, 32 * R.W + 5, None, False)])
def test_clip_range_vf_zero_reads_no_old_values_and_changes_no_bit(usim, lib, A, batch, rows, index):
    """clip_range_vf == 0 with a non-NULL old_value_dev: the bits of the call without the field (old values of NaN would poison any use of them)"""
    pb, _ = _case(usim, A, batch, rows, index)
    plain = Problem(usim, pb.pr)
    off = VfProblem(usim, dict(pb.pr, old_values=np.full(pb.pr["rows"], np.nan, dtype=np.float32)), cvf=0.0)
    a, b = run_grad(lib, plain), run_grad(lib, off)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    on = run_grad(lib, pb)
    assert not np.array_equal(_bits(on[0]), _bits(a[0]))                    # (and with the clip on, the gradient is another one)
    lo, _ = X._vf_segment(A)
    assert np.array_equal(_bits(on[0][:lo]), _bits(a[0][:lo]))              # the policy network's share does not see the value clip
