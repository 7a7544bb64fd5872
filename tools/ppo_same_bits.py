"""A hash of what usim_ppo_grad writes on one fixed seeded input, with clip_range_vf off and on -- to compare two builds of the library: the PPO instances of
the gradient kernel must compute the same bits whatever instances stand beside them (profiles/imitation/same_bits.txt is such a record).  The library is
opened directly, not through _lib.load(), so that a build which lacks newer symbols can be hashed too.

usage: python tools/ppo_same_bits.py [LIBRARY] [--out FILE]      (default: the library of this checkout)"""
import argparse
import ctypes as C
import hashlib
import importlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np
import torch

import ppo_ref as R

L = importlib.import_module("robotic-ultrasound-imaging_amd._lib")
ap = argparse.ArgumentParser()
ap.add_argument("library", nargs="?", default=str(L.LIB_PATH))
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ppo_same_bits.py needs the GPU")
lib = C.CDLL(args.library)
lib.usim_version.restype = C.c_char_p
lib.usim_ppo_work_floats.restype, lib.usim_ppo_work_floats.argtypes = C.c_int64, [C.c_int]
lib.usim_ppo_grad.restype, lib.usim_ppo_grad.argtypes = L.SYMBOLS["usim_ppo_grad"]

A, BATCH, DEV = 6, 32 * 131 + 9, "cuda:0"                                   # 132 tiles over 128 workgroups, the last one partial
pr = R.make_problem(A, BATCH, seed=1, rows=3 * BATCH, index=True)
dev = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()
theta = dev(R.flatten(pr["p"]))
ptr, o = {}, 0
for k, s in R.shapes(A).items():
    ptr[k] = theta.data_ptr() + 4 * o
    o += int(np.prod(s))
net = L.UsimPolicyNet(*(ptr[k] for k in R.FIELDS), None)
t = {k: dev(pr[k]) for k in ("obs", "act", "old_logp", "adv", "ret")}
oldv = dev(pr["ret"] + np.random.default_rng(2).normal(0, 0.3, pr["rows"]).astype(np.float32))
index = dev(pr["index"], torch.int32)
lines = [f"{lib.usim_version().decode()}  [{Path(args.library).name}]  usim_ppo_grad, act_dim {A}, batch {BATCH} of {pr['rows']} rows through an index list, seed 1"]
for cvf in (0.0, 0.2):
    b = L.UsimPpoBatch(t["obs"].data_ptr(), t["act"].data_ptr(), t["old_logp"].data_ptr(), t["adv"].data_ptr(), t["ret"].data_ptr(), index.data_ptr(), pr["rows"],
                       BATCH, A, 1, 0.2, 0.01, 0.5, 0.0, oldv.data_ptr(), None, cvf, 0.0)
    work = torch.zeros(int(lib.usim_ppo_work_floats(A)), dtype=torch.float32, device=DEV)
    grad, stats = torch.zeros(R.n_params(A), dtype=torch.float32, device=DEV), torch.zeros(8, dtype=torch.float32, device=DEV)
    rc = lib.usim_ppo_grad(C.byref(net), C.byref(b), work.data_ptr(), grad.data_ptr(), stats.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise SystemExit(f"usim_ppo_grad answered {rc}")
    torch.cuda.synchronize()
    h = lambda x: hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()[:32]
    lines.append(f"  clip_range_vf {cvf:3.1f}   grad_dev sha256 {h(grad)}   stats_dev sha256 {h(stats)}   loss {float(stats[5]):.9g}  |grad| {float(stats[6]):.9g}")
print("\n".join(lines))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
