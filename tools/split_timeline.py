"""Timeline of the split (two-wave) soft-torso step: shader-clock stamps of the arm wave and the lattice wave of workgroup 0 at their barriers."""
import importlib, os, subprocess, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
PROF = Path(os.environ.get("USIM_PROF_LIB") or ROOT / "robotic-ultrasound-imaging_amd" / "lib" / "libusim_prof.so")      # USIM_PROF_LIB: another profiling build (the parent's, for a before / after)
if not PROF.exists():
    subprocess.run(["make", "-s", "-C", str(ROOT / "robotic-ultrasound-imaging_amd" / "csrc"), "prof"], check=True)
os.environ["USIM_LIB"] = str(PROF)
sys.path.insert(0, str(ROOT))
import numpy as np, torch
usim = importlib.import_module("robotic-ultrasound-imaging_amd")
pre = int(sys.argv[1]) if len(sys.argv) > 1 else 200          # steps since the synchronous reset at which the stamps are taken
nenv = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
lanes = int(sys.argv[3]) if len(sys.argv) > 3 else 32          # 32: 16-lane groups, 64: 8-lane groups
env = usim.UltrasoundVecEnv(nenv, torso="soft", lanes_per_env=lanes, **usim.default_robosuite_kwargs())
env.reset_tensor(); env.rollout_random(0, pre); torch.cuda.synchronize()
count = int(sys.argv[4]) if len(sys.argv) > 4 else (20 if pre < 100 else 50)      # (0 100: the first 100 steps after the reset, where there is most contact)
rows = np.array([env.profile_step_raw(pre + k) for k in range(count)], dtype=np.float64)
print(f"stamps of steps {pre} .. {pre + len(rows) - 1} after the reset")
t0 = rows[:, 20:21]
names_a = ["start", "fk done", "barrier1 passed", "op-space + controller done", "barrier2 passed", "precompute done", "barrier3 passed (contacts solved)", "finish done", "barrier4 passed", "end"]
names_b = ["start", "stage+rhs done", "barrier1 passed", "solve+collide done", "barrier2 passed", "contact solve done", "barrier3 passed", "integrate done", "barrier4 passed"]
for base, names, title in ((20, names_a, "arm wave"), (30, names_b, "lattice wave")):
    print("==", title)
    for i, nm in enumerate(names):
        v = rows[:, base + i] - t0[:, 0]
        print(f"   {nm:36s} {np.median(v):9.0f}")
# The step boundary (USIM_PROFILE_NSUB > 1: the stamps are those of the last pass of a launch): hand-off (1) of the last pass counted from hand-off (3) of the pass before it.
# A library whose lattice wave runs ahead (csrc/usim_step16.h lattice_ahead) records that hand-off (3) (dbg[63] arm wave, dbg[62] lattice wave); for an older one, the same path is pieced together from the stamps of one
# pass, taken as periodic: hand-off (3) -> end of the pass, then start -> hand-off (1) (the barrier between the passes falls between the two pieces).
# (Running ahead, the lattice wave's "start" lies BEFORE the arm wave's, the zero of this table: it enters the pass while the arm wave finishes the previous one; hand-off
#  (4) exists on the last pass of a launch only, which is the one shown.)
if rows.shape[1] > 63 and (rows[:, 62:64] > 0).all():
    for col, title in ((63, "arm wave"), (62, "lattice wave")):
        base = 20 if col == 63 else 30
        print(f"== step boundary, {title}: hand-off (3) of the pass before -> hand-off (1) passed   {np.median(rows[:, base + 2] - rows[:, col]):9.0f}   (recorded)")
else:
    for base, title, last in ((20, "arm wave", 9), (30, "lattice wave", 8)):
        v = (rows[:, base + last] - rows[:, base + 6]) + (rows[:, base + 2] - rows[:, base])
        print(f"== step boundary, {title}: hand-off (3) -> end of the pass + start -> hand-off (1) passed   {np.median(v):9.0f}   (pieced together; excludes the wait at the barrier between the passes)")
# The report written late (csrc/usim_step16.h, DEF of step16_one; 16-lane groups, USIM_PROFILE_NSUB > 1): dbg[48] = the arm wave's state part of the pass before the last
# one done (counted from that pass's hand-off (3), dbg[63]), dbg[49] = that pass's report written in the last pass's wait (counted from the last pass's hand-off (2)).
if rows.shape[1] > 63 and (rows[:, 48:50] > 0).all() and (rows[:, 63] > 0).all():
    print(f"== report written late, arm wave: hand-off (3) of the pass before -> its state part done   {np.median(rows[:, 48] - rows[:, 63]):9.0f}")
    print(f"                                  state part done -> hand-off (1) passed                  {np.median(rows[:, 22] - rows[:, 48]):9.0f}")
    print(f"                                  hand-off (2) passed -> the pending report written       {np.median(rows[:, 49] - rows[:, 24]):9.0f}")
    print(f"                                  the pending report written -> precompute + draw done    {np.median(rows[:, 25] - rows[:, 49]):9.0f}")
else:
    print("== report written late: not recorded (a library without it, 8-lane groups or a launch of one pass)")
print(f"   (contact_solve entered at {np.median(rows[:, 40] - t0[:, 0]):.0f}, left at {np.median(rows[:, 44] - t0[:, 0]):.0f}: median ticks since the step's start; ncmax of this quad varies)")
for i, nm in enumerate(["contact list ready", "ncmax known", "before contact_solve", "after contact_solve"]):
    print(f"   x{i} {nm:32s} {np.median(rows[:, 50 + i] - t0[:, 0]):9.0f}")
# broad-phase queue lengths of the environments of the first lattice wave of workgroup 0 (dbg[54 ..] = 1 + nq; a library built before they were recorded leaves zeros);
# collide_queue walks the queue G elements at a time, uniformly over the wave: passes = max over the wave's environments of ceil(nq / G)
G = 16 if lanes == 32 else 8
nq = rows[:, 54:54 + 64 // G].astype(np.int64) - 1
if (nq >= 0).all():
    passes = ((nq + G - 1) // G).max(axis=1)
    print(f"== broad-phase queue (groups of {G} lanes): nq per environment, passes of collide_queue per step")
    print("   nq histogram     " + "  ".join(f"{v}:{c}" for v, c in zip(*np.unique(nq, return_counts=True))))
    print(f"   nq median {np.median(nq):.0f}  max {nq.max()}   passes histogram " + "  ".join(f"{v}:{c}" for v, c in zip(*np.unique(passes, return_counts=True))))
else:
    print("== broad-phase queue: not recorded by this library")
print("== contact solve of the lattice wave (ticks since its start)")
c0 = rows[:, 40:41]
for i, nm in enumerate(["start", "contact rows done", "Delassus blocks done", "sweeps done", "wrench done"]):
    print(f"   {nm:36s} {np.median(rows[:, 40 + i] - c0[:, 0]):9.0f}")
