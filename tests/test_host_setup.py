"""What usim_create decides before it touches the device (csrc/usim_setup.h: argument checks, model constants and tables, the usim_config -> DevCfg translation,
the mapping) against float64 restatements, on the CPU.  tests/setup_dump.hip, a host program, prints it; the restatements are tests/arm_lanes_model.py (the two
robot chains), the oracle (contact inverse weight) and the rules written out below (torso shell, lattice matrix, probe and torso constants).

Tolerance: a stored word is a float64 result narrowed once, so |got - ref| <= k * 2^-24 * |ref| + 1e-12 with k the number of float32 roundings in the expression
as written (1 almost everywhere; 3 for probe_cah, a float32 product of two narrowed values).  A stored inverse is checked by its residual, element by element:
|Ainv A - I| <= 2^-24 * (|Ainv| |A|) + 1e-12."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from arm_lanes_model import lane_tables, panda_chain, ur5e_chain
from oracle_lib import Oracle

ROOT = Path(__file__).resolve().parent.parent
EPS = 2.0 ** -24

# layouts of csrc/usim_device.h, restated
N_TOP, LROW, TB_LINV, TB_POS, TB_AXIS, TB_SHELL, TB_ARM, TB_TOTAL = 99, 100, 0, 9900, 10200, 10500, 10600, 10600 + 16 * 28
AT_RFIX, AT_LPOS, AT_LCOM, AT_MASS, AT_INERTIA, AT_QMIN, AT_QMAX, AT_TAUMAX, AT_INITQ, AT_JOINT, AT_ARMATURE, AT_STRIDE = 0, 9, 12, 15, 16, 22, 23, 24, 25, 26, 27, 28
NSH, FNE, FT_POS, FT_AXIS, FT_NBR, FT_P, FT_DIAG, FT_CONST, FT_LINV, FT_LROW = 270, 320, 0, 816, 1632, 2912, 3728, 4048, 4080, 272
W_FIX, W_TEN = 19.0, 9.5          # d_max 0.95: d / (1 - d) and half of it


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _compile(out, *flags):
    subprocess.run([_hipcc(), "-O1", "-std=c++17", "--offload-arch=gfx950", *flags, str(ROOT / "tests" / "setup_dump.hip"), "-o", str(out)], check=True)


def _number(text):
    try:
        return int(text)
    except ValueError:
        return float(text)


class Dump:
    """one run of the program: its lines by name, and the table words"""

    def __init__(self, exe, tmp, torso, shape, robot, *overrides, tables=False):
        path = tmp / f"tables_{torso}_{shape}_{robot}.bin"
        cmd = [str(exe), str(torso), str(shape), str(robot), *overrides] + ([f"tables={path}"] if tables else [])
        out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
        self.lines = {ln.split()[0]: ln.split()[1:] for ln in out.splitlines()}
        self.words = np.fromfile(path, dtype=np.float32) if tables else None

    def i(self, name):
        return int(self.lines[name][0])

    def f(self, name):
        return float(self.lines[name][0])

    def v(self, name):
        return np.array([float(x) for x in self.lines[name]])

    def cfg(self):
        return {k[4:]: _number(v[0]) for k, v in self.lines.items() if k.startswith("cfg.")}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("setup_dump")
    exe = tmp / "setup_dump"
    _compile(exe)
    return lambda *a, **kw: Dump(exe, tmp, *a, **kw)


@pytest.fixture(scope="module")
def tables(dump):
    """the table words of the six torso / shape / robot combinations, built once"""
    return {(t, s, r): dump(t, s, r, tables=True) for t, s, r in ((1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (2, 0, 0), (2, 1, 0))}


def assert_close(got, ref, k=1, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = k * EPS * np.abs(ref) + 1e-12
    worst = np.max(np.abs(got - ref) / bound)
    assert worst <= 1.0, f"{what}: {worst:.3f} of the bound"


def assert_inverse(inv, a, what=""):
    res = np.abs(inv @ a - np.eye(len(a)))
    bound = EPS * (np.abs(inv) @ np.abs(a)) + 1e-12
    assert np.max(res / bound) <= 1.0, f"{what}: residual {np.max(res / bound):.3f} of the bound"


# ---- torso shell: an element exists iff it lies on a face of the 9 x 4 x 11 box; ids in creation order (ix outer, iy, iz inner) ----
def shell():
    on = lambda a, b, c: 0 <= a < 9 and 0 <= b < 4 and 0 <= c < 11 and (a in (0, 8) or b in (0, 3) or c in (0, 10))
    cells = [(a, b, c) for a in range(9) for b in range(4) for c in range(11) if on(a, b, c)]
    ident = {cell: k for k, cell in enumerate(cells)}
    nbrs = [[ident[n] for n in ((a - 1, b, c), (a + 1, b, c), (a, b - 1, c), (a, b + 1, c), (a, b, c - 1), (a, b, c + 1)) if n in ident] for a, b, c in cells]
    return cells, ident, nbrs


def lattice_matrix(members, nbrs):
    """diagonal 1 + 19 + 9.5 * (number of shell neighbours), -9.5 to the neighbours that are members"""
    col = {e: k for k, e in enumerate(members)}
    L = np.zeros((len(members), len(members)))
    for k, e in enumerate(members):
        L[k, k] = 1.0 + W_FIX + W_TEN * len(nbrs[e])
        for n in nbrs[e]:
            if n in col:
                L[k, col[n]] = -W_TEN
    return L


# ---- arm table ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot, chain", [(0, panda_chain), (1, ur5e_chain)])
def test_arm_table_is_the_lane_tables_of_the_chain(dump, tables, robot, chain):
    ch = chain()
    T, nj = lane_tables(ch), ch["nj"]
    for scale, d in ((1.0, tables[(1, 0, robot)]), (0.0, dump(1, 0, robot, "armature_scale=0", tables=True))):
        assert d.words.size == TB_TOTAL
        arm = d.words[TB_ARM:].astype(np.float64).reshape(16, AT_STRIDE)
        assert_close(arm[:, AT_RFIX:AT_RFIX + 9].reshape(16, 3, 3).transpose(0, 2, 1), T["rfix"], what="rfix (stored by columns)")
        assert_close(arm[:, AT_LPOS:AT_LPOS + 3], T["lpos"], what="lpos")
        assert_close(arm[:, AT_LCOM:AT_LCOM + 3], T["lcom"], what="lcom")
        assert_close(arm[:, AT_MASS], T["mass"], what="mass")
        assert_close(arm[:, AT_INERTIA:AT_INERTIA + 6], T["inertia"][:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], what="inertia (upper triangle)")
        assert np.array_equal(arm[:, AT_JOINT], T["joint"])
        for col, key in ((AT_QMIN, "qmin"), (AT_QMAX, "qmax"), (AT_TAUMAX, "taumax"), (AT_INITQ, "initq")):
            assert_close(arm[:nj, col], ch[key], what=key)
        # padding lanes: identity (checked above against lane_tables), no mass, no joint, limits +-1e30
        assert np.all(arm[nj:, AT_MASS] == 0) and np.all(arm[nj:, AT_JOINT] == 0) and np.all(arm[nj:, AT_INITQ] == 0) and np.all(arm[nj:, AT_TAUMAX] == 1)
        assert_close(arm[nj:, AT_QMIN], np.full(16 - nj, -1e30)); assert_close(arm[nj:, AT_QMAX], np.full(16 - nj, 1e30))
        ref_arm = np.where(T["joint"] > 0, scale * 5.0 / (np.arange(16) + 1.0), 0.0)
        assert_close(arm[:, AT_ARMATURE], ref_arm, what="armature")
        assert_close(d.v("M.armature"), ref_arm[:7], what="M.armature")


@pytest.mark.parametrize("robot", ["Panda", "UR5e"])
def test_contact_inverse_weight_is_the_oracles(tables, robot):
    ora = Oracle(1, torso="top", robot=robot)
    ref = ora.lib.uso_contact_invweight(ora.h)
    got = tables[(1, 0, {"Panda": 0, "UR5e": 1}[robot])].f("M.invw")
    print(f"invw {robot}: {got!r} against {ref!r}")
    assert_close(got, ref, what="M.invw")


# ---- top-face lattice ---------------------------------------------------------------------------------------------------------------------------------
def test_top_face_lattice_inverse(tables):
    cells, ident, nbrs = shell()
    top = [ident[(ix, 3, iz)] for ix in range(9) for iz in range(11)]          # element e = 11 ix + iz
    L = lattice_matrix(top, nbrs)
    w = tables[(1, 0, 0)].words
    linv = w[TB_LINV:TB_LINV + N_TOP * LROW].astype(np.float64).reshape(N_TOP, LROW)
    assert np.all(linv[:, N_TOP:] == 0)                                          # the pad column
    assert_inverse(linv[:, :N_TOP], L, "TB_LINV")
    for key in ((1, 0, 1), (1, 1, 0), (1, 1, 1)):                                # the lattice does not depend on the shape or the robot
        assert np.array_equal(tables[key].words[TB_LINV:TB_POS], w[TB_LINV:TB_POS])


# ---- full torso -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [0, 1])
def test_full_torso_tables(tables, shape):
    cells, ident, nbrs = shell()
    assert len(cells) == NSH
    d = tables[(2, shape, 0)]
    w = d.words
    assert d.i("n_el") == NSH and w.size == FT_LINV + NSH * FT_LROW
    L = lattice_matrix(list(range(NSH)), nbrs)
    linv = w[FT_LINV:].astype(np.float64).reshape(NSH, FT_LROW)
    assert np.all(linv[:, NSH:] == 0)
    assert_inverse(linv[:, :NSH], L, "FT_LINV")
    diag = w[FT_DIAG:FT_DIAG + FNE]
    assert np.array_equal(diag[:NSH], np.diag(L)) and np.all(diag[NSH:] == 1)
    nbr = w[FT_NBR:FT_NBR + 4 * FNE].view(np.int32).reshape(FNE, 4)
    for e in range(FNE):
        mine = nbrs[e] if e < NSH else []
        assert sorted(nbr[e, :len(mine)]) == sorted(mine) and np.all(nbr[e, len(mine):] == FNE - 1), e
    # P = L^-1 N', S^-1 = (M I - m N P)^-1, I_b^-1, M_tot from the stored positions and axes (elements and the composite's centre geom: 0.01 kg each)
    m = 0.01
    pos, ax = w[FT_POS:FT_POS + 3 * NSH].astype(np.float64).reshape(NSH, 3), w[FT_AXIS:FT_AXIS + 3 * NSH].astype(np.float64).reshape(NSH, 3)
    P = np.linalg.solve(L, ax)
    assert_close(w[FT_P:FT_P + 3 * NSH].reshape(NSH, 3), P, what="FT_P")
    mtot = m * (NSH + 1)
    const = w[FT_CONST:FT_CONST + 32].astype(np.float64)
    assert_inverse(const[0:9].reshape(3, 3), mtot * np.eye(3) - m * ax.T @ P, "S^-1")
    c = pos - (0.0075 + 0.025) * ax                                              # capsule centres
    Ib = m * (np.sum(c * c) * np.eye(3) - c.T @ c)
    assert_inverse(const[9:18].reshape(3, 3), Ib, "I_b^-1")
    assert_close(const[18], 2.71, what="M_tot"); assert_close(const[18], mtot)
    assert_close(const[19], (1.0 / m + 2.0 / (NSH * m)) / 3.0, what="element inverse weight")
    assert np.all(const[20:] == 0)


# ---- element geometry -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [0, 1])
def test_element_geometry(tables, shape):
    cells, ident, nbrs = shell()
    top, full = tables[(1, shape, 0)].words, tables[(2, shape, 0)].words
    ids = top[TB_SHELL:TB_SHELL + N_TOP].view(np.int32)
    assert list(ids) == [ident[(ix, 3, iz)] for ix in range(9) for iz in range(11)]
    fpos, fax = full[FT_POS:FT_POS + 3 * NSH].reshape(NSH, 3), full[FT_AXIS:FT_AXIS + 3 * NSH].reshape(NSH, 3)
    assert np.array_equal(top[TB_POS:TB_POS + 3 * N_TOP].reshape(N_TOP, 3), fpos[ids])
    assert np.array_equal(top[TB_AXIS:TB_AXIS + 3 * N_TOP].reshape(N_TOP, 3), fax[ids])
    norm = np.sqrt(np.sum(fax.astype(np.float64) ** 2, axis=1))
    assert np.max(np.abs(norm - 1.0)) <= 3 * EPS
    if shape == 0:                         # the box: cells 35 mm apart about the centre; world x = -local z, y = -local x, z = local y; the slide axis is radial
        loc = np.array([[(a - 4) * 0.035, (b - 1.5) * 0.035, (c - 5) * 0.035] for a, b, c in cells])
        ref = np.stack([-loc[:, 2], -loc[:, 0], loc[:, 1]], axis=1)
        assert_close(fpos, ref, what="FT_POS")
        assert_close(fax, ref / np.linalg.norm(ref, axis=1, keepdims=True), what="FT_AXIS")


# ---- DevCfg ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, overrides", [
    (0, []), (0, ["substeps=25", "control_dt=0.05"]), (0, ["torso_drop=0"]), (0, ["torso_drop=1"]), (0, ["torso_drop=2"]), (0, ["probe_geoms=1"]), (0, ["pair_model=0"]),
    (1, []), (1, ["torso_drop=2"]), (0, ["seed=0x123456789a"]), (0, ["mode=2"])])
def test_devcfg_follows_its_formulas(dump, shape, overrides):
    d = dump(0, shape, 0, *overrides)
    c = d.cfg()
    assert d.i("check") == 1 and c["torso_shape"] == shape
    if "seed=0x123456789a" in overrides:
        assert c["seed"] == 0x123456789A > 2 ** 32
    geoms = 2 if c["probe_geoms"] == 2 else 1
    pair = 1 if geoms == 2 and c["pair_model"] != 0 else 0
    sub = max(c["substeps"], 1)
    ints = {"mode": c["mode"], "horizon": c["horizon"], "early_term": c["early_termination"], "det_traj": c["deterministic_trajectory"], "rand_solref": c["torso_solref_randomization"],
            "rand_pos": c["initial_probe_pos_randomization"], "rand_fric": c["friction_randomization"], "torso_drop": 1 if c["torso_drop"] == 1 else 0, "pgs_iters": c["pgs_iters"],
            "ik_iters": c["ik_iters"], "env_offset": c["env_offset"], "adim": 7 if c["mode"] == 2 else 6, "probe_geoms": geoms, "pair": pair, "substeps": sub,
            "key0": c["seed"] & 0xFFFFFFFF, "key1": c["seed"] >> 32}
    for name, ref in ints.items():
        assert d.i("C." + name) == ref, name
    r, r2, h, hw = c["probe_radius"], c["probe_radius2"], c["probe_height"], c["probe_halfwidth"]
    cb = (r - r2) / h
    ca = np.sqrt(1.0 - cb * cb)
    torso_z = [0.8 + 0.005 + 0.0522, 0.8 + 0.005 + 0.05][shape]               # table + z_offset - bottom_site z: box, cylinder
    floats = {"dt": c["control_dt"] / sub, "dt_ctrl": c["control_dt"], "kp_fixed": c["kp_fixed"], "damping_ratio": c["damping_ratio"], "kp_min": c["kp_min"], "kp_max": c["kp_max"],
              "out_pos": c["out_max_pos"], "out_ori": c["out_max_ori"], "stiffness": c["stiffness"], "damping": c["damping"], "elem_fric": c["elem_friction"],
              "probe_fric": c["probe_friction"], "probe_fric2": c["probe_friction2"], "probe_r": r, "probe_hl": c["probe_halflen"], "probe_hw": hw, "probe_tip": c["probe_tip"],
              "probe_r2": r2, "probe_h": h, "probe_ca": ca, "probe_cb": cb, "probe_cull2": (r + h + hw + 0.025 + 0.0075 + 1e-4) ** 2, "probe_deep0": r * (2.0 / 3.0),
              "probe_inv_band": 1.0 / (r * (0.96 - 2.0 / 3.0)), "top_off": [0.039, 0.041][shape], "y_range": [0.09, 0.05][shape],
              "drop": 0.0 if c["torso_drop"] == 0 else torso_z - 0.0525 - 0.8, "rn_scale": 0.5 if geoms == 2 and not pair else 1.0, "frictionloss": c["joint_frictionloss"]}
    for name, ref in floats.items():
        assert_close(d.f("C." + name), ref, what=name)
    assert_close(d.f("C.probe_cah"), ca * h, k=3, what="probe_cah")
    assert set(ints) | set(floats) | {"probe_cah"} == {k[2:] for k in d.lines if k.startswith("C.")}      # every field


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------------------
_CONDITIONS = {          # the conditions usim_create refuses a configuration for
    "struct_size": lambda c, size: c["struct_size"] != size,
    "probe_radius2 <= 0": lambda c, size: c["probe_radius2"] <= 0,
    "probe_height": lambda c, size: not c["probe_height"] > abs(c["probe_radius2"] - c["probe_radius"]),
    "probe_halfwidth": lambda c, size: not c["probe_halfwidth"] >= 0,
    "probe_tip": lambda c, size: not abs(c["probe_tip"]) <= 0.02,
    "torso_drop < 0": lambda c, size: c["torso_drop"] < 0, "torso_drop > 2": lambda c, size: c["torso_drop"] > 2,
    "mode < 0": lambda c, size: c["mode"] < 0, "mode > 3": lambda c, size: c["mode"] > 3,
    "torso < 0": lambda c, size: c["torso"] < 0, "torso > 2": lambda c, size: c["torso"] > 2,
    "armature_scale": lambda c, size: not c["armature_scale"] >= 0, "joint_frictionloss": lambda c, size: not c["joint_frictionloss"] >= 0,
    "horizon": lambda c, size: c["horizon"] <= 0, "control_dt": lambda c, size: c["control_dt"] <= 0, "probe_halflen": lambda c, size: c["probe_halflen"] < 1e-4,
    "probe_radius": lambda c, size: c["probe_radius"] <= 0, "pgs_iters": lambda c, size: c["pgs_iters"] < 0, "ik_iters": lambda c, size: c["ik_iters"] < 0,
    "torso_shape < 0": lambda c, size: c["torso_shape"] < 0, "torso_shape > 1": lambda c, size: c["torso_shape"] > 1,
    "waves_per_simd < 0": lambda c, size: c["waves_per_simd"] < 0, "waves_per_simd > 2": lambda c, size: c["waves_per_simd"] > 2,
    "robot < 0": lambda c, size: c["robot"] < 0, "robot > 1": lambda c, size: c["robot"] > 1,
    "warm_start < 0": lambda c, size: c["warm_start"] < 0, "warm_start > 1": lambda c, size: c["warm_start"] > 1,
}
_TRIPS = {               # one configuration per condition that trips only it
    "struct_size": ["struct_size=240"], "probe_radius2 <= 0": ["probe_radius2=-0.01", "probe_height=0.05"], "probe_height": ["probe_height=0.01"],
    "probe_halfwidth": ["probe_halfwidth=-0.001"], "probe_tip": ["probe_tip=0.03"], "torso_drop < 0": ["torso_drop=-1"], "torso_drop > 2": ["torso_drop=3"],
    "mode < 0": ["mode=-1"], "mode > 3": ["mode=4"], "torso < 0": ["torso=-1"], "torso > 2": ["torso=3"], "armature_scale": ["armature_scale=-1"],
    "joint_frictionloss": ["joint_frictionloss=-0.1"], "horizon": ["horizon=0"], "control_dt": ["control_dt=0"], "probe_halflen": ["probe_halflen=0.00005"],
    "probe_radius": ["probe_radius=0", "probe_height=0.05"], "pgs_iters": ["pgs_iters=-1"], "ik_iters": ["ik_iters=-1"], "torso_shape < 0": ["torso_shape=-1"],
    "torso_shape > 1": ["torso_shape=2"], "waves_per_simd < 0": ["waves_per_simd=-1"], "waves_per_simd > 2": ["waves_per_simd=3"], "robot < 0": ["robot=-1"],
    "robot > 1": ["robot=2"], "warm_start < 0": ["warm_start=-1"], "warm_start > 1": ["warm_start=2"],
}


def test_argument_checks(dump):
    ok = dump(1, 0, 0)
    size = ok.cfg()["struct_size"]
    assert ok.i("check") == 1 and not any(cond(ok.cfg(), size) for cond in _CONDITIONS.values())      # the default configuration is accepted
    assert set(_TRIPS) == set(_CONDITIONS)
    for name, overrides in _TRIPS.items():
        d = dump(1, 0, 0, *overrides)
        assert [k for k, cond in _CONDITIONS.items() if cond(d.cfg(), size)] == [name]
        assert d.i("check") == 0 and "build" not in d.lines, name


# ---- mapping --------------------------------------------------------------------------------------------------------------------------------------------
_MAPPINGS = [            # (torso, lanes_per_env, waves_per_simd, n_envs) -> mapping; None: refused
    ((0, 0, 0, 4096), "RIGID16"), ((0, 16, 0, 4096), "RIGID16"), ((0, 0, 2, 8192), "RIGID16"), ((0, 16, 1, 64), "RIGID16"),
    ((0, 32, 0, 4096), None), ((0, 64, 0, 4096), None), ((0, 8, 0, 4096), None), ((0, 1, 0, 4096), None),
    ((1, 16, 1, 8192), "SOFT16_W1"), ((1, 16, 2, 64), "SOFT16_W2"), ((1, 16, 0, 4096), "SOFT16_W1"), ((1, 16, 0, 4097), "SOFT16_W2"),
    ((1, 32, 0, 8192), "SPLIT16"), ((1, 32, 2, 64), "SPLIT16"), ((1, 64, 0, 64), "SPLIT8"), ((1, 64, 1, 8192), "SPLIT8"),
    ((1, 0, 0, 4096), "SPLIT16"), ((1, 0, 0, 4097), "SPLIT8"), ((1, 0, 1, 8192), "SOFT16_W1"), ((1, 0, 2, 64), "SOFT16_W2"),
    ((1, 8, 0, 4096), None), ((1, 1, 0, 4096), None), ((1, 48, 0, 4096), None), ((1, 128, 0, 4096), None), ((1, -16, 0, 4096), None),
    ((2, 0, 0, 64), "FULL"), ((2, 16, 1, 64), "FULL"), ((2, 32, 2, 64), "FULL"), ((2, 64, 0, 8192), "FULL"), ((2, 8, 0, 64), None), ((2, 1, 0, 64), None),
]


@pytest.mark.parametrize("torso", [0, 1, 2])
def test_resolve_mapping_table(dump, torso):
    for (t, lanes, waves, n), want in _MAPPINGS:
        if t == torso:
            d = dump(t, 0, 0, f"lanes_per_env={lanes}", f"waves_per_simd={waves}", f"n_envs={n}")
            assert d.i("check") == 1 and d.lines["mapping"][0] == (want or "refused"), (t, lanes, waves, n)
    for waves in (-1, 3):                  # waves_per_simd outside 0 .. 2 does not get as far as the mapping
        assert dump(torso, 0, 0, f"waves_per_simd={waves}").i("check") == 0


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="a host-only check for the machines without a GPU")
def test_setup_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program (stand-alone: nothing is preloaded) built with -fsanitize=address,undefined on the host side"""
    exe = tmp_path / "setup_dump_san"
    _compile(exe, "-g", "-Xarch_host", "-fsanitize=address,undefined")
    for t, s, r in ((1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (2, 0, 0), (2, 1, 0)):
        p = subprocess.run([str(exe), str(t), str(s), str(r), f"tables={tmp_path / 'tables.bin'}"], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (t, s, r, p.stderr[-2000:])
