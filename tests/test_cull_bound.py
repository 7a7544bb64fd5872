"""The capsule-form broad phase of the collision (csrc/usim_kernels.hip collide_cull, constant DevCfg::probe_cull2c of csrc/usim_setup.h) is conservative: whenever
its inequality says "cannot touch", no point of the probe's blade comes within ELEM_R of the element's axis segment.  On the CPU, from the constants the host computes:
tests/setup_dump.hip prints the probe's fields of DevCfg, tests/cull_dump.hip the new constant (setup_dump lists the fields it prints by name).

The blade is restated here from its description (usim_kernels.hip probe_sdf), not from the distance function: the hull of two circles in the cross-section -- radius
probe_r about the tip axis, probe_r2 about the upper axis probe_h away -- revolved about the axis direction and swept by +-probe_hl along site x and +-probe_hw along
site y; its lowest point lies probe_tip beyond the site along site z.  It is sampled as a point cloud; the elements are 10^5 random segments about random site poses,
two fifths of them grazing: placed at the cull radius +- 1 mm, with the nearest point inside the segment or at one of its ends.

Far pairs are settled by the triangle inequality on the CLOUD's own extent about the centre of the upper axis (asserted below to stay within the radius the
constant is built on); every rejected pair within 1.5 cm of the cull radius, the grazing ones among them, gets the full minimum over the cloud."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ELEM_R, ELEM_HL = 0.0075, 0.025              # csrc/usim_devmath.h (soft_box.xml:10)
PAIRS = 100_000


def _build(tmp, name):
    exe = tmp / name
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-std=c++17", "--offload-arch=gfx950", str(ROOT / "tests" / f"{name}.hip"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def constants(tmp_path_factory):
    """overrides -> the probe's DevCfg fields (float32 values as the kernels see them) and probe_cull2c"""
    tmp = tmp_path_factory.mktemp("cull_bound")
    setup, cull = _build(tmp, "setup_dump"), _build(tmp, "cull_dump")

    def run(*overrides):
        lines = {}
        for cmd in ([str(setup), "1", "0", "0", *overrides], [str(cull), *overrides]):
            out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
            lines.update({ln.split()[0]: ln.split()[1] for ln in out.splitlines() if ln.startswith(("C.probe_", "check"))})
        assert lines["check"] == "1"
        return {k[2:]: float(v) for k, v in lines.items() if k.startswith("C.")}
    return run


def blade_cloud(c, n_phi=16, n_arc=12, n_flank=8, n_rect=3):
    """points of the blade in the site frame [m, 3]"""
    r, r2, h, hl, hw, tip = c["probe_r"], c["probe_r2"], c["probe_h"], c["probe_hl"], c["probe_hw"], c["probe_tip"]
    cb = (r - r2) / h
    th = np.arctan2(cb, np.sqrt(1.0 - cb * cb))                             # direction of the flank's outward normal in the cross-section
    a0, a1 = np.linspace(-np.pi / 2, th, n_arc), np.linspace(th, np.pi / 2, n_arc)
    f = np.linspace(0.0, 1.0, n_flank)[1:-1]
    rho = np.concatenate([r * np.cos(a0), (1 - f) * r * np.cos(th) + f * r2 * np.cos(th), r2 * np.cos(a1)])
    py = np.concatenate([r * np.sin(a0), (1 - f) * r * np.sin(th) + f * (h + r2 * np.sin(th)), h + r2 * np.sin(a1)])   # along the axis direction: 0 = tip axis, h = upper axis
    phi = np.linspace(0.0, 2 * np.pi, n_phi, endpoint=False)
    bx, by = np.linspace(-hl, hl, n_rect), (np.linspace(-hw, hw, n_rect) if hw > 0 else np.zeros(1))
    BX, BY, PHI, K = np.meshgrid(bx, by, phi, np.arange(len(rho)), indexing="ij")
    pts = np.stack([BX + rho[K] * np.cos(PHI), BY + rho[K] * np.sin(PHI), tip - r - py[K]], axis=-1).reshape(-1, 3)
    return pts, np.array([0.0, 0.0, tip - r - h])                          # ... and the centre of the upper axis


def random_pairs(rng, n, centre_site, rc):
    """site poses (position, rotation with columns x y z) and element axis segments (midpoint, unit axis), world frame"""
    Q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    Q[:, :, 2] *= np.sign(np.linalg.det(Q))[:, None]
    Kx = rng.uniform(-0.5, 0.5, size=(n, 3)) + np.array([0.0, 0.0, 1.0])
    cw = Kx + np.einsum("nij,j->ni", Q, centre_site)
    ax = rng.normal(size=(n, 3))
    near_up = rng.random(n) < 0.5                                           # half the axes within ~20 degrees of world z, as on the torso's top face
    ax[near_up] = np.array([0.0, 0.0, 1.0]) + 0.2 * rng.normal(size=(int(near_up.sum()), 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    u = rng.normal(size=(n, 3))
    u -= ax * np.sum(u * ax, axis=1, keepdims=True)                          # a unit vector across the axis
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    kind = rng.random(n)
    dist = np.where(kind < 0.6, rng.uniform(0.0, 0.12, n), rc + rng.uniform(-1e-3, 1e-3, n))
    t0 = rng.uniform(-ELEM_HL, ELEM_HL, n)                                    # nearest point inside the segment ...
    end = kind > 0.9                                                          # ... or at an end: the direction to the centre then leans outwards
    side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    lean = rng.uniform(0.0, 1.0, n)
    d = np.where(end[:, None], u * np.sqrt(1 - lean ** 2)[:, None] + ax * (side * lean)[:, None], u)
    t0 = np.where(end, side * ELEM_HL, t0)
    mid = cw - d * dist[:, None] - ax * t0[:, None]
    return Kx, Q, mid, ax


def cull_says_cannot_touch(c, Kx, Q, mid, ax):
    """collide_cull's capsule form, as written there"""
    d = mid - (Kx - Q[:, :, 2] * (c["probe_r"] + c["probe_h"] - c["probe_tip"]))
    v = d - ax * np.clip(np.sum(d * ax, axis=1), -ELEM_HL, ELEM_HL)[:, None]
    return ~(np.sum(v * v, axis=1) < c["probe_cull2c"]), np.sqrt(np.sum(v * v, axis=1))


@pytest.mark.parametrize("overrides", [(), ("probe_halfwidth=0.01", "probe_tip=0.005")], ids=["shipped", "wide_blade"])
def test_a_culled_element_cannot_touch(constants, overrides):
    c = constants(*overrides)
    hh = np.hypot(c["probe_hl"], c["probe_hw"])
    radius = max(np.hypot(hh, c["probe_h"]) + c["probe_r"], hh + c["probe_r2"])           # every point of the blade within this of the centre of the upper axis
    rc = radius + ELEM_R + 1e-4
    assert abs(c["probe_cull2c"] - rc * rc) <= 2.0 ** -23 * rc * rc
    cloud, centre = blade_cloud(c)
    extent = np.linalg.norm(cloud - centre, axis=1).max()
    print(f"   blade cloud: {len(cloud)} points, at most {1e3 * extent:.2f} mm from the centre of the upper axis; the constant allows {1e3 * radius:.2f} mm")
    assert extent <= radius + 1e-9                                            # the containment the constant is built on
    rng = np.random.default_rng(20)
    Kx, Q, mid, ax = random_pairs(rng, PAIRS, centre, rc)
    culled, dist_c = cull_says_cannot_touch(c, Kx, Q, mid, ax)
    print(f"{overrides or 'shipped'}: the cull lets {100 * (1 - culled.mean()):.1f} % of {PAIRS} pairs through ({100 * (1 - culled[dist_c < 0.12].mean()):.1f} % of those within 12 cm)")
    assert 0.2 < culled.mean() < 0.9                                          # both answers are exercised
    # far pairs: |p - centre| <= extent for every point p of the cloud, so the nearest one is at least dist_c - extent away
    far = culled & (dist_c > rc + 0.015)
    assert np.all(dist_c[far] - extent > ELEM_R)
    near = np.nonzero(culled & ~far)[0]
    assert len(near) > PAIRS // 10                                            # the grazing band is populated
    ms = np.einsum("nji,nj->ni", Q[near], mid[near] - Kx[near]).astype(np.float32)     # the segment in the site frame
    as_ = np.einsum("nji,nj->ni", Q[near], ax[near]).astype(np.float32)
    P = cloud.astype(np.float32)
    worst = np.inf
    for s in range(0, len(near), 256):
        m, a = ms[s:s + 256, None, :], as_[s:s + 256, None, :]
        d = P[None, :, :] - m
        w = d - a * np.clip(np.sum(d * a, axis=2, keepdims=True), -ELEM_HL, ELEM_HL)
        worst = min(worst, float(np.sqrt(np.sum(w * w, axis=2)).min()))
    print(f"   smallest distance of a blade point from a culled element's axis: {1e3 * worst:.3f} mm (contact needs less than {1e3 * ELEM_R:.1f} mm)")
    assert worst > ELEM_R
