"""The layout of the state block and the checkpoint conversions of csrc/usim_checkpoint.h (usim_get_state / usim_set_state, the full torso's body state, the warm list),
on the CPU.  tests/checkpoint_dump.hip, a host program, runs them on arrays this file writes; the rules are restated below in numpy and compared bit for bit.

No tolerance: every conversion is a copy, one IEEE float32 addition or subtraction, an exact float32 -> float64 widening with one float64 addition or subtraction and
one narrowing, or a cast between an int32 and a float of a small integer, and numpy performs the same operations.  Arrays are compared as their uint32 / uint64 bit
patterns, so that NaN and -0.0 count."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32

# csrc/usim_device.h and include/usim.h, restated
NSCALAR, F_Q, F_Q0, NJ, F_LAT, WG = 40, 0, 14, 7, 40, 64
INT_FIELDS = (35, 36, 37, 39)                                  # t, has_touched, episode, status
BANK_ROWS = 256 * 40
N_TOP, LAT_ENV_WORDS, LAT_S, LAT_SD = 99, 200, 0, 100
NSH, LATF_ENV_WORDS, LATF_S, LATF_SD, LATF_BODY, LATF_WTAB = 270, 1712, 0, 272, 544, 560
LATF_WARM_WORDS = 4 * NSH + 8 + 64
BODY_WORDS = 13 + LATF_WARM_WORDS
PROBE_SLOTS = slice(4 * NSH, 4 * NSH + 8)                      # warm-start words that hold the elements of the probe contact slots
WARM_WORDS, MAXC = 72, 8
BASE = np.array([-0.56, 0.0, 0.913], dtype=f32)               # the robot base (csrc/usim_setup.h kBase), narrowed as DevModel::base is

KINDS = {   # n_el, nfields, lattice words and the offsets of s and sdot in them, warm words, snapshot row words
    "rigid": dict(n_el=0, nfields=40, lat_words=0, lat_s=LAT_S, lat_sd=LAT_SD, warm_words=0, snapshot_words=40),
    "top": dict(n_el=N_TOP, nfields=240, lat_words=LAT_ENV_WORDS, lat_s=LAT_S, lat_sd=LAT_SD, warm_words=0, snapshot_words=240),
    "warm": dict(n_el=N_TOP, nfields=240, lat_words=LAT_ENV_WORDS, lat_s=LAT_S, lat_sd=LAT_SD, warm_words=WARM_WORDS, snapshot_words=312),
    "full": dict(n_el=NSH, nfields=1752, lat_words=LATF_ENV_WORDS, lat_s=LATF_S, lat_sd=LATF_SD, warm_words=0, snapshot_words=1752),
}
CASES = [(kind, n) for kind in KINDS for n in (1, 70)]         # npad 64 and 128: the second has padding environments
WARM_IN = np.array([-1, 0, 98, 99, 1e9, np.nan, 3.7, 50], dtype=f32)                    # elements handed to usim_set_warm_start ...
WARM_OUT = np.array([-1, 0, 98, -1, -1, -1, 3, 50], dtype=i32)                             # ... and what the device gets: outside [0, 99) an empty slot, a NaN as well
ODD = np.array([np.nan, -0.0, np.inf, 1e-42, -np.inf], dtype=f32)      # values a copy must carry bit for bit (1e-42: a denormal)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: u32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def marker(words):
    """a block in which every word differs: small negative float32 numbers"""
    return (u32(0xA5000000) + np.arange(words, dtype=u32)).view(f32)


class Run:
    """one run of the program: its inputs, the layout lines it prints and the arrays it writes"""

    def __init__(self, exe, tmp, kind, n):
        k = KINDS[kind]
        self.kind, self.n, self.npad, self.k = kind, n, (n + WG - 1) // WG * WG, k
        rng = np.random.default_rng(1000 * n + len(kind))
        self.block = marker(k["nfields"] * self.npad)
        sc = rng.standard_normal((n, NSCALAR)).astype(f32)
        ints = np.array([0.0, 1.0, 3.7, 2.0 ** 24, 2.0 ** 24 - 1, 999.999, 12.0, 0.5], dtype=f32)     # up to 2^24, fractional (truncated), 0
        for j, f in enumerate(INT_FIELDS):
            sc[:, f] = ints[(np.arange(n) + 3 * j) % ints.size]
        copies = [f for f in range(NSCALAR) if f >= NJ and f not in INT_FIELDS and not F_Q0 <= f < F_Q0 + NJ]
        for i in range(n):
            sc[i, copies[i % len(copies)]] = ODD[i % ODD.size]
        sc[0, copies[:ODD.size]] = ODD
        self.scalars = sc
        self.lattice = rng.standard_normal((n, k["n_el"], 2)).astype(f32)
        if k["n_el"]:
            self.lattice[:, 1:1 + ODD.size, 0] = ODD
            self.lattice[:, -ODD.size:, 1] = ODD
        parts = [self.block, self.scalars, self.lattice]
        if kind == "full":
            body = rng.standard_normal((n, BODY_WORDS))                                        # float64 numbers that no float32 holds
            # positions: the float64 sum of the base and a float32 offset within a factor 2^20 of the base's magnitude (0 for the y axis: of 1), so that the device word
            # is known; environment 0 keeps general float64 positions
            self.offset = (np.where(BASE == 0, 1, np.abs(BASE)) * 2.0 ** rng.uniform(-20, 20, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(f32)
            body[1:, :3] = self.offset[1:].astype(f64) + BASE.astype(f64)
            body[:, 13:][:, PROBE_SLOTS] = np.array([-1.0, 0.0, 5.0, 269.0, 3.7, -1.0, 98.0, 12.0])[(np.arange(8)[None, :] + np.arange(n)[:, None]) % 8]
            body[:, 13 + 7] = np.inf
            body[:, 13 + 9] = -0.0
            self.body = body
            parts += [BASE, body]
        if kind == "warm":
            w = rng.standard_normal((n, WARM_WORDS)).astype(f32)
            self.slot = (np.arange(MAXC)[None, :] + np.arange(n)[:, None]) % len(WARM_IN)        # which of WARM_IN stands in slot k of environment i
            w[:, :MAXC] = WARM_IN[self.slot]
            w[:, MAXC:MAXC + ODD.size] = ODD
            self.w = w
            parts.append(w)
        stem = tmp / f"{kind}_{n}"
        Path(f"{stem}.in").write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))
        out = subprocess.run([str(exe), kind, str(n), f"{stem}.in", str(stem)], capture_output=True, text=True, check=True).stdout
        self.layout = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
        self.stem = stem

    def out(self, name, dtype=f32):
        return np.fromfile(f"{self.stem}.{name}", dtype=dtype)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("checkpoint_dump")
    exe = tmp / "checkpoint_dump"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-std=c++17", "--offload-arch=gfx950", str(ROOT / "tests" / "checkpoint_dump.hip"), "-o", str(exe)], check=True)
    return {case: Run(exe, tmp, *case) for case in CASES}


@pytest.mark.parametrize("kind, n", CASES)
def test_layout(runs, kind, n):
    r, k = runs[kind, n], KINDS[kind]
    L = r.layout
    assert L["n"] == n and L["npad"] == r.npad and r.npad % WG == 0 and 0 <= r.npad - n < WG
    for name in ("n_el", "nfields", "lat_words", "warm_words", "snapshot_words"):
        assert L[name] == k[name], name
    assert L["bank_row0"] == L["nfields"]
    assert L["words"] == (L["nfields"] + BANK_ROWS) * r.npad + L["warm_words"] * r.npad
    assert L["live_words"] == L["nfields"] * r.npad and L["lattice0"] == F_LAT * r.npad and L["warm0"] == (L["bank_row0"] + BANK_ROWS) * r.npad
    if k["n_el"]:
        assert (L["lat_s"], L["lat_sd"]) == (k["lat_s"], k["lat_sd"])


def expected_state_block(r):
    """the marker block with the words the conversion owns replaced: environment i's field f at i * 40 + f, s and sdot at their offsets of the environment's lattice words"""
    want = bits(r.block).copy()
    sc = r.scalars
    words = bits(sc).copy()
    words[:, F_Q:F_Q + NJ] = bits(sc[:, F_Q:F_Q + NJ] - sc[:, F_Q0:F_Q0 + NJ])                 # the device holds dq = q - q0: one float32 subtraction
    for f in INT_FIELDS:
        words[:, f] = sc[:, f].astype(i32).view(u32)                                             # the truncated number as an int
    want[:r.n * NSCALAR] = words.reshape(-1)
    k = r.k
    for i in range(r.n):
        at = F_LAT * r.npad + i * k["lat_words"]
        want[at + k["lat_s"]:at + k["lat_s"] + k["n_el"]] = bits(r.lattice[i, :, 0])
        want[at + k["lat_sd"]:at + k["lat_sd"] + k["n_el"]] = bits(r.lattice[i, :, 1])
    return want


@pytest.mark.parametrize("kind, n", CASES)
def test_state_host_to_device(runs, kind, n):
    """scalars, lattice, and everything the conversion does not own: the whole block against marker-or-expected"""
    r = runs[kind, n]
    got, want = bits(r.out("state_dev")), expected_state_block(r)
    assert got.shape == want.shape and np.array_equal(got, want)
    mark = bits(r.block)
    assert np.array_equal(got[n * NSCALAR:r.npad * NSCALAR], mark[n * NSCALAR:r.npad * NSCALAR])                  # the padding environments' scalar words
    k = r.k
    if k["n_el"]:
        at = F_LAT * r.npad + (n - 1) * k["lat_words"]
        gap = slice(at + k["lat_s"] + k["n_el"], at + k["lat_sd"])                                             # between the last s and the first sdot
        assert gap.stop > gap.start and np.array_equal(got[gap], mark[gap])
        rest = slice(at + k["lat_sd"] + k["n_el"], None)                                                       # behind the last sdot: the rest of the row, the padding rows
        assert np.array_equal(got[rest], mark[rest])
        assert not np.array_equal(got[at:at + k["n_el"]], mark[at:at + k["n_el"]])


@pytest.mark.parametrize("kind, n", CASES)
def test_state_device_to_host(runs, kind, n):
    r = runs[kind, n]
    dev = r.out("state_dev")[:n * NSCALAR].reshape(n, NSCALAR)
    want = dev.copy()
    want[:, F_Q:F_Q + NJ] = dev[:, F_Q0:F_Q0 + NJ] + dev[:, F_Q:F_Q + NJ]                     # q = q0 + dq: one float32 addition
    for f in INT_FIELDS:
        want[:, f] = dev[:, f].view(i32).astype(f32)
    assert same(r.out("state_scalars").reshape(n, NSCALAR), want)
    # against the inputs: the int fields come back truncated, the copies with their bits (NaN, -0.0, a denormal among them)
    got = r.out("state_scalars").reshape(n, NSCALAR)
    copies = [f for f in range(NJ, NSCALAR) if f not in INT_FIELDS]
    assert same(got[:, copies], r.scalars[:, copies])
    assert same(got[:, list(INT_FIELDS)], np.trunc(r.scalars[:, list(INT_FIELDS)]))
    assert same(r.out("state_lattice").reshape(r.lattice.shape), r.lattice)


@pytest.mark.parametrize("n", [1, 70])
def test_full_torso_body(runs, n):
    r = runs["full", n]
    off = np.zeros(13); off[:3] = BASE.astype(f64)
    want = bits(r.block)[F_LAT * r.npad:].copy().reshape(r.npad, LATF_ENV_WORDS)
    want[:n, LATF_BODY:LATF_BODY + 13] = bits((r.body[:, :13] - off).astype(f32))               # float32(float64(x) - float64(base)), base 0 behind the position
    warm = bits(r.body[:, 13:].astype(f32)).copy()                                               # float32 narrowings ...
    warm[:, PROBE_SLOTS] = r.body[:, 13:][:, PROBE_SLOTS].astype(i32).view(u32)                  # ... but the probe slots' elements: ints, truncated, -1 included
    want[:n, LATF_WTAB:LATF_WTAB + LATF_WARM_WORDS] = warm
    got = bits(r.out("body_dev")).reshape(r.npad, LATF_ENV_WORDS)
    assert np.array_equal(got, want)                       # with s, sdot, the words between the regions and the padding environments as the marker left them
    if n > 1:
        assert np.array_equal(got[1:n, LATF_BODY:LATF_BODY + 3], bits(r.offset[1:]))           # the float32 offsets the positions were made of
    dev = got.view(f32)
    back = np.concatenate([dev[:n, LATF_BODY:LATF_BODY + 13].astype(f64) + off, dev[:n, LATF_WTAB:LATF_WTAB + LATF_WARM_WORDS].astype(f64)], axis=1)
    back[:, 13:][:, PROBE_SLOTS] = got[:n, LATF_WTAB:LATF_WTAB + LATF_WARM_WORDS][:, PROBE_SLOTS].view(i32).astype(f64)
    assert same(r.out("body_back", f64).reshape(n, BODY_WORDS), back)
    assert np.array_equal(bits(r.out("body_dev2")).reshape(r.npad, LATF_ENV_WORDS), got)       # device -> host -> device restores the device bits


@pytest.mark.parametrize("n", [1, 70])
def test_warm_list(runs, n):
    r = runs["warm", n]
    empty = bits(r.out("warm_empty")).reshape(r.npad, WARM_WORDS)
    assert np.all(empty[:, :MAXC].view(i32) == -1) and np.all(empty[:, MAXC:] == 0)            # eight int32 -1, then 64 zero words, every environment of the block
    el = r.w[:, :MAXC]
    with np.errstate(invalid="ignore"):
        kept = (el >= 0) & (el < N_TOP)                                                          # a NaN fails both comparisons
    rule = np.where(kept, np.where(kept, el, 0).astype(i32), -1).astype(i32)
    assert np.array_equal(rule, WARM_OUT[r.slot])
    want = bits(r.w).copy()
    want[:, :MAXC] = rule.view(u32)
    dev = bits(r.out("warm_dev")).reshape(n, WARM_WORDS)
    assert np.array_equal(dev, want)
    back = dev.view(f32).copy()
    back[:, :MAXC] = dev[:, :MAXC].view(i32).astype(f32)                                         # the elements as numbers; the 64 force words bit for bit
    assert same(r.out("warm_back").reshape(n, WARM_WORDS), back)
    assert same(r.out("warm_back").reshape(n, WARM_WORDS)[:, MAXC:], r.w[:, MAXC:])
