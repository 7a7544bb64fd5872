"""The snapshot row sizes of the ctypes binding equal the USIM_SNAPSHOT_WORDS_* macros of include/usim.h (read as text, like tests/test_pack_layout.py), they are the
sums of the regions a row is made of, and every one is a whole number of 16-byte units."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "usim.h").read_text()

ROWS = {"RIGID": 40, "TOP": 240, "TOP_WARM": 312, "FULL": 1752}


def _macro(name):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", HEADER, flags=re.M)
    assert m, f"{name} is not an integer macro of include/usim.h"
    return int(m.group(1))


@pytest.mark.parametrize("name", sorted(ROWS))
def test_constants_equal_the_header_macros(usim, name):
    value = getattr(usim._lib, "SNAPSHOT_WORDS_" + name)
    assert value == _macro("USIM_SNAPSHOT_WORDS_" + name) == ROWS[name]
    assert value % 4 == 0                                        # rows move as 16-byte accesses


def test_rows_are_the_sums_of_their_regions(usim):
    L = usim._lib
    assert L.SNAPSHOT_WORDS_RIGID == L.NSCALAR == _macro("USIM_NSCALAR")
    assert L.SNAPSHOT_WORDS_TOP == L.NSCALAR + 200
    assert L.SNAPSHOT_WORDS_TOP_WARM == L.SNAPSHOT_WORDS_TOP + L.WARM_WORDS
    assert L.SNAPSHOT_WORDS_FULL == L.NSCALAR + 1712


def test_the_three_entry_points_are_bound(usim):
    for name in ("usim_snapshot_words", "usim_save_envs", "usim_load_envs"):
        assert name in usim._lib.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER)


@pytest.mark.parametrize("torso,warm,words", [
    ("rigid", False, 40), ("none", False, 40), ("rigid", True, 40), (0, False, 40),
    ("soft", False, 240), ("top", False, 240), ("soft", True, 312), (1, True, 312),
    ("full", False, 1752), ("full", True, 1752), (2, False, 1752)])
def test_snapshot_words(usim, torso, warm, words):
    assert usim._lib.snapshot_words(torso, warm) == words
    assert usim._lib.snapshot_words(torso, warm=int(warm)) == words


def test_snapshot_words_refuses_an_unknown_torso(usim):
    with pytest.raises((ValueError, KeyError)):
        usim._lib.snapshot_words(3)
    with pytest.raises((ValueError, KeyError)):
        usim._lib.snapshot_words("cloth")
