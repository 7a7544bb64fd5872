"""The layout constants of usim_pack_step in the ctypes binding equal the macros of include/usim.h (read as text, like tests/test_host_api.py reads the
declarations), and the binding's size formula is the header's USIM_PACK_WORDS(n)."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "usim.h").read_text()


def _macro(name):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", HEADER, flags=re.M)
    assert m, f"{name} is not an integer macro of include/usim.h"
    return int(m.group(1))


def test_constants_equal_the_header_macros(usim):
    L = usim._lib
    assert L.PACK_HEAD_WORDS == _macro("USIM_PACK_HEAD_WORDS") == L.OBS_DIM + 2            # obs[19], rew, done
    assert L.PACK_EPISODE_WORDS == _macro("USIM_PACK_EPISODE_WORDS") == L.OBS_DIM + 4      # env, length, return, status, terminal observation[19]
    assert L.OBS_DIM == _macro("USIM_OBS_DIM")
    m = re.search(r"^#define\s+USIM_PACK_WORDS\(n\)\s+(.*)$", HEADER, flags=re.M)
    assert m and re.sub(r"\s+", "", m.group(1)) == "(4+(size_t)(n)*(USIM_PACK_HEAD_WORDS+USIM_PACK_EPISODE_WORDS))"
    assert "usim_pack_step" in L.SYMBOLS


@pytest.mark.parametrize("n", [1, 67, 256, 4096, 8192])
def test_pack_words(usim, n):
    assert usim._lib.pack_words(n) == 4 + n * 44
    assert usim._lib.pack_words(n) % 4 == 0                      # the block is a whole number of 16-byte units


def test_pack_words_as_the_c_compiler_sees_it(usim, tmp_path):
    """the macro itself, expanded by the system compiler (also past 2^31 bytes: the product is formed in size_t)"""
    ns = [1, 67, 4096, 8192, 60_000_000]
    src = '#include "usim.h"\n#include <stdio.h>\nint main(){' + "".join(f'printf("%zu ", USIM_PACK_WORDS({n}));' for n in ns) + "return 0;}"
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")], check=True)
    out = subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [usim._lib.pack_words(n) for n in ns]
