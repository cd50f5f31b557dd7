"""A TB record's neighbour facts (word D of kernels/intra_rec.hpp) on the CPU.

k_intra no longer decides per sample whether a neighbour is decoded: where a wave loads its
records, each lane packs five facts of its record (below-left and above-right prefix lengths,
the left column, the row above, the corner), and the gather reads, per search position, the
sample that stands there after the substitution of 8.4.4.2.2 by a closed form on those facts.

The stand-alone driver tests/intra_avail/avail_driver.cpp (ASan + UBSan, its own main) holds
the facts, the closed form and the window addresses against the per-sample rule of 6.4.1,
restated there with a z-scan index of its own, over every format, CTB size, TB size and
position, picture extent and picture edge.  Three seconds with its build.
"""
import os
import pathlib
import re
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
SAN_ENV = dict(ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


def test_neighbour_facts_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "intra-avail-asan"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = CSRC / "build" / "intra_avail_asan" / "avail_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={**os.environ, **SAN_ENV})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0, out[-2000:]
    m = re.search(r"INTRA AVAIL OK (\d+) cases (\d+) checks", out)
    assert m, out[-2000:]
    # the enumerated space: more than 400,000 TBs, each with its 4n + 1 samples three ways
    assert int(m.group(1)) > 400000 and int(m.group(2)) > 20 * int(m.group(1))
