"""The lanes parse's tree and TB units (the TB-completion step of the
pass, the one-division PB mode bins), on the host emulation.

(a) small pictures that reach every changed path (tests/lanes_units_cases.py),
    each through the emulation's full decode against the oracle, in the lean and
    the general body; the emulation's path counters show that a picture reaches
    the paths its case is named for.
(b) the passes every wave of halfmoonbay.heic takes at three pictures per wave
    equal those of the commit before the TB-completion step (47,894 over 16
    waves, tests/golden/lanes_passes_halfmoonbay_ppw3.json): no lane needs a
    pass more or a pass fewer."""
import json
import os
import pathlib
import subprocess

import pytest

import lanes_units_cases as C
from conftest import make_emu

pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"


@pytest.fixture(scope="module")
def emu_check():
    make_emu("emu-fast")
    return str(CSRC / "build" / "emu_fast" / "emu_check")


def _emu(exe, args, **env):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "HEIFGPU_PARSE": "lanes", "HEIFGPU_LANES_STATS": "1", **env})
    return r.returncode, r.stdout + r.stderr


def _paths(out):
    tot = [0] * len(C.PATHS)
    for line in out.splitlines():
        if line.startswith("  paths"):
            v = [int(x) for x in line.split()[1:]]
            assert len(v) == len(C.PATHS), line
            tot = [a + b for a, b in zip(tot, v)]
    return dict(zip(C.PATHS, tot))


CASES = [(n, o, v) for n, o in C.LEAN.items() for v in ("auto", "general")] + \
        [(n, o, "auto") for n, o in C.GENERAL.items()]


@pytest.mark.parametrize("name,over,variant", CASES, ids=[f"{n}-{v}" for n, _, v in CASES])
def test_small_pictures_both_bodies(emu_check, tmp_path, name, over, variant):
    p = tmp_path / "p.heic"
    p.write_bytes(C.heic(over, C.CPU_SEED.get(name, 1)))
    rc, out = _emu(emu_check, [p, 5], HEIFGPU_LANES_VARIANT=variant)
    assert rc == 0 and "EMU PARITY OK" in out, out[-2000:]
    body = next(l.split(": ")[1] for l in out.splitlines() if l.startswith("lanes variant:"))
    assert body == ("lean" if name in C.LEAN and variant == "auto" else "general")
    paths = _paths(out)
    print(name, variant, paths)
    missing = [k for k in C.NEEDS[name] if paths[k] == 0]
    assert not missing, (missing, paths)


def test_pass_counts_equal_parent(emu_check):
    want = json.loads((ROOT / "tests/golden/lanes_passes_halfmoonbay_ppw3.json").read_text())
    rc, out = _emu(emu_check, [ROOT / "tests/golden/halfmoonbay.heic", 1], HEIFGPU_LANES_PPW="3")
    assert rc == 0, out[-2000:]
    got = [int(l.split()[2]) for l in out.splitlines() if l.startswith("wave ")]
    print(got)
    assert len(want["passes"]) == 16 and sum(want["passes"]) == 47894  # (the fixture itself)
    assert got == want["passes"]


def test_pass_order_knob_ignores_other_characters(emu_check, tmp_path):
    """HEIFGPU_EMU_PASS_ORDER: characters that name no unit kind are ignored (they were
    used as an index), so the default order with such characters between is the default."""
    p = tmp_path / "p.heic"
    p.write_bytes(C.heic(C.LEAN["tb_sizes"], 1))
    rc0, out0 = _emu(emu_check, [p, 5])
    rc1, out1 = _emu(emu_check, [p, 5], HEIFGPU_EMU_PASS_ORDER="1,2 3x4:5;6/8\x7f7 09")
    assert rc0 == 0 and rc1 == 0 and "EMU PARITY OK" in out1, out1[-2000:]
    waves = lambda o: [l for l in o.splitlines() if l.startswith("wave ")]
    assert waves(out0) and waves(out0) == waves(out1)
