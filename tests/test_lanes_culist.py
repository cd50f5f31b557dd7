"""The lanes parse's CU lists and word-wise neighbour lines, on the host emulation.

(a) every picture of tests/lanes_culist_cases.py through the emulation's full decode against
    the oracle, lanes and solo; the QpY and flag maps the deblocking read
    (HEIFGPU_EMU_DUMP_MAPS, as in test_lanes_maps.py) are the same bytes, none the arena's
    sentinel; the `cu_paths` and `paths` counters show that a picture reaches the CU sizes
    and the NxN CUs its case is named for.  The lean picture in both bodies.
(b) the whole-CTB CU and the clipped 72x40 pictures through the sanitizer build of the
    stand-alone checker, whose CU list is exactly as large as the library's.
(c) a 64x64 picture with one byte of slice data damaged, 8 seeds, through the sanitizer
    build: a status or parity, and no access outside the CU list (or anywhere else)."""
import os
import pathlib
import random
import subprocess

import pytest

import lanes_culist_cases as C
import lanes_units_cases as U
from conftest import make_emu

S = pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
SAN_ENV = dict(ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.fixture(scope="module")
def emu_check():
    make_emu("emu-fast")
    return str(CSRC / "build" / "emu_fast" / "emu_check")


@pytest.fixture(scope="module")
def emu_asan():
    make_emu("emu")
    return str(CSRC / "build" / "emu" / "emu_check")


def _run(exe, heic, dump, mode, **env):
    r = subprocess.run([exe, str(heic), "5"], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "HEIFGPU_PARSE": mode, "HEIFGPU_EMU_DUMP_MAPS": str(dump),
                            "HEIFGPU_LANES_STATS": "1", **env})
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "EMU PARITY OK" in out, (mode, out[-2000:])
    return out, dump.read_bytes()


def _paths(out):
    """The `paths` and `cu_paths` counters of every wave, summed, by name."""
    tot = {"  paths": [0] * len(U.PATHS), "  cu_paths": [0] * len(C.CU_PATHS)}
    for line in out.splitlines():
        for key, acc in tot.items():
            if line.startswith(key + " "):
                v = [int(x) for x in line.split()[1:]]
                assert len(v) == len(acc), line
                acc[:] = [a + b for a, b in zip(acc, v)]
    return {**dict(zip(U.PATHS, tot["  paths"])), **dict(zip(C.CU_PATHS, tot["  cu_paths"]))}


def _same_maps(lanes, solo):
    assert len(lanes) == len(solo) and len(lanes) > 0
    bad = [i for i in range(len(lanes)) if lanes[i] != solo[i]]
    assert not bad, (len(bad), bad[:8], [(lanes[i], solo[i]) for i in bad[:8]])
    assert 0xa5 not in lanes  # (a flag byte is below 8; a QpY of -91 cannot occur)


@pytest.mark.parametrize("name", list(C.CASES))
def test_maps_equal_the_solo_parse(emu_check, tmp_path, name):
    heic = tmp_path / "p.heic"
    heic.write_bytes(C.heic(name))
    out_l, lanes = _run(emu_check, heic, tmp_path / "lanes.bin", "lanes")
    out_s, solo = _run(emu_check, heic, tmp_path / "solo.bin", "solo")
    assert "parse mode: lanes" in out_l and "parse mode: solo" in out_s
    _same_maps(lanes, solo)
    paths = _paths(out_l)
    print(name, {k: paths[k] for k in C.CU_PATHS + ("nxn",)})
    missing = [k for k in C.NEEDS[name] if paths[k] == 0]
    assert not missing, (missing, paths)
    reached = [k for k in C.ZERO.get(name, ()) if paths[k] != 0]
    assert not reached, (reached, paths)


def test_every_cu_size_has_a_case():
    needed = {k for v in C.NEEDS.values() for k in v}
    assert set(C.CU_PATHS) | {"nxn"} <= needed


def test_lean_picture_in_both_bodies(emu_check, tmp_path):
    heic = tmp_path / "p.heic"
    heic.write_bytes(C.heic("lean"))
    out_a, lean = _run(emu_check, heic, tmp_path / "lean.bin", "lanes", HEIFGPU_LANES_VARIANT="auto")
    out_g, gen = _run(emu_check, heic, tmp_path / "gen.bin", "lanes", HEIFGPU_LANES_VARIANT="general")
    _, solo = _run(emu_check, heic, tmp_path / "solo.bin", "solo")
    assert "lanes variant: lean" in out_a and "lanes variant: general" in out_g
    _same_maps(lean, solo)
    _same_maps(gen, solo)


@pytest.mark.parametrize("name", ["cu64", "72x40_ctb64", "72x40_ctb16"])
def test_sanitizer_build_runs_clean(emu_asan, tmp_path, name):
    heic = tmp_path / "p.heic"
    heic.write_bytes(C.heic(name))
    r = subprocess.run([emu_asan, str(heic), "5"], capture_output=True, text=True, timeout=600,
                       env={**os.environ, **SAN_ENV, "HEIFGPU_PARSE": "lanes"})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and "EMU PARITY OK" in out, out[-2000:]


def _damaged(seed):
    """A 64x64 picture (four CTBs of 32, CUs of 8 to 32) with one bit of one slice-data byte flipped."""
    from oracle import oracle

    clean = S.single_heic(C.params(dict(width=64, height=64, log2_ctb=5, max_th_depth_intra=1)), seed=1)
    (o, n), = oracle.list_tiles(clean)[0]
    d = bytearray(clean)
    rng = random.Random(seed)
    k = o + 30 + rng.randrange(n - 30)  # past the NAL and slice headers
    d[k] ^= 1 << rng.randrange(8)
    return bytes(d)


@pytest.mark.parametrize("seed", range(8))
def test_damaged_stream_ends_in_status_or_parity(emu_asan, tmp_path, seed):
    heic = tmp_path / "p.heic"
    heic.write_bytes(_damaged(seed))
    r = subprocess.run([emu_asan, str(heic), "5"], capture_output=True, text=True, timeout=600,
                       env={**os.environ, **SAN_ENV, "HEIFGPU_PARSE": "lanes"})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode in (0, 1), out[-2000:]
    line = next(l for l in out.splitlines() if l.startswith("parse: status"))
    status = int(line.split()[2].rstrip(","), 16)
    print(seed, hex(status), r.returncode)
    assert status != 0 or "EMU PARITY OK" in out, out[-2000:]
