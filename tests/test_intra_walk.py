"""k_intra's block walk over packed record words, on the host emulation.

(a) every picture of tests/intra_walk_cases.py through the emulation's full decode against the
    oracle, lanes parse (k_transform + k_intra), with and without the luma / chroma wave split;
    the `intra_walk` counters show that a picture reaches the walk events and TB kinds its case
    is named for, and the set as a whole every event;
(b) one picture through the streaming kernel (spread parse), which shares the walk;
(c) the packed words alone: the stand-alone driver tests/intra_walk/pack_driver.cpp under
    ASan + UBSan (round trip of every reachable combination, damaged records, random records);
(d) three pictures through the sanitizer build of the stand-alone checker, whose LDS block is
    exactly as large as the library's."""
import os
import pathlib
import subprocess

import pytest

import intra_walk_cases as C
from conftest import make_emu

pytest.importorskip("heif_amd.synth_encoder")

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


def _run(exe, heic, mode, timeout=300, **env):
    r = subprocess.run([exe, str(heic), "5"], capture_output=True, text=True, timeout=timeout,
                       env={**os.environ, "HEIFGPU_PARSE": mode, "HEIFGPU_INTRA_STATS": "1", **env})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and "EMU PARITY OK" in out, (mode, env, out[-2000:])
    return out


def _counters(out):
    """The last `intra_walk` line (the process's totals), by name."""
    lines = [l for l in out.splitlines() if l.startswith("intra_walk ")]
    assert lines, out[-2000:]
    f = lines[-1].split()[1:]
    got = dict(zip(f[0::2], (int(v) for v in f[1::2])))
    assert tuple(got) == C.COUNTERS, got
    return got


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_matches_the_oracle_and_reaches_its_events(emu_check, tmp_path, name):
    heic = tmp_path / "p.heic"
    heic.write_bytes(C.heic(name))
    out = _run(emu_check, heic, "lanes", HEIFGPU_INTRA_SPLIT="0")
    assert "parse mode: lanes" in out
    got = _counters(out)
    print(name, got)
    assert got["records"] > 0 and got["ok"] == got["records"] and got["ctus"] > 0, got
    missing = [k for k in C.NEEDS.get(name, ()) if got[k] == 0]
    assert not missing, (missing, got)
    if C.CASES[name].get("chroma_format", 1):
        split = _counters(_run(emu_check, heic, "lanes", HEIFGPU_INTRA_SPLIT="1"))
        # the luma waves count the records and the walk's events, the chroma waves the pairs
        for k in ("records", "ok", "ctus", "blocks", "pairs", "pair_splits", "ctu_lane0", "blocks_no_ctu"):
            assert split[k] == got[k], (k, split, got)


def test_every_walk_event_has_a_case():
    needed = {k for v in C.NEEDS.values() for k in v}
    assert set(C.EVENTS) <= needed, set(C.EVENTS) - needed
    assert {"tb32_strong", "luma4", "pcm", "pairs"} <= needed


def test_streaming_kernel_shares_the_walk(emu_check, tmp_path):
    heic = tmp_path / "p.heic"
    heic.write_bytes(C.heic("wide_ctb32"))
    out = _run(emu_check, heic, "spread")
    assert "parse mode: spread" in out
    got = _counters(out)
    assert got["records"] > 0 and got["ok"] == got["records"] and got["pairs"] == 0, got


def test_packed_words_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "intra-pack-asan"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = CSRC / "build" / "intra_pack_asan" / "pack_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={**os.environ, **SAN_ENV})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and "INTRA PACK OK" in out, out[-2000:]


@pytest.mark.parametrize("name", ["72x40_ctb64", "cu8", "c422"])
def test_sanitizer_build_runs_clean(emu_asan, tmp_path, name):
    heic = tmp_path / "p.heic"
    heic.write_bytes(C.heic(name))
    _run(emu_asan, heic, "lanes", timeout=600, **SAN_ENV)
