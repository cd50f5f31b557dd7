"""What k_transform reads off a TB's records instead of its coefficient tile.

The DC-only test, the dot products' extents, the scaling and pass A's rounds, on
hand-built records (tests/xform_walk_vectors.py) through the kernel alone
(tests/xform/xform_driver.cpp) against the integer model of 8.6.2-8.6.4 in
tests/xform_vectors.py, with a sentinel surviving wherever no coded TB lies.  As in
tests/test_transform.py the vectors run through the host emulation here and, marked gpu,
through the product library (the ballot loops, the wave reduction of the extents and the
MFMA stages exist only there).  The record-side arithmetic alone (kernels/xform_rec.hpp)
runs as a stand-alone ASan + UBSan program.
"""
import os
import pathlib
import subprocess

import numpy as np
import pytest

import xform_vectors as xv
import xform_walk_vectors as wv
from conftest import make_emu

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
DRIVER_SRC = ROOT / "tests" / "xform" / "xform_driver.cpp"
CASE_NAMES = list(wv.CASES)
SAN_ENV = dict(ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


def run_case(exe, name, tmp_path, timeout=120):
    c = wv.case(name)
    src, out = tmp_path / f"{name}.bin", tmp_path / f"{name}.resid"
    src.write_bytes(c.blob)
    r = subprocess.run([str(exe), str(src), str(out)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"driver failed ({r.returncode}): {r.stderr}"
    return c.failures(np.fromfile(out, dtype=np.int16))


def report(bad):
    return f"{len(bad)} vectors differ from the model, the first of them:\n" + "\n".join(bad[:10])


@pytest.fixture(scope="module")
def emu_driver():
    make_emu("xform-emu")
    return CSRC / "build" / "emu_fast" / "xform_driver"


@pytest.fixture(scope="module")
def gpu_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("xform_walk_driver") / "xform_driver"
    lib_dir = ROOT / "heif_amd"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wextra", f"-I{CSRC}",
           str(DRIVER_SRC), f"-L{lib_dir}", "-lheifgpu", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


# ---------------------------------------------------------------- coverage, from the vectors alone
def _tbs(name):
    c = wv.case(name)
    return [t for p in c.pics for t in p.tbs]


def test_pictures_are_small_and_hold_both_kinds_of_sample():
    for name in CASE_NAMES:
        c = wv.case(name)
        assert all(s.width <= 64 and s.height <= 64 for s in c.seqs)
        assert (c.expected == xv.SENTINEL).any() and (c.expected != xv.SENTINEL).any(), name


def test_coverage_dc_boundary():
    tbs = _tbs("dc")
    for n in (8, 16, 32):
        for cidx in (0, 1):
            yes = [t for t in tbs if t.name.startswith("dc/yes/") and t.n == n and t.cidx == cidx]
            assert {t.scan_idx for t in yes} == {0, 1, 2}
            assert all(np.count_nonzero(t.levels) == 1 and t.levels[0, 0] for t in yes)
            assert any(t.hide == "force" for t in yes) and any(abs(t.levels[0, 0]) >= 16 for t in yes)
            assert any(t.levels[0, 0] < 0 for t in yes)
            no = {t.name.rsplit("/", 1)[1] for t in tbs if t.name.startswith(f"dc/no/n{n}/c{cidx}/")}
            assert no >= {"sig2", "subblock_1_0", "subblock_0_1", "two_records_scan0", "two_records_scan1",
                          "two_records_scan2", "tskip", "bypass"}, no
            assert any(t.name.startswith("dc/list/") and t.n == n and t.cidx == cidx for t in tbs)
    # the lists the DC TBs lie under have a factor other than 16 at (0, 0)
    c = wv.case("dc")
    m16 = [xv.sf_matrix(s.sf, 8, 0)[0, 0] for s in c.seqs if s.sf is not None]
    assert m16 and all(m != 16 for m in m16)


def test_coverage_extents():
    tbs = [t for t in _tbs("extents") if t.n == 8]
    seen = set()
    for t in tbs:
        mask = sum(1 << b for b, (x, y) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1)))
                   if t.levels[4 * y:4 * y + 4, 4 * x:4 * x + 4].any())
        assert np.count_nonzero(t.levels) == bin(mask).count("1")  # one coefficient per sub-block
        seen.add((mask, "k0" if t.name.endswith("scan_pos0") else "k15"))
    assert seen == {(m, k) for m in range(1, 16) for k in ("k0", "k15")}


def test_coverage_scaling():
    tbs = _tbs("scaling")
    c = wv.case("scaling")
    want = set(wv.SCALING_LEVELS)
    for t in tbs:
        if np.count_nonzero(t.levels) > 1:
            assert set(t.levels[t.levels != 0].tolist()) == want, t.name
    flat8 = [i for i, s in enumerate(c.seqs) if s.bd_y == 8 and s.sf is None]
    assert flat8 == [0]
    assert {int(s.sf[0]) for s in c.seqs if s.sf is not None} == {1, 16, 255}
    for si, s in enumerate(c.seqs):
        mine = [t for p in c.pics if p.seq == si for t in p.tbs]
        if s.bd_y == 8:
            assert {(t.qp, t.n) for t in mine} >= {(q, n) for q in (0, 5, 6, 51) for n in (4, 8, 16, 32)}
        else:
            top = 51 + 6 * (s.bd_y - 8)
            assert {t.n for t in mine if t.qp == top} == {4, 8, 16, 32}


def test_coverage_pass_a_rounds():
    assert wv.ballot_rounds(wv.case("pass_a")) >= {1, 2, 3, 4, 5, 6, 7}
    tbs = [t for t in _tbs("pass_a") if t.n == 4 and t.coded]
    assert {t.cidx for t in tbs} == {0, 1, 2} and {t.dst for t in tbs} == {False, True}
    assert len({t.qp for t in tbs}) > 20


def test_coverage_no_write():
    c = wv.case("no_write")
    names = [t.name for t in _tbs("no_write")]
    for part in ("log2_1", "log2_6", "cidx3/", "right/n4/", "bottom/n32/", "right/n8/c1", "bottom/n16/c2", "assembly/"):
        assert any(part in n for n in names), part
    assert any(p.flags & xv.PD_ASSEMBLY for p in c.pics)
    recs = np.concatenate([r for _, _, r in c.rows_tus])
    assert {1, 6} <= set(recs["log2"].tolist()) and (recs["flags"] & xv.TU_CIDX_MASK == 3).any()
    assert (recs["flags"] & xv.TU_CBF).all()  # every one of them would write if it ran


# ---------------------------------------------------------------- the record-side arithmetic alone
def test_record_arithmetic_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "xform-pack-asan"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = CSRC / "build" / "xform_pack_asan" / "pack_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={**os.environ, **SAN_ENV})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and "XFORM PACK OK" in out, out[-2000:]


# ---------------------------------------------------------------- the two legs
@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulated_transform_equals_model(emu_driver, tmp_path, name):
    bad = run_case(emu_driver, name, tmp_path)
    assert not bad, report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_transform_equals_model(gpu_driver, tmp_path, name):
    bad = run_case(gpu_driver, name, tmp_path)
    assert not bad, report(bad)
