"""k_transform alone, against an integer model of H.265 8.6.2-8.6.4.

The end-to-end tests see the inverse transform only through clip(pred +
residual), deblocking and SAO; here hand-built TU records and coefficient
words (tests/xform_vectors.py) go through the kernel by itself
(tests/xform/xform_driver.cpp) and the residual planes must equal the model
exactly, with a sentinel surviving wherever no coded TB lies.  The same
vectors run twice: through the host emulation of kernels/transform.hip (the
dot-product stages and pass A, here) and through the product library on the
GPU (the int8 MFMA stages of 16x16 / 32x32 TBs and the ballot loops, which
exist only there).  The coverage tests keep the vectors from going soft: they
hold on the model alone.
"""
import pathlib
import subprocess

import numpy as np
import pytest

import xform_vectors as xv
from conftest import make_emu

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
DRIVER_SRC = ROOT / "tests" / "xform" / "xform_driver.cpp"
CASE_NAMES = list(xv.CASES)


def build_gpu_driver(out_dir, lib_dir=ROOT / "heif_amd"):
    """The driver against the built product library (hg::launch_transform: the
    library's own transform object, nothing of the product recompiled)."""
    exe = pathlib.Path(out_dir) / "xform_driver"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wextra", f"-I{CSRC}",
           str(DRIVER_SRC), f"-L{lib_dir}", "-lheifgpu", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_case(exe, name, tmp_path, timeout=120):
    """The case through the driver: the failures of the residual arena it leaves."""
    c = xv.case(name)
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
    return build_gpu_driver(tmp_path_factory.mktemp("xform_driver"))


# ---------------------------------------------------------------- the model itself
def test_model_matrices_are_the_specs():
    T = xv.TRANS_MATRIX
    assert T[0].tolist() == [64] * 32
    assert T[1, :16].tolist() == [90, 90, 88, 85, 82, 78, 73, 67, 61, 54, 46, 38, 31, 22, 13, 4]
    assert T[1, 16:].tolist() == [-v for v in T[1, :16].tolist()[::-1]]
    assert T[31].tolist() == [4, -13, 22, -31, 38, -46, 54, -61, 67, -73, 78, -82, 85, -88, 90, -90,
                              90, -90, 88, -85, 82, -78, 73, -67, 61, -54, 46, -38, 31, -22, 13, -4]
    assert T[:, 0].tolist() == list(xv._COL0)
    assert xv.matrix_of(16)[1].tolist() == [90, 87, 80, 70, 57, 43, 25, 9, -9, -25, -43, -57, -70, -80, -87, -90]
    assert xv.matrix_of(8).tolist() == [[64, 64, 64, 64, 64, 64, 64, 64], [89, 75, 50, 18, -18, -50, -75, -89],
                                        [83, 36, -36, -83, -83, -36, 36, 83], [75, -18, -89, -50, 50, 89, 18, -75],
                                        [64, -64, -64, 64, 64, -64, -64, 64], [50, -89, 18, 75, -75, -18, 89, -50],
                                        [36, -83, 83, -36, -36, 83, -83, 36], [18, -50, 75, -89, 89, -75, 50, -18]]
    assert xv.matrix_of(4).tolist() == [[64, 64, 64, 64], [83, 36, -36, -83], [64, -64, -64, 64], [36, -83, 83, -36]]
    for n in (4, 8, 16, 32):  # rows orthogonal, of squared norm 4096 n, to within 1 % (integer entries):
        M = xv.matrix_of(n)   # one wrong sign or a swapped row leaves products of the order of the norm
        gram = M @ M.T
        assert np.abs(gram - np.diag(np.diag(gram))).max() <= 4096 * n // 100
        assert np.abs(np.diag(gram) - 4096 * n).max() <= 4096 * n // 100


def test_model_by_hand():
    # 4x4, 8 bit, qp 4 (levelScale 64), m 16, level 10 at DC: d = (10 * 16 * 64 + 16) >> 5 = 320,
    # first stage (64 * 320 + 64) >> 7 = 160, second (64 * 160 + 2048) >> 12 = 3 everywhere
    lv = np.zeros((4, 4), dtype=np.int64)
    lv[0, 0] = 10
    res, mid = xv.reference(lv, 4, 8, 4)
    assert mid["d"][0, 0] == 320 and res.tolist() == [[3] * 4] * 4
    # the same level at (y, x) = (0, 1) under the DST: d = 320, e[i][1] = 29 * 320 .. 84 * 320 down column 1,
    # g = (e + 64) >> 7, r[y][i] = DST[1][i] * g[y][1]
    lv[:] = 0
    lv[0, 1] = 10
    res, _ = xv.reference(lv, 4, 8, 4, dst=True)
    g = [(k * 320 + 64) >> 7 for k in (29, 55, 74, 84)]
    assert res.tolist() == [[(c * gy + 2048) >> 12 for c in (74, 74, 0, -74)] for gy in g]
    # transform skip at 8x8 ignores the list (m = 16), at 4x4 it does not
    # (level 1, qp 4: d = 16 at 8x8 and 32 or, with m = 32, 64 at 4x4; r = d << tsShift, then >> 12)
    m, one8, one4 = np.full((8, 8), 32), np.ones((8, 8), dtype=np.int64), np.ones((4, 4), dtype=np.int64)
    assert xv.reference(one8, 8, 8, 4, m, ts=True)[0].tolist() == [[(16 * 256 + 2048) >> 12] * 8] * 8
    assert xv.reference(one8, 8, 8, 4, None, ts=True)[0].tolist() == [[1] * 8] * 8
    assert xv.reference(one4, 4, 8, 4, m[:4, :4], ts=True)[0].tolist() == [[(64 * 128 + 2048) >> 12] * 4] * 4
    assert xv.reference(one4, 4, 8, 4, None, ts=True)[0].tolist() == [[(32 * 128 + 2048) >> 12] * 4] * 4


def test_scans_are_the_specs():
    assert xv.scan_order(4, 0) == [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0), (0, 3), (1, 2), (2, 1), (3, 0),
                                   (1, 3), (2, 2), (3, 1), (2, 3), (3, 2), (3, 3)]
    assert xv.scan_order(2, 0) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert xv.scan_order(4, 1)[:5] == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1)]
    assert xv.scan_order(4, 2)[:5] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)]
    for blk in (2, 4, 8):
        for sc in range(3):
            assert sorted(xv.scan_order(blk, sc)) == sorted((x, y) for x in range(blk) for y in range(blk))


# ---------------------------------------------------------------- coverage, from the model alone
def test_coverage_boundary_values():
    """For 16x16 and 32x32 the scaled d takes every value at which the int8
    halves of the MFMA operands change."""
    c = xv.case("saturation")
    for n in (16, 32):
        assert c.d_seen[n] == set(xv.BOUNDARY_D), (n, sorted(set(xv.BOUNDARY_D) - c.d_seen[n]))


def test_coverage_first_stage_clips():
    c = xv.case("saturation")
    for n in (8, 16, 32):
        assert n in c.clip_hi and n in c.clip_lo, n


def test_coverage_ballot_windows():
    """The dispatch case's long row: more records than one ballot window of
    every wave, and in each window a count of coded 4x4 TBs that leaves the
    last round of four partly empty; a 16x16 TB follows a 32x32 one on wave 0."""
    c = xv.case("dispatch")
    long_rows = [recs for _, _, recs in c.rows_tus if len(recs) > 256]
    assert len(long_rows) == 1
    recs = long_rows[0]
    counts = xv.ballot_counts(recs)
    for wave in range(4):
        for window in range(2):
            assert counts.get((wave, window), 0) % 4 != 0, (wave, window, counts)
    big = [(t, int(r["log2"])) for t, r in enumerate(recs) if t % 4 == 0 and (r["flags"] & xv.TU_CBF) and r["log2"] > 2]
    assert big[:2] == [(0, 5), (4, 4)]
    assert any(not (r["flags"] & xv.TU_CBF) for r in recs)
    # pictures that must stay untouched carry records that would write if they ran
    assert c.pic0 == 1 and any(p.flags & xv.PD_ASSEMBLY for p in c.pics)
    rows = {s.rows for s in (c.seqs[p.seq] for p in c.pics[c.pic0:])}
    assert len(rows) > 1  # a picture with fewer rows than the launch's grid


def test_coverage_records():
    c = xv.case("records")
    recs = np.concatenate([r for _, _, r in c.rows_tus])
    big = recs[recs["log2"] == 5]
    assert (big["ncoef"] == 4).any() and (big["ncoef"] == 4 * 64).any()
    for name in CASE_NAMES:
        got = xv.case(name).expected
        assert (got == xv.SENTINEL).any() and (got != xv.SENTINEL).any()


# ---------------------------------------------------------------- layout
def test_layout_mirrors_match_the_structs(emu_driver):
    r = subprocess.run([str(emu_driver), "--layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    theirs = {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}
    assert theirs == xv.layout_of_mirrors()


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
