"""k_assemble, k_deblock and k_sao_out alone, against an integer model of H.265 8.7.2 / 8.7.3.

The end-to-end tests pin the loop filter only to the oracle, whose loop filter
was written beside the kernels'.  Here hand-built maps, SAO parameters and
samples (tests/loopfilter_vectors.py) go through the three kernels by
themselves (tests/loopfilter/lf_driver.cpp), and the sample arena after
deblocking and the caller's planes after SAO must equal a model written from
the clause text (tests/loopfilter_ref.py) byte for byte, with a sentinel
intact wherever nothing may be written.  The same vectors run through the host
emulation of kernels/loopfilter.hip (here) and through the product library on
the GPU.  The coverage tests hold on the model alone: they keep the vectors
from going soft.
"""
import os
import pathlib
import subprocess
import time

import numpy as np
import pytest

import loopfilter_ref as ref
import loopfilter_vectors as lv
from conftest import make_emu

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
DRIVER_SRC = ROOT / "tests" / "loopfilter" / "lf_driver.cpp"
CASE_NAMES = list(lv.CASES)
THREE = (-1, 0, 1)
FEW_BLOCKS = {"HEIFGPU_DBK_BLOCKS": "1", "HEIFGPU_SAO_BLOCKS": "1"}


def build_gpu_driver(out_dir, lib_dir=ROOT / "heif_amd"):
    """The driver against the built product library (hg::launch_deblock / hg::launch_sao_out:
    the library's own loop-filter object, nothing of the product recompiled)."""
    exe = pathlib.Path(out_dir) / "lf_driver"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wextra", f"-I{CSRC}",
           str(DRIVER_SRC), f"-L{lib_dir}", "-lheifgpu", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_case(exe, name, tmp_path, env=None, timeout=120):
    """The case through the driver: where its two buffers differ from the model."""
    c = lv.case(name)
    src, out = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    src.write_bytes(c.blob)
    t0 = time.perf_counter()
    r = subprocess.run([str(exe), str(src), str(out)], capture_output=True, text=True, timeout=timeout,
                       env=None if env is None else {**os.environ, **env})
    print(f"{name}: driver {time.perf_counter() - t0:.2f} s")
    assert r.returncode == 0, f"driver failed ({r.returncode}): {r.stderr}"
    return c.failures(np.fromfile(out, dtype=np.uint8))


def report(bad):
    return f"{len(bad)} differences from the model, the first of them:\n" + "\n".join(bad[:12])


@pytest.fixture(scope="module")
def emu_driver():
    make_emu("lf-emu")
    return CSRC / "build" / "emu_fast" / "lf_driver"


@pytest.fixture(scope="module")
def gpu_driver(tmp_path_factory):
    return build_gpu_driver(tmp_path_factory.mktemp("lf_driver"))


# ---------------------------------------------------------------- the model itself
def test_model_tables_are_the_specs():
    # Table 8-12
    assert [int(ref.beta_prime(q)) for q in (0, 15, 16, 17, 28, 29, 30, 38, 51)] == [0, 0, 6, 7, 18, 20, 22, 38, 64]
    assert ref.TC_PRIME.tolist()[:18] == [0] * 18
    assert [int(ref.TC_PRIME[q]) for q in (18, 26, 27, 30, 31, 34, 35, 37, 38, 39, 40, 41, 42, 46, 47, 48, 53)] == \
        [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 11, 13, 14, 24]
    assert (np.diff(ref.TC_PRIME) >= 0).all() and (np.diff(ref.beta_prime(np.arange(52))) >= 0).all()
    # Table 8-10 and its ends; Min(qPi, 51) for the other formats
    assert ref.qp_chroma(np.arange(-3, 58), 1).tolist() == list(range(-3, 30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35,
                                                                                   35, 36, 36, 37, 37] + \
        list(range(38, 52))
    for fmt in (2, 3):
        assert ref.qp_chroma(np.arange(-3, 58), fmt).tolist() == list(range(-3, 52)) + [51] * 6
    # 8.7.3.2
    assert ref.band_table(30) == [3, 4] + [0] * 28 + [1, 2]
    assert ref.band_table(0)[:5] == [1, 2, 3, 4, 0]


def _luma_line(p, q, qp=30):
    """one 16x4 picture with the edge at x = 8: p3..p0 | q0..q3 on every line"""
    Y = np.zeros((4, 16), dtype=np.int64)
    Y[:, 4:12] = [p + q] * 4
    qpy = np.full((1, 4), qp, dtype=np.int8)
    flg = np.array([[0, 0, ref.MF_EDGE_V, 0]], dtype=np.uint8)
    return Y, qpy, flg


def test_model_by_hand():
    # normal filter, 8 bit, QpP = QpQ = 30: Q = 30, beta = 2 * 30 - 38 = 22; Q = 32, tC = 3.
    # p = 100 flat, q = 110 flat: d = 0 < 22, but |p0 - q0| = 10 is not below (5 * 3 + 1) >> 1 = 8, so dE = 1;
    # dp = dq = 0 < (22 + 11) >> 3 = 4: dEp = dEq = 1.  delta = (9 * 10 + 8) >> 4 = 6, below 30, clipped to 3:
    # p0 = 103, q0 = 107; delta_p = Clip3(-1, 1, (100 - 100 + 3) >> 1 = 1): p1 = 101;
    # delta_q = Clip3(-1, 1, (110 - 110 - 3) >> 1 = -2): q1 = 109
    Y, qpy, flg = _luma_line([100] * 4, [110] * 4)
    out, ev = ref.luma_vertical(Y, qpy, flg, 8, 0, 0)
    assert out[:, 4:12].tolist() == [[100, 100, 101, 103, 107, 109, 110, 110]] * 4
    assert ev["dE"].tolist() == [[1 * 4 + 2 + 1]]
    # the same at 10 bit on four times the samples: beta = 88, tC = 12, delta = (9 * 40 + 8) >> 4 = 23 clipped to 12;
    # tC >> 1 is 6, not 4 * (3 >> 1): delta_p = (400 - 400 + 12) >> 1 = 6, delta_q = (440 - 440 - 12) >> 1 = -6
    out, _ = ref.luma_vertical(Y * 4, qpy, flg, 10, 0, 0)
    assert out[:, 4:12].tolist() == [[400, 400, 406, 412, 428, 434, 440, 440]] * 4
    # strong filter: q = 104, |p0 - q0| = 4 < 8 and every other term 0: dE = 2, 2 tC = 6 binds nowhere.
    # p0 = (100 + 200 + 200 + 208 + 104 + 4) >> 3 = 102, p1 = (300 + 104 + 2) >> 2 = 101,
    # p2 = (200 + 300 + 100 + 100 + 104 + 4) >> 3 = 101, q0 = (100 + 200 + 208 + 208 + 104 + 4) >> 3 = 103,
    # q1 = (100 + 312 + 2) >> 2 = 103, q2 = (100 + 104 + 104 + 312 + 208 + 4) >> 3 = 104
    Y, qpy, flg = _luma_line([100] * 4, [104] * 4)
    out, ev = ref.luma_vertical(Y, qpy, flg, 8, 0, 0)
    assert out[:, 4:12].tolist() == [[100, 101, 101, 102, 103, 103, 104, 104]] * 4
    assert ev["dE"].tolist() == [[2 * 4 + 2 + 1]]
    # the horizontal edge is the same on the transposed picture, through deblock()
    pl, _ = ref.deblock([Y.T.copy()], qpy.T.copy(), np.array([[0], [0], [ref.MF_EDGE_H], [0]], dtype=np.uint8), 0, 8, 8,
                        0, 0, 0, 0)
    assert pl[0].T[:, 4:12].tolist() == [[100, 101, 101, 102, 103, 103, 104, 104]] * 4
    # no flag, a flag off the 8x8 grid, a flag at x = 0: nothing
    for col in (None, 1, 3, 0):
        f = np.zeros((1, 4), dtype=np.uint8)
        if col is not None:
            f[0, col] = ref.MF_EDGE_V
        assert (ref.luma_vertical(Y, qpy, f, 8, 0, 0)[0] == Y).all()
    # chroma, 4:2:0, 8 bit, QpY 30 on both sides.  Cb, offset 4: qPi = 34, QpC = 33, Q = 35, tC = 4;
    # delta = ((20 << 2) + 60 - 80 + 4) >> 3 = 8, clipped to 4: 64 | 76.  Cr, offset 0: qPi = 30, QpC = 29,
    # Q = 31, tC = 3: 63 | 77.  4:2:2 takes Min(qPi, 51): Cb QpC = 34, Q = 36, tC = 4 still; Cr Q = 32, tC = 3
    C = np.zeros((4, 16), dtype=np.int64)
    C[:, :8], C[:, 8:] = 60, 80
    qpy = np.full((2, 8), 30, dtype=np.int8)
    flg = np.zeros((2, 8), dtype=np.uint8)
    flg[:, 4] = ref.MF_EDGE_V
    for fmt in (1, 2):
        for off, want in ((4, [60, 64, 76, 80]), (0, [60, 63, 77, 80])):
            out, _ = ref.chroma_vertical(C, qpy, flg, *ref.subsampling(fmt), fmt, 8, off, 0)
            assert out[0, 6:10].tolist() == want and (out[:, :6] == 60).all() and (out[:, 10:] == 80).all()
    # the flag of the lower luma block only: in 4:2:0 that block is chroma lines 2 and 3
    flg[0, 4] = 0
    out, _ = ref.chroma_vertical(C, qpy, flg, 1, 1, 1, 8, 4, 0)
    assert out[:, 7].tolist() == [60, 60, 64, 64]
    # SAO.  Band offset, 8 bit (band = sample >> 3), position 30, offsets 5, -6, 7, -8 for bands 30, 31, 0, 1:
    # 250 (band 31) -> 244; 3 (band 0) -> 10; 100 (band 12) stays; 253 with position 31 (+5) clips to 255
    P = np.full((8, 8), 100, dtype=np.int64)
    P[0, 0], P[0, 1], P[7, 7] = 250, 3, 253
    flg = np.zeros((2, 2), dtype=np.uint8)
    prm = {"type": np.array([[[1, 0, 0]]]), "band_eo": np.array([[[30, 0, 0]]]),
           "off": np.array([[[[5, -6, 7, -8]] * 3]])}
    out, _ = ref.sao_plane(P, 0, 0, 0, prm, 4, flg, 8)
    assert (out[0, 0], out[0, 1], out[7, 7], out[3, 3]) == (244, 10, 253 - 6, 100)
    prm["band_eo"][0, 0, 0] = 31
    assert ref.sao_plane(P, 0, 0, 0, prm, 4, flg, 8)[0][7, 7] == 255
    # Edge offset, offsets 11, 12, 13, 14 for edgeIdx 1..4.  Centre (3, 3) = 40 among 50s, with left 30,
    # (2, 2) = 40, (2, 4) = 40, (4, 2) = 30:
    #   class 0: left 30, right 50: signs +1 -1, edgeIdx 2 -> 0: stays 40
    #   class 1: above 50, below 50: -1 -1, edgeIdx 0 -> 1: 40 + 11
    #   class 2: (2, 2) = 40, (4, 4) = 50: 0 -1, edgeIdx 1 -> 2: 40 + 12
    #   class 3: (y 2, x 4) = 40, (y 4, x 2) = 30: 0 +1, edgeIdx 3: 40 + 13
    # (5, 5) = 60 between two 50s in class 0: +1 +1, edgeIdx 4: 60 + 14
    # the corner (0, 0) = 10 has a neighbour outside the picture in every class: stays
    P = np.full((8, 8), 50, dtype=np.int64)
    P[3, 3], P[3, 2], P[2, 2], P[2, 4], P[4, 2], P[5, 5], P[0, 0] = 40, 30, 40, 40, 30, 60, 10
    prm = {"type": np.array([[[2, 0, 0]]]), "band_eo": np.array([[[0, 0, 0]]]),
           "off": np.array([[[[11, 12, 13, 14]] * 3]])}
    for cls, want in enumerate((40, 51, 52, 53)):
        prm["band_eo"][0, 0, 0] = cls
        out, _ = ref.sao_plane(P, 0, 0, 0, prm, 4, flg, 8)
        assert out[3, 3] == want and out[0, 0] == 10, cls
        if cls == 0:
            assert out[5, 5] == 74
    # a no-filter block keeps its samples
    flg[0, 0] = ref.MF_NOFILT
    assert ref.sao_plane(P, 0, 0, 0, prm, 4, flg, 8)[0][3, 3] == 40
    # placement: an odd visible width rounds chroma up; a picture beyond the image writes nothing
    assert ref.visible(21, 9, 100, 100, 0, 0, 1) == [(21, 9), (11, 5), (11, 5)]
    assert ref.visible(21, 9, 30, 12, 20, 8, 2) == [(10, 4), (5, 4), (5, 4)]
    assert ref.visible(21, 9, 30, 12, 30, 0, 1) == [(0, 0)] * 3


# ---------------------------------------------------------------- coverage, from the model alone
def luma_events(bd):
    """What the `decisions` case must show per bit depth and direction: every
    comparison below, at and above its threshold, every clip binding each way
    and not binding.  dE = 2 with dEp = dEq = 0 cannot happen: dE = 2 needs
    2 dpq0 and 2 dpq3 below beta >> 2, so dp + dq < beta >> 2, while dEp = dEq = 0
    needs dp and dq both at least (beta + (beta >> 1)) >> 3, about 3 beta / 8 in sum."""
    names = ("d", "dp", "dq", "Qbeta", "QtC", "delta", "clip_delta", "clip_dp", "clip_dq")
    want = {(n, s) for n in names for s in THREE}
    want |= {(f"dsam{k}{c}", s) for k in (0, 3) for c in "abc" for s in THREE}
    want |= {(f"clip1_{n}", s) for n in ("p0", "q0", "p1", "q1") for s in THREE}
    want |= {(f"strong_{n}", s) for n in ("p0", "p1", "p2", "q0", "q1", "q2") for s in THREE}
    want |= {("dE", c) for c in (0, 4, 5, 6, 7, 9, 10, 11)} | {("qp_odd", 0), ("qp_odd", 1), ("qp_neg", 0)}
    if bd > 8:  # a negative QpY, and the least there is, -QpBdOffsetY
        want |= {("qp_neg", 1), ("qp_neg", 2)}
    return want


def test_coverage_luma_decisions():
    c = lv.case("decisions")
    for bd, b in zip((8, 10, 12), c.batches):
        assert all(p.bd_y == bd for p in b.pics)
        got = c.seen("dbk", "luma", where=lambda b2, p: b2 is b)
        for d in "VH":
            missing = luma_events(bd) - got[d]
            assert not missing, (bd, d, sorted(missing))
        # the strong filter on every segment of every 8-grid line of one picture, side by side, in both
        # directions (the horizontal edges on what the vertical ones left)
        strong = next(p for p in b.pics if p.name.startswith("strong"))
        dE_v, dE_h = (strong.events["dbk", "luma", d]["dE"] >> 2 for d in "VH")
        assert dE_v.size == 7 * 8 and dE_h.size == 3 * 16 and (dE_v == 2).all() and (dE_h == 2).all()
        # corners where a vertical and a horizontal edge both change samples
        for p in b.pics:
            if p.name.startswith(("strong", "both")):
                v, _ = ref.luma_vertical(p.planes[0], p.qpy, p.flg, bd, p.beta_off, p.tc_off)
                changed_v, changed_h = v != p.planes[0], p.deblocked[0] != v
                assert (changed_v & changed_h).any(), p.name


def test_coverage_chroma():
    c = lv.case("chroma")
    want = {(n, s) for n in ("QtC", "clip_delta", "clip1_p0", "clip1_q0") for s in THREE}
    want |= {("qpi", v) for v in [-1, 52] + list(range(30, 44))}
    formats = set()
    for b, p in c.pics():
        formats.add((p.fmt, p.bd_c))
    assert formats >= {(f, bd) for f in (1, 2, 3) for bd in (8, 10)}
    assert any(p.bd_y != p.bd_c for _, p in c.pics())
    for fmt, bd in sorted(formats):
        for d in "VH":
            got = set()
            for kind in ("cb", "cr"):
                got |= c.seen("dbk", kind, where=lambda b, p: (p.fmt, p.bd_c) == (fmt, bd)).get(d, set())
            missing = want - got
            assert not missing, (fmt, bd, d, sorted(missing))
    # the two offsets differ and reach both ends; along an edge a flagged 4x4 block lies beside an
    # unflagged one, so the lines per block (4 >> sy along a vertical edge, 4 >> sx along a horizontal one) show
    assert {(-12, 12), (12, -12)} <= {(p.cb_off, p.cr_off) for _, p in c.pics()}
    for fmt in (1, 2):  # chroma widths and heights that are no multiple of 8, edge counts 1 and 2
        mine = [p for _, p in c.pics() if p.fmt == fmt]
        assert any(p.cw % 8 for p in mine) and (fmt == 2 or any(p.ch % 8 for p in mine))  # 4:2:2: ch is H
        assert {1, 2} <= {(p.cw - 1) >> 3 for p in mine} | {(p.ch - 1) >> 3 for p in mine}
    for fmt in (1, 2, 3):
        for d, bit in (("V", ref.MF_EDGE_V), ("H", ref.MF_EDGE_H)):
            ok = False
            for _, p in c.pics():
                if p.fmt == fmt:
                    f = (p.flg & bit) != 0
                    ok |= bool((f[:-1, 2::2] != f[1:, 2::2]).any() if d == "V" else (f[2::2, :-1] != f[2::2, 1:]).any())
            assert ok, (fmt, d)


def test_coverage_flags():
    c = lv.case("flags")
    for b in c.batches:
        for kind in ("luma",) + (("cb", "cr") if b.fmt else ()):
            got = c.seen("dbk", kind, where=lambda b2, p: b2 is b)
            for d in "VH":
                assert {("nofilt", k) for k in range(4)} <= got[d], (b.name, kind, d)
            types = {code for n, code in c.seen("sao", kind, where=lambda b2, p: b2 is b)[None] if n == "type"}
            assert {1, 2, 3} <= types, (b.name, kind)  # 3: a sample SAO leaves alone for MF_NOFILT
        launched = b.pics[b.pic0:b.pic0 + b.n_launch]
        # samples SAO must leave alone for MF_NOFILT reach it through the quad load and one by one, per component
        for cidx in range(3 if b.fmt else 1):
            how = set()
            for p in launched:
                if not p.flags & lv.PD_CHILD:
                    kept = p.events["sao", ("luma", "cb", "cr")[cidx]]["type"] == 3
                    how |= set(np.unique(sao_paths(b, p)[2][cidx][kept]).tolist())
            assert {1, 2} <= how, (b.name, cidx, how)
        assert any(p.dbk_disabled for p in launched) and any(p.flags & lv.PD_CHILD for p in launched)
        for p in launched:  # flags off the 8x8 grid and along the left and top
            assert (p.flg[:, 1::2] & ref.MF_EDGE_V).all() and (p.flg[:, 0] & ref.MF_EDGE_V).all()
            assert (p.flg[1::2, :] & ref.MF_EDGE_H).all() and (p.flg[0, :] & ref.MF_EDGE_H).all()
        child = next(p for p in launched if p.flags & lv.PD_CHILD)
        planes, _ = ref.deblock(child.planes, child.qpy, child.flg, child.fmt, child.bd_y, child.bd_c, 0, 0, 0, 0)
        assert any((a != b2).any() for a, b2 in zip(planes, child.planes))  # it would filter if it ran


def sao_events():
    """Per chroma format, bit depth and component: every class with every pair of signs, every class at each
    picture border and corner its neighbours leave (codes: 1 top, 2 bottom, 4 left, 8 right), every offset of
    every band position used, with and without the wrap past band 31, and the final clip each way."""
    want = {("eo", k) for k in range(36)} | {("clip", s) for s in THREE} | {("band_wrap", 0), ("band_wrap", 1)}
    want |= {("band", pos * 4 + k) for pos in lv.BAND_POSITIONS for k in range(4)} | {("band_miss", 1)}
    around = (1, 2, 4, 8, 5, 6, 9, 10)
    borders = {0: (4, 8, 5, 6, 9, 10), 1: (1, 2, 5, 6, 9, 10), 2: around, 3: around}
    want |= {("eo_border", cls * 16 + at) for cls, ats in borders.items() for at in ats}
    return want


def test_coverage_sao():
    c = lv.case("sao")
    combos = {(p.fmt, p.bd_y) for _, p in c.pics()}
    assert combos == {(f, bd) for f in range(4) for bd in (8, 10, 12)}
    assert {p.log2_ctb for _, p in c.pics()} == {4, 5, 6}
    for fmt, bd in sorted(combos):
        sel = lambda b, p: (p.fmt, p.bd_y) == (fmt, bd)
        for kind in ("luma",) + (("cb", "cr") if fmt else ()):
            missing = sao_events() - c.seen("sao", kind, where=sel)[None]
            assert not missing, (fmt, bd, kind, sorted(missing))
        mine = [p for _, p in c.pics() if sel(None, p)]
        assert any(p.W % (1 << p.log2_ctb) and p.H % (1 << p.log2_ctb) for p in mine)
        for p in mine:  # a component whose slice flag is off carries type 0
            assert p.sao_luma or not p.sao["type"][:, :, 0].any()
            assert p.sao_chroma or not p.sao["type"][:, :, 1:].any()
        # neighbouring CTBs with other parameters, and offsets at the ends of their range
        assert any((p.sao[:, :-1] != p.sao[:, 1:]).any() for p in mine if p.wctb > 1)
        for cidx in range(3 if fmt else 1):
            offs = np.concatenate([p.sao["off"][:, :, cidx].ravel() for p in mine if p.bd(cidx) == bd])
            assert offs.max() == lv.sao_max(bd) and offs.min() == -lv.sao_max(bd)
    for fmt in (1, 2, 3):  # luma and chroma of different depths with SAO on, band and edge offset on each
        for depths in ((10, 12), (12, 10)):
            mixed = [p for _, p in c.pics() if (p.fmt, p.bd_y, p.bd_c) == (fmt,) + depths]
            assert mixed and all(p.sao_luma and p.sao_chroma for p in mixed)
            for cidx in range(3):
                assert {1, 2} <= {int(t) for p in mixed for t in np.unique(p.sao["type"][:, :, cidx])}, (fmt, depths)
    for b in c.batches:  # luma only, chroma only, neither: per chroma format and sample size
        flags = {(p.sao_luma, p.sao_chroma) for p in b.pics}
        assert flags >= ({(1, 0), (0, 0)} if b.fmt == 0 else {(1, 1), (1, 0), (0, 1), (0, 0)}), (b.name, flags)
    assert lv.sao_max(12) == 31 << 2 and lv.sao_max(10) == 31 and lv.sao_max(8) == 7


def sao_paths(b, p):
    """{(cidx, row): set of "quad" / "sample"} and the store kinds, by the rule k_sao_out documents: four
    samples go through one aligned load when all four are visible (n == 4), SAO is on for the slice, the
    first one's picture column xs0 is a multiple of 4 and its address is aligned to four samples; the
    store is one word when n == 4 and the destination is aligned to four samples."""
    rows, stores, masks = {}, set(), []
    im = b.images[p.image]
    base = p.recon_off
    for cidx, (vw, vh) in enumerate(ref.visible(p.out_w, p.out_h, im.width, im.height, p.out_x, p.out_y, p.fmt)):
        kx, ky = (p.sx, p.sy) if cidx else (0, 0)
        h, w = p.shape(cidx)
        masks.append(np.zeros((h, w), dtype=np.int8))  # per picture sample: 1 through a quad, 2 by itself
        for y in range(vh):
            ys = y + (p.conf_t >> ky)
            for x0 in range(0, vw, 4):
                n, xs0 = min(4, vw - x0), x0 + (p.conf_l >> kx)
                addr = base + (ys * w + xs0) * b.sz
                quad = n == 4 and bool(p.sao_luma or p.sao_chroma) and xs0 % 4 == 0 and addr % (4 * b.sz) == 0
                rows.setdefault((cidx, y), set()).add("quad" if quad else "sample")
                masks[cidx][ys, xs0:xs0 + n] = 1 if quad else 2
                dst = b.plane_off[p.image][cidx] + ((p.out_y >> ky) + y) * b.pitch[p.image][cidx] \
                    + ((p.out_x >> kx) + x0) * b.sz
                stores.add("wide" if n == 4 and dst % (4 * b.sz) == 0 else "narrow")
        base += h * w * b.sz
    return rows, stores, masks


# (`decisions` and `chroma` run with SAO off: every load there is the plain copy)
@pytest.mark.parametrize("name", ["flags", "sao", "placement", "dispatch", "assembly"])
def test_coverage_sao_paths(name):
    c = lv.case(name)
    for sz in (1, 2):
        kinds, stores, mixed = set(), set(), False
        for b, p in c.pics():
            if b.sz != sz or p.flags & lv.PD_CHILD:
                continue
            rows, st, _ = sao_paths(b, p)
            stores |= st
            for r in rows.values():
                kinds |= r
                mixed |= len(r) == 2
        assert kinds == {"quad", "sample"} and mixed and stores == {"wide", "narrow"}, (name, sz, kinds, stores, mixed)


def test_coverage_placement():
    c = lv.case("placement")
    for b in c.batches:
        ux, uy = lv.smallest_conf(b.fmt)
        launched = b.pics[b.pic0:b.pic0 + b.n_launch]
        assert {(0, 0), (ux, uy), (4 + ux, 4 + uy)} <= {(p.conf_l, p.conf_t) for p in launched}
        for conf in ((0, 0), (ux, uy), (4 + ux, 4 + uy)):
            assert {p.out_w % 4 for p in launched if (p.conf_l, p.conf_t) == conf} == {0, 1, 2, 3}
        assert any(p.out_w % 2 and p.out_h % 2 for p in launched)
        assert {1, 3} <= {im.skew for im in b.images} and any((im.width + im.pad) % 4 for im in b.images)
        assert any(p.out_x % 4 for p in launched) and any(p.out_y for p in launched)
        shared = [p for p in launched if sum(q.image == p.image for q in launched) > 1]
        vis = [ref.visible(p.out_w, p.out_h, b.images[p.image].width, b.images[p.image].height, p.out_x, p.out_y,
                           p.fmt)[0] for p in shared]
        assert len(shared) == 4 and sum(v == (0, 0) for v in vis) == 2
        assert any((0, 0) != v != (p.out_w, p.out_h) and v[0] < p.out_w and v[1] < p.out_h for v, p in zip(vis, shared))
        assert any(not (p.sao_luma or p.sao_chroma) for p in launched)


def test_coverage_dispatch_and_assembly():
    c = lv.case("dispatch")
    for b in c.batches:
        assert b.pic0 == 2
        launched = b.pics[b.pic0:]
        assert len({(p.W, p.H) for p in launched}) == len(launched)
        assert {(p.W - 1) >> 3 for p in launched} >= {3, 5, 7, 33} and 34 in {p.W >> 2 for p in launched}
        for p in launched:
            ne, ns = (p.W - 1) >> 3, p.H >> 2
            assert (ne * ns) % 256 and (((p.out_w + 3) >> 2) * p.out_h) % 256
        before, _ = ref.deblock(b.pics[0].planes, b.pics[0].qpy, b.pics[0].flg, b.fmt, b.pics[0].bd_y, b.pics[0].bd_c,
                                2, -3, 0, 0)
        assert (before[0] != b.pics[0].planes[0]).any()  # the pictures before pic0 would be filtered
    big = max(c.batches[0].pics, key=lambda p: p.W * p.H)
    assert ((big.out_w + 3) >> 2) * big.out_h > 100000
    a = lv.case("assembly")
    for b in a.batches:
        asm = b.pics[-1]
        kids = [b.pics[i] for i in asm.children]
        assert asm.flags & lv.PD_ASSEMBLY and len(kids) == 3 and len({(k.W, k.H) for k in kids}) == 3
        assert all(k.flags & lv.PD_CHILD and k.org_x % 16 == 0 and k.org_y % 16 == 0 for k in kids)
        for k in kids:  # a child with SAO on obeys "a component whose flag is off carries type 0"
            if k.sao_luma or k.sao_chroma:
                assert k.sao_luma and (k.sao_chroma or not k.sao["type"][:, :, 1:].any())
        off = [k for k in kids if not (k.sao_luma or k.sao_chroma)]
        assert len(off) == 1 and off[0].sao["type"].any()  # garbage that must arrive as zeros
        oy, ox = off[0].org_y >> 4, off[0].org_x >> 4
        # what the case file gives the assembly itself is none of what k_assemble must leave there:
        # no QpY, no flag byte row, no CTB's parameters (the SAO-off child's region included)
        qpy0, flg0, sao0 = asm.given
        assert not asm.sao["type"][oy:oy + off[0].hctb, ox:ox + off[0].wctb].any()
        assert sao0["type"][oy:oy + off[0].hctb, ox:ox + off[0].wctb].any(axis=2).all()
        assert (sao0 != asm.sao).all() and (qpy0 != asm.qpy).any(axis=1).all() and (flg0 != asm.flg).any(axis=1).all()
        given, _ = ref.deblock(asm.planes, qpy0, flg0, asm.fmt, asm.bd_y, asm.bd_c, asm.cb_off, asm.cr_off, 0, 0)
        assert any((g != d).any() for g, d in zip(given, asm.deblocked))  # with the maps it was given: other samples
        # deblocking changes samples on both sides of a seam between two children
        changed = asm.deblocked[0] != asm.planes[0]
        assert changed[:, 29:32].any() and changed[:, 32:35].any() and changed[29:32, 32:].any()


def test_coverage_sentinels():
    for name in CASE_NAMES:
        for b in lv.case(name).batches:
            for buf in (b.expected_recon, b.expected_out):
                assert (buf == lv.SENTINEL).any() and (buf != lv.SENTINEL).any(), (name, b.name)


# ---------------------------------------------------------------- layout
def test_layout_mirrors_match_the_structs(emu_driver):
    r = subprocess.run([str(emu_driver), "--layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    theirs = {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}
    assert theirs == lv.layout_of_mirrors()


# ---------------------------------------------------------------- the two legs
@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulated_loopfilter_equals_model(emu_driver, tmp_path, name):
    bad = run_case(emu_driver, name, tmp_path)
    assert not bad, report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_loopfilter_equals_model(gpu_driver, tmp_path, name):
    bad = run_case(gpu_driver, name, tmp_path)
    assert not bad, report(bad)
    if name == "dispatch":  # once more with one workgroup per picture (read once per process)
        bad = run_case(gpu_driver, name, tmp_path, env=FEW_BLOCKS)
        assert not bad, "one workgroup per picture: " + report(bad)
