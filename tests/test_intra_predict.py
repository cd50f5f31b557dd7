"""k_intra alone, against a model of H.265 8.4.4.2 and 8.6.7 written from the clause text.

The end-to-end tests pin intra prediction only to the oracle, whose
intra_predict shares the kernel's reference-array layout, expression order and
availability derivation, and the device-only parts of kernels/intra.hip (the
ballot substitution of one, two and three chunks, group_sum, the
one-sample-per-lane path, all of predict_pair) see only random content there.
Here hand-built TU records and residual planes (tests/intra_vectors.py) go
through the kernel by itself (tests/intra/intra_driver.cpp) and the sample
arena must equal the model (tests/intra_ref.py) sample for sample, with a
sentinel intact wherever no record opens a CTU.  The same vectors run through
the host emulation (here) and through the product library on the GPU, under
HEIFGPU_INTRA_SPLIT=0 and 1 and, for two cases, one wave per picture.  The
coverage tests hold on the model alone: they keep the vectors from going soft.

heifgpu's own prepare path rejects a stream whose luma and chroma depths
differ (host/heic_image.cpp: "luma/chroma bit depth differ"); the mixed-depth
pictures of the `edges` case (luma 10 / chroma 12 and the reverse) reach the
kernel because the driver fills BatchArgs itself.

GPU leg on an MI355X: 7 tests with 16 driver runs of 0.18-0.39 s each, 8.3 s
in the tests (availability, three runs, 2.9 s), 9.6 s wall with the driver's build.
"""
import os
import pathlib
import subprocess
import time

import numpy as np
import pytest

import intra_ref as ref
import intra_vectors as iv
from conftest import make_emu

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
DRIVER_SRC = ROOT / "tests" / "intra" / "intra_driver.cpp"
CASE_NAMES = list(iv.CASES)
ONE_WAVE = ("modes", "availability")
CORE = {("all", "all", "all", "all"), ("all", "all", "none", "none"), ("all", "none", "all", "all"),
        ("all", "none", "all", "none"), ("all", "none", "none", "none"), ("none", "none", "all", "all"),
        ("none", "none", "none", "none")}


def knob_settings(name):
    out = [{"HEIFGPU_INTRA_SPLIT": "0"}]
    if iv.case(name).has_chroma:
        out.append({"HEIFGPU_INTRA_SPLIT": "1"})
    if name in ONE_WAVE:
        out.append({"HEIFGPU_INTRA_SPLIT": "0", "HEIFGPU_INTRA_WAVES": "1"})
    return out


def build_gpu_driver(out_dir, lib_dir=ROOT / "heif_amd"):
    """The driver against the built product library (hg::launch_intra: the library's own
    intra object, nothing of the product recompiled)."""
    exe = pathlib.Path(out_dir) / "intra_driver"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wextra", f"-I{CSRC}",
           str(DRIVER_SRC), f"-L{lib_dir}", "-lheifgpu", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


_stopped = {}  # driver -> its run that exited non-zero: the module starts no further run of it


def run_case(exe, name, tmp_path, env, timeout=120):
    """The case through the driver (one process: the knobs are read once): where the
    sample arena and the status words differ from the model."""
    if str(exe) in _stopped:
        pytest.fail(f"not run: an earlier driver run failed ({_stopped[str(exe)]})")
    c = iv.case(name)
    src, out = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    src.write_bytes(c.blob)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([str(exe), str(src), str(out)], capture_output=True, text=True, timeout=timeout,
                           env={**os.environ, **env})
    except subprocess.TimeoutExpired:
        _stopped[str(exe)] = f"{name} {env}: timeout"
        raise
    print(f"{name} {env}: driver {time.perf_counter() - t0:.2f} s")
    if r.returncode != 0:
        _stopped[str(exe)] = f"{name} {env}: exit {r.returncode}"
    assert r.returncode == 0, f"driver failed ({r.returncode}): {r.stderr}"
    return c.failures(np.fromfile(out, dtype=np.uint8))


def report(bad):
    return f"{len(bad)} differences from the model, the first of them:\n" + "\n".join(bad[:12])


@pytest.fixture(scope="module")
def emu_driver():
    make_emu("intra-emu")
    return CSRC / "build" / "emu_fast" / "intra_driver"


@pytest.fixture(scope="module")
def gpu_driver(tmp_path_factory):
    return build_gpu_driver(tmp_path_factory.mktemp("intra_driver"))


def tbs_of(name, pic_prefix=""):
    for p in iv.case(name).pics:
        if p.live and p.name.startswith(pic_prefix):
            for t, i in zip(p.tbs, p.infos):
                yield p, t, i


# ---------------------------------------------------------------- the model itself
def test_model_tables_are_the_specs():
    # Table 8-5 and Table 8-6, written out
    assert [ref.INTRA_PRED_ANGLE[m] for m in range(2, 35)] == [
        32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32,
        -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32]
    assert [ref.INV_ANGLE[m] for m in range(11, 26)] == [
        -4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096]
    assert sorted(ref.INV_ANGLE) == [m for m in range(2, 35) if ref.INTRA_PRED_ANGLE[m] < 0]
    assert ref.DIST_THRES == {8: 7, 16: 1, 32: 0}
    # 6.5.2: a 16 CTB of 4x4 minimum TBs in z-order, the second CTB after the first
    zs = ref.min_tb_addr_zs(ref.Geom(32, 16, 1, 8, 8, 4, 2))
    assert zs[:4, :4].T.tolist() == [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]]
    assert zs[4, 0] == 16 and zs[7, 3] == 31


def _one_tb(W, H, tb, plane, bd=8, res=None, cf=0, **kw):
    g = ref.Geom(W, H, cf, bd, bd, 4, 2, **kw)
    zs = ref.min_tb_addr_zs(g)
    r = np.zeros((H, W), dtype=np.int64) if res is None else res
    return ref.predict_tb(g, tb, np.array(plane, dtype=np.int64), r, ref.avail_by_zscan(g, zs, tb))


def test_model_by_hand():
    # 4x4 DC at the picture origin, 8 bit: nothing available, every neighbour 128; dcVal = (8 * 128 + 4) >> 3
    # = 128, and the edge filter leaves 128: (128 + 2 * 128 + 128 + 2) >> 2 and (128 + 3 * 128 + 2) >> 2
    rec, info = _one_tb(16, 16, ref.TB(0, 0, 0, 2, 1), np.zeros((16, 16)))
    assert rec.tolist() == [[128] * 4] * 4 and not info.avail.any()
    # 4x4 mode 26 at (4, 4): top row 200 201 202 203, corner 10, left column 0, 100, 250, 20 downwards.
    # Column 0 is Clip1(200 + ((left[y] - 10) >> 1)) = Clip1(200 + (-5, 45, 120, 5)) = 195, 245, 255 (clipped
    # from 320), 205; the other columns copy the top row (intraPredAngle 0: iIdx 0, iFact 0)
    pl = np.zeros((16, 16), dtype=np.int64)
    pl[3, 3], pl[3, 4:8], pl[4:8, 3] = 10, [200, 201, 202, 203], [0, 100, 250, 20]
    pl[3, 8:12], pl[8:12, 3] = 77, 66
    rec, info = _one_tb(16, 16, ref.TB(0, 4, 4, 2, 26), pl)
    assert rec.tolist() == [[195, 201, 202, 203], [245, 201, 202, 203], [255, 201, 202, 203], [205, 201, 202, 203]]
    assert {"edge_hi", "edge_mid"} <= info.clips
    # the same as a chroma TB: no boundary filter, column 0 is 200
    g = ref.Geom(32, 32, 1, 8, 8, 4, 2)
    tb = ref.TB(1, 4, 4, 2, 26)
    rec, _ = ref.predict_tb(g, tb, pl, pl * 0, ref.avail_by_zscan(g, ref.min_tb_addr_zs(g), tb))
    assert rec.tolist() == [[200, 201, 202, 203]] * 4
    # 4x4 mode 18 (intraPredAngle -32, invAngle -256) at (4, 4): nTbS * angle >> 5 = -4 < -1, so
    # ref[-1..-4] = p[-1][-1 + ((x * -256 + 128) >> 8)] = p[-1][0..3], the left column downwards;
    # iIdx = -(y + 1), iFact 0: pred[y][x] = ref[x - y]: the diagonal from the top row, the corner, the left column
    pl = np.zeros((16, 16), dtype=np.int64)
    pl[3, 3], pl[3, 4:12], pl[4:12, 3] = 50, [1, 2, 3, 4, 5, 6, 7, 8], [11, 12, 13, 14, 15, 16, 17, 18]
    rec, info = _one_tb(16, 16, ref.TB(0, 4, 4, 2, 18), pl)
    assert rec.tolist() == [[50, 1, 2, 3], [11, 50, 1, 2], [12, 11, 50, 1], [13, 12, 11, 50]]
    assert info.min_ref == -3 and info.ifact_zero and not info.ifact_nonzero
    # 8x8 planar at (16, 16) of a 48 x 48 picture of 16 CTBs (all 4n + 1 neighbours decoded) holding the
    # ramp 100 + 2 x + 3 y in coordinates relative to the TB: p[-1][y] = 98 + 3 y, p[x][-1] = 97 + 2 x,
    # p[8][-1] = 113, p[-1][8] = 122.  Planar at 8x8 filters its neighbours; [1 2 1] leaves a ramp's inner
    # samples as they are ((4 v + 2) >> 2 = v), the two ends are copied, and the corner is not used.
    # pred = ((7 - x) p[-1][y] + (x + 1) 113 + (7 - y) p[x][-1] + (y + 1) 122 + 8) >> 4
    yy, xx = np.mgrid[0:48, 0:48]
    pl = 100 + 2 * (xx - 16) + 3 * (yy - 16)
    rec, info = _one_tb(48, 48, ref.TB(0, 16, 16, 3, 0), pl)
    assert info.avail.all()
    want = [[((7 - x) * (98 + 3 * y) + (x + 1) * 113 + (7 - y) * (97 + 2 * x) + (y + 1) * 122 + 8) >> 4
             for x in range(8)] for y in range(8)]
    assert want[0][:3] == [(7 * 98 + 113 + 7 * 97 + 122 + 8) >> 4, (6 * 98 + 226 + 7 * 99 + 122 + 8) >> 4, 104]
    assert info.filt == 1 and rec.tolist() == want
    # 8.6.7: Clip1 both ways, a PCM TB is its residual, a TB without cbf is its prediction
    res = np.full((16, 16), 300, dtype=np.int64)
    pl = np.zeros((16, 16), dtype=np.int64)
    assert _one_tb(16, 16, ref.TB(0, 0, 0, 2, 1, cbf=True), pl[:16, :16], res=res)[0].tolist() == [[255] * 4] * 4
    assert _one_tb(16, 16, ref.TB(0, 0, 0, 2, 1, cbf=True), pl[:16, :16], res=-res)[0].tolist() == [[0] * 4] * 4
    assert _one_tb(16, 16, ref.TB(0, 0, 0, 2, 1, cbf=True, pcm=True), pl[:16, :16], res=res // 3)[0].tolist() == \
        [[100] * 4] * 4
    assert _one_tb(16, 16, ref.TB(0, 0, 0, 2, 1, cbf=False), pl[:16, :16], res=res)[0].tolist() == [[128] * 4] * 4


def test_model_availability_functions_agree():
    """6.4.1 over MinTbAddrZs against "already reconstructed": in one slice and one
    tile they must agree on every neighbour of every TB of every vector."""
    for name in CASE_NAMES:
        for p in iv.case(name).pics:
            assert p.agree, p.name


# ---------------------------------------------------------------- coverage, from the model alone
def _sizes(cf):
    return {0: (4, 8, 16, 32), 1: (4, 8, 16) if cf in (1, 2) else (4, 8, 16, 32)}


def test_coverage_modes():
    for cf, prefix in ((1, "modes/420"), (2, "modes/422"), (3, "modes/444")):
        seen, facts, minref = set(), {}, {}
        for p, t, i in tbs_of("modes", prefix):
            if not t.tag:
                continue
            n, cls = 1 << t.log2, min(t.cidx, 1)
            assert iv.pattern(i, n) == ("all",) * 4, t.tag
            pl = p.planes[t.cidx]
            vals = [int(pl[y, x]) for x, y in iv.neighbour_positions(p, t)]
            assert len(vals) == 4 * n + 1 and len(set(vals)) == len(vals), t.tag  # pairwise distinct
            seen.add((cls, n, t.mode))
            if t.mode >= 2:
                f = facts.setdefault((cls, n), set())
                f |= {z for z, on in ((0, i.ifact_zero), (1, i.ifact_nonzero)) if on}
            if 11 <= t.mode <= 25:
                # the lowest index the text lets a TB read: x = 0 of the last row, 1 + ((nTbS * angle) >> 5)
                assert i.min_ref == 1 + ((n * ref.INTRA_PRED_ANGLE[t.mode]) >> 5), t.tag
                minref.setdefault((cls, n), set()).add(t.mode)
        want = {(cls, n, m) for cls, ns in _sizes(cf).items() for n in ns for m in range(35)}
        assert seen == want, sorted(want - seen)[:10]
        assert all(f == {0, 1} for f in facts.values()) and len(facts) == len({(c, n) for c, n, _ in want})
        assert all(v == set(range(11, 26)) for v in minref.values())


def test_coverage_filter_flag_boundaries():
    """modes: which TBs 8.4.4.2.3 filters, per size, on both sides of every threshold"""
    filt = {}
    for p, t, i in tbs_of("modes"):
        if t.tag:
            filt.setdefault((p.g.chroma_format, min(t.cidx, 1), 1 << t.log2), {})[t.mode] = i.filt
    for cf in (1, 2, 3):
        assert not any(filt[(cf, 0, 4)].values())
        assert {m for m, f in filt[(cf, 0, 8)].items() if f} == {0, 2, 18, 34}  # and 3, 17, 19, 33 not
        assert {m for m, f in filt[(cf, 0, 16)].items() if f} == set(range(35)) - {1, 9, 10, 11, 25, 26, 27}
        assert {m for m, f in filt[(cf, 0, 32)].items() if f} == set(range(35)) - {1, 10, 26}
        for n in _sizes(cf)[1]:
            got = {m for m, f in filt[(cf, 1, n)].items() if f}
            assert got == ({m for m, f in filt[(cf, 0, n)].items() if f} if cf == 3 else set()), (cf, n)
    assert all(f in (0, 1) for d in filt.values() for f in d.values())  # (strong smoothing is off there)


def test_coverage_strong_smoothing():
    seen = set()
    for p, t, i in tbs_of("filter", "filter/bd"):
        if not t.tag or t.cidx:
            continue
        top, left, thr = i.strong_terms
        assert thr == 1 << (p.g.bd_y - 5)
        want = f"top{top}_left{left}"
        assert want in p.name, (p.name, i.strong_terms)  # the planted expressions are what the model computed
        assert i.filt == (2 if p.g.strong and top < thr and left < thr else 1)
        seen.add((p.g.bd_y, top - thr, left - thr, p.g.strong, i.filt))
    for bd in (8, 10):
        for strong in (True, False):
            assert {(bd, -1, -1, strong, 2 if strong else 1), (bd, 0, -1, strong, 1), (bd, -1, 0, strong, 1)} <= seen
    chroma = [(t, i) for p, t, i in tbs_of("filter", "filter/444") if t.tag]
    assert {(t.cidx, i.filt) for t, i in chroma} == {(0, 2), (1, 1), (2, 1)}  # chroma 32x32: [1 2 1] all the same


def test_coverage_availability_patterns():
    pat = {}
    for p, t, i in tbs_of("availability"):
        n = 1 << t.log2
        pat.setdefault((min(t.cidx, 1), n), set()).add(iv.pattern(i, n))
    # beyond the seven every size has.  Not reachable: x = 0 with above-right missing needs a TB as wide as
    # the picture, and a width is a multiple of 8 (no such 4x4 luma TB); left and below-left available with
    # above-right missing needs a taller TB on the left of a TB at the picture's right edge or before a
    # later quadrant: a 4x4 luma TB there has its 4x4 sibling on the left (width a multiple of 8), a 32x32
    # TB with below-left available is the first of a 64 CTB, whose above-right is the CTB row above;
    # part-way cuts need 2n > 8 luma samples
    narrow, taller = ("none", "none", "all", "none"), ("all", "all", "all", "none")
    part = {("all", "none", "all", "part"), ("all", "part", "all", "part")}
    extra = {(0, 4): set(), (0, 8): {narrow, taller}, (0, 16): {narrow, taller} | part,
             (0, 32): {narrow, ("all", "none", "all", "part")}, (1, 4): {narrow, taller},
             (1, 8): {narrow, taller} | part, (1, 16): {narrow, ("all", "none", "all", "part")}}
    assert set(pat) == set(extra)
    for k, e in extra.items():
        assert CORE | e <= pat[k], (k, sorted((CORE | e) - pat[k]))


def test_coverage_availability_causes():
    """each cause of a missing or present group, from the geometry alone"""
    causes = {}
    for p, t, i in tbs_of("availability"):
        if t.cidx:
            continue
        n, g = 1 << t.log2, p.g
        ctb = 1 << g.log2_ctb
        left, bl, above, ar = iv.pattern(i, n)
        c = causes.setdefault(n, set())
        same_ctu_right = (t.x + n) // ctb == t.x // ctb
        if above == "all" and ar == "none":
            c.add("ar_edge" if t.x + n >= g.W else ("ar_later_quadrant" if same_ctu_right else "ar_right_ctu"))
        if above == "all" and ar == "all" and not same_ctu_right and t.y % ctb == 0:
            c.add("ar_above_right_ctu")
        if above == "all" and t.x // ctb == (g.W - 1) // ctb and t.y % ctb == 0 and t.x + n == (t.x // ctb + 1) * ctb:
            c.add("last_ctu_column")
        same_ctu_below = (t.y + n) // ctb == t.y // ctb
        if left == "all" and bl == "none":
            c.add("bl_edge" if t.y + n >= g.H else ("bl_later_quadrant" if t.x % ctb else "bl_left_ctu_below")
                  if same_ctu_below or t.x % ctb == 0 else "bl_ctu_below")
        if left == "all" and bl == "all":
            c.add("bl_earlier_quadrant" if t.x % ctb else "bl_left_ctu")
    for n in (4, 8, 16, 32):
        want = {"ar_edge", "ar_right_ctu", "ar_above_right_ctu", "bl_edge", "bl_left_ctu"}
        if n < 32:
            want |= {"ar_later_quadrant", "bl_later_quadrant", "bl_earlier_quadrant"}
        assert want <= causes[n], (n, sorted(want - causes[n]))


def test_coverage_substitution_arms():
    arms = {}
    for name, chunk in (("availability", 64), ("pairs", 32)):
        for p, t, i in tbs_of(name):
            arms.setdefault((name, min(t.cidx, 1), 1 << t.log2), set()).update(iv.substitution_arms(i.avail, chunk))
    every = {"same_chunk", "earlier_chunk", "first_same_chunk", "first_later_chunk", "no_sample"}
    # 32x32 (129 positions: below-left and left | corner, above, above-right but its last | that last):
    assert arms[("availability", 0, 32)] == every
    # 16x16 (65 positions: all but the last above-right | that last): the first available sample in a
    # later chunk would be that last sample alone, which is never available without the ones before it
    assert arms[("availability", 0, 16)] == every - {"first_later_chunk"}
    assert arms[("availability", 1, 16)] == every - {"first_later_chunk"}
    # predict_pair's halves of 32: an 8x8 chroma TB's 33rd neighbour is its second chunk
    assert arms[("pairs", 1, 8)] >= {"same_chunk", "earlier_chunk", "first_same_chunk", "no_sample"}
    # the 33rd is its own or takes the nearest sample of the first 32 (a picture's edge never cuts the
    # above-right group before its last sample alone: widths are multiples of 4 chroma samples)
    tails = {(bool(i.avail[31]), bool(i.avail[32])) for p, t, i in tbs_of("pairs") if t.cidx and t.log2 == 3}
    assert tails == {(True, True), (False, False)}
    # mode 34 alone reads it (sample (7, 7) is ref[16]): pairs whose 33rd is substituted from the first 32
    # (with different samples at the first and at the nearest available position)
    n_33rd = 0
    for p, t, i in tbs_of("pairs"):
        if t.cidx and t.log2 == 3 and t.mode == 34 and not i.avail[32] and i.avail[:32].any():
            pos, idx, pl = ref.search_positions(8), np.flatnonzero(i.avail), p.planes[t.cidx]
            (fx, fy), (lx, ly) = pos[idx[0]], pos[idx[-1]]
            n_33rd += pl[t.y + fy, t.x + fx] != pl[t.y + ly, t.x + lx]
    assert n_33rd >= 4


def test_coverage_edges():
    clips, dc = {}, set()
    for p, t, i in tbs_of("edges", "edges/bd8/"):
        if t.tag:
            clips.setdefault((min(t.cidx, 1), 1 << t.log2, t.mode), set()).update(i.clips)
    for p, t, i in tbs_of("edges", "edges/bd10/"):
        if t.tag:
            clips.setdefault((min(t.cidx, 1), 1 << t.log2, t.mode), set()).update(i.clips)
    for n in (4, 8, 16):
        for m in (10, 26):
            assert {"edge_lo", "edge_hi", "edge_mid", "rec_lo", "rec_hi", "rec_mid"} <= clips[(0, n, m)], (n, m)
    for key, c in clips.items():
        if key[0] or key[1] == 32:
            assert not {"edge_lo", "edge_hi", "edge_mid"} & c, key  # absent at n = 32 and for chroma
    assert {k[1] for k in clips if k[0] == 1} >= {4, 8, 16} and (0, 32, 10) in clips and (0, 32, 26) in clips
    # the DC edge filter: the model's DC TB differs from a flat dcVal for luma n < 32 and nowhere else
    for p, t, i in tbs_of("modes"):
        if t.tag and t.mode == 1 and not t.cbf:
            n = 1 << t.log2
            flat = len(np.unique(p.planes[t.cidx][t.y:t.y + n, t.x:t.x + n])) == 1
            assert flat == (t.cidx > 0 or n == 32), t.tag
            dc.add((p.g.chroma_format, min(t.cidx, 1), n))
    assert {(1, 0, 4), (1, 0, 32), (1, 1, 16), (3, 1, 4), (3, 1, 16), (3, 1, 32)} <= dc
    # the two depths differ: the default value, the clip and the strong threshold from the right one
    for bdy, bdc in ((10, 12), (12, 10)):
        seen = set()
        for p, t, i in tbs_of("edges", f"edges/bd{bdy}_{bdc}/"):
            if not t.tag:
                continue
            bd = bdc if t.cidx else bdy
            n = 1 << t.log2
            blk = p.planes[t.cidx][t.y:t.y + n, t.x:t.x + n]
            if not i.avail.any() and not t.cbf:
                assert (blk == 1 << (bd - 1)).all()
                seen.add(("default", t.cidx > 0))
            if "rec_hi" in i.clips:
                assert blk.max() == (1 << bd) - 1
                seen.add(("hi", t.cidx > 0))
            if "rec_lo" in i.clips:
                seen.add(("lo", t.cidx > 0))
            if "strong_top" in p.name and t.cidx == 0:
                top, left, thr = i.strong_terms
                assert thr == 1 << (bdy - 5) and left == thr - 1 and i.filt == (2 if top < thr else 1)
                seen.add(("strong", top - thr))
        assert seen == {("default", False), ("default", True), ("hi", False), ("hi", True), ("lo", False),
                        ("lo", True), ("strong", -1), ("strong", 0)}, (bdy, bdc, seen)


def test_coverage_pairs():
    modes, combos, pats = {4: set(), 8: set()}, set(), {4: set(), 8: set()}
    lane63 = differ = big = pcm_pair = 0
    for p in iv.case("pairs").pics:
        info = {id(t): i for t, i in zip(p.tbs, p.infos)}
        for r, row in enumerate(p.rows):
            recs = p.records(r)
            paired = set(iv.formed_pairs(recs))
            for k, t in enumerate(row[:-1]):
                nx = row[k + 1]
                if t.cidx == 1 and nx.cidx == 2:
                    n = 1 << t.log2
                    if k in paired:
                        modes[n].add(t.mode)
                        combos.add((t.cbf, nx.cbf))
                        pats[n].add(iv.pattern(info[id(t)], n))
                        pcm_pair += t.pcm and nx.pcm
                        assert not (p.want[1][t.y:t.y + n, t.x:t.x + n] == p.want[2][t.y:t.y + n, t.x:t.x + n]).all()
                    elif n > 8:
                        big += 1
                    elif t.mode != nx.mode:
                        differ += 1
                    elif k % 64 == 63:
                        lane63 += 1
    assert modes[4] == set(range(35)) and modes[8] == set(range(35))
    assert combos == {(False, False), (True, False), (False, True), (True, True)}
    assert lane63 and differ and big and pcm_pair
    for n in (4, 8):
        assert CORE <= pats[n], (n, sorted(CORE - pats[n]))
    assert ("all", "part", "all", "part") in pats[8]


def test_coverage_formats():
    seen = set()
    for p, t, i in tbs_of("formats"):
        g, n = p.g, 1 << t.log2
        seen.add((g.chroma_format, g.bd_y))
        if g.chroma_format == 0:
            assert t.cidx == 0
        if g.chroma_format == 2 and t.cidx:
            x, y, l = t.tu
            lower = t.y != y
            left, bl, above, ar = iv.pattern(i, n)
            if lower:
                # above it the upper TB of the same TU; right of that a TU that comes later, always
                assert above == "all" and ar == "none"
                seen.add(("422_lower", left))
            else:
                seen.add(("422_upper_bl", bl))
            if g.log2_ctb == 6 and t.y % 64 >= 32:
                seen.add("422_ctb_64_high")
        if g.chroma_format == 3 and t.cidx and n == 32:
            seen.add(("444_chroma32", i.filt))
    assert {(cf, bd) for cf in (0, 2, 3) for bd in (8, 10)} <= seen
    assert {("422_lower", "all"), ("422_lower", "none"), ("422_upper_bl", "all"), ("422_upper_bl", "none"),
            "422_ctb_64_high", ("444_chroma32", 1), ("444_chroma32", 0)} <= seen


def test_coverage_dispatch():
    b, = iv.case("dispatch").batches
    assert b.pic0 == 1 and not b.pics[0].live
    launched = b.pics[b.pic0:]
    assert any(p.flags & iv.PD_ASSEMBLY and any(len(r) for r in p.rows) for p in launched)
    assert {p.g.log2_ctb for p in launched if p.live} == {4, 5, 6}
    rows = sorted(len(p.rows) for p in launched if p.live)
    # 10-bit 4:2:0 with a 64 CTB in the launch: the LDS holds 9 waves' windows, the launch has at most 12 rows
    assert rows[0] == 1 and rows[-1] == 12
    for kind, n_bad in (("mode35", 1), ("edge", 2), ("outside", 3)):
        p, = [p for p in launched if p.name.endswith("garbage_" + kind)]
        assert len(p.records(0)) >= len(p.rows[0]) + 3 * n_bad
    p, = [p for p in launched if p.name.endswith("stop")]
    recs = p.records(1)
    wctb = -(-p.g.W >> p.g.log2_ctb)
    k = [q["ctu"] >= wctb for q in recs].index(True)
    assert 0 < k < len(recs) - 1 and (p.planes[0][32:, 64:] < 0).all() and (p.planes[0][32:, :64] >= 0).all()


def test_coverage_sentinels():
    for name in CASE_NAMES:
        for b in iv.case(name).batches:
            sent = b.expected == iv.SENTINEL
            assert sent.any() and (~sent).any(), name


# ---------------------------------------------------------------- layout
def test_layout_mirrors_match_the_structs(emu_driver):
    r = subprocess.run([str(emu_driver), "--layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    theirs = {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}
    assert theirs == iv.layout_of_mirrors()


# ---------------------------------------------------------------- the two legs
@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulated_intra_equals_model(emu_driver, tmp_path, name):
    for env in knob_settings(name):
        bad = run_case(emu_driver, name, tmp_path, env)
        assert not bad, f"{env}: " + report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_intra_equals_model(gpu_driver, tmp_path, name):
    for env in knob_settings(name):
        bad = run_case(gpu_driver, name, tmp_path, env)
        assert not bad, f"{env}: " + report(bad)
