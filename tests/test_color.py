"""The colour-managed render on the host (no device): the colour description of an
item, the ICC reader, the transform's tables against the float64 model of
color_ref, heifgpu_color_apply against color_ref's numpy formula (exactly) and
against the unquantised float64 transform (the accuracy), and the reader over
hostile profiles as a stand-alone ASan + UBSan program.  The kernels are in
tests/test_color_gpu.py."""
import ctypes
import subprocess

import numpy as np
import pytest

import color_ref
from conftest import ROOT, make_emu

P3 = ((0x83DF, 0x3DBF, -0x45), (0x4ABF, 0xB137, 0x0AB9), (0x2838, 0x110B, 0xC8B9))  # s15.16: X Y Z of R, G, B


@pytest.fixture(scope="module")
def H():
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def S():
    from heif_amd import synth_encoder

    return synth_encoder


def image_with(H, S, colr=None, **kw):
    p = S.SynthParams(width=16, height=16, **kw)
    return H.HeifImage.parse(S.display_heic(p, colr=colr))


def apply_lib(t, rgb):
    """heifgpu_color_apply over (n, 3) codes."""
    from heif_amd import _lib

    src = np.ascontiguousarray(rgb, np.uint16)
    out = np.empty_like(src)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    _lib.check(_lib.lib.heifgpu_color_apply(ctypes.byref(t), src.ctypes.data_as(u16p), len(src), out.ctypes.data_as(u16p)))
    return out.astype(np.int64)


def test_halfmoonbay_description(H, halfmoonbay):
    """The golden sample's primary item: a Display P3 matrix/TRC profile.  (The colr box
    is 560 bytes: 8 of box header, 'prof', and a profile of 548 bytes whose own size field
    says 0x224 = 548.)"""
    img = H.HeifImage.parse(halfmoonbay)
    c = img.color
    assert c.kind == "icc" and c.status == 0 and not c.has_nclx and c.icc_size == 548
    assert np.array_equal(np.array(c.colorants) * 65536.0, np.array(P3, np.float64))
    icc = img.icc_profile
    assert len(icc) == 548 and icc[:4] == bytes([0, 0, 2, 0x24])
    assert icc[12:24] == b"mntrRGB XYZ " and icc[36:40] == b"acsp"
    assert img.color_transform("display-p3").identity == 1
    t = img.color_transform("srgb")
    assert t.identity == 0 and list(t.m) != [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]
    with pytest.raises(ValueError):
        img.color_transform("adobe-rgb")


def test_nclx_and_unlabelled_sources(H, S):
    none = image_with(H, S)
    nclx = image_with(H, S, colr=S.nclx_box(1, 13, 6, True))
    assert none.color.kind == "none" and none.icc_profile is None and none.color.icc_size == 0
    assert nclx.color.kind == "nclx" and (nclx.color.primaries, nclx.color.transfer) == (1, 13)
    assert nclx.info.matrix_coeffs == 6 and nclx.info.full_range == 1
    for img in (none, nclx):
        for bits in (8, 10, 12):
            t = img.color_transform("srgb", bits)
            assert t.identity == 1 and list(t.m) == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384], bits
        t = img.color_transform("display-p3")
        assert t.identity == 0 and t.m[1] > 1000  # sRGB red holds P3 green
    # P3 D65 primaries are Display P3's own: exactly the identity matrix
    p3 = image_with(H, S, colr=S.nclx_box(12, 13, 1, False)).color_transform("display-p3")
    assert p3.identity == 1 and list(p3.m) == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]
    # unspecified codes are taken as sRGB; PQ / HLG need tone mapping; the image itself parses
    assert image_with(H, S, colr=S.nclx_box(2, 2, 2, False)).color_transform("srgb").identity == 1
    for transfer in (16, 18):
        hdr = image_with(H, S, colr=S.nclx_box(9, transfer, 9, False))
        assert hdr.color.status == -3 and hdr.color.colorants is None
        with pytest.raises(H.UnsupportedError):
            hdr.color_transform("srgb")
    with pytest.raises(H.UnsupportedError):
        image_with(H, S, colr=S.nclx_box(5, 1, 5, False)).color_transform("srgb")


def test_profile_wins_for_colour_and_nclx_for_the_matrix(H, S):
    prof = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    for order in ((S.icc_box(prof), S.nclx_box(1, 13, 6, True)), (S.nclx_box(1, 13, 6, True), S.icc_box(prof, b"rICC"))):
        img = image_with(H, S, colr=order)
        c = img.color
        assert c.kind == "icc" and c.has_nclx and (c.primaries, c.transfer) == (1, 13) and img.icc_profile == prof
        assert img.info.matrix_coeffs == 6 and img.info.full_range == 1
        assert img.color_transform("display-p3").identity == 1 and img.color_transform("srgb").identity == 0


def test_builders_keep_existing_bytes(S):
    p = S.SynthParams(width=16, height=16)
    box = S.nclx_box(1, 13, 6, True)
    assert S.display_heic(p, colr=box) == S.display_heic(p, colr=[box]) and S.display_heic(p) == S.display_heic(p, colr=())
    assert S.icc_box(b"abc") == b"\x00\x00\x00\x0fcolrprofabc"


CURVES = {
    "curv0": lambda S: S.icc_curv(()),
    "curv1": lambda S: S.icc_curv((2.2,)),
    "curvn": lambda S: S.icc_curv([int(round(65535 * (i / 32) ** 1.8)) for i in range(33)]),
    "para0": lambda S: S.icc_para(0, (2.2,)),
    "para1": lambda S: S.icc_para(1, (2.0, 0.9, 0.1)),
    "para2": lambda S: S.icc_para(2, (2.0, 0.8, 0.1, 0.05)),
    "para3": lambda S: S.ICC_SRGB_PARA,
    "para4": lambda S: S.icc_para(4, (2.4, 0.9, 0.05, 0.07, 0.04, 0.02, 0.01)),
}


@pytest.mark.parametrize("curve", list(CURVES))
@pytest.mark.parametrize("version", [2, 4])
def test_curves_parse_and_tables_follow_the_model(H, S, curve, version):
    """Every TRC form from a profile the writer emits: in_lut and out_lut within 1 unit of
    the float64 model at 8, 10 and 12 bits (1: libm and numpy pow may differ in the last ulp
    of a value that is then rounded), m within 1 before the row fix-up and within 2 after
    (a row of three roundings is off by at most 1.5, so its largest entry moves by at most 1),
    rows summing to 16384."""
    prof = S.icc_profile(S.ICC_COLORANTS_SRGB if curve != "para3" else S.ICC_COLORANTS_DISPLAY_P3, CURVES[curve](S),
                         version=version, raw_colorants=True)
    img = image_with(H, S, colr=S.icc_box(prof))
    assert img.color.status == 0
    for dst in ("srgb", "display-p3"):
        model = color_ref.Model(prof, dst)
        for bits in (8, 10, 12):
            t = img.color_transform(dst, bits)
            _, in_lut, m, out_lut = color_ref.tables(t)
            assert np.abs(in_lut - model.in_lut(bits)).max() <= 1, (dst, bits)
            assert np.abs(out_lut - model.out_lut(bits)).max() <= 1, (dst, bits)
            assert np.abs(np.array(list(t.m_rounded)) - model.m_q14()).max() <= 1.0
            assert np.abs(m - model.m_q14()).max() <= 2.0
            assert (m.reshape(3, 3).sum(axis=1) == 16384).all()


def test_separate_curves_per_channel(H, S):
    trcs = [S.icc_curv((1.8,)), S.icc_para(0, (2.4,)), S.icc_curv(())]
    prof = S.icc_profile(S.ICC_COLORANTS_SRGB, trcs, raw_colorants=True)
    t = image_with(H, S, colr=S.icc_box(prof)).color_transform("srgb")
    model = color_ref.Model(prof, "srgb")
    _, in_lut, _, _ = color_ref.tables(t)
    assert np.abs(in_lut - model.in_lut(8)).max() <= 1
    assert len({tuple(r) for r in in_lut}) == 3 and t.identity == 0


def sources(H, S, halfmoonbay):
    bt2020 = S.icc_profile(color_ref.nclx_colorants(9), S.icc_curv((2.2,)))
    return {
        "p3-profile": (H.HeifImage.parse(halfmoonbay), H.HeifImage.parse(halfmoonbay).icc_profile),
        "srgb-nclx": (image_with(H, S, colr=S.nclx_box(1, 13, 1, False)), (1, 13)),
        "bt2020-gamma": (image_with(H, S, colr=S.icc_box(bt2020)), bt2020),
    }


CASES = [("p3-profile", "srgb"), ("srgb-nclx", "display-p3"), ("bt2020-gamma", "srgb")]
# |integer path - unquantised float64 transform| in codes over the lattice.  At 8 bits the
# bound is the issue's: 1 code (found: 0.61, 0.54, 0.62 for the three cases below).  At 10 and
# 12 bits the figures were measured on the CPU and are pinned as found: 0.99,
# 0.83, 0.98 at 10 bits and 2.80, 1.49, 2.83 at 12 (the 16-bit in_lut and the 1/16-level
# out_lut steps are coarse next to a 12-bit code near black, where the sRGB encoding is steepest)
ACCURACY = {8: 1.0, 10: 1.0, 12: 2.9}


@pytest.mark.parametrize("bits,step", [(8, 5), (10, 17), (12, 67)])
@pytest.mark.parametrize("name,dst", CASES)
def test_apply_equals_numpy_and_follows_the_float_model(H, S, halfmoonbay, name, dst, bits, step):
    img, source = sources(H, S, halfmoonbay)[name]
    t = img.color_transform(dst, bits)
    maxv = (1 << bits) - 1
    codes = color_ref.lattice(bits, step)
    got = apply_lib(t, codes)
    assert np.array_equal(got, color_ref.apply(t, codes))  # the C function is the numpy formula
    neutral = codes[(codes[:, 0] == codes[:, 1]) & (codes[:, 1] == codes[:, 2])]
    out = apply_lib(t, neutral)
    assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all()  # neutrals stay neutral
    assert apply_lib(t, [[maxv] * 3]).tolist() == [[maxv] * 3] and apply_lib(t, [[0, 0, 0]]).tolist() == [[0, 0, 0]]
    assert got.min() == 0 and got.max() == maxv  # out of gamut: both clamps
    err = np.abs(got - color_ref.Model(source, dst).transform(bits, codes)).max()
    print(f"accuracy {name} -> {dst} at {bits} bits: {err:.4f} codes")
    assert err <= ACCURACY[bits], (name, dst, bits, err)


def test_apply_rejects_codes_above_maxv(H, S):
    from heif_amd import _lib

    t = image_with(H, S).color_transform("display-p3")
    with pytest.raises(H.HeifGpuError):
        apply_lib(t, [[0, 256, 0]])
    bad = _lib.ColorTransform()
    assert _lib.lib.heifgpu_color_transform_make(image_with(H, S)._h, 2, 8, ctypes.byref(bad)) == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_color_transform_make(image_with(H, S)._h, 0, 13, ctypes.byref(bad)) == _lib.HEIFGPU_E_INVALID


def test_refused_profiles_still_parse(H, S):
    """What is refused is refused when a transform is asked for: the item parses, reports its
    profile and would decode."""
    lut = S.icc_profile(None, S.icc_curv(()), extra_tags=[(b"A2B0", b"mft2" + bytes(48))])
    cases = {
        "lut": (lut, -3),
        "lab": (S.icc_profile(S.ICC_COLORANTS_SRGB, S.icc_curv(()), pcs=b"Lab ", raw_colorants=True), -3),
        "cmyk": (S.icc_profile(S.ICC_COLORANTS_SRGB, S.icc_curv(()), data_space=b"CMYK", raw_colorants=True), -3),
        "para5": (S.icc_profile(S.ICC_COLORANTS_SRGB, S.icc_para(5, (1.0,)), raw_colorants=True), -3),
        "short": (S.icc_profile(S.ICC_COLORANTS_SRGB, S.icc_curv(()), raw_colorants=True)[:100], -2),
    }
    good = S.icc_profile(S.ICC_COLORANTS_SRGB, S.icc_curv((1.0, 2.0, 3.0)), raw_colorants=True)
    size_beyond = (len(good) + 1).to_bytes(4, "big") + good[4:]
    curv_beyond = bytearray(good)
    at = good.index(b"curv")
    curv_beyond[at + 8:at + 12] = (4).to_bytes(4, "big")  # four entries claimed, the tag holds three
    tag_outside = bytearray(good)
    tag_outside[132 + 4:132 + 8] = (len(good) - 4).to_bytes(4, "big")  # rXYZ: 20 bytes from 4 before the end
    cases.update({"size": (size_beyond, -2), "curv": (bytes(curv_beyond), -2), "tag": (bytes(tag_outside), -2)})
    for name, (prof, code) in cases.items():
        img = image_with(H, S, colr=S.icc_box(prof))
        assert img.icc_profile == prof and img.color.kind == "icc" and img.color.status == code, name
        assert img.info.width == 16
        with pytest.raises(H.UnsupportedError if code == -3 else H.HeifGpuError) as e:
            img.color_transform("srgb")
        assert e.value.code == code, name


def test_reader_under_sanitizers(H, halfmoonbay, tmp_path):
    """tests/color/icc_driver.cpp (make color-asan): halfmoonbay's profile truncated at every
    length, and the size field, the tag count and every field of the tag table set in turn to
    0, 0xFFFFFFFF and size - 1; every case answers OK, E_PARSE or E_UNSUPPORTED and the
    program exits clean.  Nothing is loaded into Python under a sanitizer."""
    make_emu("color-asan")
    prof = H.HeifImage.parse(halfmoonbay).icc_profile
    path = tmp_path / "p3.icc"
    path.write_bytes(prof)
    exe = ROOT / "heif_amd" / "csrc" / "build" / "color_asan" / "icc_driver"
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    n_tags = int.from_bytes(prof[128:132], "big")
    assert len(lines) == 1 + len(prof) + 3 * (2 + 3 * n_tags)
    assert lines[0] == "whole OK"
    answers = {ln.rsplit(" ", 1)[1] for ln in lines}
    assert answers <= {"OK", "E_PARSE", "E_UNSUPPORTED"} and "E_PARSE" in answers
    assert all(ln.endswith("E_PARSE") for ln in lines[1:1 + len(prof)])  # every truncation: the size field
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
