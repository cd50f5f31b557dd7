"""The HDR render on the host (no device): what clli / mdcv say and the source peak they
give, the tone transform's tables against the float64 model of tone_ref,
heifgpu_color_apply on a tone transform against tone_ref's numpy formula (exactly) and
against the unquantised float64 transform (the accuracy), the opt-in rule, the ABI, and
the reader and builder as a stand-alone ASan + UBSan program.  The kernels are in
tests/test_tone_gpu.py."""
import ctypes
import subprocess

import numpy as np
import pytest

import color_ref
import tone_ref
from conftest import ROOT, make_emu

SPACES = ("srgb", "display-p3")
# (name, transfer, peak_nits): PQ at two source peaks, and HLG (its peak is 1000 by rule)
SOURCES = [("pq-1000", 16, 1000.0), ("pq-4000", 16, 4000.0), ("hlg", 18, None)]


@pytest.fixture(scope="module")
def H():
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def S():
    from heif_amd import synth_encoder

    return synth_encoder


def heic_with(S, colr=None, props=(), **kw):
    return S.display_heic(S.SynthParams(width=16, height=16, **kw), colr=colr, transforms=tuple(props))


def hdr_image(H, S, transfer=16, primaries=9, props=()):
    return H.HeifImage.parse(heic_with(S, S.nclx_box(primaries, transfer, 9, False), props))


def apply_lib(t, rgb):
    """heifgpu_color_apply over (n, 3) codes, for either kind of transform."""
    from heif_amd import _lib

    src = np.ascontiguousarray(rgb, np.uint16)
    out = np.empty_like(src)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    base = t.base if tone_ref.is_tone(t) else t
    _lib.check(_lib.lib.heifgpu_color_apply(ctypes.byref(base), src.ctypes.data_as(u16p), len(src), out.ctypes.data_as(u16p)))
    return out.astype(np.int64)


# ---- the boxes and the source peak ---------------------------------------------
def test_hdr_description(H, S):
    both = hdr_image(H, S, props=(S.clli_box(400, 120), S.mdcv_box(max_nits=4000.0, min_nits=0.005)))
    h = both.hdr
    assert (h.transfer, h.max_cll, h.max_fall, h.status) == (16, 400, 120, 0)
    assert h.mastering_max == pytest.approx(4000.0) and h.mastering_min == pytest.approx(0.005)
    bare = hdr_image(H, S, transfer=18).hdr
    assert (bare.transfer, bare.max_cll, bare.max_fall, bare.mastering_max, bare.mastering_min) == (18, None, None, None, None)
    # an SDR item, an unlabelled one and one whose profile wins have none
    assert H.HeifImage.parse(heic_with(S, S.nclx_box(1, 13, 6, True), (S.clli_box(400, 120),))).hdr is None
    assert H.HeifImage.parse(heic_with(S)).hdr is None
    prof = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    assert H.HeifImage.parse(heic_with(S, (S.nclx_box(9, 16, 9, False), S.icc_box(prof)))).hdr is None
    # the reference side reads the same bytes
    ll = tone_ref.light_levels(heic_with(S, S.nclx_box(9, 16, 9, False), (S.clli_box(400, 120), S.mdcv_box(max_nits=4000.0))))
    assert ll["clli"] == (400, 120) and ll["mdcv"][0] == pytest.approx(4000.0)


LSRC_CASES = [
    ("clli only", lambda S: (S.clli_box(400, 100),), None, 400.0),
    ("mdcv only", lambda S: (S.mdcv_box(max_nits=1500.0),), None, 1500.0),
    ("both: MaxCLL first", lambda S: (S.mdcv_box(max_nits=4000.0), S.clli_box(600, 100)), None, 600.0),
    ("neither", lambda S: (), None, 1000.0),
    ("MaxCLL zero: the mdcv maximum", lambda S: (S.clli_box(0, 0), S.mdcv_box(max_nits=2000.0)), None, 2000.0),
    ("every field zero", lambda S: (S.clli_box(0, 0), S.mdcv_box(max_nits=0.0, min_nits=0.0)), None, 1000.0),
    ("peak_nits overrides", lambda S: (S.clli_box(400, 100),), 2500.0, 2500.0),
    ("clamp to 203", lambda S: (S.clli_box(80, 40),), None, 203.0),
    ("peak_nits clamped to 203", lambda S: (), 100.0, 203.0),
    ("clamp to 10000", lambda S: (S.clli_box(0xFFFF, 0),), None, 10000.0),
]


@pytest.mark.parametrize("name,props,peak,want", LSRC_CASES, ids=[c[0] for c in LSRC_CASES])
def test_source_peak_rule(H, S, name, props, peak, want):
    f = heic_with(S, S.nclx_box(9, 16, 9, False), props(S))
    assert tone_ref.source_peak(f, 16, peak) == pytest.approx(want)
    t = H.HeifImage.parse(f).color_transform("srgb", 8, "bt2390", peak)
    assert t.tone == 1 and t.transfer == 16 and t.Lsrc == pytest.approx(want)
    # the table is the model's at that peak (and so differs between peaks)
    assert np.abs(np.array(t.T[:tone_ref.ENTRIES], np.int64) - tone_ref.Model(9, 16, "srgb", want).T()).max() <= 1
    # HLG: the nominal display whatever the file or the caller says
    g = heic_with(S, S.nclx_box(9, 18, 9, False), props(S))
    assert H.HeifImage.parse(g).color_transform("srgb", 8, "bt2390", peak).Lsrc == 1000.0


def test_truncated_boxes_parse_and_are_reported_by_the_transform(H, S):
    from heif_amd import _lib

    for box, full in ((lambda n: S.clli_box(400, 100, truncate=n), 4), (lambda n: S.mdcv_box(truncate=n), 24)):
        for n in (0, 1, full - 1):
            f = heic_with(S, S.nclx_box(9, 16, 9, False), (box(n),), bit_depth=10)
            img = H.HeifImage.parse(f)  # parses as ever
            assert img.info.bit_depth == 10 and img.color.status == -3
            assert img.hdr.status == _lib.HEIFGPU_E_PARSE
            with pytest.raises(H.HeifGpuError) as e:
                img.color_transform("srgb", 10, "bt2390")
            assert e.value.code == _lib.HEIFGPU_E_PARSE and not isinstance(e.value, H.UnsupportedError)
            with pytest.raises(H.HeifGpuError):  # the caller's peak does not hide a damaged file
                img.color_transform("srgb", 10, "bt2390", 1000.0)
            assert tone_ref.light_levels(f)[("clli", "mdcv")[full == 24]] is None
        img = H.HeifImage.parse(heic_with(S, S.nclx_box(9, 16, 9, False), (box(full),)))
        assert img.hdr.status == 0 and img.color_transform("srgb", 8, "bt2390").tone == 1
    # an SDR item with a short box is not a tone transform: nothing to report
    sdr = H.HeifImage.parse(heic_with(S, S.nclx_box(1, 13, 1, False), (S.clli_box(1, 1, truncate=2),)))
    assert sdr.color_transform("srgb", 8, "bt2390").identity == 1


# ---- the tables -----------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10, 12])
@pytest.mark.parametrize("primaries", [1, 9, 12])
@pytest.mark.parametrize("name,transfer,peak", SOURCES)
def test_tables_follow_the_model(H, S, name, transfer, peak, primaries, bits):
    img = hdr_image(H, S, transfer, primaries)
    for dst in SPACES:
        t = img.color_transform(dst, bits, "bt2390", peak)
        model = tone_ref.Model(primaries, transfer, dst, peak or 1000.0)
        _, in32, w, T, m, out_lut = tone_ref.tables(t)
        assert (t.bits, t.identity, t.tone, t.transfer, t.dst) == (bits, 0, 1, transfer, ("srgb", "display-p3").index(dst))
        assert np.abs(in32 - model.in_lut32(bits)).max() <= 1 and in32.max() <= tone_ref.MAX_LEVEL
        assert (in32[0] == in32[1]).all() and (in32[1] == in32[2]).all()
        assert np.abs(T - model.T()).max() <= 1 and T.max() <= 1 << tone_ref.SHIFT
        assert T[0] == ((1 << tone_ref.SHIFT) if transfer == 16 else 0)
        assert (np.diff(T) <= 0).all() if transfer == 16 else T[1] > 0  # a PQ gain only falls
        # w by the rules of the matrix rows: rounded to nearest, the largest entry fixed up
        assert w.sum() == 16384 and (w >= 0).all()
        d = w - model.w_q14()
        big = int(np.argmax(w))
        assert np.abs(np.delete(d, big)).max() <= 0.5 + 1e-9 and abs(d[big]) <= 1.5 + 1e-9
        # m and out_lut are those of the same primaries coded linearly
        lin = H.HeifImage.parse(heic_with(S, S.nclx_box(primaries, 8, 9, False))).color_transform(dst, bits)
        assert list(t.base.m) == list(lin.m) and list(t.base.m_rounded) == list(lin.m_rounded)
        assert list(t.base.out_lut) == list(lin.out_lut)
        assert not np.array(t.base.in_lut).any()
        if primaries == color_ref.OWN_PRIMARIES[dst]:
            assert list(t.base.m) == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]


def test_index_nodes():
    """The floating index: continuous, 32 nodes per octave, node levels as the header states."""
    k = np.arange(tone_ref.ENTRIES)
    lv = tone_ref.node(k)
    assert (np.diff(lv) > 0).all() and lv[63] == 63 and lv[64] == 64 and lv[96] == 128 and lv[576] == 1 << 22
    idx, e, frac = tone_ref.index(lv[:-1])
    assert np.array_equal(idx, k[:-1]) and not frac.any()
    idx, e, frac = tone_ref.index(np.array([63, 64, 65, 127, 128, 129, tone_ref.MAX_LEVEL]))
    assert idx.tolist() == [63, 64, 64, 95, 96, 96, 575] and e.tolist() == [0, 1, 1, 1, 2, 2, 16]
    assert frac.tolist() == [0, 0, 1, 1, 0, 1, (1 << 16) - 1]


# ---- the formula and its accuracy -------------------------------------------------
def special_codes(t):
    """The grey axis, the pure primaries, and the codes around Y = 63 / 64 and around every
    octave boundary of the index (greys, whose Y is their level, and mixtures next to them)."""
    bits, in32, w, T, m, out_lut = tone_ref.tables(t)
    n = 1 << bits
    v = np.arange(n)
    z = np.zeros(n, np.int64)
    sets = [np.stack([v, v, v], -1), np.stack([v, z, z], -1), np.stack([z, v, z], -1), np.stack([z, z, v], -1)]
    edge = []
    for b in [63, 64] + [1 << s for s in range(7, 23)]:
        c = int(np.searchsorted(in32[0], b))
        for dv in (-2, -1, 0, 1, 2):
            for dr, dg, db in ((0, 0, 0), (1, 0, -1), (-1, 1, 0), (2, -1, 0), (0, -2, 3)):
                edge.append([min(max(c + dv + d, 0), n - 1) for d in (dr, dg, db)])
    sets.append(np.array(edge, np.int64))
    return np.concatenate(sets)


# |integer path - unquantised float64 transform| in codes over the lattice and the special
# codes, BT.2020 sources.  At 8 bits the bound is the project's: 1 code (found: at most 0.69;
# a gain table with 16 fractional bits gave 1.12, which is why it has 24).  At 10 and 12
# bits the figures were measured on the CPU and are pinned as found, rounded up to the next
# 0.1 code: the 16-bit levels behind the tone stage and the 1/16-level out_lut
# steps are coarse next to a 12-bit code near black, as in the SDR transform (tests/test_color.py)
ACCURACY = {
    ("pq-1000", "srgb"): {8: 1.0, 10: 1.9, 12: 4.7}, ("pq-1000", "display-p3"): {8: 1.0, 10: 1.6, 12: 3.3},
    ("pq-4000", "srgb"): {8: 1.0, 10: 1.9, 12: 5.1}, ("pq-4000", "display-p3"): {8: 1.0, 10: 1.6, 12: 3.2},
    ("hlg", "srgb"): {8: 1.0, 10: 1.5, 12: 4.4}, ("hlg", "display-p3"): {8: 1.0, 10: 1.1, 12: 2.6},
}


@pytest.mark.parametrize("bits,step", [(8, 5), (10, 17), (12, 67)])
@pytest.mark.parametrize("dst", SPACES)
@pytest.mark.parametrize("name,transfer,peak", SOURCES)
def test_apply_equals_numpy_and_follows_the_float_model(H, S, name, transfer, peak, dst, bits, step):
    t = hdr_image(H, S, transfer).color_transform(dst, bits, "bt2390", peak)
    maxv = (1 << bits) - 1
    model = tone_ref.Model(9, transfer, dst, peak or 1000.0)
    worst = 0.0
    for what, codes in (("lattice", color_ref.lattice(bits, step)), ("special", special_codes(t))):
        got = apply_lib(t, codes)
        assert np.array_equal(got, tone_ref.apply(t, codes)), what  # the C function is the numpy formula
        assert got.min() == 0 and got.max() == maxv, what
        worst = max(worst, float(np.abs(got - model.transform(bits, codes)).max()))
    grey = np.stack([np.arange(maxv + 1)] * 3, -1)
    out = apply_lib(t, grey)
    assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all()  # neutrals stay neutral
    # and keep their order, up to the ripple of the interpolated gain where the curve is flat:
    # between two nodes a chord of a gain falling like 1 / Y lies above it by at most
    # (1 / 32)^2 / 4 = 2.4e-4, 16 of the 65535 levels, less than one 12-bit code at white (36 levels)
    assert (np.diff(out[:, 0]) >= -1).all() and out[0, 0] == 0 and out[-1, 0] == maxv
    # every octave of the index that the source's range spans is reached by the special codes
    _, in32, w, T, *_ = tone_ref.tables(t)
    _, Y = tone_ref.luminance(in32, w, special_codes(t))
    _, e, _ = tone_ref.index(Y)
    top = int(tone_ref.index(np.array([in32.max()]))[1][0])
    assert set(range(top + 1)) <= set(e.tolist())
    print(f"accuracy {name} -> {dst} at {bits} bits: {worst:.4f} codes")
    assert worst <= ACCURACY[(name, dst)][bits], (name, dst, bits, worst)


def test_apply_rejects_what_would_leave_the_tables(H, S):
    from heif_amd import _lib

    t = hdr_image(H, S).color_transform("srgb", 8, "bt2390")
    u16p = ctypes.POINTER(ctypes.c_uint16)
    px = np.array([[0, 0, 256]], np.uint16)
    assert _lib.lib.heifgpu_color_apply(ctypes.byref(t.base), px.ctypes.data_as(u16p), 1, px.ctypes.data_as(u16p)) == _lib.HEIFGPU_E_INVALID
    bad = _lib.HdrTransform.from_buffer_copy(t)
    bad.in_lut32[2][9] = 1 << 22
    px = np.zeros((1, 3), np.uint16)
    assert _lib.lib.heifgpu_color_apply(ctypes.byref(bad.base), px.ctypes.data_as(u16p), 1, px.ctypes.data_as(u16p)) == _lib.HEIFGPU_E_INVALID
    bad = _lib.HdrTransform.from_buffer_copy(t)
    bad.w[1] += 1
    assert _lib.lib.heifgpu_color_apply(ctypes.byref(bad.base), px.ctypes.data_as(u16p), 1, px.ctypes.data_as(u16p)) == _lib.HEIFGPU_E_INVALID
    img = hdr_image(H, S)
    out = _lib.HdrTransform()
    assert _lib.lib.heifgpu_color_transform_make_hdr(img._h, 0, 8, 2, 0.0, ctypes.byref(out)) == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_color_transform_make_hdr(img._h, 2, 8, 1, 0.0, ctypes.byref(out)) == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_color_transform_make_hdr(img._h, 0, 13, 1, 0.0, ctypes.byref(out)) == _lib.HEIFGPU_E_INVALID
    # primaries outside the set stay unsupported with a tone map too
    with pytest.raises(H.UnsupportedError):
        hdr_image(H, S, primaries=5).color_transform("srgb", 8, "bt2390")


# ---- opt-in ------------------------------------------------------------------------
def test_without_tone_map_nothing_changes(H, S):
    from heif_amd import _lib

    for transfer in (16, 18):
        img = hdr_image(H, S, transfer, props=(S.clli_box(400, 100),))
        assert img.color.status == -3 and img.color.colorants is None
        with pytest.raises(H.UnsupportedError):
            img.color_transform("srgb")
        out = _lib.HdrTransform()
        assert _lib.lib.heifgpu_color_transform_make_hdr(img._h, 0, 8, _lib.TONE_NONE, 0.0, ctypes.byref(out)) == _lib.HEIFGPU_E_UNSUPPORTED
    with pytest.raises(ValueError):
        hdr_image(H, S).color_transform("srgb", 8, "reinhard")
    with pytest.raises(ValueError):
        hdr_image(H, S).color_transform("rec2020", 8, "bt2390")


def test_sdr_images_get_the_transforms_they_get_today(H, S):
    from heif_amd import _lib

    prof = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    for colr in (None, S.nclx_box(1, 13, 6, True), S.nclx_box(9, 4, 9, False), S.icc_box(prof),
                 (S.nclx_box(9, 16, 9, False), S.icc_box(prof))):  # (a profile wins over a PQ nclx: no tone stage)
        img = H.HeifImage.parse(heic_with(S, colr, (S.clli_box(400, 100),)))
        for dst in SPACES:
            for bits in (8, 10):
                plain, toned = img.color_transform(dst, bits), img.color_transform(dst, bits, "bt2390", 700.0)
                assert type(toned) is _lib.ColorTransform and toned.tone == 0
                assert bytes(plain) == bytes(toned)  # field for field
                # and through the C call: the base is that transform, the rest zeros
                h = _lib.HdrTransform()
                _lib.check(_lib.lib.heifgpu_color_transform_make_hdr(img._h, _lib.COLORSPACES[dst], bits, 1, 700.0, ctypes.byref(h)))
                assert bytes(h)[:ctypes.sizeof(_lib.ColorTransform)] == bytes(plain)
                assert not any(bytes(h)[ctypes.sizeof(_lib.ColorTransform):])
    # an unsupported SDR source stays unsupported
    with pytest.raises(H.UnsupportedError):
        H.HeifImage.parse(heic_with(S, S.nclx_box(5, 1, 5, False))).color_transform("srgb", 8, "bt2390")


def test_tone_map_alone_is_a_value_error(H):
    """The argument checks of the render family run before anything touches a device."""
    ctx = object.__new__(H.DecodeContext)  # no device behind it: the checks come first
    for call in (lambda **kw: ctx.render([], **kw), lambda **kw: ctx.render_scaled([], (8, 8), **kw),
                 lambda **kw: ctx.render_tensor([], (8, 8), **kw)):
        with pytest.raises(ValueError, match="colorspace"):
            call(tone_map="bt2390")
        with pytest.raises(ValueError, match="tone_map"):
            call(colorspace="srgb", tone_map="hable")
    for call in (H.HeicDecoder.decode_display, lambda d, **kw: H.HeicDecoder.decode_tensor(d, (8, 8), **kw)):
        with pytest.raises(ValueError, match="colorspace"):
            call(b"", tone_map="bt2390")


# ---- the ABI ------------------------------------------------------------------------
def test_abi_is_still_6_and_the_structs_keep_their_sizes():
    from heif_amd import _lib

    assert _lib.lib.heifgpu_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert ctypes.sizeof(_lib.ColorTransform) == 16 + 2 * 36 + 3 * 4096 * 2 + 4098 * 2 == 32860
    assert _lib.ColorTransform.tone.offset == 12 and _lib.ColorTransform.m.offset == 16
    assert ctypes.sizeof(_lib.ColorInfo) == 24 + 72
    assert _lib.HdrTransform.base.offset == 0 and _lib.HdrTransform.in_lut32.offset == 32860
    assert ctypes.sizeof(_lib.HdrInfo) == 32
    for name in ("heifgpu_image_get_hdr", "heifgpu_color_transform_make_hdr"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    header = (ROOT / "include" / "heifgpu.h").read_text()
    assert "#define HEIFGPU_ABI_VERSION 6" in header and "uint32_t in_lut32[3][4096];" in header


# ---- the reader and the builder under sanitizers ------------------------------------
def test_reader_and_builder_under_sanitizers():
    """tests/tone/hdr_driver.cpp (make tone-asan): clli and mdcv at every truncation length,
    extreme field values, the tables over peaks, primaries and depths, as a stand-alone ASan +
    UBSan program in a process of its own."""
    make_emu("tone-asan")
    exe = ROOT / "heif_amd" / "csrc" / "build" / "tone_asan" / "hdr_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ALL OK" and not [l for l in lines if l.startswith("FAILED")]
    assert [l for l in lines if l.startswith("clli ")] == [f"clli {n} {'OK' if n >= 4 else 'E_PARSE'}" for n in range(8)]
    assert [l for l in lines if l.startswith("mdcv ")] == [f"mdcv {n} {'OK' if n >= 24 else 'E_PARSE'}" for n in range(28)]
    assert len([l for l in lines if l.startswith("build ")]) == 12 and all(l.endswith(" OK") for l in lines if l.startswith("build "))
