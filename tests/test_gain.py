"""The gain-map HDR render on the host (no device): what a file says of its gain map, the
'tmap' payload's fields and refusals, the tables against the float64 rules of gain_ref,
heifgpu_gain_apply and heifgpu_gain_sample (the functions the kernel runs) against gain_ref's
numpy formula exactly, the properties of the stage, its accuracy against the unquantised
float64 model, the ABI structs, the argument checks of heifgpu_render_batch_gain, which
answer without a context, and the reader and builder as a stand-alone ASan + UBSan
program.  The kernel is in tests/test_gain_gpu.py."""
import ctypes
import subprocess

import numpy as np
import pytest

import color_ref
import gain_ref
from conftest import ROOT, make_emu

E_INVALID, E_PARSE, E_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def H():
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def S():
    from heif_amd import synth_encoder

    return synth_encoder


def pair(H, S, kind="iso", tmap=None, gain_bits=8, bits=8, colr=None):
    """(base image, gain image) of a small synthetic file."""
    f = S.gainmap_heic(S.SynthParams(width=32, height=16, bit_depth=bits),
                       S.SynthParams(width=16, height=16, chroma_format=0, bit_depth=gain_bits), kind=kind, tmap=tmap,
                       colr=colr)
    base = H.HeifImage.parse(f)
    return base, H.HeifImage.parse(f, base.gain_map.item_id)


def apply_lib(t, rgb, gq):
    from heif_amd import _lib

    src = np.ascontiguousarray(rgb, np.uint16).reshape(-1, 3)
    g = np.ascontiguousarray(gq, np.uint32).reshape(-1)
    out = np.empty_like(src)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    _lib.check(_lib.lib.heifgpu_gain_apply(ctypes.byref(t), src.ctypes.data_as(u16p),
                                           g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(src),
                                           out.ctypes.data_as(u16p)))
    return out


def sample_lib(G, bits, W, Hh):
    from heif_amd import _lib

    G = np.ascontiguousarray(G, np.uint8 if bits == 8 else np.uint16)
    out = np.empty((Hh, W), np.uint32)
    _lib.check(_lib.lib.heifgpu_gain_sample(G.ctypes.data_as(ctypes.c_void_p), G.shape[1], G.shape[0], G.strides[0], bits, W,
                                            Hh, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
    return out.astype(np.int64)


def lattice(bits, gain_bits, seed):
    """Codes and gain codes: the corners, every residue f = g & 255, the last index, random."""
    rng = np.random.default_rng(seed)
    maxv, gmax = (1 << bits) - 1, 256 * ((1 << gain_bits) - 1)
    codes = np.array([0, 1, 2, maxv // 3, maxv // 2, maxv - 1, maxv])
    rgb = np.array([(a, b, c) for a in codes for b in codes for c in codes])
    gq = np.concatenate([np.arange(256) + 256 * 7, np.arange(gmax - 256, gmax + 1), [0, 1, 255, 256, gmax // 2]])
    R = np.concatenate([np.repeat(rgb, 8, axis=0), rng.integers(0, maxv + 1, (4000, 3))])
    Gq = np.concatenate([np.tile(gq[:: max(1, len(gq) // 8)][:8], len(rgb)), rng.integers(0, gmax + 1, 4000)])
    # every residue and the last index against a few colours
    R = np.concatenate([R, np.tile(rgb[[0, 171, 342]], (len(gq), 1))])
    Gq = np.concatenate([Gq, np.repeat(gq, 3)])
    return R, Gq


# ---- what the files say ----------------------------------------------------------
def test_halfmoonbay_gain_map(H):
    data = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    gm = H.HeifImage.parse(data).gain_map
    assert (gm.kind, gm.item_id, gm.status) == ("apple", 52, 0)
    gi = H.HeifImage.parse(data, gm.item_id).info
    assert (gi.width, gi.height, gi.bit_depth, gi.chroma_format_idc) == (2016, 1512, 8, 0)


def test_tmap_fields(H, S):
    tm = S.tmap_box(base_headroom=(1, 4), alternate_headroom=(7, 2), gain_min=(-3, 8), gain_max=(5, 2), gamma=(3, 2),
                    base_offset=(1, 64), alternate_offset=(-1, 128), writer_version=7)
    base, gain = pair(H, S, tmap=tm)
    gm = base.gain_map
    assert (gm.kind, gm.item_id, gm.status, gm.version, gm.minimum_version, gm.writer_version) == ("iso", 2, 0, 0, 0, 7)
    assert (gm.multichannel, gm.use_base_colour_space) == (False, True)
    assert (gm.base_headroom, gm.alternate_headroom, gm.gain_min, gm.gain_max, gm.gamma, gm.base_offset,
            gm.alternate_offset) == (0.25, 3.5, -0.375, 2.5, 1.5, 1 / 64, -1 / 128)
    assert gain.gain_map is None and gain.info.chroma_format_idc == 0
    # a tmap wins over Apple's auxiliary image; without either there is none
    both, _ = pair(H, S, kind="both")
    assert both.gain_map.kind == "iso" and both.info.aux_item_id == 2
    assert pair(H, S, kind="apple")[0].gain_map.kind == "apple"
    assert H.HeifImage.parse(S.display_heic(S.SynthParams(width=16, height=16))).gain_map is None
    # idat-free multi-extent data reads the same
    f = S.gainmap_heic(S.SynthParams(width=32, height=16), S.SynthParams(width=16, height=16, chroma_format=0), kind="iso",
                       tmap=tm, layout=S.BoxLayout(extents=3))
    assert H.HeifImage.parse(f).gain_map.gamma == 1.5


REFUSALS = [
    ("truncated", dict(truncate=61), E_PARSE),
    ("empty", dict(truncate=0), E_PARSE),
    ("zero denominator", dict(gamma=(1, 0)), E_PARSE),
    ("zero headroom denominator", dict(alternate_headroom=(2, 0)), E_PARSE),
    ("multichannel", dict(multichannel=True), E_UNSUPPORTED),
    ("alternate colour space", dict(use_base_colour_space=False), E_UNSUPPORTED),
    ("HDR base", dict(base_headroom=2.0, alternate_headroom=0.0), E_UNSUPPORTED),
    ("equal headrooms", dict(base_headroom=1.0, alternate_headroom=1.0), E_UNSUPPORTED),
    ("gamma 0", dict(gamma=0.0), E_UNSUPPORTED),
    ("max above 8", dict(gain_max=8.5), E_UNSUPPORTED),
    ("min below -8", dict(gain_min=-8.5), E_UNSUPPORTED),
    ("headroom above 8", dict(alternate_headroom=9.0), E_UNSUPPORTED),
    ("minimum_version 1", dict(minimum_version=1), E_UNSUPPORTED),
    ("version 1", dict(version=1), E_UNSUPPORTED),
]


@pytest.mark.parametrize("name,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_tmap_refusals_at_transform_time(H, S, name, kw, code):
    base, gain = pair(H, S, tmap=S.tmap_box(**kw))  # the file parses
    assert base.gain_map.kind == "iso" and base.gain_map.status == code
    with pytest.raises(H.HeifGpuError) as e:
        base.gain_transform(gain)
    assert e.value.code == code
    assert isinstance(e.value, H.UnsupportedError) == (code == E_UNSUPPORTED)


def test_apple_needs_headroom_and_other_arguments(H, S):
    base, gain = pair(H, S, kind="apple")
    for hr in (None, 0.5, 300.0):
        with pytest.raises(H.HeifGpuError) as e:
            base.gain_transform(gain, headroom=hr)
        assert e.value.code == E_INVALID
    assert base.gain_transform(gain, headroom=1.0).kind == 1
    with pytest.raises(H.HeifGpuError) as e:
        base.gain_transform(gain, encoding="pq", pq_bits=11, headroom=2.0)
    assert e.value.code == E_INVALID
    # a PQ base is refused as the colour-managed render refuses it
    pq_base, pq_gain = pair(H, S, colr=S.nclx_box(9, 16, 9, False))
    with pytest.raises(H.UnsupportedError):
        pq_base.gain_transform(pq_gain)


def test_abi_structs(H):
    from heif_amd import _lib

    assert ctypes.sizeof(_lib.GainInfo) == 32 + 7 * 8
    assert ctypes.sizeof(_lib.GainTransform) == 72 + 24 + 3 * 4096 * 2 + 4098 * 4 + 642 * 4
    assert _lib.GainTransform.in_lut.offset == 96 and _lib.GainTransform.weight.offset == 72


# ---- the tables ------------------------------------------------------------------
@pytest.mark.parametrize("gain_bits", [8, 10, 12])
def test_tables_follow_the_float64_rules(H, S, gain_bits):
    tm = S.tmap_box(base_headroom=0.5, alternate_headroom=3.0, gain_min=-0.75, gain_max=2.75, gamma=1.6,
                    base_offset=1 / 64, alternate_offset=1 / 32)
    base, gain = pair(H, S, tmap=tm, gain_bits=gain_bits)
    ng = (1 << gain_bits) + 1
    for dh in (None, 4.0, 1.0):
        t = base.gain_transform(gain, "bt2020", "pq", 12, display_headroom=dh, sdr_white=100.0)
        w = gain_ref.weight(dh, 0.5, 3.0)
        assert t.weight == pytest.approx(w) and (t.kind, t.gain_bits, t.pq_bits) == (2, gain_bits, 12)
        T = np.ctypeslib.as_array(t.T)[:ng].astype(np.float64)
        assert np.abs(T - gain_ref.T_iso(gain_bits, w, -0.75, 2.75, 1.6)).max() <= 1
        assert T[-1] == T[-2]
        assert (t.k_b, t.k_a) == (int(gain_ref.rhu(65535 / 64)), int(gain_ref.rhu(65535 / 32)))
        E = np.ctypeslib.as_array(t.E)[:gain_ref.E_ENTRIES].astype(np.float64)
        assert np.abs(E - gain_ref.E_table(12, 100.0)).max() <= 1
    abase, again = pair(H, S, kind="apple", gain_bits=gain_bits)
    for hr, dh in ((4.0, None), (8.0, 3.0), (2.0, 0.5)):
        t = abase.gain_transform(again, headroom=hr, display_headroom=dh)
        T = np.ctypeslib.as_array(t.T)[:ng].astype(np.float64)
        assert np.abs(T - gain_ref.T_apple(gain_bits, gain_ref.apple_hr(hr, dh))).max() <= 1
        assert (t.k_b, t.k_a, t.kind) == (0, 0, 1) and T[0] == 65536
    # sdr_white defaults to 203; the last node saturates at 10000 cd/m2
    t = abase.gain_transform(again, encoding="pq", pq_bits=16, headroom=2.0, sdr_white=0.0)
    E = np.ctypeslib.as_array(t.E)[:gain_ref.E_ENTRIES].astype(np.float64)
    assert np.abs(E - gain_ref.E_table(16, 203.0)).max() <= 1 and E[-1] == 256 * 65535 and t.sdr_white == 203.0


def test_bt2020_matrix_and_the_existing_destinations(H, S):
    base, gain = pair(H, S, kind="apple")
    for cs in ("srgb", "display-p3"):
        assert list(base.gain_transform(gain, cs, headroom=2.0).m) == list(base.color_transform(cs, 8).m)
    m = np.array(list(base.gain_transform(gain, "bt2020", headroom=2.0).m)).reshape(3, 3)
    assert (m.sum(axis=1) == 16384).all()
    # sRGB primaries inside BT.2020 (BT.2087's matrix, through D50 and back: a few units of Q14)
    want = np.array([[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]])
    assert np.abs(m / 16384.0 - want).max() < 2e-3
    own, g2 = pair(H, S, kind="apple", colr=S.nclx_box(9, 13, 9, False))
    assert list(own.gain_transform(g2, "bt2020", headroom=2.0).m) == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]
    with pytest.raises(ValueError):
        base.color_transform("bt2020", 8)  # the colour-managed render keeps refusing it


# ---- the formula -----------------------------------------------------------------
CASES = [  # (kind, bits, gain_bits, colorspace, encoding, pq_bits, tmap kwargs or headroom)
    ("iso", 8, 8, "display-p3", "linear", 0, dict(gain_min=-1.0, gain_max=3.0, gamma=1.4, base_offset=1 / 64, alternate_offset=1 / 8)),
    ("iso", 10, 10, "bt2020", "pq", 10, dict(gain_min=-0.5, gain_max=2.0, gamma=0.8, base_offset=1 / 64, alternate_offset=1 / 64)),
    ("iso", 12, 8, "srgb", "pq", 16, dict(gain_min=0.0, gain_max=8.0, alternate_headroom=8.0, base_offset=0.0, alternate_offset=0.0)),
    ("apple", 8, 8, "bt2020", "pq", 12, 4.0),
    ("apple", 8, 12, "srgb", "linear", 0, 256.0),
]


def make_case(H, S, case, colr=None):
    kind, bits, gain_bits, cs, enc, pq_bits, arg = case
    base, gain = pair(H, S, kind=kind, tmap=S.tmap_box(**arg) if kind == "iso" else None, gain_bits=gain_bits, bits=bits,
                      colr=colr)
    return base.gain_transform(gain, cs, enc, pq_bits or 10, headroom=None if kind == "iso" else arg)


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}{c[5] or ''}" for c in CASES])
def test_gain_apply_equals_the_numpy_contract(H, S, case):
    wide = S.icc_box(S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True))
    t = make_case(H, S, case, colr=wide if case[3] == "srgb" else None)
    rgb, gq = lattice(case[1], case[2], 5)
    got = apply_lib(t, rgb, gq)
    assert np.array_equal(got, gain_ref.apply(t, rgb, gq))


def test_every_clamp_binds_somewhere(H, S):
    """From the model alone: H at 0 (k_a > k_b), H' at 0 (a wide-gamut colour into sRGB) and H'
    at 2^24 - 1 (a multiplier of 256 on white) all bind on the lattices above."""
    wide = S.icc_box(S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True))
    seen = dict(h_low=False, h2_low=False, h2_high=False)
    for case in CASES:
        t = make_case(H, S, case, colr=wide if case[3] == "srgb" else None)
        rgb, gq = lattice(case[1], case[2], 5)
        parts = {}
        gain_ref.levels(gain_ref.tables(t), rgb, gq, parts)
        seen["h_low"] |= bool((parts["H"] < 0).any())
        seen["h2_low"] |= bool((parts["H2"] < 0).any())
        seen["h2_high"] |= bool((parts["H2"] > gain_ref.LEVEL_MAX).any())
    assert all(seen.values()), seen


def test_apply_refuses_what_a_render_would(H, S):
    from heif_amd import _lib

    t = make_case(H, S, CASES[0])
    ok = np.array([[1, 2, 3]]), np.array([256 * 255])
    apply_lib(t, *ok)
    for rgb, gq in ((np.array([[256, 0, 0]]), ok[1]), (ok[0], np.array([256 * 255 + 1]))):
        with pytest.raises(H.HeifGpuError) as e:
            apply_lib(t, rgb, gq)
        assert e.value.code == E_INVALID
    for field, value in (("T", (1 << 24) + 1), ("k_a", 16 * 65535 + 1), ("encoding", 2), ("gain_bits", 13)):
        bad = _lib.GainTransform.from_buffer_copy(t)
        if field == "T":
            bad.T[17] = value
        else:
            setattr(bad, field, value)
        with pytest.raises(H.HeifGpuError) as e:
            apply_lib(bad, *ok)
        assert e.value.code == E_INVALID


def test_render_argument_checks_need_no_device(H, S):
    """heifgpu_render_batch_gain with a null context: every check of the arguments answers
    before the context is looked at, so a call with good arguments fails on the context and
    one with a bad argument on that argument."""
    from heif_amd import _lib as L

    base, gain = pair(H, S, kind="apple")
    t = base.gain_transform(gain, "srgb", "linear", 10, headroom=4.0)
    imgs, gimgs = (ctypes.c_void_p * 1)(base._h.value), (ctypes.c_void_p * 1)(gain._h.value)
    planes, gplanes = (L.Planes * 1)(), (L.Planes * 1)()
    for c in range(3):
        planes[0].plane[c], planes[0].pitch[c] = 0x1000 * (c + 1), 32  # never read: no launch happens
    gplanes[0].plane[0], gplanes[0].pitch[0] = 0x8000, 16
    surf = (L.Surface * 1)()
    surf[0].pixels, surf[0].pitch = 0x10000, base.display.out_width * 6

    def call(fmt=L.PIX_HDR_RGB16F, n=1, gimgs=gimgs, xf=t):
        xfs = (ctypes.c_void_p * 1)(ctypes.addressof(xf) if xf is not None else None)
        rc = L.lib.heifgpu_render_batch_gain(None, imgs, n, planes, gimgs, gplanes, None, None, fmt, xfs, surf, None)
        return rc, L.last_error()

    rc, msg = call()
    assert rc == E_INVALID and "context" in msg, msg  # good arguments: only the context is missing
    for kw, word in ((dict(fmt=L.PIX_RGB16), "format"), (dict(fmt=8), "format"), (dict(n=65536), "65535"),
                     (dict(gimgs=(ctypes.c_void_p * 1)(None)), "null image"), (dict(xf=None), "null gain transform")):
        rc, msg = call(**kw)
        assert rc == E_INVALID and word in msg and "context" not in msg, (kw, msg)


SAMPLER = [(320, 48, 160, 24, 8), (96, 64, 40, 24, 8), (33, 17, 33, 17, 10), (40, 24, 96, 64, 12), (7, 5, 1, 1, 8),
           (4032, 2, 2016, 1, 8)]


@pytest.mark.parametrize("W,Hh,Wg,Hg,bits", SAMPLER)
def test_sampler_equals_the_integer_contract(H, W, Hh, Wg, Hg, bits):
    rng = np.random.default_rng(W * 7 + Wg)
    G = rng.integers(0, 1 << bits, (Hg, Wg))
    G[0, 0], G[-1, -1] = (1 << bits) - 1, 0
    got = sample_lib(G, bits, W, Hh)
    assert np.array_equal(got, gain_ref.sample_map(G, W, Hh))
    if (Wg, Hg) == (W, Hh):
        assert np.array_equal(got, 256 * G)  # a same-size map gives the sample itself


def test_sampler_borders_and_residues():
    # 2:1 binds both border clamps; the ratios 2.4 and 2.67 walk many residues fx
    assert gain_ref.borders_bind(320, 160) == (True, True) and gain_ref.borders_bind(48, 24) == (True, True)
    assert gain_ref.borders_bind(96, 40) == (True, True) and gain_ref.borders_bind(64, 24) == (True, True)
    # a same-size map: only the second tap of the last sample is clamped, and its weight is 0
    assert gain_ref.borders_bind(33, 33) == (False, True) and (gain_ref.taps(33, 33)[2] == 0).all()
    assert len(set(gain_ref.taps(96, 40)[2].tolist())) >= 12 and len(set(gain_ref.taps(64, 24)[2].tolist())) >= 8
    # the library's sampler where the clamps bind: the outermost base columns and rows read the
    # map's edge samples alone, whatever lies next to them
    for W, Wg in ((320, 160), (96, 40)):
        G = np.random.default_rng(W).integers(0, 256, (24, Wg))
        got = sample_lib(G, 8, W, 24)  # as many rows as the map: no interpolation in y
        assert np.array_equal(got[:, 0], 256 * G[:, 0]) and np.array_equal(got[:, -1], 256 * G[:, -1])
        gotT = sample_lib(G.T, 8, 24, W)
        assert np.array_equal(gotT[0], 256 * G[:, 0]) and np.array_equal(gotT[-1], 256 * G[:, -1])


def test_oversized_tmap_item_reads_as_damaged(H, S):
    """A 'tmap' item above 64 KiB is not copied at parse: the file parses, a transform is E_PARSE;
    a payload with bytes behind its fields, up to that size, is read."""
    good = S.tmap_box()
    base, gain = pair(H, S, tmap=good + bytes(65536 - len(good)))
    assert base.gain_map.status == 0 and base.gain_map.alternate_headroom == 2.0
    base, gain = pair(H, S, tmap=good + bytes(65537 - len(good)))
    assert base.gain_map.kind == "iso" and base.gain_map.status == E_PARSE
    with pytest.raises(H.HeifGpuError) as e:
        base.gain_transform(gain)
    assert e.value.code == E_PARSE


def test_no_headroom_is_the_base_picture(H, S):
    """display_headroom at or below the base headroom: M = 2^16 everywhere, and with equal
    offsets the linear output is in_lut / 65535 (nclx sRGB into sRGB: the identity matrix)."""
    tm = S.tmap_box(base_headroom=1.0, alternate_headroom=3.0, gain_min=-1.0, gain_max=3.0, base_offset=1 / 16,
                    alternate_offset=1 / 16)
    base, gain = pair(H, S, tmap=tm)
    for dh in (2.0, 1.5):
        t = base.gain_transform(gain, "srgb", display_headroom=dh)
        assert t.weight == 0.0 and (np.ctypeslib.as_array(t.T)[:257] == 65536).all()
        rgb, gq = lattice(8, 8, 9)
        L = np.ctypeslib.as_array(t.in_lut[0])[:256].astype(np.int64)
        assert (np.ctypeslib.as_array(t.in_lut[1])[:256] == L).all()
        assert np.array_equal(apply_lib(t, rgb, gq), gain_ref.encode_linear(L[rgb]))


@pytest.mark.parametrize("case", CASES[:4], ids=[c[0] + c[4] + str(c[1]) for c in CASES[:4]])
def test_output_is_monotone_in_the_gain(H, S, case):
    t = make_case(H, S, case)
    gmax = 256 * ((1 << case[2]) - 1)
    gq = np.arange(0, gmax + 1, 3 if gmax > 70000 else 1)
    for code in (1, (1 << case[1]) // 3, (1 << case[1]) - 1):
        out = apply_lib(t, np.full((len(gq), 3), code), gq).astype(np.int64)  # (binary16 bits of non-negatives order as integers)
        assert (np.diff(out, axis=0) >= 0).all() and (out[-1] > out[0]).all()


# ---- the accuracy ----------------------------------------------------------------
# The integer path against gain_ref's float64 model (sRGB source into Display P3, ISO rule with
# min -1, max 3 stops, gamma 1.4, offsets 1/64; 8-bit codes and map): the largest difference
# over the lattice, measured and rounded up to 0.1.  Linear: in units of 1 / 65535
# of SDR white (levels reach 8 x 65535), before the half-float rounding.  PQ: in codes at depth P.
# "all": the whole lattice.  "g >= 2": gain codes of two map codes and more.  The difference
# between the two is the contract's own: T is linear between map codes, and below map code 1
# (v / maxg)^(1 / gamma) with gamma > 1 has an unbounded slope, 0.6 % of the multiplier at g = 0.3
# codes.  E's own share (the PQ code of the integer level against the table) is 0.51 code at P = 10 (0.55 at 12, 1.33 at
# 16, where 32 nodes per octave show), so widening E would not bring the first row below one code at P = 10; the second row is.
ACCURACY = {"all": {"linear": 191.0, 10: 1.6, 12: 5.8, 16: 96.3},
            "g >= 2": {"linear": 9.4, 10: 0.8, 12: 3.4, 16: 49.8}}


def test_accuracy_against_the_float64_model(H, S):
    kw = dict(gain_min=-1.0, gain_max=3.0, gamma=1.4, alternate_headroom=3.0, base_offset=1 / 64, alternate_offset=1 / 64)
    base, gain = pair(H, S, tmap=S.tmap_box(**kw))
    rgb, gq = lattice(8, 8, 11)
    trc = [color_ref.srgb_decode] * 3
    rest = gq >= 512
    found = {"all": {}, "g >= 2": {}}
    for key, pq_bits in (("linear", 0), (10, 10), (12, 12), (16, 16)):
        t = base.gain_transform(gain, "display-p3", "pq" if pq_bits else "linear", pq_bits or 10)
        tb = gain_ref.tables(t)
        lv = gain_ref.levels(tb, rgb, gq)
        model = gain_ref.model_levels(trc, tb["m"] / 16384.0, lambda x: gain_ref.log2_gain_iso(x, 1.0, -1.0, 3.0, 1.4), 1 / 64,
                                      1 / 64, 255, 255, rgb, gq / 256.0)
        if pq_bits:
            err = np.abs(gain_ref.encode_pq(tb["E"], lv).astype(np.float64) - gain_ref.model_pq(model, pq_bits))
            assert np.abs(gain_ref.encode_pq(tb["E"], lv) - gain_ref.model_pq(lv.astype(np.float64), pq_bits)).max() < {10: 0.52, 12: 0.56, 16: 1.4}[pq_bits]
        else:
            err = np.abs(lv - model)
        found["all"][key], found["g >= 2"][key] = float(err.max()), float(err[rest].max())
    print("gain accuracy (max abs):", found)
    for part, bounds in ACCURACY.items():
        for key, bound in bounds.items():
            assert found[part][key] <= bound, found
    assert found["g >= 2"][10] < 1.0  # below one code at P = 10 away from the first map code


def test_reader_builder_and_formula_under_sanitizers():
    """tests/gain/gain_driver.cpp (make gain-asan): the payload at every truncation length, every
    byte hostile in turn, random payloads, the builds and the formula and sampler at the corners
    of their domains, as a stand-alone ASan + UBSan program in a process of its own."""
    make_emu("gain-asan")
    exe = ROOT / "heif_amd" / "csrc" / "build" / "gain_asan" / "gain_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ALL OK" and not [l for l in lines if l.startswith("FAILED")]
    assert [l for l in lines if l.startswith("tmap ")] == [f"tmap {n} {'OK' if n >= 62 else 'E_PARSE'}" for n in range(63)]
    assert [l for l in lines if l.startswith("multi ")] == ["multi 62 E_PARSE", "multi 141 E_PARSE", "multi 142 E_UNSUPPORTED"]
    builds = [l for l in lines if l.startswith("build ")]
    assert len(builds) == 36 and all(l.endswith(" OK") for l in builds)
    assert "refuse E_INVALID E_INVALID E_INVALID E_INVALID" in lines
