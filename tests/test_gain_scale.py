"""The scaled gain-map HDR render on the host (no device): heifgpu_gain_average, which runs the
kernel's own accumulation and quotient (kernels/gain_scale.hpp), against the numpy contract of
gain_scale_ref; the identity; the quotient at the top of its range on sums checked with Python
integers; the argument checks of heifgpu_render_batch_gain_scaled, which answer without a
context; the names at the C-ABI; and the header's arithmetic as a stand-alone ASan + UBSan
program against 128-bit arithmetic.  The kernel is in tests/test_gain_scale_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gain_scale_ref
import scale_ref
from conftest import ROOT, make_emu

MAXCODE = 256 * 4095
U32P = ctypes.POINTER(ctypes.c_uint32)
SAN_ENV = dict(ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.fixture(scope="module")
def L():
    from heif_amd import _lib

    return _lib


def average(L, g, window, ow, oh):
    """heifgpu_gain_average of a (H, W) array: (rc, (oh, ow) uint32)."""
    g = np.ascontiguousarray(g, np.uint32)
    sc = L.Scale(ow, oh, *(window or (0, 0, 0, 0)))
    out = np.full((oh, ow), 0xFFFFFFFF, np.uint32)
    rc = L.lib.heifgpu_gain_average(g.ctypes.data_as(U32P), g.shape[1], g.shape[0], ctypes.byref(sc), out.ctypes.data_as(U32P))
    return rc, out


RATIOS = [  # (W, H, window, ow, oh)
    (320, 48, None, 100, 20),          # 3.2 and 2.4
    (320, 48, None, 160, 24),          # 2 : 1
    (61, 41, None, 61, 41),            # identity
    (61, 41, None, 90, 70),            # enlarging
    (61, 41, None, 1, 1),              # -> 1 x 1
    (96, 64, (3, 5, 57, 31), 20, 11),  # odd offset, odd size
    (96, 64, (19, 13, 61, 41), 7, 40),
    (96, 64, (95, 63, 1, 1), 3, 2),    # one code, enlarged
    (1056, 16, None, 31, 2),           # footprints straddling column 512
]


@pytest.mark.parametrize("W,H,window,ow,oh", RATIOS, ids=[f"{r[0]}x{r[1]}-{r[3]}x{r[4]}" for r in RATIOS])
def test_average_equals_the_reference(L, W, H, window, ow, oh):
    rng = np.random.default_rng(W * 7 + ow)
    for top in (MAXCODE, 256 * 255, 700):
        g = rng.integers(0, top + 1, (H, W), dtype=np.int64)
        rc, got = average(L, g, window, ow, oh)
        assert rc == 0
        assert np.array_equal(got, gain_scale_ref.average_codes(g, window, ow, oh)), (top, window)


def test_identity_returns_its_input(L):
    rng = np.random.default_rng(3)
    g = rng.integers(0, MAXCODE + 1, (41, 61), dtype=np.int64)
    rc, got = average(L, g, None, 61, 41)
    assert rc == 0 and np.array_equal(got, g)
    rc, got = average(L, g, (3, 5, 57, 31), 57, 31)
    assert rc == 0 and np.array_equal(got, g[5:36, 3:60])


def exact_average(g, ow, oh):
    """The contract's average of the whole of g in Python integers: (values, largest numerator)."""
    H, W = g.shape
    wx, wy = scale_ref.weights(W, ow), scale_ref.weights(H, oh)
    out, top = np.zeros((oh, ow), np.int64), 0
    rows = [[int(v) for v in r] for r in g]
    for Y in range(oh):
        js = [j for j in range(H) if wy[Y, j]]
        for X in range(ow):
            total = 0
            for j in js:
                r, wj = rows[j], int(wy[Y, j])
                total += wj * sum(int(wx[X, i]) * r[i] for i in range(W) if wx[X, i])
            num = 2 * total + W * H
            top = max(top, num)
            out[Y, X] = num // (2 * W * H)
    return out, top


def test_quotient_is_exact_at_the_top_of_the_range(L):
    """Codes near 256 * 4095 over more than 2^25 positions: the numerators pass 2^46 (where a
    double-precision estimate of the whole quotient, corrected once, is no longer what
    k_render_scaled proves of it) and the column sums 2^32.  The sums are taken in uint64
    (exact: below 2^46) and the numerator and quotient in Python integers; single codes are
    changed between two runs so that an average moves across its rounding boundary."""
    W, H = 8192, 4104
    g = np.empty((H, W), np.uint32)
    moved = 0
    for base, ow, oh in ((MAXCODE, 1, 1), (MAXCODE - 1, 2, 1), (MAXCODE - 255, 1, 2)):
        g[:] = base
        # half the positions of every output pixel one lower: the exact average is base - 1/2, rounded up to base
        g[:, ::2] -= 1
        before = None
        for bump in (0, 1):
            if bump:  # one position lower in every output pixel: now just below the half
                g[7, 11] -= 1
                g[H - 3, W - 5] -= 1
            rc, got = average(L, g, None, ow, oh)
            assert rc == 0
            bh, bw = H // oh, W // ow
            for Y in range(oh):
                for X in range(ow):
                    total = int(g[Y * bh:(Y + 1) * bh, X * bw:(X + 1) * bw].sum(dtype=np.uint64))
                    # (an even split: every weight of the block is ow * oh)
                    num = 2 * total * ow * oh + W * H
                    assert num > 1 << 46, num
                    assert int(got[Y, X]) == num // (2 * W * H), (base, ow, oh, X, Y, bump)
            if bump:
                moved += int((got != before).sum())
            before = got
    assert moved == 5  # every output pixel of the three cases crossed its boundary
    # an uneven split with weights that differ, small enough for Python integers throughout
    rng = np.random.default_rng(9)
    small = (MAXCODE - rng.integers(0, 300, (37, 53))).astype(np.int64)
    want, _ = exact_average(small, 4, 3)
    rc, got = average(L, small, None, 4, 3)
    assert rc == 0 and np.array_equal(got, want)


def test_column_sum_above_32_bits(L):
    """16 x 4224 codes near the top to 2 x 1: a column's sum of g passes 2^32."""
    rng = np.random.default_rng(5)
    g = (MAXCODE - rng.integers(0, 64, (4224, 16))).astype(np.int64)
    assert int(g[:, 0].sum()) > 1 << 32
    rc, got = average(L, g, None, 2, 1)
    want = [(2 * int(g[:, 8 * X:8 * X + 8].sum()) * 2 + 16 * 4224) // (2 * 16 * 4224) for X in range(2)]
    assert rc == 0 and got[0].tolist() == want
    assert np.array_equal(got, gain_scale_ref.average_codes(g, None, 2, 1))


def test_average_refusals(L):
    g = np.zeros((8, 8), np.uint32)
    INV = L.HEIFGPU_E_INVALID
    assert L.lib.heifgpu_gain_average(None, 8, 8, None, None) == INV

    def refused(scale, w=8, h=8):
        out = np.full((4, 4), 0xFFFFFFFF, np.uint32)
        sc = L.Scale(*scale)
        rc = L.lib.heifgpu_gain_average(g.ctypes.data_as(U32P), w, h, ctypes.byref(sc), out.ctypes.data_as(U32P))
        return rc == INV and bool((out == 0xFFFFFFFF).all())

    for scale in ((4, 4, 0, 0, 9, 8), (4, 4, 8, 0, 1, 1), (4, 4, 0, 0, 4, 0), (0, 4, 0, 0, 0, 0), (4, 65536, 0, 0, 0, 0)):
        assert refused(scale), scale
    assert refused((4, 4, 0, 0, 0, 0), w=0) and refused((4, 4, 0, 0, 0, 0), h=65536)
    g[3, 3] = MAXCODE + 1
    assert refused((4, 4, 0, 0, 0, 0))
    g[3, 3] = MAXCODE
    assert not refused((4, 4, 0, 0, 0, 0))


def test_new_names_are_exported(L):
    for name in ("heifgpu_render_batch_gain_scaled", "heifgpu_gain_average"):
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert L.ABI_VERSION == 6 and L.lib.heifgpu_abi_version() == 6  # new entry points only
    import heif_amd

    assert hasattr(heif_amd.DecodeContext, "render_hdr_scaled")


def test_render_argument_checks_need_no_device(L):
    """Every check of the arguments answers before the context is looked at: with a null
    context a call with good arguments fails on the context, a bad one on that argument."""
    import heif_amd as Hm
    from heif_amd import synth_encoder as S

    f = S.gainmap_heic(S.SynthParams(width=64, height=48), S.SynthParams(width=32, height=24, chroma_format=0), kind="apple",
                       transforms=(S.irot_box(1),))
    base = Hm.HeifImage.parse(f)
    gain = Hm.HeifImage.parse(f, base.gain_map.item_id)
    assert (base.display.out_width, base.display.out_height) == (48, 64)
    t = base.gain_transform(gain, "srgb", "linear", 10, headroom=4.0)
    tpq = base.gain_transform(gain, "srgb", "pq", 10, headroom=4.0)
    imgs, gimgs = (ctypes.c_void_p * 1)(base._h.value), (ctypes.c_void_p * 1)(gain._h.value)
    planes, gplanes = (L.Planes * 1)(), (L.Planes * 1)()
    for c in range(3):
        planes[0].plane[c], planes[0].pitch[c] = 0x1000 * (c + 1), 64  # never read: no launch happens
    gplanes[0].plane[0], gplanes[0].pitch[0] = 0x8000, 32
    surf = (L.Surface * 1)()
    surf[0].pixels = 0x10000

    def call(scale, pitch, fmt=L.PIX_HDR_RGB16F, xf=t, n=1, gpitch=32):
        surf[0].pitch = pitch
        gplanes[0].pitch[0] = gpitch
        sc = (L.Scale * 1)(L.Scale(*scale))
        xfs = (ctypes.c_void_p * 1)(ctypes.addressof(xf) if xf is not None else None)
        rc = L.lib.heifgpu_render_batch_gain_scaled(None, imgs, n, planes, gimgs, gplanes, None, None, fmt, sc, xfs, surf, None)
        return rc, L.last_error()

    INV, UNS = L.HEIFGPU_E_INVALID, L.HEIFGPU_E_UNSUPPORTED
    assert L.lib.heifgpu_render_batch_gain_scaled(None, None, 0, None, None, None, None, None, 4, None, None, None, None) == INV
    for good in ((17, 11, 0, 0, 0, 0), (17, 11, 5, 3, 41, 29), (48, 64, 0, 0, 48, 64), (65535, 65535, 0, 0, 0, 0)):
        rc, msg = call(good, good[0] * 6)
        assert rc == INV and "context" in msg, (good, msg)  # good arguments: only the context is missing
    for bad in ((17, 11, 0, 0, 41, 0), (17, 11, 8, 0, 41, 29), (17, 11, 48, 0, 1, 1), (17, 11, 0, 0, 49, 64)):
        rc, msg = call(bad, 17 * 6)
        assert rc == INV and "window" in msg, (bad, msg)
    for bad in ((0, 11, 0, 0, 0, 0), (17, 65536, 0, 0, 0, 0)):
        rc, msg = call(bad, 1 << 20)
        assert rc == INV and "rendered size" in msg, (bad, msg)
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6 - 2)
    assert rc == INV and "pitch" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 8 - 2, fmt=L.PIX_HDR_RGBA16F)
    assert rc == INV and "pitch" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6, gpitch=31)
    assert rc == INV and "gain plane pitch" in msg
    for fmt in (L.PIX_RGB16, 8):
        rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6, fmt=fmt)
        assert rc == INV and "format" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6, xf=tpq)
    assert rc == INV and "encoding" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6, xf=None)
    assert rc == INV and "null gain transform" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6, fmt=L.PIX_HDR_RGB16PQ, xf=tpq)
    assert rc == INV and "context" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6, n=65536)
    assert rc == INV and "65535" in msg
    base.chroma_upsampling = "bilinear"
    try:
        rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6)
        assert rc == UNS and "bilinear" in msg
    finally:
        base.chroma_upsampling = "replicate"
    # a cropped gain map under the base's m
    cropped = S.gainmap_heic(S.SynthParams(width=64, height=48), S.SynthParams(width=32, height=24, chroma_format=0), kind="apple",
                             transforms=(S.irot_box(1),), gain_transforms=(S.clap_box(16, 1, 16, 1, 0, 1, 0, 1), S.irot_box(1)))
    cg = Hm.HeifImage.parse(cropped, 2)
    gimgs[0] = cg._h.value
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 6)
    assert rc == UNS and "display map" in msg


def test_sums_and_quotient_under_sanitizers():
    """tests/gain_scale/gain_scale_driver.cpp (make gain-scale-asan): the split sums and the
    two-step quotient of kernels/gain_scale.hpp over the whole stated range, numerators up to
    2^54 and denominators up to 2^33, against 128-bit arithmetic, as a stand-alone ASan + UBSan
    program in a process of its own."""
    make_emu("gain-scale-asan")
    exe = ROOT / "heif_amd" / "csrc" / "build" / "gain_scale_asan" / "gain_scale_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={**os.environ, **SAN_ENV})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and "GAIN SCALE OK" in out, out[-2000:]
