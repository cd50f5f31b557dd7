"""The scaled render on the host (no device): heifgpu_scale_fit against the
fractions of scale_ref.fit, the checker itself (scale_ref.area_average against
the formula of include/heifgpu.h written out in Python integers), the argument
checks of heifgpu_render_batch_scaled, and the new names at the C-ABI
boundary.  The kernel is in tests/test_scale_gpu.py."""
import ctypes
import itertools

import numpy as np
import pytest

import scale_ref

MODES = ("stretch", "contain", "cover")


def lib_fit(dw, dh, bw, bh, mode):
    from heif_amd import _lib

    d = _lib.DisplayInfo(out_width=dw, out_height=dh)
    s = _lib.Scale(7, 7, 7, 7, 7, 7)
    rc = _lib.lib.heifgpu_scale_fit(ctypes.byref(d), bw, bh, _lib.FIT_MODES[mode] if isinstance(mode, str) else mode,
                                    ctypes.byref(s))
    return rc, (s.out_width, s.out_height, s.x, s.y, s.width, s.height)


SIDES = (1, 2, 3, 24, 67, 130, 224, 512, 3024, 4032, 65535)


def test_fit_against_fractions():
    n = 0
    for dw, dh, bw, bh in itertools.product(SIDES, SIDES, (1, 2, 37, 224, 512, 5000, 65535), (1, 3, 19, 224, 384, 65535)):
        for mode in MODES:
            rc, got = lib_fit(dw, dh, bw, bh, mode)
            want = scale_ref.fit(dw, dh, bw, bh, mode)
            assert rc == 0 and got == want, (dw, dh, bw, bh, mode, got, want)
            ow, oh, x, y, w, h = got
            assert ow >= 1 and oh >= 1
            if mode == "cover":  # a window of the box's aspect inside the picture, centred
                assert 1 <= w <= dw and 1 <= h <= dh and x + w <= dw and y + h <= dh and (w == dw or h == dh)
                assert abs((dw - w) - 2 * x) <= 1 and abs((dh - h) - 2 * y) <= 1
            if mode == "contain":
                assert ow <= bw and oh <= bh and (ow == bw or oh == bh)
            n += 1
    assert n > 10000


def test_fit_known_answers():
    # halfmoonbay is displayed 3024 x 4032
    assert lib_fit(3024, 4032, 224, 224, "cover") == (0, (224, 224, 0, 504, 3024, 3024))
    assert lib_fit(3024, 4032, 512, 512, "contain") == (0, (384, 512, 0, 0, 0, 0))
    assert lib_fit(3024, 4032, 512, 384, "stretch") == (0, (512, 384, 0, 0, 0, 0))
    # equal aspects: the whole picture either way
    assert lib_fit(4032, 3024, 512, 384, "cover") == (0, (512, 384, 0, 0, 4032, 3024))
    assert lib_fit(4032, 3024, 512, 384, "contain") == (0, (512, 384, 0, 0, 0, 0))
    # a box larger than the picture enlarges
    assert lib_fit(41, 29, 64, 48, "contain") == (0, (64, 45, 0, 0, 0, 0))
    # one-pixel sides; the rounded side never drops to zero
    assert lib_fit(4032, 1, 10, 10, "contain") == (0, (10, 1, 0, 0, 0, 0))
    assert lib_fit(1, 4032, 10, 10, "cover") == (0, (10, 10, 0, 2015, 1, 1))


def test_fit_rejects():
    from heif_amd import _lib

    for bw, bh, mode in ((0, 5, 0), (5, 0, 1), (0, 0, 2), (5, 5, 3), (5, 5, 0xFFFFFFFF)):
        rc, got = lib_fit(64, 48, bw, bh, mode)
        assert rc == _lib.HEIFGPU_E_INVALID and got == (7,) * 6, (bw, bh, mode)  # nothing written
    assert _lib.lib.heifgpu_scale_fit(None, 5, 5, 0, ctypes.byref(_lib.Scale())) == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_scale_fit(ctypes.byref(_lib.DisplayInfo(out_width=4, out_height=4)), 5, 5, 0,
                                      None) == _lib.HEIFGPU_E_INVALID
    with pytest.raises(ValueError):
        scale_ref.fit(4, 4, 0, 4, "cover")


# ---- the checker ------------------------------------------------------------
def literal(D, window, ow, oh):
    """include/heifgpu.h's formula in Python integers, one output sample at a time."""
    cx, cy, cw, ch = window
    out = np.zeros((oh, ow, D.shape[2]), D.dtype)
    for Y in range(oh):
        wy = [max(0, min((j + 1) * oh, (Y + 1) * ch) - max(j * oh, Y * ch)) for j in range(ch)]
        for X in range(ow):
            wx = [max(0, min((i + 1) * ow, (X + 1) * cw) - max(i * ow, X * cw)) for i in range(cw)]
            for c in range(D.shape[2]):
                acc = sum(wy[j] * wx[i] * int(D[cy + j, cx + i, c]) for j in range(ch) if wy[j] for i in range(cw) if wx[i])
                out[Y, X, c] = (2 * acc + cw * ch) // (2 * cw * ch)
    return out


@pytest.fixture(scope="module")
def picture():
    return np.random.default_rng(5).integers(0, 256, (29, 41, 3), dtype=np.uint8)


@pytest.mark.parametrize("window, ow, oh", [((0, 0, 41, 29), 17, 11), ((5, 3, 30, 20), 7, 20), ((1, 2, 13, 9), 64, 48),
                                            ((0, 0, 41, 29), 1, 1), ((40, 28, 1, 1), 3, 2)])
def test_checker_is_the_formula(picture, window, ow, oh):
    assert np.array_equal(scale_ref.area_average(picture, window, ow, oh), literal(picture, window, ow, oh))


def test_checker_identity_returns_the_window(picture):
    assert np.array_equal(scale_ref.area_average(picture, (5, 3, 30, 20), 30, 20), picture[3:23, 5:35])
    assert np.array_equal(scale_ref.area_average(picture, None, 41, 29), picture)


def test_checker_integer_ratio_is_the_rounded_block_mean(picture):
    win = picture[1:25, 2:38].astype(np.int64)  # 36 x 24 -> 12 x 6: blocks of 3 x 4
    s = win.reshape(6, 4, 12, 3, 3).sum(axis=(1, 3))
    assert np.array_equal(scale_ref.area_average(picture, (2, 1, 36, 24), 12, 6), (2 * s + 12) // 24)
    # round half up: a 2 x 2 block of 0, 0, 1, 1 is 1, not 0
    half = np.array([[0, 0], [1, 1]], np.uint8)[..., None]
    assert scale_ref.area_average(half, None, 1, 1)[0, 0, 0] == 1


@pytest.mark.parametrize("c, o", [(41, 17), (29, 11), (13, 64), (130, 65), (130, 130), (72, 1), (1, 5), (3024, 224)])
def test_checker_weights_sum(c, o):
    w = scale_ref.weights(c, o)
    assert w.shape == (o, c) and (w >= 0).all()
    assert (w.sum(axis=1) == c).all()  # every output sample covers c units
    assert (w.sum(axis=0) == o).all()  # every source sample is handed out whole


def test_checker_sum_above_32_bits():
    """A 12-bit megapixel: acc passes 2^32 and the checker neither wraps nor rounds."""
    D = np.full((1024, 1536, 1), 4095, np.uint16)
    assert 4095 * 1024 * 1536 > 1 << 32
    assert (scale_ref.area_average(D, None, 1, 1) == 4095).all() and (scale_ref.area_average(D, None, 3, 2) == 4095).all()
    D[::2, 1::2] = 0
    D[1::2, ::2] = 0  # a checkerboard of period 2: the mean is 2047.5
    assert (scale_ref.area_average(D, None, 1, 1) == 2048).all() and (scale_ref.area_average(D, None, 3, 2) == 2048).all()


# ---- the C-ABI boundary -------------------------------------------------------
def test_new_names_are_exported():
    from heif_amd import _lib

    for name in ("heifgpu_scale_fit", "heifgpu_render_batch_scaled"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert ctypes.sizeof(_lib.Scale) == 24
    assert _lib.ABI_VERSION == 6 and _lib.lib.heifgpu_abi_version() == 6  # new entry points only
    assert (_lib.FIT_STRETCH, _lib.FIT_CONTAIN, _lib.FIT_COVER) == (0, 1, 2)


def test_render_scaled_argument_checks_need_no_device():
    """Every check of the arguments answers before the context is looked at: with
    a null context a call with good arguments fails on the context, a call with
    a bad one on that argument (the surfaces and planes are never touched)."""
    import heif_amd as Hm
    from heif_amd import _lib, synth_encoder as S

    L = _lib.lib
    assert L.heifgpu_render_batch_scaled(None, None, 0, None, None, None, 0, None, None, None) == _lib.HEIFGPU_E_INVALID
    img = Hm.HeifImage.parse(S.display_heic(S.SynthParams(width=64, height=48), transforms=(S.irot_box(1),)))
    d = img.display
    assert (d.out_width, d.out_height) == (48, 64)
    imgs = (ctypes.c_void_p * 1)(img._h.value)
    planes = (_lib.Planes * 1)()
    for c in range(3):
        planes[0].plane[c], planes[0].pitch[c] = 0x1000 * (c + 1), 64  # never read: no launch happens
    surf = (_lib.Surface * 1)()
    surf[0].pixels = 0x10000

    def call(scale, pitch, fmt=0, n=1):
        surf[0].pitch = pitch
        sc = (_lib.Scale * 1)(_lib.Scale(*scale))
        rc = L.heifgpu_render_batch_scaled(None, imgs, n, planes, None, None, fmt, sc, surf, None)
        return rc, _lib.last_error()

    INV = _lib.HEIFGPU_E_INVALID
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 3)
    assert rc == INV and "context" in msg  # good arguments: only the context is missing
    rc, msg = call((17, 11, 5, 3, 41, 29), 51)
    assert rc == INV and "context" in msg
    rc, msg = call((17, 11, 0, 0, 48, 64), 51)
    assert rc == INV and "context" in msg  # the whole picture, spelt out
    for bad in ((17, 11, 0, 0, 41, 0), (17, 11, 0, 0, 0, 29), (17, 11, 8, 0, 41, 29), (17, 11, 0, 36, 41, 29),
                (17, 11, 48, 0, 1, 1), (17, 11, 0, 0, 49, 64), (17, 11, 0xFFFFFFFF, 0, 2, 2)):
        rc, msg = call(bad, 51)
        assert rc == INV and "window" in msg, (bad, msg)
    for bad in ((0, 11, 0, 0, 0, 0), (17, 0, 0, 0, 0, 0), (65536, 11, 0, 0, 0, 0), (17, 65536, 0, 0, 0, 0)):
        rc, msg = call(bad, 1 << 20)
        assert rc == INV and "rendered size" in msg, (bad, msg)
    rc, msg = call((65535, 65535, 0, 0, 0, 0), 65535 * 3)
    assert rc == INV and "context" in msg  # the largest legal size
    rc, msg = call((17, 11, 0, 0, 0, 0), 50)
    assert rc == INV and "pitch" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 17 * 8 - 2, fmt=_lib.PIX_RGBA16)
    assert rc == INV and "pitch" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 51, fmt=4)
    assert rc == INV and "format" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 51, n=65536)
    assert rc == INV and "65535" in msg
