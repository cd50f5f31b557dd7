"""The linear-light scaled render on the host (no device): heifgpu_linear_average_apply, which
runs the functions the kernel runs (kernels/color_xform.hpp), against linear_ref's numpy
restatement of the contract (exactly) and against the float64 model (the accuracy); the
consequences the header states; the extremes of the ranges; the refusals of the two new render
entry points, which answer before a context is looked at; the Python ValueErrors; the exports.
The kernels are in tests/test_linear_gpu.py."""
import ctypes

import numpy as np
import pytest

import color_ref
import linear_ref
import scale_ref

DSTS = ("srgb", "display-p3")
# (picture w, h, window or None, out w, out h): 1 x 1, the window's own size, 2 : 1, a ratio that
# is no integer, an enlargement; the first four read a window at an odd offset of a larger picture
SIZES = [(80, 44, (5, 3, 70, 38), 1, 1), (80, 44, (5, 3, 70, 38), 70, 38), (80, 44, (5, 3, 70, 38), 35, 19),
         (80, 44, (5, 3, 70, 38), 23, 11), (41, 29, None, 64, 45)]
SOURCES = ("p3-para", "bt2020-curv", "srgb-nclx", "bt2020-nclx")


@pytest.fixture(scope="module")
def H():
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def S():
    from heif_amd import synth_encoder

    return synth_encoder


@pytest.fixture(scope="module")
def sources(H, S):
    """name -> (a parsed image of that colour space, what color_ref.Model reads)."""
    p3 = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    bt2020 = S.icc_profile(color_ref.nclx_colorants(9), S.icc_curv((2.2,)), version=2)

    def image(colr):
        return H.HeifImage.parse(S.display_heic(S.SynthParams(width=16, height=16), colr=colr))

    return {"p3-para": (image(S.icc_box(p3)), p3), "bt2020-curv": (image(S.icc_box(bt2020)), bt2020),
            "srgb-nclx": (image(S.nclx_box(1, 13, 1, False)), (1, 13)),
            "bt2020-nclx": (image(S.nclx_box(9, 1, 9, False)), (9, 1))}


def apply_lib(t, D, window, ow, oh):
    """heifgpu_linear_average_apply over a picture (H, W, C) of codes."""
    from heif_amd import _lib

    src = np.ascontiguousarray(D, np.uint16)
    out = np.empty((oh, ow, src.shape[2]), np.uint16)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    win = None if window is None else ctypes.byref(_lib.Rect(*window))
    _lib.check(_lib.lib.heifgpu_linear_average_apply(ctypes.byref(t), src.ctypes.data_as(u16p), src.shape[1], src.shape[0],
                                                     src.shape[2], win, ow, oh, out.ctypes.data_as(u16p)))
    return out


def picture(bits, w, h, channels, seed):
    """Random codes with flat black and white patches: the ends of the tables are read."""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 1 << bits, (h, w, channels), dtype=np.uint16)
    D[: h // 4, : w // 4] = 0
    D[-(h // 4):, -(w // 4):] = (1 << bits) - 1
    return D


# |library - float64 model| in codes over the cases of test_apply_equals_numpy_and_follows_the_float_model,
# measured on the CPU and pinned at the measured value rounded up to the next 0.25 code:
# 0.5736 at 8 bits, 0.9315 at 10, 2.1854 at 12 (each the largest of the four sources; the own-size
# outputs of every case are per-pixel transforms, so these are 5.25's kind of figure on random codes,
# and the 8-bit one stays within 5.25's 1 code).  The yardstick is the float model, never the library.
ACCURACY = {8: 0.75, 10: 1.0, 12: 2.25}
measured = {}


@pytest.mark.parametrize("bits", [8, 10, 12])
@pytest.mark.parametrize("name", SOURCES)
def test_apply_equals_numpy_and_follows_the_float_model(sources, name, bits):
    img, source = sources[name]
    worst = 0.0
    for dst in DSTS:
        t = img.color_transform(dst, bits)
        model = color_ref.Model(source, dst)
        for channels in (3, 4):
            for k, (w, h, window, ow, oh) in enumerate(SIZES):
                D = picture(bits, w, h, channels, 1000 * bits + 10 * k + channels)
                got = apply_lib(t, D, window, ow, oh)
                want = linear_ref.linear_average(t, D, window, ow, oh)
                assert np.array_equal(got, want), (name, dst, bits, channels, k)
                err = np.abs(got[..., :3].astype(np.float64) - linear_ref.model_average(model, bits, D, window, ow, oh)).max()
                worst = max(worst, float(err))
    measured[(name, bits)] = worst
    print(f"linear accuracy {name} at {bits} bits: {worst:.4f} codes")
    assert worst <= ACCURACY[bits], (name, bits, worst)


@pytest.mark.parametrize("bits", [8, 12])
def test_own_size_is_the_per_pixel_transform(sources, bits):
    """Identity at the window's own size: S = cw ch L, so the result is color_ref's per-pixel
    transform of the window; for an identity transform it is the window itself."""
    D = picture(bits, 41, 29, 4, 7)
    window = (3, 2, 33, 25)
    for name in SOURCES:
        for dst in DSTS:
            t = sources[name][0].color_transform(dst, bits)
            got = apply_lib(t, D, window, 33, 25)
            win = D[2:27, 3:36]
            assert np.array_equal(got[..., :3], color_ref.apply(t, win[..., :3])), (name, dst)
            assert np.array_equal(got[..., 3], win[..., 3])
            if t.identity:
                assert np.array_equal(got, win), (name, dst)
    assert sources["srgb-nclx"][0].color_transform("srgb", bits).identity  # (the case above ran)


@pytest.mark.parametrize("bits", [8, 10])
def test_uniform_window_gives_the_per_pixel_result(sources, bits):
    rng = np.random.default_rng(3)
    for name in SOURCES:
        t = sources[name][0].color_transform("srgb", bits)
        for _ in range(8):
            code = rng.integers(0, 1 << bits, 4)
            D = np.broadcast_to(code.astype(np.uint16), (38, 70, 4))
            for ow, oh in ((1, 1), (23, 11), (90, 50)):
                got = apply_lib(t, D, None, ow, oh)
                assert (got[..., :3] == color_ref.apply(t, code[None, :3])[0]).all(), (name, code)
                assert (got[..., 3] == code[3]).all()


@pytest.mark.parametrize("bits", [8, 12])
def test_largest_column_sum(sources, bits):
    """A 65535 x 1 window of all-maxv into one pixel: the weighted sum down the line is
    65535 * 65535, the largest a 32-bit column sum has to hold."""
    maxv = (1 << bits) - 1
    t = sources["p3-para"][0].color_transform("display-p3", bits)
    assert t.identity and t.in_lut[0][maxv] == 65535
    for shape in ((65535, 1, 3), (1, 65535, 3)):
        D = np.full(shape, maxv, np.uint16)
        got = apply_lib(t, D, None, 1, 1)
        assert np.array_equal(got, linear_ref.linear_average(t, D, None, 1, 1))
        assert got.tolist() == [[[maxv] * 3]]


def test_checkerboard_keeps_its_light(sources):
    """A full-range black / white pixel-pitch checkerboard 64 x 64 -> 32 x 32 through the identity
    sRGB transform: half of linear white, which sRGB encodes as 188, where the average of the
    codes is 128."""
    t = sources["srgb-nclx"][0].color_transform("srgb", 8)
    assert t.identity
    yy, xx = np.mgrid[:64, :64]
    D = np.repeat((((yy + xx) & 1) * 255).astype(np.uint16)[..., None], 3, axis=2)
    want = linear_ref.linear_average(t, D, None, 32, 32)
    got = apply_lib(t, D, None, 32, 32)
    assert np.array_equal(got, want)
    coded = scale_ref.area_average(D, None, 32, 32)
    assert (coded == 128).all()
    assert len(np.unique(got)) == 1 and int(got[0, 0, 0]) - 128 > 40 and abs(int(got[0, 0, 0]) - 188) <= 1


def test_apply_refusals(H, S, sources):
    from heif_amd import _lib

    L = _lib.lib
    t = sources["p3-para"][0].color_transform("srgb", 8)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    D = np.zeros((4, 5, 3), np.uint16)
    out = np.zeros((2, 2, 3), np.uint16)

    def call(tt=t, d=D, w=5, h=4, ch=3, win=None, ow=2, oh=2):
        rc = L.heifgpu_linear_average_apply(ctypes.byref(tt), d.ctypes.data_as(u16p), w, h, ch,
                                            None if win is None else ctypes.byref(_lib.Rect(*win)), ow, oh,
                                            out.ctypes.data_as(u16p))
        return rc, _lib.last_error()

    INV = _lib.HEIFGPU_E_INVALID
    assert call()[0] == _lib.HEIFGPU_OK
    assert call(ch=2)[0] == INV and call(ch=5)[0] == INV
    for win in ((0, 0, 6, 4), (5, 0, 1, 1), (0, 0, 0, 3), (2, 2, 4, 1)):
        rc, msg = call(win=win)
        assert rc == INV and "window" in msg, win
    assert call(ow=0)[0] == INV and call(oh=65536)[0] == INV
    bad = D.copy()
    bad[1, 1, 2] = 256
    rc, msg = call(d=bad)
    assert rc == INV and "maxv" in msg
    pq = H.HeifImage.parse(S.display_heic(S.SynthParams(width=16, height=16), colr=S.nclx_box(9, 16, 9, False)))
    hdr = pq.color_transform("srgb", 8, tone_map="bt2390")
    assert hdr.base.tone
    rc, msg = call(tt=hdr.base)
    assert rc == _lib.HEIFGPU_E_UNSUPPORTED and "tone" in msg
    assert not out.any()


def test_render_argument_checks_need_no_device(H, S):
    """The refusals of the two linear entry points answer before the context is looked at: with a
    null context a call with good arguments fails on the context, a call with a bad transform
    array on that (the surfaces and planes are never touched)."""
    from heif_amd import _lib

    L = _lib.lib
    p3 = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    img = H.HeifImage.parse(S.display_heic(S.SynthParams(width=64, height=48, bit_depth=10), colr=S.icc_box(p3)))
    pq = H.HeifImage.parse(S.display_heic(S.SynthParams(width=64, height=48, bit_depth=10), colr=S.nclx_box(9, 16, 9, False)))
    t8, t10, tid = img.color_transform("srgb", 8), img.color_transform("srgb", 10), img.color_transform("display-p3", 8)
    tone = pq.color_transform("srgb", 8, tone_map="bt2390")
    assert tid.identity and tone.base.tone
    planes = (_lib.Planes * 1)()
    for c in range(3):
        planes[0].plane[c], planes[0].pitch[c] = 0x1000 * (c + 1), 128  # never read: no launch happens
    surf = (_lib.Surface * 1)()
    surf[0].pixels, surf[0].pitch = 0x10000, 17 * 8
    tsurf = (_lib.TensorSurface * 1)()
    tsurf[0].data, tsurf[0].stride_c, tsurf[0].stride_y = 0x10000, 17 * 11 * 4, 17 * 4
    sc = (_lib.Scale * 1)(_lib.Scale(17, 11, 0, 0, 0, 0))

    def scaled(image, xf, fmt=0):
        imgs = (ctypes.c_void_p * 1)(image._h.value)
        rc = L.heifgpu_render_batch_scaled_linear(None, imgs, 1, planes, None, None, fmt, sc, xf, surf, None)
        return rc, _lib.last_error()

    def tensor(image, xf, src=0):
        imgs = (ctypes.c_void_p * 1)(image._h.value)
        tf = _lib.TensorFormat(src=src, elem=_lib.ELEM_F32, layout=_lib.LAYOUTS["chw"])
        for c in range(4):
            tf.a[c], tf.b[c] = 1.0, 0.0
        rc = L.heifgpu_render_batch_tensor_linear(None, imgs, 1, planes, None, None, ctypes.byref(tf), sc, None, xf, tsurf,
                                                  None)
        return rc, _lib.last_error()

    def ptrs(t):
        return (ctypes.c_void_p * 1)(None if t is None else ctypes.addressof(t))

    INV, UNS = _lib.HEIFGPU_E_INVALID, _lib.HEIFGPU_E_UNSUPPORTED
    for call in (scaled, tensor):
        for good in (t8, tid):  # an identity transform is a transform here
            rc, msg = call(img, ptrs(good))
            assert rc == INV and "context" in msg, msg
        rc, msg = call(img, ptrs(t10), _lib.PIX_RGB16)
        assert rc == INV and "context" in msg, msg
        rc, msg = call(img, None)
        assert rc == INV and "without transforms" in msg, msg
        rc, msg = call(img, ptrs(None))
        assert rc == INV and "without a transform" in msg, msg
        rc, msg = call(img, ptrs(t10))  # rendered at 8 bits
        assert rc == INV and "depth" in msg, msg
        rc, msg = call(img, ptrs(t8), _lib.PIX_RGBA16)  # rendered at 10
        assert rc == INV and "depth" in msg, msg
        rc, msg = call(pq, ptrs(tone.base))
        assert rc == UNS and "tone" in msg, msg


def test_python_refusals_come_before_any_device_work(H, S):
    ctx = H.DecodeContext.__new__(H.DecodeContext)  # no device behind it: every refusal comes first
    ctx._h = None
    data = S.display_heic(S.SynthParams(width=16, height=16))
    for call in (
        lambda **kw: ctx.render_scaled([], (8, 8), **kw),
        lambda **kw: ctx.render_tensor([], (8, 8), **kw),
        lambda **kw: ctx.render_jpeg([], (8, 8), **kw),
        lambda **kw: H.HeicDecoder.decode_display(data, size=(8, 8), **kw),
        lambda **kw: H.HeicDecoder.decode_tensor(data, (8, 8), **kw),
        lambda **kw: H.HeicDecoder.decode_jpeg(data, size=(8, 8), **kw),
    ):
        with pytest.raises(ValueError, match="colorspace"):
            call(linear=True)
        with pytest.raises(ValueError, match="filter"):
            call(linear=True, colorspace="srgb", filter="bicubic")
        with pytest.raises(ValueError, match="tone_map"):
            call(linear=True, colorspace="srgb", tone_map="bt2390")
    with pytest.raises(ValueError, match="size"):
        ctx.render_jpeg([], linear=True, colorspace="srgb")
    with pytest.raises(ValueError, match="size"):
        H.HeicDecoder.decode_jpeg(data, linear=True, colorspace="srgb")
    with pytest.raises(ValueError, match="size"):
        H.HeicDecoder.decode_display(data, linear=True, colorspace="srgb")


def test_new_names_are_exported():
    from heif_amd import _lib

    for name in ("heifgpu_render_batch_scaled_linear", "heifgpu_render_batch_tensor_linear", "heifgpu_linear_average_apply"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.ABI_VERSION == 6 and _lib.lib.heifgpu_abi_version() == 6  # new entry points only
