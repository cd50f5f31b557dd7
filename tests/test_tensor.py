"""The tensor render on the host (no device): the new names at the C-ABI
boundary, the argument checks of heifgpu_render_batch_tensor (all of them
answer before the context is looked at, so a null context serves), and the
checker tests/tensor_ref.py against bit patterns known by hand.  The kernel is
in tests/test_tensor_gpu.py."""
import ctypes

import numpy as np
import pytest

import tensor_ref


# ---- the C-ABI boundary -------------------------------------------------------
def test_new_names_are_exported():
    from heif_amd import _lib

    assert "heifgpu_render_batch_tensor" in _lib.EXPORTS and hasattr(_lib.lib, "heifgpu_render_batch_tensor")
    assert _lib.ABI_VERSION == 6 and _lib.lib.heifgpu_abi_version() == 6  # new entry points only
    assert ctypes.sizeof(_lib.TensorFormat) == 12 + 32 and ctypes.sizeof(_lib.TensorSurface) == 24
    assert (_lib.ELEM_F32, _lib.ELEM_F16, _lib.ELEM_BF16) == (0, 1, 2)
    assert (_lib.LAYOUT_CHW, _lib.LAYOUT_HWC) == (0, 1)


@pytest.fixture(scope="module")
def caller():
    """call(**changes) -> (rc, message): heifgpu_render_batch_tensor with a null
    context over one 48 x 64 displayed picture; the planes and the tensor are
    addresses that are never touched, because no launch happens."""
    import heif_amd as Hm
    from heif_amd import _lib, synth_encoder as S

    img = Hm.HeifImage.parse(S.display_heic(S.SynthParams(width=64, height=48), transforms=(S.irot_box(1),)))
    assert (img.display.out_width, img.display.out_height) == (48, 64)
    imgs = (ctypes.c_void_p * 1)(img._h.value)
    planes = (_lib.Planes * 1)()
    for c in range(3):
        planes[0].plane[c], planes[0].pitch[c] = 0x1000 * (c + 1), 64

    def call(scale=(17, 11, 0, 0, 0, 0), src=0, elem=1, layout=0, a=(1, 1, 1, 1), b=(0, 0, 0, 0), flip=0,
             data=0x10000, stride_c=None, stride_y=None, n=1, null=()):
        esz = 4 if elem == 0 else 2
        C = 4 if src & 1 else 3
        row = scale[0] * esz * (C if layout == 1 else 1)
        fmt = _lib.TensorFormat(src=src, elem=elem, layout=layout)
        for c in range(4):
            fmt.a[c], fmt.b[c] = a[c], b[c]
        surf = (_lib.TensorSurface * 1)()
        surf[0].data = data
        surf[0].stride_y = row if stride_y is None else stride_y
        surf[0].stride_c = row * scale[1] if stride_c is None else stride_c
        sc = (_lib.Scale * 1)(_lib.Scale(*scale))
        fl = None if flip is None else (ctypes.c_uint32 * 1)(flip)
        args = dict(imgs=imgs, planes=planes, fmt=ctypes.byref(fmt), sc=sc, surf=surf)
        for k in null:
            args[k] = None
        rc = _lib.lib.heifgpu_render_batch_tensor(None, args["imgs"], n, args["planes"], None, None, args["fmt"],
                                                  args["sc"], fl, args["surf"], None)
        return rc, _lib.last_error()

    call.img = img  # (keeps the parsed image alive)
    return call


def test_good_arguments_fail_on_the_context_only(caller):
    from heif_amd import _lib

    INV = _lib.HEIFGPU_E_INVALID
    for kw in (dict(), dict(flip=None), dict(flip=3), dict(elem=0), dict(elem=2, layout=1), dict(src=1, layout=1),
               dict(src=2, elem=0), dict(src=3), dict(scale=(17, 11, 5, 3, 41, 29), flip=1),
               dict(data=0x10002), dict(data=0x10004, elem=0), dict(stride_y=17 * 2 + 2, stride_c=2),
               dict(a=(2.0 ** -24, 1e30, -3.0, float("nan"))),  # the fourth constant is not used by an RGB source
               dict(layout=1, stride_c=1)):                     # stride_c is not used by HWC
        rc, msg = caller(**kw)
        assert rc == INV and "context" in msg, (kw, msg)


def test_rejections_need_no_device(caller):
    from heif_amd import _lib

    INV = _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_render_batch_tensor(None, None, 0, None, None, None, None, None, None, None,
                                                None) == INV
    for null in ("imgs", "planes", "fmt", "sc", "surf"):
        rc, msg = caller(null=(null,))
        assert rc == INV and "argument" in msg, null
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(src=4), "source format"), (dict(src=0xFFFFFFFF), "source format"),
        (dict(elem=3), "element type"), (dict(layout=2), "layout"),
        (dict(flip=4), "flip"), (dict(flip=0xFFFFFFFF), "flip"),
        (dict(a=(1, nan, 1, 1)), "finite"), (dict(a=(inf, 1, 1, 1)), "finite"), (dict(b=(0, 0, -inf, 0)), "finite"),
        (dict(src=1, b=(0, 0, 0, nan)), "finite"), (dict(src=3, a=(1, 1, 1, inf)), "finite"),
        (dict(data=0), "data"), (dict(data=0x10001), "aligned"), (dict(data=0x10002, elem=0), "aligned"),
        (dict(data=0x10001, elem=2, layout=1), "aligned"),
        (dict(stride_y=17 * 2 - 2), "stride_y"), (dict(stride_y=17 * 2 + 1), "stride_y"),
        (dict(elem=0, stride_y=17 * 4 + 2), "stride_y"), (dict(elem=0, stride_y=17 * 4 - 4), "stride_y"),
        (dict(layout=1, stride_y=17 * 3 * 2 - 2), "stride_y"), (dict(src=1, layout=1, elem=0, stride_y=17 * 16 - 4), "stride_y"),
        (dict(stride_y=-64), "stride_y"),
        (dict(stride_c=1001), "stride_c"), (dict(elem=0, stride_c=1002), "stride_c"),
        # every check of heifgpu_render_batch_scaled
        (dict(scale=(17, 11, 0, 0, 41, 0)), "window"), (dict(scale=(17, 11, 8, 0, 41, 29)), "window"),
        (dict(scale=(17, 11, 0, 0, 49, 64)), "window"), (dict(scale=(17, 11, 0xFFFFFFFF, 0, 2, 2)), "window"),
        (dict(scale=(0, 11, 0, 0, 0, 0), stride_y=64), "rendered size"),
        (dict(scale=(17, 65536, 0, 0, 0, 0)), "rendered size"),
        (dict(n=65536), "65535"),
    ]
    for kw, word in cases:
        rc, msg = caller(**kw)
        assert rc == INV and word in msg and "context" not in msg, (kw, msg)


# ---- the checker against itself -------------------------------------------------
LEVELS = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)


def test_checker_unit_scale_returns_the_levels():
    one, zero = (1, 1, 1), (0, 0, 0)
    f32 = tensor_ref.tensor(LEVELS, one, zero, "f32", "hwc")
    assert f32.dtype == np.uint32 and np.array_equal(f32.view(np.float32), LEVELS.astype(np.float32))
    f16 = tensor_ref.tensor(LEVELS, one, zero, "f16", "hwc")
    assert f16.dtype == np.uint16 and np.array_equal(f16.view(np.float16).astype(np.int64), LEVELS)  # < 2048: exact
    bf = tensor_ref.tensor(LEVELS, one, zero, "bf16", "hwc")
    assert bf.dtype == np.uint16
    back = (bf.astype(np.uint32) << 16).view(np.float32)  # 8 significant bits hold 0..255 exactly
    assert np.array_equal(back, LEVELS.astype(np.float32))
    assert bf[0, 1, 0] == 0x3F80 and bf[15, 15, 0] == 0x437F and bf[0, 0, 0] == 0


def test_checker_f16_subnormals_are_the_levels_bit_patterns():
    """R * 2^-24 is R units of binary16's smallest subnormal: the bit pattern is R itself
    (1..255 are below 1024, so none of them is normal)."""
    a = (2.0 ** -24,) * 3
    f16 = tensor_ref.tensor(LEVELS, a, (0, 0, 0), "f16", "hwc")
    assert np.array_equal(f16, LEVELS.astype(np.uint16))
    assert f16[0, 1, 0] == 0x0001 and f16[15, 15, 0] == 0x00FF
    # and the float32 intermediates were normal numbers, inside the contract
    f32 = tensor_ref.tensor(LEVELS, a, (0, 0, 0), "f32", "hwc").view(np.float32)
    assert (f32[LEVELS > 0] >= np.finfo(np.float32).tiny).all()


def test_checker_bf16_rounds_ties_to_even():
    # 257 = 0x43808000: exactly between bf16 0x4380 (256) and 0x4381 (258): to the even 0x4380
    # 259 = 0x43818000: exactly between 0x4381 (258) and 0x4382 (260): to the even 0x4382
    R = np.array([[[257, 259, 258]]], np.uint16)
    bf = tensor_ref.tensor(R, (1, 1, 1), (0, 0, 0), "bf16", "hwc")
    assert np.array_equal(np.array([257, 259], np.float32).view(np.uint32), [0x43808000, 0x43818000])
    assert bf[0, 0].tolist() == [0x4380, 0x4382, 0x4381]
    # not a tie: one unit in the last place of float32 above and below it
    f = np.array([0x43808001, 0x43807FFF], np.uint32).view(np.float32)
    assert tensor_ref.bf16_bits(f).tolist() == [0x4381, 0x4380]
    # negative values round the magnitude; the largest finite float32 overflows to infinity
    f = np.array([-257.0, -259.0, np.finfo(np.float32).max], np.float32)
    assert tensor_ref.bf16_bits(f).tolist() == [0xC380, 0xC382, 0x7F80]


def test_checker_two_roundings_not_one():
    """A case where the fused multiply-add differs: the checker must give the two-rounding value."""
    a, b = np.float32(1.0 / (255.0 * 0.229)), np.float32(-0.485 / 0.229)
    diff = 0
    for r in range(256):
        two = np.float32(np.float32(r) * a) + b
        one = np.float32(float(np.float32(r)) * float(a) + float(b))  # exact product and sum in double, one rounding
        got = tensor_ref.tensor(np.full((1, 1, 3), r, np.uint8), (a,) * 3, (b,) * 3, "f32", "hwc").view(np.float32)[0, 0, 0]
        assert got == two
        diff += int(one != two)
    assert diff > 0  # the distinction is real at these constants


def test_checker_layout_flip_and_constants():
    rng = np.random.default_rng(7)
    R = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    a, b = tensor_ref.constants((0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25), 255)
    assert a.dtype == np.float32 and a[3] == np.float32(1.0 / (255.0 * 0.25)) and b[0] == np.float32(-0.485 / 0.229)
    hwc = tensor_ref.tensor(R, a, b, "f32", "hwc")
    chw = tensor_ref.tensor(R, a, b, "f32", "chw")
    assert chw.shape == (4, 5, 7) and np.array_equal(chw, hwc.transpose(2, 0, 1))
    assert np.array_equal(tensor_ref.tensor(R, a, b, "f32", "chw", flip=1), chw[:, :, ::-1])
    assert np.array_equal(tensor_ref.tensor(R, a, b, "f32", "chw", flip=2), chw[:, ::-1])
    assert np.array_equal(tensor_ref.tensor(R, a, b, "f32", "hwc", flip=3), hwc[::-1, ::-1])
