"""The colour-managed render on the device: render / render_scaled / render_tensor /
decode_display with colorspace= against color_ref's numpy formula applied to what
display_ref, scale_ref and tensor_ref give for the planes the GPU decoded, byte for
byte.  The tables the formula reads come from the library and are checked against
the float64 model in tests/test_color.py; here only the kernels are under test.

The batch is the smallest that reaches every path: a turned picture (the transposing
LDS path of k_render, partial 64 x 64 tiles) with a P3 profile and an alpha image, a
mirrored 4:4:4 one whose profile decides the colour and whose nclx the matrix, an
unlabelled one (identity to sRGB: untouched), and a cropped one at an odd offset with a
BT.2020 gamma-2.2 profile; 8-bit formats, then the first and third at 10 and 12 bits."""
import numpy as np
import pytest

import color_ref
import display_ref
import scale_ref
import tensor_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SPACES = ("srgb", "display-p3")
CLAP = ("clap", (41, 1, 29, 1, 1, 2, 1, 2))  # 41 x 29 at left 15, top 5 of 70 x 38


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def S():
    from heif_amd import synth_encoder

    return synth_encoder


@pytest.fixture(scope="module")
def ctx(H):
    return H.HeicDecoder.context(0)


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def bits_of(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def boxes(S, steps):
    make = {"clap": lambda a: S.clap_box(*a), "irot": S.irot_box, "imir": S.imir_box}
    return tuple(make[k](a) for k, a in steps)


def specs(S, depth=8):
    """(params, steps, colr boxes, alpha params) of the four pictures."""
    p3 = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    bt2020 = S.icc_profile(color_ref.nclx_colorants(9), S.icc_curv((2.2,)), version=2)
    return [
        (S.SynthParams(width=136, height=72, conf_right=6, bit_depth=depth), [("irot", 1)], [S.icc_box(p3)],
         S.SynthParams(width=136, height=72, conf_right=6, chroma_format=0, bit_depth=depth)),
        (S.SynthParams(width=72, height=40, chroma_format=3, bit_depth=depth), [("imir", 0)],
         [S.nclx_box(1, 13, 6, True), S.icc_box(p3)], None),
        (S.SynthParams(width=64, height=64, bit_depth=depth), [], [], None),
        (S.SynthParams(width=72, height=40, conf_right=2, conf_bottom=2, bit_depth=depth), [CLAP], [S.icc_box(bt2020)], None),
    ]


class Batch:
    """The pictures decoded once (never written to), their alpha images, and the
    displayed picture D of each by display_ref, per format."""

    def __init__(self, H, S, depth, pick):
        self.steps, self.outs, self.alphas = [], [], []
        for k in pick:
            p, steps, colr, ap = specs(S, depth)[k]
            aux = (S.AuxImage(ap, seed=50 + k, urn=S.ALPHA_URN_MPEGB),) if ap is not None else ()
            f = S.display_heic(p, seed=40 + k, transforms=boxes(S, steps), colr=colr, aux=aux)
            self.outs.append(H.HeicDecoder.decode(f))
            self.alphas.append(H.HeicDecoder.decode(f, item_id=2) if ap is not None else None)
            self.steps.append(steps)
        self.depth = depth
        self._D = {}

    def D(self, fmt):
        if fmt not in self._D:
            res = []
            for o, al, steps in zip(self.outs, self.alphas, self.steps):
                y, cb, cr = [None if t is None else host(t) for t in (o.y, o.cb, o.cr)]
                inf = o.info
                res.append(display_ref.render(y, cb, cr, inf.matrix_coeffs, bool(inf.full_range), inf.bit_depth, steps, fmt,
                                              alpha=None if al is None or not fmt.startswith("rgba") else host(al.y),
                                              alpha_depth=8 if al is None else al.info.bit_depth))
            self._D[fmt] = res
        return self._D[fmt]

    def transforms(self, space, fmt):
        return [o.image.color_transform(space, self.depth if fmt.endswith("16") else 8) for o in self.outs]


@pytest.fixture(scope="module")
def batch8(H, S):
    return Batch(H, S, 8, (0, 1, 2, 3))


def test_sources_as_the_batch_needs_them(batch8):
    """What the other tests rely on: which pictures are identities to which space, the
    nclx matrix beside the profile, and that P3 to sRGB leaves the gamut on both sides."""
    ident = {sp: [t.identity for t in batch8.transforms(sp, "rgb8")] for sp in SPACES}
    assert ident == {"srgb": [0, 0, 1, 0], "display-p3": [1, 1, 0, 0]}
    o = batch8.outs[1]
    assert o.image.color.kind == "icc" and (o.info.matrix_coeffs, o.info.full_range) == (6, 1)
    assert [tuple(d.shape) for d in batch8.D("rgb8")] == [(130, 72, 3), (40, 72, 3), (64, 64, 3), (29, 41, 3)]
    want = color_ref.transform_picture(batch8.transforms("srgb", "rgb8")[0], batch8.D("rgb8")[0])
    assert (want == 0).any() and (want == 255).any() and (want != batch8.D("rgb8")[0]).any()


@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
def test_render(ctx, batch8, fmt):
    plain = [host(t) for t in ctx.render(batch8.outs, fmt, batch8.alphas)]
    for k, D in enumerate(batch8.D(fmt)):
        assert np.array_equal(plain[k], D), k  # the default path is what it was
    for space in SPACES:
        ts = batch8.transforms(space, fmt)
        got = [host(t) for t in ctx.render(batch8.outs, fmt, batch8.alphas, colorspace=space)]
        for k, (D, t) in enumerate(zip(batch8.D(fmt), ts)):
            want = color_ref.transform_picture(t, D)
            assert np.array_equal(got[k], want), (space, k)
            if t.identity:
                assert np.array_equal(got[k], plain[k]), (space, k)
            else:
                assert (got[k][..., :3] != plain[k][..., :3]).any(), (space, k)
            if fmt == "rgba8":
                assert np.array_equal(got[k][..., 3], plain[k][..., 3]), (space, k)  # alpha untouched
        if space == "srgb":  # P3 noise leaves sRGB's gamut: both clamps are exercised
            want = color_ref.transform_picture(ts[0], batch8.D(fmt)[0])[..., :3]
            assert (want == 0).any() and (want == 255).any()
    if fmt == "rgba8":
        assert len(np.unique(plain[0][..., 3])) > 4 and (plain[1][..., 3] == 255).all()


@pytest.mark.parametrize("depth", [10, 12])
def test_render_rgb16(H, S, ctx, depth):
    b = Batch(H, S, depth, (0, 2))
    maxv = (1 << depth) - 1
    plain = [host(t) for t in ctx.render(b.outs, "rgb16")]
    for space in SPACES:
        ts = b.transforms(space, "rgb16")
        assert [t.bits for t in ts] == [depth, depth]
        got = [host(t) for t in ctx.render(b.outs, "rgb16", colorspace=space)]
        for k, (D, t) in enumerate(zip(b.D("rgb16"), ts)):
            assert np.array_equal(plain[k], D), k
            want = color_ref.transform_picture(t, D)
            assert np.array_equal(got[k], want), (space, k)
            assert t.identity == (1 if (space, k) in (("srgb", 1), ("display-p3", 0)) else 0)
        if space == "srgb":
            want = color_ref.transform_picture(ts[0], b.D("rgb16")[0])
            assert (want == 0).any() and (want == maxv).any()
    # an 8-bit transform for a picture rendered at its own depth is refused before any launch
    from heif_amd import _lib
    import ctypes

    t8 = b.outs[0].image.color_transform("srgb", 8)
    imgs = (ctypes.c_void_p * 1)(b.outs[0].image._h.value)
    xf = (ctypes.c_void_p * 1)(ctypes.addressof(t8))
    surf = (_lib.Surface * 1)()
    out = torch.zeros((130, 72, 3), dtype=torch.int16, device="cuda:0")
    surf[0].pixels, surf[0].pitch = out.data_ptr(), 72 * 6
    rc = _lib.lib.heifgpu_render_batch_color(ctx._h, imgs, 1, H.DecodeContext.planes_of(b.outs[:1]), None, None,
                                             _lib.PIX_RGB16, xf, surf, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc == _lib.HEIFGPU_E_INVALID
    torch.cuda.synchronize()
    assert not out.any()


def scales_for(batch, window_on=3):
    """cover onto (31, 50) for every picture, and an explicit window on one of them."""
    res = []
    for k, D in enumerate(batch.D("rgb8")):
        dh, dw = D.shape[:2]
        res.append(scale_ref.fit(dw, dh, 50, 31, "cover"))
    res[window_on] = (50, 31, 3, 2, 33, 25)
    return res


def averaged(D, sc):
    ow, oh, x, y, w, h = sc
    return scale_ref.area_average(D, (x, y, w, h) if w or h else None, ow, oh)


@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
def test_render_scaled(ctx, batch8, fmt):
    """cover, and one explicit window: the transform of scale_ref's integers."""
    scs = scales_for(batch8)
    Rs = [averaged(D, sc) for D, sc in zip(batch8.D(fmt), scs)]
    windows = [(sc[2], sc[3], sc[4], sc[5]) for sc in scs]
    plain = host(ctx.render_scaled(batch8.outs, (31, 50), fmt=fmt, alphas=batch8.alphas, windows=windows))
    cover = host(ctx.render_scaled(batch8.outs[:3], (31, 50), "cover", fmt, batch8.alphas[:3], colorspace="srgb"))
    for k, R in enumerate(Rs):
        assert np.array_equal(plain[k], R), k
    for space in SPACES:
        ts = batch8.transforms(space, fmt)
        got = host(ctx.render_scaled(batch8.outs, (31, 50), fmt=fmt, alphas=batch8.alphas, windows=windows, colorspace=space))
        for k, (R, t) in enumerate(zip(Rs, ts)):
            assert np.array_equal(got[k], color_ref.transform_picture(t, R)), (space, k)
            if t.identity:
                assert np.array_equal(got[k], plain[k])
        if space == "srgb":
            assert np.array_equal(cover, got[:3])  # mode="cover" is those windows


def test_render_tensor(ctx, batch8):
    scs = scales_for(batch8)
    Rs = [averaged(D, sc) for D, sc in zip(batch8.D("rgb8"), scs)]
    windows = [(sc[2], sc[3], sc[4], sc[5]) for sc in scs]
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    flips = [0, 1, 2, 3]
    for dtype, elem, layout in ((torch.float16, "f16", "chw"), (torch.float32, "f32", "hwc")):
        plain = bits_of(ctx.render_tensor(batch8.outs, (31, 50), dtype=dtype, layout=layout, windows=windows, flips=flips))
        for k, R in enumerate(Rs):
            assert np.array_equal(plain[k], tensor_ref.tensor(R, a, b, elem, layout, flip=flips[k])), (layout, k)
        for space in SPACES:
            ts = batch8.transforms(space, "rgb8")
            got = bits_of(ctx.render_tensor(batch8.outs, (31, 50), dtype=dtype, layout=layout, windows=windows, flips=flips,
                                            colorspace=space))
            for k, (R, t) in enumerate(zip(Rs, ts)):
                want = tensor_ref.tensor(color_ref.transform_picture(t, R), a, b, elem, layout, flip=flips[k])
                assert np.array_equal(got[k], want), (space, layout, k)


def test_decode_display_halfmoonbay(H, ctx, halfmoonbay):
    """Real content, the real profile: 12 megapixels, irot 3, contained in 96 x 128."""
    o = H.HeicDecoder.decode(halfmoonbay)
    D = host(ctx.render([o], "rgb8")[0])
    R = averaged(D, scale_ref.fit(3024, 4032, 128, 96, "contain"))
    assert R.shape == (96, 72, 3)
    t = o.image.color_transform("srgb")
    got = host(H.HeicDecoder.decode_display(halfmoonbay, colorspace="srgb", size=(96, 128)))
    want = color_ref.transform_picture(t, R)
    assert np.array_equal(got, want) and (want != R).any()
    assert np.array_equal(host(H.HeicDecoder.decode_display(halfmoonbay, colorspace="display-p3", size=(96, 128))), R)
    assert np.array_equal(host(H.HeicDecoder.decode_display(halfmoonbay, size=(96, 128))), R)


def test_back_to_back_batches_share_the_cache(H, S, ctx, batch8):
    """Two different batches (other sources, another depth: other tables) rendered back to
    back on one stream with no synchronisation in between; then again, from a warm cache."""
    other = Batch(H, S, 10, (0, 2))
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        first = ctx.render(batch8.outs, "rgb8", colorspace="srgb")
        second = ctx.render(other.outs, "rgb16", colorspace="display-p3")
        third = ctx.render(batch8.outs[::-1], "rgb8", colorspace="display-p3")
        runs.append((first, second, third))
    torch.cuda.synchronize()
    for first, second, third in runs:
        for k, (D, t) in enumerate(zip(batch8.D("rgb8"), batch8.transforms("srgb", "rgb8"))):
            assert np.array_equal(host(first[k]), color_ref.transform_picture(t, D)), k
        for k, (D, t) in enumerate(zip(other.D("rgb16"), other.transforms("display-p3", "rgb16"))):
            assert np.array_equal(host(second[k]), color_ref.transform_picture(t, D)), k
        for k, (D, t) in enumerate(zip(batch8.D("rgb8")[::-1], batch8.transforms("display-p3", "rgb8")[::-1])):
            assert np.array_equal(host(third[k]), color_ref.transform_picture(t, D)), k


def test_unsupported_source_raises_before_any_launch(H, S, ctx):
    f = S.display_heic(S.SynthParams(width=64, height=64), seed=7, colr=S.nclx_box(9, 16, 9, False))
    o = H.HeicDecoder.decode(f)  # decodes as ever
    assert tuple(ctx.render([o])[0].shape) == (64, 64, 3)
    for call in (lambda: ctx.render([o], colorspace="srgb"), lambda: ctx.render_scaled([o], (8, 8), colorspace="srgb"),
                 lambda: ctx.render_tensor([o], (8, 8), colorspace="display-p3")):
        with pytest.raises(H.UnsupportedError):
            call()
    with pytest.raises(ValueError):
        ctx.render([o], colorspace="rec2020")
