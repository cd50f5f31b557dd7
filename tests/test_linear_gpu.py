"""The linear-light scaled render on the device: render_scaled / render_tensor / render_jpeg /
decode_display with linear=True against linear_ref's numpy contract applied to display_ref's
picture of the planes the GPU decoded, byte for byte.  The arithmetic's host twin and the
accuracy are in tests/test_linear.py; here the kernels (render_linear.hip) are under test.

The batch is test_color_gpu's four pictures (a turned one with a P3 profile and an alpha
image: the swapped-axes path; a mirrored 4:4:4 one; an unlabelled one, whose identity
transform must be applied all the same; one cropped at an odd offset with a BT.2020 profile)
and a 1536 x 16 one whose tile footprint spans three 512-column chunks; 8-bit formats,
then the first and third at 10 and 12 bits."""
import ctypes

import numpy as np
import pytest

import chroma_ref
import color_ref
import display_ref
import linear_ref
import scale_ref
import tensor_ref
import window_cases as WC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SPACES = ("srgb", "display-p3")
CLAP = ("clap", (41, 1, 29, 1, 1, 2, 1, 2))  # 41 x 29 at left 15, top 5 of 70 x 38
BOX = (31, 50)  # (h, w)


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
    """(params, steps, colr boxes, alpha params) of the five pictures."""
    p3 = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    bt2020 = S.icc_profile(color_ref.nclx_colorants(9), S.icc_curv((2.2,)), version=2)
    return [
        (S.SynthParams(width=136, height=72, conf_right=6, bit_depth=depth), [("irot", 1)], [S.icc_box(p3)],
         S.SynthParams(width=136, height=72, conf_right=6, chroma_format=0, bit_depth=depth)),
        (S.SynthParams(width=72, height=40, chroma_format=3, bit_depth=depth), [("imir", 0)],
         [S.nclx_box(1, 13, 6, True), S.icc_box(p3)], None),
        (S.SynthParams(width=64, height=64, bit_depth=depth), [], [], None),
        (S.SynthParams(width=72, height=40, conf_right=2, conf_bottom=2, bit_depth=depth), [CLAP], [S.icc_box(bt2020)], None),
        (S.SynthParams(width=1536, height=16, bit_depth=depth), [], [S.icc_box(p3)], None),
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
    return Batch(H, S, 8, (0, 1, 2, 3, 4))


def lin(t, D, sc):
    ow, oh, x, y, w, h = sc
    return linear_ref.linear_average(t, D, (x, y, w, h) if w or h else None, ow, oh)


def fits(batch, mode, box=BOX):
    return [scale_ref.fit(D.shape[1], D.shape[0], box[1], box[0], mode) for D in batch.D("rgb8")]


# explicit windows onto BOX: the first at its own size (50 x 31), one at an odd offset, the long
# picture's whole width (three chunks per a-line) and a strip of it that begins inside a chunk
WINDOWS = [(11, 40, 50, 31), (3, 2, 65, 33), (0, 0, 64, 64), (3, 2, 33, 25), (0, 0, 1536, 16)]
WINDOWS_B = [(0, 0, 72, 130), (7, 1, 50, 31), (1, 1, 62, 62), (0, 0, 41, 29), (301, 3, 1100, 11)]


def test_sources_as_the_batch_needs_them(batch8):
    ident = {sp: [t.identity for t in batch8.transforms(sp, "rgb8")] for sp in SPACES}
    assert ident == {"srgb": [0, 0, 1, 0, 0], "display-p3": [1, 1, 0, 0, 1]}
    assert [tuple(d.shape) for d in batch8.D("rgb8")] == [(130, 72, 3), (40, 72, 3), (64, 64, 3), (29, 41, 3), (16, 1536, 3)]


@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
def test_render_scaled(ctx, batch8, fmt):
    """cover, stretch, contain and explicit windows (one at its own size), then every picture
    into one pixel: linear_ref of display_ref's picture, byte for byte."""
    Ds = batch8.D(fmt)
    for space in SPACES:
        ts = batch8.transforms(space, fmt)
        for mode in ("cover", "stretch", "contain"):
            got = ctx.render_scaled(batch8.outs, BOX, mode, fmt, batch8.alphas, colorspace=space, linear=True)
            for k, (D, t, sc) in enumerate(zip(Ds, ts, fits(batch8, mode))):
                assert np.array_equal(host(got[k]), lin(t, D, sc)), (space, mode, k)
        for windows in (WINDOWS, WINDOWS_B):
            got = host(ctx.render_scaled(batch8.outs, BOX, fmt=fmt, alphas=batch8.alphas, windows=windows, colorspace=space,
                                         linear=True))
            for k, (D, t, w) in enumerate(zip(Ds, ts, windows)):
                assert np.array_equal(got[k], lin(t, D, (BOX[1], BOX[0]) + w)), (space, k)
        one = host(ctx.render_scaled(batch8.outs, (1, 1), "stretch", fmt, batch8.alphas, colorspace=space, linear=True))
        for k, (D, t) in enumerate(zip(Ds, ts)):
            assert np.array_equal(one[k], lin(t, D, (1, 1, 0, 0, 0, 0))), (space, k)
    # the identity transform was applied: the unlabelled picture differs from its encoded average
    sc = fits(batch8, "stretch")[2]
    want = lin(batch8.transforms("srgb", fmt)[2], Ds[2], sc)
    assert (want != scale_ref.area_average(Ds[2], None, sc[0], sc[1])).any()
    if fmt == "rgba8":  # alpha is the scaled render's average of the codes
        sc = fits(batch8, "cover")[0]
        got = host(ctx.render_scaled(batch8.outs[:1], BOX, "cover", fmt, batch8.alphas[:1], colorspace="srgb", linear=True))
        assert np.array_equal(got[0][..., 3], scale_ref.area_average(Ds[0], sc[2:], sc[0], sc[1])[..., 3])
        assert len(np.unique(got[0][..., 3])) > 4


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("fmt", ["rgb16", "rgba16"])
def test_render_scaled_16(H, S, ctx, depth, fmt):
    b = Batch(H, S, depth, (0, 2))
    Ds = b.D(fmt)
    windows = [(11, 40, 50, 31), (1, 1, 62, 62)]
    for space in SPACES:
        ts = b.transforms(space, fmt)
        assert [t.bits for t in ts] == [depth, depth]
        for mode in ("cover", "stretch"):
            got = host(ctx.render_scaled(b.outs, BOX, mode, fmt, b.alphas, colorspace=space, linear=True))
            for k, (D, t, sc) in enumerate(zip(Ds, ts, fits(b, mode))):
                assert np.array_equal(got[k], lin(t, D, sc)), (space, mode, k)
        got = host(ctx.render_scaled(b.outs, BOX, fmt=fmt, alphas=b.alphas, windows=windows, colorspace=space, linear=True))
        full = ctx.render(b.outs, fmt, b.alphas, colorspace=space)
        for k, (D, t, w) in enumerate(zip(Ds, ts, windows)):
            assert np.array_equal(got[k], lin(t, D, (BOX[1], BOX[0]) + w)), (space, k)
        x, y, w, h = windows[0]  # at its own size: the window of the managed full-size render
        assert np.array_equal(got[0], host(full[0])[y:y + h, x:x + w]), space


def test_render_tensor(ctx, batch8):
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    flips = [0, 1, 2, 3, 1]
    scs = [(BOX[1], BOX[0]) + w for w in WINDOWS]
    for dtype, elem, layout in ((torch.float16, "f16", "chw"), (torch.float32, "f32", "hwc"), (torch.bfloat16, "bf16", "chw"),
                                (torch.float16, "f16", "hwc")):
        for space in SPACES:
            ts = batch8.transforms(space, "rgb8")
            got = bits_of(ctx.render_tensor(batch8.outs, BOX, dtype=dtype, layout=layout, windows=WINDOWS, flips=flips,
                                            colorspace=space, linear=True))
            for k, (D, t, sc) in enumerate(zip(batch8.D("rgb8"), ts, scs)):
                want = tensor_ref.tensor(lin(t, D, sc), a, b, elem, layout, flip=flips[k])
                assert np.array_equal(got[k], want), (space, elem, layout, k)
    # an RGBA source with the alpha image, cover, and "contain" (a list)
    a4, b4 = tensor_ref.constants(tensor_ref.IMAGENET_MEAN + (0.5,), tensor_ref.IMAGENET_STD + (0.25,), 255)
    ts = batch8.transforms("srgb", "rgba8")
    for mode in ("cover", "contain"):
        got = ctx.render_tensor(batch8.outs, BOX, mode, torch.float32, "chw", tensor_ref.IMAGENET_MEAN + (0.5,),
                                tensor_ref.IMAGENET_STD + (0.25,), "rgba8", alphas=batch8.alphas, colorspace="srgb", linear=True)
        for k, (D, t, sc) in enumerate(zip(batch8.D("rgba8"), ts, fits(batch8, mode))):
            assert np.array_equal(bits_of(got[k]), tensor_ref.tensor(lin(t, D, sc), a4, b4, "f32", "chw")), (mode, k)


@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
def test_own_size_window_is_the_managed_render(ctx, batch8, fmt):
    """out = the window's size: bit for bit the window of render(colorspace=X), which for an
    identity transform is the window of plain render()."""
    windows = [(11, 40, 50, 31), (7, 1, 50, 31), (5, 9, 50, 31), (0, 0, 41, 29), (700, 0, 50, 16)]
    for space in SPACES:
        full = ctx.render(batch8.outs, fmt, batch8.alphas, colorspace=space)
        plain = ctx.render(batch8.outs, fmt, batch8.alphas)
        for k, (x, y, w, h) in enumerate(windows):
            got = host(ctx.render_scaled(batch8.outs[k:k + 1], (h, w), fmt=fmt, alphas=batch8.alphas[k:k + 1], windows=[windows[k]],
                                         colorspace=space, linear=True))[0]
            assert np.array_equal(got, host(full[k])[y:y + h, x:x + w]), (space, k)
            if batch8.transforms(space, fmt)[k].identity:
                assert np.array_equal(got, host(plain[k])[y:y + h, x:x + w]), (space, k)


def test_mixed_batch_of_bilinear_and_replicated_chroma(H, S, ctx):
    p3 = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    p = S.SynthParams(width=136, height=72, conf_right=6)
    o = H.HeicDecoder.decode(S.display_heic(p, seed=3, colr=[S.icc_box(p3)]))
    cases = [([("irot", 1)], 1), ([("irot", 1)], None), ([], 4), ([("imir", 0)], None)]
    outs = []
    for steps, loc in cases:
        img = H.HeifImage.parse(S.display_heic(p, transforms=boxes(S, steps), colr=[S.icc_box(p3)]),
                                chroma="bilinear" if loc is not None else None)
        img.chroma_loc = loc
        outs.append(H.DecodedImage(o.y, o.cb, o.cr, o.info, img))
    y, cb, cr = (host(t) for t in (o.y, o.cb, o.cr))
    inf = o.info
    got = host(ctx.render_scaled(outs, BOX, "cover", "rgb8", colorspace="srgb", linear=True))
    seen = []
    for k, (steps, loc) in enumerate(cases):
        c = (cb, cr) if loc is None else chroma_ref.upsample(cb, cr, inf.chroma_format_idc, loc, inf.height, inf.width)
        D = display_ref.render(y, c[0], c[1], inf.matrix_coeffs, bool(inf.full_range), inf.bit_depth, steps, "rgb8")
        sc = scale_ref.fit(D.shape[1], D.shape[0], BOX[1], BOX[0], "cover")
        want = lin(outs[k].image.color_transform("srgb", 8), D, sc)
        assert np.array_equal(got[k], want), k
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])  # each image its own rule


def test_window_decoded_image(H, ctx):
    """prepare(windows=) decodes the tiles the window reads: the rectangle is the area render's."""
    data = WC.fixture("rot1_mir")
    img = H.HeifImage.parse(data)
    full = H.HeicDecoder.decode(data)
    window = (20, 30, 100, 90)
    outs = ctx.alloc_outputs([img])
    b = ctx.prepare([img], windows=[window])
    b.decode_async(outs)
    assert b.status() == [0] and b.pictures < 12
    got = host(ctx.render_scaled(outs, (9, 7), fmt="rgb8", windows=[window], colorspace="srgb", linear=True))[0]
    b.free()
    y, cb, cr = (host(t) for t in (full.y, full.cb, full.cr))
    inf = full.info
    D = display_ref.render(y, cb, cr, inf.matrix_coeffs, bool(inf.full_range), inf.bit_depth, list(WC.VARIANTS["rot1_mir"]), "rgb8")
    assert np.array_equal(got, lin(img.color_transform("srgb", 8), D, (7, 9) + window))
    assert np.array_equal(got, host(ctx.render_scaled([full], (9, 7), fmt="rgb8", windows=[window], colorspace="srgb",
                                                      linear=True))[0])


def test_render_jpeg(ctx, batch8):
    outs = batch8.outs[:4]
    files = ctx.render_jpeg(outs, BOX, "cover", colorspace="srgb", linear=True)
    rgb = ctx.render_scaled(outs, BOX, "cover", "rgb8", colorspace="srgb", linear=True)
    assert files == ctx.encode_jpeg(rgb)
    assert files != ctx.render_jpeg(outs, BOX, "cover", colorspace="srgb")
    assert all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" for f in files)


def test_refusals_write_nothing(H, S, ctx, batch8):
    from heif_amd import _lib

    for call in (lambda **kw: ctx.render_scaled(batch8.outs, BOX, **kw), lambda **kw: ctx.render_tensor(batch8.outs, BOX, **kw)):
        with pytest.raises(ValueError):
            call(colorspace="srgb", linear=True, filter="bicubic")
        with pytest.raises(ValueError):
            call(linear=True)
    # a tone transform in the batch, straight at the C entry point: refused before any launch
    pq = H.HeicDecoder.decode(S.display_heic(S.SynthParams(width=64, height=64), seed=7, colr=S.nclx_box(9, 16, 9, False)))
    outs = [batch8.outs[2], pq]
    keep = [outs[0].image.color_transform("srgb", 8), pq.image.color_transform("srgb", 8, tone_map="bt2390")]
    assert keep[1].base.tone
    xf = (ctypes.c_void_p * 2)(ctypes.addressof(keep[0]), ctypes.addressof(keep[1].base))
    imgs = (ctypes.c_void_p * 2)(*[o.image._h.value for o in outs])
    sc = (_lib.Scale * 2)(_lib.Scale(20, 10, 0, 0, 0, 0), _lib.Scale(20, 10, 0, 0, 0, 0))
    out = torch.full((2, 10, 20, 3), 0xA5, dtype=torch.uint8, device="cuda:0")
    surf = (_lib.Surface * 2)()
    for i in range(2):
        surf[i].pixels, surf[i].pitch = out[i].data_ptr(), 60
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    planes = H.DecodeContext.planes_of(outs)
    rc = _lib.lib.heifgpu_render_batch_scaled_linear(ctx._h, imgs, 2, planes, None, None, _lib.PIX_RGB8, sc, xf, surf, stream)
    assert rc == _lib.HEIFGPU_E_UNSUPPORTED and "tone" in _lib.last_error()
    xf[1] = None
    rc = _lib.lib.heifgpu_render_batch_scaled_linear(ctx._h, imgs, 2, planes, None, None, _lib.PIX_RGB8, sc, xf, surf, stream)
    assert rc == _lib.HEIFGPU_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    with pytest.raises(ValueError):
        ctx.render_scaled(outs, BOX, colorspace="srgb", tone_map="bt2390", linear=True)


def test_without_linear_the_managed_render_is_what_it_was(ctx, batch8):
    for fmt in ("rgb8", "rgba8"):
        for space in SPACES:
            ts = batch8.transforms(space, fmt)
            got = host(ctx.render_scaled(batch8.outs, BOX, fmt=fmt, alphas=batch8.alphas, windows=WINDOWS, colorspace=space))
            for k, (D, t, w) in enumerate(zip(batch8.D(fmt), ts, WINDOWS)):
                want = color_ref.transform_picture(t, scale_ref.area_average(D, w, BOX[1], BOX[0]))
                assert np.array_equal(got[k], want), (fmt, space, k)
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    ts = batch8.transforms("srgb", "rgb8")
    got = bits_of(ctx.render_tensor(batch8.outs, BOX, dtype=torch.float32, windows=WINDOWS, colorspace="srgb"))
    for k, (D, t, w) in enumerate(zip(batch8.D("rgb8"), ts, WINDOWS)):
        want = color_ref.transform_picture(t, scale_ref.area_average(D, w, BOX[1], BOX[0]))
        assert np.array_equal(got[k], tensor_ref.tensor(want, a, b, "f32", "chw")), k
