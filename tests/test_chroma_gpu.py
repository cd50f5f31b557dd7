"""Bilinear chroma upsampling on the device: the renders of images set to "bilinear"
against the existing references (display_ref, scale_ref, resample_ref, tensor_ref,
color_ref, tone_ref) fed the planes the GPU decoded with Cb and Cr upsampled by chroma_ref,
as a 4:4:4 picture.  Every comparison is exact.  The pictures are the small ones of
test_display_gpu: partial tiles on both paths of k_render, odd phases, the picture's edge."""
import numpy as np
import pytest

import chroma_ref
import color_ref
import display_ref
import resample_ref
import scale_ref
import tensor_ref
import tone_ref
from test_display_gpu import ORIENTATIONS, boxes, host, planes, render_raw

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


@pytest.fixture(scope="module")
def decoded(H, S):
    """Pictures decoded once and shared (never written to): get(seed, **params) -> (params, image)."""
    cache = {}

    def get(seed, colr=None, **kw):
        key = (seed, colr, tuple(sorted(kw.items())))
        if key not in cache:
            p = S.SynthParams(**kw)
            cache[key] = (p, H.HeicDecoder.decode(S.display_heic(p, seed=seed, colr=colr)))
        return cache[key]

    return get


def view(H, S, o, params, steps, chroma=None, loc=None, colr=None):
    """The decoded picture `o` under another parsed image: display steps, chroma setting."""
    img = H.HeifImage.parse(S.display_heic(params, transforms=boxes(S, steps), colr=colr), chroma=chroma)
    img.chroma_loc = loc
    return H.DecodedImage(o.y, o.cb, o.cr, o.info, img)


def displayed(o, steps, fmt, loc=None):
    """display_ref's picture; loc None: replicated chroma, else C' at that location as 4:4:4."""
    y, cb, cr = planes(o)
    inf = o.info
    if loc is not None and cb is not None:
        cb, cr = chroma_ref.upsample(cb, cr, inf.chroma_format_idc, loc, inf.height, inf.width)
        assert cb.shape == y.shape
    return display_ref.render(y, cb, cr, inf.matrix_coeffs, bool(inf.full_range), inf.bit_depth, steps, fmt)


SIZES = {"130x72": dict(width=136, height=72, conf_right=6), "262x24": dict(width=264, height=24, conf_right=2)}


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("loc", [0, 1, 4])
@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
def test_render_all_orientations(H, S, ctx, decoded, size, loc, fmt):
    p, o = decoded(3, **SIZES[size])
    outs = [view(H, S, o, p, steps, "bilinear", loc) for steps in ORIENTATIONS]
    got = ctx.render(outs, fmt)  # the eight orientations in one call
    for steps, g in zip(ORIENTATIONS, got):
        assert np.array_equal(host(g), displayed(o, steps, fmt, loc)), steps
    assert not np.array_equal(host(got[0]), displayed(o, ORIENTATIONS[0], fmt))  # not the replicated picture


def test_taps_cross_an_odd_clap(H, S, ctx, decoded):
    p, o = decoded(21, width=64, height=48)
    clap = ("clap", (41, 1, 29, 1, -13, 2, -13, 2))  # left 5, top 3: the taps read real samples outside the crop
    orients = [[clap], [clap, ("irot", 1)], [("irot", 3), ("clap", (29, 1, 41, 1, -9, 2, 7, 2)), ("imir", 0)]]
    for loc in (0, 1, 5):
        outs = [view(H, S, o, p, steps, "bilinear", loc) for steps in orients]
        for steps, g in zip(orients, ctx.render(outs, "rgb8")):
            assert np.array_equal(host(g), displayed(o, steps, "rgb8", loc)), (steps, loc)


@pytest.mark.parametrize("loc", range(6))
def test_picture_edge_clamps(H, S, ctx, decoded, loc):
    """66 x 38: chroma planes of 33 x 19, the last luma column and row tap past them."""
    p, o = decoded(9, width=72, height=40, conf_right=6, conf_bottom=2)
    assert (o.info.width, o.info.height) == (66, 38) and tuple(o.cb.shape) == (19, 33)
    orients = [[], [("irot", 1)], [("imir", 1)]]
    outs = [view(H, S, o, p, steps, "bilinear", loc) for steps in orients]
    for steps, g in zip(orients, ctx.render(outs, "rgb8")):
        assert np.array_equal(host(g), displayed(o, steps, "rgb8", loc)), steps


@pytest.mark.parametrize("chroma, depth, fmt", [(1, 10, "rgb16"), (1, 10, "rgb8"), (2, 8, "rgb8"), (2, 8, "rgba16"), (2, 12, "rgb16")])
def test_depths_and_422(H, S, ctx, decoded, chroma, depth, fmt):
    p, o = decoded(10 + chroma, width=72, height=40, conf_right=6, chroma_format=chroma, bit_depth=depth)
    orients = [[("imir", 0)], [("irot", 1), ("imir", 1)]]
    for loc in (1, 4):
        outs = [view(H, S, o, p, steps, "bilinear", loc) for steps in orients]
        for steps, g in zip(orients, ctx.render(outs, fmt)):
            assert np.array_equal(host(g), displayed(o, steps, fmt, loc)), (steps, loc)
    if chroma == 2:  # 4:2:2 is co-sited with no vertical filter whatever the location says
        assert np.array_equal(displayed(o, [], fmt, 1), displayed(o, [], fmt, 4))


@pytest.mark.parametrize("fmt", ["rgb8", "rgb16"])
def test_unaligned_pitch_keeps_padding(H, S, ctx, decoded, fmt):
    p, o = decoded(4, width=136, height=72, conf_right=6, bit_depth=10)
    orients = [[], [("irot", 1)], [("imir", 0)]]
    outs = [view(H, S, o, p, steps, "bilinear", 1) for steps in orients]
    wide = fmt.endswith("16")
    bpp = 3 * (2 if wide else 1)
    pad = [(-(w * bpp) % 4) + (6 if wide else 5) for w in (130, 72, 130)]
    rc, bufs = render_raw(H, ctx, outs, fmt, pad)
    assert rc == 0
    for steps, b, pd in zip(orients, bufs, pad):
        want = displayed(o, steps, fmt, 1)
        row = want.shape[1] * bpp
        got = np.ascontiguousarray(b[:, :row]).view(want.dtype).reshape(want.shape)
        assert np.array_equal(got, want), steps
        assert (b[:, row:] == 0xA5).all(), steps


def test_mixed_batch_each_image_its_own_rule(H, S, ctx, decoded):
    p1, o1 = decoded(3, **SIZES["130x72"])
    p3, o3 = decoded(5, width=72, height=40, conf_right=5, chroma_format=3)
    p0, o0 = decoded(6, width=48, height=32, chroma_format=0)
    outs = [view(H, S, o1, p1, [("irot", 1)], "bilinear", 1), view(H, S, o1, p1, [("irot", 1)]),
            view(H, S, o3, p3, [("imir", 0)], "bilinear", 1), view(H, S, o1, p1, [], "bilinear", 4),
            view(H, S, o0, p0, [], "bilinear")]
    got = [host(g) for g in ctx.render(outs, "rgb8")]
    assert np.array_equal(got[0], displayed(o1, [("irot", 1)], "rgb8", 1))
    assert np.array_equal(got[1], displayed(o1, [("irot", 1)], "rgb8"))  # replicate, beside bilinear ones
    assert np.array_equal(got[2], displayed(o3, [("imir", 0)], "rgb8"))
    assert np.array_equal(got[3], displayed(o1, [], "rgb8", 4))
    assert np.array_equal(got[4], displayed(o0, [], "rgb8"))
    assert not np.array_equal(got[0], got[1])
    # a call with only a 4:4:4 image set to bilinear: its replicate output
    alone = ctx.render([outs[2]], "rgb8")[0]
    assert np.array_equal(host(alone), host(ctx.render([view(H, S, o3, p3, [("imir", 0)])], "rgb8")[0]))


# ---- k_render_scaled, the tensor epilogue ---------------------------------------------------
def averaged(D, scale):
    ow, oh, x, y, w, h = scale
    return scale_ref.area_average(D, (x, y, w, h) if w or h else None, ow, oh)


@pytest.mark.parametrize("size", [(17, 23), (64, 64)])
def test_scaled_cover(H, S, ctx, decoded, size):
    p, o = decoded(3, **SIZES["130x72"])
    p2, o2 = decoded(12, width=72, height=40, conf_right=6, chroma_format=2)
    cases = [(o, p, [], 1), (o, p, [("irot", 1)], 0), (o, p, [("irot", 2), ("imir", 0)], 4), (o2, p2, [("irot", 3)], 0),
             (o, p, [("imir", 1)], None)]  # (the last one replicates, in the same call)
    outs = [view(H, S, oo, pp, steps, "bilinear" if loc is not None else None, loc) for oo, pp, steps, loc in cases]
    got = ctx.render_scaled(outs, size, "cover", "rgb8")
    for k, (oo, pp, steps, loc) in enumerate(cases):
        D = displayed(oo, steps, "rgb8", loc)
        sc = scale_ref.fit(D.shape[1], D.shape[0], size[1], size[0], "cover")
        assert np.array_equal(host(got[k]), averaged(D, sc)), (steps, loc)


def test_scaled_windows_with_odd_origins(H, S, ctx, decoded):
    p, o = decoded(3, **SIZES["130x72"])
    p10, o10 = decoded(4, width=136, height=72, conf_right=6, bit_depth=10)
    for oo, pp, fmt in ((o, p, "rgba8"), (o10, p10, "rgb16")):
        cases = [([], (5, 3, 121, 65), 2), ([("irot", 1)], (1, 7, 67, 119), 1), ([("imir", 0)], (129, 71, 1, 1), 5),
                 ([("irot", 3), ("imir", 1)], (0, 0, 72, 130), 0), ([], (63, 1, 3, 70), 1)]
        outs = [view(H, S, oo, pp, steps, "bilinear", loc) for steps, _, loc in cases]
        got = ctx.render_scaled(outs, (13, 29), fmt=fmt, windows=[w for _, w, _ in cases])
        for k, (steps, w, loc) in enumerate(cases):
            D = displayed(oo, steps, fmt, loc)
            assert np.array_equal(host(got[k]), scale_ref.area_average(D, w, 29, 13)), (fmt, steps, w)


def test_tensor_f16_chw_with_flip(H, S, ctx, decoded):
    p, o = decoded(3, **SIZES["130x72"])
    cases = [([], 1, 1), ([("irot", 1)], 3, 4), ([("imir", 0)], 2, 0)]
    outs = [view(H, S, o, p, steps, "bilinear", loc) for steps, _, loc in cases]
    got = ctx.render_tensor(outs, (24, 16), "cover", torch.float16, "chw", flips=[f for _, f, _ in cases])
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    for k, (steps, flip, loc) in enumerate(cases):
        D = displayed(o, steps, "rgb8", loc)
        R = averaged(D, scale_ref.fit(D.shape[1], D.shape[0], 16, 24, "cover"))
        bits = got[k].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(bits, tensor_ref.tensor(R, a, b, "f16", "chw", flip=flip)), steps


# ---- k_render_resampled -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bilinear", "bicubic"])
@pytest.mark.parametrize("size", [(19, 31), (150, 200)], ids=["reduce", "enlarge"])
def test_resampled(H, S, ctx, decoded, name, size):
    p, o = decoded(3, **SIZES["130x72"])
    cases = [([], None, 1), ([("irot", 1)], (3, 5, 61, 99), 4), ([("imir", 0)], (1, 1, 127, 69), 0)]
    for steps, w, loc in cases:
        out = view(H, S, o, p, steps, "bilinear", loc)
        D = displayed(o, steps, "rgb8", loc)
        if w is None:
            got = ctx.render_scaled([out], size, "stretch", "rgb8", filter=name)[0]
        else:
            got = ctx.render_scaled([out], size, fmt="rgb8", windows=[w], filter=name)[0]
        assert np.array_equal(host(got), resample_ref.resize(D, w, size[1], size[0], name, 8)), (steps, w)


# ---- the colour and tone stages behind it ---------------------------------------------------
def test_colorspace_srgb(H, S, ctx, decoded):
    colr = S.nclx_box(12, 13, 6, True)  # Display P3 primaries, sRGB transfer
    p, o = decoded(52, colr=colr, width=72, height=40, conf_right=6)
    out = view(H, S, o, p, [("irot", 1)], "bilinear", 1, colr=colr)
    t = out.image.color_transform("srgb", 8)
    D = displayed(o, [("irot", 1)], "rgb8", 1)
    want = color_ref.transform_picture(t, D)
    assert (want != D).any()
    assert np.array_equal(host(ctx.render([out], "rgb8", colorspace="srgb")[0]), want)
    R = averaged(D, scale_ref.fit(D.shape[1], D.shape[0], 20, 30, "cover"))
    assert np.array_equal(host(ctx.render_scaled([out], (30, 20), "cover", "rgb8", colorspace="srgb")[0]),
                          color_ref.transform_picture(t, R))


def test_tone_map_bt2390(H, S, ctx, decoded):
    colr = S.nclx_box(9, 16, 9, False)  # BT.2020 PQ
    p, o = decoded(61, colr=colr, width=72, height=40, conf_right=6)
    out = view(H, S, o, p, [("imir", 0)], "bilinear", 0, colr=colr)
    t = out.image.color_transform("srgb", 8, "bt2390")
    assert tone_ref.is_tone(t)
    D = displayed(o, [("imir", 0)], "rgb8", 0)
    got = ctx.render([out], "rgb8", colorspace="srgb", tone_map="bt2390")[0]
    assert np.array_equal(host(got), tone_ref.transform_picture(t, D))
    got = ctx.render_scaled([out], (30, 20), "stretch", "rgb8", colorspace="srgb", tone_map="bt2390", filter="bilinear")[0]
    assert np.array_equal(host(got), tone_ref.transform_picture(t, resample_ref.resize(D, None, 20, 30, "bilinear", 8)))


# ---- the signalled location, the one-file calls ---------------------------------------------
def test_signalled_location_is_used(H, S, ctx):
    p = S.SynthParams(width=72, height=40, conf_right=6, chroma_loc=1)
    f = S.single_heic(p, seed=8)
    o = H.HeicDecoder.decode(f)
    assert o.image.chroma.signalled and o.image.chroma.loc == 1
    shown = H.HeicDecoder.decode_display(f, chroma="bilinear")  # no override: the stream's location
    assert np.array_equal(host(shown), displayed(o, [], "rgb8", 1))
    assert not np.array_equal(host(shown), displayed(o, [], "rgb8", 0))
    assert np.array_equal(host(H.HeicDecoder.decode_display(f, chroma="bilinear", chroma_loc=0)), displayed(o, [], "rgb8", 0))
    assert np.array_equal(host(H.HeicDecoder.decode_display(f)), displayed(o, [], "rgb8"))  # the default replicates
    t = H.HeicDecoder.decode_tensor(f, (20, 33), "stretch", chroma="bilinear", dtype=torch.float32)
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    R = scale_ref.area_average(displayed(o, [], "rgb8", 1), None, 33, 20)
    assert np.array_equal(t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32), tensor_ref.tensor(R, a, b, "f32", "chw"))


def test_window_decode_takes_the_tapped_tiles(H, S, ctx):
    """A 2 x 2 grid of 64 x 64 tiles, cropped to img[64:104, 64:104]: at location 1 the first
    column taps chroma column 31, in the tiles to the left; the rows tap the tiles above."""
    p = S.SynthParams(width=64, height=64, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=2)
    clap = ("clap", (40, 1, 40, 1, 20, 1, 20, 1))
    assert display_ref.clap_rect(128, 128, clap[1]) == (64, 64, 40, 40)
    f = S.grid_heic(128, 128, p, seed=11, transforms=boxes(S, [clap]))
    rep, bil = H.HeifImage.parse(f), H.HeifImage.parse(f, chroma="bilinear")
    bil.chroma_loc = 1
    assert rep.tiles_for(rep.source_rect()) == (1, 1, 1, 1) and bil.tiles_for(bil.source_rect()) == (0, 0, 2, 2)
    full = H.HeicDecoder.decode(f)
    want = displayed(full, [clap], "rgb8", 1)
    for tiles in ("all", "window"):
        got = H.HeicDecoder.decode_display(f, tiles=tiles, chroma="bilinear", chroma_loc=1)
        assert np.array_equal(host(got), want), tiles
    # the planes of a decode prepared for the replicate rectangle do not hold what a bilinear render reads
    outs = ctx.alloc_outputs([bil])
    batch = ctx.prepare([bil], rects=[rep.source_rect()])
    try:
        assert batch.pictures == 1
        batch.decode_async(outs)
        assert batch.status() == [0]
    finally:
        batch.free()
    with pytest.raises(ValueError, match="was decoded for the rectangle"):
        ctx.render(outs, "rgb8")
    with pytest.raises(ValueError, match="was decoded for the rectangle"):
        ctx.render_scaled(outs, (10, 10), "stretch")
    bil.chroma_upsampling = "replicate"  # the same planes serve the replicate render
    assert np.array_equal(host(ctx.render(outs, "rgb8")[0]), displayed(full, [clap], "rgb8"))


def test_default_is_untouched(H, S, ctx, decoded):
    p, o = decoded(3, **SIZES["130x72"])
    out = view(H, S, o, p, [("irot", 1)])
    assert out.image.chroma_upsampling == "replicate"
    D = displayed(o, [("irot", 1)], "rgb8")
    assert np.array_equal(host(ctx.render([out], "rgb8")[0]), D)
    R = averaged(D, scale_ref.fit(D.shape[1], D.shape[0], 23, 17, "cover"))
    assert np.array_equal(host(ctx.render_scaled([out], (17, 23), "cover", "rgb8")[0]), R)
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    t = ctx.render_tensor([out], (17, 23), "cover", torch.float32, "hwc")[0]
    assert np.array_equal(t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32), tensor_ref.tensor(R, a, b, "f32", "hwc"))
