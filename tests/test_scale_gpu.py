"""The scaled render on the device: heifgpu_render_batch_scaled /
DecodeContext.render_scaled against scale_ref.area_average of the displayed
picture display_ref.render builds from the planes the GPU decoded, so only
k_render_scaled is under test.  Every comparison is exact.  The pictures are a
few CTBs each; the sizes are the smallest at which the kernel can go wrong:
partial tiles on both of its paths (8 x 64..256 output pixels for maps that
keep the axes, 64 x 64 for those that swap them), footprints that end inside a
source column pair and an odd chroma phase, non-integer, 2:1, identity,
enlarging and degenerate ratios, unaligned pitches.  Two cases need their size:
the 64-bit sum (a 12-bit picture of 1.5 megapixels whose planes the test
fills) and halfmoonbay's 12 megapixels through the chunk loops."""
import ctypes

import numpy as np
import pytest

import display_ref
import scale_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMATS = ("rgb8", "rgba8", "rgb16", "rgba16")
ORIENTATIONS = [[("irot", k)] + m for k in range(4) for m in ([], [("imir", 0)])]


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


def boxes(S, steps):
    make = {"clap": lambda a: S.clap_box(*a), "irot": S.irot_box, "imir": S.imir_box}
    return tuple(make[k](a) for k, a in steps)


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def displayed(o, steps, fmt, alpha=None):
    """D: the displayed picture of the decoded planes, by display_ref."""
    y, cb, cr = [None if t is None else host(t) for t in (o.y, o.cb, o.cr)]
    inf = o.info
    return display_ref.render(y, cb, cr, inf.matrix_coeffs, bool(inf.full_range), inf.bit_depth, steps, fmt,
                              alpha=None if alpha is None else host(alpha.y),
                              alpha_depth=8 if alpha is None else alpha.info.bit_depth)


def with_steps(H, S, o, params, steps, **kw):
    """The decoded picture `o` as the primary of a file that carries `steps`."""
    img = H.HeifImage.parse(S.display_heic(params, transforms=boxes(S, steps), **kw))
    return H.DecodedImage(o.y, o.cb, o.cr, o.info, img)


def bytes_per_pixel(fmt):
    return (4 if fmt.startswith("rgba") else 3) * (2 if fmt.endswith("16") else 1)


def scaled_raw(H, ctx, outs, fmt, scales, pad=None, alphas=None, sentinel=0xA5, sync=True):
    """heifgpu_render_batch_scaled with scales[i] = (ow, oh, x, y, w, h) into
    sentinel-filled buffers whose pitch is the row plus pad[i] bytes; returns
    (rc, [buffer as (oh, pitch) uint8 device tensor])."""
    from heif_amd import _lib

    f = _lib.PIX_FORMATS[fmt]
    bpp, n = bytes_per_pixel(fmt), len(outs)
    surf, sc, bufs = (_lib.Surface * n)(), (_lib.Scale * n)(), []
    for i in range(n):
        sc[i] = _lib.Scale(*scales[i])
        pitch = scales[i][0] * bpp + (pad[i] if pad else 0)
        b = torch.full((scales[i][1], pitch), sentinel, dtype=torch.uint8, device="cuda:0")
        surf[i].pixels, surf[i].pitch = b.data_ptr(), pitch
        bufs.append(b)
    imgs = (ctypes.c_void_p * n)(*[o.image._h.value for o in outs])
    aimgs = aplanes = None
    if alphas is not None:
        aimgs = (ctypes.c_void_p * n)(*[a.image._h.value if a is not None else None for a in alphas])
        aplanes = (_lib.Planes * n)()
        for i, a in enumerate(alphas):
            if a is not None:
                aplanes[i].plane[0] = a.y.data_ptr()
                aplanes[i].pitch[0] = a.y.stride(0) * a.y.element_size()
    rc = _lib.lib.heifgpu_render_batch_scaled(ctx._h, imgs, n, H.DecodeContext.planes_of(outs), aimgs, aplanes, f, sc,
                                              surf, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    if sync:
        torch.cuda.synchronize()
    return rc, bufs


def pixels(buf, ow, fmt):
    """The (oh, ow, C) pixels of a buffer scaled_raw filled, and its pad bytes."""
    b = buf.cpu().numpy()
    row = ow * bytes_per_pixel(fmt)
    px = np.ascontiguousarray(b[:, :row]).view(np.uint16 if fmt.endswith("16") else np.uint8)
    return px.reshape(b.shape[0], ow, 4 if fmt.startswith("rgba") else 3), b[:, row:]


def want(D, scale):
    ow, oh, x, y, w, h = scale
    return scale_ref.area_average(D, (x, y, w, h) if w or h else None, ow, oh)


@pytest.fixture(scope="module")
def decoded(H, S):
    """Pictures decoded once and shared (never written to)."""
    cache = {}

    def get(seed, **kw):
        key = (seed, tuple(sorted(kw.items())))
        if key not in cache:
            p = S.SynthParams(**kw)
            cache[key] = (p, H.HeicDecoder.decode(S.single_heic(p, seed=seed)))
        return cache[key]

    return get


# 37 x 19: no integer ratio, partial tiles; 65 x 36: 2:1 of 130 x 72; 130 x 72: its identity;
# then the degenerate sides.  None: the picture's own size (identity for both pictures).
TARGETS = [(37, 19), (65, 36), (130, 72), (1, 1), (1, 72), (130, 1), None]


@pytest.mark.parametrize("size", [dict(width=136, height=72, conf_right=6),   # 130 x 72: 3 x 2 tiles when swapped
                                  dict(width=264, height=24, conf_right=2)],  # 262 x 24: 2 tiles along x at identity
                         ids=["130x72", "262x24"])
def test_sizes_all_orientations(H, S, ctx, decoded, size):
    p, o = decoded(3, **size)
    outs = [with_steps(H, S, o, p, steps) for steps in ORIENTATIONS]
    Ds = [displayed(o, steps, "rgb8") for steps in ORIENTATIONS]
    full = ctx.render(outs, "rgb8")
    for target in TARGETS:
        scales = []
        for k, out in enumerate(outs):
            d = out.image.display
            tw, th = target or (d.out_width, d.out_height)
            if target and k in (2, 3, 6, 7):  # irot 1 and 3 show the picture turned: turn the target with it
                tw, th = th, tw
            scales.append((tw, th, 0, 0, 0, 0))
        rc, bufs = scaled_raw(H, ctx, outs, "rgb8", scales)  # the eight orientations in one call
        assert rc == 0
        for steps, D, b, sc, f in zip(ORIENTATIONS, Ds, bufs, scales, full):
            got, _ = pixels(b, sc[0], "rgb8")
            assert np.array_equal(got, want(D, sc)), (target, steps)
            if target is None:  # identity: heifgpu_render_batch bit for bit
                assert np.array_equal(got, host(f)), steps


def test_enlargement(H, S, ctx, decoded):
    p, o = decoded(21, width=64, height=48)
    orients = [[], [("irot", 1)], [("irot", 2), ("imir", 1)]]
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    scales = [(64, 48, 5, 3, 41, 29), (48, 64, 3, 5, 29, 41), (64, 48, 5, 3, 41, 29)]
    rc, bufs = scaled_raw(H, ctx, outs, "rgb8", scales)
    assert rc == 0
    for steps, b, sc in zip(orients, bufs, scales):
        assert np.array_equal(pixels(b, sc[0], "rgb8")[0], want(displayed(o, steps, "rgb8"), sc)), steps


def test_odd_phase_window_on_420(H, S, ctx, decoded):
    p, o = decoded(21, width=64, height=48)
    clap = ("clap", (41, 1, 29, 1, -13, 2, -13, 2))  # left 5, top 3: both odd on 4:2:0
    assert display_ref.clap_rect(64, 48, clap[1]) == (5, 3, 41, 29)
    # the window alone; behind the odd clap (a window of it); behind the clap and a turn
    cases = [([], (17, 11, 5, 3, 41, 29)), ([clap], (17, 11, 0, 0, 0, 0)), ([clap], (7, 5, 3, 2, 21, 16)),
             ([clap, ("irot", 1)], (11, 17, 0, 0, 0, 0)), ([clap, ("irot", 1)], (5, 7, 2, 3, 16, 21))]
    outs = [with_steps(H, S, o, p, steps) for steps, _ in cases]
    rc, bufs = scaled_raw(H, ctx, outs, "rgb8", [sc for _, sc in cases])
    assert rc == 0
    res = [pixels(b, sc[0], "rgb8")[0] for b, (_, sc) in zip(bufs, cases)]
    for (steps, sc), got in zip(cases, res):
        assert np.array_equal(got, want(displayed(o, steps, "rgb8"), sc)), (steps, sc)
    assert np.array_equal(res[0], res[1])  # the window of the picture is the whole of the clapped one


@pytest.mark.parametrize("chroma, depth", [(c, d) for c in (0, 1, 2, 3) for d in (8, 10, 12)])
def test_formats_and_chroma(H, S, ctx, decoded, chroma, depth):
    # a 67-wide displayed picture (66 for the subsampled formats, which crop by whole chroma samples) to 23 x 13
    p, o = decoded(10 + chroma, width=72, height=40, conf_right=5 if chroma in (0, 3) else 6, chroma_format=chroma,
                   bit_depth=depth)
    assert o.info.bit_depth == depth and o.info.chroma_format_idc == chroma
    orients = [[("imir", 0)], [("irot", 1), ("imir", 1)]]  # one that keeps the axes, one that swaps them
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    for fmt in FORMATS:
        got = ctx.render_scaled(outs, (13, 23), "stretch", fmt)
        assert tuple(got.shape) == (2, 13, 23, 4 if fmt.startswith("rgba") else 3)
        assert got.dtype == (torch.int16 if fmt.endswith("16") else torch.uint8)
        for steps, g in zip(orients, host(got)):
            w = scale_ref.area_average(displayed(o, steps, fmt), None, 23, 13)
            assert np.array_equal(g, w), (fmt, steps)
            if chroma == 0:
                assert (w[..., 0] == w[..., 1]).all() and (w[..., 0] == w[..., 2]).all()
            if fmt.startswith("rgba"):
                assert (g[..., 3] == ((1 << depth) - 1 if fmt.endswith("16") else 255)).all()  # opaque stays opaque


def test_alpha_is_averaged(H, S, ctx):
    p = S.SynthParams(width=64, height=48, bit_depth=10)
    a = S.SynthParams(width=64, height=48, chroma_format=0, bit_depth=12)
    steps = [("clap", (41, 1, 29, 1, -13, 2, -13, 2)), ("imir", 0), ("irot", 1)]
    f = S.display_heic(p, seed=40, transforms=boxes(S, steps), aux=(S.AuxImage(a, seed=41, urn=S.ALPHA_URN_MPEGB),))
    o, al = H.HeicDecoder.decode(f), H.HeicDecoder.decode(f, item_id=2)
    assert o.image.display.alpha_item_id == 2 and al.info.bit_depth == 12
    opaque = with_steps(H, S, o, p, [("imir", 1)])  # the same planes, no alpha, in the same batch
    for fmt in ("rgba8", "rgba16"):
        scales = [(11, 17, 0, 0, 0, 0), (23, 13, 0, 0, 0, 0)]
        rc, bufs = scaled_raw(H, ctx, [o, opaque], fmt, scales, alphas=[al, None])
        assert rc == 0
        w0 = want(displayed(o, steps, fmt, alpha=al), scales[0])
        assert np.array_equal(pixels(bufs[0], 11, fmt)[0], w0), fmt
        assert len(np.unique(w0[..., 3])) > 4  # a real alpha plane, not a constant
        g1 = pixels(bufs[1], 23, fmt)[0]
        assert np.array_equal(g1, want(displayed(o, [("imir", 1)], fmt), scales[1])), fmt
        assert (g1[..., 3] == (1023 if fmt == "rgba16" else 255)).all()


def test_sum_above_32_bits(H, S, ctx):
    """12-bit samples over 1.5 megapixels: the sum passes 2^32 (4095 * 1536 * 1024
    = 1.5 * 2^32).  The planes are filled here, under a parsed header."""
    p = S.SynthParams(width=1536, height=1024, chroma_format=3, bit_depth=12)
    img = H.HeifImage.parse(S.display_heic(p, colr=S.nclx_box(1, 1, 6, True)))  # BT.601, full range
    inf = img.info
    assert (inf.width, inf.height, inf.bit_depth, inf.full_range, inf.chroma_format_idc) == (1536, 1024, 12, 1, 3)
    dev = torch.device("cuda", 0)
    grey = torch.full((1024, 1536), 2048, dtype=torch.int16, device=dev)
    y = torch.full((1024, 1536), 4095, dtype=torch.int16, device=dev)
    o = H.DecodedImage(y, grey, grey, inf, img)
    for size in ((1, 1), (2, 3)):
        got = host(ctx.render_scaled([o], size, "stretch", "rgb16"))
        assert got.shape == (1, size[0], size[1], 3) and (got == 4095).all(), (size, got)
    # a 0 / 4095 checkerboard of period 2: the mean is 2047.5, round half up 2048 (2047 rounds down; a wrapped sum
    # gives something else altogether)
    yy, xx = torch.meshgrid(torch.arange(1024, device=dev), torch.arange(1536, device=dev), indexing="ij")
    o = H.DecodedImage((((yy + xx) & 1) * 4095).to(torch.int16), grey, grey, inf, img)
    for size in ((1, 1), (2, 3)):
        got = host(ctx.render_scaled([o], size, "stretch", "rgb16"))
        assert (got == 2048).all(), (size, got)


def test_mixed_batch_one_call(H, S, ctx):
    """Three images that differ in size, orientation, chroma format, matrix and
    ratio (a reduction, an identity, an enlargement) in one call."""
    specs = [
        (S.SynthParams(width=136, height=72, conf_right=6), [("irot", 1)], S.nclx_box(1, 1, 6, True), (31, 50, 3, 7, 60, 111)),
        (S.SynthParams(width=72, height=40, conf_right=5, chroma_format=3), [("imir", 0)], S.nclx_box(1, 1, 1, False),
         (67, 40, 0, 0, 0, 0)),
        (S.SynthParams(width=48, height=32, chroma_format=0), [("clap", (27, 1, 22, 1, -5, 2, 3, 1)), ("irot", 2)], None,
         (40, 33, 0, 0, 0, 0)),
    ]
    outs = [H.HeicDecoder.decode(S.display_heic(p, seed=30 + k, transforms=boxes(S, steps), colr=colr))
            for k, (p, steps, colr, _) in enumerate(specs)]
    assert (outs[0].info.matrix_coeffs, outs[0].info.full_range) == (6, 1)
    assert (outs[1].info.matrix_coeffs, outs[1].info.full_range) == (1, 0)
    assert (outs[2].image.display.out_width, outs[2].image.display.out_height) == (27, 22)
    rc, bufs = scaled_raw(H, ctx, outs, "rgb8", [sc for *_, sc in specs])
    assert rc == 0
    for (p, steps, _, sc), o, b in zip(specs, outs, bufs):
        assert np.array_equal(pixels(b, sc[0], "rgb8")[0], want(displayed(o, steps, "rgb8"), sc)), steps
    assert np.array_equal(pixels(bufs[1], 67, "rgb8")[0], host(ctx.render([outs[1]], "rgb8")[0]))  # the identity


@pytest.mark.parametrize("fmt", FORMATS)
def test_unaligned_pitch_keeps_padding(H, S, ctx, decoded, fmt):
    p, o = decoded(4, width=136, height=72, conf_right=6, bit_depth=10)
    orients = [[], [("irot", 1)], [("imir", 0)]]
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    wide, bpp = fmt.endswith("16"), bytes_per_pixel(fmt)
    scales = [(37, 19, 0, 0, 0, 0), (19, 37, 0, 0, 0, 0), (130, 72, 0, 0, 0, 0)]
    # pitch = 1 mod 4 (2 mod 4 for 16-bit samples): most rows start off a dword, and the pitch exceeds the row
    pad = [(-(sc[0] * bpp) % 4) + (6 if wide else 5) for sc in scales]
    rc, bufs = scaled_raw(H, ctx, outs, fmt, scales, pad=pad)
    assert rc == 0
    for steps, b, sc, pd in zip(orients, bufs, scales, pad):
        got, rest = pixels(b, sc[0], fmt)
        assert rest.shape[1] == pd and b.shape[1] % 4 == (2 if wide else 1)
        assert np.array_equal(got, want(displayed(o, steps, fmt), sc)), steps
        assert (rest == 0xA5).all(), steps  # the pad bytes keep the sentinel


def test_pitch_below_row_rejected(H, S, ctx, decoded):
    p, o = decoded(21, width=64, height=48)
    rc, bufs = scaled_raw(H, ctx, [with_steps(H, S, o, p, [])], "rgb8", [(17, 11, 0, 0, 0, 0)], pad=[-1])
    assert rc == -1 and (bufs[0] == 0xA5).all()  # HEIFGPU_E_INVALID, nothing written
    rc, bufs = scaled_raw(H, ctx, [with_steps(H, S, o, p, [])], "rgb8", [(17, 11, 60, 0, 5, 5)])
    assert rc == -1 and (bufs[0] == 0xA5).all()  # a window outside the picture


def test_back_to_back_calls_keep_their_descriptors(H, S, ctx, decoded):
    """Calls issued without a host synchronise in between (more of them than the
    staging ring has slots, a full-size render between them) each render their own batch."""
    (p1, o1), (p2, o2) = decoded(3, width=136, height=72, conf_right=6), decoded(5, width=72, height=40, chroma_format=3)
    calls = []
    for k in range(6):
        s1, s2 = ORIENTATIONS[k], ORIENTATIONS[7 - k]
        batch = [(o1, p1, s1, (37 - k, 19 + k, 0, 0, 0, 0)), (o2, p2, s2, (13 + k, 9, k, 1, 30, 33))][::1 if k % 2 else -1]
        calls.append(([with_steps(H, S, o, p, s) for o, p, s, _ in batch], batch))
    torch.cuda.synchronize()
    results = []
    for k, (outs, batch) in enumerate(calls):  # six launches queued, no synchronise between them
        results.append(scaled_raw(H, ctx, outs, "rgb8", [sc for *_, sc in batch], sync=False))
        if k == 2:
            full = ctx.render(outs, "rgb8")  # shares the ring
    torch.cuda.synchronize()
    for (outs, batch), (rc, bufs) in zip(calls, results):
        assert rc == 0
        for (o, p, steps, sc), b in zip(batch, bufs):
            assert np.array_equal(pixels(b, sc[0], "rgb8")[0], want(displayed(o, steps, "rgb8"), sc)), (steps, sc)
    for (o, p, steps, _), f in zip(calls[2][1], full):
        assert np.array_equal(host(f), displayed(o, steps, "rgb8"))


def test_python_surface(H, S, ctx):
    files = [S.display_heic(S.SynthParams(width=136, height=72, conf_right=6), seed=60, transforms=boxes(S, [("irot", 1)])),
             S.display_heic(S.SynthParams(width=72, height=40, conf_right=5, chroma_format=3), seed=61)]
    outs = [H.HeicDecoder.decode(f) for f in files]
    Ds = [displayed(outs[0], [("irot", 1)], "rgb8"), displayed(outs[1], [], "rgb8")]
    dims = [(72, 130), (67, 40)]
    cover = ctx.render_scaled(outs, (16, 24), mode="cover")
    assert tuple(cover.shape) == (2, 16, 24, 3) and cover.dtype == torch.uint8 and cover.is_contiguous()
    for g, D, (dw, dh) in zip(host(cover), Ds, dims):
        assert np.array_equal(g, want(D, scale_ref.fit(dw, dh, 24, 16, "cover")))
    contain = ctx.render_scaled(outs, (16, 24), mode="contain")
    assert isinstance(contain, list) and len(contain) == 2
    for g, D, (dw, dh) in zip(contain, Ds, dims):
        sc = scale_ref.fit(dw, dh, 24, 16, "contain")
        assert tuple(g.shape) == (sc[1], sc[0], 3)
        assert np.array_equal(host(g), want(D, sc))
    assert [tuple(g.shape[:2]) for g in contain] == [(16, 9), (14, 24)]
    windows = [(3, 7, 60, 111), (1, 2, 41, 29)]
    win = ctx.render_scaled(outs, (16, 24), windows=windows, fmt="rgba8")
    assert tuple(win.shape) == (2, 16, 24, 4)
    for g, o, st, w in zip(host(win), outs, ([("irot", 1)], []), windows):
        assert np.array_equal(g, want(displayed(o, st, "rgba8"), (24, 16) + w))
    # decode_display(size=): "contain" unless told otherwise, as the two above
    shown = H.HeicDecoder.decode_display(files[0], size=(16, 24))
    assert torch.equal(shown, contain[0])
    assert torch.equal(H.HeicDecoder.decode_display(files[1], size=(16, 24), mode="cover"), cover[1])
    assert tuple(H.HeicDecoder.decode_display(files[0]).shape) == (130, 72, 3)  # size None: unchanged
    with pytest.raises(ValueError):
        ctx.render_scaled(outs, (16, 24), mode="fill")
    with pytest.raises(H.HeifGpuError):
        ctx.render_scaled(outs, (16, 24), windows=[(0, 0, 73, 1), (0, 0, 1, 1)])


def test_halfmoonbay_cover_and_contain(H, ctx, halfmoonbay):
    """irot 3 at full size: the swapped path, 12 megapixels through the chunk
    loops, against the checker fed with heifgpu_render_batch's own output."""
    o = H.HeicDecoder.decode(halfmoonbay)
    D = host(ctx.render([o], "rgb8")[0])
    assert D.shape == (4032, 3024, 3)
    cover = ctx.render_scaled([o], (224, 224), mode="cover")
    sc = scale_ref.fit(3024, 4032, 224, 224, "cover")
    assert sc == (224, 224, 0, 504, 3024, 3024)
    assert np.array_equal(host(cover)[0], want(D, sc))
    contain = ctx.render_scaled([o], (512, 512), mode="contain")
    assert tuple(contain[0].shape) == (512, 384, 3)
    assert np.array_equal(host(contain[0]), scale_ref.area_average(D, None, 384, 512))
    assert torch.equal(H.HeicDecoder.decode_display(halfmoonbay, size=(512, 512)), contain[0])
