"""The filtered renders on the device: heifgpu_render_batch_resampled /
heifgpu_render_batch_tensor_resampled (render_scaled / render_tensor with
filter=) against resample_ref.resize, the numpy restatement of Pillow's
antialiased BILINEAR / BICUBIC that tests/test_resample.py pins to Pillow, over
the displayed picture display_ref.render builds from the planes the GPU decoded,
so only k_render_resampled is under test.  Every comparison is exact.

The kernel takes 64 x 16 stored pixels per workgroup, walks D in chunks of 16
rows x 256 columns and takes as many of its 64 columns together as fit a chunk.
The pictures are a few CTBs each and the sizes the smallest at which it can go
wrong: partial tiles, more than one tile along both axes, every orientation,
reduction, identity, enlargement and degenerate sides, a picture just wider than
a chunk, hard edges for both clips, unaligned pitches.  One case has the
workload's size: halfmoonbay's 12 megapixels to 224 x 224."""
import ctypes

import numpy as np
import pytest

import color_ref
import display_ref
import resample_ref as R
import tensor_ref

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


def resampled_raw(H, ctx, outs, fmt, scales, name, pad=None, alphas=None, sentinel=0xA5, sync=True):
    """heifgpu_render_batch_resampled with scales[i] = (ow, oh, x, y, w, h) into
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
    rc = _lib.lib.heifgpu_render_batch_resampled(ctx._h, imgs, n, H.DecodeContext.planes_of(outs), aimgs, aplanes, f, sc,
                                                 R.CODES[name], None, surf,
                                                 ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    if sync:
        torch.cuda.synchronize()
    return rc, bufs


def pixels(buf, ow, fmt):
    """The (oh, ow, C) pixels of a buffer resampled_raw filled, and its pad bytes."""
    b = buf.cpu().numpy()
    row = ow * bytes_per_pixel(fmt)
    px = np.ascontiguousarray(b[:, :row]).view(np.uint16 if fmt.endswith("16") else np.uint8)
    return px.reshape(b.shape[0], ow, 4 if fmt.startswith("rgba") else 3), b[:, row:]


def depth_of(o, fmt):
    return o.info.bit_depth if fmt.endswith("16") else 8


def want(D, scale, name, bits=8):
    ow, oh, x, y, w, h = scale
    return R.resize(D, (x, y, w, h) if w or h else None, ow, oh, name, bits)


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


# 37 x 19: no integer ratio, partial tiles; 65 x 36: 2:1 of 130 x 72; then the degenerate
# sides.  None: the picture's own size (identity for both pictures).
TARGETS = [(37, 19), (65, 36), (1, 1), (1, 72), (130, 1), None]


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("size", [dict(width=136, height=72, conf_right=6),   # 130 x 72: 3 x 5 tiles at identity
                                  dict(width=264, height=24, conf_right=2)],  # 262 x 24: 5 tiles along x, two column chunks
                         ids=["130x72", "262x24"])
def test_sizes_all_orientations(H, S, ctx, decoded, size, name):
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
        rc, bufs = resampled_raw(H, ctx, outs, "rgb8", scales, name)  # the eight orientations in one call
        assert rc == 0
        for steps, D, b, sc, f in zip(ORIENTATIONS, Ds, bufs, scales, full):
            got, _ = pixels(b, sc[0], "rgb8")
            assert np.array_equal(got, want(D, sc, name)), (target, steps)
            if target is None:  # identity: heifgpu_render_batch byte for byte
                assert np.array_equal(got, host(f)), steps


@pytest.mark.parametrize("name", R.FILTERS)
def test_enlargement_from_an_odd_phase_window(H, S, ctx, decoded, name):
    """41 x 29 -> 64 x 48 from the window at (5, 3), both odd on 4:2:0; the taps reach
    into the picture around the window."""
    p, o = decoded(21, width=64, height=48)
    orients = [[], [("irot", 1)], [("irot", 2), ("imir", 1)]]
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    scales = [(64, 48, 5, 3, 41, 29), (48, 64, 3, 5, 29, 41), (64, 48, 5, 3, 41, 29)]
    rc, bufs = resampled_raw(H, ctx, outs, "rgb8", scales, name)
    assert rc == 0
    for steps, b, sc in zip(orients, bufs, scales):
        D = displayed(o, steps, "rgb8")
        got = pixels(b, sc[0], "rgb8")[0]
        assert np.array_equal(got, want(D, sc, name)), steps
        x, y, w, h = sc[2:]
        alone = R.resize(np.ascontiguousarray(D[y:y + h, x:x + w]), None, sc[0], sc[1], name)
        assert (got != alone).any()  # the halo is read: the window alone gives another picture


@pytest.mark.parametrize("chroma, depth", [(c, d) for c in (0, 1, 2, 3) for d in (8, 10, 12)])
def test_formats_and_chroma(H, S, ctx, decoded, chroma, depth):
    # a 67-wide displayed picture (66 for the subsampled formats, which crop by whole chroma samples) to 23 x 13
    p, o = decoded(10 + chroma, width=72, height=40, conf_right=5 if chroma in (0, 3) else 6, chroma_format=chroma,
                   bit_depth=depth)
    assert o.info.bit_depth == depth and o.info.chroma_format_idc == chroma
    orients = [[("imir", 0)], [("irot", 1), ("imir", 1)]]  # one that keeps the axes, one that swaps them
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    for fmt in FORMATS:
        for name in R.FILTERS:
            got = ctx.render_scaled(outs, (13, 23), "stretch", fmt, filter=name)
            assert tuple(got.shape) == (2, 13, 23, 4 if fmt.startswith("rgba") else 3)
            assert got.dtype == (torch.int16 if fmt.endswith("16") else torch.uint8)
            for steps, g in zip(orients, host(got)):
                w = R.resize(displayed(o, steps, fmt), None, 23, 13, name, depth_of(o, fmt))
                assert np.array_equal(g, w), (fmt, name, steps)
                if chroma == 0:
                    assert (w[..., 0] == w[..., 1]).all() and (w[..., 0] == w[..., 2]).all()
                if fmt.startswith("rgba"):
                    assert (g[..., 3] == ((1 << depth) - 1 if fmt.endswith("16") else 255)).all()  # opaque stays opaque


def test_alpha_is_a_channel_like_the_others(H, S, ctx):
    p = S.SynthParams(width=64, height=48, bit_depth=10)
    a = S.SynthParams(width=64, height=48, chroma_format=0, bit_depth=12)
    steps = [("clap", (41, 1, 29, 1, -13, 2, -13, 2)), ("imir", 0), ("irot", 1)]
    f = S.display_heic(p, seed=40, transforms=boxes(S, steps), aux=(S.AuxImage(a, seed=41, urn=S.ALPHA_URN_MPEGB),))
    o, al = H.HeicDecoder.decode(f), H.HeicDecoder.decode(f, item_id=2)
    assert o.image.display.alpha_item_id == 2 and al.info.bit_depth == 12
    opaque = with_steps(H, S, o, p, [("imir", 1)])  # the same planes, no alpha, in the same batch
    for fmt in ("rgba8", "rgba16"):
        bits = 10 if fmt == "rgba16" else 8
        scales = [(11, 17, 0, 0, 0, 0), (23, 13, 0, 0, 0, 0)]
        rc, bufs = resampled_raw(H, ctx, [o, opaque], fmt, scales, "bicubic", alphas=[al, None])
        assert rc == 0
        w0 = want(displayed(o, steps, fmt, alpha=al), scales[0], "bicubic", bits)
        assert np.array_equal(pixels(bufs[0], 11, fmt)[0], w0), fmt
        assert len(np.unique(w0[..., 3])) > 4  # a real alpha plane, not a constant
        g1 = pixels(bufs[1], 23, fmt)[0]
        assert np.array_equal(g1, want(displayed(o, [("imir", 1)], fmt), scales[1], "bicubic", bits)), fmt
        assert (g1[..., 3] == (1023 if fmt == "rgba16" else 255)).all()


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
    for name in R.FILTERS:
        rc, bufs = resampled_raw(H, ctx, outs, "rgb8", [sc for *_, sc in specs], name)
        assert rc == 0
        for (p, steps, _, sc), o, b in zip(specs, outs, bufs):
            assert np.array_equal(pixels(b, sc[0], "rgb8")[0], want(displayed(o, steps, "rgb8"), sc, name)), (name, steps)
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
    rc, bufs = resampled_raw(H, ctx, outs, fmt, scales, "bicubic", pad=pad)
    assert rc == 0
    for steps, b, sc, pd in zip(orients, bufs, scales, pad):
        got, rest = pixels(b, sc[0], fmt)
        assert rest.shape[1] == pd and b.shape[1] % 4 == (2 if wide else 1)
        assert np.array_equal(got, want(displayed(o, steps, fmt), sc, "bicubic", depth_of(o, fmt))), steps
        assert (rest == 0xA5).all(), steps  # the pad bytes keep the sentinel


def test_back_to_back_calls_keep_their_descriptors(H, S, ctx, decoded):
    """Six calls issued without a host synchronise in between (more than the staging ring
    has slots, an area render and a full-size render between them) each render their own batch."""
    (p1, o1), (p2, o2) = decoded(3, width=136, height=72, conf_right=6), decoded(5, width=72, height=40, chroma_format=3)
    calls = []
    for k in range(6):
        s1, s2 = ORIENTATIONS[k], ORIENTATIONS[7 - k]
        batch = [(o1, p1, s1, (37 - k, 19 + k, 0, 0, 0, 0)), (o2, p2, s2, (13 + k, 9, k, 1, 30, 33))][::1 if k % 2 else -1]
        calls.append(([with_steps(H, S, o, p, s) for o, p, s, _ in batch], batch, R.FILTERS[k & 1]))
    torch.cuda.synchronize()
    results = []
    for k, (outs, batch, name) in enumerate(calls):  # six launches queued, no synchronise between them
        results.append(resampled_raw(H, ctx, outs, "rgb8", [sc for *_, sc in batch], name, sync=False))
        if k == 2:
            full = ctx.render(outs, "rgb8")  # shares the ring
            area = ctx.render_scaled(outs, (9, 13), "stretch")
    torch.cuda.synchronize()
    for (outs, batch, name), (rc, bufs) in zip(calls, results):
        assert rc == 0
        for (o, p, steps, sc), b in zip(batch, bufs):
            assert np.array_equal(pixels(b, sc[0], "rgb8")[0], want(displayed(o, steps, "rgb8"), sc, name)), (steps, sc)
    for (o, p, steps, _), f in zip(calls[2][1], full):
        assert np.array_equal(host(f), displayed(o, steps, "rgb8"))
    assert tuple(area.shape) == (2, 9, 13, 3)


def test_hard_edges_fire_both_clips(H, S, ctx):
    """A 12-bit 4:4:4 picture whose planes the test fills with 0 / 4095 blocks under a
    parsed full-range header (grey chroma: R = G = B = Y): the bicubic overshoot clips at
    both ends in the first pass and in the second."""
    p = S.SynthParams(width=72, height=40, chroma_format=3, bit_depth=12)
    img = H.HeifImage.parse(S.display_heic(p, colr=S.nclx_box(1, 1, 6, True)))  # BT.601, full range
    inf = img.info
    assert (inf.width, inf.height, inf.bit_depth, inf.full_range, inf.chroma_format_idc) == (72, 40, 12, 1, 3)
    dev = torch.device("cuda", 0)
    yy, xx = torch.meshgrid(torch.arange(40, device=dev), torch.arange(72, device=dev), indexing="ij")
    y = ((((yy // 3) + (xx // 4)) & 1) * 4095).to(torch.int16)
    grey = torch.full((40, 72), 2048, dtype=torch.int16, device=dev)
    o = H.DecodedImage(y, grey, grey, inf, img)
    D = displayed(o, [], "rgb16")
    assert set(np.unique(D)) == {0, 4095}
    for size in ((13, 23), (60, 100), (40, 72)):
        for name in R.FILTERS:
            got = host(ctx.render_scaled([o], size, "stretch", "rgb16", filter=name))[0]
            assert np.array_equal(got, R.resize(D, None, size[1], size[0], name, 12)), (size, name)
    up = R.resize(D, None, 100, 60, "bicubic", 12)
    assert up.max() == 4095 and up.min() == 0
    assert (up != R.resize(D, None, 100, 60, "bicubic", 12, clip_mid=False)).any()
    assert (up != R.resize(D, None, 100, 60, "bicubic", 12, vertical_first=True)).any()


@pytest.mark.parametrize("name", R.FILTERS)
def test_footprint_wider_than_a_chunk(H, S, ctx, decoded, name):
    """262 x 24: six columns wider than the kernel's chunk of 256 columns of D and eight
    rows taller than its 16 rows.  To 1 x 1 and 2 x 3 every output's taps span several
    chunks along both axes (kept and swapped axes)."""
    p, o = decoded(3, width=264, height=24, conf_right=2)
    orients = [[], [("irot", 1)], [("irot", 3), ("imir", 0)]]
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    for size in ((1, 1), (2, 3)):
        scales = [(size[1], size[0], 0, 0, 0, 0), (size[0], size[1], 0, 0, 0, 0), (size[0], size[1], 0, 0, 0, 0)]
        rc, bufs = resampled_raw(H, ctx, outs, "rgb8", scales, name)
        assert rc == 0
        for steps, b, sc in zip(orients, bufs, scales):
            assert np.array_equal(pixels(b, sc[0], "rgb8")[0], want(displayed(o, steps, "rgb8"), sc, name)), (size, steps)


def bits_of(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("dtype, elem", [(torch.float32, "f32"), (torch.float16, "f16"), (torch.bfloat16, "bf16")])
def test_render_tensor_flips_layouts_elements(H, S, ctx, decoded, dtype, elem):
    """The four flips in one call: a flip acts on R at the store, the taps stay D's."""
    p, o = decoded(3, width=136, height=72, conf_right=6)
    orients = [[], [("irot", 1)], [("imir", 0)], [("irot", 3), ("imir", 1)]]
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    Ds = [displayed(o, steps, "rgb8") for steps in orients]
    flips = [0, 1, 2, 3]
    windows = [(3, 5, 101, 61), (5, 3, 61, 101), (0, 0, 130, 72), (1, 2, 70, 127)]
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    for name in R.FILTERS:
        Rs = [R.resize(D, w, 70, 19, name) for D, w in zip(Ds, windows)]
        for layout in ("chw", "hwc"):
            got = bits_of(ctx.render_tensor(outs, (19, 70), dtype=dtype, layout=layout, windows=windows, flips=flips,
                                            filter=name))
            for k, Rk in enumerate(Rs):
                assert np.array_equal(got[k], tensor_ref.tensor(Rk, a, b, elem, layout, flip=flips[k])), (name, layout, k)


def test_colorspace_transforms_the_rounded_result(H, S, ctx):
    p = S.SynthParams(width=72, height=40, chroma_format=3)
    f = S.display_heic(p, seed=52, transforms=boxes(S, [("irot", 1)]), colr=S.nclx_box(12, 13, 6, True))  # P3 D65
    o = H.HeicDecoder.decode(f)
    t = o.image.color_transform("srgb")
    assert not t.identity
    D = displayed(o, [("irot", 1)], "rgba8")
    for name in R.FILTERS:
        Rr = R.resize(D, None, 13, 23, name)
        got = host(ctx.render_scaled([o], (23, 13), "stretch", "rgba8", colorspace="srgb", filter=name))[0]
        assert np.array_equal(got, color_ref.transform_picture(t, Rr)), name
        assert (got != Rr).any()
        assert np.array_equal(host(ctx.render_scaled([o], (23, 13), "stretch", "rgba8", filter=name))[0], Rr)


def test_window_decode_needs_the_halo(H, ctx):
    """prepare(windows=, size=, filter="bicubic") decodes the window and its taps' halo:
    the render equals the full decode's bit for bit; a decode for the plain window is refused."""
    import window_cases as WC

    img = H.HeifImage.parse(WC.fixture("rot1"))
    window, size = (70, 66, 60, 58), (24, 20)  # ends on tile borders of the source: the halo crosses them
    plain, wide = img.source_rect(window), img.source_rect(window, size, "bicubic")
    assert wide != plain and wide[2] > plain[2] and wide[3] > plain[3]
    full = ctx.alloc_outputs([img])
    b = ctx.prepare([img])
    b.decode_async(full)
    assert b.status() == [0]
    b.free()
    outs = ctx.alloc_outputs([img])
    for t in (outs[0].y, outs[0].cb, outs[0].cr):
        t.fill_(0x55)
    b = ctx.prepare([img], windows=[window], size=size, filter="bicubic")
    b.decode_async(outs)
    assert b.status() == [0] and outs[0].valid == wide and b.pictures < 12
    b.free()
    want_px = ctx.render_scaled(full, size, windows=[window], filter="bicubic")
    assert torch.equal(ctx.render_scaled(outs, size, windows=[window], filter="bicubic"), want_px)
    D = host(ctx.render(full, "rgb8")[0])
    assert np.array_equal(host(want_px)[0], R.resize(D, window, size[1], size[0], "bicubic"))
    b = ctx.prepare([img], windows=[window])  # the plain window: enough for the area render only
    b.decode_async(outs)
    assert b.status() == [0] and outs[0].valid == plain
    b.free()
    ctx.render_scaled(outs, size, windows=[window])
    with pytest.raises(ValueError):
        ctx.render_scaled(outs, size, windows=[window], filter="bicubic")
    with pytest.raises(ValueError):
        ctx.render_tensor(outs, size, windows=[window], filter="bilinear")


def test_python_surface(H, S, ctx):
    f = S.display_heic(S.SynthParams(width=136, height=72, conf_right=6), seed=60, transforms=boxes(S, [("irot", 1)]))
    o = H.HeicDecoder.decode(f)
    D = displayed(o, [("irot", 1)], "rgb8")
    shown = H.HeicDecoder.decode_display(f, size=(300, 400), filter="bicubic")  # contain: 72 x 130 enlarged to 166 x 300
    assert tuple(shown.shape) == (300, 166, 3)
    assert np.array_equal(host(shown), R.resize(D, None, 166, 300, "bicubic"))
    win = H.HeicDecoder.decode_display(f, size=(16, 24), mode="cover", tiles="window", filter="bilinear")
    assert np.array_equal(host(win), host(ctx.render_scaled([o], (16, 24), "cover", filter="bilinear"))[0])
    t = H.HeicDecoder.decode_tensor(f, (16, 24), filter="bicubic", dtype=torch.float32)
    assert torch.equal(t, ctx.render_tensor([o], (16, 24), filter="bicubic", dtype=torch.float32)[0])
    assert torch.equal(ctx.render_scaled([o], (16, 24), filter="area"), ctx.render_scaled([o], (16, 24)))
    with pytest.raises(ValueError):
        ctx.render_scaled([o], (16, 24), filter="lanczos")


def test_halfmoonbay_cover_224_bicubic(H, ctx, halfmoonbay):
    """irot 3 at full size: the swapped path, 12 megapixels through the chunk loops at the
    workload's ratio, against the restatement fed with heifgpu_render_batch's own output."""
    o = H.HeicDecoder.decode(halfmoonbay)
    D = host(ctx.render([o], "rgb8")[0])
    assert D.shape == (4032, 3024, 3)
    cover = ctx.render_scaled([o], (224, 224), mode="cover", filter="bicubic")
    assert np.array_equal(host(cover)[0], R.resize(D, (0, 504, 3024, 3024), 224, 224, "bicubic"))
