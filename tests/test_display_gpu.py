"""The render stage on the device: heifgpu_render_batch / DecodeContext.render
against the step-by-step numpy restatement (display_ref), which is fed the
planes the GPU decoded, so only the render stage is under test.  Every
comparison is exact.  The pictures are a few CTBs each; the sizes are the
smallest at which k_render can go wrong: partial tiles in both axes on both of
its paths (256 x 16 tiles for maps that keep the axes, 64 x 64 through LDS for
those that swap them), widths that are no multiple of 4, odd chroma phase,
unaligned pitches."""
import ctypes

import numpy as np
import pytest

import display_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMATS = ("rgb8", "rgba8", "rgb16", "rgba16")


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


def planes(o):
    return [None if t is None else host(t) for t in (o.y, o.cb, o.cr)]


def expected(o, steps, fmt, alpha=None):
    y, cb, cr = planes(o)
    inf = o.info
    return display_ref.render(y, cb, cr, inf.matrix_coeffs, bool(inf.full_range), inf.bit_depth, steps, fmt,
                              alpha=None if alpha is None else host(alpha.y),
                              alpha_depth=8 if alpha is None else alpha.info.bit_depth)


def with_steps(H, S, o, params, steps, **kw):
    """The decoded picture `o` as the primary of a file that carries `steps`:
    the same planes under another parsed image (the display map is the image's)."""
    img = H.HeifImage.parse(S.display_heic(params, transforms=boxes(S, steps), **kw))
    return H.DecodedImage(o.y, o.cb, o.cr, o.info, img)


def render_raw(H, ctx, outs, fmt, pad, alphas=None, sentinel=0xA5):
    """heifgpu_render_batch into sentinel-filled buffers whose pitch is the row
    size plus pad[i] bytes; returns (rc, [buffer as (H', pitch) uint8 array])."""
    from heif_amd import _lib

    f = _lib.PIX_FORMATS[fmt]
    bpp = (4 if f & 1 else 3) * (2 if f >= 2 else 1)
    n = len(outs)
    surf = (_lib.Surface * n)()
    bufs = []
    for i, o in enumerate(outs):
        d = o.image.display
        pitch = d.out_width * bpp + pad[i]
        b = torch.full((d.out_height, pitch), sentinel, dtype=torch.uint8, device="cuda:0")
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
    torch.cuda.synchronize()
    rc = _lib.lib.heifgpu_render_batch(ctx._h, imgs, n, H.DecodeContext.planes_of(outs), aimgs, aplanes, f, surf,
                                       ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    torch.cuda.synchronize()
    return rc, [b.cpu().numpy() for b in bufs]


ORIENTATIONS = [[("irot", k)] + m for k in range(4) for m in ([], [("imir", 0)])]


@pytest.mark.parametrize("size", [dict(width=136, height=72, conf_right=6),   # 130 x 72: 3 x 2 LDS tiles, 5 row tiles
                                  dict(width=264, height=24, conf_right=2)],  # 262 x 24: 2 row tiles in x
                         ids=["130x72", "262x24"])
def test_edge_tiles_all_orientations(H, S, ctx, size):
    p = S.SynthParams(**size)
    o = H.HeicDecoder.decode(S.single_heic(p, seed=3))
    outs = [with_steps(H, S, o, p, steps) for steps in ORIENTATIONS]
    got = ctx.render(outs, "rgb8")  # the eight orientations in one call
    for steps, g in zip(ORIENTATIONS, got):
        want = expected(o, steps, "rgb8")
        assert tuple(g.shape) == want.shape, steps
        assert np.array_equal(host(g), want), steps


@pytest.mark.parametrize("chroma, depth", [(0, 8), (0, 12), (1, 8), (1, 10), (2, 8), (2, 12), (3, 8), (3, 10)])
def test_formats_and_chroma(H, S, ctx, chroma, depth):
    # 4:4:4 and 4:0:0 with an odd displayed width (67); the subsampled formats crop by whole chroma samples
    p = S.SynthParams(width=72, height=40, conf_right=5 if chroma in (0, 3) else 6, chroma_format=chroma, bit_depth=depth)
    o = H.HeicDecoder.decode(S.single_heic(p, seed=10 + chroma))
    assert o.info.bit_depth == depth and o.info.chroma_format_idc == chroma
    orients = [[("imir", 0)], [("irot", 1), ("imir", 1)]]  # one that keeps the axes, one that swaps them
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    for fmt in FORMATS:
        got = ctx.render(outs, fmt)
        for steps, g in zip(orients, got):
            want = expected(o, steps, fmt)
            assert g.dtype == (torch.int16 if fmt.endswith("16") else torch.uint8)
            assert np.array_equal(host(g), want), (fmt, steps)
            if chroma == 0:
                assert (want[..., 0] == want[..., 1]).all() and (want[..., 0] == want[..., 2]).all()
            if fmt.startswith("rgba"):
                assert (want[..., 3] == ((1 << depth) - 1 if fmt.endswith("16") else 255)).all()  # opaque


def test_chroma_phase_under_odd_clap(H, S, ctx):
    p = S.SynthParams(width=64, height=48)
    o = H.HeicDecoder.decode(S.single_heic(p, seed=21))
    clap = ("clap", (41, 1, 29, 1, -13, 2, -13, 2))  # left 5, top 3: both odd on 4:2:0
    assert display_ref.clap_rect(64, 48, clap[1]) == (5, 3, 41, 29)
    orients = [[clap], [clap, ("irot", 1)], [("irot", 3), ("clap", (29, 1, 41, 1, -9, 2, 7, 2)), ("imir", 0)]]
    assert display_ref.clap_rect(48, 64, orients[2][1][1]) == (5, 15, 29, 41)
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    for steps, g in zip(orients, ctx.render(outs, "rgb8")):
        assert np.array_equal(host(g), expected(o, steps, "rgb8")), steps


@pytest.mark.parametrize("fmt", FORMATS)
def test_unaligned_pitch_keeps_padding(H, S, ctx, fmt):
    p = S.SynthParams(width=136, height=72, conf_right=6, bit_depth=10)
    o = H.HeicDecoder.decode(S.single_heic(p, seed=4))
    orients = [[], [("irot", 1)], [("imir", 0)]]
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    wide = fmt.endswith("16")
    bpp = (4 if fmt.startswith("rgba") else 3) * (2 if wide else 1)
    # pitch = 1 mod 4 (2 mod 4 for 16-bit samples): most rows start off a dword, and the pitch exceeds the row
    pad = [(-(steps_w * bpp) % 4) + (6 if wide else 5) for steps_w in (130, 72, 130)]
    rc, bufs = render_raw(H, ctx, outs, fmt, pad)
    assert rc == 0
    for steps, b, pd in zip(orients, bufs, pad):
        want = expected(o, steps, fmt)
        row = want.shape[1] * bpp
        assert (b.shape[1] - row) == pd and b.shape[1] % 4 == (2 if wide else 1)
        got = np.ascontiguousarray(b[:, :row]).view(want.dtype).reshape(want.shape)
        assert np.array_equal(got, want), steps
        assert (b[:, row:] == 0xA5).all(), steps  # the pad bytes keep the sentinel


def test_pitch_below_row_rejected(H, S, ctx):
    p = S.SynthParams(width=64, height=48)
    o = H.HeicDecoder.decode(S.single_heic(p, seed=21))
    rc, bufs = render_raw(H, ctx, [with_steps(H, S, o, p, [])], "rgb8", [-1])
    assert rc == -1 and (bufs[0] == 0xA5).all()  # HEIFGPU_E_INVALID, nothing written


def test_mixed_batch_one_call(H, S, ctx):
    """Three images of different size, orientation, chroma format and matrix in
    one call (one k_render launch over (tile, image): DESIGN.md)."""
    specs = [
        (S.SynthParams(width=136, height=72, conf_right=6), [("irot", 1)], S.nclx_box(1, 1, 6, True)),       # BT.601 full
        (S.SynthParams(width=72, height=40, conf_right=5, chroma_format=3), [("imir", 0)], S.nclx_box(1, 1, 1, False)),
        (S.SynthParams(width=48, height=32, chroma_format=0), [("clap", (27, 1, 22, 1, -5, 2, 3, 1)), ("irot", 2)], None),
    ]
    outs = []
    for k, (p, steps, colr) in enumerate(specs):
        f = S.display_heic(p, seed=30 + k, transforms=boxes(S, steps), colr=colr)
        outs.append(H.HeicDecoder.decode(f))
    assert (outs[0].info.matrix_coeffs, outs[0].info.full_range) == (6, 1)
    assert (outs[1].info.matrix_coeffs, outs[1].info.full_range) == (1, 0)
    got = ctx.render(outs, "rgb8")
    for (p, steps, _), o, g in zip(specs, outs, got):
        assert np.array_equal(host(g), expected(o, steps, "rgb8")), steps
    # the matrix matters: the BT.709 limited image differs from a BT.601 full rendering of its planes
    y, cb, cr = planes(outs[1])
    assert not np.array_equal(host(got[1]), display_ref.render(y, cb, cr, 6, True, 8, specs[1][1], "rgb8"))


@pytest.mark.parametrize("depth, alpha_depth", [(8, 8), (10, 10), (10, 12)])
def test_alpha(H, S, ctx, depth, alpha_depth):
    p = S.SynthParams(width=64, height=48, bit_depth=depth)
    a = S.SynthParams(width=64, height=48, chroma_format=0, bit_depth=alpha_depth)
    steps = [("clap", (41, 1, 29, 1, -13, 2, -13, 2)), ("imir", 0), ("irot", 1)]
    f = S.display_heic(p, seed=40, transforms=boxes(S, steps), aux=(S.AuxImage(a, seed=41, urn=S.ALPHA_URN_MPEGB),))
    o = H.HeicDecoder.decode(f)
    assert o.image.display.alpha_item_id == 2
    al = H.HeicDecoder.decode(f, item_id=2)
    opaque = with_steps(H, S, o, p, [("imir", 1)])  # the same planes, no alpha, in the same batch
    for fmt in ("rgba8", "rgba16"):
        got = ctx.render([o, opaque], fmt, alphas=[al, None])
        want = expected(o, steps, fmt, alpha=al)
        assert np.array_equal(host(got[0]), want), fmt
        assert len(np.unique(want[..., 3])) > 4  # a real alpha plane, not a constant
        wo = expected(o, [("imir", 1)], fmt)
        assert np.array_equal(host(got[1]), wo), fmt
        assert (host(got[1])[..., 3] == ((1 << depth) - 1 if fmt == "rgba16" else 255)).all()
    # the RGB formats ignore the alpha arguments
    assert np.array_equal(host(ctx.render([o], "rgb8", alphas=[al])[0]), expected(o, steps, "rgb8"))


def test_alpha_of_another_size_is_unsupported(H, S, ctx):
    p = S.SynthParams(width=64, height=48)
    a = S.SynthParams(width=48, height=32, chroma_format=0)
    f = S.display_heic(p, seed=40, aux=(S.AuxImage(a, seed=41),))
    o, al = H.HeicDecoder.decode(f), H.HeicDecoder.decode(f, item_id=2)
    rc, bufs = render_raw(H, ctx, [o], "rgba8", [0], alphas=[al])
    assert rc == -3 and (bufs[0] == 0xA5).all()  # HEIFGPU_E_UNSUPPORTED before anything is launched
    with pytest.raises(H.UnsupportedError):
        ctx.render([o], "rgba8", alphas=[al])


def test_back_to_back_calls_keep_their_descriptors(H, S, ctx):
    """Calls issued without a host synchronise in between (more of them than the
    staging ring has slots) each render their own batch."""
    p1, p2 = S.SynthParams(width=136, height=72, conf_right=6), S.SynthParams(width=72, height=40, chroma_format=3)
    o1, o2 = H.HeicDecoder.decode(S.single_heic(p1, seed=3)), H.HeicDecoder.decode(S.single_heic(p2, seed=5))
    batches = []
    for k in range(6):
        s1, s2 = ORIENTATIONS[k], ORIENTATIONS[7 - k]
        batch = [with_steps(H, S, o1, p1, s1), with_steps(H, S, o2, p2, s2)][::1 if k % 2 else -1]
        batches.append((batch, [(o1, s1), (o2, s2)][::1 if k % 2 else -1]))
    torch.cuda.synchronize()
    results = [ctx.render(b, "rgb8") for b, _ in batches]  # six launches queued, no synchronise between them
    torch.cuda.synchronize()
    for (_, what), got in zip(batches, results):
        for (o, steps), g in zip(what, got):
            assert np.array_equal(host(g), expected(o, steps, "rgb8")), steps


def test_halfmoonbay_render_equals_to_rgb(H, ctx, halfmoonbay):
    """irot 3 at full size through the new kernel's LDS path, compared on the device."""
    o = H.HeicDecoder.decode(halfmoonbay)
    old = ctx.to_rgb(o)
    new = ctx.render([o], "rgb8")[0]
    assert tuple(new.shape) == (4032, 3024, 3)
    assert torch.equal(new, old)
    shown = H.HeicDecoder.decode_display(halfmoonbay)  # no alpha, 8 bits: RGB8
    assert shown.dtype == torch.uint8 and torch.equal(shown, H.HeicDecoder.decode_rgb(halfmoonbay))


def test_decode_display_ten_bit_clap_imir_alpha(H, S):
    p = S.SynthParams(width=64, height=48, bit_depth=10)
    a = S.SynthParams(width=64, height=48, chroma_format=0, bit_depth=10)
    steps = [("clap", (41, 1, 29, 1, -13, 2, -13, 2)), ("imir", 0)]
    f = S.display_heic(p, seed=50, transforms=boxes(S, steps), aux=(S.AuxImage(a, seed=51),))
    shown = H.HeicDecoder.decode_display(f)
    assert shown.dtype == torch.int16 and tuple(shown.shape) == (29, 41, 4)  # RGBA16 picked
    o, al = H.HeicDecoder.decode(f), H.HeicDecoder.decode(f, item_id=2)
    assert np.array_equal(host(shown), expected(o, steps, "rgba16", alpha=al))
    assert H.HeicDecoder.decode_display(f, fmt="rgb8").shape == (29, 41, 3)
