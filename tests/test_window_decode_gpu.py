"""Window decode on the device: DecodeContext.prepare(windows=)
decodes the tiles a window reads into sentinel-filled planes; the selected
tiles equal the full decode of the same file (which the existing suite pins to
the oracle), every other sample keeps the sentinel, and every render of the
window is bit-identical to the same call on the full decode.  Every comparison
is exact.  The fixture is window_cases': 4 x 3 tiles of 64 x 64, 250 x 180."""
import ctypes

import numpy as np
import pytest

import window_cases as WC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5
# per orientation of WC.EIGHT, a window in source coordinates (None: the whole picture):
# one tile, four, the grown two, the cropped corner (one pixel), one pixel at the origin,
# six tiles, everything, four tiles across the middle
SOURCE_WINDOWS = WC.SOURCE_WINDOWS + [(0, 0, 1, 1), (100, 30, 120, 60), None, (127, 127, 2, 2)]
TILES = [1, 4, 2, 1, 1, 6, 12, 4]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def ctx(H):
    return H.HeicDecoder.context(0)


def host(t):
    return None if t is None else t.cpu().numpy()


def planes(o):
    return [host(t) for t in (o.y, o.cb, o.cr)]


def fill(outs):
    for o in outs:
        for t in (o.y, o.cb, o.cr):
            if t is not None:
                t.fill_(SENTINEL)


def decode_full(ctx, imgs):
    outs = ctx.alloc_outputs(imgs)
    b = ctx.prepare(imgs)
    b.decode_async(outs)
    assert not any(b.status())
    b.free()
    return outs


@pytest.fixture(scope="module")
def eight(H, ctx):
    """The eight orientations: images, their full decodes (one batch, once), and
    the displayed window of each."""
    imgs = [H.HeifImage.parse(WC.fixture(n)) for n in WC.EIGHT]
    full = decode_full(ctx, imgs)
    windows = [WC.displayed_window(WC.VARIANTS[n], w) for n, w in zip(WC.EIGHT, SOURCE_WINDOWS)]
    return imgs, full, windows


def expected(full_planes, rect, tile_w, tile_h):
    """The planes a window decode of `rect` leaves in sentinel-filled planes: the
    grid tiles that meet the rectangle from the full decode, the sentinel elsewhere."""
    y = full_planes[0]
    mask = np.zeros(y.shape, bool)
    if rect is None:
        mask[:] = True
    else:
        x0, y0, w, h = rect
        for c, r in tiles_of_rect(rect, tile_w, tile_h):
            mask[r * tile_h:(r + 1) * tile_h, c * tile_w:(c + 1) * tile_w] = True
    out = [np.where(mask, y, SENTINEL).astype(y.dtype)]
    for p in full_planes[1:]:
        if p is None:
            out.append(None)
            continue
        sy, sx = int(p.shape[0] < y.shape[0]), int(p.shape[1] < y.shape[1])
        out.append(np.where(mask[::1 << sy, ::1 << sx], p, SENTINEL).astype(p.dtype))
    return out, int(mask.sum())


def tiles_of_rect(rect, tile_w=WC.TILE, tile_h=WC.TILE):
    if rect is None:
        rect = (0, 0, WC.W, WC.H)
    x0, y0, w, h = rect
    return {(c, r) for c in range(x0 // tile_w, (x0 + w - 1) // tile_w + 1)
            for r in range(y0 // tile_h, (y0 + h - 1) // tile_h + 1)}


def assert_planes(o, full, rect, tag, tile=(WC.TILE, WC.TILE)):
    want, n = expected(planes(full), rect, *tile)
    for g, w, c in zip(planes(o), want, "YUV"):
        if w is None:
            assert g is None
            continue
        assert np.array_equal(g, w), (tag, c, int((g != w).sum()))
    return n


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = a.contiguous(), b.contiguous()
    if a.dtype.is_floating_point:  # bit patterns
        it = torch.int32 if a.dtype == torch.float32 else torch.int16
        a, b = a.view(it), b.view(it)
    return a.shape == b.shape and bool((a == b).all())


def win(w):
    return (0, 0, 0, 0) if w is None else w


# ---------------------------------------------------------- 4: one batch
@pytest.mark.parametrize("parse", ["lanes", "solo", "spread"])
def test_eight_orientations_in_one_batch(H, ctx, eight, parse):
    imgs, full, windows = eight
    outs = ctx.alloc_outputs(imgs)
    fill(outs)
    b = ctx.prepare(imgs, windows=windows, parse=parse)
    assert b.parse_geometry()["mode"] == parse
    assert b.pictures == sum(TILES)
    b.decode_async(outs)
    assert b.status() == [0] * 8
    for i, (o, f, im, sw) in enumerate(zip(outs, full, imgs, SOURCE_WINDOWS)):
        rect = None if sw is None else im.source_rect(windows[i])
        assert b.rects[i] == o.valid == (rect if sw is not None else None), i
        assert_planes(o, f, rect, (parse, i))
        assert len(tiles_of_rect(rect)) == TILES[i], i
    # the renders of the windows: bit for bit those of the full decode
    ws = [win(w) for w in windows]
    for fmt in ("rgb8", "rgba16"):
        assert same(ctx.render_scaled(outs, (9, 7), fmt=fmt, windows=ws), ctx.render_scaled(full, (9, 7), fmt=fmt, windows=ws))
    flips = [i & 3 for i in range(8)]
    for dtype, layout in ((torch.float32, "chw"), (torch.float16, "hwc")):
        got = ctx.render_tensor(outs, (8, 10), dtype=dtype, layout=layout, windows=ws, flips=flips)
        assert same(got, ctx.render_tensor(full, (8, 10), dtype=dtype, layout=layout, windows=ws, flips=flips))
    b.free()
    # render(): the whole displayed picture of a file whose clap is a window's size
    small = H.HeifImage.parse(WC.fixture("clap_small_rot3"))
    assert small.source_rect(None) == WC.CLAP_SMALL
    o = ctx.alloc_outputs([small])
    fill(o)
    bs = ctx.prepare([small], windows=[None], parse=parse)
    assert bs.pictures == 12  # no window: everything
    bs.free()
    bs = ctx.prepare([small], windows=[(0, 0, 10, 10)], parse=parse)
    assert bs.pictures == 4
    bs.decode_async(o)
    assert bs.status() == [0]
    bs.free()
    f = H.DecodedImage(full[0].y, full[0].cb, full[0].cr, full[0].info, small)
    assert_planes(o[0], f, WC.CLAP_SMALL, "clap")
    assert same(ctx.render(o, "rgb8"), ctx.render([f], "rgb8"))
    assert same(ctx.render(o, "rgba16"), ctx.render([f], "rgba16"))


def test_prepare_rects_without_rectangles_is_prepare_ex(H, ctx, eight):
    from heif_amd import _lib

    imgs = eight[0]
    arr = (ctypes.c_void_p * 8)(*[im._h.value for im in imgs])
    h = ctypes.c_void_p()
    _lib.check(_lib.lib.heifgpu_batch_prepare_ex(ctx._h, arr, 8, None, ctypes.byref(h)))
    n = ctypes.c_uint32()
    _lib.check(_lib.lib.heifgpu_batch_picture_count(h, ctypes.byref(n)))
    _lib.lib.heifgpu_batch_free(h)
    b = ctx.prepare(imgs)
    assert b.pictures == n.value == 96 and b.rects == [None] * 8
    b.free()
    b = ctx.prepare(imgs, windows=[None] * 8, rects=[(0, 0, 0, 0)] * 8)
    assert b.pictures == 96 and b.rects == [None] * 8
    b.free()


# -------------------------------------------------------------- 5: reload
def test_reload_full_windowed_other_windows_full(H, ctx, eight):
    """One batch reloaded four times; every load decoded twice back to back
    (descriptor generations, parse-output sets), statuses all zero."""
    imgs, full, windows = eight
    outs = ctx.alloc_outputs(imgs)
    other_src = SOURCE_WINDOWS[3:] + SOURCE_WINDOWS[:3]
    other = [WC.displayed_window(WC.VARIANTS[n], w) for n, w in zip(WC.EIGHT, other_src)]
    batch = None
    for load, (ws, srcs) in enumerate([(None, [None] * 8), (windows, SOURCE_WINDOWS), (other, other_src),
                                       (None, [None] * 8)]):
        batch = ctx.prepare(imgs, windows=ws, reuse=batch, wait=False)
        fill(outs)
        batch.decode_async(outs)
        batch.decode_async(outs)
        assert batch.status() == [0] * 8, load
        prev = batch.status_previous()
        assert prev == ([] if load == 0 else [0] * 8), load
        for i, (o, f, im, sw) in enumerate(zip(outs, full, imgs, srcs)):
            rect = None if sw is None else im.source_rect(ws[i])
            assert o.valid == rect
            assert_planes(o, f, rect, (load, i))
    assert batch.pictures == 96
    batch.free()


# --------------------------------------------------------------- 6: alpha
def test_alpha_on_another_grid(H, ctx):
    """The alpha image (4:0:0, 2 x 2 tiles of 128 x 96) is decoded with the
    colour image's source rectangle and selects by its own grid."""
    data = WC.fixture("rot1_mir", aux=True)
    colour = H.HeifImage.parse(data)
    alpha = H.HeifImage.parse(data, colour.display.alpha_item_id)
    assert (alpha.info.grid_cols, alpha.info.grid_rows, alpha.info.tile_width, alpha.info.tile_height) == (2, 2, 128, 96)
    fc, fa = decode_full(ctx, [colour])[0], decode_full(ctx, [alpha])[0]
    for src_window, ctiles, atiles in (((10, 10, 60, 60), 4, 1), ((120, 90, 10, 10), 2, 4), ((249, 179, 1, 1), 1, 1)):
        window = WC.displayed_window(WC.VARIANTS["rot1_mir"], src_window)
        rect = colour.source_rect(window)
        oc, oa = ctx.alloc_outputs([colour]), ctx.alloc_outputs([alpha])
        fill(oc + oa)
        bc, ba = ctx.prepare([colour], windows=[window]), ctx.prepare([alpha], rects=[rect])
        assert (bc.pictures, ba.pictures) == (ctiles, atiles)
        bc.decode_async(oc)
        ba.decode_async(oa)
        assert bc.status() == [0] and ba.status() == [0]
        assert_planes(oc[0], fc, rect, "colour")
        assert_planes(oa[0], fa, rect, "alpha", tile=(128, 96))
        got = ctx.render_scaled(oc, (6, 5), fmt="rgba8", alphas=oa, windows=[window])
        assert same(got, ctx.render_scaled([fc], (6, 5), fmt="rgba8", alphas=[fa], windows=[window]))
        bc.free()
        ba.free()
    # an alpha image decoded for less than the render reads is refused
    with pytest.raises(ValueError):
        ctx.render_scaled([fc], (6, 5), fmt="rgba8", alphas=oa, windows=[(0, 0, 0, 0)])


# ------------------------------------------------------- 7: the helpers
def test_single_file_helpers_equal_their_full_decodes(H, ctx, halfmoonbay):
    files = [WC.fixture("rot1_mir"), WC.fixture("clap_rot1_mir", aux=True), halfmoonbay]
    for k, data in enumerate(files):
        size = (224, 224) if k == 2 else (16, 16)
        for kw in (dict(), dict(dtype=torch.float32, layout="hwc", flip=1), dict(src="rgba8", mean=(0.5,) * 4, std=(0.25,) * 4)):
            a = H.HeicDecoder.decode_tensor(data, size, tiles="all", **kw)
            assert same(H.HeicDecoder.decode_tensor(data, size, tiles="window", **kw), a), (k, kw)
        a = H.HeicDecoder.decode_display(data, size=size, mode="cover", tiles="all")
        assert same(H.HeicDecoder.decode_display(data, size=size, mode="cover", tiles="window"), a), k
        if k < 2:  # the full-size picture: a clap is the only thing that reads less
            a = H.HeicDecoder.decode_display(data, tiles="all")
            assert same(H.HeicDecoder.decode_display(data, tiles="window"), a), k
    with pytest.raises(ValueError):
        H.HeicDecoder.decode_display(files[0], tiles="some")
    # halfmoonbay, cover 224 x 224: 42 of its 48 tiles
    img = H.HeifImage.parse(halfmoonbay)
    window = H.HeicDecoder._fit_window(img, (224, 224), "cover")
    rows = -(-img.info.tile_height // (1 << img.tile_params(0)["log2_ctb"]))  # a substream per CTB row (WPP)
    for parse, groups in (("solo", 42), ("spread", 42 * rows)):  # workgroups: pictures; substreams
        b = ctx.prepare([img], windows=[window], parse=parse)
        assert b.pictures == 42 and b.parse_geometry()["workgroups"] == groups
        b.free()
    out = H.HeicDecoder.decode(halfmoonbay, window=window)
    assert out.valid == (504, 0, 3024, 3024)


# ---------------------------------------------------------------- 8: guards
def test_a_render_outside_valid_raises_and_calls_nothing(H, ctx, eight, monkeypatch):
    imgs, full, windows = eight
    outs = ctx.alloc_outputs(imgs[:2])
    b = ctx.prepare(imgs[:2], windows=windows[:2])
    b.decode_async(outs)
    assert b.status() == [0, 0]
    b.free()
    inside = [win(w) for w in windows[:2]]
    ok = ctx.render_scaled(outs, (4, 4), windows=inside)

    def never(*a, **k):
        raise AssertionError("the library was called")

    for name in ("heifgpu_render_batch", "heifgpu_render_batch_scaled", "heifgpu_render_batch_tensor",
                 "heifgpu_ycbcr_to_rgb"):
        monkeypatch.setattr(H.lib, name, never)
    x, y, w, h = inside[1]
    for bad in ([inside[0], (x, y, w + 60, h)], [(0, 0, 0, 0), inside[1]]):
        with pytest.raises(ValueError):
            ctx.render_scaled(outs, (4, 4), windows=bad)
        with pytest.raises(ValueError):
            ctx.render_tensor(outs, (4, 4), windows=bad)
    with pytest.raises(ValueError):
        ctx.render_scaled(outs, (4, 4), mode="stretch")
    with pytest.raises(ValueError):
        ctx.render(outs)
    with pytest.raises(ValueError):
        ctx.to_rgb(outs[0])
    monkeypatch.undo()
    assert same(ctx.render_scaled(outs, (4, 4), windows=inside), ok)


def test_an_invalid_rectangle_leaves_a_reloaded_batch_decodable(H, ctx, eight):
    imgs, full, windows = eight
    outs = ctx.alloc_outputs(imgs)
    b = ctx.prepare(imgs, windows=windows)
    b.decode_async(outs)
    assert b.status() == [0] * 8
    rects = list(b.rects)
    for bad in ((0, 0, WC.W + 1, 1), (0, 0, 0, 3), (WC.W, 0, 1, 1)):
        with pytest.raises(H.HeifGpuError) as e:
            ctx.prepare(imgs, reuse=b, rects=[bad] + [None] * 7)
        assert e.value.code == -1  # HEIFGPU_E_INVALID
    with pytest.raises(ValueError):  # a window outside the displayed picture: refused before the library
        ctx.prepare(imgs, reuse=b, windows=[(0, 0, 999, 1)] + [None] * 7)
    assert b.rects == rects and b.pictures == sum(TILES)
    fill(outs)
    b.decode_async(outs)
    assert b.status() == [0] * 8
    for i, (o, f) in enumerate(zip(outs, full)):
        assert_planes(o, f, rects[i], i)
    b.free()
