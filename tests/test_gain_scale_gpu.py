"""The scaled gain-map HDR render on the device: heifgpu_render_batch_gain_scaled,
DecodeContext.render_hdr_scaled and HeicDecoder.decode_hdr(size=) against gain_scale_ref's numpy
contract over the planes the GPU decoded, bit for bit, and against render_hdr at the identity.

The pictures are those of tests/test_gain_gpu.py (rebuilt here): an 8-bit batch of a 320 x 48
picture with a 160 x 24 map, mirrored, with an alpha image (axes kept); a 320 x 48 picture with a
same-size map under irot 1 (axes swapped); a 96 x 64 picture with a 40 x 24 map (ratios 2.4 and
2.67) under an odd-offset clap to 61 x 41 and irot 3; a 72 x 40 picture with a 10-bit map beside
its u8 samples; and a 10-bit batch of a 4:2:2 base with an 8-bit map, turned, and a 4:2:0 base
with a 10-bit map and a 10-bit alpha image.  Two more are filled by the tests under parsed
headers: the sums of gain codes that pass 32 bits in a column and 2^46 in the numerator."""
import ctypes

import numpy as np
import pytest

import gain_ref
import gain_scale_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CLAP = ("clap", (61, 1, 41, 1, 3, 2, 1, 2))  # 61 x 41 at left 19, top 12 of 96 x 64
SENTINEL = 0x5A
MAXCODE = 256 * 4095


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
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def boxes(S, steps):
    make = {"clap": lambda a: S.clap_box(*a), "irot": S.irot_box, "imir": S.imir_box}
    return tuple(make[k](a) for k, a in steps)


ISO_OFFSETS = dict(gain_min=-1.0, gain_max=3.0, gamma=1.4, alternate_headroom=3.0, base_offset=1 / 64, alternate_offset=1 / 8)
ISO_8STOPS = dict(gain_min=0.0, gain_max=8.0, gamma=0.7, alternate_headroom=8.0, base_offset=1.0, alternate_offset=0.0)


def specs(S):
    """name -> (base params, seed, steps, colr, gain params, gain seed, kind, tmap kwargs, alpha params)."""
    p3 = S.icc_box(S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True))
    P = S.SynthParams
    return {
        "wide-iso": (P(width=320, height=48), 71, [("imir", 0)], p3, P(width=160, height=24, chroma_format=0), 171, "iso",
                     ISO_OFFSETS, P(width=320, height=48, chroma_format=0)),
        "turned-apple": (P(width=320, height=48, chroma_format=3), 72, [("irot", 1)], S.nclx_box(1, 13, 1, True),
                         P(width=320, height=48, chroma_format=0), 172, "apple", None, None),
        "ratio-iso": (P(width=96, height=64), 73, [CLAP, ("irot", 3)], p3, P(width=40, height=24, chroma_format=0), 173, "both",
                      ISO_8STOPS, None),
        "deepmap-apple": (P(width=72, height=40), 74, [], S.nclx_box(12, 13, 6, False),
                          P(width=40, height=24, chroma_format=0, bit_depth=10), 174, "apple", None, None),
        "422-iso": (P(width=136, height=72, conf_right=6, chroma_format=2, bit_depth=10), 75, [("irot", 1)], p3,
                    P(width=64, height=40, chroma_format=0), 175, "iso", ISO_OFFSETS, None),
        "deep-apple": (P(width=72, height=40, bit_depth=10), 76, [("imir", 1)], None,
                       P(width=40, height=24, chroma_format=0, bit_depth=10), 176, "apple", None,
                       P(width=72, height=40, chroma_format=0, bit_depth=10)),
        # more than 512 columns along the source's x, kept and turned
        "long": (P(width=1056, height=16), 77, [], None, P(width=528, height=8, chroma_format=0), 177, "apple", None, None),
        "long-turned": (P(width=1056, height=16), 77, [("irot", 1)], None, P(width=528, height=8, chroma_format=0), 177, "apple",
                        None, None),
    }


def build(S, sp):
    p, seed, steps, colr, gp, gseed, kind, tm, ap = sp
    return S.gainmap_heic(p, gp, seed=seed, gain_seed=gseed, kind=kind, tmap=S.tmap_box(**tm) if tm else None,
                          transforms=boxes(S, steps), colr=colr,
                          alpha=S.AuxImage(ap, seed=seed + 100, urn=S.ALPHA_URN_MPEGB) if ap is not None else None)


class Batch:
    """The pictures, their gain maps and alpha images decoded once (never written to)."""

    def __init__(self, H, S, names):
        self.names = list(names)
        self.specs = [specs(S)[n] for n in names]
        self.files = [build(S, sp) for sp in self.specs]
        self.outs = [H.HeicDecoder.decode(f) for f in self.files]
        self.gains = [H.HeicDecoder.decode(f, item_id=o.image.gain_map.item_id) for f, o in zip(self.files, self.outs)]
        self.alphas = [H.HeicDecoder.decode(f, item_id=o.image.display.alpha_item_id) if sp[8] is not None else None
                       for f, o, sp in zip(self.files, self.outs, self.specs)]

    def pick(self, ks):
        """The batch of pictures ks (a picture may repeat)."""
        b = object.__new__(Batch)
        b.names, b.specs, b.files = [self.names[k] for k in ks], [self.specs[k] for k in ks], [self.files[k] for k in ks]
        b.outs, b.gains, b.alphas = [self.outs[k] for k in ks], [self.gains[k] for k in ks], [self.alphas[k] for k in ks]
        return b

    def transforms(self, colorspace, fmt, pq_bits, headroom=4.0, display_headroom=None, sdr_white=203.0):
        return [o.image.gain_transform(g.image, colorspace, "pq" if fmt.endswith("pq") else "linear", pq_bits, headroom,
                                       display_headroom, sdr_white) for o, g in zip(self.outs, self.gains)]

    def reference(self, k, t, fmt, scale):
        """gain_scale_ref.render of picture k for scale (ow, oh, x, y, w, h)."""
        o, g, al, sp = self.outs[k], self.gains[k], self.alphas[k], self.specs[k]
        planes = [None if p is None else host(p) for p in (o.y, o.cb, o.cr)]
        ow, oh, x, y, w, h = scale
        return gain_scale_ref.render(t, *planes, o.info.matrix_coeffs, bool(o.info.full_range), host(g.y), sp[2],
                                     (x, y, w, h) if w or h else None, ow, oh, with_alpha=fmt.startswith("rgba"),
                                     alpha=None if al is None else host(al.y),
                                     alpha_depth=8 if al is None else al.info.bit_depth)


@pytest.fixture(scope="module")
def batch8(H, S):
    return Batch(H, S, ("wide-iso", "turned-apple", "ratio-iso", "deepmap-apple"))


@pytest.fixture(scope="module")
def batch10(H, S):
    return Batch(H, S, ("422-iso", "deep-apple"))


@pytest.fixture(scope="module")
def batch_long(H, S):
    return Batch(H, S, ("long", "long-turned"))


def raw(H, ctx, b, fmt, scales, ts, pad=None, with_alphas=True):
    """heifgpu_render_batch_gain_scaled with scales[i] = (ow, oh, x, y, w, h) into sentinel-filled
    buffers whose pitch is the row plus pad[i] bytes, with a guard row above and below; returns
    (rc, [buffer as (oh + 2, pitch) uint8 device tensor])."""
    from heif_amd import _lib

    f = _lib.HDR_FORMATS[fmt]
    bpp, n = (8 if fmt.startswith("rgba") else 6), len(b.outs)
    surf, sc, bufs = (_lib.Surface * n)(), (_lib.Scale * n)(), []
    for i in range(n):
        sc[i] = _lib.Scale(*scales[i])
        pitch = scales[i][0] * bpp + (pad[i] if pad else 0)
        buf = torch.full((scales[i][1] + 2, pitch), SENTINEL, dtype=torch.uint8, device="cuda:0")
        surf[i].pixels, surf[i].pitch = buf.data_ptr() + pitch, pitch
        bufs.append(buf)
    alphas = b.alphas if with_alphas and fmt.startswith("rgba") and any(a is not None for a in b.alphas) else None
    imgs, aimgs, aplanes = ctx._render_args(b.outs, alphas)
    gimgs, _, _ = ctx._render_args(b.gains, None)
    xf = (ctypes.c_void_p * n)(*[ctypes.addressof(t) for t in ts])
    rc = _lib.lib.heifgpu_render_batch_gain_scaled(ctx._h, imgs, n, ctx.planes_of(b.outs), gimgs, ctx.planes_of(b.gains), aimgs,
                                                   aplanes, f, sc, xf, surf,
                                                   ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    torch.cuda.synchronize()
    return rc, bufs


def pixels(buf, ow, fmt):
    """The (oh, ow, C) uint16 pixels of a buffer raw() filled, and everything else of it."""
    a = buf.cpu().numpy()
    row = ow * (8 if fmt.startswith("rgba") else 6)
    px = np.ascontiguousarray(a[1:-1, :row]).view(np.uint16).reshape(a.shape[0] - 2, ow, 4 if fmt.startswith("rgba") else 3)
    rest = np.concatenate([a[0], a[-1], a[1:-1, row:].ravel()])
    return px, rest


def check_raw(H, ctx, b, fmt, colorspace, pq_bits, scales, pad=None):
    ts = b.transforms(colorspace, fmt, pq_bits)
    rc, bufs = raw(H, ctx, b, fmt, scales, ts, pad)
    assert rc == 0
    for k, (buf, t, sc) in enumerate(zip(bufs, ts, scales)):
        got, rest = pixels(buf, sc[0], fmt)
        want = b.reference(k, t, fmt, sc)
        assert got.shape == want.shape, (b.names[k], got.shape, want.shape)
        assert np.array_equal(got, want), (b.names[k], fmt, colorspace, sc, int((got != want).sum()))
        assert (rest == SENTINEL).all(), (b.names[k], sc)  # nothing outside ow x oh pixels is written
    return bufs


def whole(o):
    return (o.image.display.out_width, o.image.display.out_height, 0, 0, 0, 0)


# ---- 1. the identity ----------------------------------------------------------
@pytest.mark.parametrize("which,fmt,pq_bits", [("8", "rgba16f", 10), ("8", "rgb16pq", 10), ("10", "rgb16f", 10), ("10", "rgba16pq", 12)])
def test_identity_is_render_hdr(H, ctx, batch8, batch10, which, fmt, pq_bits):
    """At the displayed size over the whole picture every average is the value itself: the
    new kernel writes what k_render_gain writes, on both of its tile paths."""
    b = batch8 if which == "8" else batch10
    assert [o.image.display.m[0] == 0 for o in batch8.outs] == [False, True, True, False]  # axes kept and swapped
    ts = b.transforms("display-p3", fmt, pq_bits)
    want = ctx.render_hdr(b.outs, b.gains, fmt, "display-p3", 4.0, None, 203.0, pq_bits, b.alphas, transforms=ts)
    rc, bufs = raw(H, ctx, b, fmt, [whole(o) for o in b.outs], ts)
    assert rc == 0
    for k, (buf, w) in enumerate(zip(bufs, want)):
        got, rest = pixels(buf, w.shape[1], fmt)
        assert np.array_equal(got, bits_of(w)), (b.names[k], fmt, int((got != bits_of(w)).sum()))
        assert (rest == SENTINEL).all()


# ---- 2. ratios, against the reference -----------------------------------------
RATIO_CONFIGS = [("rgba16f", "display-p3", 10), ("rgb16pq", "srgb", 10), ("rgb16pq", "bt2020", 16)]


@pytest.mark.parametrize("fmt,colorspace,pq_bits", RATIO_CONFIGS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in RATIO_CONFIGS])
def test_ratios(H, ctx, batch8, fmt, colorspace, pq_bits):
    """320 x 48 -> 100 x 20 (3.2 and 2.4) and -> 160 x 24 (2 : 1, coinciding with the 2 : 1 map);
    the 61 x 41 clap picture under irot 3 (41 x 61 displayed) -> 90 x 70, enlarging, and -> 1 x 1;
    a window at an odd offset and of odd size: footprints end inside a column pair and inside
    a map cell.  One call for the five."""
    b = batch8.pick([0, 0, 2, 2, 0])
    assert (b.outs[2].image.display.out_width, b.outs[2].image.display.out_height) == (41, 61)
    scales = [(100, 20, 0, 0, 0, 0), (160, 24, 0, 0, 0, 0), (90, 70, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0), (20, 11, 3, 5, 57, 31)]
    bufs = check_raw(H, ctx, b, fmt, colorspace, pq_bits, scales)
    if fmt == "rgba16f":  # the alpha image's average, and HDR levels above SDR white
        a = pixels(bufs[0], 100, fmt)[0][..., 3].view(np.float16)
        assert float(a.max()) <= 1.0 and len(np.unique(a)) > 8
        assert float(pixels(bufs[2], 90, fmt)[0][..., :3].view(np.float16).max()) > 1.0


# ---- 3. map geometry and depth; 6. one batch, padded pitches, sentinels --------
def test_map_geometries_in_one_batch(H, ctx, batch8, batch10):
    """Same-size map (axes swapped), 2 : 1 map, the 40 x 24 map under 96 x 64, a 10-bit map
    beside a u8 base; then the 10-bit 4:2:2 base with an 8-bit map: pictures of different sizes
    and orientations into different scales in one call, into buffers with padded pitches."""
    for b in (batch8, batch10):  # (the planes are what the test reads: from the reference alone)
        for o, g, sp in zip(b.outs, b.gains, b.specs):
            if g.info.width < o.info.width and not any(k == "clap" for k, _ in sp[2]):  # the whole picture is the window
                assert gain_ref.borders_bind(o.info.width, g.info.width) == (True, True)
                assert gain_ref.borders_bind(o.info.height, g.info.height) == (True, True)
    scales = [(77, 13, 0, 0, 0, 0), (20, 100, 0, 0, 0, 0), (17, 23, 0, 0, 0, 0), (30, 17, 0, 0, 0, 0)]
    pad = [(-(sc[0] * 8) % 4) + 6 for sc in scales]  # pitch 2 mod 4: most rows start off a dword
    check_raw(H, ctx, batch8, "rgba16f", "display-p3", 10, scales, pad)
    pad = [(-(sc[0] * 6) % 4) + 6 for sc in scales]
    check_raw(H, ctx, batch8, "rgb16pq", "srgb", 12, scales, pad)
    scales10 = [(31, 40, 0, 0, 0, 0), (29, 17, 0, 0, 0, 0)]
    assert batch10.outs[0].info.chroma_format_idc == 2 and batch10.gains[0].info.bit_depth == 8
    check_raw(H, ctx, batch10, "rgba16pq", "bt2020", 10, scales10, [6, 2])
    check_raw(H, ctx, batch10, "rgb16f", "srgb", 10, scales10, [2, 6])


def test_unclapped_ratio_map_binds_both_borders(H, S, ctx, batch8):
    """The 96 x 64 picture without its clap (the decoded planes under a header that only turns
    them): the window is the whole picture, where both clamps of the 40 x 24 map bind."""
    sp = list(specs(S)["ratio-iso"])
    sp[2] = [("irot", 3)]
    b = Batch(H, S, ("ratio-iso",))
    f = build(S, tuple(sp))
    img = H.HeifImage.parse(f)
    b.specs, b.outs = [tuple(sp)], [H.DecodedImage(b.outs[0].y, b.outs[0].cb, b.outs[0].cr, b.outs[0].info, img)]
    assert (img.display.out_width, img.display.out_height) == (64, 96)
    assert gain_ref.borders_bind(96, 40) == (True, True) and gain_ref.borders_bind(64, 24) == (True, True)
    check_raw(H, ctx, b, "rgb16f", "display-p3", 10, [(23, 37, 0, 0, 0, 0)])


# ---- 4. the chunk boundary ------------------------------------------------------
@pytest.mark.parametrize("fmt,pq_bits", [("rgb16f", 10), ("rgba16pq", 16)])
def test_footprint_straddles_a_chunk(H, ctx, batch_long, fmt, pq_bits):
    """1056 source columns to 31: output 15 reads columns 510.97 .. 545.03, across column 512,
    where one chunk of column sums ends and the next begins; axes kept and swapped."""
    b = batch_long
    assert [o.image.display.m[0] == 0 for o in b.outs] == [False, True]
    assert 15 * 1056 // 31 < 512 < 16 * 1056 // 31
    check_raw(H, ctx, b, fmt, "srgb", pq_bits, [(31, 2, 0, 0, 0, 0), (2, 31, 0, 0, 0, 0)])


# ---- 5. wide sums ---------------------------------------------------------------
def filled(H, S, bw, bh, gw, gh, luma, gain_plane):
    """A base of constant luma (monochrome, 8 bits) and a 12-bit gain plane under parsed headers."""
    P = S.SynthParams
    f = S.gainmap_heic(P(width=bw, height=bh, chroma_format=0), P(width=gw, height=gh, chroma_format=0, bit_depth=12), kind="apple")
    base = H.HeifImage.parse(f)
    gimg = H.HeifImage.parse(f, base.gain_map.item_id)
    assert (base.info.width, base.info.height, gimg.info.width, gimg.info.height, gimg.info.bit_depth) == (bw, bh, gw, gh, 12)
    y = luma if torch.is_tensor(luma) else torch.full((bh, bw), luma, dtype=torch.uint8, device="cuda:0")
    b = object.__new__(Batch)
    b.names, b.specs, b.files = ["filled"], [(None, 0, [], None, None, 0, "apple", None, None)], [f]
    b.outs = [H.DecodedImage(y, None, None, base.info, base)]
    b.gains = [H.DecodedImage(gain_plane, None, None, gimg.info, gimg)]
    b.alphas = [None]
    return b


def test_column_sum_above_32_bits(H, S, ctx):
    """A 16 x 4224 base with an 8 x 2112 12-bit map whose codes lie near maxg, to 2 x 1: the
    column sum of g over the one output line passes 2^32.  Random luma and map, the numpy
    reference, and the sums once more in Python integers."""
    rng = np.random.default_rng(51)
    G = (4095 - rng.integers(0, 40, (2112, 8))).astype(np.uint16)
    Y = rng.integers(0, 256, (4224, 16)).astype(np.uint8)
    b = filled(H, S, 16, 4224, 8, 2112, torch.from_numpy(Y).cuda(), torch.from_numpy(G.view(np.int16)).cuda())
    gq = gain_ref.sample_map(G, 16, 4224)
    assert int(gq[:, 0].sum()) > 1 << 32
    want_g = [(2 * 2 * int(gq[:, 8 * X:8 * X + 8].sum()) + 16 * 4224) // (2 * 16 * 4224) for X in range(2)]
    assert gain_scale_ref.average_codes(gq, None, 2, 1)[0].tolist() == want_g
    check_raw(H, ctx, b, "rgb16f", "srgb", 10, [(2, 1, 0, 0, 0, 0)])
    check_raw(H, ctx, b, "rgb16pq", "display-p3", 12, [(1, 2, 0, 0, 0, 0)])


def test_numerator_above_2_46(H, S, ctx):
    """An 8192 x 4104 base (2^25 pixels and more) with a 12-bit map near maxg, to 1 x 1 and to
    2 x 1: the numerator passes 2^46, the column sums 2^32.  The map varies along one axis only
    (rows for 1 x 1, columns for 2 x 1), so the gain code depends on that coordinate alone and the
    reference is a plain sum in Python integers over one line, times the other side."""
    bw, bh, gw, gh = 8192, 4104, 64, 40
    rng = np.random.default_rng(52)
    from heif_amd import _lib

    for axis, (ow, oh) in ((0, (1, 1)), (1, (2, 1))):
        line = (4095 - rng.integers(0, 3, gh if axis == 0 else gw)).astype(np.uint16)
        G = np.repeat(line[:, None], gw, axis=1) if axis == 0 else np.repeat(line[None, :], gh, axis=0)
        G = np.ascontiguousarray(G)
        b = filled(H, S, bw, bh, gw, gh, 180, torch.from_numpy(G.view(np.int16)).cuda())
        # the codes along the axis that varies: a map of one column (row) under a base of one
        codes = gain_ref.sample_map(line[:, None], 1, bh)[:, 0] if axis == 0 else gain_ref.sample_map(line[None, :], bw, 1)[0]
        full = gain_ref.sample_map(G, 64, 64)  # (spot check on a small base: the code does not depend on the other axis)
        assert (full == full[:, :1]).all() if axis == 0 else (full == full[:1]).all()
        if axis == 0:
            sums = [bw * sum(int(v) for v in codes)]
        else:
            sums = [bh * sum(int(v) for v in codes[X * bw // 2:(X + 1) * bw // 2]) for X in range(2)]
        nums = [2 * s * ow * oh + bw * bh for s in sums]
        assert min(nums) > 1 << 46
        Gq = np.array([[n // (2 * bw * bh) for n in nums]], np.int64)
        assert Gq.shape == (oh, ow) and Gq.min() > MAXCODE - 3 * 256
        for fmt, pq_bits in (("rgb16f", 10), ("rgb16pq", 16)):
            t = b.transforms("srgb", fmt, pq_bits)[0]
            o = b.outs[0]
            C = display_of_constant(o, 180, int(t.bits))
            want = gain_ref.apply_tables(gain_ref.tables(t), np.broadcast_to(C, (oh, ow, 3)), Gq)
            rc, bufs = raw(H, ctx, b, fmt, [(ow, oh, 0, 0, 0, 0)], [t])
            assert rc == 0
            got, rest = pixels(bufs[0], ow, fmt)
            assert np.array_equal(got, want), (axis, fmt, got, want)
            assert (rest == SENTINEL).all()
        del b
    assert _lib.lib.heifgpu_abi_version() == 6


def display_of_constant(o, luma, bits):
    """The base's integers of a constant monochrome picture: (3,) int64."""
    import display_ref

    y = np.full((1, 1), luma, np.uint8)
    return display_ref.rgb_at_depth(y, None, None, o.info.matrix_coeffs, bool(o.info.full_range), bits)[0, 0]


# ---- 6. the Python surface --------------------------------------------------------
def test_python_surface(H, ctx, batch8):
    """render_hdr_scaled: one (N, h, w, C) tensor for cover, stretch and windows, a list for
    contain; float16 / uint16; the pixels of the C call."""
    b = batch8
    ts = b.transforms("display-p3", "rgba16f", 10)
    got = ctx.render_hdr_scaled(b.outs, b.gains, (20, 30), "stretch", "rgba16f", "display-p3", 4.0, alphas=b.alphas)
    assert got.dtype == torch.float16 and tuple(got.shape) == (4, 20, 30, 4)
    for k, t in enumerate(ts):
        assert np.array_equal(bits_of(got[k]), b.reference(k, t, "rgba16f", (30, 20, 0, 0, 0, 0))), b.names[k]
    cover = ctx.render_hdr_scaled(b.outs, b.gains, (16, 16), "cover", "rgb16pq", "srgb", 4.0, pq_bits=12)
    assert cover.dtype == torch.uint16 and tuple(cover.shape) == (4, 16, 16, 3)
    from heif_amd import _lib
    import scale_ref

    tq = b.transforms("srgb", "rgb16pq", 12)
    for k, o in enumerate(b.outs):
        d = o.image.display
        sc = scale_ref.fit(d.out_width, d.out_height, 16, 16, "cover")
        assert np.array_equal(bits_of(cover[k]), b.reference(k, tq[k], "rgb16pq", sc)), b.names[k]
    contain = ctx.render_hdr_scaled(b.outs, b.gains, (24, 24), "contain", "rgb16f", "srgb", 4.0)
    assert isinstance(contain, list) and [tuple(c.shape) for c in contain] == [
        (scale_ref.fit(o.image.display.out_width, o.image.display.out_height, 24, 24, "contain")[1],
         scale_ref.fit(o.image.display.out_width, o.image.display.out_height, 24, 24, "contain")[0], 3) for o in b.outs]
    wins = ctx.render_hdr_scaled(b.outs[:1], b.gains[:1], (11, 20), fmt="rgb16f", colorspace="srgb", windows=[(3, 5, 57, 31)])
    tl = b.transforms("srgb", "rgb16f", 10)
    assert np.array_equal(bits_of(wins[0]), b.reference(0, tl[0], "rgb16f", (20, 11, 3, 5, 57, 31)))
    with pytest.raises(ValueError):
        ctx.render_hdr_scaled(b.outs, b.gains, (8, 8), fmt="rgb16")
    assert _lib.HDR_FORMATS["rgb16f"] == _lib.PIX_HDR_RGB16F


# ---- 7. refusals ------------------------------------------------------------------
def test_refusals_launch_nothing(H, S, ctx, batch8):
    """Every refusal answers before anything is launched: the surfaces keep their sentinel."""
    from heif_amd import _lib

    b = batch8
    ts = b.transforms("srgb", "rgb16f", 10)

    def refused(exc, code=None, **kw):
        out = [torch.full((9, 13, 3), 0x5A5A, dtype=torch.int16, device="cuda") for _ in b.outs]
        args = dict(outs=b.outs, gains=b.gains, size=(9, 13), mode="stretch", fmt="rgb16f", colorspace="srgb", headroom=4.0,
                    transforms=ts, out=out)
        args.update(kw)
        with pytest.raises(exc) as e:
            ctx.render_hdr_scaled(**args)
        if code is not None:
            assert e.value.code == code, e.value
        torch.cuda.synchronize()
        assert all(bool((s == 0x5A5A).all()) for s in out)

    # a window-decoded image
    win = H.HeicDecoder.decode(b.files[2], window=(0, 0, 16, 16))
    assert win.valid is not None
    refused(H.UnsupportedError, _lib.HEIFGPU_E_UNSUPPORTED, outs=b.outs[:2] + [win] + b.outs[3:])
    # an image set to bilinear chroma
    b.outs[0].image.chroma_upsampling = "bilinear"
    try:
        refused(H.UnsupportedError, _lib.HEIFGPU_E_UNSUPPORTED)
    finally:
        b.outs[0].image.chroma_upsampling = "replicate"
    # a cropped gain map under the base's m (the identity here)
    sp = b.specs[3]
    cropped = S.gainmap_heic(sp[0], sp[4], seed=sp[1], gain_seed=sp[5], kind="apple",
                             gain_transforms=(S.clap_box(32, 1, 24, 1, 0, 1, 0, 1),), colr=sp[3])
    cg = H.HeicDecoder.decode(cropped, item_id=2)
    assert list(cg.image.display.m) == list(b.outs[3].image.display.m) and cg.image.display.out_width == 32
    refused(H.UnsupportedError, _lib.HEIFGPU_E_UNSUPPORTED, gains=b.gains[:3] + [cg])
    # a window outside the picture (the 72 x 40 picture's)
    refused(H.HeifGpuError, _lib.HEIFGPU_E_INVALID, windows=[(0, 0, 8, 8)] * 3 + [(70, 0, 8, 8)])
    # ... and the same call with good arguments writes every surface
    out = [torch.full((9, 13, 3), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.float16) for _ in b.outs]
    res = ctx.render_hdr_scaled(b.outs, b.gains, (9, 13), "stretch", "rgb16f", "srgb", 4.0, transforms=ts, out=out)
    assert isinstance(res, list) and res[0] is out[0]
    for k, t in enumerate(ts):
        assert np.array_equal(bits_of(out[k]), b.reference(k, t, "rgb16f", (13, 9, 0, 0, 0, 0))), b.names[k]


# ---- 8. decode_hdr(size=) on the project's own HDR photo ----------------------------
def test_decode_hdr_size_halfmoonbay(H, ctx, halfmoonbay):
    """decode_hdr(size=(756, 1008)) (contain: 567 x 756 of the 3024 x 4032 displayed picture,
    16 source pixels to 3) against the reference computed from the planes the GPU decoded, on
    three blocks of 48 x 48 output pixels, two of them corners.  An output block that starts
    at a multiple of 3 reads exactly a 256 x 256 block of the displayed picture, with weights
    in the same proportion as the whole render's: the same rounded quotient.  (The numpy
    reference of the whole picture would take a unit test too long.)"""
    import display_ref

    data = halfmoonbay
    got = H.HeicDecoder.decode_hdr(data, headroom=4.0, size=(756, 1008))
    base = H.HeicDecoder.decode(data)
    gain = H.HeicDecoder.decode(data, item_id=base.image.gain_map.item_id)
    d = base.image.display
    oh, ow = got.shape[0], got.shape[1]
    assert got.dtype == torch.float16 and got.shape[2] == 3
    assert (ow * 256, oh * 256) == (d.out_width * 48, d.out_height * 48), (ow, oh)
    t = base.image.gain_transform(gain.image, "display-p3", "linear", 10, headroom=4.0)
    tb = gain_ref.tables(t)
    W, Hh = base.info.width, base.info.height
    y, cb, cr, G = host(base.y), host(base.cb), host(base.cr), host(gain.y)
    x0s, x1s, fxs, _ = gain_ref.taps(W, G.shape[1])
    y0s, y1s, fys, _ = gain_ref.taps(Hh, G.shape[0])
    Gi = G.astype(np.int64)
    out = bits_of(got)
    for X0, Y0 in ((0, 0), (ow - 48, oh - 48), (3 * 70, 3 * 101)):
        # the displayed block and the decoded window it shows
        oy, ox = np.mgrid[Y0 * 256 // 48:Y0 * 256 // 48 + 256, X0 * 256 // 48:X0 * 256 // 48 + 256]
        sx, sy = d.m[0] * ox + d.m[1] * oy + d.t[0], d.m[2] * ox + d.m[3] * oy + d.t[1]
        wx, wy = int(sx.min()), int(sy.min())
        assert int(sx.max()) - wx == 255 and int(sy.max()) - wy == 255
        ys, xs = slice(wy, wy + 256), slice(wx, wx + 256)
        rows, cols = (np.arange(wy, wy + 256) >> 1)[:, None], (np.arange(wx, wx + 256) >> 1)[None, :]
        px = display_ref.rgb_at_depth(y[ys, xs], cb[rows, cols], cr[rows, cols], base.info.matrix_coeffs,
                                      bool(base.info.full_range), 8)
        fx, fy = fxs[xs][None, :], fys[ys][:, None]
        top = (256 - fx) * Gi[y0s[ys]][:, x0s[xs]] + fx * Gi[y0s[ys]][:, x1s[xs]]
        bot = (256 - fx) * Gi[y1s[ys]][:, x0s[xs]] + fx * Gi[y1s[ys]][:, x1s[xs]]
        gq = ((256 - fy) * top + fy * bot + 128) >> 8
        want = gain_scale_ref.from_displayed(tb, px[sy - wy, sx - wx], gq[sy - wy, sx - wx], None, 8, None, 48, 48, False)
        assert np.array_equal(out[Y0:Y0 + 48, X0:X0 + 48], want), (X0, Y0)
    # without a size decode_hdr does what it did: render_hdr's picture
    full = H.HeicDecoder.decode_hdr(data, headroom=4.0)
    same = ctx.render_hdr([base], [gain], "rgb16f", "display-p3", 4.0)[0]
    assert tuple(full.shape) == (d.out_height, d.out_width, 3) and torch.equal(full.view(torch.int16), same.view(torch.int16))
