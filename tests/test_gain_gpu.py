"""The gain-map HDR render on the device: DecodeContext.render_hdr and HeicDecoder.decode_hdr
against gain_ref's numpy formula over display_ref, computed from the planes the GPU decoded,
byte for byte.  The tables the formula reads come from the library and are checked against
the float64 rules in tests/test_gain.py; here the kernel is under test.

An 8-bit batch in one call: a 320 x 48 picture with a 160 x 24 map, mirrored (the axis-keeping
path, 2 x 3 workgroups), with a Display P3 profile, an alpha image and an ISO map with offsets
(k_a > k_b), gamma 1.4 and min < 0; a 320 x 48 picture with a same-size Apple map turned by
irot 1 (the transposing path, 1 x 5 workgroups), nclx; a 96 x 64 picture with a 40 x 24 map
(ratios 2.4 and 2.67) under an odd-offset clap and irot 3, ISO with max 8 stops and a base offset of 1, Display P3 profile (H' passes 2^24 - 1 into sRGB); a 72 x 40
picture with a 10-bit map (a u16 gain plane beside a u8 base).  A 10-bit batch: a 4:2:2 base
with an 8-bit map, turned, and a 4:2:0 base with a 10-bit map and a 10-bit alpha image.  The
seeds were picked on the CPU with the oracle so that every clamp of the formula and both border
clamps of the sampler bind in these vectors (asserted below from the reference alone)."""
import numpy as np
import pytest

import gain_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CLAP = ("clap", (61, 1, 41, 1, 3, 2, 1, 2))  # 61 x 41 at left 19, top 12 of 96 x 64
SENTINEL = 0x5A5A


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

    def transforms(self, colorspace, fmt, pq_bits, headroom, display_headroom, sdr_white=203.0):
        return [o.image.gain_transform(g.image, colorspace, "pq" if fmt.endswith("pq") else "linear", pq_bits, headroom,
                                       display_headroom, sdr_white) for o, g in zip(self.outs, self.gains)]

    def reference(self, k, t, fmt, parts=None):
        o, g, al, sp = self.outs[k], self.gains[k], self.alphas[k], self.specs[k]
        planes = [None if p is None else host(p) for p in (o.y, o.cb, o.cr)]
        return gain_ref.render(t, *planes, o.info.matrix_coeffs, bool(o.info.full_range), host(g.y), sp[2],
                               with_alpha=fmt.startswith("rgba"), alpha=None if al is None else host(al.y),
                               alpha_depth=8 if al is None else al.info.bit_depth, parts=parts)


@pytest.fixture(scope="module")
def batch8(H, S):
    return Batch(H, S, ("wide-iso", "turned-apple", "ratio-iso", "deepmap-apple"))


@pytest.fixture(scope="module")
def batch10(H, S):
    return Batch(H, S, ("422-iso", "deep-apple"))


def check(ctx, b, fmt, colorspace, pq_bits, headroom, display_headroom, sdr_white=203.0):
    got = ctx.render_hdr(b.outs, b.gains, fmt, colorspace, headroom, display_headroom, sdr_white, pq_bits, b.alphas)
    ts = b.transforms(colorspace, fmt, pq_bits, headroom, display_headroom, sdr_white)
    for k, (g, t) in enumerate(zip(got, ts)):
        assert g.dtype == (torch.uint16 if fmt.endswith("pq") else torch.float16)
        want = b.reference(k, t, fmt)
        assert tuple(g.shape) == want.shape, (b.names[k], g.shape, want.shape)
        assert np.array_equal(bits_of(g), want), (b.names[k], fmt, colorspace, int((bits_of(g) != want).sum()))
    return got


def test_batches_are_what_the_tests_need(batch8, batch10):
    kinds = [o.image.gain_map.kind for o in batch8.outs + batch10.outs]
    assert kinds == ["iso", "apple", "iso", "apple", "iso", "apple"]
    assert [g.info.bit_depth for g in batch8.gains] == [8, 8, 8, 10] and [o.info.bit_depth for o in batch8.outs] == [8] * 4
    assert [(g.info.width, g.info.height) for g in batch8.gains] == [(160, 24), (320, 48), (40, 24), (40, 24)]
    assert batch10.outs[0].info.chroma_format_idc == 2 and [a is not None for a in batch10.alphas] == [False, True]
    assert [o.image.display.m[0] == 0 for o in batch8.outs] == [False, True, True, False]  # both paths of the kernel
    # the clamps and the sampler's borders, from the reference alone
    seen = dict(h_low=False, h2_low=False, h2_high=False)
    for cs, dh in (("srgb", None), ("display-p3", 2.5)):
        for k, t in enumerate(batch8.transforms(cs, "rgb16f", 10, 4.0, dh)):
            parts = {}
            batch8.reference(k, t, "rgb16f", parts)
            seen["h_low"] |= bool((parts["H"] < 0).any())
            seen["h2_low"] |= bool((parts["H2"] < 0).any())
            seen["h2_high"] |= bool((parts["H2"] > gain_ref.LEVEL_MAX).any())
    assert all(seen.values()), seen
    assert gain_ref.borders_bind(320, 160) == (True, True) and gain_ref.borders_bind(64, 24) == (True, True)
    assert len(set(gain_ref.taps(96, 40)[2].tolist())) >= 12  # many residues fx


CONFIGS = [  # (fmt, colorspace, pq_bits, headroom, display_headroom)
    ("rgba16f", "display-p3", 10, 4.0, 2.5),
    ("rgb16f", "srgb", 10, 4.0, None),
    ("rgb16pq", "bt2020", 10, 4.0, 2.5),
    ("rgba16pq", "display-p3", 16, 8.0, None),
]


@pytest.mark.parametrize("fmt,colorspace,pq_bits,headroom,dh", CONFIGS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CONFIGS])
def test_render_hdr_8bit_batch(ctx, batch8, fmt, colorspace, pq_bits, headroom, dh):
    got = check(ctx, batch8, fmt, colorspace, pq_bits, headroom, dh)
    if fmt == "rgba16f":
        a = got[0][..., 3].float()
        assert float(a.max()) <= 1.0 and bool((got[1][..., 3] == 1.0).all())  # an alpha image; an opaque picture
        assert float(got[2][..., :3].float().max()) > 1.0  # above SDR white


@pytest.mark.parametrize("fmt,colorspace,pq_bits", [("rgba16f", "bt2020", 10), ("rgba16pq", "srgb", 12), ("rgb16pq", "display-p3", 16)])
def test_render_hdr_10bit_batch(ctx, batch10, fmt, colorspace, pq_bits):
    check(ctx, batch10, fmt, colorspace, pq_bits, 3.0, None, sdr_white=100.0)


def test_decode_hdr_halfmoonbay(H, ctx):
    """decode_hdr of the project's own HDR photo against the reference on three 256 x 256
    windows of the decoded picture, two of them corners (the whole 12-megapixel numpy reference
    would take a unit test too long)."""
    from conftest import ROOT

    data = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    got = H.HeicDecoder.decode_hdr(data, headroom=4.0)
    assert got.dtype == torch.float16 and got.shape[2] == 3
    with pytest.raises(H.HeifGpuError):
        H.HeicDecoder.decode_hdr(data)  # an Apple map needs the caller's headroom
    base = H.HeicDecoder.decode(data)
    gain = H.HeicDecoder.decode(data, item_id=base.image.gain_map.item_id)
    d = base.image.display
    assert (got.shape[0], got.shape[1]) == (d.out_height, d.out_width)
    t = base.image.gain_transform(gain.image, "display-p3", "linear", 10, headroom=4.0)
    tb = gain_ref.tables(t)
    W, Hh = base.info.width, base.info.height
    y, cb, cr, G = host(base.y), host(base.cb), host(base.cr), host(gain.y)
    import display_ref

    out = bits_of(got)
    oy, ox = np.mgrid[0:d.out_height, 0:d.out_width]
    sx_of, sy_of = d.m[0] * ox + d.m[1] * oy + d.t[0], d.m[2] * ox + d.m[3] * oy + d.t[1]
    x0s, x1s, fxs, _ = gain_ref.taps(W, G.shape[1])
    y0s, y1s, fys, _ = gain_ref.taps(Hh, G.shape[0])
    Gi = G.astype(np.int64)
    for wx, wy in ((0, 0), (W - 256, Hh - 256), (1777, 1301)):
        ys, xs = slice(wy, wy + 256), slice(wx, wx + 256)
        # chroma indexed from the absolute position (rgb_at_depth then takes it as 4:4:4)
        Y = y[ys, xs]
        rows, cols = (np.arange(wy, wy + 256) >> 1)[:, None], (np.arange(wx, wx + 256) >> 1)[None, :]
        px = display_ref.rgb_at_depth(Y, cb[rows, cols], cr[rows, cols], base.info.matrix_coeffs, bool(base.info.full_range), 8)
        fx, fy = fxs[xs][None, :], fys[ys][:, None]
        top = (256 - fx) * Gi[y0s[ys]][:, x0s[xs]] + fx * Gi[y0s[ys]][:, x1s[xs]]
        bot = (256 - fx) * Gi[y1s[ys]][:, x0s[xs]] + fx * Gi[y1s[ys]][:, x1s[xs]]
        gqw = ((256 - fy) * top + fy * bot + 128) >> 8
        want = gain_ref.apply_tables(tb, px, gqw)
        sel = (sx_of >= wx) & (sx_of < wx + 256) & (sy_of >= wy) & (sy_of < wy + 256)
        assert int(sel.sum()) == 256 * 256
        assert np.array_equal(out[sel], want[sy_of[sel] - wy, sx_of[sel] - wx]), (wx, wy)
    with pytest.raises(ValueError):
        from heif_amd import synth_encoder as S

        H.HeicDecoder.decode_hdr(S.display_heic(S.SynthParams(width=16, height=16)))


def test_refusals_launch_nothing(H, S, ctx, batch8):
    """Every refusal answers before anything is launched: the surfaces keep their sentinel."""
    from heif_amd import _lib

    b = batch8
    ts = b.transforms("srgb", "rgb16f", 10, 4.0, None)

    def surfaces():
        return [torch.full((o.image.display.out_height, o.image.display.out_width, 3), SENTINEL, dtype=torch.int16, device="cuda")
                for o in b.outs]

    def refused(code, **kw):
        out = surfaces()
        args = dict(outs=b.outs, gains=b.gains, fmt="rgb16f", colorspace="srgb", headroom=4.0, transforms=ts, out=out)
        args.update(kw)
        with pytest.raises(H.HeifGpuError) as e:
            ctx.render_hdr(**args)
        assert e.value.code == code, e.value
        torch.cuda.synchronize()
        assert all(bool((s == SENTINEL).all()) for s in out)

    # a chroma-bilinear image
    b.outs[0].image.chroma_upsampling = "bilinear"
    try:
        refused(_lib.HEIFGPU_E_UNSUPPORTED)
    finally:
        b.outs[0].image.chroma_upsampling = "replicate"
    # a window-decoded image
    f = b.files[2]
    win = H.HeicDecoder.decode(f, window=(0, 0, 16, 16))
    assert win.valid is not None
    refused(_lib.HEIFGPU_E_UNSUPPORTED, outs=b.outs[:2] + [win] + b.outs[3:])
    # a gain image with a display map of its own that is not the base's
    sp = b.specs[3]
    foreign = S.gainmap_heic(sp[0], sp[4], seed=sp[1], gain_seed=sp[5], kind="apple", gain_transforms=(S.irot_box(2),), colr=sp[3])
    fg = H.HeicDecoder.decode(foreign, item_id=2)
    refused(_lib.HEIFGPU_E_UNSUPPORTED, gains=b.gains[:3] + [fg])
    # the boundary of "the base's": the base's own m (the identity here) over a crop of the map is foreign
    cropped = S.gainmap_heic(sp[0], sp[4], seed=sp[1], gain_seed=sp[5], kind="apple",
                             gain_transforms=(S.clap_box(32, 1, 24, 1, 0, 1, 0, 1),), colr=sp[3])
    cg = H.HeicDecoder.decode(cropped, item_id=2)
    assert list(cg.image.display.m) == list(b.outs[3].image.display.m) and cg.image.display.out_width == 32
    refused(_lib.HEIFGPU_E_UNSUPPORTED, gains=b.gains[:3] + [cg])
    # ... and the base's irot over the map's whole picture is the base's (what Apple's files carry)
    sp1 = b.specs[1]
    turned = S.gainmap_heic(sp1[0], sp1[4], seed=sp1[1], gain_seed=sp1[5], kind="apple", transforms=boxes(S, sp1[2]),
                            gain_transforms=boxes(S, sp1[2]), colr=sp1[3])
    tg = H.HeicDecoder.decode(turned, item_id=2)
    assert tg.image.display.m[0] == 0
    same = ctx.render_hdr(b.outs[:2], [b.gains[0], tg], "rgb16f", "srgb", 4.0, transforms=ts[:2])
    want = ctx.render_hdr(b.outs[:2], b.gains[:2], "rgb16f", "srgb", 4.0, transforms=ts[:2])
    assert torch.equal(same[1].view(torch.int16), want[1].view(torch.int16))
    # transforms that disagree with the images or the format
    pq = b.transforms("srgb", "rgb16pq", 10, 4.0, None)
    refused(_lib.HEIFGPU_E_INVALID, transforms=pq)  # made for the other encoding
    refused(_lib.HEIFGPU_E_INVALID, transforms=ts[:3] + [ts[0]])  # gain_bits 8 beside a 10-bit map
    deep = _lib.GainTransform.from_buffer_copy(ts[1])
    deep.bits = 10
    refused(_lib.HEIFGPU_E_INVALID, transforms=[ts[0], deep] + ts[2:])
    big = _lib.GainTransform.from_buffer_copy(ts[1])
    big.T[100] = (1 << 24) + 1
    refused(_lib.HEIFGPU_E_INVALID, transforms=[ts[0], big] + ts[2:])
    # a NULL transform and a pitch too small, at the C boundary
    out = surfaces()
    imgs, _, _ = ctx._render_args(b.outs, None)
    gimgs, _, _ = ctx._render_args(b.gains, None)
    import ctypes

    xf = (ctypes.c_void_p * 4)(*[ctypes.addressof(t) for t in ts])
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def call(xf_arr, surf):
        return _lib.lib.heifgpu_render_batch_gain(ctx._h, imgs, 4, ctx.planes_of(b.outs), gimgs, ctx.planes_of(b.gains), None,
                                                  None, _lib.PIX_HDR_RGB16F, xf_arr, surf, stream)

    null_xf = (ctypes.c_void_p * 4)(xf[0], xf[1], None, xf[3])
    assert call(null_xf, ctx._surfaces(out)) == _lib.HEIFGPU_E_INVALID
    narrow = ctx._surfaces(out)
    narrow[2].pitch -= 2
    assert call(xf, narrow) == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_render_batch_gain(ctx._h, imgs, 4, ctx.planes_of(b.outs), gimgs, ctx.planes_of(b.gains), None, None,
                                              _lib.PIX_RGB16, xf, ctx._surfaces(out), stream) == _lib.HEIFGPU_E_INVALID
    torch.cuda.synchronize()
    assert all(bool((s == SENTINEL).all()) for s in out)
