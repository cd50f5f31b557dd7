"""The HDR render on the device: render / render_scaled (three filters) / render_tensor /
decode_display with colorspace= and tone_map="bt2390" against tone_ref's numpy formula
applied to what display_ref, scale_ref, resample_ref and tensor_ref give for the planes
the GPU decoded, byte for byte.  The tables the formula reads come from the library and
are checked against the float64 model in tests/test_tone.py; here only the kernels are
under test.

A 10-bit batch: a PQ BT.2020 4:2:2 picture turned by irot 1 (the transposing LDS path,
partial tiles) with an alpha image and a clli of MaxCLL 400, an HLG BT.2020 picture
mirrored, a PQ P3 picture cropped at an odd offset with no light-level box, an SDR picture
with the Display P3 profile (the managed path inside the tone kernels) and an unlabelled
one (identity to sRGB: untouched).  An 8-bit batch, PQ, HLG and SDR, for the 1-byte
kernels.  The seeds were picked on the CPU with the oracle so that every HDR picture has
pixels in every region of its tone curve (coverage(), asserted below)."""
import numpy as np
import pytest

import color_ref
import display_ref
import resample_ref
import scale_ref
import tensor_ref
import tone_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SPACES = ("srgb", "display-p3")
TONE = "bt2390"
CLAP = ("clap", (41, 1, 29, 1, 1, 2, 1, 2))  # 41 x 29 at left 15, top 5 of 70 x 38
SIZE = (16, 24)  # (h, w) of the scaled renders


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


def specs(S, depth):
    """name -> (params, seed, display steps, colr boxes, further properties, alpha params, Lsrc or None for SDR)."""
    p3 = S.icc_profile(S.ICC_COLORANTS_DISPLAY_P3, S.ICC_SRGB_PARA, raw_colorants=True)
    P = S.SynthParams
    return {
        "pq2020": (P(width=136, height=72, conf_right=6, chroma_format=2, bit_depth=depth), 61, [("irot", 1)],
                   [S.nclx_box(9, 16, 9, False)], (S.clli_box(400, 90),),
                   P(width=136, height=72, conf_right=6, chroma_format=0, bit_depth=depth), 400.0),
        "hlg2020": (P(width=72, height=40, bit_depth=depth), 62, [("imir", 0)], [S.nclx_box(9, 18, 9, False)], (), None, 1000.0),
        "pqp3": (P(width=72, height=40, conf_right=2, conf_bottom=2, bit_depth=depth), 63, [CLAP],
                 [S.nclx_box(12, 16, 1, True)], (), None, 1000.0),
        "sdr-p3": (P(width=72, height=40, chroma_format=3, bit_depth=depth), 64, [], [S.icc_box(p3)], (), None, None),
        "unlabelled": (P(width=64, height=64, bit_depth=depth), 65, [], [], (), None, None),
    }


def build(S, spec):
    p, seed, steps, colr, props, ap, _ = spec
    aux = (S.AuxImage(ap, seed=seed + 100, urn=S.ALPHA_URN_MPEGB),) if ap is not None else ()
    return S.display_heic(p, seed=seed, transforms=boxes(S, steps) + tuple(props), colr=colr, aux=aux)


def displayed(planes, info, steps, fmt, alpha=None, alpha_depth=8):
    y, cb, cr = planes
    return display_ref.render(y, cb, cr, info.matrix_coeffs, bool(info.full_range), info.bit_depth, steps, fmt,
                              alpha=alpha if fmt.startswith("rgba") else None, alpha_depth=alpha_depth)


def coverage(t, D, lsrc, want_above):
    """What the pixels of a displayed picture D reach of tone transform t, from the reference
    side: (below the knee, inside the spline, above the source peak, the index octaves missing
    between the lowest and the highest one reached)."""
    _, in32, w, *_ = tone_ref.tables(t)
    _, Y = tone_ref.luminance(in32, w, D[..., :3].reshape(-1, 3))
    model = tone_ref.Model(9, t.transfer, "srgb", lsrc)
    light = model.display_light(tone_ref.WHITE * Y / tone_ref.U)
    knee = tone_ref.knee(model.lsrc)
    _, e, _ = tone_ref.index(Y)
    octs = set(e.tolist())  # 0: the unit-spaced nodes below 64
    missing = set(range(min(octs), max(octs) + 1)) - octs
    return bool((light < knee).any()), bool(((light >= knee) & (light < model.lsrc)).any()), \
        bool((light > model.lsrc).any()) or not want_above, missing


class Batch:
    """The pictures decoded once (never written to), their alpha images, and the displayed
    picture D of each by display_ref, per format."""

    def __init__(self, H, S, depth, names):
        self.names, self.depth = list(names), depth
        self.specs = [specs(S, depth)[n] for n in names]
        self.files = [build(S, sp) for sp in self.specs]
        self.outs = [H.HeicDecoder.decode(f) for f in self.files]
        self.alphas = [H.HeicDecoder.decode(f, item_id=2) if sp[5] is not None else None for f, sp in zip(self.files, self.specs)]
        self._D = {}

    def D(self, fmt):
        if fmt not in self._D:
            self._D[fmt] = [displayed([None if t is None else host(t) for t in (o.y, o.cb, o.cr)], o.info, sp[2], fmt,
                                      None if al is None else host(al.y), 8 if al is None else al.info.bit_depth)
                            for o, al, sp in zip(self.outs, self.alphas, self.specs)]
        return self._D[fmt]

    def transforms(self, space, fmt, tone_map=TONE):
        return [o.image.color_transform(space, self.depth if fmt.endswith("16") else 8, tone_map) for o in self.outs]

    def hdr(self):
        return [k for k, sp in enumerate(self.specs) if sp[6] is not None]


@pytest.fixture(scope="module")
def batch10(H, S):
    return Batch(H, S, 10, ("pq2020", "hlg2020", "pqp3", "sdr-p3", "unlabelled"))


@pytest.fixture(scope="module")
def batch8(H, S):
    return Batch(H, S, 8, ("pq2020", "hlg2020", "sdr-p3"))


def test_sources_as_the_batch_needs_them(batch10, batch8):
    """What the other tests rely on: which pictures get a tone transform, their peaks, the
    opt-in, and that every HDR picture reaches every region of its curve."""
    for b, fmts in ((batch10, ("rgb8", "rgb16")), (batch8, ("rgb8",))):
        for fmt in fmts:
            ts = b.transforms("srgb", fmt)
            assert [tone_ref.is_tone(t) for t in ts] == [sp[6] is not None for sp in b.specs]
            for k in b.hdr():
                assert ts[k].Lsrc == b.specs[k][6]
                below, inside, above, missing = coverage(ts[k], b.D(fmt)[k], b.specs[k][6], b.names[k] == "pq2020")
                assert below and inside and above and not missing, (b.names[k], fmt, below, inside, above, missing)
    assert [tuple(d.shape) for d in batch10.D("rgb8")] == [(130, 72, 3), (40, 72, 3), (29, 41, 3), (40, 72, 3), (64, 64, 3)]
    o = batch10.outs[0]
    assert o.info.chroma_format_idc == 2 and o.image.hdr.max_cll == 400 and batch10.outs[2].image.hdr.max_cll is None
    assert batch10.outs[3].image.hdr is None and batch10.transforms("srgb", "rgb8")[4].identity == 1


def check_render(ctx, b, fmt):
    plain = [host(t) for t in ctx.render(b.outs, fmt, b.alphas)]
    for k, D in enumerate(b.D(fmt)):
        assert np.array_equal(plain[k], D), k  # the default path is what it was
    for space in SPACES:
        ts = b.transforms(space, fmt)
        got = [host(t) for t in ctx.render(b.outs, fmt, b.alphas, colorspace=space, tone_map=TONE)]
        for k, (D, t) in enumerate(zip(b.D(fmt), ts)):
            assert np.array_equal(got[k], tone_ref.transform_picture(t, D)), (space, b.names[k])
            if fmt.startswith("rgba"):
                assert np.array_equal(got[k][..., 3], plain[k][..., 3]), (space, k)  # alpha untouched
            if tone_ref.is_tone(t):
                assert (got[k][..., :3] != plain[k][..., :3]).any()
        # the SDR pictures of the same call: exactly today's colorspace=-only result
        sdr = [k for k in range(len(b.outs)) if k not in b.hdr()]
        today = ctx.render([b.outs[k] for k in sdr], fmt, [b.alphas[k] for k in sdr], colorspace=space)
        for k, t in zip(sdr, today):
            assert np.array_equal(got[k], host(t)), (space, b.names[k])
    if fmt.startswith("rgba"):
        assert len(np.unique(plain[0][..., 3])) > 4


@pytest.mark.parametrize("fmt", ["rgb8", "rgba8", "rgb16", "rgba16"])
def test_render(ctx, batch10, fmt):
    check_render(ctx, batch10, fmt)


@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
def test_render_8bit_sources(ctx, batch8, fmt):
    check_render(ctx, batch8, fmt)


def test_without_tone_map_the_batch_is_refused_as_ever(H, ctx, batch8):
    o = batch8.outs[0]
    assert tuple(ctx.render([o])[0].shape) == (130, 72, 3)
    for call in (lambda: ctx.render(batch8.outs, colorspace="srgb"), lambda: ctx.render_scaled([o], SIZE, colorspace="srgb"),
                 lambda: ctx.render_tensor([o], SIZE, colorspace="display-p3")):
        with pytest.raises(H.UnsupportedError):
            call()
    with pytest.raises(ValueError):
        ctx.render([o], tone_map=TONE)
    with pytest.raises(ValueError):
        ctx.render([o], colorspace="srgb", tone_map="reinhard")


def scaled_refs(b, fmt, name):
    """The integers render_scaled(mode="stretch", filter=name) gives, per picture."""
    oh, ow = SIZE
    if name == "area":
        return [scale_ref.area_average(D, None, ow, oh) for D in b.D(fmt)]
    bits = b.depth if fmt.endswith("16") else 8
    return [resample_ref.resize(D, None, ow, oh, name, bits=bits) for D in b.D(fmt)]


@pytest.mark.parametrize("name", ["area", "bilinear", "bicubic"])
def test_render_scaled(ctx, batch10, batch8, name):
    for b, fmts in ((batch10, ("rgba8", "rgb16")), (batch8, ("rgb8",))):
        for fmt in fmts:
            Rs = scaled_refs(b, fmt, name)
            plain = host(ctx.render_scaled(b.outs, SIZE, "stretch", fmt, b.alphas, filter=name))
            for k, R in enumerate(Rs):
                assert np.array_equal(plain[k], R), (name, fmt, k)
            for space in SPACES:
                ts = b.transforms(space, fmt)
                got = host(ctx.render_scaled(b.outs, SIZE, "stretch", fmt, b.alphas, colorspace=space, filter=name,
                                             tone_map=TONE))
                for k, (R, t) in enumerate(zip(Rs, ts)):
                    assert np.array_equal(got[k], tone_ref.transform_picture(t, R)), (name, fmt, space, b.names[k])
                sdr = [k for k in range(len(b.outs)) if k not in b.hdr()]
                today = host(ctx.render_scaled([b.outs[k] for k in sdr], SIZE, "stretch", fmt, [b.alphas[k] for k in sdr],
                                               colorspace=space, filter=name))
                for j, k in enumerate(sdr):
                    assert np.array_equal(got[k], today[j]), (name, fmt, space, b.names[k])


def test_render_tensor(ctx, batch10, batch8):
    a, bb = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    for b in (batch10, batch8):
        flips = [k & 3 for k in range(len(b.outs))]
        for name in ("area", "bicubic"):
            Rs = scaled_refs(b, "rgb8", name)
            for space in SPACES:
                ts = b.transforms(space, "rgb8")
                got = bits_of(ctx.render_tensor(b.outs, SIZE, "stretch", dtype=torch.float16, layout="chw", flips=flips,
                                                colorspace=space, filter=name, tone_map=TONE))
                for k, (R, t) in enumerate(zip(Rs, ts)):
                    want = tensor_ref.tensor(tone_ref.transform_picture(t, R), a, bb, "f16", "chw", flip=flips[k])
                    assert np.array_equal(got[k], want), (name, space, b.names[k])


def test_decode_display(H, ctx, batch10):
    """One file, named: the alpha image found by itself, the file's peak and the caller's."""
    f = batch10.files[0]
    D = batch10.D("rgba16")[0]
    for space in SPACES:
        t = batch10.outs[0].image.color_transform(space, 10, TONE)
        got = host(H.HeicDecoder.decode_display(f, colorspace=space, tone_map=TONE))
        assert np.array_equal(got, tone_ref.transform_picture(t, D)), space
    t = batch10.outs[0].image.color_transform("srgb", 10, TONE, 1000.0)
    assert t.Lsrc == 1000.0
    got = host(H.HeicDecoder.decode_display(f, colorspace="srgb", tone_map=TONE, peak_nits=1000.0))
    want = tone_ref.transform_picture(t, D)
    assert np.array_equal(got, want)
    assert (want != tone_ref.transform_picture(batch10.outs[0].image.color_transform("srgb", 10, TONE), D)).any()
    oh, ow = SIZE
    R = scale_ref.area_average(batch10.D("rgb8")[0], None, ow, oh)
    t8 = batch10.outs[0].image.color_transform("display-p3", 8, TONE)
    got = host(H.HeicDecoder.decode_display(f, "rgb8", size=SIZE, mode="stretch", colorspace="display-p3", tone_map=TONE))
    assert np.array_equal(got, tone_ref.transform_picture(t8, R))
    a, bb = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
    got = bits_of(H.HeicDecoder.decode_tensor(f, SIZE, "stretch", colorspace="display-p3", tone_map=TONE))
    assert np.array_equal(got, tensor_ref.tensor(tone_ref.transform_picture(t8, R), a, bb, "f16", "chw"))
    with pytest.raises(H.UnsupportedError):
        H.HeicDecoder.decode_display(f, colorspace="srgb")


def test_back_to_back_calls_share_the_cache(ctx, batch10, batch8):
    """Two calls with different tables (other depth, other space, a managed-only call between
    them) back to back on one stream with no synchronisation in between; then again, warm."""
    torch.cuda.synchronize()
    sdr = [3, 4]
    runs = []
    for _ in range(2):
        first = ctx.render(batch10.outs, "rgb16", colorspace="srgb", tone_map=TONE)
        second = ctx.render(batch8.outs, "rgb8", colorspace="display-p3", tone_map=TONE)
        third = ctx.render([batch10.outs[k] for k in sdr], "rgb16", colorspace="srgb")
        fourth = ctx.render(batch10.outs[::-1], "rgb8", colorspace="display-p3", tone_map=TONE)
        runs.append((first, second, third, fourth))
    torch.cuda.synchronize()
    for first, second, third, fourth in runs:
        for k, (D, t) in enumerate(zip(batch10.D("rgb16"), batch10.transforms("srgb", "rgb16"))):
            assert np.array_equal(host(first[k]), tone_ref.transform_picture(t, D)), k
        for k, (D, t) in enumerate(zip(batch8.D("rgb8"), batch8.transforms("display-p3", "rgb8"))):
            assert np.array_equal(host(second[k]), tone_ref.transform_picture(t, D)), k
        for j, k in enumerate(sdr):
            assert np.array_equal(host(third[j]), host(first[k])), k
        for k, (D, t) in enumerate(zip(batch10.D("rgb8")[::-1], batch10.transforms("display-p3", "rgb8")[::-1])):
            assert np.array_equal(host(fourth[k]), tone_ref.transform_picture(t, D)), k
