"""The PNG output on the device: heifgpu_png_encode_batch through ctypes into sentinel-filled
buffers on every case of tests/png_cases.py, whole against the model (tests/png_ref.py); the
too-small capacity; the refused arguments; DecodeContext.encode_png and its retry; and
render_png / decode_png end to end on the golden HEIC and a synthetic 10-bit file with alpha."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest

import png_cases as pc
import png_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5
ROOM = 64  # sentinel bytes kept behind every capacity


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
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def body_of(name):
    data, head, _ = pc.reference(name)
    return data[head:]


def chunks(data):
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack_from(">I", data, at)
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert zlib.crc32(kind + body) == struct.unpack_from(">I", data, at + 8 + n)[0], kind
        out.append((kind, body))
        at += 12 + n
    return out


def encode_raw(H, ctx, cases, caps, opts=None, widths=None, heights=None, pitches=None, n=None):
    """heifgpu_png_encode_batch on the cases' surfaces into buffers of caps[i] + ROOM sentinel bytes
    (capacity caps[i]); the keyword arguments replace what the cases state.  Returns (rc, size
    words, output buffers as bytes)."""
    L = H._lib
    fmt, bits, filt = cases[0].opts
    o = opts if opts is not None else L.PngOpts(pc.FORMAT_CODES[fmt], bits, filt, 0)
    k = len(cases)
    src, dst = (L.Surface * k)(), (L.Surface * k)()
    keep, outs = [], []
    for i, c in enumerate(cases):
        buf, pitch = pc.surface(c)
        t = torch.from_numpy(buf).cuda()
        keep.append(t)
        src[i].pixels = t.data_ptr() + c.lead
        src[i].pitch = pitches[i] if pitches else pitch
        b = torch.full((caps[i] + ROOM,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        outs.append(b)
        dst[i].pixels = b.data_ptr()
        dst[i].pitch = caps[i]
    ws = (ctypes.c_uint32 * k)(*(widths or [c.px.shape[1] for c in cases]))
    hs = (ctypes.c_uint32 * k)(*(heights or [c.px.shape[0] for c in cases]))
    sizes = torch.full((k,), -1, dtype=torch.int64, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    rc = L.lib.heifgpu_png_encode_batch(ctx._h, k if n is None else n, src, ws, hs, ctypes.byref(o), dst,
                                        ctypes.cast(sizes.data_ptr(), ctypes.POINTER(ctypes.c_uint64)), stream)
    torch.cuda.synchronize()
    return rc, [int(v) & (2 ** 64 - 1) for v in sizes.cpu().tolist()], [bytes(b.cpu().numpy()) for b in outs]


@pytest.mark.parametrize("batch", pc.BATCHES, ids=lambda b: b[0].name)
def test_cases_equal_model(H, ctx, batch):
    """Every case, 7 bytes of capacity to spare: exact size, the model's bytes, the sentinel behind them."""
    bodies = [body_of(c.name) for c in batch]
    rc, sizes, outs = encode_raw(H, ctx, batch, [len(s) + 7 for s in bodies])
    assert rc == H._lib.HEIFGPU_OK, H._lib.last_error()
    for c, s, size, out in zip(batch, bodies, sizes, outs):
        assert size == len(s), c.name
        assert out[:size] == s, c.name
        assert out[size:] == bytes([SENTINEL]) * (7 + ROOM), c.name


def test_too_small_capacity(H, ctx):
    """Nothing at or past the capacity is written, the bytes that fit are the first, and the size
    comes back exact with bit 63 set; a picture beside it that fits is whole.  Then the same on a
    picture of three blocks, whose later chunks lie wholly past the capacity."""
    batch = pc.BATCHES[0]
    bodies = [body_of(c.name) for c in batch]
    for cap0 in (0, 1, len(bodies[0]) // 2, len(bodies[0]) - 1):
        caps = [cap0, len(bodies[1]), len(bodies[2]) - 1]
        rc, sizes, outs = encode_raw(H, ctx, batch, caps)
        assert rc == H._lib.HEIFGPU_OK, H._lib.last_error()
        for s, cap, size, out in zip(bodies, caps, sizes, outs):
            assert size == len(s) | (H._lib.PNG_TOO_SMALL if cap < len(s) else 0)
            assert out[:cap] == s[:cap]
            assert out[cap:] == bytes([SENTINEL]) * ROOM
    three = [pc.BY_NAME["stream_65540"]]
    s = body_of(three[0].name)
    for cap in (0, 1, len(s) // 2, len(s) - 1):
        rc, sizes, outs = encode_raw(H, ctx, three, [cap])
        assert rc == H._lib.HEIFGPU_OK, H._lib.last_error()
        assert sizes[0] == len(s) | H._lib.PNG_TOO_SMALL
        assert outs[0][:cap] == s[:cap] and outs[0][cap:] == bytes([SENTINEL]) * ROOM


def test_refused_arguments(H, ctx):
    """E_INVALID before any launch: the outputs and the size words keep what they held."""
    L = H._lib
    c = [pc.BY_NAME["odd_5x3"]]
    good = dict(opts=L.PngOpts(0, 8, 5, 0))
    bad = [dict(opts=L.PngOpts(4, 8, 5, 0)), dict(opts=L.PngOpts(0, 10, 5, 0)), dict(opts=L.PngOpts(2, 7, 5, 0)),
           dict(opts=L.PngOpts(3, 17, 5, 0)), dict(opts=L.PngOpts(0, 8, 6, 0)), dict(opts=L.PngOpts(0, 8, 5, 1)),
           dict(good, widths=[0]), dict(good, heights=[0]), dict(good, widths=[65536]), dict(good, heights=[65536]),
           dict(good, pitches=[3 * 5 - 1]), dict(good, n=65536)]
    for kw in bad:
        rc, sizes, outs = encode_raw(H, ctx, c, [256], **kw)
        assert rc == L.HEIFGPU_E_INVALID, kw
        assert sizes == [2 ** 64 - 1] and outs[0] == bytes([SENTINEL]) * (256 + ROOM), kw
    rc, sizes, _ = encode_raw(H, ctx, c, [4096], **good)
    assert rc == L.HEIFGPU_OK and sizes[0] < 4096


def test_encode_png_mixed_batch(H, ctx):
    """DecodeContext.encode_png on three pictures of different sizes with strided rows, a profile on one;
    then a 16-bit RGBA list with bits=12 and a cICP chunk."""
    batch = pc.BATCHES[0]
    pics = []
    for c in batch:
        h, w, _ = c.px.shape
        wide = torch.zeros((h, w + 5, 3), dtype=torch.uint8, device="cuda:0")
        wide[:, :w] = torch.from_numpy(c.px).cuda()
        pics.append(wide[:, :w])
    icc = [None, bytes(range(200)), None]
    got = ctx.encode_png(pics, icc_profiles=icc)
    for c, p, g in zip(batch, icc, got):
        assert g == ref.encode(c.px, "rgb8", icc=p)
    deep = [pc.smooth(33, 9, 3, 4, 4095), pc.noise(7, 21, 4, 4, 4095)]
    got = ctx.encode_png([torch.from_numpy(d.view(np.int16)).cuda() for d in deep], bits=12, filter="paeth", cicp=(9, 16, 0, 1))
    for d, g in zip(deep, got):
        assert g == ref.encode(d, "rgba16", 12, 4, cicp=(9, 16, 0, 1))
        assert dict(chunks(g))[b"cICP"] == bytes((9, 16, 0, 1)) and dict(chunks(g))[b"sBIT"] == bytes([12] * 4)
    with pytest.raises(ValueError):
        ctx.encode_png(pics, srgb=True, cicp=(1, 13, 0, 1))


def test_encode_png_retries_a_picture_that_does_not_fit(H, ctx, monkeypatch):
    """Noise does not compress: against a first guess of half the filtered bytes the picture is
    encoded again with the size the device stated; a flat picture beside it fits at once."""
    rgb = pc.noise(300, 200, 77)
    want = ref.encode(rgb, "rgb8")
    assert len(want) - 33 > 200 * 901 // 2 + 64
    flat = np.full((24, 40, 3), 90, np.uint8)
    assert len(ref.encode(flat, "rgb8")) - 33 < 24 * 121 // 2 + 64
    monkeypatch.setattr(H.DecodeContext, "_png_first_guess", staticmethod(lambda filtered: filtered // 2 + 64))
    got = ctx.encode_png([torch.from_numpy(rgb).cuda(), torch.from_numpy(flat).cuda()])
    assert got[0] == want and got[1] == ref.encode(flat, "rgb8")
    whole = ctx.encode_png(torch.from_numpy(np.stack([flat, flat])).cuda())  # an (N, h, w, 3) tensor
    assert whole == [got[1], got[1]]


def test_render_png_halfmoonbay(H, ctx, halfmoonbay):
    """render_png of the golden HEIC scaled to 756 x 1008 is the model fed render_scaled's pixels,
    carries the item's ICC profile, and Pillow decodes it to exactly those pixels."""
    from PIL import Image

    img = H.HeifImage.parse(halfmoonbay)
    outs = ctx.alloc_outputs([img])
    batch = ctx.prepare([img])
    batch.decode_async(outs)
    assert batch.status() == [0]
    batch.free()
    got = ctx.render_png(outs, size=(1008, 756))[0]
    rgb = host(ctx.render_scaled(outs, (1008, 756), "cover", "rgb8")[0])
    assert rgb.shape == (1008, 756, 3)
    assert got == ref.encode(rgb, "rgb8", icc=img.icc_profile)
    im = Image.open(io.BytesIO(got))
    im.load()
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)
    assert img.icc_profile and im.info["icc_profile"] == img.icc_profile
    assert H.HeicDecoder.decode_png(halfmoonbay, size=(1008, 756)) == got
    kinds = [k for k, _ in chunks(ctx.render_png(outs, size=(64, 64), colorspace="srgb")[0])]
    assert b"sRGB" in kinds and b"iCCP" not in kinds
    p3 = dict(chunks(ctx.render_png(outs, size=(64, 64), colorspace="display-p3")[0]))
    assert p3[b"cICP"] == bytes((12, 13, 0, 1))


def test_decode_png_ten_bit_alpha(H):
    """A synthetic 10-bit picture with an alpha image: RGBA of 16 bits with sBIT 10, whose samples
    shifted down by 6 are decode_display's."""
    from heif_amd import synth_encoder as S

    p = S.SynthParams(width=64, height=48, bit_depth=10)
    a = S.SynthParams(width=64, height=48, chroma_format=0, bit_depth=10)
    f = S.display_heic(p, seed=50, transforms=(S.imir_box(0),), aux=(S.AuxImage(a, seed=51),))
    shown = host(H.HeicDecoder.decode_display(f))
    assert shown.shape == (48, 64, 4) and shown.dtype == np.uint16
    got = H.HeicDecoder.decode_png(f)
    cs = chunks(got)
    assert cs[0] == (b"IHDR", struct.pack(">IIBBBBB", 64, 48, 16, 6, 0, 0, 0))
    assert dict(cs)[b"sBIT"] == bytes([10] * 4)
    assert got == ref.encode(shown, "rgba16", 10)
    stream = zlib.decompress(b"".join(b for k, b in cs if k == b"IDAT"))
    assert len(stream) == 48 * (64 * 8 + 1)
    windowed = H.HeicDecoder.decode_png(f, size=(24, 24), tiles="window")
    assert windowed == H.HeicDecoder.decode_png(f, size=(24, 24))


def test_pq_surface_with_cicp(H, ctx):
    """What render_hdr(fmt="rgb16pq") writes (16-bit words of pq_bits bits) with cicp=: the chunk is there,
    sBIT states the bits and the samples come back."""
    pq = pc.smooth(40, 30, 5, 3, 1023)
    got = ctx.encode_png([torch.from_numpy(pq.view(np.int16)).cuda()], bits=10, cicp=(9, 16, 0, 1))[0]
    cs = dict(chunks(got))
    assert cs[b"cICP"] == bytes((9, 16, 0, 1)) and cs[b"sBIT"] == bytes([10] * 3)
    assert got == ref.encode(pq, "rgb16", 10, cicp=(9, 16, 0, 1))
