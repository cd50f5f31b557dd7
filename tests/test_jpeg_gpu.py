"""The JPEG output on the device: heifgpu_jpeg_encode_batch through ctypes into sentinel-filled
buffers on every case of tests/jpeg_cases.py, whole against the numpy model (tests/jpeg_ref.py);
the too-small capacity; the refused arguments; DecodeContext.encode_jpeg; and render_jpeg end
to end on the golden HEIC."""
import ctypes
import io

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_ref as ref

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


def scan_of(name):
    data, head, _ = jc.reference(name)
    return data[head:]


def encode_raw(H, ctx, cases, caps, opts=None, widths=None, heights=None, pitches=None, n=None):
    """heifgpu_jpeg_encode_batch on the cases' surfaces into buffers of caps[i] + ROOM sentinel bytes
    (capacity caps[i]); the keyword arguments replace what the cases state.  Returns (rc, size
    words, output buffers as bytes)."""
    L = H._lib
    q, sub, restart = cases[0].opts
    o = opts if opts is not None else L.JpegOpts(q, L.JPEG_SUBSAMPLINGS[sub], restart, 0)
    k = len(cases)
    src, dst = (L.Surface * k)(), (L.Surface * k)()
    keep, outs = [], []
    for i, c in enumerate(cases):
        buf, pitch = jc.surface(c)
        t = torch.from_numpy(buf).cuda()
        keep.append(t)
        src[i].pixels = t.data_ptr() + c.lead
        src[i].pitch = pitches[i] if pitches else pitch
        b = torch.full((caps[i] + ROOM,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        outs.append(b)
        dst[i].pixels = b.data_ptr()
        dst[i].pitch = caps[i]
    ws = (ctypes.c_uint32 * k)(*(widths or [c.rgb.shape[1] for c in cases]))
    hs = (ctypes.c_uint32 * k)(*(heights or [c.rgb.shape[0] for c in cases]))
    sizes = torch.full((k,), -1, dtype=torch.int64, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    rc = L.lib.heifgpu_jpeg_encode_batch(ctx._h, k if n is None else n, src, ws, hs, ctypes.byref(o), dst,
                                         ctypes.cast(sizes.data_ptr(), ctypes.POINTER(ctypes.c_uint64)), stream)
    torch.cuda.synchronize()
    return rc, [int(v) & (2 ** 64 - 1) for v in sizes.cpu().tolist()], [bytes(b.cpu().numpy()) for b in outs]


@pytest.mark.parametrize("batch", jc.BATCHES, ids=lambda b: b[0].name)
def test_cases_equal_model(H, ctx, batch):
    """Every case, 7 bytes of capacity to spare: exact size, the model's bytes, the sentinel behind them."""
    scans = [scan_of(c.name) for c in batch]
    rc, sizes, outs = encode_raw(H, ctx, batch, [len(s) + 7 for s in scans])
    assert rc == H._lib.HEIFGPU_OK, H._lib.last_error()
    for c, s, size, out in zip(batch, scans, sizes, outs):
        assert size == len(s), c.name
        assert out[:size] == s, c.name
        assert out[size:] == bytes([SENTINEL]) * (7 + ROOM), c.name


def test_too_small_capacity(H, ctx):
    """Nothing at or past the capacity is written, the bytes that fit are the scan's first, and
    the size comes back exact with bit 63 set; a picture beside it that fits is whole."""
    batch = jc.BATCHES[0]
    scans = [scan_of(c.name) for c in batch]
    for cap0 in (0, 1, len(scans[0]) // 2, len(scans[0]) - 1):
        caps = [cap0, len(scans[1]), len(scans[2]) - 1]
        rc, sizes, outs = encode_raw(H, ctx, batch, caps)
        assert rc == H._lib.HEIFGPU_OK, H._lib.last_error()
        for s, cap, size, out in zip(scans, caps, sizes, outs):
            assert size == len(s) | (H._lib.JPEG_TOO_SMALL if cap < len(s) else 0)
            assert out[:cap] == s[:cap]
            assert out[cap:] == bytes([SENTINEL]) * ROOM


def test_refused_arguments(H, ctx):
    """E_INVALID before any launch: the outputs and the size words keep what they held."""
    L = H._lib
    c = [jc.BY_NAME["size_17x9_4:2:0"]]
    good = dict(opts=L.JpegOpts(90, L.JPEG_420, 0, 0))
    bad = [dict(opts=L.JpegOpts(0, L.JPEG_420, 0, 0)), dict(opts=L.JpegOpts(101, L.JPEG_420, 0, 0)),
           dict(good, widths=[0]), dict(good, heights=[0]), dict(good, widths=[65536]), dict(good, heights=[65536]),
           dict(good, pitches=[3 * 17 - 1]), dict(good, n=65536)]
    for kw in bad:
        rc, sizes, outs = encode_raw(H, ctx, c, [256], **kw)
        assert rc == L.HEIFGPU_E_INVALID, kw
        assert sizes == [2 ** 64 - 1] and outs[0] == bytes([SENTINEL]) * (256 + ROOM), kw
    rc, sizes, _ = encode_raw(H, ctx, c, [4096], **good)
    assert rc == L.HEIFGPU_OK and sizes[0] < 4096


def test_encode_jpeg_mixed_batch(H, ctx):
    """DecodeContext.encode_jpeg on three pictures of different sizes with strided rows, a profile on one."""
    batch = jc.BATCHES[0]
    pics = []
    for c in batch:
        h, w, _ = c.rgb.shape
        wide = torch.zeros((h, w + 5, 3), dtype=torch.uint8, device="cuda:0")
        wide[:, :w] = torch.from_numpy(c.rgb).cuda()
        pics.append(wide[:, :w])
    icc = [None, bytes(range(200)), None]
    q, sub, restart = batch[0].opts
    got = ctx.encode_jpeg(pics, q, sub, icc, restart)
    for c, p, g in zip(batch, icc, got):
        assert g == ref.encode(c.rgb, q, sub, restart, p)


def test_encode_jpeg_retries_a_picture_that_does_not_fit(H, ctx):
    """Noise at quality 100, 4:4:4, is several bytes per pixel: past the first guess of capacity."""
    rgb = jc.noise(128, 128, 77)
    want = ref.encode(rgb, 100, "4:4:4", 0, fast=True)
    assert len(want) > 128 * 128 * 1.25 + 4096 + 1000
    flat = np.full((24, 40, 3), 90, np.uint8)
    got = ctx.encode_jpeg([torch.from_numpy(rgb).cuda(), torch.from_numpy(flat).cuda()], 100, "4:4:4")
    assert got[0] == want and got[1] == ref.encode(flat, 100, "4:4:4")
    whole = ctx.encode_jpeg(torch.from_numpy(np.stack([flat, flat])).cuda(), 100, "4:4:4")  # an (N, h, w, 3) tensor
    assert whole == [got[1], got[1]]


def test_render_jpeg_halfmoonbay(H, ctx, halfmoonbay):
    """render_jpeg is the model fed render()'s pixels, Pillow decodes it to the displayed size and
    finds the item's ICC profile in it; the same with size=(224, 224)."""
    from PIL import Image

    img = H.HeifImage.parse(halfmoonbay)
    outs = ctx.alloc_outputs([img])
    batch = ctx.prepare([img])
    batch.decode_async(outs)
    assert batch.status() == [0]
    batch.free()
    d = img.display
    for size, shape in ((None, (d.out_height, d.out_width)), ((224, 224), (224, 224))):
        got = ctx.render_jpeg(outs, size=size)[0]
        rgb = (ctx.render(outs, "rgb8")[0] if size is None else ctx.render_scaled(outs, size, "cover", "rgb8")[0]).cpu().numpy()
        assert rgb.shape == shape + (3,)
        assert got == ref.encode(rgb, 90, "4:2:0", 0, img.icc_profile, fast=True)
        im = Image.open(io.BytesIO(got))
        im.load()
        assert im.size == (shape[1], shape[0]) and im.mode == "RGB"
        assert img.icc_profile and im.info["icc_profile"] == img.icc_profile
    assert H.HeicDecoder.decode_jpeg(halfmoonbay, size=(224, 224)) == got
    assert "icc_profile" not in Image.open(io.BytesIO(ctx.render_jpeg(outs, size=(64, 64), colorspace="srgb")[0])).info
