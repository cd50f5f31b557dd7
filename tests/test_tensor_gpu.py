"""The tensor render on the device: heifgpu_render_batch_tensor /
DecodeContext.render_tensor against tensor_ref.tensor over the integer picture
scale_ref.area_average(display_ref.render(planes the GPU decoded)), so only
k_render_scaled's tensor epilogue and the host's flip are under test.  Every
comparison is on the bit patterns of the elements, exact.  Pictures and sizes
are tests/test_scale_gpu.py's: a few CTBs, 130 x 72 and 262 x 24 displayed, the
smallest that give partial tiles on both of the kernel's paths; 37 and 19 are
odd widths (a ragged last element for the packed stores), 65 ends one pixel
into a second 64-pixel segment, 36 is even."""
import ctypes

import numpy as np
import pytest

import display_ref
import scale_ref
import tensor_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SOURCES = ("rgb8", "rgba8", "rgb16", "rgba16")
ELEMS = {"f32": (0, 4), "f16": (1, 2), "bf16": (2, 2)}  # code, bytes
LAYOUTS = {"chw": 0, "hwc": 1}
ORIENTATIONS = [[("irot", k)] + m for k in range(4) for m in ([], [("imir", 0)])]
SWAPPED = (2, 3, 6, 7)  # the orientations that show the picture turned
SENTINEL = 0xA5


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


def bits(t):
    """The bit patterns of a float tensor as numpy unsigned integers."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


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


def want(D, scale):
    ow, oh, x, y, w, h = scale
    return scale_ref.area_average(D, (x, y, w, h) if w or h else None, ow, oh)


def tensor_raw(H, ctx, outs, src, elem, layout, scales, a, b, flips=None, alphas=None, padded=False, sync=True):
    """heifgpu_render_batch_tensor with scales[i] = (ow, oh, x, y, w, h) into
    sentinel-filled byte buffers.  padded: stride_y exceeds the row (and is 2 mod 4
    for the 2-byte elements, so that every other row starts off a dword), stride_c
    exceeds the plane, and the base is one element into the buffer.
    Returns (rc, [(buffer, offset, stride_c, stride_y)])."""
    from heif_amd import _lib

    code, esz = ELEMS[elem]
    C, n = (4 if src.startswith("rgba") else 3), len(outs)
    fmt = _lib.TensorFormat(src=_lib.PIX_FORMATS[src], elem=code, layout=LAYOUTS[layout])
    for c in range(C):
        fmt.a[c], fmt.b[c] = a[c], b[c]
    surf, sc, bufs = (_lib.TensorSurface * n)(), (_lib.Scale * n)(), []
    for i in range(n):
        sc[i] = _lib.Scale(*scales[i])
        ow, oh = scales[i][:2]
        row = ow * esz * (C if layout == "hwc" else 1)
        stride_y, off, pad_c = row, 0, 0
        if padded:
            stride_y = row + 2 * esz
            if esz == 2 and stride_y % 4 != 2:
                stride_y += 2
            off, pad_c = esz, 6 * esz
        stride_c = oh * stride_y + pad_c if layout == "chw" else 0
        size = off + (C * stride_c if layout == "chw" else oh * stride_y)
        buf = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        surf[i].data, surf[i].stride_c, surf[i].stride_y = buf.data_ptr() + off, stride_c, stride_y
        bufs.append((buf, off, stride_c, stride_y))
    imgs = (ctypes.c_void_p * n)(*[o.image._h.value for o in outs])
    aimgs = aplanes = None
    if alphas is not None:
        aimgs = (ctypes.c_void_p * n)(*[x.image._h.value if x is not None else None for x in alphas])
        aplanes = (_lib.Planes * n)()
        for i, x in enumerate(alphas):
            if x is not None:
                aplanes[i].plane[0] = x.y.data_ptr()
                aplanes[i].pitch[0] = x.y.stride(0) * x.y.element_size()
    fl = None if flips is None else (ctypes.c_uint32 * n)(*flips)
    rc = _lib.lib.heifgpu_render_batch_tensor(ctx._h, imgs, n, H.DecodeContext.planes_of(outs), aimgs, aplanes,
                                              ctypes.byref(fmt), sc, fl, surf,
                                              ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    if sync:
        torch.cuda.synchronize()
    return rc, bufs


def elements(entry, ow, oh, C, elem, layout):
    """The element bit patterns of a buffer tensor_raw filled, shaped like
    tensor_ref.tensor's result, and the bytes no element covers."""
    buf, off, stride_c, stride_y = entry
    b = buf.cpu().numpy()
    esz = ELEMS[elem][1]
    covered = np.zeros(b.shape, bool)
    covered[:off] = False
    dt = np.uint32 if esz == 4 else np.uint16
    if layout == "chw":
        out = np.empty((C, oh, ow), dt)
        for c in range(C):
            for y in range(oh):
                s = off + c * stride_c + y * stride_y
                out[c, y] = b[s:s + ow * esz].copy().view(dt)
                covered[s:s + ow * esz] = True
    else:
        out = np.empty((oh, ow, C), dt)
        for y in range(oh):
            s = off + y * stride_y
            out[y] = b[s:s + ow * C * esz].copy().view(dt).reshape(ow, C)
            covered[s:s + ow * C * esz] = True
    return out, b[~covered]


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


IMAGENET = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 255)
# 37 x 19: no integer ratio, partial tiles; 65 x 36: 2:1 of 130 x 72; None: the identity; 1 x 1
TARGETS = [(37, 19), (65, 36), None, (1, 1)]


@pytest.mark.parametrize("size", [dict(width=136, height=72, conf_right=6),   # 130 x 72: 3 x 2 tiles when swapped
                                  dict(width=264, height=24, conf_right=2)],  # 262 x 24: 2 tiles along x at identity
                         ids=["130x72", "262x24"])
def test_orientations_and_flips(H, S, ctx, decoded, size):
    """The eight orientations x the four flips in one call per target, f32 CHW."""
    from heif_amd import _lib

    p, o = decoded(3, **size)
    outs = [with_steps(H, S, o, p, steps) for steps in ORIENTATIONS]
    Ds = [displayed(o, steps, "rgb8") for steps in ORIENTATIONS]
    a, b = IMAGENET
    for target in TARGETS:
        scales = []
        for k, out in enumerate(outs):
            d = out.image.display
            tw, th = target or (d.out_width, d.out_height)
            if target and k in SWAPPED:
                tw, th = th, tw
            scales.append((tw, th, 0, 0, 0, 0))
        rc, bufs = tensor_raw(H, ctx, [out for out in outs for _ in range(4)], "rgb8", "f32", "chw",
                              [sc for sc in scales for _ in range(4)], a, b, flips=[0, 1, 2, 3] * 8)
        assert rc == 0
        # the integers of the GPU's own scaled render, through the same checker
        surf, scs, raws = (_lib.Surface * 8)(), (_lib.Scale * 8)(), []
        for i, sc in enumerate(scales):
            t = torch.empty((sc[1], sc[0], 3), dtype=torch.uint8, device="cuda:0")
            surf[i].pixels, surf[i].pitch, scs[i] = t.data_ptr(), sc[0] * 3, _lib.Scale(*sc)
            raws.append(t)
        imgs = (ctypes.c_void_p * 8)(*[x.image._h.value for x in outs])
        assert _lib.lib.heifgpu_render_batch_scaled(ctx._h, imgs, 8, H.DecodeContext.planes_of(outs), None, None, 0, scs,
                                                    surf, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)) == 0
        torch.cuda.synchronize()
        for k, (steps, D, sc) in enumerate(zip(ORIENTATIONS, Ds, scales)):
            R = want(D, sc)
            assert np.array_equal(host(raws[k]), R), (target, steps)
            got = [elements(bufs[4 * k + f], sc[0], sc[1], 3, "f32", "chw") for f in range(4)]
            for f in range(4):
                g, rest = got[f]
                assert rest.size == 0
                assert np.array_equal(g, tensor_ref.tensor(R, a, b, "f32", "chw", flip=f)), (target, steps, f)
                assert np.array_equal(g, tensor_ref.tensor(host(raws[k]), a, b, "f32", "chw", flip=f)), (target, steps, f)
            assert np.array_equal(got[1][0], got[0][0][:, :, ::-1]), (target, steps)  # flip 1: the last axis reversed


@pytest.fixture(scope="module")
def format_cases(H, S):
    """The pictures of test_formats, decoded once, and their integer pictures R per
    source format: an 8-bit and a 10-bit picture of 130 x 72, each with an alpha
    plane, shown as they are (axes kept) and turned (axes swapped)."""
    orients = [[], [("irot", 1)]]
    scales = {(37, 19): [(37, 19, 0, 0, 0, 0), (19, 37, 0, 0, 0, 0)], (65, 36): [(65, 36, 0, 0, 0, 0), (36, 65, 0, 0, 0, 0)]}
    pics = {}
    for depth, adepth, seed in ((8, 8, 70), (10, 12, 72)):
        p = S.SynthParams(width=136, height=72, conf_right=6, bit_depth=depth)
        ap = S.SynthParams(width=136, height=72, conf_right=6, chroma_format=0, bit_depth=adepth)
        f = S.display_heic(p, seed=seed, aux=(S.AuxImage(ap, seed=seed + 1, urn=S.ALPHA_URN_MPEGB),))
        o, al = H.HeicDecoder.decode(f), H.HeicDecoder.decode(f, item_id=2)
        assert o.image.display.alpha_item_id == 2 and al.info.bit_depth == adepth and o.info.bit_depth == depth
        pics[depth] = (p, o, al)
    cache = {}

    def get(src, target):
        key = (src, target)
        if key not in cache:
            p, o, al = pics[10 if src.endswith("16") else 8]
            rgba = src.startswith("rgba")
            outs = [with_steps(H, S, o, p, steps) for steps in orients]
            Rs = [want(displayed(o, steps, src, alpha=al if rgba else None), sc)
                  for steps, sc in zip(orients, scales[target])]
            if rgba:
                assert len(np.unique(Rs[0][..., 3])) > 4  # a real alpha plane, not a constant
            cache[key] = (outs, [al, al] if rgba else None, scales[target], Rs)
        return cache[key]

    return get


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("elem", list(ELEMS))
@pytest.mark.parametrize("src", SOURCES)
def test_formats(H, ctx, format_cases, src, elem, layout):
    """Element type x layout x source format, into padded buffers whose base is one
    element in: the pad bytes keep the sentinel, rows on and off a dword, odd and even widths."""
    C = 4 if src.startswith("rgba") else 3
    maxv = 1023 if src.endswith("16") else 255
    a, b = tensor_ref.constants(tensor_ref.IMAGENET_MEAN + (0.5,), tensor_ref.IMAGENET_STD + (0.25,), maxv)
    a, b = a[:C], b[:C]
    for target in ((37, 19), (65, 36)):
        outs, alphas, scales, Rs = format_cases(src, target)
        rc, bufs = tensor_raw(H, ctx, outs, src, elem, layout, scales, a, b, flips=[0, 1], alphas=alphas, padded=True)
        assert rc == 0
        for k, (sc, R) in enumerate(zip(scales, Rs)):
            stride_y, off = bufs[k][3], bufs[k][1]
            if elem != "f32":
                assert off == 2 and stride_y % 4 == 2  # rows alternate between off and on a dword
            g, rest = elements(bufs[k], sc[0], sc[1], C, elem, layout)
            assert np.array_equal(g, tensor_ref.tensor(R, a, b, elem, layout, flip=k)), (target, k)
            assert rest.size > 0 and (rest == SENTINEL).all(), (target, k)


def test_known_answers(H, S, ctx, decoded):
    """a = 1, b = 0 returns the levels in every element type; a = 2^-24 into f16
    returns them as subnormals, whose bit pattern is the level itself (a conversion
    that flushes would give zeros)."""
    p, o = decoded(3, width=136, height=72, conf_right=6)
    orients = [[], [("irot", 3), ("imir", 0)]]
    outs = [with_steps(H, S, o, p, steps) for steps in orients]
    scales = [(37, 19, 0, 0, 0, 0), (19, 37, 0, 0, 0, 0)]
    Rs = [want(displayed(o, steps, "rgb8"), sc) for steps, sc in zip(orients, scales)]
    assert all(R.max() > 128 and len(np.unique(R)) > 32 for R in Rs)
    one, zero = (1.0,) * 3, (0.0,) * 3
    for layout in LAYOUTS:
        for elem in ELEMS:
            rc, bufs = tensor_raw(H, ctx, outs, "rgb8", elem, layout, scales, one, zero)
            assert rc == 0
            for e, sc, R in zip(bufs, scales, Rs):
                g, _ = elements(e, sc[0], sc[1], 3, elem, layout)
                Rl = R.transpose(2, 0, 1) if layout == "chw" else R
                if elem == "f32":
                    back = g.view(np.float32)
                elif elem == "f16":
                    back = g.view(np.float16).astype(np.float32)
                else:
                    back = (g.astype(np.uint32) << 16).view(np.float32)
                assert np.array_equal(back, Rl.astype(np.float32)), (layout, elem)
        rc, bufs = tensor_raw(H, ctx, outs, "rgb8", "f16", layout, scales, (2.0 ** -24,) * 3, zero)
        assert rc == 0
        for e, sc, R in zip(bufs, scales, Rs):
            g, _ = elements(e, sc[0], sc[1], 3, "f16", layout)
            assert np.array_equal(g, (R.transpose(2, 0, 1) if layout == "chw" else R).astype(np.uint16)), layout


def test_mixed_batch_into_one_tensor(H, S, ctx):
    """One call into the slices of one (N, C, h, w) tensor: pictures that differ in
    size, orientation and chroma format, windows with an odd origin, mixed flips."""
    specs = [
        (S.SynthParams(width=136, height=72, conf_right=6), [("irot", 1)], (3, 7, 60, 111), 1),
        (S.SynthParams(width=72, height=40, conf_right=5, chroma_format=3), [("imir", 0)], (1, 3, 41, 29), 2),
        (S.SynthParams(width=48, height=32, chroma_format=0), [("clap", (27, 1, 22, 1, -5, 2, 3, 1)), ("irot", 2)],
         (5, 1, 20, 19), 3),
        (S.SynthParams(width=136, height=72, conf_right=6), [], (13, 5, 101, 67), 0),
    ]
    outs = [H.HeicDecoder.decode(S.display_heic(p, seed=30 + k, transforms=boxes(S, steps)))
            for k, (p, steps, _, _) in enumerate(specs)]
    assert [o.info.chroma_format_idc for o in outs] == [1, 3, 0, 1]
    got = ctx.render_tensor(outs, (16, 24), windows=[w for *_, w, _ in specs], flips=[f for *_, f in specs])
    assert tuple(got.shape) == (4, 3, 16, 24) and got.dtype == torch.float16 and got.is_contiguous()
    a, b = IMAGENET
    gb = bits(got)
    for k, ((p, steps, w, f), o) in enumerate(zip(specs, outs)):
        R = want(displayed(o, steps, "rgb8"), (24, 16) + w)
        assert np.array_equal(gb[k], tensor_ref.tensor(R, a, b, "f16", "chw", flip=f)), (steps, f)


def test_halfmoonbay_cover(H, ctx, halfmoonbay):
    """12 megapixels, irot 3 (the swapped path) to 224 x 224: f16 CHW and bf16 HWC."""
    o = H.HeicDecoder.decode(halfmoonbay)
    D = host(ctx.render([o], "rgb8")[0])
    assert D.shape == (4032, 3024, 3)
    R = want(D, scale_ref.fit(3024, 4032, 224, 224, "cover"))
    a, b = IMAGENET
    chw = ctx.render_tensor([o], (224, 224), flips=[1])
    assert tuple(chw.shape) == (1, 3, 224, 224) and chw.dtype == torch.float16
    assert np.array_equal(bits(chw)[0], tensor_ref.tensor(R, a, b, "f16", "chw", flip=1))
    hwc = ctx.render_tensor([o], (224, 224), dtype=torch.bfloat16, layout="hwc")
    assert tuple(hwc.shape) == (1, 224, 224, 3) and hwc.dtype == torch.bfloat16
    assert np.array_equal(bits(hwc)[0], tensor_ref.tensor(R, a, b, "bf16", "hwc"))


def test_back_to_back_calls_keep_their_descriptors(H, S, ctx, decoded):
    """Six calls issued without a host synchronise in between: the ring of four
    descriptor slots wraps, and every call still renders its own batch."""
    (p1, o1), (p2, o2) = decoded(3, width=136, height=72, conf_right=6), decoded(5, width=72, height=40, chroma_format=3)
    a, b = IMAGENET
    kinds = [("f16", "chw"), ("bf16", "hwc"), ("f32", "chw"), ("f16", "hwc"), ("f32", "hwc"), ("bf16", "chw")]
    calls = []
    for k in range(6):
        s1, s2 = ORIENTATIONS[k], ORIENTATIONS[7 - k]
        batch = [(o1, p1, s1, (37 - k, 19 + k, 0, 0, 0, 0), k & 3), (o2, p2, s2, (13 + k, 9, k, 1, 30, 33), (k + 1) & 3)]
        batch = batch[::1 if k % 2 else -1]
        calls.append(([with_steps(H, S, o, p, s) for o, p, s, *_ in batch], batch))
    torch.cuda.synchronize()
    results = []
    for (outs, batch), (elem, layout) in zip(calls, kinds):  # six launches queued, no synchronise between them
        results.append(tensor_raw(H, ctx, outs, "rgb8", elem, layout, [sc for *_, sc, _ in batch], a, b,
                                  flips=[f for *_, f in batch], sync=False))
    torch.cuda.synchronize()
    for (outs, batch), (rc, bufs), (elem, layout) in zip(calls, results, kinds):
        assert rc == 0
        for (o, p, steps, sc, f), e in zip(batch, bufs):
            g, _ = elements(e, sc[0], sc[1], 3, elem, layout)
            R = want(displayed(o, steps, "rgb8"), sc)
            assert np.array_equal(g, tensor_ref.tensor(R, a, b, elem, layout, flip=f)), (steps, sc, f, elem, layout)


def test_python_surface(H, S, ctx):
    files = [S.display_heic(S.SynthParams(width=136, height=72, conf_right=6), seed=60, transforms=boxes(S, [("irot", 1)])),
             S.display_heic(S.SynthParams(width=72, height=40, conf_right=5, chroma_format=3), seed=61)]
    outs = [H.HeicDecoder.decode(f) for f in files]
    Ds = [displayed(outs[0], [("irot", 1)], "rgb8"), displayed(outs[1], [], "rgb8")]
    dims = [(72, 130), (67, 40)]
    a, b = IMAGENET
    cover = ctx.render_tensor(outs, (16, 24))
    assert tuple(cover.shape) == (2, 3, 16, 24) and cover.dtype == torch.float16 and cover.is_contiguous()
    for g, D, (dw, dh) in zip(bits(cover), Ds, dims):
        assert np.array_equal(g, tensor_ref.tensor(want(D, scale_ref.fit(dw, dh, 24, 16, "cover")), a, b, "f16", "chw"))
    hwc = ctx.render_tensor(outs, (16, 24), mode="stretch", dtype=torch.float32, layout="hwc", flips=[2, 0])
    assert tuple(hwc.shape) == (2, 16, 24, 3) and hwc.dtype == torch.float32
    for g, D, f in zip(bits(hwc), Ds, (2, 0)):
        assert np.array_equal(g, tensor_ref.tensor(scale_ref.area_average(D, None, 24, 16), a, b, "f32", "hwc", flip=f))
    contain = ctx.render_tensor(outs, (16, 24), mode="contain", dtype=torch.bfloat16)
    assert isinstance(contain, list) and [tuple(g.shape) for g in contain] == [(3, 16, 9), (3, 14, 24)]
    for g, D, (dw, dh) in zip(contain, Ds, dims):
        assert g.dtype == torch.bfloat16
        assert np.array_equal(bits(g), tensor_ref.tensor(want(D, scale_ref.fit(dw, dh, 24, 16, "contain")), a, b, "bf16", "chw"))
    windows = [(3, 7, 60, 111), (1, 2, 41, 29)]
    mean4, std4 = tensor_ref.IMAGENET_MEAN + (0.0,), tensor_ref.IMAGENET_STD + (1.0,)
    win = ctx.render_tensor(outs, (16, 24), windows=windows, src="rgba8", mean=mean4, std=std4, dtype=torch.float32)
    assert tuple(win.shape) == (2, 4, 16, 24)
    a4, b4 = tensor_ref.constants(mean4, std4, 255)
    for g, o, st, w in zip(bits(win), outs, ([("irot", 1)], []), windows):
        assert np.array_equal(g, tensor_ref.tensor(want(displayed(o, st, "rgba8"), (24, 16) + w), a4, b4, "f32", "chw"))
    # scale_bias passes the constants as they are
    raw = ctx.render_tensor(outs, (16, 24), scale_bias=((1, 1, 1), (0, 0, 0)), dtype=torch.float32)
    assert torch.equal(raw, ctx.render_scaled(outs, (16, 24)).permute(0, 3, 1, 2).float())
    # decode_tensor: cover unless told otherwise
    one = H.HeicDecoder.decode_tensor(files[1], (16, 24))
    assert tuple(one.shape) == (3, 16, 24) and torch.equal(one, cover[1])
    flipped = H.HeicDecoder.decode_tensor(files[1], (16, 24), flip=1, layout="hwc")
    assert tuple(flipped.shape) == (16, 24, 3) and torch.equal(flipped, cover[1].permute(1, 2, 0).flip(1))
    for bad in (dict(mode="fill"), dict(layout="nchw"), dict(dtype=torch.float64), dict(flips=[0, 4]), dict(flips=[0]),
                dict(mean=(0.5,) * 4), dict(src="rgba8"), dict(scale_bias=((1, 1), (0, 0, 0)))):
        with pytest.raises(ValueError):
            ctx.render_tensor(outs, (16, 24), **bad)
    with pytest.raises(H.HeifGpuError):
        ctx.render_tensor(outs, (16, 24), windows=[(0, 0, 73, 1), (0, 0, 1, 1)])
    with pytest.raises(H.HeifGpuError):
        ctx.render_tensor(outs, (16, 24), scale_bias=((1, float("inf"), 1), (0, 0, 0)))


def test_mixed_bit_depths_need_explicit_constants(H, S, ctx):
    """A 16-bit source takes every picture at its own depth, so mean / std give no
    common scale for a 10-bit and a 12-bit picture: ValueError; scale_bias is accepted."""
    outs = [H.HeicDecoder.decode(S.display_heic(S.SynthParams(width=64, height=48, bit_depth=d), seed=80 + d))
            for d in (10, 12)]
    with pytest.raises(ValueError):
        ctx.render_tensor(outs, (11, 17), src="rgb16")
    a = (1.0 / 4095,) * 3
    got = ctx.render_tensor(outs, (11, 17), src="rgb16", scale_bias=(a, (0, 0, 0)), dtype=torch.float32)
    ints = host(ctx.render_scaled(outs, (11, 17), fmt="rgb16"))
    for g, R in zip(bits(got), ints):
        assert np.array_equal(g, tensor_ref.tensor(R, np.float32(a), (0, 0, 0), "f32", "chw"))
    # one depth throughout: mean / std at that depth
    same = ctx.render_tensor(outs[:1], (11, 17), src="rgb16", dtype=torch.float32)
    a10, b10 = tensor_ref.constants(tensor_ref.IMAGENET_MEAN, tensor_ref.IMAGENET_STD, 1023)
    assert np.array_equal(bits(same)[0], tensor_ref.tensor(ints[0], a10, b10, "f32", "chw"))
