"""k_ycbcr_rgb and k_gather_tiles alone on the device: heifgpu_ycbcr_to_rgb and
heifgpu_gather_tiles called through the C ABI on fabricated planes (rgb_gather_cases.py),
against rgb_ref.py and gather_ref.py.  Every buffer is a torch uint8 tensor of sentinel
guard band, payload, sentinel guard band, and the pointer handed over lies GUARD (+ a
base offset) bytes inside it; the whole tensor is compared, so a store outside the rows
it owes shows as a changed guard or padding byte.  Both operations are exact."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import rgb_gather_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import heif_amd
    from heif_amd import _lib

    ctx = heif_amd.DecodeContext(0)
    yield SimpleNamespace(L=_lib, lib=_lib.lib, h=ctx._h, stream=ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    torch.cuda.synchronize()
    ctx.close()


def upload(buf):
    t = torch.from_numpy(np.array(buf, dtype=np.uint8)).to("cuda:0")
    assert t.data_ptr() % 16 == 0  # what rgb_rows() and gather_chunks() count from
    return t


def same(t, want) -> bool:
    return np.array_equal(t.cpu().numpy(), want)


def image_info(L, **fields):
    info = L.ImageInfo(grid_rows=1, grid_cols=1, num_tiles=1)
    for k, v in fields.items():
        setattr(info, k, int(v))
    return info


def planes_of(L, tensors, pitches, offset=0):
    p = L.Planes()
    for k, t in enumerate(tensors):
        p.plane[k] = t.data_ptr() + C.GUARD + offset
        p.pitch[k] = pitches[k]
    return p


# ---- heifgpu_ycbcr_to_rgb ----------------------------------------------------------------------
def rgb_info(L, c, **over):
    f = dict(width=c.w, height=c.h, chroma_format_idc=c.chroma, bit_depth=c.depth, bytes_per_sample=C.rgb_bps(c),
             tile_width=c.w, tile_height=c.h, rotation=c.rot, matrix_coeffs=c.matrix, full_range=c.full)
    f.update(over)
    return image_info(L, **f)


def rgb_call(env, c, info=None, planes=None, pitch=None, null_rgb=False):
    """One call on fresh buffers: (return code, output tensor, source tensors)."""
    n = 3 if c.chroma else 1
    src = [upload(C.rgb_source(c, k)) for k in range(n)]
    out = upload(C.rgb_blank(c))
    p = planes_of(env.L, src, [C.rgb_src_pitch(c, k) for k in range(n)])
    if planes is not None:
        planes(p)
    rgb = None if null_rgb else ctypes.c_void_p(out.data_ptr() + C.GUARD + c.off)
    rc = env.lib.heifgpu_ycbcr_to_rgb(env.h, ctypes.byref(info if info is not None else rgb_info(env.L, c)),
                                      ctypes.byref(p), rgb, C.rgb_pitch(c) if pitch is None else pitch, env.stream)
    return rc, out, src


def run_rgb(env, cases):
    """Every case launched, one synchronisation, every buffer compared whole: the names that differ."""
    assert cases
    runs = [(c, rgb_call(env, c)) for c in cases]
    torch.cuda.synchronize()
    bad = []
    for c, (rc, out, src) in runs:
        if rc != env.L.HEIFGPU_OK:
            bad.append((c.name, "rc", rc))
        elif not same(out, C.rgb_expected(c)):
            bad.append((c.name, "rgb"))
        elif not all(same(t, C.rgb_source(c, k)) for k, t in enumerate(src)):
            bad.append((c.name, "source written"))
    return bad


def crossed(c) -> bool:
    """The depth x matrix x range x chroma cross at 37 x 22 turned once (its own test below)."""
    return (c.w, c.h, c.rot) == (37, 22, 1)


@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb_shapes(env, shape, rot):
    """Every chroma format at 8 and 10 bits, tight and padded rgb_pitch, base offsets 0..3."""
    bad = run_rgb(env, [c for c in C.RGB_CASES if (c.w, c.h) == shape and c.rot == rot and c.depth in (8, 10)])
    assert not bad, bad


@pytest.mark.parametrize("depth", C.DEPTHS)
def test_rgb_depths_matrices_ranges(env, depth):
    cases = [c for c in C.RGB_CASES if crossed(c) and c.depth == depth]
    assert len(cases) >= 24
    bad = run_rgb(env, cases)
    assert not bad, bad


def refused(env, rc, out, c):
    torch.cuda.synchronize()
    return rc == env.L.HEIFGPU_E_INVALID and same(out, C.rgb_blank(c))


def test_rgb_refusals(env):
    L = env.L
    tall = C.rgb_case(6, 20, 1, 1, 8, 1, True, 0, 0, 0)  # turned: 20 wide, so 60 bytes a row
    assert C.rgb_out_dims(tall) == (20, 6)
    for c, pitch in ((tall, 59), (tall, 18), (C.rgb_case(37, 22, 0, 3, 10, 9, False, 0, 1, 1), 110),
                     (C.rgb_case(8, 8, 2, 0, 8, 6, True, 0, 0, 0), 0), (C.rgb_case(8, 8, 3, 2, 8, 6, True, 0, 0, 0), -24)):
        rc, out, _ = rgb_call(env, c, pitch=pitch)
        assert refused(env, rc, out, c), (c.name, pitch)
    rc, out, _ = rgb_call(env, tall)  # and 60 is enough
    torch.cuda.synchronize()
    assert rc == L.HEIFGPU_OK and same(out, C.rgb_expected(tall))

    c = C.rgb_case(37, 22, 1, 1, 8, 1, False, 5, 2, 1)

    def drop(k):
        def f(p):
            p.plane[k] = None
        return f

    for k in (0, 1, 2):
        rc, out, _ = rgb_call(env, c, planes=drop(k))
        assert refused(env, rc, out, c), k
    rc, out, _ = rgb_call(env, c, info=rgb_info(L, c, chroma_format_idc=4))
    assert refused(env, rc, out, c)
    for depth, bps in ((7, 1), (17, 2), (0, 1)):
        rc, out, _ = rgb_call(env, c, info=rgb_info(L, c, bit_depth=depth, bytes_per_sample=bps))
        assert refused(env, rc, out, c), depth
    rc, out, _ = rgb_call(env, c, null_rgb=True)
    assert refused(env, rc, out, c)
    mono = C.rgb_case(8, 8, 0, 0, 8, 1, False, 0, 0, 0)  # 4:0:0 needs no chroma plane
    rc, out, _ = rgb_call(env, mono)
    torch.cuda.synchronize()
    assert rc == L.HEIFGPU_OK and same(out, C.rgb_expected(mono))


# ---- heifgpu_gather_tiles ----------------------------------------------------------------------
def gather_call(env, c, src, stride, offset, info=None, edit=None):
    """One call into sentinel-filled destinations: (return code, destination tensors)."""
    n = C.gather_planes(c)
    dst = [upload(C.gather_blank(c, k)) for k in range(n)]
    d, s = planes_of(env.L, dst, c.dpitch, c.doff), planes_of(env.L, src, c.spitch)
    if edit is not None:
        edit(d, s)
    if info is None:
        info = image_info(env.L, **vars(C.gather_info(c)))
    rc = env.lib.heifgpu_gather_tiles(ctypes.byref(info), ctypes.byref(d), ctypes.byref(s), stride, offset, env.stream)
    return rc, dst


@pytest.mark.parametrize("c", C.GATHER_CASES, ids=lambda c: c.name)
def test_gather(env, c):
    held = C.gather_sources(c)
    src = [upload(b) for b in held]
    assert C.gather_info(c).num_tiles == c.cols * c.rows
    bad = []
    for stride, offset in c.pairs:
        rc, dst = gather_call(env, c, src, stride, offset)
        torch.cuda.synchronize()
        if rc != env.L.HEIFGPU_OK:
            bad.append((stride, offset, "rc", rc))
            continue
        for k, (t, want) in enumerate(zip(dst, C.gather_expected(c, stride, offset))):
            if not same(t, want):
                bad.append((stride, offset, "plane", k))
    assert not bad, bad
    assert all(same(t, b) for t, b in zip(src, held))


def test_gather_refusals(env):
    L = env.L
    c = next(c for c in C.GATHER_CASES if c.name == "grid420_8")
    src = [upload(b) for b in C.gather_sources(c)]

    def refused(rc, dst):
        torch.cuda.synchronize()
        return rc == L.HEIFGPU_E_INVALID and all(same(t, C.gather_blank(c, k)) for k, t in enumerate(dst))

    for stride, offset in ((1, 1), (2, 2), (2, 7), (0, 1), (9, 9)):
        assert refused(*gather_call(env, c, src, stride, offset)), (stride, offset)
    info = image_info(L, **{**vars(C.gather_info(c)), "chroma_format_idc": 4})
    assert refused(*gather_call(env, c, src, 1, 0, info=info))

    def drop(which, k):
        def f(d, s):
            (d, s)[which].plane[k] = None
        return f

    for which in (0, 1):
        for k in (0, 1, 2):
            assert refused(*gather_call(env, c, src, 1, 0, edit=drop(which, k))), (which, k)
