"""The filtered renders without a device: the numpy restatement of Pillow's
antialiased BILINEAR / BICUBIC (resample_ref) against Pillow itself (live where
PIL imports, always against the recorded tests/golden/pillow_resize.npz), and
the library's host hooks, which run the arithmetic the kernel runs
(kernels/resample.hpp), against the restatement.  Every comparison is exact."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import display_ref
import resample_ref as R
from conftest import GOLDEN, ROOT, make_emu

CODES = R.CODES


@pytest.fixture(scope="module")
def L():
    from heif_amd import _lib

    return _lib


def blocks(h, w, c, maxv, seed):
    """0 / maxv blocks of a few samples with some noise between: overshoot on every edge, so
    both clips of both passes fire."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    D = np.empty((h, w, c), np.uint16 if maxv > 255 else np.uint8)
    for k in range(c):
        D[..., k] = ((((yy // (2 + k)) + (xx // (3 + k))) & 1) * maxv)
    noise = rng.integers(0, maxv + 1, (h, w, c))
    mask = rng.random((h, w, 1)) < 0.1
    return np.where(mask, noise, D).astype(D.dtype)


# ---- the restatement against Pillow ---------------------------------------------
def test_restatement_equals_recorded_pillow():
    z = np.load(GOLDEN / "pillow_resize.npz")
    cases, outs = z["cases"], z["outs"]
    assert len(cases) >= 20 and (GOLDEN / "pillow_resize.npz").stat().st_size < 16384
    seen, at = set(), 0
    for k, case in enumerate(cases):
        x, y, w, h, ow, oh, code, p = (int(v) for v in case)
        D = z[f"pic_{p}"]
        name = {1: "bilinear", 2: "bicubic"}[code]
        want = outs[at:at + oh * ow * D.shape[2]].reshape(oh, ow, D.shape[2])
        at += want.size
        got = R.resize(D, (x, y, w, h), ow, oh, name)
        assert np.array_equal(got, want), (k, name, (x, y, w, h), (ow, oh))
        seen.add((name, (ow > w) - (ow < w)))
    assert at == outs.size
    assert {n for n, _ in seen} == set(R.FILTERS) and {s for _, s in seen} == {-1, 0, 1}  # reduce, identity, enlarge


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    pf = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
    D = blocks(29, 41, 3, 255, 5)
    for win in ((0, 0, 41, 29), (5, 3, 30, 20), (40, 28, 1, 1), (0, 0, 41, 7)):
        for ow, oh in ((17, 11), (64, 48), (1, 1), (win[2], win[3]), (41, 29)):
            for name in R.FILTERS:
                box = (win[0], win[1], win[0] + win[2], win[1] + win[3])
                want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(D[..., c])).resize((ow, oh), pf[name], box=box))
                                 for c in range(3)], axis=-1)
                assert np.array_equal(R.resize(D, win, ow, oh, name), want), (win, ow, oh, name)


def test_intermediate_rounding_and_order_matter():
    """The issue's example: 41 x 29 -> 17 x 11 of hard 0 / 255 samples.  Without the clip
    between the passes, or with the passes in the other order, the answer differs, so
    neither can be dropped unnoticed."""
    D = blocks(29, 41, 3, 255, 7)
    right = R.resize(D, None, 17, 11, "bicubic")
    assert (right != R.resize(D, None, 17, 11, "bicubic", clip_mid=False)).any()
    assert (right != R.resize(D, None, 17, 11, "bicubic", vertical_first=True)).any()


# ---- heifgpu_resample_coeffs ----------------------------------------------------
def lib_coeffs(L, in_size, in0, in1, out, name, bits):
    ks = ctypes.c_uint32()
    assert L.lib.heifgpu_resample_coeffs(in_size, in0, in1, out, CODES[name], bits, None, None, 0, ctypes.byref(ks)) == 0
    bounds = (ctypes.c_int32 * (2 * out))()
    kk = (ctypes.c_int32 * (out * ks.value))()
    rc = L.lib.heifgpu_resample_coeffs(in_size, in0, in1, out, CODES[name], bits, bounds, kk, out * ks.value, ctypes.byref(ks))
    assert rc == 0, L.last_error()
    return ks.value, np.array(bounds).reshape(out, 2), np.array(kk).reshape(out, ks.value)


# the side pairs of test_scale.py's test_checker_weights_sum, whole, then windows at offsets
AXES = [(c, 0, c, o) for c, o in [(41, 17), (29, 11), (13, 64), (130, 65), (130, 130), (72, 1), (1, 5), (3024, 224)]] + \
       [(41, 5, 35, 17), (41, 40, 41, 3), (130, 1, 14, 64), (4032, 504, 3528, 224), (72, 0, 7, 7), (72, 65, 72, 2)]


@pytest.mark.parametrize("bits", (8, 10, 12))
@pytest.mark.parametrize("name", R.FILTERS)
def test_coeffs_equal_restatement(L, name, bits):
    for in_size, in0, in1, out in AXES:
        ks, bounds, kk = lib_coeffs(L, in_size, in0, in1, out, name, bits)
        assert ks == R.ksize(in0, in1, out, name)
        want = R.coeffs(in_size, in0, in1, out, name, R.precision(bits))
        for X, (xmin, k) in enumerate(want):
            assert tuple(bounds[X]) == (xmin, len(k)), (in_size, in0, in1, out, X)
            assert list(kk[X, :len(k)]) == k and not kk[X, len(k):].any(), (in_size, in0, in1, out, X)


def test_coeffs_argument_checks(L):
    ks = ctypes.c_uint32()
    f = L.lib.heifgpu_resample_coeffs
    INV = L.HEIFGPU_E_INVALID
    assert f(41, 0, 41, 17, 2, 8, None, None, 0, ctypes.byref(ks)) == 0 and ks.value == 2 * 5 + 1
    assert f(41, 0, 41, 17, 2, 8, None, None, 0, None) == INV
    for bad in ((0, 0, 0, 1), (41, 0, 42, 17), (41, 5, 5, 17), (41, 0, 41, 0), (65536, 0, 1, 1), (41, 0, 41, 65536)):
        assert f(*bad, 2, 8, None, None, 0, ctypes.byref(ks)) == INV, bad
    assert f(41, 0, 41, 17, 0, 8, None, None, 0, ctypes.byref(ks)) == INV  # area has no coefficients of this kind
    assert f(41, 0, 41, 17, 3, 8, None, None, 0, ctypes.byref(ks)) == INV
    assert f(41, 0, 41, 17, 2, 7, None, None, 0, ctypes.byref(ks)) == INV
    assert f(41, 0, 41, 17, 2, 13, None, None, 0, ctypes.byref(ks)) == INV
    kk = (ctypes.c_int32 * (17 * 11))()
    assert f(41, 0, 41, 17, 2, 8, None, kk, 17 * 11 - 1, ctypes.byref(ks)) == INV and "kk" in L.last_error()
    assert f(41, 0, 41, 17, 2, 8, None, kk, 17 * 11, ctypes.byref(ks)) == 0


# ---- heifgpu_resample_apply -----------------------------------------------------
def lib_apply(L, D, window, ow, oh, name, bits):
    D = np.ascontiguousarray(D)
    out = np.zeros((oh, ow, D.shape[2]), D.dtype)
    w = None if window is None else ctypes.byref(L.Rect(*window))
    rc = L.lib.heifgpu_resample_apply(D.ctypes.data_as(ctypes.c_void_p), D.shape[1], D.shape[0], D.shape[2], bits, w,
                                      ow, oh, CODES[name], out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, L.last_error()
    return out


@pytest.mark.parametrize("bits, ch", [(8, 3), (8, 4), (10, 3), (12, 4), (8, 1)])
@pytest.mark.parametrize("name", R.FILTERS)
def test_apply_equals_restatement(L, name, bits, ch):
    maxv = (1 << bits) - 1
    D = blocks(29, 41, ch, maxv, bits + ch)
    for window, (ow, oh) in [(None, (17, 11)), (None, (64, 48)), (None, (41, 29)), ((5, 3, 30, 20), (7, 20)),
                             ((36, 25, 5, 4), (17, 11)), (None, (1, 1)), ((0, 0, 1, 1), (3, 2))]:
        got = lib_apply(L, D, window, ow, oh, name, bits)
        want = R.resize(D, window, ow, oh, name, bits)
        assert np.array_equal(got, want), (window, ow, oh)
        if window is None and (ow, oh) == (41, 29):
            assert np.array_equal(got, D)  # identity
    # the case cannot go soft: on this picture the clip between the passes decides samples
    if name == "bicubic":
        assert (R.resize(D, None, 17, 11, name, bits) != R.resize(D, None, 17, 11, name, bits, clip_mid=False)).any()
        up = R.resize(D, None, 64, 48, name, bits)  # the enlargement overshoots the hard edges: both ends clip
        assert up.max() == maxv and up.min() == 0 and (up != R.resize(D, None, 64, 48, name, bits, clip_mid=False)).any()


def test_apply_argument_checks(L):
    D = np.zeros((4, 5, 3), np.uint8)
    out = np.zeros((2, 2, 3), np.uint8)
    f = L.lib.heifgpu_resample_apply
    p, q = D.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    INV = L.HEIFGPU_E_INVALID
    assert f(p, 5, 4, 3, 8, None, 2, 2, 1, q) == 0
    assert f(None, 5, 4, 3, 8, None, 2, 2, 1, q) == INV and f(p, 5, 4, 3, 8, None, 2, 2, 1, None) == INV
    assert f(p, 5, 4, 0, 8, None, 2, 2, 1, q) == INV and f(p, 5, 4, 5, 8, None, 2, 2, 1, q) == INV
    assert f(p, 5, 4, 3, 8, None, 2, 2, 0, q) == INV and f(p, 5, 4, 3, 8, None, 2, 2, 3, q) == INV
    assert f(p, 5, 4, 3, 8, None, 0, 2, 1, q) == INV and f(p, 5, 4, 3, 8, None, 2, 65536, 1, q) == INV
    assert f(p, 5, 4, 3, 8, ctypes.byref(L.Rect(4, 0, 2, 2)), 2, 2, 1, q) == INV
    assert f(p, 5, 4, 3, 8, ctypes.byref(L.Rect(0, 0, 5, 0)), 2, 2, 1, q) == INV
    wide = np.full((4, 5, 3), 1024, np.uint16)
    assert f(wide.ctypes.data_as(ctypes.c_void_p), 5, 4, 3, 10, None, 2, 2, 1, q) == INV and "maxv" in L.last_error()


# ---- heifgpu_window_source_rect_resampled ---------------------------------------
ORIENTATIONS = [[("irot", k)] + m for k in range(4) for m in ([], [("imir", 0)])]
W, H = 64, 48


def restated_rect(steps, window, chroma):
    """The source coordinates of the displayed picture's pixels as arrays; min / max over
    the window; grown to the chroma grid, clipped (tests/test_window_decode.py's)."""
    ys, xs = np.mgrid[0:H, 0:W]
    tx, ty = display_ref.apply_transforms(xs, steps), display_ref.apply_transforms(ys, steps)
    x, y, w, h = window
    sx, sy = tx[y:y + h, x:x + w], ty[y:y + h, x:x + w]
    mx = 1 if chroma in (1, 2) else 0
    my = 1 if chroma == 1 else 0
    x0, y0 = int(sx.min()) & ~mx, int(sy.min()) & ~my
    x1, y1 = min(int(sx.max()) | mx, W - 1), min(int(sy.max()) | my, H - 1)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


@pytest.mark.parametrize("chroma", (0, 1, 2, 3))
def test_source_rect_resampled_against_restatement(L, chroma):
    import heif_amd as Hm
    from heif_amd import synth_encoder as S

    make = {"irot": S.irot_box, "imir": S.imir_box}
    widened = 0
    for steps in ORIENTATIONS:
        img = Hm.HeifImage.parse(S.display_heic(S.SynthParams(width=W, height=H, chroma_format=chroma),
                                                transforms=tuple(make[k](a) for k, a in steps)))
        d = img.display
        dw, dh = d.out_width, d.out_height
        for window, size in [((7, 9, 21, 15), (5, 7)), ((7, 9, 21, 15), (15, 21)), ((7, 9, 21, 15), (40, 50)),
                             (None, (11, 13)), ((0, 0, 3, 3), (2, 2)), ((dw - 3, dh - 3, 3, 3), (1, 1))]:
            plain = img.source_rect(window)
            assert img.source_rect(window, size, "area") == plain
            for name in R.FILTERS:
                halo = R.halo_window(dw, dh, window, size[1], size[0], name)
                assert halo[0] >= 0 and halo[1] >= 0 and halo[0] + halo[2] <= dw and halo[1] + halo[3] <= dh
                got = img.source_rect(window, size, name)
                assert got == restated_rect(steps, halo, chroma), (steps, window, size, name)
                widened += got != plain
    assert widened > 20  # the halo shows
    with pytest.raises(ValueError):
        img.source_rect((7, 9, 21, 15), None, "bicubic")  # a filtered rectangle needs the rendered size
    with pytest.raises(ValueError):
        img.source_rect((7, 9, 21, 15), (5, 7), "lanczos")
    with pytest.raises(ValueError):
        img.source_rect((60, 9, 21, 15), (5, 7), "bicubic")


# ---- the C-ABI boundary -----------------------------------------------------------
NEW = ("heifgpu_render_batch_resampled", "heifgpu_render_batch_tensor_resampled", "heifgpu_resample_coeffs",
       "heifgpu_resample_apply", "heifgpu_window_source_rect_resampled")


def test_new_names_are_exported(L):
    header = (ROOT / "include" / "heifgpu.h").read_text()
    syms = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in L.EXPORTS and hasattr(L.lib, name) and name in exported, name
    assert L.ABI_VERSION == 6 and L.lib.heifgpu_abi_version() == 6  # new entry points only
    assert (L.FILTER_AREA, L.FILTER_BILINEAR, L.FILTER_BICUBIC) == (0, 1, 2)
    for k, v in (("AREA", 0), ("BILINEAR", 1), ("BICUBIC", 2)):
        assert re.search(rf"HEIFGPU_FILTER_{k}\s*=\s*{v}\b", header)


def test_render_resampled_argument_checks_need_no_device(L):
    """Every check of the arguments answers before the context is looked at: with a null
    context a call with good arguments fails on the context, a call with a bad one on
    that argument (the surfaces and planes are never touched)."""
    import heif_amd as Hm
    from heif_amd import synth_encoder as S

    lib = L.lib
    INV = L.HEIFGPU_E_INVALID
    assert lib.heifgpu_render_batch_resampled(None, None, 0, None, None, None, 0, None, 2, None, None, None) == INV
    img = Hm.HeifImage.parse(S.display_heic(S.SynthParams(width=64, height=48), transforms=(S.irot_box(1),)))
    imgs = (ctypes.c_void_p * 1)(img._h.value)
    planes = (L.Planes * 1)()
    for c in range(3):
        planes[0].plane[c], planes[0].pitch[c] = 0x1000 * (c + 1), 64  # never read: no launch happens
    surf = (L.Surface * 1)()
    surf[0].pixels = 0x10000

    def call(scale, pitch, fmt=0, filt=2):
        surf[0].pitch = pitch
        sc = (L.Scale * 1)(L.Scale(*scale))
        rc = lib.heifgpu_render_batch_resampled(None, imgs, 1, planes, None, None, fmt, sc, filt, None, surf, None)
        return rc, L.last_error()

    for filt in (0, 1, 2):  # area forwards to the scaled call and answers as it does
        rc, msg = call((17, 11, 0, 0, 0, 0), 51, filt=filt)
        assert rc == INV and "context" in msg, (filt, msg)
    rc, msg = call((17, 11, 5, 3, 41, 29), 51)
    assert rc == INV and "context" in msg
    rc, msg = call((65535, 65535, 0, 0, 0, 0), 65535 * 3)
    assert rc == INV and "context" in msg  # the largest legal size
    for filt in (3, 7, 0xFFFFFFFF):
        rc, msg = call((17, 11, 0, 0, 0, 0), 51, filt=filt)
        assert rc == INV and "filter" in msg, (filt, msg)
    for bad in ((17, 11, 0, 0, 41, 0), (17, 11, 8, 0, 41, 29), (17, 11, 48, 0, 1, 1), (17, 11, 0, 0, 49, 64)):
        rc, msg = call(bad, 51)
        assert rc == INV and "window" in msg, (bad, msg)
    for bad in ((0, 11, 0, 0, 0, 0), (17, 65536, 0, 0, 0, 0)):
        rc, msg = call(bad, 1 << 20)
        assert rc == INV and "rendered size" in msg, (bad, msg)
    rc, msg = call((17, 11, 0, 0, 0, 0), 50)
    assert rc == INV and "pitch" in msg
    rc, msg = call((17, 11, 0, 0, 0, 0), 51, fmt=4)
    assert rc == INV and "format" in msg

    # the tensor call
    tf = L.TensorFormat(src=0, elem=0, layout=0)
    for c in range(3):
        tf.a[c], tf.b[c] = 1.0, 0.0
    ts = (L.TensorSurface * 1)()
    ts[0].data, ts[0].stride_c, ts[0].stride_y = 0x10000, 17 * 11 * 4, 17 * 4
    sc = (L.Scale * 1)(L.Scale(17, 11, 0, 0, 0, 0))

    def tcall(filt=2, flip=0):
        fl = (ctypes.c_uint32 * 1)(flip)
        rc = lib.heifgpu_render_batch_tensor_resampled(None, imgs, 1, planes, None, None, ctypes.byref(tf), sc, filt, fl,
                                                       None, ts, None)
        return rc, L.last_error()

    for filt in (0, 1, 2):
        rc, msg = tcall(filt)
        assert rc == INV and "context" in msg, (filt, msg)
    rc, msg = tcall(3)
    assert rc == INV and "filter" in msg
    rc, msg = tcall(2, flip=4)
    assert rc == INV and "flip" in msg
    ts[0].stride_y = 17 * 4 - 4
    rc, msg = tcall(1)
    assert rc == INV and "stride_y" in msg


def test_python_rejects_unknown_filter():
    import heif_amd as Hm

    with pytest.raises(ValueError):
        Hm._filter_code("lanczos")
    assert [Hm._filter_code(n) for n in ("area", "bilinear", "bicubic")] == [0, 1, 2]


# ---- the host hooks under ASan + UBSan, as a program of their own -----------------
def test_resample_driver_clean():
    """tests/resample/resample_driver.cpp (make resample-asan): the coefficient rows and
    both passes over degenerate sizes (1 -> 1, 1 -> 65535, 65535 -> 1, windows touching
    each edge) into buffers of exactly the promised size.  Nothing is loaded into
    Python under a sanitizer."""
    make_emu("resample-asan")
    exe = pathlib.Path(ROOT) / "heif_amd" / "csrc" / "build" / "resample_asan" / "resample_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and sum(ln.startswith("axis") for ln in lines) == 60
    assert sum(ln.startswith("apply") for ln in lines) == 20
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
