"""The checker of the filtered renders (test infrastructure): include/heifgpu.h's
statement of Pillow's antialiased BILINEAR / BICUBIC resize, restated in plain
Python floats (IEEE binary64, every operation rounded on its own) and numpy
integers.  It shares no code with the library.

Unlike the other checkers this one is pinned from outside: for 8-bit samples it
equals PIL.Image.resize(size, filter, box=) bit for bit, checked live where PIL
imports and always against tests/golden/pillow_resize.npz, which holds Pillow's
own outputs (tools/make_resample_golden.py wrote it).  Above 8 bits Pillow has
no such mode and the rule at P = 32 - 2 - B is pinned to this file only.
"""
import numpy as np

FILTERS = ("bilinear", "bicubic")
CODES = {"area": 0, "bilinear": 1, "bicubic": 2}


def bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


F = {"bilinear": (bilinear, 1.0), "bicubic": (bicubic, 2.0)}


def precision(bits):
    return 32 - 2 - max(8, bits)


def ksize(in0, in1, out_size, name):
    """Pillow's row length: (int)ceil(support) * 2 + 1."""
    fs = max((in1 - in0) / out_size, 1.0)
    return int(np.ceil(F[name][1] * fs)) * 2 + 1


def coeffs(in_size, in0, in1, out_size, name, prec):
    """[(xmin, [k...])] for every output of one axis."""
    f, sup = F[name]
    scale = fs = (in1 - in0) / out_size
    if fs < 1.0:
        fs = 1.0
    support = sup * fs
    ss = 1.0 / fs
    out = []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        k = [f((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        ki = [int(-0.5 + w * (1 << prec)) if w < 0 else int(0.5 + w * (1 << prec)) for w in k]
        out.append((xmin, ki))
    return out


def _pass(src, rows, prec, mx, clip=True):
    """One pass along axis 0 of src (n, ...): out[X] = clip((half + sum k * src[xmin + t]) >> prec)."""
    out = np.empty((len(rows),) + src.shape[1:], np.int64)
    for X, (xmin, k) in enumerate(rows):
        kv = np.asarray(k, np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        acc = (1 << (prec - 1)) + (kv * src[xmin:xmin + len(k)]).sum(axis=0)
        assert np.abs(acc).max(initial=0) < 1 << 31  # the library's sums are int32
        out[X] = np.clip(acc >> prec, 0, mx) if clip else acc >> prec
    return out


def resize(D, window, ow, oh, name, bits=8, clip_mid=True, vertical_first=False):
    """D (H, W, C) through both passes: along x into the rounded, clipped intermediate,
    then along y.  window = (x, y, w, h) or None for the whole of D.  clip_mid=False and
    vertical_first=True are the wrong answers the tests tell the right one from."""
    prec, mx = precision(bits), (1 << bits) - 1
    H, W, _ = D.shape
    cx, cy, cw, ch = window if window is not None else (0, 0, W, H)
    kx = coeffs(W, cx, cx + cw, ow, name, prec)
    ky = coeffs(H, cy, cy + ch, oh, name, prec)
    src = D.astype(np.int64)
    if vertical_first:
        mid = _pass(src, ky, prec, mx)                                    # (oh, W, C)
        return _pass(mid.transpose(1, 0, 2), kx, prec, mx).transpose(1, 0, 2).astype(D.dtype)
    mid = _pass(src.transpose(1, 0, 2), kx, prec, mx, clip_mid)           # (ow, H, C)
    return _pass(mid.transpose(1, 0, 2), ky, prec, mx).astype(D.dtype)    # (oh, ow, C)


def halo_window(dw, dh, window, ow, oh, name):
    """The window widened by the taps' halo, in D: per axis [xmin(0), xmax(out - 1))."""
    cx, cy, cw, ch = window if window is not None else (0, 0, dw, dh)
    kx = coeffs(dw, cx, cx + cw, ow, name, 22)
    ky = coeffs(dh, cy, cy + ch, oh, name, 22)
    x0, x1 = kx[0][0], kx[-1][0] + len(kx[-1][1])
    y0, y1 = ky[0][0], ky[-1][0] + len(ky[-1][1])
    return x0, y0, x1 - x0, y1 - y0
