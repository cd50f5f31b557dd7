"""The checker of the scaled render (test infrastructure): the exact area
average of include/heifgpu.h, stated literally in numpy int64 (or Python ints
where the sum passes 2^63), and heifgpu_scale_fit's rules in fractions.

D, the displayed picture, comes from display_ref.render, so nothing here shares
code with the library's folded map.  Like display_ref it is "parity unpinned":
nothing at hand renders a scaled HEIC to compare with.
"""
from fractions import Fraction
import math

import numpy as np


def weights(c: int, o: int) -> np.ndarray:
    """(o, c) int64: w[X, i] = max(0, min((i+1)*o, (X+1)*c) - max(i*o, X*c))."""
    X = np.arange(o, dtype=np.int64)[:, None]
    i = np.arange(c, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * o, (X + 1) * c) - np.maximum(i * o, X * c))


def area_average(D: np.ndarray, window, ow: int, oh: int) -> np.ndarray:
    """R of the window (cx, cy, cw, ch) of D (H, W, C) on an ow x oh grid;
    window None = the whole picture.  The dtype of D is kept."""
    if window is None:
        window = (0, 0, D.shape[1], D.shape[0])
    cx, cy, cw, ch = window
    assert cw >= 1 and ch >= 1 and cx >= 0 and cy >= 0 and cx + cw <= D.shape[1] and cy + ch <= D.shape[0]
    win = D[cy:cy + ch, cx:cx + cw]
    wx, wy = weights(cw, ow), weights(ch, oh)
    # acc <= max(D) * cw * ch: above 2^32 for a 12-bit megapixel, below 2^53 for any window
    # the library takes (sides up to 65535, 12-bit samples: 2^44).  The two sums are matrix
    # products, taken in float64 for speed: every product and every partial sum is an
    # integer below 2^53, which float64 holds exactly in whatever order they are added.
    assert int(win.max(initial=0)) * cw * ch < 1 << 53
    out = np.empty((oh, ow, D.shape[2]), D.dtype)
    fx, fy = wx.astype(np.float64).T, wy.astype(np.float64)
    for c in range(D.shape[2]):
        rows = win[..., c].astype(np.float64) @ fx     # [j, X] = sum_i wx(X, i) * D[j, i]
        acc = (fy @ rows).astype(np.int64)             # [Y, X] = sum_j wy(Y, j) * rows[j, X]
        out[..., c] = (2 * acc + cw * ch) // (2 * cw * ch)
    return out


def round_half_up(v: Fraction) -> int:
    return math.floor(v + Fraction(1, 2))


def fit(dw: int, dh: int, bw: int, bh: int, mode: str):
    """(out_width, out_height, x, y, width, height) as heifgpu_scale_fit gives
    them; the whole picture is (.., 0, 0, 0, 0)."""
    if bw < 1 or bh < 1:
        raise ValueError("box")
    wider = Fraction(dw, dh) >= Fraction(bw, bh)
    if mode == "stretch":
        return bw, bh, 0, 0, 0, 0
    if mode == "contain":
        if wider:
            return bw, max(1, round_half_up(Fraction(dh * bw, dw))), 0, 0, 0, 0
        return max(1, round_half_up(Fraction(dw * bh, dh))), bh, 0, 0, 0, 0
    if mode == "cover":
        if wider:
            w = max(1, round_half_up(Fraction(dh * bw, bh)))
            return bw, bh, (dw - w) // 2, 0, w, dh
        h = max(1, round_half_up(Fraction(dw * bh, bw)))
        return bw, bh, 0, (dh - h) // 2, dw, h
    raise ValueError(mode)
