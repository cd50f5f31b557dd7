"""numpy restatement of the display stage (test infrastructure).

Deliberately independent of the library's folded map: the transformative
properties are applied one after the other, as array operations on the whole
picture, in the order given:

  ("clap", (wN, wD, hN, hD, hoffN, hoffD, voffN, voffD))  img[top:top+ch, left:left+cw]
  ("irot", k)                                               np.rot90(img, k)  (anticlockwise)
  ("imir", axis)                                            axis 0: img[:, ::-1]; axis 1: img[::-1]

The colour conversion happens first, on the decoded picture (so replicated
chroma keeps its phase under an odd crop): at 8 bits through rgb_ref, at the
image's own depth B with the formulas of include/heifgpu.h.  Like rgb_ref it
is the checker, "parity unpinned": nothing at hand renders imir or clap.
"""
from fractions import Fraction
import math

import numpy as np

import rgb_ref


def round_half_up(v: Fraction) -> int:
    return math.floor(v + Fraction(1, 2))


def clap_rect(W: int, H: int, f):
    """(left, top, cw, ch) of a clap on a W x H image; ValueError if it is not a
    rectangle inside the image."""
    wn, wd, hn, hd, hon, hod, von, vod = f
    if min(wd, hd, hod, vod) <= 0:
        raise ValueError("denominator")
    cw, ch = round_half_up(Fraction(wn, wd)), round_half_up(Fraction(hn, hd))
    left = round_half_up(Fraction(hon, hod) + Fraction(W - cw, 2))
    top = round_half_up(Fraction(von, vod) + Fraction(H - ch, 2))
    if cw < 1 or ch < 1 or left < 0 or top < 0 or left + cw > W or top + ch > H:
        raise ValueError("rectangle")
    return left, top, cw, ch


def apply_transforms(img: np.ndarray, steps):
    for kind, arg in steps:
        if kind == "clap":
            left, top, cw, ch = clap_rect(img.shape[1], img.shape[0], arg)
            img = img[top:top + ch, left:left + cw]
        elif kind == "irot":
            img = np.rot90(img, arg & 3)
        elif kind == "imir":
            img = img[::-1] if arg & 1 else img[:, ::-1]
        else:
            raise ValueError(kind)
    return img


def gather(img: np.ndarray, d):
    """img through a heifgpu_display_info-like map (out_width, out_height, m, t)."""
    oy, ox = np.mgrid[0:d.out_height, 0:d.out_width]
    return img[d.m[2] * ox + d.m[3] * oy + d.t[1], d.m[0] * ox + d.m[1] * oy + d.t[0]]


def rgb_at_depth(y, cb, cr, matrix: int, full: bool, B: int):
    """(H, W, 3) int64 at bit depth B (the 16-bit formats)."""
    kr, kb = 0.299, 0.114
    if matrix == 1:
        kr, kb = 0.2126, 0.0722
    elif matrix == 9:
        kr, kb = 0.2627, 0.0593
    kg = 1.0 - kr - kb
    top = (1 << B) - 1
    ys, cs = (1.0, 1.0) if full else (top / (219 << (B - 8)), top / (224 << (B - 8)))

    def fx(v):
        return int(v * 65536.0 + 0.5)

    yoff = 0 if full else 16 << (B - 8)
    Y = y.astype(np.int64)
    if cb is None:
        Cb = Cr = np.zeros_like(Y)
    else:
        h, w = Y.shape
        sy, sx = int(cb.shape[0] < h), int(cb.shape[1] < w)
        rows, cols = np.arange(h)[:, None] >> sy, np.arange(w)[None, :] >> sx
        Cb = cb.astype(np.int64)[rows, cols] - (1 << (B - 1))
        Cr = cr.astype(np.int64)[rows, cols] - (1 << (B - 1))
    yv = fx(ys) * (Y - yoff)
    r = (yv + fx(2 * (1 - kr) * cs) * Cr + 32768) >> 16
    g = (yv - fx(2 * kb * (1 - kb) / kg * cs) * Cb - fx(2 * kr * (1 - kr) / kg * cs) * Cr + 32768) >> 16
    b = (yv + fx(2 * (1 - kb) * cs) * Cb + 32768) >> 16
    assert max(abs(yv).max(), abs(r).max(), abs(g).max(), abs(b).max()) < 1 << 30  # int32 is enough
    return np.clip(np.stack([r, g, b], axis=-1), 0, top)


def render(y, cb, cr, matrix: int, full: bool, bit_depth: int, steps, fmt: str, alpha=None, alpha_depth: int = 8):
    """The displayed picture: (H', W', 3 or 4), uint8 for rgb8 / rgba8, uint16 for
    rgb16 / rgba16.  alpha: the alpha image's decoded luma (None = opaque)."""
    wide, with_alpha = fmt.endswith("16"), fmt.startswith("rgba")
    if wide:
        px = rgb_at_depth(y, cb, cr, matrix, full, bit_depth)
        top, depth = (1 << bit_depth) - 1, bit_depth
    else:
        px = rgb_ref.ycbcr_to_rgb(y, cb, cr, matrix, full, 0, bit_depth).astype(np.int64)
        top, depth = 255, 8
    if with_alpha:
        if alpha is None:
            a = np.full(y.shape, top, np.int64)
        else:
            a = alpha.astype(np.int64)
            a = a >> (alpha_depth - depth) if alpha_depth >= depth else a << (depth - alpha_depth)
        px = np.concatenate([px, a[..., None]], axis=-1)
    out = apply_transforms(px, steps)
    return np.ascontiguousarray(out).astype(np.uint16 if wide else np.uint8)
