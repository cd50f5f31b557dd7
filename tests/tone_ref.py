"""numpy restatement of the HDR render's tone stage (test infrastructure).

Two independent halves, as include/heifgpu.h ("HDR render") states them:

  apply(t, rgb)     the per-pixel integer formula over the tables, the luminance
                    weights and the Q14 matrix read out of a heifgpu_hdr_transform;
                    the library (heifgpu_color_apply, the kernels) must equal it
                    exactly;
  Model(...)        a float64 model from the nclx codes and a source peak: its own
                    ST 2084, HLG and BT.2390 code, the tables they round to and the
                    unquantised transform; light_levels() is its own reading of clli
                    and mdcv from the file's bytes and source_peak() the Lsrc rule.

The model follows the contract's structure (the gain comes from the luminance, every
channel is clamped to the destination white before the matrix, the result clips to the
destination's gamut); like color_ref's it uses the true matrix, rows not normalised.
"""
import struct

import numpy as np

import color_ref

U = 65535.0
WHITE = 203.0           # cd/m2 that U stands for (BT.2408)
ENTRIES = 577
MAX_LEVEL = (1 << 22) - 1
SHIFT = 24              # the gain table's fractional bits


# ---- the integer formula -------------------------------------------------------
def node(k):
    """The level of node k of the gain table."""
    k = np.asarray(k, np.int64)
    return np.where(k < 64, k, (32 + ((k - 32) & 31)) << np.maximum((k - 32) >> 5, 0))


def tables(t):
    """(bits, in_lut32 (3, n), w (3,), T (577,), m (9,), out_lut (4097,)) of an HdrTransform, as int64."""
    n = 1 << t.base.bits
    in32 = np.array([list(t.in_lut32[c][:n]) for c in range(3)], np.int64)
    return (t.base.bits, in32, np.array(list(t.w), np.int64), np.array(list(t.T[:ENTRIES]), np.int64),
            np.array(list(t.base.m), np.int64), np.array(list(t.base.out_lut[:color_ref.OUT_ENTRIES]), np.int64))


def luminance(in32, w, rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    L = np.stack([in32[c][rgb[..., c]] for c in range(3)], axis=-1)
    return L, (w[0] * L[..., 0] + w[1] * L[..., 1] + w[2] * L[..., 2] + 8192) >> 14


def index(Y):
    """(idx, e, frac) of the floating index at luminance Y (int64 arrays); e = 0 below 64."""
    Y = np.asarray(Y, np.int64)
    bl = np.zeros_like(Y)
    v = Y.copy()
    while (v > 0).any():
        bl += v > 0
        v >>= 1
    e = np.where(Y < 64, 0, bl - 6)
    idx = np.where(Y < 64, Y, 32 * e + (Y >> e))
    return idx, e, np.where(Y < 64, 0, Y & ((1 << e) - 1))


def gain(T, Y):
    idx, e, frac = index(Y)
    hi = T[np.minimum(idx + 1, ENTRIES - 1)]
    half = np.where(e > 0, 1 << np.maximum(e - 1, 0), 0)
    return np.where(e == 0, T[idx], (T[idx] * ((1 << e) - frac) + hi * frac + half) >> e)


def apply_tables(in32, w, T, m, out_lut, rgb):
    L, Y = luminance(in32, w, rgb)
    g = gain(T, Y)
    L2 = np.minimum((L * g[..., None] + (1 << (SHIFT - 1))) >> SHIFT, 65535)
    out = np.empty_like(L2)
    for k in range(3):
        s = m[3 * k] * L2[..., 0] + m[3 * k + 1] * L2[..., 1] + m[3 * k + 2] * L2[..., 2]
        Lp = np.clip((s + 8192) >> 14, 0, 65535)
        i, f = Lp >> 4, Lp & 15
        out[..., k] = (out_lut[i] * (16 - f) + out_lut[i + 1] * f + 128) >> 8
    return out


def apply(t, rgb):
    """The formula over t's tables for (..., 3) integer codes; int64 out."""
    _, in32, w, T, m, out_lut = tables(t)
    return apply_tables(in32, w, T, m, out_lut, rgb)


def is_tone(t):
    return t is not None and bool(getattr(t, "tone", 0))


def transform_picture(t, px):
    """A rendered picture (H, W, 3 or 4) through t, whichever kind t is: a tone transform
    by the formula above, any other as color_ref.transform_picture does; alpha and dtype kept."""
    if not is_tone(t):
        return color_ref.transform_picture(t, px)
    out = px.copy()
    out[..., :3] = apply(t, px[..., :3]).astype(px.dtype)
    return out


# ---- the float64 model ---------------------------------------------------------
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0


def pq_eotf(e):
    """ST 2084: code value in [0, 1] to cd/m2."""
    p = np.maximum(np.asarray(e, np.float64), 0.0) ** (1.0 / M2)
    return 10000.0 * (np.maximum(p - C1, 0.0) / (C2 - C3 * p)) ** (1.0 / M1)


def pq_inverse(nits):
    y = (np.maximum(np.asarray(nits, np.float64), 0.0) / 10000.0) ** M1
    return ((C1 + C2 * y) / (1.0 + C3 * y)) ** M2


def hlg_inverse_oetf(x):
    """BT.2100: HLG signal in [0, 1] to scene light in [0, 1]."""
    a = 0.17883277
    b, c = 1.0 - 4.0 * a, 0.5 - a * np.log(4.0 * a)
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.5, x * x / 3.0, (np.exp((np.maximum(x, 0.5) - c) / a) + b) / 12.0)


def eetf(x, lsrc):
    """BT.2390 5.4.1 from a display of peak lsrc to one of 203 cd/m2, cd/m2 in and out,
    on PQ values normalised to the source range; black 0 on both sides."""
    x = np.minimum(np.asarray(x, np.float64), lsrc)
    n0 = pq_inverse(0.0)
    span = pq_inverse(lsrc) - n0
    e1 = (pq_inverse(x) - n0) / span
    max_lum = (pq_inverse(WHITE) - n0) / span
    ks = 1.5 * max_lum - 0.5
    t = np.where(e1 > ks, (e1 - ks) / np.where(ks < 1.0, 1.0 - ks, 1.0), 0.0)
    e2 = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1 - ks) + (3 * t ** 2 - 2 * t ** 3) * max_lum
    return np.where(e1 > ks, pq_eotf(e2 * span + n0), x)


def knee(lsrc):
    """The luminance in cd/m2 at which the spline starts (the EETF is the identity below it)."""
    n0 = pq_inverse(0.0)
    span = pq_inverse(lsrc) - n0
    ks = 1.5 * (pq_inverse(WHITE) - n0) / span - 0.5
    return float(pq_eotf(ks * span + n0))


class Model:
    """The float64 model of one nclx HDR source (primaries 1, 9, 12; transfer 16, 18),
    a source peak in cd/m2 (HLG: always 1000) and a destination."""

    def __init__(self, primaries, transfer, dst, lsrc=1000.0):
        assert transfer in (16, 18)
        self.transfer, self.dst = transfer, dst
        self.lsrc = 1000.0 if transfer == 18 else float(min(max(lsrc, WHITE), 10000.0))
        self.matrix = color_ref.Model((primaries, 8), dst)
        xy = color_ref.NCLX_XY[1 if primaries == 2 else primaries]
        P = np.array([[x / y, 1.0, (1 - x - y) / y] for x, y in xy]).T
        W = np.array([0.3127 / 0.3290, 1.0, (1 - 0.3127 - 0.3290) / 0.3290])
        S = np.linalg.solve(P, W)  # the Y row of RGB -> XYZ
        self.w = S / S.sum()

    def light(self, x):
        """cd/m2 of a code value in [0, 1] (HLG: scene light scaled to 1000, before the OOTF)."""
        return pq_eotf(x) if self.transfer == 16 else 1000.0 * hlg_inverse_oetf(x)

    def G(self, yn):
        """The gain at luminance yn in cd/m2."""
        yn = np.asarray(yn, np.float64)
        safe = np.where(yn > 0, yn, 1.0)
        if self.transfer == 16:
            return np.where(yn > 0, np.minimum(eetf(safe, self.lsrc) / safe, 1.0), 1.0)
        ys = safe / 1000.0
        yd = 1000.0 * ys ** 1.2
        return np.where(yn > 0, np.minimum(ys ** 0.2 * eetf(yd, 1000.0) / yd, 1.0), 0.0)

    def in_lut32(self, bits):
        maxv = (1 << bits) - 1
        return np.floor(U * self.light(np.arange(maxv + 1) / maxv) / WHITE + 0.5).astype(np.int64)

    def T(self):
        return np.floor(float(1 << SHIFT) * self.G(WHITE * node(np.arange(ENTRIES)) / U) + 0.5).astype(np.int64)

    def w_q14(self):
        """The weights in Q14, unrounded."""
        return self.w * 16384.0

    def display_light(self, yn):
        """The luminance in cd/m2 that the tone curve sees (HLG: after the OOTF)."""
        yn = np.asarray(yn, np.float64)
        return yn if self.transfer == 16 else 1000.0 * (yn / 1000.0) ** 1.2

    def transform(self, bits, rgb):
        """The unquantised transform of (..., 3) codes: float64 codes out, not rounded."""
        maxv = (1 << bits) - 1
        L = self.light(np.asarray(rgb, np.float64) / maxv)
        g = self.G(L @ self.w)
        lin = np.minimum(L * g[..., None] / WHITE, 1.0)
        M = np.eye(3) if self.matrix.own else self.matrix.M_true
        return maxv * color_ref.srgb_encode(np.clip(lin @ M.T, 0.0, 1.0))


# ---- clli / mdcv from the file's bytes -----------------------------------------
def _boxes(buf, start, end):
    """(type, payload start, payload end) of the boxes in buf[start:end]."""
    pos = start
    while pos + 8 <= end:
        size, typ = struct.unpack_from(">I4s", buf, pos)
        head = 8
        if size == 1:
            size, head = struct.unpack_from(">Q", buf, pos + 8)[0], 16
        elif size == 0:
            size = end - pos
        if size < head or pos + size > end:
            return
        yield typ, pos + head, pos + size
        pos += size


def light_levels(heic: bytes):
    """{"clli": (MaxCLL, MaxFALL), "mdcv": (max cd/m2, min cd/m2)} of the first clli and mdcv
    in the file's ipco; a key is missing without the box and None for one shorter than its fields."""
    out = {}

    def walk(start, end, path):
        for typ, a, b in _boxes(heic, start, end):
            if typ == b"meta":
                walk(a + 4, b, path + [typ])  # FullBox
            elif typ in (b"iprp", b"ipco"):
                walk(a, b, path + [typ])
            elif typ == b"clli" and path and path[-1] == b"ipco" and "clli" not in out:
                out["clli"] = struct.unpack_from(">HH", heic, a) if b - a >= 4 else None
            elif typ == b"mdcv" and path and path[-1] == b"ipco" and "mdcv" not in out:
                out["mdcv"] = tuple(v * 1e-4 for v in struct.unpack_from(">II", heic, a + 16)) if b - a >= 24 else None

    walk(0, len(heic), [])
    return out


def source_peak(heic: bytes, transfer, peak_nits=None):
    """Lsrc by the header's rule."""
    if transfer == 18:
        return 1000.0
    ll = light_levels(heic)
    l = 1000.0
    if peak_nits is not None and peak_nits > 0:
        l = float(peak_nits)
    elif ll.get("clli") and ll["clli"][0]:
        l = float(ll["clli"][0])
    elif ll.get("mdcv") and ll["mdcv"][0]:
        l = ll["mdcv"][0]
    return min(max(l, WHITE), 10000.0)
