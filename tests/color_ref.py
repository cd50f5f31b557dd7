"""numpy restatement of the colour-managed render (test infrastructure).

Two independent halves, as include/heifgpu.h ("colour-managed render") states them:

  apply(t, rgb)        the per-pixel integer formula over the tables and the Q14
                       matrix read out of a heifgpu_color_transform; the library
                       (heifgpu_color_apply, the kernels) must equal it exactly;
  Model(source, dst)   a float64 model built from the profile's bytes (its own ICC
                       reader) or the nclx codes: the curves, the matrix, the
                       tables they round to and the unquantised transform.  It is
                       the yardstick for the tables (within 1 unit: libm and numpy
                       pow may differ in the last ulp of a value that is then
                       rounded) and for the accuracy of the integer path.

"Parity unpinned", like display_ref: no CMM is at hand, the float model is the checker.
"""
import struct

import numpy as np

D50 = np.array([0xF6D6, 0x10000, 0xD32D], np.float64) / 65536.0
DST = {
    "srgb": np.array([[0x6FA2, 0x38F5, 0x0390], [0x6299, 0xB785, 0x18DA], [0x24A0, 0x0F84, 0xB6CF]], np.float64),
    "display-p3": np.array([[0x83DF, 0x3DBF, -0x45], [0x4ABF, 0xB137, 0x0AB9], [0x2838, 0x110B, 0xC8B9]], np.float64),
}
OWN_PRIMARIES = {"srgb": 1, "display-p3": 12}
OUT_ENTRIES = 4097


# ---- the integer formula -------------------------------------------------------
def tables(t):
    """(bits, in_lut (3, 1 << bits), m (9,), out_lut (4097,)) of a ColorTransform, as int64."""
    n = 1 << t.bits
    in_lut = np.array([list(t.in_lut[c][:n]) for c in range(3)], np.int64)
    return t.bits, in_lut, np.array(list(t.m), np.int64), np.array(list(t.out_lut[:OUT_ENTRIES]), np.int64)


def apply_tables(in_lut, m, out_lut, rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    L = np.stack([in_lut[c][rgb[..., c]] for c in range(3)], axis=-1)
    out = np.empty_like(L)
    for k in range(3):
        s = m[3 * k] * L[..., 0] + m[3 * k + 1] * L[..., 1] + m[3 * k + 2] * L[..., 2]
        Lp = np.clip((s + 8192) >> 14, 0, 65535)  # (numpy's >> on int64 is arithmetic)
        i, f = Lp >> 4, Lp & 15
        out[..., k] = (out_lut[i] * (16 - f) + out_lut[i + 1] * f + 128) >> 8
    return out


def apply(t, rgb):
    """The formula over t's tables for (..., 3) integer codes; int64 out."""
    _, in_lut, m, out_lut = tables(t)
    return apply_tables(in_lut, m, out_lut, rgb)


def transform_picture(t, px):
    """A rendered picture (H, W, 3 or 4) through t: colour converted, alpha kept, dtype kept.
    An identity transform (or None) returns the picture as it is, which is what a render does."""
    if t is None or t.identity:
        return px
    out = px.copy()
    out[..., :3] = apply(t, px[..., :3]).astype(px.dtype)
    return out


def lattice(bits, step):
    """Every step-th code of the cube (and maxv), as (n, 3) codes."""
    maxv = (1 << bits) - 1
    v = np.unique(np.append(np.arange(0, maxv + 1, step), maxv))
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


# ---- the float64 model ---------------------------------------------------------
def srgb_decode(x):
    x = np.asarray(x, np.float64)
    return np.where(x >= 0.04045, ((x + 0.055) / 1.055) ** 2.4, x / 12.92)


def srgb_encode(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.maximum(x, 0.0) ** (1.0 / 2.4) - 0.055)


def _pow(base, g):
    return np.where(base > 0, np.maximum(base, 0.0) ** g, 0.0)


def _s15f16(b, o):
    return struct.unpack_from(">i", b, o)[0] / 65536.0


def read_trc(tag):
    """A curv / para tag body as a function of x in [0, 1] (float64 arrays)."""
    kind = tag[:4]
    if kind == b"curv":
        n = struct.unpack_from(">I", tag, 8)[0]
        if n == 0:
            return lambda x: np.asarray(x, np.float64)
        if n == 1:
            g = struct.unpack_from(">H", tag, 12)[0] / 256.0
            return lambda x: _pow(np.asarray(x, np.float64), g)
        tab = np.array(struct.unpack_from(">%dH" % n, tag, 12), np.float64) / 65535.0
        return lambda x: np.interp(np.asarray(x, np.float64) * (n - 1), np.arange(n), tab)
    assert kind == b"para", kind
    fn = struct.unpack_from(">H", tag, 8)[0]
    cnt = (1, 3, 4, 5, 7)[fn]
    p = [_s15f16(tag, 12 + 4 * i) for i in range(cnt)] + [0.0] * 7
    g, a, b, c, d, e, f = p[:7]
    if fn == 0:
        return lambda x: _pow(np.asarray(x, np.float64), g)
    if fn == 1:
        return lambda x: np.where(np.asarray(x) >= -b / a, _pow(a * np.asarray(x, np.float64) + b, g), 0.0)
    if fn == 2:
        return lambda x: np.where(np.asarray(x) >= -b / a, _pow(a * np.asarray(x, np.float64) + b, g) + c, c)
    if fn == 3:
        return lambda x: np.where(np.asarray(x) >= d, _pow(a * np.asarray(x, np.float64) + b, g), c * np.asarray(x))
    return lambda x: np.where(np.asarray(x) >= d, _pow(a * np.asarray(x, np.float64) + b, g) + e, c * np.asarray(x) + f)


def read_profile(icc: bytes):
    """(colourants (3, 3): row c = X Y Z of primary c, [f_r, f_g, f_b]) of a matrix/TRC profile."""
    n = struct.unpack_from(">I", icc, 128)[0]
    tags = {}
    for k in range(n):
        sig, off, ln = struct.unpack_from(">4sII", icc, 132 + 12 * k)
        tags.setdefault(sig, icc[off:off + ln])
    col = np.array([[_s15f16(tags[s], 8 + 4 * k) for k in range(3)] for s in (b"rXYZ", b"gXYZ", b"bXYZ")])
    return col, [read_trc(tags[s]) for s in (b"rTRC", b"gTRC", b"bTRC")]


NCLX_XY = {1: ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)),
           9: ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)),
           12: ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))}
BRADFORD = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])


def nclx_colorants(primaries):
    """Chromaticities to XYZ with the D65 white, then Bradford to the ICC D50 white."""
    xy = NCLX_XY[1 if primaries == 2 else primaries]
    P = np.array([[x / y, 1.0, (1 - x - y) / y] for x, y in xy]).T  # columns: the primaries
    W = np.array([0.3127 / 0.3290, 1.0, (1 - 0.3127 - 0.3290) / 0.3290])
    S = np.linalg.solve(P, W)
    A = np.linalg.inv(BRADFORD) @ np.diag((BRADFORD @ D50) / (BRADFORD @ W)) @ BRADFORD
    return (A @ (P * S)).T


def nclx_trc(transfer):
    if transfer in (1, 2, 6, 13, 14, 15):
        return srgb_decode
    if transfer == 8:
        return lambda x: np.asarray(x, np.float64)
    assert transfer == 4, transfer
    return lambda x: _pow(np.asarray(x, np.float64), 2.2)


class Model:
    """The float64 model of one source and destination.  source: the profile's bytes,
    or (primaries, transfer) of an nclx, or None (no colr: sRGB)."""

    def __init__(self, source, dst):
        self.dst = dst
        self.own = False
        if isinstance(source, (bytes, bytearray)):
            self.col, self.trc = read_profile(bytes(source))
        else:
            prim, tr = source if source is not None else (2, 2)
            self.col, self.trc = nclx_colorants(prim), [nclx_trc(tr)] * 3
            self.own = (1 if prim == 2 else prim) == OWN_PRIMARIES[dst]
        # XYZ = col.T @ rgb; the true colorimetric matrix and the contract's (rows normalised)
        self.M_true = np.linalg.inv((DST[dst] / 65536.0).T) @ self.col.T
        self.M = np.eye(3) if self.own else self.M_true / self.M_true.sum(axis=1, keepdims=True)

    def in_lut(self, bits):
        maxv = (1 << bits) - 1
        x = np.arange(maxv + 1) / maxv
        return np.array([np.floor(65535.0 * np.clip(f(x), 0.0, 1.0) + 0.5) for f in self.trc]).astype(np.int64)

    def out_lut(self, bits):
        maxv = (1 << bits) - 1
        l = np.minimum(16 * np.arange(OUT_ENTRIES), 65535) / 65535.0
        return np.floor(16.0 * maxv * srgb_encode(l) + 0.5).astype(np.int64)

    def m_q14(self):
        """The model's matrix in Q14, unrounded."""
        return (self.M * 16384.0).reshape(9)

    def transform(self, bits, rgb):
        """The unquantised transform of (..., 3) codes: float64 codes out, not rounded.
        The true matrix (rows not normalised), clipped to the destination's gamut."""
        maxv = (1 << bits) - 1
        x = np.asarray(rgb, np.float64) / maxv
        lin = np.stack([np.clip(self.trc[c](x[..., c]), 0.0, 1.0) for c in range(3)], axis=-1)
        M = np.eye(3) if self.own else self.M_true
        return maxv * srgb_encode(np.clip(lin @ M.T, 0.0, 1.0))
