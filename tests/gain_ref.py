"""numpy restatement of the gain-map HDR render (test infrastructure), written from
include/heifgpu.h "Gain-map HDR render": the sampler's position arithmetic in exact
integers, the multiplier, the apply, the matrix and the two encodings bit for bit, the
table rules in float64, and a float64 model of the whole stage with no fixed point
anywhere (its matrix is the transform's Q14 one read as a float: that rounding is the
colour-managed render's, measured there).  Nothing here calls the library.
"""
import math

import numpy as np

import display_ref

U = 65535
LEVEL_MAX = (1 << 24) - 1
E_ENTRIES = 641


# ---- the sampler ---------------------------------------------------------------
def taps(W: int, Wg: int):
    """(i0, i1, f) int64 arrays over decoded base positions s = 0 .. W - 1, by the
    contract's own integers: n = (2 s + 1) Wg - W, d = 2 W."""
    s = np.arange(W, dtype=np.int64)
    n, d = (2 * s + 1) * Wg - W, 2 * W
    i = n // d  # floor (numpy's // floors for negatives)
    f = (256 * (n - i * d)) // d
    return np.clip(i, 0, Wg - 1), np.clip(i + 1, 0, Wg - 1), f, i


def sample_map(G: np.ndarray, W: int, H: int) -> np.ndarray:
    """The Q8 gain code of every decoded base position: (H, W) int64."""
    G = G.astype(np.int64)
    Hg, Wg = G.shape
    x0, x1, fx, _ = taps(W, Wg)
    y0, y1, fy, _ = taps(H, Hg)
    fx, fy = fx[None, :], fy[:, None]
    top = (256 - fx) * G[y0][:, x0] + fx * G[y0][:, x1]
    bot = (256 - fx) * G[y1][:, x0] + fx * G[y1][:, x1]
    return ((256 - fy) * top + fy * bot + 128) >> 8


def borders_bind(W: int, Wg: int):
    """(low, high): whether the clamp at 0 and the clamp at Wg - 1 change a tap."""
    _, _, _, i = taps(W, Wg)
    return bool((i < 0).any()), bool((i + 1 > Wg - 1).any())


# ---- the tables in float64 -----------------------------------------------------
def rhu(v):
    return np.floor(np.asarray(v, np.float64) + 0.5)


def f709(v):
    v = np.asarray(v, np.float64)
    return np.where(v < 0.081, v / 4.5, ((v + 0.099) / 1.099) ** (1 / 0.45))


def pq_inverse(y):
    m1, m2 = 2610 / 16384, 2523 / 4096 * 128
    c1, c2, c3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    p = np.maximum(np.asarray(y, np.float64), 0.0) ** m1
    return ((c1 + c2 * p) / (1 + c3 * p)) ** m2


def weight(display_headroom, hbase, halt):
    if display_headroom is None or display_headroom <= 0:
        return 1.0
    return min(max((math.log2(display_headroom) - hbase) / (halt - hbase), 0.0), 1.0)


def log2_gain_iso(x, w, gmin, gmax, gamma):
    """log2 of the multiplier at map value x in [0, 1] (float)."""
    return w * (gmin + (gmax - gmin) * np.asarray(x, np.float64) ** (1.0 / gamma))


def T_iso(gain_bits, w, gmin, gmax, gamma):
    maxg = (1 << gain_bits) - 1
    v = np.arange(maxg + 1) / maxg
    T = rhu(65536.0 * 2.0 ** log2_gain_iso(v, w, gmin, gmax, gamma))
    return np.append(T, T[-1])


def apple_hr(headroom, display_headroom):
    if display_headroom is None or display_headroom <= 0:
        return headroom
    return min(headroom, max(display_headroom, 1.0))


def T_apple(gain_bits, hr):
    maxg = (1 << gain_bits) - 1
    T = rhu(65536.0 * (1.0 + (hr - 1.0) * f709(np.arange(maxg + 1) / maxg)))
    return np.append(T, T[-1])


def node(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 64, k, (32 + ((k - 32) & 31)) << np.maximum((k - 32) >> 5, 0))


def E_table(pq_bits, sdr_white=203.0):
    maxp = (1 << pq_bits) - 1
    nits = np.minimum(sdr_white * node(np.arange(E_ENTRIES)) / U, 10000.0)
    return rhu(256.0 * maxp * pq_inverse(nits / 10000.0))


# ---- the per-pixel formula, bit for bit ----------------------------------------
def tables(t):
    """What apply_tables reads, from a _lib.GainTransform."""
    n, ng = 1 << t.bits, (1 << t.gain_bits) + 1
    in_lut = np.array([np.ctypeslib.as_array(t.in_lut[c])[:n] for c in range(3)], np.int64)
    return dict(in_lut=in_lut, T=np.ctypeslib.as_array(t.T)[:ng].astype(np.int64),
                E=np.ctypeslib.as_array(t.E)[:E_ENTRIES].astype(np.int64), m=np.array(list(t.m), np.int64),
                k_b=int(t.k_b), k_a=int(t.k_a), encoding=int(t.encoding), pq_bits=int(t.pq_bits))


def multiplier(T, gq):
    i, f = gq >> 8, gq & 255
    return (T[i] * (256 - f) + T[i + 1] * f + 128) >> 8


def levels(tb, rgb, gq, parts=None):
    """H' (..., 3) int64 of codes rgb (..., 3) and gain codes gq (...).  parts: a dict
    that receives the unclamped H and H' (which clamps bind)."""
    rgb, gq = np.asarray(rgb, np.int64), np.asarray(gq, np.int64)
    M = multiplier(tb["T"], gq)[..., None]
    L = np.stack([tb["in_lut"][c][rgb[..., c]] for c in range(3)], axis=-1)
    raw = (((L + tb["k_b"]) * M + 32768) >> 16) - tb["k_a"]
    Hc = np.clip(raw, 0, LEVEL_MAX)
    m = tb["m"].reshape(3, 3)
    raw2 = ((Hc[..., None, :] * m).sum(axis=-1) + 8192) >> 14
    if parts is not None:
        parts["H"], parts["H2"] = raw, raw2
    return np.clip(raw2, 0, LEVEL_MAX)


def encode_linear(level):
    """binary16 bits of fmul_rn(float32(level), c), c the binary32 nearest to 1 / 65535."""
    c = np.float32(1.0) / np.float32(65535.0)
    f = np.asarray(level).astype(np.float32) * c
    return f.astype(np.float16).view(np.uint16)


def encode_pq(E, level):
    Y = np.asarray(level, np.int64)
    bl = np.zeros_like(Y)
    v = Y.copy()
    while (v > 0).any():
        bl += v > 0
        v >>= 1
    e = np.maximum(bl - 6, 1)
    idx = np.where(Y < 64, Y, 32 * e + (Y >> e))
    frac = Y & ((1 << e) - 1)
    wide = (E[idx] * ((1 << e) - frac) + E[np.minimum(idx + 1, E_ENTRIES - 1)] * frac + (1 << (e - 1))) >> e
    return ((np.where(Y < 64, E[idx], wide) + 128) >> 8).astype(np.uint16)


def apply_tables(tb, rgb, gq, parts=None):
    lv = levels(tb, rgb, gq, parts)
    return encode_pq(tb["E"], lv) if tb["encoding"] == 1 else encode_linear(lv)


def apply(t, rgb, gq):
    return apply_tables(tables(t), rgb, gq)


def encode_alpha(tb, alpha, alpha_depth, shape):
    """The alpha channel of a picture of `shape` (H, W): uint16."""
    if tb["encoding"] == 1:
        P = tb["pq_bits"]
        if alpha is None:
            return np.full(shape, (1 << P) - 1, np.uint16)
        a = alpha.astype(np.int64)
        return (a << (P - alpha_depth) if P >= alpha_depth else a >> (alpha_depth - P)).astype(np.uint16)
    if alpha is None:
        return np.full(shape, 0x3C00, np.uint16)
    ca = np.float32(1.0) / np.float32((1 << alpha_depth) - 1)
    return (alpha.astype(np.float32) * ca).astype(np.float16).view(np.uint16)


def render(t, y, cb, cr, matrix, full, gain_plane, steps, with_alpha=False, alpha=None, alpha_depth=8, parts=None):
    """The displayed HDR picture as uint16 (H', W', 3 or 4): binary16 bits or PQ codes.
    The planes are the decoded ones; steps as display_ref.apply_transforms takes them."""
    tb = tables(t)
    px = display_ref.rgb_at_depth(y, cb, cr, matrix, full, int(t.bits))
    gq = sample_map(gain_plane, y.shape[1], y.shape[0])
    out = apply_tables(tb, px, gq, parts)
    if with_alpha:
        out = np.concatenate([out, encode_alpha(tb, alpha, alpha_depth, y.shape)[..., None]], axis=-1)
    return np.ascontiguousarray(display_ref.apply_transforms(out, steps))


# ---- the float64 model ---------------------------------------------------------
def model_levels(trc, m_float, log2_gain, base_offset, alt_offset, maxv, maxg, rgb, g_float):
    """H' in units of 1 / 65535 of SDR white, float64, unquantised: trc(code / maxv) per
    channel, the multiplier 2^log2_gain(g / maxg) of the float gain sample g_float, the
    offsets as fractions of SDR white, the matrix, the clamps of the contract."""
    rgb = np.asarray(rgb, np.float64)
    L = np.stack([trc[c](rgb[..., c] / maxv) for c in range(3)], axis=-1)
    M = 2.0 ** log2_gain(np.asarray(g_float, np.float64) / maxg)
    Hc = np.clip((L + base_offset) * M[..., None] - alt_offset, 0.0, LEVEL_MAX / U)
    out = (Hc[..., None, :] * np.asarray(m_float, np.float64).reshape(3, 3)).sum(axis=-1)
    return np.clip(out, 0.0, LEVEL_MAX / U) * U


def model_pq(level_float, pq_bits, sdr_white=203.0):
    """PQ codes (float, unrounded) of levels in units of 1 / 65535 of SDR white."""
    nits = np.minimum(sdr_white * np.asarray(level_float, np.float64) / U, 10000.0)
    return ((1 << pq_bits) - 1) * pq_inverse(nits / 10000.0)
