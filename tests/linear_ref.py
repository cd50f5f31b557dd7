"""The checker of the linear-light scaled render (test infrastructure): the contract of
include/heifgpu.h ("Linear-light scaled render") stated in numpy int64.

    L_c  = in_lut[c][code_c]                        per source pixel of the window
    S_c  = sum_j sum_i wy(Y,j) wx(X,i) L_c(j,i)     scale_ref.weights
    Lm_c = floor((2 S_c + cw ch) / (2 cw ch))
    out  = color_ref's matrix and out_lut step on (Lm_0, Lm_1, Lm_2)
    alpha = scale_ref.area_average of the codes

It shares no code with the library: the tables are read out of the transform the way
color_ref reads them, the weights are scale_ref's, the matrix and the encoding are
color_ref.apply_tables behind an input table that maps every level to itself.

model_average is the float64 yardstick of the accuracy test: per-pixel unquantised
linear levels from color_ref.Model, averaged in double, the true matrix, the encoding.
"""
import numpy as np

import color_ref
import scale_ref

LEVELS = np.tile(np.arange(65536, dtype=np.int64), (3, 1))  # the input table that leaves a level alone


def window_of(D, window):
    if window is None:
        window = (0, 0, D.shape[1], D.shape[0])
    cx, cy, cw, ch = window
    assert cw >= 1 and ch >= 1 and cx >= 0 and cy >= 0 and cx + cw <= D.shape[1] and cy + ch <= D.shape[0]
    return D[cy:cy + ch, cx:cx + cw], cw, ch


def mean_levels(in_lut, win, ow, oh):
    """Lm (oh, ow, 3) int64 of a window of codes (ch, cw, >= 3)."""
    ch, cw = win.shape[:2]
    wx, wy = scale_ref.weights(cw, ow), scale_ref.weights(ch, oh)
    # every product and partial sum is an integer below 2^48: exact in float64 in any order
    fx, fy = wx.astype(np.float64).T, wy.astype(np.float64)
    Lm = np.empty((oh, ow, 3), np.int64)
    for c in range(3):
        L = in_lut[c][win[..., c].astype(np.int64)]
        rows = L.astype(np.float64) @ fx               # [j, X] = sum_i wx(X, i) L[j, i]
        assert rows.max(initial=0) < 2.0 ** 53
        S = (fy @ rows).astype(np.int64)               # [Y, X]
        assert int(S.max(initial=0)) < 1 << 48
        Lm[..., c] = (2 * S + cw * ch) // (2 * cw * ch)
    return Lm


def linear_average(t, D, window, ow, oh):
    """The contract for a picture D (H, W, 3 or 4) of codes at t.bits and the window
    (cx, cy, cw, ch) of it (None: all) on an ow x oh grid; D's dtype is kept."""
    _, in_lut, m, out_lut = color_ref.tables(t)
    win, cw, ch = window_of(D, window)
    out = np.empty((oh, ow, D.shape[2]), D.dtype)
    Lm = mean_levels(in_lut, win, ow, oh)
    assert Lm.min() >= 0 and Lm.max() <= 65535
    out[..., :3] = color_ref.apply_tables(LEVELS, m, out_lut, Lm).astype(D.dtype)
    if D.shape[2] == 4:
        out[..., 3:] = scale_ref.area_average(win[..., 3:], None, ow, oh)
    return out


def model_average(model, bits, D, window, ow, oh):
    """float64 codes (oh, ow, 3), not rounded: the unquantised linear light of every pixel
    (the source's curves), the area average in double, the true matrix clipped to the
    destination's gamut, the sRGB encoding."""
    maxv = (1 << bits) - 1
    win, cw, ch = window_of(D, window)
    x = win[..., :3].astype(np.float64) / maxv
    lin = np.stack([np.clip(model.trc[c](x[..., c]), 0.0, 1.0) for c in range(3)], axis=-1)
    # sum_i wx(X, i) = cw and sum_j wy(Y, j) = ch: normalised, each output's weights sum to 1
    wx = scale_ref.weights(cw, ow).astype(np.float64) / cw
    wy = scale_ref.weights(ch, oh).astype(np.float64) / ch
    mean = np.einsum("Yj,jic,Xi->YXc", wy, lin, wx)
    M = np.eye(3) if model.own else model.M_true
    return maxv * color_ref.srgb_encode(np.clip(mean @ M.T, 0.0, 1.0))
