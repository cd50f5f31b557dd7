"""numpy restatement of the scaled gain-map HDR render (test infrastructure), written from
include/heifgpu.h "Gain-map HDR render", the scaled call, out of the existing checkers:

  - the base's integers at depth B (display_ref.rgb_at_depth) and the Q8 gain code of every
    decoded base position (gain_ref.sample_map), brought into displayed orientation
    (display_ref.apply_transforms), with the alpha samples as decoded;
  - scale_ref.area_average of each over the window: C_c, Gq, A;
  - gain_ref.apply_tables on (C, Gq), gain_ref.encode_alpha on A.

Nothing here calls the library or shares code with it.
"""
import numpy as np

import display_ref
import gain_ref
import scale_ref


def displayed(t, y, cb, cr, matrix, full, gain_plane, steps, alpha=None):
    """(rgb (H', W', 3), gq (H', W'), alpha (H', W') or None), int64, in displayed orientation."""
    px = display_ref.rgb_at_depth(y, cb, cr, matrix, full, int(t.bits))
    gq = gain_ref.sample_map(gain_plane, y.shape[1], y.shape[0])
    rgb = np.ascontiguousarray(display_ref.apply_transforms(px, steps))
    g = np.ascontiguousarray(display_ref.apply_transforms(gq, steps))
    a = None if alpha is None else np.ascontiguousarray(display_ref.apply_transforms(alpha.astype(np.int64), steps))
    return rgb, g, a


def average_codes(gq, window, ow, oh):
    """avg(g) of a (H, W) array of gain codes: (oh, ow) int64."""
    return scale_ref.area_average(np.asarray(gq, np.int64)[..., None], window, ow, oh)[..., 0]


def from_displayed(tb, rgb, gq, alpha, alpha_depth, window, ow, oh, with_alpha):
    """The rendered picture, uint16 (oh, ow, 3 or 4), from the displayed arrays; window
    (cx, cy, cw, ch) or None for the whole picture."""
    C = scale_ref.area_average(rgb, window, ow, oh)
    G = average_codes(gq, window, ow, oh)
    out = gain_ref.apply_tables(tb, C, G)
    if with_alpha:
        A = None if alpha is None else scale_ref.area_average(alpha[..., None], window, ow, oh)[..., 0]
        out = np.concatenate([out, gain_ref.encode_alpha(tb, A, alpha_depth, (oh, ow))[..., None]], axis=-1)
    return np.ascontiguousarray(out)


def render(t, y, cb, cr, matrix, full, gain_plane, steps, window, ow, oh, with_alpha=False, alpha=None, alpha_depth=8):
    """heifgpu_render_batch_gain_scaled of one picture: the planes are the decoded ones,
    steps as display_ref.apply_transforms takes them."""
    rgb, gq, a = displayed(t, y, cb, cr, matrix, full, gain_plane, steps, alpha if with_alpha else None)
    return from_displayed(gain_ref.tables(t), rgb, gq, a, alpha_depth, window, ow, oh, with_alpha)
