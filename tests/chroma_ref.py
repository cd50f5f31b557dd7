"""numpy statement of bilinear chroma upsampling at the signalled sample location
(test infrastructure; include/heifgpu.h "chroma upsampling").

Written from the geometry, not from the library's header: a chroma sample sits at a
position on a grid of quarter chroma steps, a luma sample between two of them takes
both in inverse proportion to its distance, in quarters.  The weights are explicit
tables per phase, indexed by the luma position's parity; the sample indices come from
np.floor_divide and np.clip.

upsample(cb, cr, chroma_format, loc, H, W) returns the two (H, W) planes; every test
feeds them to an existing reference (display_ref, scale_ref, ...) as a 4:4:4 picture.
"""
import numpy as np

# horizontal phase of a 4:2:0 sample location: 0 = on the even luma column, 1 = midway to the next
PX = {0: 0, 1: 1, 2: 0, 3: 1, 4: 0, 5: 1}
# vertical phase: locations 0, 1 midway between the two luma rows (1), 2, 3 on the top row (0), 4, 5 on the bottom row (2)
PY = {0: 1, 1: 1, 2: 0, 3: 0, 4: 2, 5: 2}

# per phase: for an even and an odd luma position p, (offset of the first chroma sample
# from p // 2, weight of the first, weight of the second), the weights in quarters.
#   phase 0 (chroma on the even position): even p sits on sample p/2; odd p halfway to the next
#   phase 1 (chroma a quarter step after the even position): even p a quarter before its
#            sample, so 1/4 of the previous one; odd p a quarter after it, so 1/4 of the next
#   phase 2 (chroma on the odd position): even p halfway between the previous and its own; odd p on its own
TAPS = {
    0: ((0, 4, 0), (0, 2, 2)),
    1: ((-1, 1, 3), (0, 3, 1)),
    2: ((-1, 2, 2), (0, 4, 0)),
}


def axis_taps(n_luma: int, n_chroma: int, phase, start: int = 0):
    """(i0, i1, w0, w1) arrays over luma positions start .. start + n_luma - 1; phase
    None: no filter (4:2:2 rows), the sample itself."""
    p = np.arange(start, start + n_luma)
    if phase is None:
        i = np.clip(p, 0, n_chroma - 1)
        return i, i, np.full(n_luma, 4), np.zeros(n_luma, dtype=int)
    table = np.array(TAPS[phase])[p & 1]  # (n, 3)
    first = np.floor_divide(p, 2) + table[:, 0]
    return (np.clip(first, 0, n_chroma - 1), np.clip(first + 1, 0, n_chroma - 1), table[:, 1], table[:, 2])


def phases(chroma_format: int, loc: int):
    if chroma_format == 1:
        return PX[loc], PY[loc]
    if chroma_format == 2:
        return 0, None
    raise ValueError("nothing to upsample")


def upsample_plane(c, chroma_format, loc, H, W, x0=0, y0=0):
    c = np.asarray(c).astype(np.int64)
    px, py = phases(chroma_format, loc)
    ix0, ix1, wx0, wx1 = axis_taps(W, c.shape[1], px, x0)
    iy0, iy1, wy0, wy1 = axis_taps(H, c.shape[0], py, y0)
    top = c[iy0][:, ix0] * wx0 + c[iy0][:, ix1] * wx1
    bot = c[iy1][:, ix0] * wx0 + c[iy1][:, ix1] * wx1
    return (top * wy0[:, None] + bot * wy1[:, None] + 8) >> 4


def upsample(cb, cr, chroma_format, loc, H, W):
    """Cb and Cr on the H x W luma grid; 4:4:4 planes come back as they are."""
    if chroma_format == 3:
        return np.asarray(cb), np.asarray(cr)
    dt = np.asarray(cb).dtype
    return (upsample_plane(cb, chroma_format, loc, H, W).astype(dt), upsample_plane(cr, chroma_format, loc, H, W).astype(dt))


def tapped_rect(chroma_format, loc, W, H, luma_box):
    """Brute force: the bounding box (x, y, w, h), in decoded luma coordinates clipped to
    W x H, of the luma samples of luma_box = (x, y, w, h) and of the cells of every chroma
    sample one of them taps (both taps, whatever their weights: the kernels load both)."""
    sx = 2
    sy = 2 if chroma_format == 1 else 1
    wc, hc = (W + sx - 1) // sx, (H + sy - 1) // sy
    px, py = phases(chroma_format, loc)
    x, y, w, h = luma_box
    xs, ys = set(range(x, x + w)), set(range(y, y + h))
    ix0, ix1, _, _ = axis_taps(w, wc, px, x)
    iy0, iy1, _, _ = axis_taps(h, hc, py, y)
    for i in set(ix0.tolist()) | set(ix1.tolist()):
        xs |= {v for v in range(i * sx, i * sx + sx) if v < W}
    for j in set(iy0.tolist()) | set(iy1.tolist()):
        ys |= {v for v in range(j * sy, j * sy + sy) if v < H}
    # (a luma sample's own cell is always among the tapped ones)
    return (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1)
