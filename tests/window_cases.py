"""What the two window-decode test files share (test infrastructure): the small
grid fixture in its orientations, the windows, and a picture counter.

The fixture: a grid of 4 x 3 tiles of 64 x 64 (CTB 16: 4 WPP rows per tile),
output 250 x 180 (the last column and row are cropped), 4:2:0, 8 bits.
"""
import ctypes
import functools

import numpy as np

import display_ref
from heif_amd import _lib
import heif_amd.synth_encoder as S

W, H, TILE = 250, 180, 64
PARAMS = S.SynthParams(width=TILE, height=TILE, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=2)
SEED = 11

# an odd crop: left 5, top 3, 201 x 151 (offsets -39/2 and -23/2 from the centred position)
CLAP_FIELDS = (201, 1, 151, 1, -39, 2, -23, 2)
CLAP = (5, 3, 201, 151)  # left, top, width, height

# (name, steps in display_ref's form): irot 0..3, each with and without imir 0, and
# one with the odd clap in front
ORIENTATIONS = []
for _k in range(4):
    ORIENTATIONS.append((f"rot{_k}", (("irot", _k),) if _k else ()))
    ORIENTATIONS.append((f"rot{_k}_mir", (("irot", _k), ("imir", 0))))
EIGHT = [n for n, _ in ORIENTATIONS]
ORIENTATIONS.append(("clap_rot1_mir", (("clap", CLAP_FIELDS), ("irot", 1), ("imir", 0))))
# a clap of a window's size, so that the plain render reads four tiles: img[60:70, 60:70], turned
CLAP_SMALL = (60, 60, 10, 10)
VARIANTS = dict(ORIENTATIONS)
VARIANTS["clap_small_rot3"] = (("clap", (10, 1, 10, 1, -60, 1, -25, 1)), ("irot", 3))


def boxes(steps):
    out = []
    for kind, arg in steps:
        out.append({"clap": lambda a: S.clap_box(*a), "irot": S.irot_box, "imir": S.imir_box}[kind](arg))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixture(name: str, aux: bool = False) -> bytes:
    """The fixture in orientation `name`; aux: with a 4:0:0 alpha image on
    another grid (2 x 2 tiles of 128 x 96)."""
    extra = ()
    if aux:
        extra = (S.AuxImage(S.SynthParams(width=128, height=96, chroma_format=0), seed=5),)
    return S.grid_heic(W, H, PARAMS, seed=SEED, transforms=boxes(VARIANTS[name]), aux=extra)


# windows in the coordinates of the untransformed picture, and the tiles each reads
SOURCE_WINDOWS = [(64, 64, 64, 64), (60, 60, 10, 10), (63, 64, 2, 1), (249, 179, 1, 1)]
SOURCE_WINDOW_TILES = {(64, 64, 64, 64): 1, (60, 60, 10, 10): 4, (63, 64, 2, 1): 2, (249, 179, 1, 1): 1}


def displayed_window(steps, src_window):
    """Where the pixels of src_window (source coordinates) are shown: their
    bounding box in displayed coordinates, None if the transforms hide them all
    (or for src_window None: the whole picture)."""
    if src_window is None:
        return None
    ys, xs = np.mgrid[0:H, 0:W]
    tx, ty = display_ref.apply_transforms(xs, steps), display_ref.apply_transforms(ys, steps)
    x, y, w, h = src_window
    oy, ox = np.nonzero((tx >= x) & (tx < x + w) & (ty >= y) & (ty < y + h))
    if not len(ox):
        return None
    return (int(ox.min()), int(oy.min()), int(ox.max() - ox.min() + 1), int(oy.max() - oy.min() + 1))


def count_pictures(imgs, rects, opts=None) -> int:
    """heifgpu_batch_count_pictures: rects None, or one (x, y, w, h) / None per image."""
    n = len(imgs)
    arr = (ctypes.c_void_p * n)(*[im._h.value for im in imgs])
    src = None
    if rects is not None:
        src = (_lib.Rect * n)(*[_lib.Rect(*r) if r is not None else _lib.Rect() for r in rects])
    v = ctypes.c_uint32()
    _lib.check(_lib.lib.heifgpu_batch_count_pictures(arr, n, ctypes.byref(opts) if opts is not None else None, src,
                                                     ctypes.byref(v)))
    return v.value
