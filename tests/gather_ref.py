"""numpy restatement of heifgpu_gather_tiles (test infrastructure).

The geometry is the one include/heifgpu.h gives a grid image: plane c of a W x H
picture is ceil(W / SubWidthC) x ceil(H / SubHeightC) samples, grid tile k (row-major,
grid_cols per row) starts at luma (col * tile_width, row * tile_height), a chroma
window at that origin shifted down by the subsampling and ends at the tile's far edge
rounded up the same way, and every window is clipped to the plane.  A tile whose origin lies beyond the plane (the grid's canvas is larger
than the cropped picture) has no window and is skipped.  An image without a grid
(tile_width == 0, num_tiles == 0) is one tile, the whole picture.  The tiles k with
k % stride == offset are copied; stride 0 means 1.

Planes are 2-D uint8 arrays of shape (rows, pitch): bytes, not samples, so the row
padding is part of what is compared.  `info` is anything with heifgpu_image_info's
field names (the ctypes structure, or a SimpleNamespace).
"""
import numpy as np

SUB = ((0, 0), (1, 1), (1, 0), (0, 0))  # chroma_format_idc -> log2 (SubWidthC, SubHeightC)


def planes(info) -> int:
    return 3 if info.chroma_format_idc else 1


def plane_dims(info, c: int):
    """(width, height) of plane c in samples."""
    sx, sy = SUB[info.chroma_format_idc] if c else (0, 0)
    return (info.width + (1 << sx) - 1) >> sx, (info.height + (1 << sy) - 1) >> sy


def tiles(info) -> int:
    return max(1, info.num_tiles)


def window(info, k: int, c: int):
    """(x0, y0, w, h) in samples of grid tile k in plane c, or None for a skipped tile."""
    sx, sy = SUB[info.chroma_format_idc] if c else (0, 0)
    pw, ph = plane_dims(info, c)
    cols = max(1, info.grid_cols)
    tw, th = info.tile_width or info.width, info.tile_height or info.height
    tx, ty = (k % cols) * tw, (k // cols) * th  # the tile's luma origin
    x0, y0 = tx >> sx, ty >> sy
    if x0 >= pw or y0 >= ph:
        return None
    # the tile's far edge rounds up, as the plane's does: a 37 x 23 picture's only tile has 19 x 12 chroma
    x1, y1 = min((tx + tw + (1 << sx) - 1) >> sx, pw), min((ty + th + (1 << sy) - 1) >> sy, ph)
    return x0, y0, x1 - x0, y1 - y0


def selected(info, stride: int, offset: int):
    stride = stride or 1
    if offset >= stride:
        raise ValueError("tile_offset must be below tile_stride")
    return list(range(offset, tiles(info), stride))


def gather(dst_bytes, src_bytes, info, stride: int, offset: int):
    """The planes dst must hold after the call: copies of dst_bytes with the selected
    tiles' windows taken from src_bytes; every other byte as it was."""
    bps = info.bytes_per_sample
    out = [None if d is None else np.array(d, dtype=np.uint8, copy=True) for d in dst_bytes]
    for k in selected(info, stride, offset):
        for c in range(planes(info)):
            win = window(info, k, c)
            if win is None:
                continue
            x0, y0, w, h = win
            out[c][y0:y0 + h, x0 * bps:(x0 + w) * bps] = src_bytes[c][y0:y0 + h, x0 * bps:(x0 + w) * bps]
    return out
