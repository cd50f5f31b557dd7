"""Cases for k_ycbcr_rgb (heifgpu_ycbcr_to_rgb) and k_gather_tiles (heifgpu_gather_tiles)
run alone on fabricated planes, and what each case must hold afterwards.

Every device buffer is laid out here, on the host, as bytes: GUARD sentinel bytes, the
payload (a base offset, then rows of `pitch` bytes), GUARD sentinel bytes.  The pointer
a kernel gets is buffer + GUARD + offset, so the expected buffer, guards and row padding
included, is compared whole.  The buffers start 16-aligned (test_rgb_gather_gpu asserts
it), so the path a store or a copy takes follows from the offsets and pitches alone:
rgb_rows() and gather_chunks() count them for test_rgb_gather.py, which keeps these
lists from going soft.

Samples are uniform draws from [0, 1 << depth), seeded from the case's name; a draw
whose values do not reach both ends of every channel is drawn again from the same stream.
"""
import functools
import zlib
from collections import Counter, namedtuple
from types import SimpleNamespace

import numpy as np

import gather_ref
import rgb_ref

GUARD = 256
SENTINEL = 0xA5


def rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def framed(payload: int):
    """A buffer of `payload` bytes between its guard bands, all sentinel."""
    return np.full(GUARD + payload + GUARD, SENTINEL, np.uint8)


def rows_of(buf, offset: int, rows: int, pitch: int):
    """The (rows, pitch) view of the plane that starts `offset` bytes into buf's payload."""
    return buf[GUARD + offset:GUARD + offset + rows * pitch].reshape(rows, pitch)


def sample_bytes(a):
    """(h, w) samples as (h, w * bytes per sample) bytes."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


# ---- k_ycbcr_rgb -----------------------------------------------------------------------------
RgbCase = namedtuple("RgbCase", "name w h rot chroma depth matrix full pad off src_pad")

SHAPES = [(1, 1), (5, 3), (8, 8), (37, 22), (64, 48), (1030, 6)]
MATRIX_RANGE = [(m, full) for m in (1, 2, 6, 9) for full in (False, True)]
DEPTHS = (8, 9, 10, 11, 12, 16)
RGB_PAD = 5  # the padded rgb_pitch is 3 * out_w + RGB_PAD: the rows' alignment walks through 0..3


def rgb_case(w, h, rot, chroma, depth, matrix, full, pad, off, src_pad):
    name = f"{w}x{h}_r{rot}_c{chroma}_d{depth}_m{matrix}{'f' if full else 'l'}_p{pad}_o{off}_s{src_pad}"
    return RgbCase(name, w, h, rot, chroma, depth, matrix, full, pad, off, src_pad)


def _rgb_cases():
    out = {}
    # every shape x rotation x chroma format at 8 and 10 bits.  The eight (chroma, depth) pairs of a
    # (shape, rotation) take the eight (matrix, range) pairs, both pitches and the four offsets.
    for si, (w, h) in enumerate(SHAPES):
        for rot in range(4):
            for chroma in range(4):
                for di, depth in enumerate((8, 10)):
                    matrix, full = MATRIX_RANGE[(2 * chroma + di + si + rot) % 8]
                    c = rgb_case(w, h, rot, chroma, depth, matrix, full, RGB_PAD * ((chroma + di + si) & 1),
                                  (chroma + 2 * di + rot + si) % 4, (chroma + di + rot) & 1)
                    out[c.name] = c
    # 37 x 22 turned by 90 degrees: every depth x matrix x range, without and with chroma
    n = 0
    for depth in DEPTHS:
        for matrix, full in MATRIX_RANGE:
            for chroma in (0, 1, 3):
                c = rgb_case(37, 22, 1, chroma, depth, matrix, full, RGB_PAD * (n & 1), (n >> 1) % 4, int(n % 3 != 0))
                out.setdefault(c.name, c)
                n += 1
    return list(out.values())


RGB_CASES = _rgb_cases()


def rgb_bps(c) -> int:
    return 1 if c.depth == 8 else 2


def rgb_out_dims(c):
    return (c.h, c.w) if c.rot & 1 else (c.w, c.h)


def rgb_pitch(c) -> int:
    return 3 * rgb_out_dims(c)[0] + c.pad


def rgb_plane_dims(c, k: int):
    sx, sy = gather_ref.SUB[c.chroma] if k else (0, 0)
    return (c.w + (1 << sx) - 1) >> sx, (c.h + (1 << sy) - 1) >> sy


def rgb_src_pitch(c, k: int) -> int:
    """Bytes per row of source plane k: tight, or 3 + k samples of padding (Cb and Cr then differ)."""
    return (rgb_plane_dims(c, k)[0] + (3 + k if c.src_pad else 0)) * rgb_bps(c)


@functools.lru_cache(maxsize=None)
def rgb_samples(c):
    """(y, cb, cr): uint8 or uint16 samples below 1 << depth; cb = cr = None for 4:0:0."""
    r = rng(c.name)
    dt = np.uint8 if rgb_bps(c) == 1 else np.uint16
    for _ in range(64):
        out = []
        for k in range(3 if c.chroma else 1):
            pw, ph = rgb_plane_dims(c, k)
            out.append(r.integers(0, 1 << c.depth, size=(ph, pw)).astype(dt))
        out += [None] * (3 - len(out))
        if (c.w, c.h) in GEOMETRY_ONLY or _clips_both_ways(c, out):
            break  # (nearly always the first draw; an 8 x 8 plane now and then misses an end)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return tuple(out)


GEOMETRY_ONLY = ((1, 1), (5, 3))  # too few samples to promise values at both ends


def _clips_both_ways(c, planes) -> bool:
    """What test_rgb_gather.py asks of a case's values: each of R, G, B below 0 somewhere and
    above 255 somewhere, and a pixel with all three inside (4:0:0: both ends in limited
    range, where they exist).  The draw is repeated from the same stream until it holds."""
    u = rgb_ref.unclipped(planes[0], planes[1], planes[2], c.matrix, c.full, c.depth)
    if not c.chroma:
        return c.full or bool((u < 0).any() and (u > 255).any())
    ends = all((u[..., ch] < 0).any() and (u[..., ch] > 255).any() for ch in range(3))
    return ends and bool(((u >= 0) & (u <= 255)).all(axis=-1).any())


def rgb_source(c, k: int):
    """Plane k's whole buffer (guards, padded rows), as the device gets it."""
    a = rgb_samples(c)[k]
    pitch = rgb_src_pitch(c, k)
    buf = framed(a.shape[0] * pitch)
    b = sample_bytes(a)
    rows_of(buf, 0, a.shape[0], pitch)[:, :b.shape[1]] = b
    return buf


def rgb_unclipped(c):
    y, cb, cr = rgb_samples(c)
    return rgb_ref.unclipped(y, cb, cr, c.matrix, c.full, c.depth)


@functools.lru_cache(maxsize=None)
def rgb_expected(c):
    """The whole output buffer after the call."""
    y, cb, cr = rgb_samples(c)
    want = rgb_ref.ycbcr_to_rgb(y, cb, cr, c.matrix, c.full, c.rot, c.depth)
    ow, oh = rgb_out_dims(c)
    assert want.shape == (oh, ow, 3)
    pitch = rgb_pitch(c)
    buf = rgb_blank(c)
    for oy in range(oh):  # the last row ends at its last pixel: nothing is owed beyond it
        o = GUARD + c.off + oy * pitch
        buf[o:o + 3 * ow] = want[oy].reshape(-1)
    buf.setflags(write=False)
    return buf


def rgb_blank(c):
    """The output buffer before the call: the last row has its padding too, then the guard."""
    return framed(c.off + rgb_out_dims(c)[1] * rgb_pitch(c))


def rgb_rows(c) -> Counter:
    """How the kernel's groups of four pixels along a row fall: full groups on rows whose
    address is 4-aligned (three dword stores) and on the others (byte stores), partial
    groups by size, and the longest row in groups."""
    ow, oh = rgb_out_dims(c)
    n = Counter()
    for oy in range(oh):
        aligned = ((c.off + oy * rgb_pitch(c)) & 3) == 0  # a group starts 12 bytes after the one before
        n["full_aligned" if aligned else "full_unaligned"] += ow // 4
        if ow % 4:
            n[f"partial{ow % 4}"] += 1
    n["groups_per_row"] = (ow + 3) // 4
    return n


# ---- k_gather_tiles --------------------------------------------------------------------------
GatherCase = namedtuple("GatherCase", "name W H chroma bps tw th cols rows dpitch spitch doff pairs")

EVERY = ((1, 0), (0, 0), (2, 0), (2, 1))


def _tight(W, H, chroma, bps):
    info = SimpleNamespace(width=W, height=H, chroma_format_idc=chroma)
    return tuple(gather_ref.plane_dims(info, c)[0] * bps for c in range(3 if chroma else 1))


GATHER_CASES = [
    GatherCase("grid420_8", 300, 200, 1, 1, 128, 96, 3, 3, _tight(300, 200, 1, 1), _tight(300, 200, 1, 1), 0,
               ((1, 0), (2, 0), (2, 1), (4, 3), (16, 3), (16, 9), (0, 0))),
    GatherCase("grid422_16", 300, 200, 2, 2, 128, 96, 3, 3, (608, 304, 304), (640, 320, 320), 0, EVERY),
    GatherCase("unaligned_x0", 200, 60, 3, 1, 72, 20, 3, 3, (208, 208, 208), (224, 224, 224), 0, EVERY),
    GatherCase("mono", 130, 70, 0, 2, 64, 64, 3, 2, _tight(130, 70, 0, 2), _tight(130, 70, 0, 2), 0, EVERY),
    GatherCase("wide", 2300, 10, 1, 1, 1150, 6, 2, 2, (2304, 1152, 1152), (2320, 1168, 1168), 0, EVERY + ((4, 3),)),
    GatherCase("odd_nogrid", 37, 23, 1, 1, 0, 0, 0, 0, _tight(37, 23, 1, 1), _tight(37, 23, 1, 1), 0, EVERY),
    GatherCase("beyond", 100, 40, 1, 1, 64, 32, 3, 2, _tight(100, 40, 1, 1), _tight(100, 40, 1, 1), 0,
               EVERY + ((3, 2), (6, 5))),
    GatherCase("dst_off3", 300, 200, 1, 1, 128, 96, 3, 3, (304, 160, 160), (304, 160, 160), 3, EVERY),
]
GATHER_BY_NAME = {c.name: c for c in GATHER_CASES}


def gather_info(c):
    """heifgpu_image_info's fields of the case (the ones the gather reads, and the depth)."""
    return SimpleNamespace(width=c.W, height=c.H, chroma_format_idc=c.chroma, bit_depth=8 if c.bps == 1 else 10,
                           bytes_per_sample=c.bps, grid_rows=c.rows, grid_cols=c.cols, tile_width=c.tw,
                           tile_height=c.th, num_tiles=c.cols * c.rows)


def gather_planes(c) -> int:
    return 3 if c.chroma else 1


def gather_rows(c, k: int) -> int:
    return gather_ref.plane_dims(gather_info(c), k)[1]


@functools.lru_cache(maxsize=None)
def gather_sources(c):
    """The source buffers: random bytes between the guards, one per plane."""
    r = rng(c.name)
    out = []
    for k in range(gather_planes(c)):
        buf = framed(gather_rows(c, k) * c.spitch[k])
        buf[GUARD:-GUARD] = r.integers(0, 256, size=buf.size - 2 * GUARD, dtype=np.uint8)  # padding too: never copied
        buf.setflags(write=False)
        out.append(buf)
    return tuple(out)


def gather_blank(c, k: int):
    """Destination buffer k before a call."""
    return framed(c.doff + gather_rows(c, k) * c.dpitch[k])


def gather_expected(c, stride: int, offset: int):
    """The destination buffers after gather(stride, offset) into blank ones."""
    src = [rows_of(b, 0, gather_rows(c, k), c.spitch[k]) for k, b in enumerate(gather_sources(c))]
    bufs = [gather_blank(c, k) for k in range(gather_planes(c))]
    dst = [rows_of(b, c.doff, gather_rows(c, k), c.dpitch[k]) for k, b in enumerate(bufs)]
    for view, plane in zip(dst, gather_ref.gather(dst, src, gather_info(c), stride, offset)):
        view[...] = plane
    return bufs


def gather_chunks(c, stride: int, offset: int) -> Counter:
    """How the kernel's 16-byte chunks of every copied row fall, from the addresses: a row
    whose source and destination are both 16-aligned moves whole chunks as vectors and a
    shorter last chunk by bytes; any other row goes by bytes throughout.  "second_step"
    counts chunks 1024 bytes or more into a row (the 64 lanes' second turn), "skipped"
    the (tile, plane) pairs without a window."""
    info = gather_info(c)
    n = Counter()
    for k in gather_ref.selected(info, stride, offset):
        for p in range(gather_planes(c)):
            win = gather_ref.window(info, k, p)
            if win is None:
                n["skipped"] += 1
                continue
            x0, y0, w, h = win
            wb = w * c.bps
            for y in range(y0, y0 + h):
                s, d = y * c.spitch[p] + x0 * c.bps, c.doff + y * c.dpitch[p] + x0 * c.bps
                aligned = ((s | d) & 15) == 0
                for o in range(0, wb, 16):
                    n["vector" if aligned and o + 16 <= wb else "tail" if aligned else "bytes"] += 1
                    n["second_step"] += o >= 1024
    return n
