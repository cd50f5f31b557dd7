"""The PNG encoder's cases: fabricated pictures (and one crop of the golden HEIC's displayed
picture, rendered from the oracle's planes by display_ref), each with its format, options,
surface layout (row padding, an odd start address) and colour chunk, grouped into the batches
the kernels are driven with.  reference() is the model's file for a case, computed once per
process."""
import functools
import pathlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

import png_ref

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
FORMAT_CODES = {"rgb8": 0, "rgba8": 1, "rgb16": 2, "rgba16": 3}


@dataclass
class Case:
    name: str
    px: np.ndarray            # (h, w, C) uint8 or uint16
    fmt: str = "rgb8"
    bits: int = 8
    filt: int = png_ref.ADAPTIVE
    pad: int = 0              # bytes between rows
    lead: int = 0             # bytes before the first pixel in its buffer
    srgb: bool = False
    cicp: Optional[tuple] = None
    icc: Optional[bytes] = None
    photo: bool = False       # photo-like: its size is compared with zlib's Huffman-only coding

    @property
    def opts(self):
        return (self.fmt, self.bits, self.filt)

    @property
    def bpp(self):
        ch, wide = png_ref.FORMATS[self.fmt]
        return ch * (2 if wide else 1)


def noise(w, h, seed, ch=3, top=255):
    return np.random.default_rng(seed).integers(0, top + 1, (h, w, ch), dtype=np.uint16 if top > 255 else np.uint8)


def smooth(w, h, seed=0, ch=3, top=255):
    """Gradients under a little seeded noise."""
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(1000 + seed)
    base = np.stack([(3 * x + y + 17 * seed), (2 * y + x // 2), (x + 5 * y), (255 - x - y)][:ch], -1) * (top + 1) // 256
    return ((base + rng.integers(-2, 3, base.shape) * max(1, (top + 1) // 256)) % (top + 1)).astype(np.uint16 if top > 255 else np.uint8)


def fibonacci_picture():
    """199 x 48 rgb8 (28656 bytes) for filter 0, whose block's 21 symbols have Fibonacci counts:
    1 (symbol 256, which takes the place of the sequence's other 1), then 1, 2, 3, 5, ... 6765 for
    the values 19 down to 1, and the rest for value 0 (10947, and the 48 filter bytes: more than
    the 10946 of the sequence, which only keeps it last).  Every merge then joins the next leaf to
    the chain, and the unlimited code is 20 bits deep."""
    fib = [1, 2]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    assert fib[-1] == 6765 and sum(fib) == 17709
    counts = [199 * 48 * 3 - sum(fib)] + fib[::-1]
    vals = np.concatenate([np.full(c, v, np.uint8) for v, c in enumerate(counts)])
    return np.random.default_rng(3).permutation(vals).reshape(48, 199, 3)


def dyadic_picture():
    """10 x 1057 rgb8 for filter 0 (a stream of 32767 bytes): 177 values and symbol 256 with the
    counts 2^(15 - l) of a complete code that has 5, 11, 14, 10, 9, 0, 7, 1, 3, 0, 2, 116 codes of
    the lengths 4 .. 15, so these are the literal code's lengths; the numbers of codes of each
    length (and 80 zeros) then make a code-length code 8 bits deep, which the limit of 7 repairs."""
    per_len = {4: 5, 5: 11, 6: 14, 7: 10, 8: 9, 10: 7, 11: 1, 12: 3, 14: 2, 15: 116}
    lens = [l for l, k in sorted(per_len.items()) for _ in range(k)]
    assert sum(2 ** (15 - l) for l in lens) == 32768 and len(lens) == 178
    counts = [2 ** (15 - l) for l in lens[:-1]]  # (the last code of 15 bits is symbol 256's)
    counts[0] -= 1057                            # value 0: the filter bytes are among its 2048
    vals = np.concatenate([np.full(c, v, np.uint8) for v, c in enumerate(counts)])
    return np.random.default_rng(4).permutation(vals).reshape(1057, 10, 3)


def filter_rows_picture():
    """64 x 6 rgb8 whose rows are won by none (tied with up: there is no row above), sub, up
    (tied with Paeth), Paeth and average in turn, then a row of noise."""
    n = 192
    rng = np.random.default_rng(11)
    rows = [rng.choice(np.array([0, 1, 255], np.uint8), n)]      # small magnitudes as they are
    rows.append(((7 * (np.arange(n) // 3) + 3) % 256).astype(np.uint8))  # a horizontal ramp: constant differences
    rows.append(rows[1].copy())                                    # the row above again
    r3 = rows[2].copy()                                            # follows the row above, then the pixel before
    r3[n // 2:] = 200
    rows.append(r3)
    r4 = np.zeros(n, np.int32)                                     # the mean of left and above
    for i in range(n):
        r4[i] = ((r4[i - 3] if i >= 3 else 0) + int(r3[i])) >> 1
    rows.append(r4.astype(np.uint8))
    rows.append(rng.integers(0, 256, n, dtype=np.uint8))
    return np.stack(rows).reshape(6, 64, 3)


@functools.lru_cache(maxsize=None)
def photo_crop(w=512, h=384, x0=1200, y0=1800):
    """A w x h crop at (x0, y0) of halfmoonbay's displayed picture: the oracle's planes through
    display_ref (only the part of the planes the crop reads is converted)."""
    import display_ref
    import heif_amd as H
    from oracle import oracle

    data = (GOLDEN / "halfmoonbay.heic").read_bytes()
    img = H.HeifImage.parse(data)
    o = oracle.decode_heic(data, with_checks=False)
    d, inf = img.display, img.info
    oy, ox = np.mgrid[y0:y0 + h, x0:x0 + w]
    sy, sx = d.m[2] * ox + d.m[3] * oy + d.t[1], d.m[0] * ox + d.m[1] * oy + d.t[0]
    ya, yb, xa, xb = sy.min() & ~1, sy.max() + 1, sx.min() & ~1, sx.max() + 1
    sub_h, sub_w = o.y.shape[0] // o.cb.shape[0], o.y.shape[1] // o.cb.shape[1]
    assert (sub_h, sub_w) == (2, 2)
    part = display_ref.render(o.y[ya:yb, xa:xb], o.cb[ya // 2:(yb + 1) // 2, xa // 2:(xb + 1) // 2],
                              o.cr[ya // 2:(yb + 1) // 2, xa // 2:(xb + 1) // 2], inf.matrix_coeffs, bool(inf.full_range),
                              inf.bit_depth, [], "rgb8")
    return np.ascontiguousarray(part[sy - ya, sx - xa])


def build_cases():
    cases = [
        # the smallest pictures
        Case("one_rgb8", noise(1, 1, 1)),
        Case("one_rgba16_b10", noise(1, 1, 2, 4, 1023), "rgba16", 10),
        Case("odd_5x3", smooth(5, 3, 2), pad=13, lead=1),
        # filtered streams of 32767, 32768 and 32769 bytes, and of two full blocks and four bytes
        Case("stream_32767", smooth(10, 1057, 3)),
        Case("stream_32768", noise(21, 512, 4)),
        Case("stream_32769", smooth(110, 99, 5), lead=3),
        Case("stream_65540", smooth(193, 113, 6), pad=1),
        # chosen bytes through filter 0
        Case("zeros", np.zeros((8, 16, 3), np.uint8), filt=0),
        Case("ramp256", np.tile(np.arange(256, dtype=np.uint8), 4).reshape(4, 64, 4), "rgba8", filt=0),
        Case("fibonacci", fibonacci_picture(), filt=0),
        Case("dyadic", dyadic_picture(), filt=0),
        # every filter type as an adaptive choice, and each forced
        Case("filter_rows", filter_rows_picture()),
    ]
    for t in range(1, 5):
        cases.append(Case(f"forced_{t}", smooth(23, 9, 10 + t, 4), "rgba8", filt=t, pad=t))
    cases += [
        # sixteen bits
        Case("rgb16_b12", smooth(37, 11, 7, 3, 4095), "rgb16", 12, pad=2),
        Case("rgba16_b16", noise(9, 14, 8, 4, 65535), "rgba16", 16, lead=2),
        Case("rgba16_b8", smooth(6, 4, 9, 4, 255).astype(np.uint16), "rgba16", 8),
        # the colour chunks
        Case("srgb", smooth(12, 7, 12), srgb=True),
        Case("cicp_pq", smooth(12, 7, 13, 3, 1023), "rgb16", 10, cicp=(9, 16, 0, 1)),
        Case("icc_70k", smooth(12, 7, 14), icc=np.random.default_rng(9).integers(0, 256, 70_000, dtype=np.uint8).tobytes()),
        # photo-like
        Case("photo", photo_crop(), photo=True),
        Case("photo_rgba", np.concatenate([photo_crop()[:96, :128], smooth(128, 96, 15, 1)], -1), "rgba8", photo=True),
    ]
    # a batch of three pictures of different sizes, one set of options
    for n, (w, h) in enumerate([(260, 40), (19, 50), (64, 16)]):
        cases.append(Case(f"mixed_{n}", noise(w, h, 50 + n) if n == 1 else smooth(w, h, n), pad=(13, 0, 1)[n], lead=(1, 0, 0)[n]))
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
# the batches: the mixed three together, every other picture alone
BATCHES = [[c for c in CASES if c.name.startswith("mixed_")]] + [[c] for c in CASES if not c.name.startswith("mixed_")]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the model's file, its header's length, the model's facts) of a case; the facts are
    {"types": the rows' filter types, "ties": the rows two types tie on, "blocks": per block {"repair15", "repair7", "distinct",
    "lit"}, "stream": the filtered bytes}."""
    c = BY_NAME[name]
    facts = []
    h, w, _ = c.px.shape
    head = png_ref.header(w, h, c.fmt, c.bits, c.srgb, c.cicp, c.icc)
    return head + png_ref.body(c.px, c.fmt, c.bits, c.filt, facts), len(head), facts[0]


def surface(c):
    """(buffer bytes, pitch): the case's picture laid out with its row padding behind `lead`
    bytes, everything that is not a pixel filled with 0xA5."""
    h, w, _ = c.px.shape
    row = w * c.bpp
    pitch = row + c.pad
    raw = np.ascontiguousarray(c.px.astype("<u2" if c.px.dtype == np.uint16 else np.uint8)).view(np.uint8).reshape(h, row)
    buf = np.full(c.lead + (h - 1) * pitch + row, 0xA5, np.uint8)
    for y in range(h):
        buf[c.lead + y * pitch: c.lead + y * pitch + row] = raw[y]
    return buf, pitch
