"""The JPEG encoder's cases: fabricated RGB arrays only (no decode is needed to test an
encoder), each with its options, its surface layout (row padding, an odd start address) and
an optional ICC profile, grouped into the batches the kernels are driven with.  reference()
is the numpy model's file for a case, computed once per process."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

import jpeg_ref

SIZES = [(1, 1), (8, 8), (16, 16), (17, 9), (33, 31), (47, 33), (130, 18)]  # width, height
SUBS = ("4:4:4", "4:2:0")


@dataclass
class Case:
    name: str
    rgb: np.ndarray           # (h, w, 3) uint8
    quality: int = 90
    sub: str = "4:2:0"
    restart: int = 0
    pad: int = 0              # bytes between rows
    lead: int = 0             # bytes before the first pixel in its buffer
    icc: Optional[bytes] = None

    @property
    def opts(self):
        return (self.quality, self.sub, self.restart)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(w, h, seed=0):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(3 * x + y + 17 * seed) % 256, (2 * y + x // 2) % 256, (x + 5 * y) % 256], -1).astype(np.uint8)


def grey_blocks(blocks):
    """A grey picture of 8 x 8 blocks side by side, each given as {natural index: coefficient
    of the orthonormal DCT of (p - 128)}."""
    from scipy.fft import idctn

    out = []
    for coefs in blocks:
        c = np.zeros(64)
        for k, v in coefs.items():
            c[k] = v
        out.append(np.clip(np.rint(idctn(c.reshape(8, 8), norm="ortho") + 128), 0, 255))
    g = np.concatenate(out, axis=1).astype(np.uint8)
    return np.repeat(g[..., None], 3, axis=2)


def sign_block(u, v):
    """0 / 255 by the sign of basis function (v, u): the largest coefficient a block can have there."""
    k = np.arange(8)
    bu, bv = np.cos((2 * k + 1) * u * np.pi / 16), np.cos((2 * k + 1) * v * np.pi / 16)
    g = np.where(np.outer(bv, bu) >= 0, 255, 0).astype(np.uint8)
    return np.repeat(g[..., None], 3, axis=2)


def first_seed(build, want, limit=200):
    """The first seed whose case's model statistics satisfy `want`."""
    for seed in range(limit):
        c = build(seed)
        st = {}
        jpeg_ref.scan(c.rgb, c.quality, c.sub, c.restart, st)
        if want(st):
            return c
    raise AssertionError("no seed found")


def build_cases():
    cases = []
    # every size in both subsamplings; pitch, start address, quality and restart interval vary along
    for i, (w, h) in enumerate(SIZES):
        for j, sub in enumerate(SUBS):
            k = 2 * i + j
            cases.append(Case(f"size_{w}x{h}_{sub}", noise(w, h, k) if k % 3 else smooth(w, h, k),
                              quality=(1, 50, 75, 100)[k % 4], sub=sub, restart=(0, 1, 3)[k % 3],
                              pad=(0, 1, 13)[(k // 2) % 3], lead=k % 2))
    # block contents that force specific paths
    zrl = grey_blocks([{0: 200, 58: 300}, {0: -100, 63: 250, 20: -120}])
    cases.append(Case("zrl_run", zrl, quality=50, sub="4:4:4"))
    cases.append(Case("last_coef", noise(16, 8, 5), quality=100, sub="4:4:4"))             # no EOB
    cases.append(Case("flat", np.full((16, 16, 3), 77, np.uint8), quality=75, sub="4:2:0"))  # all-zero AC
    bw = np.zeros((8, 16, 3), np.uint8)
    bw[:, 8:] = 255
    cases.append(Case("dc_cat11", bw, quality=100, sub="4:4:4"))
    cases.append(Case("ac_cat10", sign_block(1, 0), quality=100, sub="4:4:4"))
    cases.append(first_seed(lambda s: Case("stuffing", noise(24, 16, 100 + s), quality=90, sub="4:2:0", restart=1),
                            lambda st: st["stuffed"] > 0))
    cases.append(first_seed(lambda s: Case("aligned_end", noise(40, 24, 300 + s), quality=75, sub="4:4:4", restart=1),
                            lambda st: st["aligned"] > 0 and st["intervals"] > 8))
    # profiles: one chunk, and 200 KB in four
    rng = np.random.default_rng(9)
    cases.append(Case("icc_small", smooth(20, 12, 3), icc=rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()))
    cases.append(Case("icc_200k", smooth(9, 20, 4), sub="4:4:4", icc=rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()))
    # a batch of three pictures of different sizes, one set of options
    for n, (w, h) in enumerate([(260, 40), (19, 50), (64, 16)]):
        cases.append(Case(f"mixed_{n}", noise(w, h, 50 + n) if n else smooth(w, h, 1), quality=75, sub="4:2:0", restart=3,
                          pad=(13, 0, 1)[n], lead=(1, 0, 0)[n]))
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
# the batches: the mixed three together, every other picture alone
BATCHES = [[c for c in CASES if c.name.startswith("mixed_")]] + [[c] for c in CASES if not c.name.startswith("mixed_")]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the model's file, its header's length, the scan's statistics) of a case."""
    c = BY_NAME[name]
    st = {}
    h, w, _ = c.rgb.shape
    head = jpeg_ref.header(w, h, c.quality, c.sub, c.restart, c.icc)
    return head + jpeg_ref.scan(c.rgb, c.quality, c.sub, c.restart, st), len(head), st


def surface(c):
    """(buffer bytes, pitch): the case's picture laid out with its row padding behind `lead`
    bytes, everything that is not a pixel filled with 0xA5."""
    h, w, _ = c.rgb.shape
    pitch = 3 * w + c.pad
    buf = np.full(c.lead + (h - 1) * pitch + 3 * w, 0xA5, np.uint8)
    for y in range(h):
        buf[c.lead + y * pitch: c.lead + y * pitch + 3 * w] = c.rgb[y].reshape(-1)
    return buf, pitch
