"""The checker of the tensor render (test infrastructure): include/heifgpu.h's
formula over an integer picture R, in numpy float32, compared by bit pattern.

    F = float32(float32(float32(Rf) * a[c]) + b[c])      two roundings, no fused multiply-add
    Rf = R with columns reversed if flip & 1, rows reversed if flip & 2

numpy rounds every float32 operation on its own, so the product and the sum
are the two roundings of the definition.  binary16 is numpy's astype (round to
nearest even, gradual underflow, overflow to infinity); bfloat16, which numpy
lacks, is round to nearest even on the uint32 view of the float32.

R comes from scale_ref.area_average(display_ref.render(...)): nothing here
shares code with the library.  Like those two it is "parity unpinned": nothing
at hand renders a HEIC into a normalised tensor to compare with.
"""
import numpy as np

ELEMS = ("f32", "f16", "bf16")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def constants(mean, std, maxv):
    """a = float32(1 / (maxv * std)), b = float32(-mean / std): derived in double, rounded once."""
    a = np.array([1.0 / (float(maxv) * float(s)) for s in std], np.float64).astype(np.float32)
    b = np.array([-float(m) / float(s) for m, s in zip(mean, std)], np.float64).astype(np.float32)
    return a, b


def bf16_bits(f: np.ndarray) -> np.ndarray:
    """float32 -> the bfloat16 bit patterns (uint16), round to nearest even; finite input."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def flipped(R: np.ndarray, flip: int) -> np.ndarray:
    if flip & 1:
        R = R[:, ::-1]
    if flip & 2:
        R = R[::-1]
    return R


def tensor(R: np.ndarray, a, b, elem: str = "f32", layout: str = "chw", flip: int = 0) -> np.ndarray:
    """The bit patterns the tensor render writes for the integer picture R
    (h, w, C): uint32 for "f32", uint16 for "f16" / "bf16", shaped (C, h, w) for
    "chw" and (h, w, C) for "hwc"."""
    C = R.shape[2]
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == (C,) and b.shape == (C,) and np.isfinite(a).all() and np.isfinite(b).all()
    x = flipped(R, flip).astype(np.float32)  # exact: R < 2^24
    assert int(R.max(initial=0)) < 1 << 24
    prod = x * a[None, None, :]
    assert prod.dtype == np.float32
    F = prod + b[None, None, :]
    assert F.dtype == np.float32
    if elem == "f32":
        bits = np.ascontiguousarray(F).view(np.uint32)
    elif elem == "f16":
        with np.errstate(over="ignore"):
            bits = np.ascontiguousarray(F.astype(np.float16)).view(np.uint16)
    elif elem == "bf16":
        bits = bf16_bits(F)
    else:
        raise ValueError(elem)
    return np.ascontiguousarray(bits.transpose(2, 0, 1)) if layout == "chw" else bits
