#!/usr/bin/env python3
"""Writes tests/golden/pillow_resize.npz: inputs, boxes and Pillow's own outputs
of Image.resize(size, BILINEAR | BICUBIC, box=) for a handful of small cases,
so that tests/resample_ref.py stays pinned to Pillow where Pillow is absent.

    python tools/make_resample_golden.py

Needs PIL.  Every channel is resized as an "L" image (nothing premultiplied).
The file holds the pictures pic_p (H, W, C) uint8, cases[k] = (x, y, w, h, ow,
oh, filter code 1 | 2, p), outs: Pillow's (oh, ow, C) uint8 results flattened one
after the other in the order of the cases, and `pillow`, the version that wrote it.
"""
import pathlib

import numpy as np
import PIL
from PIL import Image

ROOT = pathlib.Path(__file__).resolve().parent.parent
FILTERS = {1: Image.BILINEAR, 2: Image.BICUBIC}


def pictures():
    rng = np.random.default_rng(18)
    noise = rng.integers(0, 256, (29, 41, 1), dtype=np.uint8)
    noise[:14, :20] = rng.choice(np.array([0, 255], np.uint8), (14, 20, 1))  # hard edges: the overshoot clips
    yy, xx = np.mgrid[0:23, 0:31]
    blocks = ((((yy // 3) + (xx // 4)) & 1) * 255).astype(np.uint8)[..., None].repeat(2, axis=2)
    return [noise, blocks]


# (picture, window, (ow, oh)): reduction, enlargement, identity, 1 x 1, windows at every edge
CASES = [
    (0, (0, 0, 41, 29), (17, 11)), (0, (0, 0, 41, 29), (50, 37)), (0, (0, 0, 41, 29), (41, 29)),
    (0, (0, 0, 41, 29), (1, 1)), (0, (5, 3, 30, 20), (7, 20)), (0, (1, 2, 13, 9), (3, 2)),
    (0, (40, 28, 1, 1), (3, 2)), (0, (0, 0, 41, 7), (41, 5)), (0, (36, 0, 5, 29), (9, 9)),
    (1, (0, 0, 31, 23), (11, 7)), (1, (2, 1, 27, 20), (40, 33)),
]


def main():
    pics = pictures()
    data = {"pillow": np.array(PIL.__version__), **{f"pic_{p}": D for p, D in enumerate(pics)}}
    cases, outs = [], []
    for p, (x, y, w, h), (ow, oh) in CASES:
        D = pics[p]
        for code, filt in FILTERS.items():
            out = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(D[..., c])).resize(
                (ow, oh), filt, box=(x, y, x + w, y + h))) for c in range(D.shape[2])], axis=-1)
            assert out.shape == (oh, ow, D.shape[2]) and out.dtype == np.uint8
            cases.append([x, y, w, h, ow, oh, code, p])
            outs.append(out.ravel())
    data["cases"] = np.array(cases, np.int32)
    data["outs"] = np.concatenate(outs)
    path = ROOT / "tests" / "golden" / "pillow_resize.npz"
    np.savez_compressed(path, **data)
    print(f"{path}: {len(cases)} cases, {path.stat().st_size} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
