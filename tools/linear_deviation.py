"""How far the encoded average of the scaled renders lies from the average in linear light.

    python tools/linear_deviation.py [--out deviation.json]

render_scaled(colorspace=X) averages the gamma-coded R'G'B' integers and transforms the rounded
average; render_scaled(colorspace=X, linear=True) decodes every source pixel to linear light
first (include/heifgpu.h "Linear-light scaled render").  This tool measures the difference in
codes, max and mean over all samples, on two pictures at 8 bits:
  halfmoonbay   tests/golden/halfmoonbay.heic, 4032 x 3024 decoded by the reference decoder
                (oracle/), its Display P3 profile to sRGB, cover to 224 x 224 (a 3024 x 3024
                window, 13.5 : 1);
  checkerboard  a full-range black / white pixel-pitch checkerboard 64 x 64 -> 32 x 32 through
                the identity sRGB transform: the worst case, 128 against 188.
Both on the CPU: the encoded rule is tests/scale_ref.py and tests/color_ref.py, the linear one is
the library's heifgpu_linear_average_apply, which runs the functions the kernel runs.  It needs
no device.  Information for callers; nothing is gated.
"""
import argparse
import ctypes
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import color_ref  # noqa: E402
import display_ref  # noqa: E402
import heif_amd as H  # noqa: E402
import scale_ref  # noqa: E402
from heif_amd import _lib, synth_encoder as S  # noqa: E402

ROWS = 256  # decoded rows per strip (the int64 temporaries of a whole picture are gigabytes)


def linear_average(t, D, window, ow, oh):
    src = np.ascontiguousarray(D, np.uint16)
    out = np.empty((oh, ow, 3), np.uint16)
    u16p = ctypes.POINTER(ctypes.c_uint16)
    _lib.check(_lib.lib.heifgpu_linear_average_apply(ctypes.byref(t), src.ctypes.data_as(u16p), src.shape[1], src.shape[0], 3,
                                                     ctypes.byref(_lib.Rect(*window)), ow, oh, out.ctypes.data_as(u16p)))
    return out.astype(np.int64)


def deviation(t, D, window, ow, oh):
    enc = color_ref.apply(t, scale_ref.area_average(D, window, ow, oh))
    lin = linear_average(t, D, window, ow, oh)
    d = np.abs(enc - lin)
    return {"from": [window[2], window[3]], "to": [ow, oh], "samples": int(d.size), "max": int(d.max()),
            "mean": round(float(d.mean()), 3), "p99": round(float(np.percentile(d, 99)), 2),
            "linear_minus_encoded_mean": round(float((lin - enc).mean()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from oracle import oracle

    data = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    img = H.HeifImage.parse(data)
    o = oracle.decode_heic(data, with_checks=False)
    Hh, W = o.y.shape
    D = np.empty((Hh, W, 3), np.uint16)
    for r0 in range(0, Hh, ROWS):
        rs = slice(r0, min(r0 + ROWS, Hh))
        rows, cols = (np.arange(rs.start, rs.stop) >> 1)[:, None], (np.arange(W) >> 1)[None, :]
        D[rs] = display_ref.rgb_at_depth(o.y[rs], o.cb[rows, cols], o.cr[rows, cols], img.info.matrix_coeffs,
                                         bool(img.info.full_range), 8)
    ow, oh, x, y, w, h = scale_ref.fit(W, Hh, 224, 224, "cover")
    result = {"bits": 8, "halfmoonbay": dict(transform="Display P3 profile -> sRGB",
                                             **deviation(img.color_transform("srgb", 8), D, (x, y, w, h), ow, oh))}
    srgb = H.HeifImage.parse(S.display_heic(S.SynthParams(width=16, height=16), colr=S.nclx_box(1, 13, 1, False)))
    yy, xx = np.mgrid[:64, :64]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint16)[..., None], 3, axis=2)
    result["checkerboard"] = dict(transform="sRGB -> sRGB (identity, applied)",
                                  **deviation(srgb.color_transform("srgb", 8), board, (0, 0, 64, 64), 32, 32))
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
