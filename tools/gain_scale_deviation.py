"""How far the scaled gain-map HDR render's rule lies from an average in linear light.

    python tools/gain_scale_deviation.py [--headroom 4.0] [--out deviation.json]

heifgpu_render_batch_gain_scaled averages the base's integers and the Q8 gain codes over an
output pixel's footprint and applies the HDR formula once to the averages (include/heifgpu.h
"Gain-map HDR render", the scaled call).  The other rule a caller might expect is the average
of the full-size HDR levels H' in linear light.  This tool measures the difference on the
project's own HDR photo, tests/golden/halfmoonbay.heic, 4032 x 3024 decoded, at 1008 x 756
(4 : 1, every footprint a whole 4 x 4 block, so the display map's rotation plays no part): on
the CPU, in numpy, from the planes of the reference decoder (oracle/), through the library's
host-side tables (Display P3 out, Apple rule) and tests/gain_ref.py's formula.  It needs no
device.  Reported: the maximum and the mean over all samples of |contract - linear-light
average|, in units of 1 / 65535 of SDR white and in PQ codes at 10 bits (203 cd/m2 at SDR
white), with the mean level for scale.  Information for callers; nothing is gated.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import display_ref  # noqa: E402
import gain_ref  # noqa: E402
import heif_amd as H  # noqa: E402
from oracle import oracle  # noqa: E402

K = 4  # the ratio
ROWS = 256  # decoded rows per strip (the int64 temporaries of a whole picture are gigabytes)


def block_sum(a):
    """Sums over K x K blocks of (h, w, ...) -> (h / K, w / K, ...)."""
    h, w = a.shape[:2]
    return a.reshape(h // K, K, w // K, K, *a.shape[2:]).sum(axis=(1, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--headroom", type=float, default=4.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    data = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    base = H.HeifImage.parse(data)
    gimg = H.HeifImage.parse(data, base.gain_map.item_id)
    o = oracle.decode_heic(data, with_checks=False)
    (off, n), = oracle.list_tiles(data, base.gain_map.item_id)[0]
    ho, hl = oracle.list_tiles(data, base.gain_map.item_id)[1]
    G, _, _ = oracle.decode_tile(data[ho:ho + hl], data[off:off + n], gimg.info.width, gimg.info.height)
    Hh, W = o.y.shape
    assert (W, Hh) == (base.info.width, base.info.height) and W % K == 0 and Hh % K == 0 and ROWS % (2 * K) == 0
    t = base.gain_transform(gimg, "display-p3", "linear", 10, headroom=args.headroom)
    tb = gain_ref.tables(t)
    x0, x1, fx, _ = gain_ref.taps(W, G.shape[1])
    y0, y1, fy, _ = gain_ref.taps(Hh, G.shape[0])
    Gi = G.astype(np.int64)
    dev_lin, dev_pq, level_sum, count = [], [], 0.0, 0
    for r0 in range(0, Hh, ROWS):
        rs = slice(r0, min(r0 + ROWS, Hh))
        rows = (np.arange(rs.start, rs.stop) >> 1)[:, None]
        cols = (np.arange(W) >> 1)[None, :]
        px = display_ref.rgb_at_depth(o.y[rs], o.cb[rows, cols], o.cr[rows, cols], base.info.matrix_coeffs,
                                      bool(base.info.full_range), int(t.bits))
        fxs, fys = fx[None, :], fy[rs][:, None]
        top = (256 - fxs) * Gi[y0[rs]][:, x0] + fxs * Gi[y0[rs]][:, x1]
        bot = (256 - fxs) * Gi[y1[rs]][:, x0] + fxs * Gi[y1[rs]][:, x1]
        gq = ((256 - fys) * top + fys * bot + 128) >> 8
        # the average in linear light of the full-size levels, float64
        lin = block_sum(gain_ref.levels(tb, px, gq).astype(np.float64)) / (K * K)
        # the contract: the rounded averages, then the formula once
        C = (2 * block_sum(px) + K * K) // (2 * K * K)
        Gq = (2 * block_sum(gq) + K * K) // (2 * K * K)
        con = gain_ref.levels(tb, C, Gq).astype(np.float64)
        dev_lin.append(np.abs(con - lin))
        dev_pq.append(np.abs(gain_ref.model_pq(con, 10) - gain_ref.model_pq(lin, 10)))
        level_sum += float(lin.sum())
        count += lin.size
    dl, dp = np.concatenate(dev_lin), np.concatenate(dev_pq)
    assert dl.shape == (Hh // K, W // K, 3)
    result = {"file": "tests/golden/halfmoonbay.heic", "from": [W, Hh], "to": [W // K, Hh // K], "headroom": args.headroom,
              "destination": "display-p3", "samples": int(dl.size),
              "units_of_1_65535_sdr_white": {"max": round(float(dl.max()), 2), "mean": round(float(dl.mean()), 3),
                                             "p99": round(float(np.percentile(dl, 99)), 2),
                                             "mean_level": round(level_sum / count, 1)},
              "pq10_codes": {"max": round(float(dp.max()), 3), "mean": round(float(dp.mean()), 4),
                             "p99": round(float(np.percentile(dp, 99)), 3)}}
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
