"""Window decode: what decoding only the tiles a crop reads buys.

Workload: images synthetic.permuted_heic(halfmoonbay, seed) (4032 x 3024 in 48
grid tiles of 512 x 512, displayed 3024 x 4032), each with a crop drawn from
torchvision's RandomResizedCrop distribution (scale 0.08-1, ratio 3/4-4/3, ten
attempts, then the centred fallback) in displayed coordinates from a fixed numpy
seed.  Variants, all in one process on one batch that is reloaded in place:
  a  N images decoded whole (what the library did before)
  b  the same N images with windows= (only the tiles each crop reads)
  c  as many images with windows= as bring the picture count back to a's
     (N = 128 only)
One step is --reps pipelined decode_async calls of the prepared batch followed
by one render_tensor(224 x 224) of the crops, between two HIP events on the
stream; step_ms is that time divided by --reps (the bench's step: one decode of
the batch).  The planes are touched before anything is timed, every load is
decoded once untimed, the variants alternate, and the whole is repeated --runs
times: the figure is the median, the spread max - min over the runs.  prepare_ms
(host flatten plus upload, synchronised) is timed apart, on the host clock.
Before timing, b's tensor is compared bit for bit with the tensor a's planes
give for the same crops.

Condition: b's step is not slower than a's by more than the larger of the two
spreads (it decodes a subset of the same pictures).  How much faster b is, and
c's images/s against a's, are results.  N = 16 and N = 1 (the spread parse) are
reported with a and b.

usage: python tools/window_bench.py [--images 128] [--reps 20] [--runs 5] [--out window_decode.json]
"""
import argparse
import json
import math
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import heif_amd as H  # noqa: E402
from heif_amd import synthetic  # noqa: E402

SIZE = (224, 224)


def random_resized_crop(rng, w, h, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """(x, y, cw, ch): torchvision.transforms.RandomResizedCrop.get_params."""
    area = w * h
    for _ in range(10):
        target = area * rng.uniform(*scale)
        aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        cw, ch = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            return int(rng.randint(0, w - cw + 1)), int(rng.randint(0, h - ch + 1)), cw, ch
    r = w / h
    if r < ratio[0]:
        cw, ch = w, int(round(w / ratio[0]))
    elif r > ratio[1]:
        cw, ch = int(round(h * ratio[1])), h
    else:
        cw, ch = w, h
    return (w - cw) // 2, (h - ch) // 2, cw, ch


def count_pictures(imgs, windows):
    import ctypes
    from heif_amd import _lib

    n = len(imgs)
    arr = (ctypes.c_void_p * n)(*[im._h.value for im in imgs])
    src = (_lib.Rect * n)(*[_lib.Rect(*im.source_rect(w)) for im, w in zip(imgs, windows)])
    v = ctypes.c_uint32()
    _lib.check(_lib.lib.heifgpu_batch_count_pictures(arr, n, None, src, ctypes.byref(v)))
    return v.value


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="window_decode.json")
    args = ap.parse_args()
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    ctx = H.DecodeContext(0)
    rng = np.random.RandomState(20)
    n = args.images
    d = H.HeifImage.parse(golden).display
    # images and crops; for variant c keep adding until the crops select a's picture count
    cap = 8 * n
    files = [synthetic.permuted_heic(golden, s) for s in range(n)]
    imgs = H.HeifImage.parse_many(files)
    windows = [random_resized_crop(rng, d.out_width, d.out_height) for _ in range(n)]
    whole = count_pictures(imgs, [None] * n)
    selected = count_pictures(imgs, windows)
    while len(imgs) < cap:  # (an image's pictures do not depend on the rest of the batch)
        img = H.HeifImage.parse(synthetic.permuted_heic(golden, len(imgs)))
        w = random_resized_crop(rng, d.out_width, d.out_height)
        selected += count_pictures([img], [w])
        if selected > whole:
            break
        imgs.append(img)
        windows.append(w)
    n_c = len(imgs)
    outs = ctx.alloc_outputs(imgs)
    for o in outs:  # touch the planes
        for t in (o.y, o.cb, o.cr):
            t.zero_()
    torch.cuda.synchronize()
    ws = [tuple(w) for w in windows]

    def variants_for(m):
        v = {"a": (m, None), "b": (m, ws[:m])}
        if m == n:
            v["c"] = (n_c, ws)
        return v

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "runs": args.runs, "render": list(SIZE),
              "crop_seed": 20, "batches": {}}
    batch = None
    ok = True
    for m in dict.fromkeys((n, 16, 1)):
        if m > n:
            continue
        variants = variants_for(m)
        # b's tensor against a's, bit for bit, before anything is timed
        tensors = {}
        for name in ("a", "b"):
            k, w = variants[name]
            batch = ctx.prepare(imgs[:k], windows=w, reuse=batch)
            batch.decode_async(outs[:k])
            assert not any(batch.status()), name
            tensors[name] = ctx.render_tensor(outs[:k], SIZE, windows=ws[:k])
        equal = bool((tensors["a"].view(torch.int16) == tensors["b"].view(torch.int16)).all())
        del tensors
        ok &= equal
        times = {v: [] for v in variants}
        prep = {v: [] for v in variants}
        pics, geom = {}, {}
        for _ in range(args.runs):
            for name, (k, w) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch = ctx.prepare(imgs[:k], windows=w, reuse=batch, wait=True)
                prep[name].append((time.perf_counter() - t0) * 1e3)
                pics[name], geom[name] = batch.pictures, batch.parse_geometry()["mode"]
                batch.decode_async(outs[:k])  # untimed: the first decode of a load
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    batch.decode_async(outs[:k])
                ctx.render_tensor(outs[:k], SIZE, windows=ws[:k])
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.reps)
                assert not any(batch.status()), name
        entry = {"tensors_b_equal_a": equal}
        for name, (k, w) in variants.items():
            med = statistics.median(times[name])
            entry[name] = {"images": k, "pictures": pics[name], "parse": geom[name], "step_ms": round(med, 4),
                           "spread_ms": round(max(times[name]) - min(times[name]), 4),
                           "step_ms_runs": [round(v, 4) for v in times[name]],
                           "images_per_s": round(k / med * 1e3, 1),
                           "prepare_ms": round(statistics.median(prep[name]), 3)}
        a, b = entry["a"], entry["b"]
        entry["b_minus_a_ms"] = round(b["step_ms"] - a["step_ms"], 4)
        entry["gate_b_not_slower"] = b["step_ms"] - a["step_ms"] <= max(a["spread_ms"], b["spread_ms"])
        ok &= entry["gate_b_not_slower"]
        result["batches"][str(m)] = entry
        for name in variants:
            e = entry[name]
            print(f"N={m:<4} {name}: {e['images']:4d} images {e['pictures']:5d} pictures ({e['parse']}) "
                  f"step {e['step_ms']:8.3f} ms (spread {e['spread_ms']:.3f}) {e['images_per_s']:8.1f} images/s "
                  f"prepare {e['prepare_ms']:.1f} ms")
        print(f"N={m:<4} b equals a bit for bit: {equal}; b - a = {entry['b_minus_a_ms']} ms; "
              f"gate (b not slower beyond the spread): {entry['gate_b_not_slower']}")
    batch.free()
    result["ok"] = ok
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"ok": ok, "out": args.out}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
