"""Display-ready RGB of a whole batch: one heifgpu_render_batch call against a
loop of heifgpu_ycbcr_to_rgb calls (the only RGB path before it).

Workload: N images (default 128) of halfmoonbay's geometry, 4032 x 3024 in
4:2:0 at 8 bits, from planes already on the device (every image its own
planes and its own output, so nothing is served from a cache), with the irot
rotation forced to 0 and to 3.  Variants, alternated in one process after a
warm-up, each timed with HIP events around --reps repetitions:
  loop   N heifgpu_ycbcr_to_rgb calls (N launches, a (out_w / 1024, out_h) grid each)
  batch  one heifgpu_render_batch(RGB8) call (one launch)
The whole measurement is repeated --runs times; the spread is min..max over
the runs.  GB/s counts the algorithmic bytes (1.5 read + 3 written per pixel);
the share is of the 8.0 TB/s HBM3E peak.  RGBA16 of a 10-bit batch (3 bytes
read, 8 written per pixel) is reported alone: it has no earlier counterpart.

usage: python tools/render_bench.py [--images 128] [--reps 20] [--runs 5] [--out render.json]
"""
import argparse
import ctypes
import json
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import heif_amd as H  # noqa: E402
from heif_amd import _lib, synth_encoder as S  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, spec
W, HGT = 4032, 3024


def forced_rotation(data: bytes, rot: int) -> bytes:
    i = data.index(b"irot") + 4  # the irot property's one payload byte
    out = bytearray(data)
    out[i] = rot
    return bytes(out)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(ms_runs, bytes_per_batch):
    med = statistics.median(ms_runs)
    gbs = bytes_per_batch / med / 1e6
    return {"ms_per_batch": round(med, 4), "ms_min": round(min(ms_runs), 4), "ms_max": round(max(ms_runs), 4),
            "ms_runs": [round(v, 4) for v in ms_runs], "GBps": round(gbs, 1),
            "share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    g = torch.Generator(device=dev).manual_seed(1)

    def planes_of(dtype, top):
        ys = [torch.randint(0, top, (HGT, W), generator=g, device=dev, dtype=torch.int32).to(dtype) for _ in range(n)]
        cs = [[torch.randint(0, top, (HGT // 2, W // 2), generator=g, device=dev, dtype=torch.int32).to(dtype)
               for _ in range(n)] for _ in range(2)]
        arr = (_lib.Planes * n)()
        for i in range(n):
            for c, t in enumerate((ys[i], cs[0][i], cs[1][i])):
                arr[i].plane[c] = t.data_ptr()
                arr[i].pitch[c] = t.stride(0) * t.element_size()
        return arr, (ys, cs)

    planes8, keep8 = planes_of(torch.uint8, 256)
    result = {"images": n, "width": W, "height": HGT, "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK_GBS, "rgb8": {}}
    px = n * W * HGT
    for rot in (0, 3):
        img = H.HeifImage.parse(forced_rotation(golden, rot))
        info, d = img.info, img.display
        assert info.rotation == rot and d.n_transforms == 1 and (info.width, info.height) == (W, HGT)
        outs_a = [torch.empty((d.out_height, d.out_width, 3), dtype=torch.uint8, device=dev) for _ in range(n)]
        outs_b = [torch.empty_like(t) for t in outs_a]
        surf = (_lib.Surface * n)()
        for i, t in enumerate(outs_b):
            surf[i].pixels, surf[i].pitch = t.data_ptr(), t.stride(0)
        imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
        one = [ctypes.cast(ctypes.byref(planes8[i]), ctypes.POINTER(_lib.Planes)) for i in range(n)]

        def loop():
            for i in range(n):
                _lib.check(_lib.lib.heifgpu_ycbcr_to_rgb(ctx._h, ctypes.byref(info), one[i],
                                                         ctypes.c_void_p(outs_a[i].data_ptr()), outs_a[i].stride(0), stream))

        def batch():
            _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs, n, planes8, None, None, _lib.PIX_RGB8, surf, stream))

        loop(), batch()  # warm-up, and the two must agree
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs_a, outs_b)), "render_batch differs from ycbcr_to_rgb"
        ms = {"loop": [], "batch": []}
        for _ in range(args.runs):
            for name, fn in (("loop", loop), ("batch", batch)):
                ms[name].append(timed(fn, args.reps))
        r = {name: summary(v, px * 4.5) for name, v in ms.items()}
        spread = max(r["loop"]["ms_max"] - r["loop"]["ms_min"], r["batch"]["ms_max"] - r["batch"]["ms_min"])
        r["spread_ms"] = round(spread, 4)
        r["batch_minus_loop_ms"] = round(r["batch"]["ms_per_batch"] - r["loop"]["ms_per_batch"], 4)
        result["rgb8"][f"rotation_{rot}"] = r
        print(f"rotation {rot}: loop {r['loop']['ms_per_batch']:.3f} ms ({r['loop']['GBps']:.0f} GB/s), "
              f"batch {r['batch']['ms_per_batch']:.3f} ms ({r['batch']['GBps']:.0f} GB/s), spread {spread:.3f} ms",
              flush=True)
        del outs_a, outs_b
    del keep8, planes8
    torch.cuda.empty_cache()

    # RGBA16 of a 10-bit batch of the same geometry (one synthetic tile repeated: only the host parse is needed)
    p10 = S.SynthParams(bit_depth=10)
    img10 = H.HeifImage.parse(S.grid_heic(W, HGT, p10, pictures=[S.picture(p10, 1)] * 48))
    assert img10.info.bit_depth == 10 and (img10.info.width, img10.info.height) == (W, HGT)
    planes10, keep10 = planes_of(torch.int16, 1024)
    outs = [torch.empty((HGT, W, 4), dtype=torch.int16, device=dev) for _ in range(n)]
    surf = (_lib.Surface * n)()
    for i, t in enumerate(outs):
        surf[i].pixels, surf[i].pitch = t.data_ptr(), t.stride(0) * 2
    imgs = (ctypes.c_void_p * n)(*[img10._h.value] * n)

    def batch16():
        _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs, n, planes10, None, None, _lib.PIX_RGBA16, surf, stream))

    batch16()
    torch.cuda.synchronize()
    result["rgba16_10bit"] = summary([timed(batch16, args.reps) for _ in range(args.runs)], px * 11.0)
    print(f"rgba16 10-bit: {result['rgba16_10bit']['ms_per_batch']:.3f} ms ({result['rgba16_10bit']['GBps']:.0f} GB/s)")
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
