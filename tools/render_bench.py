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

--scaled measures the scaled render instead (heifgpu_render_batch_scaled,
DESIGN 5.17), on the same images, at rotation 0 and 3, the variants alternated
in one process in each of the --runs runs:
  full      heifgpu_render_batch RGB8 at full size (the kernel before it, unchanged)
  cover512  heifgpu_render_batch_scaled RGB8, COVER to 512 x 384
  cover224  the same to 224 x 224
  torch     for the record: the route without it, `full`, a float conversion and
            torch.nn.functional.interpolate(mode="area") to 512 x 384, image by
            image (the float copy of a whole batch would not fit)
GB/s over algorithmic bytes: 1.5 read per source pixel of the window plus the
output bytes.  The condition of 5.17: cover512 and cover224 no slower than
`full` at the same rotation beyond the measured spread (max - min over runs).

--tensor measures the tensor render (heifgpu_render_batch_tensor),
same images, COVER to 224 x 224, rotation 0 and 3, half of the batch flipped,
the variants alternated in one process in each of the --runs runs:
  scaled       heifgpu_render_batch_scaled RGB8 (the integers, as before it)
  scaled_torch `scaled`, then what a caller wrote before it: permute, float, / 255,
               - mean, / std, half, and the flip of half the batch (to f16 NCHW)
  f16_chw      heifgpu_render_batch_tensor, f16 CHW, the same flips: one launch
  f32_chw      the same to f32 CHW
  bf16_hwc     the same to bf16 HWC
The condition of 5.19: f16_chw faster than scaled_torch by more than the larger
spread (max - min over runs) of the two; f16_chw - scaled is reported.  Before
timing, f16_chw is compared bit for bit with float32(R) * a + b of `scaled`'s
integers computed by torch (a product, then a sum), at the size timed.

--color measures the colour-managed render (heifgpu_render_batch_color and its
kin), Display P3 (halfmoonbay's profile) to sRGB, against the
unmanaged call on the same images, the variants alternated in one process in
each of the --runs runs:
  rgb8_rot0 / rgb8_rot3   heifgpu_render_batch RGB8 at full size, rotation 0 and 3
  rgba16_10bit            the same in RGBA16 of a 10-bit batch
  tensor224_f16           heifgpu_render_batch_tensor, COVER to 224 x 224, f16 CHW
each as `plain` and as `managed`.  With a library that has no colour entry
points (HEIFGPU_LIBRARY naming the parent commit's build) only `plain` is
measured: that is the A/B of the unmanaged kernels across the two commits.

--filter measures the filtered render (heifgpu_render_batch_resampled, DESIGN
5.27), same images, RGB8, COVER to 224 x 224 and to 512 x 384, rotation 0 and 3,
the variants alternated in one process in each of the --runs runs:
  full                  heifgpu_render_batch at full size
  coverNNN_area         heifgpu_render_batch_scaled (the area average)
  coverNNN_bilinear     heifgpu_render_batch_resampled, Pillow's BILINEAR
  coverNNN_bicubic      the same, BICUBIC
  coverNNN_torch        today's route to such pixels: `full`, a float copy and
                        torch.nn.functional.interpolate(mode="bicubic", antialias=True),
                        image by image
The condition of 5.27: each filtered cell faster than its box's torch route by
more than the larger spread (max - min over runs) of the two; the ratios to the
area render and to `full` are reported, not gated.

--tone measures the tone stage of the HDR render (heifgpu_color_transform_make_hdr,
DESIGN 5.28): a 10-bit batch labelled BT.2020 PQ, to sRGB with tone_map bt2390,
against the same planes labelled BT.2020 gamma 2.2 (managed, no tone stage), the
variants alternated in one process in each of the --runs runs:
  rgb8            heifgpu_render_batch_color RGB8 at full size
  rgba16          the same in RGBA16
  tensor224_f16   heifgpu_render_batch_tensor_color, COVER to 224 x 224, f16 CHW
each as `managed` and as `tone`; tone / managed is reported.

--chroma bilinear measures bilinear chroma upsampling: `full`, and
COVER to 224 x 224 and 512 x 384 through the area, BILINEAR and BICUBIC filters, each
with images that replicate chroma and with the same planes under images set to
bilinear, alternated in one process.  bilinear / replicate is reported, nothing is
gated.  With HEIFGPU_LIBRARY naming the parent commit's build (no setter) the replicate
columns alone are measured: the figures to hold this build's replicate launch against.

--gain measures the gain-map HDR render (heifgpu_render_batch_gain): 8-bit
pictures of halfmoonbay's geometry with 2016 x 1512 8-bit gain maps (every image its own
planes), Display P3 to sRGB, Apple rule at headroom 4, against the colour-managed render of
the same planes that writes as many bytes, alternated in one process in each of the --runs runs:
  render_rgba16 / render_hdr_rgba16f   heifgpu_render_batch_color RGBA16 / the HDR render, linear half-float
  render_rgb16 / render_hdr_rgb16pq    the same in RGB16 / the HDR render, PQ at 10 bits
hdr / managed is reported per pair with the spreads (max - min over runs); nothing is gated.

--gain --scaled measures the scaled gain-map HDR render (heifgpu_render_batch_gain_scaled, DESIGN
5.35) on --gain's geometry and transforms, to 224 x 224 cover and to 1008 x 756 stretch, as rgba16f
and as rgb16pq at 10 bits, beside two things the parent commit's code already does, alternated in
one process in each of the --runs runs:
  scaled_sdr_rgba16      heifgpu_render_batch_scaled_color RGBA16 to sRGB of the same planes to the
                         same size: the SDR render that reads the same bytes (hdr / sdr is what the
                         gain pass costs)
  full_hdr_*             the full-size heifgpu_render_batch_gain: what a caller pays today before
                         any resize
Min and spread (max - min over runs) are reported; nothing is gated.

--linear measures the linear-light scaled renders (heifgpu_render_batch_scaled_linear and
_tensor_linear) against the encoded-managed calls on the same planes; see linear_main.

--png measures the PNG output (heifgpu_png_encode_batch): render + encode_png of the golden
picture's planes as rgb8, and of a 10-bit batch as rgba16, against render + copy + Pillow's save() at
compress_level 1 and 6 on one core; see png_main.

usage: python tools/render_bench.py [--images 128] [--reps 20] [--runs 5] [--out render.json]
                                    [--scaled | --tensor | --color | --filter | --tone | --chroma bilinear | --gain [--scaled] | --jpeg | --png | --linear]
"""
import argparse
import ctypes
import json
import os
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


def scaled_main(args):
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    g = torch.Generator(device=dev).manual_seed(1)
    ys = [torch.randint(0, 256, (HGT, W), generator=g, device=dev, dtype=torch.int32).to(torch.uint8) for _ in range(n)]
    cs = [[torch.randint(0, 256, (HGT // 2, W // 2), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
           for _ in range(n)] for _ in range(2)]
    planes = (_lib.Planes * n)()
    for i in range(n):
        for c, t in enumerate((ys[i], cs[0][i], cs[1][i])):
            planes[i].plane[c] = t.data_ptr()
            planes[i].pitch[c] = t.stride(0) * t.element_size()
    result = {"images": n, "width": W, "height": HGT, "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK_GBS, "rgb8": {}}
    for rot in (0, 3):
        img = H.HeifImage.parse(forced_rotation(golden, rot))
        d = img.display
        imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
        full_out = [torch.empty((d.out_height, d.out_width, 3), dtype=torch.uint8, device=dev) for _ in range(n)]
        full_surf = (_lib.Surface * n)()
        for i, t in enumerate(full_out):
            full_surf[i].pixels, full_surf[i].pitch = t.data_ptr(), t.stride(0)

        def full():
            _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8, full_surf, stream))

        def scaled_variant(bw, bh):
            sc = (_lib.Scale * n)()
            for i in range(n):
                _lib.check(_lib.lib.heifgpu_scale_fit(ctypes.byref(d), bw, bh, _lib.FIT_COVER, ctypes.byref(sc[i])))
            out = torch.empty((n, bh, bw, 3), dtype=torch.uint8, device=dev)
            surf = (_lib.Surface * n)()
            for i in range(n):
                surf[i].pixels, surf[i].pitch = out[i].data_ptr(), out[i].stride(0)

            def run():
                _lib.check(_lib.lib.heifgpu_render_batch_scaled(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8, sc,
                                                                surf, stream))
            window_px = (sc[0].width or d.out_width) * (sc[0].height or d.out_height)
            return run, out, sc, n * (window_px * 1.5 + bw * bh * 3)

        cover512, out512, sc512, bytes512 = scaled_variant(512, 384)
        cover224, out224, sc224, bytes224 = scaled_variant(224, 224)
        small = torch.empty((n, 3, 384, 512), dtype=torch.float32, device=dev)

        def torch_route():
            full()
            for i in range(n):
                s = sc512[i]
                win = full_out[i][s.y:s.y + s.height, s.x:s.x + s.width].permute(2, 0, 1)[None].float()
                small[i] = torch.nn.functional.interpolate(win, size=(384, 512), mode="area")[0]

        variants = (("full", full, n * W * HGT * 4.5), ("cover512", cover512, bytes512),
                    ("cover224", cover224, bytes224), ("torch", torch_route, n * W * HGT * 4.5))
        for _, fn, _ in variants:  # warm-up
            fn()
        torch.cuda.synchronize()
        # for the record, how far the float route is from the exact average: at a non-integer ratio
        # interpolate(mode="area") gives every source pixel a window touches the same weight, whole
        # (on these noise planes that is levels, not rounding; tests/test_scale_gpu.py pins the exact result)
        diff = (small.permute(0, 2, 3, 1) - out512.float()).abs()
        agree = {"mean_abs_diff_vs_torch": round(float(diff.mean()), 4), "max_abs_diff_vs_torch": round(float(diff.max()), 4)}
        ms = {name: [] for name, _, _ in variants}
        for _ in range(args.runs):
            for name, fn, _ in variants:
                ms[name].append(timed(fn, args.reps if name != "torch" else max(1, args.reps // 10)))
        r = {name: summary(ms[name], nbytes) for name, _, nbytes in variants}
        r["torch"].pop("GBps"), r["torch"].pop("share_of_hbm_peak")  # no algorithmic byte count of its own
        for name in ("full", "cover512", "cover224", "torch"):
            r[name]["spread_ms"] = round(r[name]["ms_max"] - r[name]["ms_min"], 4)
        for name in ("cover512", "cover224"):
            spread = max(r[name]["spread_ms"], r["full"]["spread_ms"])
            r[name]["minus_full_ms"] = round(r[name]["ms_per_batch"] - r["full"]["ms_per_batch"], 4)
            r[name]["of_full"] = round(r[name]["ms_per_batch"] / r["full"]["ms_per_batch"], 4)
            r[name]["no_slower_than_full_beyond_spread"] = bool(r[name]["ms_per_batch"] <= r["full"]["ms_per_batch"] + spread)
        r["cover512"]["torch_over_it"] = round(r["torch"]["ms_per_batch"] / r["cover512"]["ms_per_batch"], 2)
        r["cover512"].update(agree)
        result["rgb8"][f"rotation_{rot}"] = r
        print(f"rotation {rot}: " + ", ".join(f"{name} {r[name]['ms_per_batch']:.3f} ms (spread {r[name]['spread_ms']:.3f})"
                                              for name, _, _ in variants), flush=True)
        del full_out, out512, out224, small
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def tensor_main(args):
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    g = torch.Generator(device=dev).manual_seed(1)
    ys = [torch.randint(0, 256, (HGT, W), generator=g, device=dev, dtype=torch.int32).to(torch.uint8) for _ in range(n)]
    cs = [[torch.randint(0, 256, (HGT // 2, W // 2), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
           for _ in range(n)] for _ in range(2)]
    planes = (_lib.Planes * n)()
    for i in range(n):
        for c, t in enumerate((ys[i], cs[0][i], cs[1][i])):
            planes[i].plane[c] = t.data_ptr()
            planes[i].pitch[c] = t.stride(0) * t.element_size()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    a = torch.tensor([1.0 / (255.0 * v) for v in std], dtype=torch.float64).float().to(dev)
    b = torch.tensor([-m / v for m, v in zip(mean, std)], dtype=torch.float64).float().to(dev)
    mean_t, std_t = torch.tensor(mean, device=dev).view(1, 3, 1, 1), torch.tensor(std, device=dev).view(1, 3, 1, 1)
    flips = [i & 1 for i in range(n)]  # half of the batch mirrored
    flip_idx = torch.tensor([i for i in range(n) if flips[i]], device=dev)
    flip_arr = (ctypes.c_uint32 * n)(*flips)
    bw = bh = 224
    result = {"images": n, "width": W, "height": HGT, "box": [bh, bw], "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "tensor": {}}
    for rot in (0, 3):
        img = H.HeifImage.parse(forced_rotation(golden, rot))
        d = img.display
        imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
        sc = (_lib.Scale * n)()
        for i in range(n):
            _lib.check(_lib.lib.heifgpu_scale_fit(ctypes.byref(d), bw, bh, _lib.FIT_COVER, ctypes.byref(sc[i])))
        ints = torch.empty((n, bh, bw, 3), dtype=torch.uint8, device=dev)
        surf = (_lib.Surface * n)()
        for i in range(n):
            surf[i].pixels, surf[i].pitch = ints[i].data_ptr(), ints[i].stride(0)

        def scaled():
            _lib.check(_lib.lib.heifgpu_render_batch_scaled(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8, sc, surf,
                                                            stream))

        keep = {}

        def scaled_torch():
            scaled()
            x = ints.permute(0, 3, 1, 2).float().div(255).sub(mean_t).div(std_t).half()
            x[flip_idx] = x[flip_idx].flip(-1)
            keep["x"] = x

        def tensor_variant(dtype, elem, layout):
            chw = layout == _lib.LAYOUT_CHW
            out = torch.empty((n, 3, bh, bw) if chw else (n, bh, bw, 3), dtype=dtype, device=dev)
            fmt = _lib.TensorFormat(src=_lib.PIX_RGB8, elem=elem, layout=layout)
            for c in range(3):
                fmt.a[c], fmt.b[c] = float(a[c]), float(b[c])
            ts = (_lib.TensorSurface * n)()
            for i in range(n):
                ts[i].data = out[i].data_ptr()
                ts[i].stride_c = out[i].stride(0) * out.element_size() if chw else 0
                ts[i].stride_y = out[i].stride(1 if chw else 0) * out.element_size()

            def run():
                _lib.check(_lib.lib.heifgpu_render_batch_tensor(ctx._h, imgs, n, planes, None, None, ctypes.byref(fmt), sc,
                                                                flip_arr, ts, stream))
            return run, out

        f16_chw, out16 = tensor_variant(torch.float16, _lib.ELEM_F16, _lib.LAYOUT_CHW)
        f32_chw, out32 = tensor_variant(torch.float32, _lib.ELEM_F32, _lib.LAYOUT_CHW)
        bf16_hwc, outbf = tensor_variant(torch.bfloat16, _lib.ELEM_BF16, _lib.LAYOUT_HWC)
        variants = (("scaled", scaled), ("scaled_torch", scaled_torch), ("f16_chw", f16_chw), ("f32_chw", f32_chw),
                    ("bf16_hwc", bf16_hwc))
        for _, fn in variants:  # warm-up
            fn()
        torch.cuda.synchronize()
        # the results at the size timed: the definition over `scaled`'s integers, by torch (a product, then a sum)
        want = ints.permute(0, 3, 1, 2).float() * a.view(1, 3, 1, 1) + b.view(1, 3, 1, 1)
        want[flip_idx] = want[flip_idx].flip(-1)
        assert torch.equal(out32, want), "f32_chw differs from float32(R) * a + b"
        assert torch.equal(out16.view(torch.int16), want.half().view(torch.int16)), "f16_chw differs"
        assert torch.equal(outbf.view(torch.int16), want.permute(0, 2, 3, 1).bfloat16().view(torch.int16)), "bf16_hwc differs"
        route_diff = float((keep["x"].float() - out16.float()).abs().max())  # the float route rounds in another order
        ms = {name: [] for name, _ in variants}
        for _ in range(args.runs):
            for name, fn in variants:
                ms[name].append(timed(fn, args.reps))
        r = {}
        for name, _ in variants:
            v = ms[name]
            r[name] = {"ms_per_batch": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                       "ms_max": round(max(v), 4), "ms_runs": [round(x, 4) for x in v],
                       "spread_ms": round(max(v) - min(v), 4)}
        pair = max(r["f16_chw"]["spread_ms"], r["scaled_torch"]["spread_ms"])
        r["f16_chw"]["scaled_torch_minus_it_ms"] = round(r["scaled_torch"]["ms_per_batch"] - r["f16_chw"]["ms_per_batch"], 4)
        r["f16_chw"]["faster_than_scaled_torch_beyond_spread"] = bool(
            r["scaled_torch"]["ms_per_batch"] - r["f16_chw"]["ms_per_batch"] > pair)
        for name in ("f16_chw", "f32_chw", "bf16_hwc"):
            r[name]["minus_scaled_ms"] = round(r[name]["ms_per_batch"] - r["scaled"]["ms_per_batch"], 4)
        r["f16_chw"]["max_abs_diff_vs_scaled_torch"] = round(route_diff, 6)
        result["tensor"][f"rotation_{rot}"] = r
        print(f"rotation {rot}: " + ", ".join(f"{name} {r[name]['ms_per_batch']:.3f} ms (spread {r[name]['spread_ms']:.3f})"
                                              for name, _ in variants), flush=True)
        del ints, out16, out32, outbf, want, keep
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def color_main(args):
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    managed_ok = hasattr(_lib.lib, "heifgpu_render_batch_color")
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

    def transforms(img, bits):
        if not managed_ok:
            return None, None
        t = img.color_transform("srgb", bits)
        assert not t.identity
        return (ctypes.c_void_p * n)(*[ctypes.addressof(t)] * n), t

    px = n * W * HGT
    result = {"images": n, "width": W, "height": HGT, "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK_GBS, "library": _lib.LIB_PATH.name,
              "managed": managed_ok, "transform": "Display P3 profile (halfmoonbay) -> sRGB", "cases": {}}
    cases = []  # (name, plain, managed or None, algorithmic bytes, what to keep alive)
    planes8, keep8 = planes_of(torch.uint8, 256)
    for rot in (0, 3):
        img = H.HeifImage.parse(forced_rotation(golden, rot))
        d = img.display
        outs = [torch.empty((d.out_height, d.out_width, 3), dtype=torch.uint8, device=dev) for _ in range(n)]
        surf = (_lib.Surface * n)()
        for i, t in enumerate(outs):
            surf[i].pixels, surf[i].pitch = t.data_ptr(), t.stride(0)
        imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
        xf, keep = transforms(img, 8)

        def plain(imgs=imgs, surf=surf):
            _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs, n, planes8, None, None, _lib.PIX_RGB8, surf, stream))

        def managed(imgs=imgs, surf=surf, xf=xf):
            _lib.check(_lib.lib.heifgpu_render_batch_color(ctx._h, imgs, n, planes8, None, None, _lib.PIX_RGB8, xf, surf,
                                                           stream))
        cases.append((f"rgb8_rot{rot}", plain, managed if managed_ok else None, px * 4.5, (img, outs, keep)))
        if rot == 3:  # the tensor render of the same pictures
            sc = (_lib.Scale * n)()
            for i in range(n):
                _lib.check(_lib.lib.heifgpu_scale_fit(ctypes.byref(d), 224, 224, _lib.FIT_COVER, ctypes.byref(sc[i])))
            out = torch.empty((n, 3, 224, 224), dtype=torch.float16, device=dev)
            fmt = _lib.TensorFormat(src=_lib.PIX_RGB8, elem=_lib.ELEM_F16, layout=_lib.LAYOUT_CHW)
            for c, (m_, s_) in enumerate(zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
                fmt.a[c], fmt.b[c] = 1.0 / (255.0 * s_), -m_ / s_
            ts = (_lib.TensorSurface * n)()
            for i in range(n):
                ts[i].data, ts[i].stride_c, ts[i].stride_y = out[i].data_ptr(), 224 * 224 * 2, 224 * 2

            def tplain(imgs=imgs, sc=sc, ts=ts, fmt=fmt):
                _lib.check(_lib.lib.heifgpu_render_batch_tensor(ctx._h, imgs, n, planes8, None, None, ctypes.byref(fmt), sc,
                                                                None, ts, stream))

            def tmanaged(imgs=imgs, sc=sc, ts=ts, fmt=fmt, xf=xf):
                _lib.check(_lib.lib.heifgpu_render_batch_tensor_color(ctx._h, imgs, n, planes8, None, None,
                                                                      ctypes.byref(fmt), sc, None, xf, ts, stream))
            window_px = (sc[0].width or d.out_width) * (sc[0].height or d.out_height)
            cases.append(("tensor224_f16", tplain, tmanaged if managed_ok else None,
                          n * (window_px * 1.5 + 224 * 224 * 6), (out,)))
    # RGBA16 of a 10-bit batch of the same geometry carrying the same profile (only the host parse is needed)
    p10 = S.SynthParams(bit_depth=10)
    colr = S.icc_box(H.HeifImage.parse(golden).icc_profile) if managed_ok else None
    img10 = H.HeifImage.parse(S.grid_heic(W, HGT, p10, pictures=[S.picture(p10, 1)] * 48, colr=colr))
    planes10, keep10 = planes_of(torch.int16, 1024)
    outs16 = [torch.empty((HGT, W, 4), dtype=torch.int16, device=dev) for _ in range(n)]
    surf16 = (_lib.Surface * n)()
    for i, t in enumerate(outs16):
        surf16[i].pixels, surf16[i].pitch = t.data_ptr(), t.stride(0) * 2
    imgs10 = (ctypes.c_void_p * n)(*[img10._h.value] * n)
    xf10, keep_t10 = transforms(img10, 10)

    def plain16():
        _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs10, n, planes10, None, None, _lib.PIX_RGBA16, surf16, stream))

    def managed16():
        _lib.check(_lib.lib.heifgpu_render_batch_color(ctx._h, imgs10, n, planes10, None, None, _lib.PIX_RGBA16, xf10,
                                                       surf16, stream))
    cases.append(("rgba16_10bit", plain16, managed16 if managed_ok else None, px * 11.0, (img10, keep_t10)))

    variants = []
    for name, plain, managed, nbytes, _ in cases:
        variants.append((name, "plain", plain, nbytes))
        if managed is not None:
            variants.append((name, "managed", managed, nbytes))
    for *_, fn, _ in variants:  # warm-up (and the tables' one upload)
        fn()
    torch.cuda.synchronize()
    ms = {(name, kind): [] for name, kind, _, _ in variants}
    for _ in range(args.runs):
        for name, kind, fn, _ in variants:
            ms[(name, kind)].append(timed(fn, args.reps))
    for name, kind, _, nbytes in variants:
        r = summary(ms[(name, kind)], nbytes)
        r["spread_ms"] = round(r["ms_max"] - r["ms_min"], 4)
        result["cases"].setdefault(name, {})[kind] = r
    for name, r in result["cases"].items():
        if "managed" in r:
            r["managed_over_plain"] = round(r["managed"]["ms_per_batch"] / r["plain"]["ms_per_batch"], 4)
            r["managed_minus_plain_ms"] = round(r["managed"]["ms_per_batch"] - r["plain"]["ms_per_batch"], 4)
            r["difference_inside_spread"] = bool(abs(r["managed_minus_plain_ms"]) <=
                                                 max(r["managed"]["spread_ms"], r["plain"]["spread_ms"]))
        print(f"{name}: " + ", ".join(f"{k} {r[k]['ms_per_batch']:.3f} ms ({r[k]['GBps']:.0f} GB/s, spread "
                                      f"{r[k]['spread_ms']:.3f})" for k in ("plain", "managed") if k in r), flush=True)
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def tone_main(args):
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    p10 = S.SynthParams(bit_depth=10)
    pics = [S.picture(p10, 1)] * 48  # (only the host parse is needed: the planes below are random)
    sources = {"managed": S.nclx_box(9, 4, 9, False), "tone": S.nclx_box(9, 16, 9, False)}
    imgs = {k: H.HeifImage.parse(S.grid_heic(W, HGT, p10, pictures=pics, colr=c)) for k, c in sources.items()}
    ys = [torch.randint(0, 1024, (HGT, W), generator=g, device=dev, dtype=torch.int32).to(torch.int16) for _ in range(n)]
    cs = [[torch.randint(0, 1024, (HGT // 2, W // 2), generator=g, device=dev, dtype=torch.int32).to(torch.int16)
           for _ in range(n)] for _ in range(2)]
    planes = (_lib.Planes * n)()
    for i in range(n):
        for c, t in enumerate((ys[i], cs[0][i], cs[1][i])):
            planes[i].plane[c] = t.data_ptr()
            planes[i].pitch[c] = t.stride(0) * t.element_size()
    xfs = {}
    for bits in (8, 10):
        xfs["managed", bits] = imgs["managed"].color_transform("srgb", bits)
        xfs["tone", bits] = imgs["tone"].color_transform("srgb", bits, "bt2390")
        assert not xfs["managed", bits].tone and xfs["tone", bits].tone

    def handles(kind, bits):
        return ((ctypes.c_void_p * n)(*[imgs[kind]._h.value] * n), (ctypes.c_void_p * n)(*[ctypes.addressof(xfs[kind, bits])] * n))

    px = n * W * HGT
    result = {"images": n, "width": W, "height": HGT, "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK_GBS, "library": _lib.LIB_PATH.name,
              "managed": "10-bit BT.2020 gamma 2.2 -> sRGB", "tone": "10-bit BT.2020 PQ -> sRGB, bt2390, Lsrc 1000",
              "cases": {}}
    out8 = [torch.empty((HGT, W, 3), dtype=torch.uint8, device=dev) for _ in range(n)]
    out16 = [torch.empty((HGT, W, 4), dtype=torch.int16, device=dev) for _ in range(n)]
    surf8, surf16 = (_lib.Surface * n)(), (_lib.Surface * n)()
    for i in range(n):
        surf8[i].pixels, surf8[i].pitch = out8[i].data_ptr(), out8[i].stride(0)
        surf16[i].pixels, surf16[i].pitch = out16[i].data_ptr(), out16[i].stride(0) * 2
    d = imgs["tone"].display
    sc = (_lib.Scale * n)()
    for i in range(n):
        _lib.check(_lib.lib.heifgpu_scale_fit(ctypes.byref(d), 224, 224, _lib.FIT_COVER, ctypes.byref(sc[i])))
    tout = torch.empty((n, 3, 224, 224), dtype=torch.float16, device=dev)
    fmt = _lib.TensorFormat(src=_lib.PIX_RGB8, elem=_lib.ELEM_F16, layout=_lib.LAYOUT_CHW)
    for c, (m_, s_) in enumerate(zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        fmt.a[c], fmt.b[c] = 1.0 / (255.0 * s_), -m_ / s_
    ts = (_lib.TensorSurface * n)()
    for i in range(n):
        ts[i].data, ts[i].stride_c, ts[i].stride_y = tout[i].data_ptr(), 224 * 224 * 2, 224 * 2
    window_px = (sc[0].width or d.out_width) * (sc[0].height or d.out_height)

    variants, keep = [], []
    for kind in ("managed", "tone"):
        h8, h10 = handles(kind, 8), handles(kind, 10)
        keep += [h8, h10]

        def rgb8(h=h8):
            _lib.check(_lib.lib.heifgpu_render_batch_color(ctx._h, h[0], n, planes, None, None, _lib.PIX_RGB8, h[1], surf8, stream))

        def rgba16(h=h10):
            _lib.check(_lib.lib.heifgpu_render_batch_color(ctx._h, h[0], n, planes, None, None, _lib.PIX_RGBA16, h[1], surf16,
                                                           stream))

        def tensor(h=h8):
            _lib.check(_lib.lib.heifgpu_render_batch_tensor_color(ctx._h, h[0], n, planes, None, None, ctypes.byref(fmt), sc,
                                                                  None, h[1], ts, stream))
        variants += [("rgb8", kind, rgb8, px * 6.0), ("rgba16", kind, rgba16, px * 11.0),
                     ("tensor224_f16", kind, tensor, n * (window_px * 3.0 + 224 * 224 * 6))]
    for *_, fn, _ in variants:  # warm-up (and the tables' one upload)
        fn()
    torch.cuda.synchronize()
    ms = {(name, kind): [] for name, kind, _, _ in variants}
    for _ in range(args.runs):
        for name, kind, fn, _ in variants:
            ms[(name, kind)].append(timed(fn, args.reps))
    for name, kind, _, nbytes in variants:
        r = summary(ms[(name, kind)], nbytes)
        r["spread_ms"] = round(r["ms_max"] - r["ms_min"], 4)
        result["cases"].setdefault(name, {})[kind] = r
    for name, r in result["cases"].items():
        r["tone_over_managed"] = round(r["tone"]["ms_per_batch"] / r["managed"]["ms_per_batch"], 4)
        r["tone_minus_managed_ms"] = round(r["tone"]["ms_per_batch"] - r["managed"]["ms_per_batch"], 4)
        r["difference_inside_spread"] = bool(abs(r["tone_minus_managed_ms"]) <= max(r["tone"]["spread_ms"], r["managed"]["spread_ms"]))
        print(f"{name}: " + ", ".join(f"{k} {r[k]['ms_per_batch']:.3f} ms ({r[k]['GBps']:.0f} GB/s, spread "
                                      f"{r[k]['spread_ms']:.3f})" for k in ("managed", "tone")) +
              f", tone / managed {r['tone_over_managed']:.4f}", flush=True)
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def filter_main(args):
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    g = torch.Generator(device=dev).manual_seed(1)
    ys = [torch.randint(0, 256, (HGT, W), generator=g, device=dev, dtype=torch.int32).to(torch.uint8) for _ in range(n)]
    cs = [[torch.randint(0, 256, (HGT // 2, W // 2), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
           for _ in range(n)] for _ in range(2)]
    planes = (_lib.Planes * n)()
    for i in range(n):
        for c, t in enumerate((ys[i], cs[0][i], cs[1][i])):
            planes[i].plane[c] = t.data_ptr()
            planes[i].pitch[c] = t.stride(0) * t.element_size()
    boxes = (("cover224", 224, 224), ("cover512", 512, 384))
    filters = (("bilinear", _lib.FILTER_BILINEAR), ("bicubic", _lib.FILTER_BICUBIC))
    result = {"images": n, "width": W, "height": HGT, "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "rgb8": {}}
    for rot in (0, 3):
        img = H.HeifImage.parse(forced_rotation(golden, rot))
        d = img.display
        imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
        full_out = [torch.empty((d.out_height, d.out_width, 3), dtype=torch.uint8, device=dev) for _ in range(n)]
        full_surf = (_lib.Surface * n)()
        for i, t in enumerate(full_out):
            full_surf[i].pixels, full_surf[i].pitch = t.data_ptr(), t.stride(0)

        def full():
            _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8, full_surf, stream))

        variants, keep = [("full", full)], []
        for box, bw, bh in boxes:
            sc = (_lib.Scale * n)()
            for i in range(n):
                _lib.check(_lib.lib.heifgpu_scale_fit(ctypes.byref(d), bw, bh, _lib.FIT_COVER, ctypes.byref(sc[i])))

            def surfaces():
                out = torch.empty((n, bh, bw, 3), dtype=torch.uint8, device=dev)
                surf = (_lib.Surface * n)()
                for i in range(n):
                    surf[i].pixels, surf[i].pitch = out[i].data_ptr(), out[i].stride(0)
                keep.append(out)
                return out, surf

            _, asurf = surfaces()

            def area(sc=sc, surf=asurf):
                _lib.check(_lib.lib.heifgpu_render_batch_scaled(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8, sc, surf,
                                                                stream))
            variants.append((f"{box}_area", area))
            for fname, code in filters:
                _, fsurf = surfaces()

                def filtered(sc=sc, surf=fsurf, code=code):
                    _lib.check(_lib.lib.heifgpu_render_batch_resampled(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8,
                                                                       sc, code, None, surf, stream))
                variants.append((f"{box}_{fname}", filtered))
            small = torch.empty((n, 3, bh, bw), dtype=torch.float32, device=dev)
            keep.append(small)

            def torch_route(sc=sc, small=small, bw=bw, bh=bh):
                # today's route to a bicubic picture: the full-size render, a float copy and an antialiased
                # interpolation, image by image (the float copy of a whole batch would not fit)
                full()
                for i in range(n):
                    s = sc[i]
                    win = full_out[i][s.y:s.y + s.height, s.x:s.x + s.width].permute(2, 0, 1)[None].float()
                    small[i] = torch.nn.functional.interpolate(win, size=(bh, bw), mode="bicubic", antialias=True)[0]
            variants.append((f"{box}_torch", torch_route))
        for _, fn in variants:  # warm-up
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in variants}
        for _ in range(args.runs):
            for name, fn in variants:
                ms[name].append(timed(fn, args.reps if not name.endswith("_torch") else max(1, args.reps // 10)))
        r = {}
        for name, _ in variants:
            v = ms[name]
            r[name] = {"ms_per_batch": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                       "ms_max": round(max(v), 4), "ms_runs": [round(x, 4) for x in v],
                       "spread_ms": round(max(v) - min(v), 4)}
        for box, _, _ in boxes:
            for fname, _ in filters:
                c, route = r[f"{box}_{fname}"], r[f"{box}_torch"]
                pair = max(c["spread_ms"], route["spread_ms"])
                c["torch_minus_it_ms"] = round(route["ms_per_batch"] - c["ms_per_batch"], 4)
                c["beats_torch_route_beyond_spread"] = bool(route["ms_per_batch"] - c["ms_per_batch"] > pair)
                c["of_area"] = round(c["ms_per_batch"] / r[f"{box}_area"]["ms_per_batch"], 3)
                c["of_full"] = round(c["ms_per_batch"] / r["full"]["ms_per_batch"], 3)
        result["rgb8"][f"rotation_{rot}"] = r
        print(f"rotation {rot}: " + ", ".join(f"{name} {r[name]['ms_per_batch']:.3f} ms (spread {r[name]['spread_ms']:.3f})"
                                              for name, _ in variants), flush=True)
        del full_out, keep, variants
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def chroma_main(args):
    """--chroma bilinear: the full-size render, the area-scaled render and the filtered render
    (cover 224 x 224 and 512 x 384, rotation 0 and 3, RGB8) of a batch whose images replicate
    chroma and of the same planes under images set to bilinear upsampling, interleaved in the
    same run.  The replicate figures are this library's launch of the kernels it had before:
    run the tool again with HEIFGPU_LIBRARY naming the parent commit's build (which has no
    setter: the replicate columns alone are then measured) to set them beside the parent's."""
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    g = torch.Generator(device=dev).manual_seed(1)
    ys = [torch.randint(0, 256, (HGT, W), generator=g, device=dev, dtype=torch.int32).to(torch.uint8) for _ in range(n)]
    cs = [[torch.randint(0, 256, (HGT // 2, W // 2), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
           for _ in range(n)] for _ in range(2)]
    planes = (_lib.Planes * n)()
    for i in range(n):
        for c, t in enumerate((ys[i], cs[0][i], cs[1][i])):
            planes[i].plane[c] = t.data_ptr()
            planes[i].pitch[c] = t.stride(0) * t.element_size()
    has_setter = hasattr(_lib.lib, "heifgpu_image_set_chroma_upsampling")
    modes = ("replicate", args.chroma) if has_setter and args.chroma != "replicate" else ("replicate",)
    result = {"images": n, "width": W, "height": HGT, "reps": args.reps, "runs": args.runs, "modes": list(modes),
              "library": os.environ.get("HEIFGPU_LIBRARY", "default"), "device": torch.cuda.get_device_name(0), "rgb8": {}}
    for rot in (0, 3):
        variants, keep = [], []
        for mode in modes:
            img = H.HeifImage.parse(forced_rotation(golden, rot))
            if mode != "replicate":
                img.chroma_upsampling = mode
            keep.append(img)
            d = img.display
            imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
            full_out = torch.empty((n, d.out_height, d.out_width, 3), dtype=torch.uint8, device=dev)
            keep.append(full_out)

            def surfaces(out):
                surf = (_lib.Surface * n)()
                for i in range(n):
                    surf[i].pixels, surf[i].pitch = out[i].data_ptr(), out[i].stride(0)
                return surf

            def full(imgs=imgs, surf=surfaces(full_out)):
                _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8, surf, stream))
            variants.append((f"full_{mode}", full))
            for box, bw, bh in (("cover224", 224, 224), ("cover512", 512, 384)):
                sc = (_lib.Scale * n)()
                for i in range(n):
                    _lib.check(_lib.lib.heifgpu_scale_fit(ctypes.byref(d), bw, bh, _lib.FIT_COVER, ctypes.byref(sc[i])))
                for fname, code in (("area", _lib.FILTER_AREA), ("bilinear", _lib.FILTER_BILINEAR), ("bicubic", _lib.FILTER_BICUBIC)):
                    out = torch.empty((n, bh, bw, 3), dtype=torch.uint8, device=dev)
                    keep.append(out)

                    def scaled(imgs=imgs, sc=sc, surf=surfaces(out), code=code):
                        _lib.check(_lib.lib.heifgpu_render_batch_resampled(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGB8,
                                                                           sc, code, None, surf, stream))
                    variants.append((f"{box}_{fname}_{mode}", scaled))
        for _, fn in variants:  # warm-up
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in variants}
        for _ in range(args.runs):
            for name, fn in variants:
                ms[name].append(timed(fn, args.reps))
        r = {}
        for name, _ in variants:
            v = ms[name]
            r[name] = {"ms_per_batch": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                       "ms_runs": [round(x, 4) for x in v], "spread_ms": round(max(v) - min(v), 4)}
        if len(modes) == 2:
            for name in [k for k in r if k.endswith("_replicate")]:
                b = r[name[:-len("replicate")] + modes[1]]
                b["of_replicate"] = round(b["ms_per_batch"] / r[name]["ms_per_batch"], 3)
                b["minus_replicate_ms"] = round(b["ms_per_batch"] - r[name]["ms_per_batch"], 4)
        result["rgb8"][f"rotation_{rot}"] = r
        print(f"rotation {rot}: " + ", ".join(f"{name} {r[name]['ms_per_batch']:.3f} ms (spread {r[name]['spread_ms']:.3f})"
                                              for name, _ in variants), flush=True)
        del variants, keep
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def gain_main(args):
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = forced_rotation((ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes(), 0)
    g = torch.Generator(device=dev).manual_seed(1)
    img = H.HeifImage.parse(golden)
    gimg = H.HeifImage.parse(golden, img.gain_map.item_id)
    gi = gimg.info
    assert (img.info.width, img.info.height, gi.width, gi.height) == (W, HGT, W // 2, HGT // 2)

    def plane(h, w):
        return torch.randint(0, 256, (h, w), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)

    keep = [[plane(HGT, W), plane(HGT // 2, W // 2), plane(HGT // 2, W // 2), plane(gi.height, gi.width)] for _ in range(n)]
    planes, gplanes = (_lib.Planes * n)(), (_lib.Planes * n)()
    for i, (y, cb, cr, gm) in enumerate(keep):
        for c, t in enumerate((y, cb, cr)):
            planes[i].plane[c], planes[i].pitch[c] = t.data_ptr(), t.stride(0)
        gplanes[i].plane[0], gplanes[i].pitch[0] = gm.data_ptr(), gm.stride(0)
    # one 8-byte-per-pixel surface per image; the 6-byte formats write into the same memory
    outs = [torch.empty((HGT, W, 4), dtype=torch.int16, device=dev) for _ in range(n)]
    surf = {ch: (_lib.Surface * n)() for ch in (3, 4)}
    for ch in (3, 4):
        for i, t in enumerate(outs):
            surf[ch][i].pixels, surf[ch][i].pitch = t.data_ptr(), W * ch * 2
    imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
    gimgs = (ctypes.c_void_p * n)(*[gimg._h.value] * n)
    ct = img.color_transform("srgb", 8)
    assert not ct.identity
    xf = (ctypes.c_void_p * n)(*[ctypes.addressof(ct)] * n)
    gts = {enc: img.gain_transform(gimg, "srgb", enc, 10, headroom=4.0) for enc in ("linear", "pq")}
    gxf = {enc: (ctypes.c_void_p * n)(*[ctypes.addressof(t)] * n) for enc, t in gts.items()}

    def managed(fmt, ch):
        def run():
            _lib.check(_lib.lib.heifgpu_render_batch_color(ctx._h, imgs, n, planes, None, None, fmt, xf, surf[ch], stream))
        return run

    def hdr(fmt, ch, enc):
        def run():
            _lib.check(_lib.lib.heifgpu_render_batch_gain(ctx._h, imgs, n, planes, gimgs, gplanes, None, None, fmt, gxf[enc],
                                                          surf[ch], stream))
        return run

    px = n * W * HGT
    variants = [("rgba", "render_rgba16", managed(_lib.PIX_RGBA16, 4), px * 9.5),
                ("rgba", "render_hdr_rgba16f", hdr(_lib.PIX_HDR_RGBA16F, 4, "linear"), px * 9.75),
                ("rgb", "render_rgb16", managed(_lib.PIX_RGB16, 3), px * 7.5),
                ("rgb", "render_hdr_rgb16pq", hdr(_lib.PIX_HDR_RGB16PQ, 3, "pq"), px * 7.75)]
    result = {"images": n, "width": W, "height": HGT, "gain_width": gi.width, "gain_height": gi.height, "reps": args.reps,
              "runs": args.runs, "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK_GBS,
              "library": _lib.LIB_PATH.name, "transform": "Display P3 profile (halfmoonbay) -> sRGB; Apple rule, headroom 4",
              "cases": {}}
    for *_, fn, _ in variants:  # warm-up (and the tables' one upload)
        fn()
    torch.cuda.synchronize()
    ms = {kind: [] for _, kind, _, _ in variants}
    for _ in range(args.runs):
        for _, kind, fn, _ in variants:
            ms[kind].append(timed(fn, args.reps))
    for name, kind, _, nbytes in variants:
        r = summary(ms[kind], nbytes)
        r["spread_ms"] = round(r["ms_max"] - r["ms_min"], 4)
        result["cases"].setdefault(name, {})[kind] = r
    for name, r in result["cases"].items():
        base, new = [k for k in r if not k.startswith("render_hdr")][0], [k for k in r if k.startswith("render_hdr")][0]
        r["hdr_over_managed"] = round(r[new]["ms_per_batch"] / r[base]["ms_per_batch"], 4)
        r["hdr_minus_managed_ms"] = round(r[new]["ms_per_batch"] - r[base]["ms_per_batch"], 4)
        print(f"{name}: " + ", ".join(f"{k} {r[k]['ms_per_batch']:.3f} ms ({r[k]['GBps']:.0f} GB/s, spread "
                                      f"{r[k]['spread_ms']:.3f})" for k in (base, new)) +
              f", ratio {r['hdr_over_managed']:.3f}", flush=True)
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def gain_scaled_main(args):
    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    golden = forced_rotation((ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes(), 0)
    g = torch.Generator(device=dev).manual_seed(1)
    img = H.HeifImage.parse(golden)
    gimg = H.HeifImage.parse(golden, img.gain_map.item_id)
    gi, d = gimg.info, img.display
    assert (img.info.width, img.info.height, gi.width, gi.height) == (W, HGT, W // 2, HGT // 2)

    def plane(h, w):
        return torch.randint(0, 256, (h, w), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)

    keep = [[plane(HGT, W), plane(HGT // 2, W // 2), plane(HGT // 2, W // 2), plane(gi.height, gi.width)] for _ in range(n)]
    planes, gplanes = (_lib.Planes * n)(), (_lib.Planes * n)()
    for i, (y, cb, cr, gm) in enumerate(keep):
        for c, t in enumerate((y, cb, cr)):
            planes[i].plane[c], planes[i].pitch[c] = t.data_ptr(), t.stride(0)
        gplanes[i].plane[0], gplanes[i].pitch[0] = gm.data_ptr(), gm.stride(0)
    imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
    gimgs = (ctypes.c_void_p * n)(*[gimg._h.value] * n)
    ct = img.color_transform("srgb", 8)
    assert not ct.identity
    xf = (ctypes.c_void_p * n)(*[ctypes.addressof(ct)] * n)
    gts = {enc: img.gain_transform(gimg, "srgb", enc, 10, headroom=4.0) for enc in ("linear", "pq")}
    gxf = {enc: (ctypes.c_void_p * n)(*[ctypes.addressof(t)] * n) for enc, t in gts.items()}

    def surfaces(h, w, ch):
        # one 8-byte-per-pixel surface per image; the 6-byte format writes into the same memory
        out = torch.empty((n, h, w, 4), dtype=torch.int16, device=dev)
        surf = (_lib.Surface * n)()
        for i in range(n):
            surf[i].pixels, surf[i].pitch = out[i].data_ptr(), w * ch * 2
        return out, surf

    full_px, full_surf4 = surfaces(HGT, W, 4)
    full_surf3 = (_lib.Surface * n)()
    for i in range(n):
        full_surf3[i].pixels, full_surf3[i].pitch = full_px[i].data_ptr(), W * 6

    def full_hdr(fmt, surf, enc):
        def run():
            _lib.check(_lib.lib.heifgpu_render_batch_gain(ctx._h, imgs, n, planes, gimgs, gplanes, None, None, fmt, gxf[enc],
                                                          surf, stream))
        return run

    variants = [("full", "full_hdr_rgba16f", full_hdr(_lib.PIX_HDR_RGBA16F, full_surf4, "linear"), n * W * HGT * 9.75),
                ("full", "full_hdr_rgb16pq", full_hdr(_lib.PIX_HDR_RGB16PQ, full_surf3, "pq"), n * W * HGT * 7.75)]
    keep_out = []
    for name, bw, bh, mode in (("cover224", 224, 224, _lib.FIT_COVER), ("stretch1008", 1008, 756, _lib.FIT_STRETCH)):
        sc = (_lib.Scale * n)()
        for i in range(n):
            _lib.check(_lib.lib.heifgpu_scale_fit(ctypes.byref(d), bw, bh, mode, ctypes.byref(sc[i])))
        window_px = (sc[0].width or d.out_width) * (sc[0].height or d.out_height)
        out, surf4 = surfaces(bh, bw, 4)
        surf3 = (_lib.Surface * n)()
        for i in range(n):
            surf3[i].pixels, surf3[i].pitch = out[i].data_ptr(), bw * 6
        keep_out.append(out)

        def sdr(sc=sc, surf=surf4):
            _lib.check(_lib.lib.heifgpu_render_batch_scaled_color(ctx._h, imgs, n, planes, None, None, _lib.PIX_RGBA16, sc, xf,
                                                                  surf, stream))

        def hdr(fmt, surf, enc, sc=sc):
            def run():
                _lib.check(_lib.lib.heifgpu_render_batch_gain_scaled(ctx._h, imgs, n, planes, gimgs, gplanes, None, None, fmt,
                                                                     sc, gxf[enc], surf, stream))
            return run

        # bytes: the window's luma and chroma (1.5 per pixel), for HDR its quarter-size map (0.25), and the output
        variants += [(name, "scaled_sdr_rgba16", sdr, n * (window_px * 1.5 + bw * bh * 8)),
                     (name, "scaled_hdr_rgba16f", hdr(_lib.PIX_HDR_RGBA16F, surf4, "linear"), n * (window_px * 1.75 + bw * bh * 8)),
                     (name, "scaled_hdr_rgb16pq", hdr(_lib.PIX_HDR_RGB16PQ, surf3, "pq"), n * (window_px * 1.75 + bw * bh * 6))]
    result = {"images": n, "width": W, "height": HGT, "gain_width": gi.width, "gain_height": gi.height, "reps": args.reps,
              "runs": args.runs, "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK_GBS,
              "library": _lib.LIB_PATH.name, "transform": "Display P3 profile (halfmoonbay) -> sRGB; Apple rule, headroom 4",
              "cases": {}}
    for *_, fn, _ in variants:  # warm-up (and the tables' one upload)
        fn()
    torch.cuda.synchronize()
    ms = {(name, kind): [] for name, kind, _, _ in variants}
    for _ in range(args.runs):
        for name, kind, fn, _ in variants:
            ms[(name, kind)].append(timed(fn, args.reps))
    for name, kind, _, nbytes in variants:
        r = summary(ms[(name, kind)], nbytes)
        r["spread_ms"] = round(r["ms_max"] - r["ms_min"], 4)
        result["cases"].setdefault(name, {})[kind] = r
    full = result["cases"]["full"]
    for name, r in result["cases"].items():
        if name == "full":
            continue
        for enc in ("rgba16f", "rgb16pq"):
            r[f"hdr_{enc}_over_sdr"] = round(r[f"scaled_hdr_{enc}"]["ms_min"] / r["scaled_sdr_rgba16"]["ms_min"], 4)
            r[f"hdr_{enc}_of_full_hdr"] = round(r[f"scaled_hdr_{enc}"]["ms_min"] / full[f"full_hdr_{enc}"]["ms_min"], 4)
    for name, r in result["cases"].items():
        print(f"{name}: " + ", ".join(f"{k} min {v['ms_min']:.3f} ms (spread {v['spread_ms']:.3f})" for k, v in r.items()
                                      if isinstance(v, dict)) +
              "".join(f", {k} {v}" for k, v in r.items() if not isinstance(v, dict)), flush=True)
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def jpeg_main(args):
    """--jpeg: n copies of the golden twelve-megapixel picture to JPEG files in host memory
    (quality 90, 4:2:0).  "device": render() then encode_jpeg(), the files copied to the host;
    "pillow": render(), every surface copied to the host, Pillow's save() at the same settings,
    one picture after another on one core.  Wall-clock time per batch.  Beside them the encode
    call alone (events around heifgpu_jpeg_encode_batch, buffers allocated beforehand) for a
    restart interval of one MCU row and of 16 MCUs, which is what the default was chosen by."""
    import io
    import time

    from PIL import Image

    n = args.images
    ctx = H.DecodeContext(0)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    out = H.HeicDecoder.decode(golden)
    outs = [out] * n
    d = out.image.display
    result = {"images": n, "width": d.out_width, "height": d.out_height, "quality": 90, "subsampling": "4:2:0",
              "reps": args.reps, "runs": args.runs, "device": torch.cuda.get_device_name(0)}

    def wall(fn, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    files = {}

    def device_route(restart):
        def run():
            files[restart] = ctx.encode_jpeg(ctx.render(outs, "rgb8"), 90, "4:2:0", restart_mcus=restart)
        return run

    def pillow_route():
        res = []
        for t in ctx.render(outs, "rgb8"):
            b = io.BytesIO()
            Image.fromarray(t.cpu().numpy()).save(b, "JPEG", quality=90, subsampling="4:2:0")
            res.append(b.getvalue())
        files["pillow"] = res

    def render_only():
        ctx.render(outs, "rgb8")

    # the encode call alone
    rgb = ctx.render(outs, "rgb8")
    cap = d.out_width * d.out_height
    buf = torch.empty((n, cap), dtype=torch.uint8, device="cuda:0")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda:0")
    src, dst = ctx._surfaces(rgb), (_lib.Surface * n)()
    for i in range(n):
        dst[i].pixels, dst[i].pitch = buf[i].data_ptr(), cap
    ws, hs = (ctypes.c_uint32 * n)(*[d.out_width] * n), (ctypes.c_uint32 * n)(*[d.out_height] * n)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def call_of(restart):
        o = _lib.JpegOpts(90, _lib.JPEG_420, restart, 0)
        return lambda: _lib.check(_lib.lib.heifgpu_jpeg_encode_batch(
            ctx._h, n, src, ws, hs, ctypes.byref(o), dst, ctypes.cast(sizes.data_ptr(), ctypes.POINTER(ctypes.c_uint64)), stream))

    result["encode_call"] = {}
    for restart in (0, 16):
        fn = call_of(restart)
        fn()
        torch.cuda.synchronize()
        ms = [timed(fn, args.reps) for _ in range(args.runs)]
        total = int(sizes.sum().item())
        result["encode_call"][f"restart_{restart}"] = {
            "ms_per_batch": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "scan_bytes_per_picture": total // n}
        print(f"encode call, restart_mcus {restart}: {statistics.median(ms):.3f} ms per batch of {n} "
              f"(min {min(ms):.3f}, max {max(ms):.3f}), {total // n} scan bytes per picture", flush=True)
    del buf, rgb
    for name, fn, reps in (("render", render_only, args.reps), ("device_row", device_route(0), 2),
                           ("device_16", device_route(16), 2), ("pillow", pillow_route, 1)):
        fn()
        ms = [wall(fn, reps) for _ in range(min(args.runs, 3) if name != "pillow" else 1)]
        result[name] = {"ms_per_batch": round(statistics.median(ms), 2), "ms_min": round(min(ms), 2),
                        "ms_max": round(max(ms), 2), "ms_per_picture": round(statistics.median(ms) / n, 3)}
        print(f"{name}: {statistics.median(ms):.2f} ms per batch of {n}, {statistics.median(ms) / n:.3f} ms per picture",
              flush=True)
    result["file_bytes_per_picture"] = {k: sum(len(f) for f in v) // n for k, v in files.items()}
    result["pillow_over_device_row"] = round(result["pillow"]["ms_per_batch"] / result["device_row"]["ms_per_batch"], 2)
    result["pillow_over_device_16"] = round(result["pillow"]["ms_per_batch"] / result["device_16"]["ms_per_batch"], 2)
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def png_main(args):
    """--png: n copies of the golden twelve-megapixel picture to PNG files in host memory.
    "rgb8": render() then encode_png(), the files copied to the host.  "rgba16_10bit": the golden
    picture's decoded planes shifted up to 10 bits with two seeded random low bits, under a
    10-bit image of the same geometry, rendered opaque as rgba16 and encoded with bits=10 (the
    constant alpha is a flat region: a bit per byte).  "cpu_1" / "cpu_6": render(), a surface
    copied to the host, Pillow's save(compress_level=1 / 6) on one core (for the 16-bit RGBA
    pictures, which Pillow does not write: a Sub filter in numpy and zlib at that level), over
    --pillow-pictures pictures and scaled to n (said so in the result).  Wall-clock time per batch; beside it the
    encode call alone (events around heifgpu_png_encode_batch, buffers allocated beforehand).
    One picture of "flat" is the flat-region limitation measured: the golden picture with its left
    half fully transparent black, as rgba8, against Pillow."""
    import io
    import time
    import zlib

    import numpy as np
    from PIL import Image

    n = args.images
    dev = torch.device("cuda", 0)
    ctx = H.DecodeContext(0)
    golden = (ROOT / "tests" / "golden" / "halfmoonbay.heic").read_bytes()
    out = H.HeicDecoder.decode(golden)
    d = out.image.display
    result = {"images": n, "width": d.out_width, "height": d.out_height, "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0)}

    def wall(fn, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    # the 10-bit batch: the golden planes at 10 bits under a synthetic 10-bit image's handle
    p10 = S.SynthParams(bit_depth=10)
    img10 = H.HeifImage.parse(S.grid_heic(W, HGT, p10, pictures=[S.picture(p10, 1)] * 48))
    assert img10.info.bit_depth == 10 and (img10.info.width, img10.info.height) == (W, HGT)
    g = torch.Generator(device=dev).manual_seed(1)

    def deep(t):
        low = torch.randint(0, 4, t.shape, generator=g, device=dev, dtype=torch.int32)
        return ((t.to(torch.int32) << 2) | low).to(torch.int16)

    y10, cb10, cr10 = deep(out.y), deep(out.cb), deep(out.cr)
    planes10 = (_lib.Planes * n)()
    for i in range(n):
        for c, t in enumerate((y10, cb10, cr10)):
            planes10[i].plane[c] = t.data_ptr()
            planes10[i].pitch[c] = t.stride(0) * t.element_size()
    imgs10 = (ctypes.c_void_p * n)(*[img10._h.value] * n)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def render16(m):
        res = [torch.empty((HGT, W, 4), dtype=torch.int16, device=dev) for _ in range(m)]
        _lib.check(_lib.lib.heifgpu_render_batch(ctx._h, imgs10, m, planes10, None, None, _lib.PIX_RGBA16,
                                                 ctx._surfaces(res), stream))
        return res

    def pillow_png(a, level):
        b = io.BytesIO()
        Image.fromarray(a).save(b, "PNG", compress_level=level)
        return b.getvalue()

    def numpy_zlib_png(a, level):
        """Pillow writes no 16-bit RGBA: the big-endian replicated samples, every row filtered by Sub
        in numpy, through zlib at `level` (the IDAT payload a plain CPU writer would make)."""
        s = a.view(np.uint16).astype(np.uint32)
        v = ((s << 6) | (s >> 4)).astype(">u2")
        rows = v.reshape(v.shape[0], -1).view(np.uint8)
        sub = rows.copy()
        sub[:, 8:] -= rows[:, :-8]
        return zlib.compress(np.concatenate([np.ones((rows.shape[0], 1), np.uint8), sub], axis=1).tobytes(), level)

    files = {}
    routes = {
        "rgb8": (lambda m: ctx.render([out] * m, "rgb8"), lambda px: ctx.encode_png(px), 3, 8, pillow_png,
                 "Pillow save(compress_level=L)"),
        "rgba16_10bit": (render16, lambda px: ctx.encode_png(px, bits=10), 8, 10, numpy_zlib_png,
                         "numpy Sub filter + zlib level L (Pillow writes no 16-bit RGBA)"),
    }
    for name, (render, encode, bpp, bits, cpu_writer, cpu_name) in routes.items():
        # the encode call alone
        px = render(n)
        h, w = px[0].shape[0], px[0].shape[1]
        cap = ctx._png_first_guess(h * (w * bpp + 1))
        buf = torch.empty((n, (cap + 15) // 16 * 16), dtype=torch.uint8, device=dev)
        sizes = torch.empty(n, dtype=torch.int64, device=dev)
        src, dst = ctx._surfaces(px), (_lib.Surface * n)()
        for i in range(n):
            dst[i].pixels, dst[i].pitch = buf[i].data_ptr(), cap
        ws, hs = (ctypes.c_uint32 * n)(*[w] * n), (ctypes.c_uint32 * n)(*[h] * n)
        o = _lib.PngOpts(_lib.PIX_RGB8 if bpp == 3 else _lib.PIX_RGBA16, bits, 5, 0)

        def call():
            _lib.check(_lib.lib.heifgpu_png_encode_batch(ctx._h, n, src, ws, hs, ctypes.byref(o), dst,
                                                         ctypes.cast(sizes.data_ptr(), ctypes.POINTER(ctypes.c_uint64)), stream))

        call()
        torch.cuda.synchronize()
        ms = [timed(call, args.reps) for _ in range(args.runs)]
        total = int(sizes.sum().item())
        result[name] = {"encode_call": {"ms_per_batch": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
                                        "ms_max": round(max(ms), 3), "idat_bytes_per_picture": total // n}}
        print(f"{name}: encode call {statistics.median(ms):.3f} ms per batch of {n} (min {min(ms):.3f}, max {max(ms):.3f}), "
              f"{total // n} bytes per picture", flush=True)
        del buf, px

        def device_route():
            files[name] = encode(render(n))

        device_route()
        ms = [wall(device_route, 1) for _ in range(min(args.runs, 3))]
        result[name]["device"] = {"ms_per_batch": round(statistics.median(ms), 2), "ms_min": round(min(ms), 2),
                                  "ms_max": round(max(ms), 2), "ms_per_picture": round(statistics.median(ms) / n, 3)}
        result[name]["file_bytes_per_picture"] = {"device": sum(len(f) for f in files[name]) // n}
        print(f"{name}: render + encode_png {statistics.median(ms):.2f} ms per batch of {n}", flush=True)
        # the CPU route on one core over a few pictures, scaled to the batch
        k = max(1, min(args.pillow_pictures, n))
        result[name]["cpu_writer"] = cpu_name
        for level in (1, 6):
            def cpu_route():
                files[f"{name}_cpu_{level}"] = [cpu_writer(t.cpu().numpy(), level) for t in render(k)]
            ms1 = wall(cpu_route, 1)
            result[name][f"cpu_{level}"] = {"pictures_timed": k, "ms_per_picture": round(ms1 / k, 2),
                                            "ms_per_batch_scaled_to_n": round(ms1 / k * n, 1)}
            result[name]["file_bytes_per_picture"][f"cpu_{level}"] = sum(len(f) for f in files[f"{name}_cpu_{level}"]) // k
            print(f"{name}: {cpu_name}, L={level}: {ms1 / k:.1f} ms per picture on one core "
                  f"({k} timed; {ms1 / k * n:.0f} ms scaled to {n})", flush=True)
            result[name][f"cpu_{level}_over_device"] = round(result[name][f"cpu_{level}"]["ms_per_batch_scaled_to_n"] /
                                                             result[name]["device"]["ms_per_batch"], 2)
        torch.cuda.empty_cache()
    # the flat-region limitation: the left half fully transparent
    rgba = ctx.render([out], "rgba8")[0].clone()
    rgba[:, : rgba.shape[1] // 2] = 0
    ours = ctx.encode_png([rgba])[0]
    flat = {"device": len(ours)}
    for level in (1, 6):
        b = io.BytesIO()
        Image.fromarray(rgba.cpu().numpy()).save(b, "PNG", compress_level=level)
        flat[f"pillow_{level}"] = len(b.getvalue())
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours))), rgba.cpu().numpy())
    result["flat_half_transparent_rgba8_bytes"] = flat
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def linear_main(args):
    """--linear: the linear-light scaled renders (heifgpu_render_batch_scaled_linear / _tensor_linear,
    DESIGN 5.38) beside the encoded-managed calls (colorspace="srgb" as before: the rounded average
    transformed) on the same planes, Display P3 (halfmoonbay's profile) to sRGB, RGB8 and f16 CHW, to
    224 x 224 (cover) and to 1008 x 756 (stretch, 4 : 1), rotation 0 and 3, and RGB16 of a 10-bit and of a
    12-bit batch to 224 x 224 (the table placement of the 16-bit formats), the variants alternated in one process
    in each of the --runs runs.  linear / managed is reported, nothing is gated.  HEIFGPU_LIBRARY
    naming a build with another table placement (make variant VDEFS=-DHG_LIN_LDS8=0 or
    -DHG_LIN_LDS16=0) gives the other half of that A/B."""
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

    result = {"images": n, "width": W, "height": HGT, "reps": args.reps, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "library": os.environ.get("HEIFGPU_LIBRARY", "default"),
              "transform": "Display P3 profile (halfmoonbay) -> sRGB", "cases": {}}
    variants, keep = [], []
    L = _lib.lib

    def add_cases(tag, img, planes, bits, pix, boxes):
        d = img.display
        imgs = (ctypes.c_void_p * n)(*[img._h.value] * n)
        t = img.color_transform("srgb", bits)
        assert not t.identity
        xf = (ctypes.c_void_p * n)(*[ctypes.addressof(t)] * n)
        keep.extend([img, imgs, t, xf])
        wide = pix >= _lib.PIX_RGB16
        for box, bw, bh, mode in boxes:
            sc = (_lib.Scale * n)()
            for i in range(n):
                _lib.check(L.heifgpu_scale_fit(ctypes.byref(d), bw, bh, mode, ctypes.byref(sc[i])))
            out = torch.empty((n, bh, bw, 3), dtype=torch.int16 if wide else torch.uint8, device=dev)
            surf = (_lib.Surface * n)()
            for i in range(n):
                surf[i].pixels, surf[i].pitch = out[i].data_ptr(), out[i].stride(0) * out.element_size()
            keep.extend([sc, out, surf])
            for kind, fn in (("managed", L.heifgpu_render_batch_scaled_color), ("linear", L.heifgpu_render_batch_scaled_linear)):
                def run(fn=fn, sc=sc, surf=surf):
                    _lib.check(fn(ctx._h, imgs, n, planes, None, None, pix, sc, xf, surf, stream))
                variants.append((f"scaled{box}_{tag}", kind, run))
            if wide:
                continue
            tout = torch.empty((n, 3, bh, bw), dtype=torch.float16, device=dev)
            fmt = _lib.TensorFormat(src=pix, elem=_lib.ELEM_F16, layout=_lib.LAYOUT_CHW)
            for c, (m_, s_) in enumerate(zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
                fmt.a[c], fmt.b[c] = 1.0 / (255.0 * s_), -m_ / s_
            ts = (_lib.TensorSurface * n)()
            for i in range(n):
                ts[i].data, ts[i].stride_c, ts[i].stride_y = tout[i].data_ptr(), bh * bw * 2, bw * 2
            keep.extend([tout, fmt, ts])
            for kind, fn in (("managed", L.heifgpu_render_batch_tensor_color), ("linear", L.heifgpu_render_batch_tensor_linear)):
                def trun(fn=fn, sc=sc, ts=ts, fmt=fmt):
                    _lib.check(fn(ctx._h, imgs, n, planes, None, None, ctypes.byref(fmt), sc, None, xf, ts, stream))
                variants.append((f"tensor{box}_{tag}", kind, trun))

    planes8, keep8 = planes_of(torch.uint8, 256)
    for rot in (0, 3):
        img = H.HeifImage.parse(forced_rotation(golden, rot))
        big = ("1008", 1008, 756, _lib.FIT_STRETCH) if rot == 0 else ("1008", 756, 1008, _lib.FIT_STRETCH)
        add_cases(f"rgb8_rot{rot}", img, planes8, 8, _lib.PIX_RGB8, (("224", 224, 224, _lib.FIT_COVER), big))
    p10 = S.SynthParams(bit_depth=10)
    colr = S.icc_box(H.HeifImage.parse(golden).icc_profile)
    img10 = H.HeifImage.parse(S.grid_heic(W, HGT, p10, pictures=[S.picture(p10, 1)] * 48, colr=colr))
    planes10, keep10 = planes_of(torch.int16, 1024)
    add_cases("rgb16_10bit", img10, planes10, 10, _lib.PIX_RGB16, (("224", 224, 224, _lib.FIT_COVER),))
    p12 = S.SynthParams(bit_depth=12)
    img12 = H.HeifImage.parse(S.grid_heic(W, HGT, p12, pictures=[S.picture(p12, 1)] * 48, colr=colr))
    planes12, keep12 = planes_of(torch.int16, 4096)
    add_cases("rgb16_12bit", img12, planes12, 12, _lib.PIX_RGB16, (("224", 224, 224, _lib.FIT_COVER),))

    for *_, fn in variants:  # warm-up (and the tables' one upload)
        fn()
    torch.cuda.synchronize()
    ms = {(name, kind): [] for name, kind, _ in variants}
    for _ in range(args.runs):
        for name, kind, fn in variants:
            ms[(name, kind)].append(timed(fn, args.reps))
    for name, kind, _ in variants:
        v = ms[(name, kind)]
        result["cases"].setdefault(name, {})[kind] = {
            "ms_per_batch": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "ms_runs": [round(x, 4) for x in v], "spread_ms": round(max(v) - min(v), 4)}
    for name, r in result["cases"].items():
        r["linear_over_managed"] = round(r["linear"]["ms_per_batch"] / r["managed"]["ms_per_batch"], 4)
        r["linear_minus_managed_ms"] = round(r["linear"]["ms_per_batch"] - r["managed"]["ms_per_batch"], 4)
        print(f"{name}: " + ", ".join(f"{k} {r[k]['ms_per_batch']:.3f} ms (spread {r[k]['spread_ms']:.3f})"
                                      for k in ("managed", "linear")) + f", linear / managed {r['linear_over_managed']:.3f}",
              flush=True)
    print(json.dumps(result))
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--scaled", action="store_true", help="measure heifgpu_render_batch_scaled (see above)")
    ap.add_argument("--tensor", action="store_true", help="measure heifgpu_render_batch_tensor (see above)")
    ap.add_argument("--color", action="store_true", help="measure the colour-managed render (see above)")
    ap.add_argument("--filter", action="store_true", help="measure the bilinear / bicubic render (see above)")
    ap.add_argument("--tone", action="store_true", help="measure the tone stage of the HDR render (see above)")
    ap.add_argument("--chroma", choices=("replicate", "bilinear"), default=None,
                    help="measure the render, scaled and filtered calls with chroma upsampling set, beside replicate")
    ap.add_argument("--gain", action="store_true", help="measure the gain-map HDR render (see above)")
    ap.add_argument("--jpeg", action="store_true", help="measure render + encode_jpeg against render + copy + Pillow")
    ap.add_argument("--linear", action="store_true", help="measure the linear-light scaled renders beside the managed ones")
    ap.add_argument("--png", action="store_true", help="measure render + encode_png against render + copy + Pillow")
    ap.add_argument("--pillow-pictures", type=int, default=3, help="--png: pictures Pillow is timed over")
    args = ap.parse_args()
    if args.linear:
        return linear_main(args)
    if args.jpeg:
        return jpeg_main(args)
    if args.png:
        return png_main(args)
    if args.gain and args.scaled:
        return gain_scaled_main(args)
    if args.gain:
        return gain_main(args)
    if args.chroma:
        return chroma_main(args)
    if args.filter:
        return filter_main(args)
    if args.tone:
        return tone_main(args)
    if args.color:
        return color_main(args)
    if args.scaled:
        return scaled_main(args)
    if args.tensor:
        return tensor_main(args)
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
