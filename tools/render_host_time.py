"""Host time per render call: tiny pictures, so the wall time of a call is the library's host work
(checks, descriptors, ring slot, copy, launch, event).  Prints one JSON line, µs per call of the four
forms; run it once per library (HEIFGPU_LIBRARY names another build of the same ABI), DESIGN.md 5.26.

usage: python tools/render_host_time.py"""
import ctypes
import json
import os
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import heif_amd as H  # noqa: E402
from heif_amd import _lib, synth_encoder as S  # noqa: E402

lib = _lib.lib
N, CALLS, RUNS = 16, 2000, 5
ctx = H.DecodeContext(0)
data = S.single_heic(S.SynthParams(width=96, height=64, log2_ctb=4, log2_max_tb=4), seed=1)
img = H.HeifImage.parse(data)
imgs_py = [img] * N
outs = ctx.alloc_outputs(imgs_py)
b = ctx.prepare(imgs_py)
b.decode_async(outs)
torch.cuda.synchronize()
stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
imgs, _, _ = ctx._render_args(outs, None)
planes = ctx.planes_of(outs)
dev = torch.device("cuda", 0)
d = img.display
full = [torch.empty((d.out_height, d.out_width, 3), dtype=torch.uint8, device=dev) for _ in range(N)]
small = [torch.empty((32, 32, 3), dtype=torch.uint8, device=dev) for _ in range(N)]
tens = [torch.empty((3, 32, 32), dtype=torch.float16, device=dev) for _ in range(N)]


def surfaces(ts):
    s = (_lib.Surface * N)()
    for i, t in enumerate(ts):
        s[i].pixels, s[i].pitch = t.data_ptr(), t.stride(0) * t.element_size()
    return s


sf, ss = surfaces(full), surfaces(small)
st = (_lib.TensorSurface * N)()
for i, t in enumerate(tens):
    st[i].data, st[i].stride_c, st[i].stride_y = t.data_ptr(), t.stride(0) * 2, t.stride(1) * 2
scales = (_lib.Scale * N)()
for i in range(N):
    _lib.check(lib.heifgpu_scale_fit(ctypes.byref(d), 32, 32, _lib.FIT_MODES["cover"], ctypes.byref(scales[i])))
tf = _lib.TensorFormat(src=_lib.PIX_RGB8, elem=_lib.ELEM_F16, layout=_lib.LAYOUTS["chw"])
for c in range(3):
    tf.a[c], tf.b[c] = 1.0 / 255, 0.0
try:
    keep = [img.color_transform("display-p3", 8) for _ in range(N)]
    xf = (ctypes.c_void_p * N)(*[ctypes.addressof(t) for t in keep])
except Exception as e:  # a picture without a colour description the library transforms
    print("no colour form:", e, file=sys.stderr)
    xf = None
forms = {
    "plain": lambda: lib.heifgpu_render_batch(ctx._h, imgs, N, planes, None, None, _lib.PIX_RGB8, sf, stream),
    "color": lambda: lib.heifgpu_render_batch_color(ctx._h, imgs, N, planes, None, None, _lib.PIX_RGB8, xf, sf, stream),
    "scaled": lambda: lib.heifgpu_render_batch_scaled(ctx._h, imgs, N, planes, None, None, _lib.PIX_RGB8, scales, ss,
                                                      stream),
    "tensor": lambda: lib.heifgpu_render_batch_tensor(ctx._h, imgs, N, planes, None, None, ctypes.byref(tf), scales,
                                                      None, st, stream),
}
res = {"library": os.path.basename(str(_lib.LIB_PATH)), "images": N, "calls": CALLS, "us_per_call": {}}
if xf is None:
    del forms["color"]
for name, fn in forms.items():
    _lib.check(fn())
    torch.cuda.synchronize()
    runs = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / CALLS * 1e6)
    res["us_per_call"][name] = {"median": round(statistics.median(runs), 2), "runs": [round(r, 2) for r in runs]}
print(json.dumps(res))
