"""Small pictures for the lanes parse's CU lists and word-wise neighbour lines.

The vector engines append one word per CU to the CTB row's CU list and k_paint_flags
paints the QpY map from the words; a CU's segments of the IntraPredModeY, CtDepth and
QpY lines are updated as masked 64-bit words.  The pictures reach what can go wrong there:
- cu64: a picture that is one whole-CTB 64x64 CU (the 16-row paint, both words of an
  IntraPredModeY line, the mask that fills a word); cu64_mixed: such CUs beside CUs of every
  other size, which read the lines they left (3 x 2 CTBs);
- 72x40 at CTBs of 64 and of 16: the paint clipped at the map's last column and row, the
  forced splits at the picture's edges;
- mincb16: no 8x8 CU (the smallest run of a line is two bytes; its NxN CUs have 8x8 PBs),
  no cu_qp_delta;
- nxn_qg: 8x8 CUs of four PBs in quantization groups smaller than the CTB;
- lean: the lean tool set's picture, run in both bodies;
- c422 (device only): a 4:2:2 picture.
CU_PATHS names the counters of the emulation's `cu_paths` line (HEIFGPU_LANES_STATS; the
COV_CU_DONE entries of enum Cov in kernels/parse_state.hpp), NEEDS what each case must reach.
Run as a program it decodes the cases on the device (tests/test_lanes_culist_gpu.py)."""
import os
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = {
    "cu64": dict(width=64, height=64, log2_ctb=6, max_th_depth_intra=1, density=4),
    "cu64_mixed": dict(width=192, height=128, log2_ctb=6, max_th_depth_intra=1, density=4),
    "72x40_ctb64": dict(width=72, height=40, log2_ctb=6, max_th_depth_intra=1, density=20),
    "72x40_ctb16": dict(width=72, height=40, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=1),
    "mincb16": dict(width=64, height=64, log2_ctb=5, log2_min_cb=4, cu_qp_delta=0),
    "nxn_qg": dict(width=128, height=64, log2_ctb=5, diff_cu_qp_delta_depth=2, max_th_depth_intra=1, log2_max_tb=4,
                   density=20),
    "lean": dict(width=128, height=64, log2_ctb=5, max_th_depth_intra=2),
}
C422 = dict(width=128, height=64, log2_ctb=5, chroma_format=2, max_th_depth_intra=2)
SEEDS = {"cu64": 3, "cu64_mixed": 2, "72x40_ctb64": 2, "72x40_ctb16": 1, "mincb16": 2, "nxn_qg": 1, "lean": 1}
# the `cu_paths` line: CUs of 8, 16, 32 and 64 samples that reached cu_done; "nxn" is on the `paths` line
CU_PATHS = ("cu8", "cu16", "cu32", "cu64")
NEEDS = {
    "cu64": ("cu64",),
    "cu64_mixed": ("cu8", "cu16", "cu32", "cu64", "nxn"),
    "72x40_ctb64": ("cu8", "cu16", "cu32"),
    "72x40_ctb16": ("cu8", "cu16"),
    "mincb16": ("cu16", "cu32", "nxn"),
    "nxn_qg": ("cu8", "nxn"),
    "lean": ("cu8", "cu16", "cu32"),
}
ZERO = {"cu64": ("cu8", "cu16", "cu32"), "mincb16": ("cu8",), "72x40_ctb16": ("cu32", "cu64")}


def params(over):
    from heif_amd import synth_encoder as S

    return S.SynthParams(**{**dict(wpp=1), **over})


def heic(name):
    from heif_amd import synth_encoder as S

    return S.single_heic(params(CASES[name]), seed=SEEDS[name])


def run_gpu():
    """The 4:2:0 cases in one batch and the 4:2:2 picture in another, lanes parse, against the
    oracle; each batch decoded four times (a batch has at most three parse-output sets, so the
    last decode writes the set the first one used: a stale CU word or count would show)."""
    import numpy as np
    import torch

    import heif_amd as H
    from heif_amd import synth_encoder as S
    from oracle import oracle

    assert torch.cuda.is_available(), "needs a HIP device"
    os.environ.pop("HEIFGPU_LANES_VARIANT", None)
    ctx = H.DecodeContext(0)
    try:
        for label, datas in (("420", [heic(n) for n in CASES]), ("422", [S.single_heic(params(C422), seed=1)])):
            refs = [oracle.decode_heic(d, with_checks=False) for d in datas]
            imgs = [H.HeifImage.parse(d) for d in datas]
            b = ctx.prepare(imgs, parse="lanes")
            try:
                assert b.parse_geometry()["mode"] == "lanes", b.parse_geometry()
                outs = ctx.alloc_outputs(imgs)
                for rep in range(4):
                    b.decode_async(outs)
                    assert not any(b.status()), (label, rep, b.status())
                    if rep not in (0, 3):
                        continue
                    for k, (o, ref) in enumerate(zip(outs, refs)):
                        for g, r, c in zip((o.y, o.cb, o.cr), (ref.y, ref.cb, ref.cr), "YUV"):
                            g = g.cpu().numpy().astype(np.uint16)
                            assert g.shape == r.shape and np.array_equal(g, r), (label, rep, k, c)
            finally:
                b.free()
            print(f"{label}: {len(datas)} pictures, 4 decodes")
    finally:
        ctx.close()
    print("LANES CULIST GPU OK")


if __name__ == "__main__":
    run_gpu()
