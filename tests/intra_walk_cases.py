"""Small pictures for k_intra's block walk over packed record words.

A wave loads its row's TU records 64 at a time, forms each record's facts as packed words
(kernels/intra_rec.hpp) and walks the block by two masks: the records that are its own and
the records that open a CTU.  The pictures reach what can go wrong there:
- walk events (the emulation's `intra_walk` line, HEIFGPU_INTRA_STATS=1): a Cb TB in lane 63
  whose Cr TB opens the next block (the unpaired path), a CTU start at lane 0 of a later
  block, a block without a CTU start, a row of fewer than 64 and one of more than 128
  records, more CTB rows than a workgroup has waves (a wave takes a second row);
- geometry: 72x40 at CTBs of 64 and of 16 (partial CTUs on both edges, the write-back that
  is not full width), a picture that is one 8x8 CU;
- formats: 4:0:0, 4:2:0, 4:2:2, 4:4:4, 8 and 10 bits;
- tools: PCM CUs, cu_transquant_bypass CUs, 32x32 luma TBs under strong intra smoothing,
  NxN CUs of four 4x4 luma TBs.
NEEDS names the counters a case must reach.  Run as a program it decodes the cases on the
device (tests/test_intra_walk_gpu.py): a batch per sample format, each decoded twice, and one
picture through the streaming kernel."""
import os
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = {
    # walk events
    "wide_ctb16": dict(width=512, height=32, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=1, density=60),
    "wide_ctb32": dict(width=512, height=64, log2_ctb=5, max_th_depth_intra=1, density=60),
    "dense_ctb64": dict(width=128, height=64, log2_ctb=6, max_th_depth_intra=1, density=60),
    "tall_ctb16": dict(width=32, height=288, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=1),
    # geometry
    "72x40_ctb64": dict(width=72, height=40, log2_ctb=6, max_th_depth_intra=1, density=20),
    "72x40_ctb16": dict(width=72, height=40, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=1),
    "cu8": dict(width=8, height=8, log2_ctb=4, log2_max_tb=4),
    # tools
    "pcm": dict(width=64, height=64, log2_ctb=5, pcm=1, pcm_pct=30),
    "bypass": dict(width=64, height=64, log2_ctb=5, tq_bypass=1),
    "strong32": dict(width=128, height=128, log2_ctb=5, strong_intra=1, density=4),
    "nxn": dict(width=128, height=64, log2_ctb=5, diff_cu_qp_delta_depth=2, max_th_depth_intra=1, log2_max_tb=4,
                density=20),
    # formats (a batch shares one, so each is a batch of its own on the device)
    "c400": dict(width=128, height=64, log2_ctb=5, chroma_format=0, max_th_depth_intra=2),
    "c422": dict(width=128, height=64, log2_ctb=5, chroma_format=2, max_th_depth_intra=2),
    "c444": dict(width=128, height=64, log2_ctb=5, chroma_format=3, max_th_depth_intra=2),
    "c420_10": dict(width=72, height=40, log2_ctb=5, bit_depth=10, max_th_depth_intra=1),
    "c444_10": dict(width=72, height=40, log2_ctb=5, chroma_format=3, bit_depth=10, max_th_depth_intra=1),
}
SEEDS = {n: 1 for n in CASES}
# the `intra_walk` line's counters, in its order
COUNTERS = ("records", "ok", "pairs", "ctus", "blocks", "pair_splits", "ctu_lane0", "blocks_no_ctu", "rows_lt64",
            "rows_gt128", "second_rows", "tb32_strong", "luma4", "pcm")
NEEDS = {
    "wide_ctb16": ("ctu_lane0", "rows_gt128", "pairs"),
    "wide_ctb32": ("pair_splits", "rows_gt128", "pairs"),
    "dense_ctb64": ("blocks_no_ctu",),
    "tall_ctb16": ("second_rows", "rows_lt64"),
    "cu8": ("rows_lt64",),
    "pcm": ("pcm",),
    "strong32": ("tb32_strong",),
    "nxn": ("luma4",),
}
# every walk event the set must contain at least once
EVENTS = ("pair_splits", "ctu_lane0", "blocks_no_ctu", "rows_lt64", "rows_gt128", "second_rows")


def params(over):
    from heif_amd import synth_encoder as S

    return S.SynthParams(**{**dict(wpp=1), **over})


def heic(name):
    from heif_amd import synth_encoder as S

    return S.single_heic(params(CASES[name]), seed=SEEDS[name])


def batches():
    """The cases by sample format: {(chroma_format, bit_depth): [names]}."""
    out = {}
    for n, c in CASES.items():
        out.setdefault((c.get("chroma_format", 1), c.get("bit_depth", 8)), []).append(n)
    return out


def _same(o, ref, what):
    import numpy as np

    planes = ((o.y, ref.y, "Y"),) if ref.cb is None or o.cb is None else ((o.y, ref.y, "Y"), (o.cb, ref.cb, "Cb"),
                                                                         (o.cr, ref.cr, "Cr"))
    for g, r, c in planes:
        g = g.cpu().numpy().astype(np.uint16)
        assert g.shape == r.shape and np.array_equal(g, r), (what, c)


def run_gpu():
    """Every batch through the lanes parse, k_transform and k_intra, decoded twice, and one picture
    through k_intra_stream (spread parse), twice; every plane against the oracle.  The luma /
    chroma wave split is whatever HEIFGPU_INTRA_SPLIT says (read once per process)."""
    import torch

    import heif_amd as H
    from oracle import oracle

    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = H.DecodeContext(0)
    try:
        for (cf, bd), names in batches().items():
            datas = [heic(n) for n in names]
            refs = [oracle.decode_heic(d, with_checks=False) for d in datas]
            imgs = [H.HeifImage.parse(d) for d in datas]
            b = ctx.prepare(imgs, parse="lanes")
            try:
                outs = ctx.alloc_outputs(imgs)
                for rep in range(2):
                    b.decode_async(outs)
                    assert not any(b.status()), (cf, bd, rep, b.status())
                    for n, o, ref in zip(names, outs, refs):
                        _same(o, ref, (n, rep))
            finally:
                b.free()
            print(f"format {cf} depth {bd}: {len(names)} pictures, 2 decodes")
        data = heic("wide_ctb32")
        ref = oracle.decode_heic(data, with_checks=False)
        img = H.HeifImage.parse(data)
        b = ctx.prepare([img], parse="spread")
        try:
            outs = ctx.alloc_outputs([img])
            for rep in range(2):
                b.decode_async(outs)
                assert b.status() == [0], (rep, b.status())
                _same(outs[0], ref, ("stream", rep))
        finally:
            b.free()
        print("streaming: 1 picture, 2 decodes")
    finally:
        ctx.close()
    print("INTRA WALK GPU OK split=" + os.environ.get("HEIFGPU_INTRA_SPLIT", "auto"))


if __name__ == "__main__":
    run_gpu()
