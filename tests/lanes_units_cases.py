"""Small pictures for the lanes parse's tree / TB units (tests/test_lanes_units.py on the
host emulation, tests/test_lanes_units_gpu.py on the device).

Every picture is 128x64 with 32x32 CTBs and WPP: two CTB rows of four CTUs, so
the context hand-off and the 2-CTU lag between a picture's two lanes are in
play.  The synthetic encoder draws the syntax at random (35 % of the smallest
CUs are NxN with four PBs, a third of the PBs take an MPM, 30 % of the
cu_qp_delta_abs values are drawn over the whole range, 30 % of the last
positions over the whole TB), so a case is a parameter set that makes the path
it is named for frequent.  The emulation counts those paths (the `paths` line
of HEIFGPU_LANES_STATS, enum Cov of kernels/parse_state.hpp), and NEEDS names
the ones each case's first picture has to reach, which the CPU test asserts.

Run as a program with a device (`python tests/lanes_units_cases.py`, which
is what the GPU test does, once per pictures-per-wave setting because the
library reads HEIFGPU_LANES_PPW once per process) it decodes the cases as
batches forced to the lanes parse, in the lean and the general body, and
compares every plane with the oracle."""
import os
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

BASE = dict(width=128, height=64, log2_ctb=5, wpp=1)

# inside the lean tool set (4:2:0, no transform_skip / PCM / bypass): run in both bodies
LEAN = {
    # luma TBs of 32, 16, 8 and 4, chroma TBs of 16, 8 and 4 (32x32 CUs down to 8x8, two tree levels)
    "tb_sizes": dict(log2_max_tb=5, log2_min_tb=2, max_th_depth_intra=2, density=35),
    # 8x8 CUs (a 16x16 CTB would leave the 2 x 4 CTU layout; min CB 8 in 32x32 CTBs): NxN with four PBs,
    # MPM (mpm_idx 0, 1, 2) and non-MPM modes side by side
    "nxn": dict(log2_max_tb=4, max_th_depth_intra=1, density=20, cu_qp_delta=0),
    # a quantization group per 8x8: many cu_qp_delta_abs, the values of 5 and above take the EG0 suffix
    "dqp_eg0": dict(cu_qp_delta=1, diff_cu_qp_delta_depth=2, density=35),
    # dense 16x16 and 32x32 TBs: last positions above 3 take suffix bits (1 to 3 of them)
    "last_suffix": dict(log2_max_tb=5, max_th_depth_intra=1, density=60, cu_qp_delta=0),
    # 32x32 CUs of one TB each, every TB coded: last_sig_coeff prefixes of 9, which take the fifth context
    "last_32": dict(log2_min_cb=5, max_th_depth_intra=0, density=100, cu_qp_delta=0, diff_cu_qp_delta_depth=0),
    # sparse: most TBs have no coefficients and are followed by coded ones of the same TU / CU
    "no_coef": dict(density=10, sign_hiding=0, cu_qp_delta=1),
    # every TB coded and no transform tree below the CU: each CU ends at its Cr TB's last sub-block
    "cu_ends_in_sb": dict(max_th_depth_intra=0, density=100, cu_qp_delta=0, sign_hiding=1),
}
# outside it: the general body only
GENERAL = {
    "c422": dict(chroma_format=2, max_th_depth_intra=2),
    "c444": dict(chroma_format=3, max_th_depth_intra=2),  # chroma TBs up to 32, NxN chroma modes per PB
    "tskip": dict(transform_skip=1, max_th_depth_intra=2, density=50),
}
SEEDS = (1, 2, 3)  # three pictures of a case: one wave at three pictures per wave
# the picture of a case that the emulation runs (c444: seed 2 has 32x32 chroma TBs)
CPU_SEED = {"c444": 2}

# the emulation's path counters, in the order of its `paths` line (enum Cov)
PATHS = ("luma4", "luma8", "luma16", "luma32", "chroma4", "chroma8", "chroma16", "chroma32", "nxn", "nxn_mpm0",
         "nxn_mpm1", "nxn_mpm2", "nxn_rem", "dqp", "dqp_eg0", "last_suffix", "coded_after_empty", "cu_ends_in_sb",
         "tskip", "last_ctx5")
NEEDS = {
    "tb_sizes": ("luma4", "luma8", "luma16", "luma32", "chroma4", "chroma8", "chroma16"),
    "nxn": ("nxn", "nxn_mpm0", "nxn_mpm1", "nxn_mpm2", "nxn_rem"),
    "dqp_eg0": ("dqp", "dqp_eg0"),
    "last_suffix": ("last_suffix",),
    "last_32": ("luma32", "chroma16", "last_ctx5"),
    "no_coef": ("coded_after_empty",),
    "cu_ends_in_sb": ("cu_ends_in_sb",),
    "c422": ("chroma4", "chroma8", "chroma16", "nxn"),
    "c444": ("chroma4", "chroma8", "chroma16", "chroma32", "nxn"),
    "tskip": ("tskip",),
}


def heic(over, seed=1):
    from heif_amd import synth_encoder as S

    return S.single_heic(S.SynthParams(**{**BASE, **over}), seed=seed)


def _decode_batch(H, ctx, np, oracle, datas, variant, want):
    os.environ["HEIFGPU_LANES_VARIANT"] = variant
    imgs = [H.HeifImage.parse(d) for d in datas]
    b = ctx.prepare(imgs, parse="lanes")
    try:
        geom = b.parse_geometry()
        assert geom["mode"] == "lanes", geom
        ppw = int(os.environ.get("HEIFGPU_LANES_PPW", "0"))
        assert not ppw or geom["pics_per_wave"] == ppw, geom
        assert b.lanes_variant() == want, (b.lanes_variant(), want)
        outs = ctx.alloc_outputs(imgs)
        b.decode_async(outs)
        assert not any(b.status()), b.status()
    finally:
        b.free()
    for k, (d, o) in enumerate(zip(datas, outs)):
        ref = oracle(d)
        for g, r, c in zip((o.y, o.cb, o.cr), (ref.y, ref.cb, ref.cr), "YUV"):
            g = g.cpu().numpy().astype(np.uint16)
            assert g.shape == r.shape and np.array_equal(g, r), (variant, k, c)
    return geom


def run_gpu():
    """Every case as batches on the device, pictures per wave as HEIFGPU_LANES_PPW says."""
    import numpy as np
    import torch

    import heif_amd as H
    from oracle import oracle

    assert torch.cuda.is_available(), "needs a HIP device"
    refs = {}

    def ref(d):
        if d not in refs:
            refs[d] = oracle.decode_heic(d, with_checks=False)
        return refs[d]

    ctx = H.DecodeContext(0)
    try:
        # the lean set in one batch (18 pictures), in both bodies
        lean = [heic(over, s) for over in LEAN.values() for s in SEEDS]
        for variant, want in (("auto", "lean"), ("general", "general")):
            geom = _decode_batch(H, ctx, np, ref, lean, variant, want)
            print(f"lean set, {variant}: {geom}")
        for name, over in GENERAL.items():  # (a batch shares one chroma format)
            geom = _decode_batch(H, ctx, np, ref, [heic(over, s) for s in SEEDS], "auto", "general")
            print(f"{name}: {geom}")
    finally:
        ctx.close()
    print("LANES UNITS GPU OK")


if __name__ == "__main__":
    run_gpu()
