"""Small pictures for the lanes parse's sub-block unit (tests/test_lanes_sb.py on the host
emulation, tests/test_lanes_sb_gpu.py on the device), in the manner of
tests/lanes_units_cases.py.

Every picture is 128x64 with 32x32 CTBs and WPP (two CTB rows of four CTUs).  The
synthetic encoder draws the syntax at random (levels with a long tail: 10 % of them
up to 200 or 3000, so Rice parameters reach 4 and levels escape), so a case is a
parameter set that makes the path it is named for frequent, or that excludes the
other paths.  The emulation counts the paths of the unit (the `sb_paths` line of
HEIFGPU_LANES_STATS, the COV_SB_ entries of enum Cov in kernels/parse_state.hpp, next
to the `paths` line of the TB sizes); NEEDS names the counters a case has to reach and
ZERO the ones it must not, which the CPU test asserts.

For three pictures per wave the emulation, which decodes one file, gets the three
pictures of a case as the tiles of one grid image (`grid`); the device gets them as a
batch of three files.

Run as a program with a device (`python tests/lanes_sb_cases.py`, once per
pictures-per-wave setting: the library reads HEIFGPU_LANES_PPW once per process) it
decodes the cases as batches forced to the lanes parse, in the lean and the general
body, and compares every plane with the oracle."""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BASE = dict(width=128, height=64, log2_ctb=5, wpp=1, cu_qp_delta=0)

# every case is inside the lean tool set (4:2:0, no transform_skip / PCM / bypass): both bodies run it
CASES = {
    # a largest TB of 4x4: every transform tree splits down to 4x4 luma TBs, with the two 4x4 chroma
    # TBs of each 8x8 node (one sub-block per TB, nine significance contexts)
    "tb4_only": dict(log2_max_tb=2, max_th_depth_intra=1, density=60),
    # 32x32 CUs without a transform tree below them: luma TBs of 32, or 16 under NxN, chroma TBs of 16
    # and 8 (the encoder's smallest TB is 4x4, so the sizes are kept up through the CU size).  No 4x4
    # TB in any picture, so no unit run holds one
    "tb_large": dict(log2_min_cb=5, max_th_depth_intra=0, density=50, diff_cu_qp_delta_depth=0),
    # every size side by side: 4x4 and larger TBs in the same unit run (the nine-slot loop with four-slot lanes)
    "tb_mixed": dict(log2_min_tb=2, log2_max_tb=5, max_th_depth_intra=2, density=45),
    # every TB coded and dense: more than eight significant coefficients, long remainder chains
    # (Rice parameter 4, EGk suffixes, escapes), sign hiding with the first and last far apart
    "dense_hide": dict(max_th_depth_intra=1, density=100, sign_hiding=1),
    # the same without sign hiding: every sign decoded
    "dense_nohide": dict(max_th_depth_intra=1, density=100, sign_hiding=0),
    # sparse: single coefficients (sign hiding on but not applied), last positions at 0, inferred DCs
    "sparse": dict(max_th_depth_intra=2, density=12, sign_hiding=1),
}
SEEDS = (1, 2, 3)  # three pictures of a case: one wave at three pictures per wave

# the emulation's sub-block path counters, in the order of its `sb_paths` line
SB_PATHS = ("sig4", "sig", "beyond8", "rice4", "escape", "egk", "hide", "no_hide", "ctxset_inc", "infer_dc",
            "last_pos0", "gt2", "run_any4", "run_no4")
# (TB size counters of the `paths` line: lanes_units_cases.PATHS)
NEEDS = {
    "tb4_only": ("luma4", "chroma4", "sig4", "run_any4", "beyond8", "escape", "gt2"),
    "tb_large": ("luma16", "luma32", "chroma8", "chroma16", "sig", "run_no4", "ctxset_inc", "beyond8"),
    "tb_mixed": ("luma4", "luma8", "luma16", "chroma4", "chroma8", "sig4", "sig", "run_any4", "ctxset_inc", "last_pos0"),
    "dense_hide": ("beyond8", "rice4", "escape", "egk", "hide", "gt2", "ctxset_inc"),
    "dense_nohide": ("beyond8", "rice4", "escape", "egk", "gt2"),
    "sparse": ("hide", "no_hide", "last_pos0", "infer_dc", "ctxset_inc", "sig4", "sig"),
}
ZERO = {
    "tb4_only": ("luma8", "luma16", "luma32", "chroma8", "chroma16", "chroma32", "sig", "run_no4"),
    "tb_large": ("luma4", "luma8", "chroma4", "sig4", "run_any4"),
    "dense_nohide": ("hide", "no_hide"),
}


def params(over):
    from heif_amd import synth_encoder as S

    return S.SynthParams(**{**BASE, **over})


def heic(over, seed=1):
    from heif_amd import synth_encoder as S

    return S.single_heic(params(over), seed=seed)


def grid(over):
    """The case's three pictures as the tiles of one 384x64 grid image."""
    from heif_amd import synth_encoder as S

    p = params(over)
    return S.grid_heic(3 * p.width, p.height, p, pictures=[S.picture(p, s) for s in SEEDS])


def run_gpu():
    """Every case as batches on the device, pictures per wave as HEIFGPU_LANES_PPW says."""
    import numpy as np
    import torch

    import heif_amd as H
    import lanes_units_cases as U
    from oracle import oracle

    assert torch.cuda.is_available(), "needs a HIP device"
    refs = {}

    def ref(d):
        if d not in refs:
            refs[d] = oracle.decode_heic(d, with_checks=False)
        return refs[d]

    ctx = H.DecodeContext(0)
    try:
        # every case in one batch (18 pictures), in both bodies
        every = [heic(over, s) for over in CASES.values() for s in SEEDS]
        for variant, want in (("auto", "lean"), ("general", "general")):
            geom = U._decode_batch(H, ctx, np, ref, every, variant, want)
            print(f"all cases, {variant}: {geom}")
        # the pictures without a 4x4 TB as a batch of their own: no unit run of any wave holds one
        large = [heic(CASES["tb_large"], s) for s in SEEDS]
        for variant, want in (("auto", "lean"), ("general", "general")):
            geom = U._decode_batch(H, ctx, np, ref, large, variant, want)
            print(f"tb_large, {variant}: {geom}")
    finally:
        ctx.close()
    print("LANES SB GPU OK")


if __name__ == "__main__":
    run_gpu()
