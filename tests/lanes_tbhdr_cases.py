"""Small pictures for the residual header of the lanes parse's TB unit: the
last_sig_coeff_{x,y}_prefix loops, their suffixes and the swapped scan, in
the manner of tests/lanes_sb_cases.py (tests/test_lanes_tbhdr.py on the host emulation,
tests/test_lanes_tbhdr_gpu.py on the device).

Every picture is 128x64 with 32x32 CTBs and WPP (two CTB rows of four CTUs).  The
synthetic encoder draws the last position at random (70 % within the first eight
columns and rows, 30 % over the whole TB), so a case is a parameter set under which
the prefix pairs it is named for are frequent.  The emulation counts them (the
`tb_paths` line of HEIFGPU_LANES_STATS, the COV_LAST_ entries of enum Cov in
kernels/parse_state.hpp, next to the `paths` line of the TB sizes); NEEDS names the
counters the case has to reach, which the CPU test asserts.

The context of a prefix bin is CTX_LAST_X/Y + offset + (prefix >> shift) with the
offset and shift of the TB's component and size, so the sizes 4 to 32 of luma and of
chroma are all among the cases, and a case runs alone and as the three tiles of one
grid image in one wave, where the lanes of a unit run sit in different TBs and so at
different bins of the loops.

Run as a program with a device (`python tests/lanes_tbhdr_cases.py`, once per
pictures-per-wave setting: the library reads HEIFGPU_LANES_PPW once per process) it
decodes the cases as batches forced to the lanes parse, in the lean and the general
body, and compares every plane after deblocking and SAO with the oracle."""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BASE = dict(width=128, height=64, log2_ctb=5, wpp=1, cu_qp_delta=0)

# inside the lean tool set (4:2:0, no transform_skip / PCM / bypass): run in both bodies
LEAN = {
    # luma TBs of 32, 16, 8 and 4, chroma TBs of 16, 8 and 4, most of them coded: every (offset, shift)
    # of 4:2:0, the corner prefix pairs, suffixes on one axis, the swapped scan of 4x4 and 8x8 TBs
    "sizes": dict(log2_max_tb=5, log2_min_tb=2, max_th_depth_intra=2, density=70),
    # a largest TB of 4x4 (cMax 3, no suffix): (3, 3) ends both prefixes without a terminating bin
    "tb4": dict(log2_max_tb=2, max_th_depth_intra=1, density=80),
    # 32x32 CUs of one TB each, every TB coded: prefixes of 9 (the fifth context of 32x32 luma), 16x16 chroma
    "tb32": dict(log2_min_cb=5, max_th_depth_intra=0, density=100, diff_cu_qp_delta_depth=0),
}
# outside it: the general body only
GENERAL = {
    "c444": dict(chroma_format=3, max_th_depth_intra=2, density=70),  # chroma TBs up to 32, swapped chroma 8x8
    "c422": dict(chroma_format=2, max_th_depth_intra=2, density=70),  # two stacked chroma TBs per component
}
SEEDS = (1, 2, 3)  # three pictures of a case: one wave at three pictures per wave

# the emulation's last-position counters, in the order of its `tb_paths` line
TB_PATHS = ("last_00", "last_0m", "last_m0", "last_mm", "suffix_x_only", "suffix_y_only", "swap")
# (TB size counters, last_suffix and last_ctx5 of the `paths` line: lanes_units_cases.PATHS)
CORNERS = ("last_00", "last_0m", "last_m0", "last_mm")
NEEDS = {
    "sizes": ("luma4", "luma8", "luma16", "luma32", "chroma4", "chroma8", "chroma16", "last_suffix",
              "suffix_x_only", "suffix_y_only", "swap") + CORNERS,
    "tb4": ("luma4", "chroma4", "swap") + CORNERS,
    "tb32": ("luma32", "chroma16", "last_ctx5", "last_suffix", "suffix_x_only", "suffix_y_only"),
    "c444": ("luma32", "chroma4", "chroma8", "chroma16", "chroma32", "last_suffix", "swap") + CORNERS,
    "c422": ("chroma4", "chroma8", "last_suffix", "swap") + CORNERS,
}
ZERO = {
    "tb4": ("luma8", "luma16", "luma32", "chroma8", "chroma16", "chroma32", "last_suffix", "suffix_x_only",
            "suffix_y_only"),
    "tb32": ("swap",),  # (no TB small enough for the mode-dependent scan)
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
        # the lean set in one batch (9 pictures), in both bodies
        lean = [heic(over, s) for over in LEAN.values() for s in SEEDS]
        for variant, want in (("auto", "lean"), ("general", "general")):
            geom = U._decode_batch(H, ctx, np, ref, lean, variant, want)
            print(f"lean set, {variant}: {geom}")
        for name, over in GENERAL.items():  # (a batch shares one chroma format)
            geom = U._decode_batch(H, ctx, np, ref, [heic(over, s) for s in SEEDS], "auto", "general")
            print(f"{name}: {geom}")
    finally:
        ctx.close()
    print("LANES TBHDR GPU OK")


if __name__ == "__main__":
    run_gpu()
