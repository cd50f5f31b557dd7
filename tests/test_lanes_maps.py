"""The deblocking maps of the lanes parse, on the host emulation.

The lanes parse no longer stores the edge / no-filter map (MF_*) while it parses: the
map is painted from the luma TB records after the parse (k_paint_flags), except the
blocks of PCM CUs.  The solo parse still writes the map as it goes.  So every picture
here is decoded twice through the emulation, lanes and solo, each run against the
oracle, and the QpY and flag maps that the deblocking read (the emulation's
HEIFGPU_EMU_DUMP_MAPS dump, which starts the arena from a sentinel byte so that a
block nobody wrote shows) have to be the same bytes."""
import os
import pathlib
import subprocess

import pytest

from conftest import make_emu

S = pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"

CASES = {
    "64x64": dict(width=64, height=64),
    # no multiple of the CTB: the map's last column and row of blocks are cropped at w4 / h4
    "72x40": dict(width=72, height=40, max_th_depth_intra=2, density=50),
    "72x40_ctb16": dict(width=72, height=40, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=2),
    # 8x8 CUs of four PBs (the transform tree splits once more)
    "nxn": dict(width=128, height=64, log2_max_tb=4, max_th_depth_intra=1, density=20),
    # sparse TUs in quantization groups of several: the first TUs of a group have no cbf and are
    # recorded with the predicted QpY, a later one carries cu_qp_delta (the QpY map takes the final value)
    "late_dqp": dict(width=128, height=64, cu_qp_delta=1, diff_cu_qp_delta_depth=1, density=10, max_th_depth_intra=2),
    "dqp_dense": dict(width=128, height=64, cu_qp_delta=1, diff_cu_qp_delta_depth=2, density=35),
    "pcm": dict(width=128, height=64, pcm=1, pcm_pct=30, pcm_lf_disabled=0),
    "pcm_lf_disabled": dict(width=128, height=64, pcm=1, pcm_pct=30, pcm_lf_disabled=1),
    "pcm_bypass": dict(width=128, height=64, pcm=1, pcm_pct=30, tq_bypass=1),
    "bypass": dict(width=128, height=64, tq_bypass=1, max_th_depth_intra=2),
    "c422": dict(width=128, height=64, chroma_format=2, max_th_depth_intra=2),
    "c444": dict(width=72, height=40, chroma_format=3, max_th_depth_intra=2),
    # HEVC tiles: every tile a picture of its own, the maps put together by k_assemble
    "tiles_2x2": dict(width=128, height=96, wpp=0, tile_cols=2, tile_rows=2),
    "tiles_3x2_wpp": dict(width=256, height=192, tile_cols=3, tile_rows=2),
    # dependent slice segments at CTB rows and inside them (tests/test_slices.py DEP_CASES)
    "dep_all_wpp": dict(width=128, height=96, slice_ctus=4, slice_dependent=1),
    "dep_mid_nowpp": dict(width=128, height=96, wpp=0, slice_ctus=5, slice_dependent=1),
}


@pytest.fixture(scope="module")
def emu_check():
    make_emu("emu-fast")
    return str(CSRC / "build" / "emu_fast" / "emu_check")


def _run(exe, heic, dump, mode, **env):
    r = subprocess.run([exe, str(heic), "5"], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "HEIFGPU_PARSE": mode, "HEIFGPU_EMU_DUMP_MAPS": str(dump), **env})
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "EMU PARITY OK" in out, (mode, out[-2000:])
    return out, dump.read_bytes()


@pytest.mark.parametrize("name", list(CASES))
def test_maps_equal_the_solo_parse(emu_check, tmp_path, name):
    p = S.SynthParams(**{**dict(log2_ctb=5, wpp=1), **CASES[name]})
    heic = tmp_path / "p.heic"
    heic.write_bytes(S.single_heic(p, seed=1))
    out_l, lanes = _run(emu_check, heic, tmp_path / "lanes.bin", "lanes")
    out_s, solo = _run(emu_check, heic, tmp_path / "solo.bin", "solo")
    assert "parse mode: lanes" in out_l, out_l[-1000:]
    if name != "dep_mid_nowpp":  # (segments inside CTB rows: a lanes parse whatever is asked)
        assert "parse mode: solo" in out_s, out_s[-1000:]
    assert len(lanes) == len(solo) and len(lanes) > 0
    bad = [i for i in range(len(lanes)) if lanes[i] != solo[i]]
    assert not bad, (len(bad), bad[:8], [(lanes[i], solo[i]) for i in bad[:8]])
    # both maps of every picture written throughout: nothing left of the arena's sentinel in the flags
    # (a flag byte is below 8; a QpY of -91 cannot occur)
    assert 0xa5 not in lanes


def test_maps_equal_in_the_general_body(emu_check, tmp_path):
    """The lean tool set's picture through the general body paints the same map."""
    p = S.SynthParams(**{**dict(log2_ctb=5, wpp=1), **CASES["72x40"]})
    heic = tmp_path / "p.heic"
    heic.write_bytes(S.single_heic(p, seed=2))
    out_a, lean = _run(emu_check, heic, tmp_path / "lean.bin", "lanes", HEIFGPU_LANES_VARIANT="auto")
    out_g, gen = _run(emu_check, heic, tmp_path / "gen.bin", "lanes", HEIFGPU_LANES_VARIANT="general")
    _, solo = _run(emu_check, heic, tmp_path / "solo.bin", "solo")
    assert "lanes variant: lean" in out_a and "lanes variant: general" in out_g
    assert lean == solo and gen == solo
