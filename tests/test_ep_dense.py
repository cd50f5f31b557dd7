"""Streams dense in emulation-prevention bytes, end to end.

The synthetic streams of the other modules hold next to no
emulation_prevention_three_bytes (none in the 1.5 MB of test_synth.py's cases),
so k_rbsp's compaction and its entry-point remap behind removed bytes see
nothing of them there.  With pcm_mask = 3 every PCM sample is 0..3 and the
generator has to escape about one payload byte in 25.  Each stream below goes
through the oracle, the kernels compiled for the host (emu_check) and the
library on the GPU, in the three parse modes, bit-exact against the oracle.

Two conditions keep the streams from going soft, both counted by the model of
tests/rbsp_ref.py on the bytes the generator wrote: every substream but the
picture's first holds a removed byte (so every later entry point lies behind
one), and at least 2 % of the payload bytes are removed ones.  The seeds were
chosen so that the generator meets both.

The last part puts emulation-prevention bytes INTO the slice header: a WPP
picture's header re-emitted with 32-bit entry point offsets.
"""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import rbsp_ref as ref
from conftest import make_emu
from hevc_tiles import BitWriter, _ep, _nal_units, slice_header
from test_slices import DEP_CASES

S = pytest.importorskip("heif_amd.synth_encoder")

DEP = dict(DEP_CASES)
DEP_WPP = ["dep_all_wpp", "dep_alt_wpp", "dep_crop_10b_dbk", "dep_alt_across", "dep_mid_wpp", "dep_mid_wpp_10b_dbk",
           "dep_mid_wpp_ctb16_tall", "dep_mid_wpp_c422"]
DEP_NOWPP = ["dep_all_nowpp", "dep_alt_nowpp_ctb16_pcm", "dep_mid_nowpp", "dep_mid_1ctu_10b", "dep_mid_ctb16_pcm",
             "dep_mid_c444_across"]
assert sorted(DEP_WPP + DEP_NOWPP) == sorted(DEP) and all(bool(DEP[n].get("wpp")) == (n in DEP_WPP) for n in DEP)

# the first two seeds at which every substream of the geometry holds a removed byte (most: 0 and 1)
SEEDS = {"dep_mid_wpp": (3, 5), "dep_mid_wpp_10b_dbk": (3, 4), "dep_mid_wpp_ctb16_tall": (78, 91),
         "dep_mid_1ctu_10b": (34, 35)}
# (name, overrides, the two seeds)
CASES = [
    ("wpp_ctb16", dict(width=96, height=64, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=2, wpp=1), (0, 1)),
    ("nowpp", dict(), (0, 1)),
    # tile_lf_across 0: the tiles are substream ranges of the NAL unit (a nonzero start); 1: children of an assembly
    ("tiles_2x2", dict(tile_cols=2, tile_rows=2, tile_lf_across=0), (0, 1)),
    ("tiles_2x2_across", dict(tile_cols=2, tile_rows=2, tile_lf_across=1), (0, 1)),
    ("slices_across", dict(slice_ctus=8, slice_lf_across=1, wpp=1), (0, 1)),
    ("c444_12b", dict(chroma_format=3, bit_depth=12, pcm_bd_y=12, pcm_bd_c=11, wpp=1), (0, 1)),
] + [(n, DEP[n], SEEDS.get(n, (0, 1))) for n in DEP_WPP + DEP_NOWPP]
IDS = [c[0] for c in CASES]
MIN_DENSITY = 0.02


def params(over):
    """test_slices.py's base (128x96, CTB 32, no WPP) with half of the eligible CUs PCM and samples 0..3"""
    p = S.SynthParams(**{**dict(width=128, height=96, wpp=0), **over})
    return dataclasses.replace(p, pcm=1, pcm_pct=50, pcm_mask=3, pcm_log2_max=min(5, p.log2_ctb, p.pcm_log2_max))


def density(p, seed):
    """(both conditions hold, removed bytes / payload bytes, what fails) of one picture, by the model"""
    removed = total = 0
    why, first = "", True
    for nal in _nal_units(S.picture_item(p, seed)):
        payload = nal[2:]
        rem = ref.unescape(payload)[1]
        removed += len(rem)
        total += len(payload)
        starts = slice_header(p, nal)["starts"] + [len(payload)]
        for k in range(len(starts) - 1):
            if not first and not any(starts[k] <= r < starts[k + 1] for r in rem):
                why = why or f"no removed byte in substream [{starts[k]}, {starts[k + 1]})"
            first = False
    frac = removed / total
    if frac < MIN_DENSITY:
        why = why or f"{removed} of {total} payload bytes"
    return not why, frac, why


def checks_ok(img):
    return all(c["term_ok"] and c["raw_start"] == c["raw_entry"] for c in img.checks)


def test_mask_zero_is_the_generator_as_it_was():
    """pcm_mask = 0 draws and writes what the generator always did: two streams pinned by their bytes'
    hashes as they were before the field existed (tests/golden/synth_planes.json pins two more)."""
    import hashlib

    import test_synth

    want = {"pcm_8b": "52c983e722f6f84434bcc7b92244ccc05e0ffe464d82b024136cb894ef6c5c09",
            "c444_12b_pcm": "936871b8964bb6d61859ce76f70ea7111941f1457b43761de84b1828f773ac0b"}
    for name, sha in want.items():
        p = test_synth.params(dict(test_synth.CASES)[name])
        assert p.pcm and p.pcm_mask == 0
        assert hashlib.sha256(S.picture(p, 3)).hexdigest() == sha, name
        assert S.picture(dataclasses.replace(p, pcm_mask=3), 3) != S.picture(p, 3)
        # a mask of every bit leaves the samples as drawn: the draws themselves are the same
        assert S.picture(dataclasses.replace(p, pcm_mask=(1 << p.bit_depth) - 1), 3) == S.picture(p, 3)
    with pytest.raises(ValueError):
        S.picture(dataclasses.replace(test_synth.params(dict(pcm=1)), pcm_mask=-1), 0)


@pytest.mark.parametrize("name,over,seeds", CASES, ids=IDS)
def test_streams_are_dense(name, over, seeds):
    p = params(over)
    for seed in seeds:
        ok, frac, why = density(p, seed)
        print(f"{name} seed {seed}: {100 * frac:.1f} % of the payload bytes removed")
        assert ok, (name, seed, why)


@pytest.mark.parametrize("name,over,seeds", CASES, ids=IDS)
def test_oracle_decodes_dense_streams(oracle_mod, name, over, seeds):
    p = params(over)
    for seed in seeds:
        img = oracle_mod.decode_heic(S.single_heic(p, seed=seed))
        assert checks_ok(img), (name, seed)
        assert img.y.shape == (p.height - p.conf_bottom, p.width - p.conf_right)


CSRC = os.path.join(os.path.dirname(__file__), "..", "heif_amd", "csrc")


@pytest.fixture(scope="module")
def emu_check():
    make_emu("emu-fast")
    return os.path.join(CSRC, "build", "emu_fast", "emu_check")


def run_emu(emu_check, path, parse):
    r = subprocess.run([emu_check, str(path), "5"], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "HEIFGPU_PARSE": parse})
    assert r.returncode == 0 and "EMU PARITY OK" in r.stdout + r.stderr, (r.stdout + r.stderr)[-2000:]


@pytest.mark.parametrize("parse", ["solo", "spread", "lanes"])
@pytest.mark.parametrize("name,over,seeds", CASES, ids=IDS)
def test_emulated_kernels_dense_streams(emu_check, tmp_path, name, over, seeds, parse):
    for seed in seeds:
        path = tmp_path / f"{seed}.heic"
        path.write_bytes(S.single_heic(params(over), seed=seed))
        run_emu(emu_check, path, parse)


# ---------------------------------------------------------------- EP bytes inside the slice header
# 4:0:0, 7 CTB rows: 8 header bits, 5 of num_entry_point_offsets = 6 and 11 of offset_len_minus1 = 31 put the
# 32-bit offsets on byte boundaries, so each offset below 1025 is 00 00 0x xx and takes an escape
HEADER_CASE = (dict(width=32, height=112, chroma_format=0, log2_ctb=4, log2_max_tb=4, max_th_depth_intra=2, wpp=1), 0)


def wide_header(p, nal):
    """nal with offset_len_minus1 = 31: every entry point offset a 32-bit field, whose leading zero
    bytes have to be escaped; the slice data unchanged.  (the new NAL unit, its header's raw length)"""
    h = slice_header(p, nal)
    assert h["offsets"]
    w = BitWriter()
    bits = "".join(f"{b:08b}" for b in h["rbsp"])[:h["entries_pos"]]
    for b in bits:
        w.u(int(b), 1)
    w.ue(len(h["offsets"]))
    w.ue(31)
    for o in h["offsets"]:
        w.u(o - 1, 32)
    w.trailing()
    hdr = _ep(w.bytes())
    return nal[:2] + hdr + nal[2 + h["data_raw"]:], len(hdr)


@pytest.fixture(scope="module")
def header_streams():
    over, seed = HEADER_CASE
    p = params(over)
    nal = S.picture(p, seed)
    wide, hdr_len = wide_header(p, nal)
    return p, S.single_heic(p, nal=nal), S.single_heic(p, nal=wide), wide, hdr_len


def test_header_with_ep_bytes_is_read(oracle_mod, header_streams):
    import heif_amd as H

    p, plain, wide, nal, hdr_len = header_streams
    assert len([r for r in ref.unescape(nal[2:])[1] if r < hdr_len]) >= 3
    t0, t1 = H.HeifImage.parse(plain).tile_params(0), H.HeifImage.parse(wide).tile_params(0)
    assert t1["slice_data_raw_offset"] == hdr_len and t1["entry_point_offset"] == t0["entry_point_offset"]
    assert t1["payload_bytes"] - hdr_len == t0["payload_bytes"] - t0["slice_data_raw_offset"]
    a, b = oracle_mod.decode_heic(plain), oracle_mod.decode_heic(wide)
    assert checks_ok(a) and checks_ok(b)
    for x, y in zip((a.y, a.cb, a.cr), (b.y, b.cb, b.cr)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("parse", ["solo", "spread", "lanes"])
def test_emulated_kernels_header_with_ep_bytes(emu_check, tmp_path, header_streams, parse):
    path = tmp_path / "wide.heic"
    path.write_bytes(header_streams[2])
    run_emu(emu_check, path, parse)


# ------------------------------------------------------------------ GPU parity
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def gctx(H):
    c = H.DecodeContext(0)
    yield c
    c.close()


def _planes(o):
    return [None if t is None else t.cpu().numpy().astype(np.uint16) for t in (o.y, o.cb, o.cr)]


def _assert_equal(got, img, tag):
    for g, r, c in zip(got, (img.y, img.cb, img.cr), "YUV"):
        if r is None:
            assert g is None, tag
            continue
        assert g.shape == r.shape, (tag, c)
        bad = int((g != r).sum())
        assert bad == 0, f"{tag} {c}: {bad} samples differ"


def _decode(H, ctx, data, parse):
    imgs = [H.HeifImage.parse(data)]
    b = ctx.prepare(imgs, parse=parse)
    outs = ctx.alloc_outputs(imgs)
    b.decode_async(outs)
    st = b.status()
    b.free()
    return outs[0], st


@pytest.mark.gpu
@pytest.mark.parametrize("parse", ["solo", "spread", "lanes"])
@pytest.mark.parametrize("name,over,seeds", CASES, ids=IDS)
def test_gpu_dense_streams_bit_exact(H, gctx, oracle_mod, name, over, seeds, parse):
    p = params(over)
    for seed in seeds:
        data = S.single_heic(p, seed=seed)
        out, st = _decode(H, gctx, data, parse)
        assert st == [0], (name, seed)
        _assert_equal(_planes(out), oracle_mod.decode_heic(data, with_checks=False), (name, seed))


@pytest.mark.gpu
@pytest.mark.parametrize("parse", ["solo", "spread", "lanes"])
def test_gpu_header_with_ep_bytes(H, gctx, oracle_mod, header_streams, parse):
    p, plain, wide, nal, hdr_len = header_streams
    want = oracle_mod.decode_heic(plain, with_checks=False)
    out, st = _decode(H, gctx, wide, parse)
    assert st == [0]
    _assert_equal(_planes(out), want, "wide header")
