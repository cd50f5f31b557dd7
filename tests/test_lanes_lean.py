"""The lanes parse's two bodies: k_parse_lanes keeps every coding
tool of every chroma format at run time, k_parse_lean is the same source
compiled for the tool set nearly every HEIC still uses (4:2:0, no PCM,
transform_skip or cu_transquant_bypass, no slice segments inside a picture,
no WPP rows beyond the picture's lanes).  One predicate over the batch picks
the body at prepare time (lanes_variant_for; HEIFGPU_LANES_VARIANT=general
keeps the general one), and the host emulation runs the body the GPU would.

CPU: the product library holds both kernels at two waves per SIMD without
scratch, the lean one smaller; both bodies decode a halfmoonbay tile and small
synthetic pictures bit-exactly in emulation; batches outside the lean set fall
back; a corrupt single-substream picture ends in status bits in both bodies
and reads nothing out of range (ASan build of the emulation).
GPU: the same pictures and the mixed batches on the device."""
import os
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import make_emu

S = pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
LLVM = pathlib.Path("/opt/rocm/llvm/bin")

# 96x64, CTB 32: 3 x 2 CTBs (two WPP rows, so a picture takes two lanes)
BASE = dict(width=96, height=64)
CASES = {
    "wpp_sh_dqp": dict(wpp=1, sign_hiding=1, cu_qp_delta=1),
    "wpp_plain": dict(wpp=1, sign_hiding=0, cu_qp_delta=0),
    "nowpp_sh_dqp": dict(wpp=0, sign_hiding=1, cu_qp_delta=1),
    "nowpp_plain": dict(wpp=0, sign_hiding=0, cu_qp_delta=0),
}
# pictures outside the lean tool set (each makes its batch a general one)
OUTSIDE = {
    "tskip_bypass": dict(wpp=1, transform_skip=1, tq_bypass=1),
    "pcm": dict(wpp=1, pcm=1, pcm_pct=20, pcm_log2_max=4),
    "dep_mid": dict(wpp=0, slice_ctus=2, slice_dependent=1),  # segments starting inside CTB rows
}
C422 = dict(wpp=1, chroma_format=2)  # (a batch shares one chroma format: on its own)


def params(over):
    return S.SynthParams(**{**BASE, **over})


def heic(over, seed=3):
    return S.single_heic(params(over), seed=seed)


# ------------------------------------------------------------ the product's kernels
def _kernels(tmp_path):
    """{kernel symbol: (code bytes, metadata text)} of the gfx950 code objects in libheifgpu.so."""
    from heif_amd import _lib

    # (no skip: this is the only occupancy and scratch guard on k_parse_lean)
    assert (LLVM / "llvm-objdump").exists() and (LLVM / "llvm-readelf").exists(), "ROCm's llvm-objdump / llvm-readelf"
    lib = tmp_path / "lib.so"
    shutil.copy(_lib.LIB_PATH, lib)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    out = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950")):
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "-s", "--wide", str(co)], check=True, capture_output=True,
                              text=True).stdout
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        for m in re.finditer(r"\s(\d+)\s+FUNC\s+GLOBAL\s+\S+\s+\d+\s+(\S*k_parse_l\w+)", syms):
            out[m.group(2)] = (int(m.group(1)), _kernel_block(notes, m.group(2)))
    return out


def _kernel_block(notes: str, name: str) -> str:
    """The amdhsa.kernels entry of `name` (a YAML list: every entry starts with '  - .')."""
    entries = re.split(r"\n  - ", notes)
    hits = [e for e in entries if re.search(rf"\.name:\s+{re.escape(name)}\n", e)]
    assert len(hits) == 1, name
    return hits[0]


def _field(block: str, key: str) -> int:
    m = re.search(rf"\.{key}:\s+(\d+)", block)
    assert m, (key, block[:400])
    return int(m.group(1))


def test_product_has_both_bodies_at_two_waves(tmp_path):
    k = _kernels(tmp_path)
    general = [n for n in k if "k_parse_lanes" in n]
    lean = [n for n in k if "k_parse_lean" in n]
    assert len(general) == 1 and len(lean) == 1, sorted(k)
    for n in general + lean:
        blk = k[n][1]
        vgprs = _field(blk, "vgpr_count")
        # gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8
        assert 512 // ((vgprs + 7) // 8 * 8) == 2, (n, vgprs)
        assert vgprs > 168, (n, vgprs)  # at <= 168 a SIMD would hold three
        assert _field(blk, "private_segment_fixed_size") == 0, n  # no scratch
        assert _field(blk, "vgpr_spill_count") == 0, n
    assert k[lean[0]][0] < k[general[0]][0], {n: v[0] for n, v in k.items()}


# ------------------------------------------------------------ host emulation
@pytest.fixture(scope="module")
def emu_check():
    make_emu("emu-fast")
    return str(CSRC / "build" / "emu_fast" / "emu_check")


def _emu(exe, args, variant, timeout=600):
    env = {**os.environ, "HEIFGPU_PARSE": "lanes", "HEIFGPU_LANES_VARIANT": variant}
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=timeout)
    return r.returncode, r.stdout + r.stderr


def _variant(out):
    return next(l.split(": ")[1] for l in out.splitlines() if l.startswith("lanes variant:"))


@pytest.mark.parametrize("variant", ["auto", "general"])
def test_emulated_halfmoonbay_tile(emu_check, variant):
    """One tile of the bench's stream (tile 7 of 48) through each body."""
    rc, out = _emu(emu_check, [ROOT / "tests/golden/halfmoonbay.heic", 5, 48, 7], variant)
    assert rc == 0 and "EMU PARITY OK" in out, out[-2000:]
    assert _variant(out) == ("lean" if variant == "auto" else "general")


@pytest.mark.parametrize("variant", ["auto", "general"])
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_synthetic(emu_check, tmp_path, name, variant):
    p = tmp_path / "p.heic"
    p.write_bytes(heic(CASES[name]))
    rc, out = _emu(emu_check, [p, 5], variant)
    assert rc == 0 and "EMU PARITY OK" in out, out[-2000:]
    assert _variant(out) == ("lean" if variant == "auto" else "general")


def test_predicate_falls_back_to_general(emu_check, tmp_path):
    """prepare's predicate (the emulation driver's host-only stage builds the
    batch and asks it): lean for pictures of the set, general as soon as one
    picture of the batch is outside it."""
    inside = tmp_path / "in.heic"
    inside.write_bytes(heic(CASES["wpp_sh_dqp"]))
    inside2 = tmp_path / "in2.heic"
    inside2.write_bytes(heic(CASES["nowpp_plain"], seed=4))
    rc, out = _emu(emu_check, [inside, 0, inside2], "auto")
    assert rc == 0 and "host ok: 2 pictures" in out and _variant(out) == "lean", out
    rc, out = _emu(emu_check, [inside, 0, inside2], "general")
    assert rc == 0 and _variant(out) == "general", out
    for name, over in OUTSIDE.items():
        other = tmp_path / f"{name}.heic"
        other.write_bytes(heic(over))
        for order in ([inside, 0, other], [other, 0, inside]):
            rc, out = _emu(emu_check, order, "auto")
            assert rc == 0 and _variant(out) == "general", (name, out)
    c422 = tmp_path / "c422.heic"
    c422.write_bytes(heic(C422))
    rc, out = _emu(emu_check, [c422, 0], "auto")
    assert rc == 0 and _variant(out) == "general", out


# ------------------------------------------------------------ corrupt streams (unit_ctu_end)
def _corrupt(data: bytes, k: int) -> bytes:
    """The picture's slice data damaged in a few ways: bytes of the second half
    overwritten with ones (end_of_slice_segment_flag and split flags decode as
    1 early), with zeros, or at random."""
    import random

    from oracle import oracle

    d = bytearray(data)
    tiles, _ = oracle.list_tiles(data)
    (o, n), = tiles
    lo = o + 24 + (n - 24) // 3
    if k == 0:
        d[lo:o + n] = b"\xff" * (o + n - lo)
    elif k == 1:
        d[lo:o + n] = bytes(o + n - lo)
    else:
        rng = random.Random(k)
        for _ in range(40):
            d[lo + rng.randrange(o + n - lo)] = rng.randrange(256)
    return bytes(d)


# the random damages 8, 50, 188 and 231 decode an end_of_slice_segment_flag of 1
# inside a row (found by search; the code before this change read one entry
# past the substream table there, which the sanitizer build reported)
CORRUPT_SEEDS = (0, 1, 8, 50, 188, 231)


@pytest.fixture(scope="module")
def emu_asan():
    make_emu("emu")
    return str(CSRC / "build" / "emu" / "emu_check")


@pytest.mark.parametrize("variant", ["auto", "general"])
def test_corrupt_single_substream_picture(emu_asan, tmp_path, variant):
    """A corrupt picture of one substream (no WPP, no slice segments): an
    end_of_slice_segment_flag of 1 inside a row is an error at once, not a
    switch to a dependent segment the picture does not have (whose entry would
    lie past the picture's part of the substream table).  Status bits in both
    bodies, and no out-of-range access in the sanitizer build.  (The parse
    status word is what the emulation shows; heifgpu_batch_status maps any
    non-zero word to HEIFGPU_E_DECODE on the device, which needs a GPU and is
    covered for corrupt streams by test_gpu.py's
    test_corrupt_stream_sets_status_not_fault, not here.)"""
    good = heic(dict(wpp=0, sign_hiding=1, cu_qp_delta=1), seed=7)
    flagged = 0
    for k in CORRUPT_SEEDS:
        p = tmp_path / f"c{k}.heic"
        p.write_bytes(_corrupt(good, k))
        rc, out = _emu(emu_asan, [p, 1], variant)
        assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
        assert rc in (0, 1), out[-2000:]
        line = next(l for l in out.splitlines() if l.startswith("parse: status"))
        flagged += int(line.split()[2].rstrip(","), 16) != 0
        if k == CORRUPT_SEEDS[0]:
            assert _variant(out) == ("lean" if variant == "auto" else "general")
    assert flagged == len(CORRUPT_SEEDS), flagged


# ------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def H():
    torch = pytest.importorskip("torch")  # (here, so that the CPU tests above never depend on it)
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import heif_amd

    return heif_amd


@pytest.fixture(scope="module")
def ctx(H):
    c = H.DecodeContext(0)
    yield c
    c.close()


_ref_cache = {}


def _ref(oracle_mod, data):
    if data not in _ref_cache:
        _ref_cache[data] = oracle_mod.decode_heic(data, with_checks=False)
    return _ref_cache[data]


def _decode_and_check(H, ctx, oracle_mod, datas, want_variant, monkeypatch, variant):
    monkeypatch.setenv("HEIFGPU_LANES_VARIANT", variant)
    imgs = [H.HeifImage.parse(d) for d in datas]
    b = ctx.prepare(imgs, parse="lanes")
    try:
        assert b.parse_geometry()["mode"] == "lanes"
        assert b.lanes_variant() == ("general" if variant == "general" else want_variant)
        outs = ctx.alloc_outputs(imgs)
        b.decode_async(outs)
        assert not any(b.status())
    finally:
        b.free()
    for k, (d, o) in enumerate(zip(datas, outs)):
        img = _ref(oracle_mod, d)
        for g, r, c in zip((o.y, o.cb, o.cr), (img.y, img.cb, img.cr), "YUV"):
            g = g.cpu().numpy().astype(np.uint16)
            assert g.shape == r.shape and np.array_equal(g, r), (k, c)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "general"])
def test_gpu_lean_set(H, ctx, oracle_mod, monkeypatch, variant):
    """Every 96x64 case in one batch (WPP and one-substream pictures side by side), then a
    batch of 7 pictures (14 lanes: a partly filled wave) and a 10-bit one."""
    datas = [heic(over, seed=s) for over in CASES.values() for s in (1, 2)]
    _decode_and_check(H, ctx, oracle_mod, datas, "lean", monkeypatch, variant)
    seven = [heic(CASES["wpp_sh_dqp"], seed=s) for s in range(10, 17)]
    _decode_and_check(H, ctx, oracle_mod, seven, "lean", monkeypatch, variant)
    ten = [heic({**CASES["wpp_sh_dqp"], "bit_depth": 10}, seed=s) for s in (1, 2)] + \
          [heic({**CASES["nowpp_plain"], "bit_depth": 10}, seed=3)]
    _decode_and_check(H, ctx, oracle_mod, ten, "lean", monkeypatch, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OUTSIDE) + ["c422"])
def test_gpu_mixed_batches_run_general(H, ctx, oracle_mod, monkeypatch, name):
    """A picture outside the lean set makes the whole batch a general one, bit-exact
    for the pictures inside the set too."""
    if name == "c422":
        datas = [heic(C422, seed=s) for s in (1, 2)]
    else:
        datas = [heic(CASES["wpp_sh_dqp"], seed=1), heic(OUTSIDE[name], seed=2), heic(CASES["nowpp_plain"], seed=3)]
    _decode_and_check(H, ctx, oracle_mod, datas, "general", monkeypatch, "auto")
