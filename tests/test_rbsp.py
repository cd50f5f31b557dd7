"""k_rbsp alone, against a model of H.265 7.3.1.1 / 7.4.2 / 7.4.7.1 written from the clause text.

k_rbsp is the first kernel of every decode: it removes the emulation-prevention
bytes and remaps every entry point from raw to RBSP offsets.  Its 64-lane logic
(16 bytes per lane, the dwords fetched across lane boundaries, the wave prefix
sum, the carry between 1 KiB steps, the 16-byte store against the byte-wise
compaction, the entry-point loop) is not compiled under HG_HOST_EMU, where
emu_rbsp restates the result, and the end-to-end streams hold next to no
emulation-prevention bytes.  Here hand-built payloads and substream tables
(tests/rbsp_vectors.py) go through the kernel by itself
(tests/rbsp/rbsp_driver.cpp): the RBSP bytes, every remapped word and every
zeroed counter must equal the model (tests/rbsp_ref.py) exactly, and every other
byte and word of every output arena must still hold the sentinel, except the
bytes between a picture's RBSP length and its payload rounded up to 16, which
the 16-byte store may fill.  The same vectors run through emu_rbsp as a
stand-alone ASan + UBSan program (here) and through the product library on the
GPU.  The coverage tests hold on the model alone: they keep the vectors from
going soft.

The bytes behind a payload are the case's to plant (`ends`); the product
zero-fills them.  Entries at or past a payload's end (`entries`) stay in bounds:
the kernel compares an entry with bits_len before it uses it.

GPU leg on an MI355X: 7 tests, one driver run each of 0.28-0.37 s, 2.2 s in the
tests, 3.6 s wall with the driver's build.
"""
import ctypes
import itertools
import pathlib
import subprocess
import time

import numpy as np
import pytest

import rbsp_ref as ref
import rbsp_vectors as rv
from conftest import make_emu

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
DRIVER_SRC = ROOT / "tests" / "rbsp" / "rbsp_driver.cpp"
CASE_NAMES = list(rv.CASES)


def build_gpu_driver(out_dir, lib_dir=ROOT / "heif_amd"):
    """The driver against the built product library (hg::launch_rbsp: the library's own
    object, nothing of the product recompiled)."""
    exe = pathlib.Path(out_dir) / "rbsp_driver"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wextra", f"-I{CSRC}",
           str(DRIVER_SRC), f"-L{lib_dir}", "-lheifgpu", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


_stopped = {}  # driver -> its run that exited non-zero: the module starts no further run of it


def run_case(exe, name, tmp_path, timeout=120):
    """The case through the driver: where its buffers differ from the model."""
    if str(exe) in _stopped:
        pytest.fail(f"not run: an earlier driver run failed ({_stopped[str(exe)]})")
    c = rv.case(name)
    src, out = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    src.write_bytes(c.blob)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([str(exe), str(src), str(out)], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _stopped[str(exe)] = f"{name}: timeout"
        raise
    print(f"{name}: driver {time.perf_counter() - t0:.2f} s")
    if r.returncode != 0:
        _stopped[str(exe)] = f"{name}: exit {r.returncode}"
    assert r.returncode == 0, f"driver failed ({r.returncode}): {r.stderr}"
    return c.failures(np.fromfile(out, dtype=np.uint8))


def report(bad):
    return f"{len(bad)} differences from the model, the first of them:\n" + "\n".join(bad[:12])


@pytest.fixture(scope="module")
def emu_driver():
    make_emu("rbsp-emu")
    return CSRC / "build" / "rbsp_emu" / "rbsp_driver"


@pytest.fixture(scope="module")
def gpu_driver(tmp_path_factory):
    return build_gpu_driver(tmp_path_factory.mktemp("rbsp_driver"))


def all_pics():
    for name in CASE_NAMES:
        for b in rv.case(name).batches:
            for p in b.pics:
                yield name, b, p


# ---------------------------------------------------------------- the model itself
def test_model_by_hand():
    assert ref.unescape(b"\x00\x00\x03\x00") == (b"\x00\x00\x00", [2])
    assert ref.unescape(b"\x00\x00\x03\x04") == (b"\x00\x00\x03\x04", [])
    assert ref.unescape(b"\x01\x00\x00\x03") == (b"\x01\x00\x00", [3])       # the 03 ends the payload
    assert ref.unescape(b"\x00\x00\x00\x03\x01") == (b"\x00\x00\x00\x01", [3])
    assert ref.unescape(b"\x00\x00\x03\x03\x03") == (b"\x00\x00\x03\x03", [2])  # a removed byte is no zero
    assert ref.unescape(b"\x00\x00\x03\x00\x00\x03\x01") == (b"\x00\x00\x00\x00\x01", [2, 5])
    assert ref.unescape(b"\x03\x00\x00") == (b"\x03\x00\x00", []) and ref.unescape(b"") == (b"", [])
    assert ref.unescape(rv.REAL_SPS)[0] == bytes([0x01, 0x03, 0x70, 0, 0, 0, 0xB0, 0, 0, 0, 0, 0, 0x5A, 0xA0, 0x04])
    # entries: on the first zero, on the 03 itself, right behind it, at the end, past it; the flags ride along
    raw = b"\x07\x00\x00\x03\x01\x00\x00\x03"
    assert ref.remap(raw, [0, 1, 3, 4, 7, 8, 9, ref.SUB_OFFSET])[1] == [0, 1, 3, 3, 6, 6, 6, 6]
    assert ref.remap(raw, [4 | ref.SUB_CONTINUE, 8 | ref.SUB_SEG_END, 100 | ref.SUB_CONTINUE | ref.SUB_SEG_END])[1] == \
        [3 | ref.SUB_CONTINUE, 6 | ref.SUB_SEG_END, 6 | ref.SUB_CONTINUE | ref.SUB_SEG_END]


def test_model_equals_the_kernels_predicate():
    """The sequential scan against the per-position predicate kernels/rbsp.hip states in its
    header, on every string over {0, 1, 3, 4} up to length 10."""
    n = 0
    for length in range(11):
        for t in itertools.product((0, 1, 3, 4), repeat=length):
            raw = bytes(t)
            n += 1
            got = ref.unescape(raw)[1]
            if got != ref.predicate(raw):
                pytest.fail(f"{raw.hex()}: scan {got}, predicate {ref.predicate(raw)}")
    assert n == 1398101


def test_model_equals_host_reader_and_oracle(oracle_mod):
    import heif_amd as H

    seen = 0
    for name, b, p in all_pics():
        want = ref.unescape(p.raw)[0]
        assert H.RbspReader.remove_emulation_prevention(p.raw) == want, (name, p.name)
        src = (ctypes.c_uint8 * max(len(p.raw), 1)).from_buffer_copy(p.raw or b"\0")
        out = (ctypes.c_uint8 * max(len(p.raw), 1))()
        n = oracle_mod.lib.oracle_remove_emulation_prevention(src, len(p.raw), out)
        assert bytes(out[:n]) == want, (name, p.name)
        seen += len(p.removed)
    assert seen > 1000


# ---------------------------------------------------------------- coverage, from the model alone
def test_coverage_positions():
    at = set()
    for _, p in itertools.chain.from_iterable(rv.case(n).pics() for n in CASE_NAMES):
        at |= set(p.removed)
    assert {a % 16 for a in at} == set(range(16))
    assert {a % 1024 for a in at} >= {0, 1, 2, 1022, 1023}  # the first and last bytes of a step
    assert {a // 1024 for a in at} >= {0, 1, 2}


def test_coverage_boundaries():
    c = rv.case("boundaries")
    pics = {p.name: p for _, p in c.pics()}
    for g, group in enumerate(rv.BOUNDARY_GROUPS):
        for f in rv.FOLLOWERS:
            p = pics[f"g{g}_f{f:02x}"]
            assert all(p.raw[a - 2:a + 2] == bytes([0, 0, 3, f]) for a in group)
            assert p.removed == (list(group) if f <= 3 else []), p.name
    assert sorted(a for g in rv.BOUNDARY_GROUPS for a in g) == \
        [2] + list(range(14, 19)) + list(range(1022, 1027)) + list(range(2046, 2051))
    for name, p in pics.items():
        if name.startswith("not_"):
            assert not p.removed and 3 in p.raw[:4], name
    # 00 01 03 00 and 01 00 03 00 with the 03 in the last two and first two bytes of a lane and of a step
    for name in ("not_00_01_03_00", "not_01_00_03_00"):
        head = bytes(int(x, 16) for x in name[4:].split("_"))
        where = {i + 2 for i in range(3100) if pics[name].raw[i:i + 4] == head}
        assert {w % 16 for w in where} >= {14, 15, 0, 1} and {w % 1024 for w in where} >= {1022, 1023, 0}, name


def test_coverage_ends():
    pics = {p.name: p for _, p in rv.case("ends").pics()}
    for n in rv.END_LENGTHS:
        for kind in ("end03", "end03z"):
            p = pics[f"{kind}_{n}"]
            assert len(p.raw) == n and p.removed == ([n - 1] if n >= 3 else []), p.name
            assert p.pad[:1] == (b"\xff" if kind == "end03" else b"\x00")  # only `pos + 1 == len` may decide
        if n >= 2:
            p = pics[f"end00_{n}"]
            assert p.raw[-2:] == b"\0\0" and p.pad[:2] == b"\x03\x00" and not p.removed and len(p.rbsp) == n
        if n >= 4:
            p = pics[f"end04_{n}"]
            assert p.raw[-4:] == b"\0\0\x03\x04" and p.pad[:1] == b"\x00" and not p.removed
    b, = rv.case("ends").batches
    for i, p in enumerate(b.pics):  # the planted bytes are what lies behind the payload in the arena
        off = int(b.pic_arr[i]["bits_off"]) + len(p.raw)
        assert b.bits[off:off + len(p.pad)] == p.pad, p.name


def test_coverage_runs_and_paths():
    pics = {p.name: p for _, p in rv.case("runs").pics()}
    assert pics["000003_x400"].removed == list(range(2, 1200, 3)) and pics["000003_x400"].rbsp == bytes(800)
    assert pics["real_sps"].removed == [5, 10, 13]
    for name, least in (("random_0_3", 150), ("random_0_to_4", 10)):
        assert len(pics[name].raw) == 3000 and len(pics[name].removed) >= least, (name, len(pics[name].removed))
        assert {a // 1024 for a in pics[name].removed} == {0, 1, 2}
    pics = {p.name: p for _, p in rv.case("paths").pics()}
    assert pics["late"].removed == [2500] and pics["early"].removed == [2] and pics["none"].removed == []
    for p in pics.values():
        assert len(p.raw) == 3072
        chunks = np.frombuffer(p.raw, dtype=np.uint8).reshape(-1, 16)
        with3 = (chunks == 3).any(axis=1)
        assert with3.any() and not with3.all()  # unchanged chunks with and without a 03 byte
    assert (np.frombuffer(pics["late"].raw, dtype=np.uint8)[:2048].reshape(-1, 16) == 3).any()


def test_coverage_entries():
    pics = {p.name: p for _, p in rv.case("entries").pics()}
    p = pics["kinds"]
    n, rem = len(p.raw), set(p.removed)
    offs = [e & ref.SUB_OFFSET for e in p.entries]
    assert offs[0] == 0 and offs[-1] == n
    assert any(e - 1 in rem for e in offs) and any(e + 2 in rem for e in offs) and any(e in rem for e in offs)
    assert {n - 1, n, n + 5, ref.SUB_OFFSET} <= set(offs)
    assert {e >> 30 for e in p.entries} == {0, 1, 2, 3}
    assert {e >> 30 for e in p.entries if (e & ref.SUB_OFFSET) >= n} >= {0, 1, 2}
    # an entry right behind a removed byte that is the first and the last byte of a lane and of a step
    assert {(e - 1) % 16 for e in offs if e - 1 in rem} >= {0, 15} and 1025 in offs and 2048 in offs
    assert any(a != b for a, b in zip(p.entries, p.rentries))
    q = pics["130_entries"]
    assert len(q.entries) == 130 and q.n_sub == 129 and len(q.raw) == 3000
    qo = [e & ref.SUB_OFFSET for e in q.entries]
    assert {e // 1024 for e in qo[:64]} == {0, 1} and {e // 1024 for e in qo[64:128]} == {1, 2} and qo[128] // 1024 == 2
    assert len({a - b for a, b in zip(q.entries, q.rentries)}) > 60
    r = pics["nmid3"]
    assert r.nmid == 3 and r.n_sub == 4 and len(r.tail) == 4
    assert all(a != b for a, b in zip(r.entries[5:], r.rentries[5:]))  # each segment start behind a removed byte
    b, = rv.case("entries").batches
    s0 = int(b.pic_arr[2]["sub_first"])
    assert (b.expected_rsubs[s0 + 8:s0 + 13] == rv.SENT32).all() and (b.expected_rsubs[s0:s0 + 8] != rv.SENT32).all()


def test_coverage_batch_and_zeroing():
    b, = rv.case("batch").batches
    assert b.pic0 == 1 and b.pic0 + b.n_launch == len(b.pics) - 1
    assert b.pics[0].removed and b.pics[-1].removed  # they would change if they were launched
    asm = b.pics[3]
    assert asm.flags & rv.PD_ASSEMBLY and asm.raw == b"" and asm.entries == (0,) and asm.n_sub == 0 and asm.hctb == 3
    live = [p for i, p in enumerate(b.pics) if b.launched(i) and not p.flags & rv.PD_ASSEMBLY]
    assert {p.log2_ctb for p in live} == {4, 5, 6} and all(p.H % (1 << p.log2_ctb) for p in live)
    assert len({p.hctb for p in live}) > 1
    zs = rv.case("zeroing").batches
    assert {(z.opt, z.intra_stream) for z in zs} == {(rv.OPT_ALL, 1), (rv.OPT_ALL, 0), (0, 1), (0, 0)}
    for z in zs:
        w = z.expected_words
        ro = [int(v) for v in z.pic_arr["row_off"]]
        assert (w["status"] == 0).tolist() == [False, True, True, True, True, False]
        for name in ("row_counts", "cu_counts", "xprog", "xntu"):
            per = 2 if name == "row_counts" else 1
            zero = w[name][:per * z.total_rows] == 0
            want = np.zeros(z.total_rows, dtype=bool)
            on = name == "row_counts" or (z.opt and (name != "xntu" or z.intra_stream))
            for i in (1, 2, 4):  # not the assembly's rows, not the rows of pictures outside the launch
                want[ro[i]:ro[i] + z.pics[i].hctb] = bool(on)
            assert (zero == np.repeat(want, per)).all(), (z.name, name)
        n = len(z.pics)
        assert (w["xntu"][z.total_rows:] == 0).tolist() == \
            [bool(z.opt and z.intra_stream) and i in (1, 2, 4) for i in range(n)]
        assert (w["xjob"][0] == 0) == bool(z.opt)


def test_coverage_sentinels():
    for name in CASE_NAMES:
        for b in rv.case(name).batches:
            assert (b.expected_rsubs == rv.SENT32).any() and (b.expected_rsubs != rv.SENT32).any()
            assert (b.expected_rbsp[~b.free] == rv.SENTINEL).any() and b.free.any()
            assert len(b.bits) % 64 == 0 and all(int(o) % 64 == 0 for o in b.pic_arr["bits_off"])
            for i, p in enumerate(b.pics):
                assert len(p.raw) <= 3 * 1024 + 64


# ---------------------------------------------------------------- layout
def test_layout_mirrors_match_the_structs(emu_driver):
    r = subprocess.run([str(emu_driver), "--layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    theirs = {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}
    assert theirs == rv.layout_of_mirrors()


# ---------------------------------------------------------------- the two legs
@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulated_rbsp_equals_model(emu_driver, tmp_path, name):
    """emu_rbsp as a stand-alone program under ASan and UBSan"""
    bad = run_case(emu_driver, name, tmp_path)
    assert not bad, report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_rbsp_equals_model(gpu_driver, tmp_path, name):
    bad = run_case(gpu_driver, name, tmp_path)
    assert not bad, report(bad)
