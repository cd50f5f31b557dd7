"""k_intra's neighbour gather on the record's availability facts, against the model of 8.4.4.2.

The pictures of tests/intra_avail_vectors.py (a few CTBs each, distinct values planted on every
probe TB's neighbours) go through the kernel by itself (tests/intra/intra_driver.cpp) and the
sample arena must equal tests/intra_ref.py sample for sample: through the host emulation here,
and through the product library on the GPU, each under HEIFGPU_INTRA_SPLIT=0 and 1.  The
coverage test holds on the model alone: every gather path (one chunk: luma 4x4 and 8x8; two
chunks: 16x16; three: 32x32; a Cb / Cr pair: 4x4 and 8x8) meets nothing available, a first
search position that takes a later sample, a missing left column under a present row above,
full below-left and above-right groups, and, where a TB is larger than the picture's
granularity, groups that the picture's edge cuts part-way.

GPU leg on an MI355X: 3 tests with 6 driver runs of 0.26-0.53 s each (profiles/r25/gpu_suite.txt);
building the three cases and their expectation takes 5 s once, on the CPU.
"""
import os
import pathlib
import subprocess
import time

import numpy as np
import pytest

import intra_avail_vectors as av
from conftest import make_emu
from intra_vectors import formed_pairs

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"
DRIVER_SRC = ROOT / "tests" / "intra" / "intra_driver.cpp"
KNOBS = ({"HEIFGPU_INTRA_SPLIT": "0"}, {"HEIFGPU_INTRA_SPLIT": "1"})
BASE = {"nothing", "forward_fill", "left_missing", "full_bl_ar"}
PART = {"part_bl", "part_ar"}


def run_case(exe, name, tmp_path, env):
    c = av.case(name)
    src, out = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
    src.write_bytes(c.blob)
    t0 = time.perf_counter()
    r = subprocess.run([str(exe), str(src), str(out)], capture_output=True, text=True, timeout=120,
                       env={**os.environ, **env})
    print(f"{name} {env}: driver {time.perf_counter() - t0:.2f} s")
    assert r.returncode == 0, f"driver failed ({r.returncode}): {r.stderr}"
    return c.failures(np.fromfile(out, dtype=np.uint8))


def report(bad):
    return f"{len(bad)} differences from the model, the first of them:\n" + "\n".join(bad[:12])


@pytest.fixture(scope="module")
def emu_driver():
    make_emu("intra-emu")
    return CSRC / "build" / "emu_fast" / "intra_driver"


@pytest.fixture(scope="module")
def gpu_driver(tmp_path_factory):
    """The driver against the built product library (nothing of the product recompiled)."""
    lib_dir = ROOT / "heif_amd"
    exe = tmp_path_factory.mktemp("intra_avail_driver") / "intra_driver"
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wextra", f"-I{CSRC}",
           str(DRIVER_SRC), f"-L{lib_dir}", "-lheifgpu", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_coverage_every_path_meets_every_arm():
    seen = {}
    for p in av.case("avail420").pics:
        info = {id(t): i for t, i in zip(p.tbs, p.infos)}
        paired = set()
        for r, row in enumerate(p.rows):
            paired |= {id(row[k]) for k in formed_pairs(p.records(r))}
        for t in p.tbs:
            if not t.tag or t.cidx == 2:
                continue
            n = 1 << t.log2
            assert p.agree
            if t.cidx == 0:
                path = ("luma", n)
            elif id(t) in paired:
                path = ("pair", n)
            else:
                path = ("chroma", n)
            # the probe's neighbours are pairwise distinct in the model's planes: a wrong source is a wrong value
            pl = p.planes[t.cidx]
            w, h = p.g.plane(t.cidx)
            vals = [int(pl[t.y + dy, t.x + dx]) for (dx, dy), a in zip(av.ref.search_positions(n), info[id(t)].avail)
                    if a and 0 <= t.x + dx < w and 0 <= t.y + dy < h]
            assert len(set(vals)) == len(vals), (p.name, t.tag)
            seen.setdefault(path, set()).update(av.arms(info[id(t)].avail, n))
    # one chunk, two, three; the pairs; a 4:2:0 chroma 16x16 TB takes the two-chunk path as a TB of its own
    want = {("luma", 4): BASE, ("luma", 8): BASE, ("luma", 16): BASE | PART, ("luma", 32): BASE | PART,
            ("pair", 4): BASE, ("pair", 8): BASE | PART, ("chroma", 16): BASE | PART}
    for path, arms in want.items():
        assert arms <= seen.get(path, set()), (path, sorted(arms - seen.get(path, set())))
    for name in ("avail422", "avail444"):
        c = av.case(name)
        assert all(p.agree for p in c.pics) and any(t.tag for p in c.pics for t in p.tbs)


@pytest.mark.parametrize("name", list(av.CASES))
def test_emulated_gather_equals_model(emu_driver, tmp_path, name):
    for env in KNOBS:
        bad = run_case(emu_driver, name, tmp_path, env)
        assert not bad, f"{env}: " + report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(av.CASES))
def test_gpu_gather_equals_model(gpu_driver, tmp_path, name):
    for env in KNOBS:
        bad = run_case(gpu_driver, name, tmp_path, env)
        assert not bad, f"{env}: " + report(bad)
