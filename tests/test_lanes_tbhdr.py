"""The residual header of the lanes parse's TB unit (the last-position
prefix loops, where a lane of a unit run stops at its own bin), on the host emulation.

(a) small pictures with coded TBs of every size and component and the corner prefix
    pairs (tests/lanes_tbhdr_cases.py), each through the emulation's full decode against
    the oracle, in the lean and the general body, alone (one picture per wave) and as the
    three tiles of a grid image in one wave; the emulation's path counters show that a
    picture reaches the paths its case is named for and none of those it excludes.
(b) the passes every wave of halfmoonbay.heic takes at three pictures per wave equal
    tests/golden/lanes_passes_halfmoonbay_ppw3.json: every lane's pass count is as
    it was."""
import json
import os
import pathlib
import subprocess

import pytest

import lanes_tbhdr_cases as C
import lanes_units_cases as U
from conftest import make_emu

pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "heif_amd" / "csrc"


@pytest.fixture(scope="module")
def emu_check():
    make_emu("emu-fast")
    return str(CSRC / "build" / "emu_fast" / "emu_check")


def _emu(exe, args, **env):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "HEIFGPU_PARSE": "lanes", "HEIFGPU_LANES_STATS": "1", **env})
    return r.returncode, r.stdout + r.stderr


def _paths(out):
    """The `paths` and `tb_paths` counters of every wave, summed, by name."""
    tot = {"  paths": [0] * len(U.PATHS), "  tb_paths": [0] * len(C.TB_PATHS)}
    for line in out.splitlines():
        for key, acc in tot.items():
            if line.startswith(key + " "):
                v = [int(x) for x in line.split()[1:]]
                assert len(v) == len(acc), line
                acc[:] = [a + b for a, b in zip(acc, v)]
    return {**dict(zip(U.PATHS, tot["  paths"])), **dict(zip(C.TB_PATHS, tot["  tb_paths"]))}


RUNS = [(n, v, ppw) for n in C.LEAN for v in ("auto", "general") for ppw in (1, 3)] + \
       [(n, "auto", ppw) for n in C.GENERAL for ppw in (1, 3)]


@pytest.mark.parametrize("name,variant,ppw", RUNS, ids=[f"{n}-{v}-ppw{p}" for n, v, p in RUNS])
def test_tbhdr_cases_both_bodies(emu_check, tmp_path, name, variant, ppw):
    over = {**C.LEAN, **C.GENERAL}[name]
    p = tmp_path / "p.heic"
    p.write_bytes(C.heic(over, 1) if ppw == 1 else C.grid(over))
    rc, out = _emu(emu_check, [p, 5], HEIFGPU_LANES_VARIANT=variant, HEIFGPU_LANES_PPW=str(ppw))
    assert rc == 0 and "EMU PARITY OK" in out, out[-2000:]
    body = next(l.split(": ")[1] for l in out.splitlines() if l.startswith("lanes variant:"))
    assert body == ("lean" if name in C.LEAN and variant == "auto" else "general")
    # one wave either way: the picture alone, or the three tiles together
    assert len([l for l in out.splitlines() if l.startswith("wave ")]) == 1, out[-2000:]
    paths = _paths(out)
    print(name, variant, ppw, paths)
    missing = [k for k in C.NEEDS[name] if paths[k] == 0]
    assert not missing, (missing, paths)
    reached = [k for k in C.ZERO.get(name, ()) if paths[k] != 0]
    assert not reached, (reached, paths)


def test_every_path_has_a_case():
    """Every counter of the `tb_paths` line, every TB size and the prefix of 9 are required by some case."""
    needed = {k for v in C.NEEDS.values() for k in v}
    want = set(C.TB_PATHS) | {p for p in U.PATHS if p.startswith(("luma", "chroma"))} | {"last_ctx5", "last_suffix"}
    assert want <= needed, want - needed


def test_pass_counts_equal_parent(emu_check):
    want = json.loads((ROOT / "tests/golden/lanes_passes_halfmoonbay_ppw3.json").read_text())
    rc, out = _emu(emu_check, [ROOT / "tests/golden/halfmoonbay.heic", 1], HEIFGPU_LANES_PPW="3")
    assert rc == 0, out[-2000:]
    got = [int(l.split()[2]) for l in out.splitlines() if l.startswith("wave ")]
    print(got)
    assert len(want["passes"]) == 16 and sum(want["passes"]) == 47894  # (the fixture itself)
    assert got == want["passes"]
