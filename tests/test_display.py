"""Display geometry and alpha discovery on the host (no device): the folded
clap / irot / imir map of heifgpu_image_get_display against the step-by-step
restatement in display_ref, the clap arithmetic and its rejects, which
auxiliary image counts as alpha, and the two new names at the C-ABI boundary.
The render stage itself is in tests/test_display_gpu.py."""
import itertools
import pathlib
import re
import subprocess

import numpy as np
import pytest

import display_ref
from conftest import make_emu

ROOT = pathlib.Path(__file__).resolve().parents[1]
W, H = 48, 32  # a non-square picture of a few CTBs


def _params(**kw):
    from heif_amd import synth_encoder as S

    return S.SynthParams(width=W, height=H, **kw)


def _boxes(steps):
    from heif_amd import synth_encoder as S

    make = {"clap": lambda a: S.clap_box(*a), "irot": S.irot_box, "imir": S.imir_box}
    return tuple(make[k](a) for k, a in steps)


def _display(steps=(), **kw):
    import heif_amd as Hm
    from heif_amd import synth_encoder as S

    return Hm.HeifImage.parse(S.display_heic(_params(), transforms=_boxes(steps), **kw)).display


CLAP = ("clap", (27, 1, 22, 1, -5, 2, 3, 1))  # 27 x 22 at left 8, top 8 of 48 x 32; fits 32 x 48 too
ORDERS = ([list(p) for p in itertools.permutations([CLAP, ("irot", 1), ("imir", 0)])] +
          [list(p) for p in itertools.permutations([CLAP, ("irot", 3), ("imir", 1)])] +
          [[("irot", 1), ("irot", 1)],
           [("imir", 0), ("imir", 1), ("imir", 0)],
           [("irot", 1), CLAP, ("irot", 2), ("imir", 0), ("clap", (9, 1, 7, 1, 1, 1, -1, 2))],
           []])


def test_halfmoonbay_display(halfmoonbay):
    import heif_amd as Hm

    img = Hm.HeifImage.parse(halfmoonbay)
    d, inf = img.display, img.info
    assert (d.out_width, d.out_height) == (3024, 4032)
    assert (inf.width, inf.height, inf.rotation) == (4032, 3024, 3)
    # irot 3: output (ox, oy) shows sample (oy, h - 1 - ox)
    assert list(d.m) == [0, 1, -1, 0] and list(d.t) == [0, 3023]
    assert d.n_transforms == 1
    # item 52 is the HDR gain map (an Apple auxC URN): an auxiliary image, not alpha
    assert inf.aux_item_id == 52 and d.alpha_item_id == 0 and d.alpha_premultiplied == 0


@pytest.mark.parametrize("steps", ORDERS, ids=lambda s: "-".join(f"{k}{a if k != 'clap' else ''}" for k, a in s) or "none")
def test_transform_orders(steps):
    d = _display(steps)
    idx = np.arange(W * H).reshape(H, W)
    want = display_ref.apply_transforms(idx, steps)
    assert (d.out_height, d.out_width) == want.shape
    assert d.n_transforms == len(steps)
    assert sorted(abs(v) for v in d.m) == [0, 0, 1, 1]
    assert np.array_equal(display_ref.gather(idx, d), want)


@pytest.mark.parametrize("fields, rect", [
    ((40, 1, 20, 1, 0, 1, 0, 1), (4, 6, 40, 20)),      # integer centre
    ((41, 1, 21, 1, 0, 1, 0, 1), (4, 6, 41, 21)),      # 3.5 and 5.5 round up
    ((40, 1, 20, 1, -9, 2, -13, 2), (0, 0, 40, 20)),   # -0.5 rounds up to 0
    ((81, 2, 41, 2, 0, 1, 0, 1), (4, 6, 41, 21)),      # 40.5 x 20.5 -> 41 x 21
    ((40, 1, 20, 1, -3, 1, -5, 1), (1, 1, 40, 20)),    # negative offsets, odd left and top
    ((27, 1, 22, 1, -5, 2, 3, 1), (8, 8, 27, 22)),     # 10.5 - 2.5 = 8, 5 + 3 = 8
    ((48, 1, 32, 1, 0, 1, 0, 1), (0, 0, 48, 32)),      # the whole picture
])
def test_clap_arithmetic(fields, rect):
    assert display_ref.clap_rect(W, H, fields) == rect  # the restatement agrees with the hand-worked figures
    d = _display([("clap", fields)])
    assert (d.t[0], d.t[1], d.out_width, d.out_height) == rect
    assert list(d.m) == [1, 0, 0, 1] and d.n_transforms == 1


def _reject_files():
    from heif_amd import synth_encoder as S

    cases = {
        "zero_denominator": S.clap_box(40, 0, 20, 1, 0, 1, 0, 1),
        "zero_offset_denominator": S.clap_box(40, 1, 20, 1, 0, 1, 0, 0),
        "negative_denominator": S.clap_box(40, 1, 20, -1, 0, 1, 0, 1),
        "empty_width": S.clap_box(1, 4, 20, 1, 0, 1, 0, 1),
        "empty_height": S.clap_box(40, 1, 0, 1, 0, 1, 0, 1),
        "too_wide": S.clap_box(49, 1, 20, 1, 0, 1, 0, 1),
        "off_the_right": S.clap_box(40, 1, 20, 1, 5, 1, 0, 1),
        "off_the_top": S.clap_box(40, 1, 20, 1, 0, 1, -7, 1),
        "truncated": S.clap_box(40, 1, 20, 1, 0, 1, 0, 1)[:-1],
        "outside_after_rotation": None,
    }
    p = _params()
    out = {}
    for name, box in cases.items():
        if box is None:  # 40 x 20 fits 48 x 32 but not the 32 x 48 an irot leaves
            tr = (S.irot_box(1), S.clap_box(40, 1, 20, 1, 0, 1, 0, 1))
        else:
            if name == "truncated":  # keep the box header's size right
                box = S._box(b"clap", box[8:])
            tr = (box,)
        out[name] = S.display_heic(p, transforms=tr)
    return out


@pytest.mark.parametrize("name", ["zero_denominator", "zero_offset_denominator", "negative_denominator", "empty_width",
                                  "empty_height", "too_wide", "off_the_right", "off_the_top", "truncated",
                                  "outside_after_rotation"])
def test_clap_rejects(name):
    import heif_amd as Hm

    with pytest.raises(Hm.HeifGpuError) as e:
        Hm.HeifImage.parse(_reject_files()[name])
    assert e.value.code == -2  # HEIFGPU_E_PARSE


def test_alpha_discovery():
    import heif_amd as Hm
    from heif_amd import synth_encoder as S

    mono = _params(chroma_format=0)
    for urn in (S.ALPHA_URN_HEVC, S.ALPHA_URN_MPEGB):
        d = _display(aux=(S.AuxImage(mono, urn=urn),))
        assert d.alpha_item_id == 2 and d.alpha_premultiplied == 0
    # a foreign URN (a gain map, depth, a prefix of the real one) is an auxiliary image but not alpha
    for urn in ("urn:com:apple:photo:2020:aux:hdrgainmap", "urn:mpeg:hevc:2015:auxid:2", "urn:mpeg:hevc:2015:auxid:",
                S.ALPHA_URN_HEVC + "0"):
        f = S.display_heic(_params(), aux=(S.AuxImage(mono, urn=urn, premultiplied=True),))
        img = Hm.HeifImage.parse(f)
        assert img.display.alpha_item_id == 0 and img.display.alpha_premultiplied == 0
        assert img.info.aux_item_id == 2  # aux_item_id keeps its meaning: the first auxl of any type
    d = _display(aux=(S.AuxImage(mono, premultiplied=True),))
    assert d.alpha_item_id == 2 and d.alpha_premultiplied == 1
    # alpha behind a non-alpha auxiliary image is still found
    f = S.display_heic(_params(), aux=(S.AuxImage(mono, urn="urn:com:apple:photo:2020:aux:hdrgainmap"),
                                       S.AuxImage(mono, seed=2, urn=S.ALPHA_URN_MPEGB, premultiplied=True)))
    img = Hm.HeifImage.parse(f)
    assert img.info.aux_item_id == 2 and img.display.alpha_item_id == 3 and img.display.alpha_premultiplied == 1
    # the alpha item parses as an image of its own, with no alpha of its own
    a = Hm.HeifImage.parse(f, 3)
    assert a.info.chroma_format_idc == 0 and a.display.alpha_item_id == 0


def test_builder_keeps_existing_bytes():
    """display_heic without extras is single_heic, byte for byte."""
    from heif_amd import synth_encoder as S

    assert S.display_heic(_params(), seed=5) == S.single_heic(_params(), seed=5)


def test_new_entry_points_at_the_abi():
    from heif_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "heifgpu.h").read_text(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                          check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    for name in ("heifgpu_image_get_display", "heifgpu_render_batch"):
        assert re.search(rf"\b{name}\s*\(", header)
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert name in exported  # unmangled
    assert _lib.lib.heifgpu_abi_version() == 6  # added within ABI 6
    import ctypes

    assert ctypes.sizeof(_lib.DisplayInfo) == 44 and ctypes.sizeof(_lib.Surface) == 16


def test_render_argument_checks_need_no_device():
    """The checks in front of the device work answer without a context."""
    import ctypes

    from heif_amd import _lib

    rc = _lib.lib.heifgpu_render_batch(None, None, 0, None, None, None, 0, None, None)
    assert rc == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_image_get_display(None, ctypes.byref(_lib.DisplayInfo())) == _lib.HEIFGPU_E_INVALID


def test_parser_under_sanitizers(tmp_path):
    """The clap / auxC parser as a stand-alone ASan + UBSan program (make
    display-asan): its built-in checks run display_clap on heap copies of exact
    length, then it parses every file given; a reject must be an error, never a
    sanitizer report."""
    make_emu("display-asan")
    files = _reject_files()
    paths = []
    for name, data in files.items():
        p = tmp_path / f"{name}.heic"
        p.write_bytes(data)
        paths.append(str(p))
    from heif_amd import synth_encoder as S

    good = tmp_path / "good.heic"
    good.write_bytes(S.display_heic(_params(), transforms=_boxes([CLAP, ("irot", 1), ("imir", 1)]),
                                    aux=(S.AuxImage(_params(chroma_format=0), premultiplied=True),)))
    exe = ROOT / "heif_amd" / "csrc" / "build" / "display_asan" / "display_asan"
    r = subprocess.run([str(exe), str(good)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(line.split(": ", 1) for line in r.stdout.splitlines() if ": " in line)
    assert lines[str(good)].startswith("ok 22x27 n=3 alpha=2 prem=1"), lines[str(good)]
    for p in paths:
        assert lines[p].startswith("parse error"), (p, lines[p])
