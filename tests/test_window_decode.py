"""Window decode: decode only the pictures a window reads.

CPU half: the geometry against an independent restatement, the kernels'
sources under the host emulation with a rectangle (selected pictures equal the
oracle, everything else keeps the sentinel), and the ABI surface.  The GPU half
is tests/test_window_decode_gpu.py; window_cases.py holds what they share.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import display_ref
import window_cases as WC
from conftest import make_emu

S = pytest.importorskip("heif_amd.synth_encoder")
H = pytest.importorskip("heif_amd")
from heif_amd import _lib  # noqa: E402


# ------------------------------------------------------------------ geometry
def restated_rect(steps, window, chroma=(1, 1)):
    """The source rectangle, restated: the source coordinates of every pixel of
    the W x H picture pushed through the transforms as arrays; min / max of what
    lands inside the window; grown to the chroma sample grid, clipped."""
    ys, xs = np.mgrid[0:WC.H, 0:WC.W]
    tx, ty = display_ref.apply_transforms(xs, steps), display_ref.apply_transforms(ys, steps)
    x, y, w, h = window if window is not None else (0, 0, tx.shape[1], tx.shape[0])
    sx, sy = tx[y:y + h, x:x + w], ty[y:y + h, x:x + w]
    assert sx.shape == (h, w)
    mx, my = (1 << chroma[0]) - 1, (1 << chroma[1]) - 1
    x0, y0 = int(sx.min()) & ~mx, int(sy.min()) & ~my
    x1, y1 = min(int(sx.max()) | mx, WC.W - 1), min(int(sy.max()) | my, WC.H - 1)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def tiles_touched(rect):
    x, y, w, h = rect
    return {(c, r) for c in range(x // WC.TILE, (x + w - 1) // WC.TILE + 1)
            for r in range(y // WC.TILE, (y + h - 1) // WC.TILE + 1)}


def tiles_of(tf):
    c0, r0, nc, nr = tf
    return {(c, r) for c in range(c0, c0 + nc) for r in range(r0, r0 + nr)}


@pytest.mark.parametrize("name", [n for n, _ in WC.ORIENTATIONS])
def test_source_rect_and_tiles_against_restatement(name):
    steps = dict(WC.ORIENTATIONS)[name]
    img = H.HeifImage.parse(WC.fixture(name))
    d = img.display
    shown = display_ref.apply_transforms(np.zeros((WC.H, WC.W), np.uint8), steps)
    assert (d.out_height, d.out_width) == shown.shape
    n_checked = 0
    for src_window in WC.SOURCE_WINDOWS + [None]:
        window = WC.displayed_window(steps, src_window)
        if window is None and src_window is not None:
            assert "clap" in name  # only a crop can hide a source window altogether
            continue
        want = restated_rect(steps, window)
        got = img.source_rect(window)
        assert got == want, (name, src_window, window)
        assert tiles_of(img.tiles_for(got)) == tiles_touched(want), (name, src_window)
        if "clap" not in name and src_window is not None:
            # an orientation only moves the window: the same samples, whatever it is
            assert got == restated_rect((), src_window), (name, src_window)
            assert len(tiles_touched(got)) == WC.SOURCE_WINDOW_TILES[src_window]
        n_checked += 1
    assert n_checked >= 4


def test_the_windows_of_the_issue_on_the_plain_fixture():
    img = H.HeifImage.parse(WC.fixture("rot0"))
    assert img.tiles_for(img.source_rect((64, 64, 64, 64))) == (1, 1, 1, 1)
    assert img.tiles_for(img.source_rect((60, 60, 10, 10))) == (0, 0, 2, 2)
    assert img.source_rect((63, 64, 2, 1)) == (62, 64, 4, 2)  # x 62..65, y 64..65
    assert img.tiles_for((62, 64, 4, 2)) == (0, 1, 2, 1)
    assert img.tiles_for(img.source_rect((249, 179, 1, 1))) == (3, 2, 1, 1)
    assert img.source_rect(None) == img.source_rect((0, 0, 0, 0)) == (0, 0, WC.W, WC.H)
    assert img.tiles_for(None) == img.tiles_for((0, 0, WC.W, WC.H)) == (0, 0, 4, 3)


def test_halfmoonbay_cover_reads_42_of_48(halfmoonbay):
    img = H.HeifImage.parse(halfmoonbay)
    window = H.HeicDecoder._fit_window(img, (224, 224), "cover")
    assert window == (0, 504, 3024, 3024)
    rect = img.source_rect(window)
    c0, r0, nc, nr = img.tiles_for(rect)
    assert nc * nr == 42 and img.info.num_tiles == 48
    assert WC.count_pictures([img], [rect]) == 42 and WC.count_pictures([img], None) == 48


def test_rejections():
    img = H.HeifImage.parse(WC.fixture("rot0"))
    for bad in [(0, 0, 0, 5), (0, 0, 5, 0), (250, 0, 1, 1), (0, 180, 1, 1), (200, 0, 51, 10), (0, 100, 10, 81),
                (0xFFFFFFFF, 0, 2, 1)]:
        with pytest.raises(ValueError):
            img.source_rect(bad)
        with pytest.raises(ValueError):
            img.tiles_for(bad)  # the same rules for a rectangle of the decoded planes
    clap = H.HeifImage.parse(WC.fixture("clap_rot1_mir"))
    d = clap.display
    assert (d.out_width, d.out_height) == (WC.CLAP[3], WC.CLAP[2])  # turned: 151 x 201
    clap.source_rect((0, 0, d.out_width, d.out_height))
    for bad in [(0, 0, WC.W, WC.H), (0, 0, d.out_width + 1, 1), (0, d.out_height, 1, 1)]:
        with pytest.raises(ValueError):  # inside the decoded picture, outside the displayed one
            clap.source_rect(bad)


# ------------------------------------------------------- emulated kernels
CSRC = os.path.join(os.path.dirname(__file__), "..", "heif_amd", "csrc")


@pytest.fixture(scope="module")
def emu_check():
    make_emu("emu-fast")
    return os.path.join(CSRC, "build", "emu_fast", "emu_check")


def run_emu(emu_check, path, rect, parse=None, stages="5"):
    env = dict(os.environ)
    env.pop("HEIFGPU_PARSE", None)
    if parse:
        env["HEIFGPU_PARSE"] = parse
    r = subprocess.run([emu_check, str(path), stages, "rect=%d,%d,%d,%d" % tuple(rect)], capture_output=True, text=True,
                       timeout=600, env=env)
    return r.returncode, r.stdout + r.stderr


def assert_emu_ok(res, pictures):
    rc, out = res
    assert rc == 0 and "EMU PARITY OK" in out, out[-2000:]
    assert f"pictures: {pictures}\n" in out, out[-2000:]
    assert ": 0 samples not covered" in out, out[-2000:]


@pytest.fixture(scope="module")
def fixture_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("window") / "grid.heic"
    p.write_bytes(WC.fixture("rot0"))
    return p


@pytest.mark.parametrize("window", WC.SOURCE_WINDOWS + [None], ids=str)
def test_emulated_kernels_decode_the_selected_tiles_only(emu_check, fixture_path, window):
    img = H.HeifImage.parse(fixture_path.read_bytes())
    rect = img.source_rect(window)
    assert_emu_ok(run_emu(emu_check, fixture_path, rect), 12 if window is None else WC.SOURCE_WINDOW_TILES[window])
    # the host-only form reports the same count
    rc, out = run_emu(emu_check, fixture_path, rect, stages="0")
    assert rc == 0 and "host ok: %d pictures" % (12 if window is None else WC.SOURCE_WINDOW_TILES[window]) in out, out


@pytest.mark.parametrize("parse", ["lanes", "solo", "spread"])
def test_emulated_kernels_window_in_every_parse_mode(emu_check, fixture_path, parse):
    res = run_emu(emu_check, fixture_path, (60, 60, 10, 10), parse=parse)
    assert f"parse mode: {parse}" in res[1]
    assert_emu_ok(res, 4)


def test_emulated_kernels_rect_combines_with_the_tile_stride(emu_check, fixture_path):
    """Tiles 0, 1, 4, 5 pass the rectangle, 1 and 5 the stride as well."""
    r = subprocess.run([emu_check, str(fixture_path), "0", "rect=60,60,10,10"], capture_output=True, text=True)
    assert "host ok: 4 pictures" in r.stdout
    img = H.HeifImage.parse(fixture_path.read_bytes())
    opts = _lib.BatchOpts(2, 1, 0, 0, 0)
    assert WC.count_pictures([img], [(60, 60, 10, 10)], opts) == 2
    assert WC.count_pictures([img], None, opts) == 6


def _single(tmp_path, name, **over):
    p = S.SynthParams(**{**dict(width=128, height=128, wpp=0), **over})
    path = tmp_path / (name + ".heic")
    path.write_bytes(S.single_heic(p, seed=7))
    return path


def test_emulated_kernels_one_hevc_tile_of_a_picture(emu_check, tmp_path):
    """2 x 2 HEVC tiles, nothing filtered across: a rectangle inside one tile
    decodes that sub-picture alone (and the skipped tiles' substreams are still
    counted: the tile decoded is the last one)."""
    path = _single(tmp_path, "tiles", tile_cols=2, tile_rows=2, tile_lf_across=0)
    assert_emu_ok(run_emu(emu_check, path, (70, 80, 20, 30)), 1)
    assert_emu_ok(run_emu(emu_check, path, (60, 10, 10, 10)), 2)
    assert_emu_ok(run_emu(emu_check, path, (0, 0, 128, 128)), 4)


def test_emulated_kernels_assembly_is_taken_whole(emu_check, tmp_path):
    """The same tiles filtered across their boundaries: four children and their
    assembly, whatever part is asked for."""
    path = _single(tmp_path, "across", tile_cols=2, tile_rows=2, tile_lf_across=1)
    assert_emu_ok(run_emu(emu_check, path, (70, 80, 20, 30)), 5)


def test_emulated_kernels_row_slices(emu_check, tmp_path):
    """One slice per CTB row (4 rows of 32), nothing filtered across slices: the
    rectangle's rows only."""
    path = _single(tmp_path, "slices", slice_ctus=4, slice_lf_across=0)
    assert_emu_ok(run_emu(emu_check, path, (10, 40, 50, 10)), 1)
    assert_emu_ok(run_emu(emu_check, path, (10, 60, 50, 10)), 2)
    across = _single(tmp_path, "slices_across", slice_ctus=4, slice_lf_across=1)
    assert_emu_ok(run_emu(emu_check, across, (10, 40, 50, 10)), 5)


def test_emulated_kernels_halfmoonbay_cover(emu_check, halfmoonbay):
    path = os.path.join(os.path.dirname(__file__), "golden", "halfmoonbay.heic")
    rect = H.HeifImage.parse(halfmoonbay).source_rect((0, 504, 3024, 3024))
    assert_emu_ok(run_emu(emu_check, path, rect), 42)


def test_emu_check_positional_forms_are_undisturbed(emu_check, fixture_path):
    r = subprocess.run([emu_check, str(fixture_path), "5", "3", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "EMU PARITY OK" in r.stdout and "pictures: 4\n" in r.stdout, r.stdout[-2000:]
    r = subprocess.run([emu_check, str(fixture_path), "0", str(fixture_path)], capture_output=True, text=True)
    assert "host ok: 24 pictures" in r.stdout


# ------------------------------------------------------------- ABI surface
def test_new_exports_and_abi_version():
    for name in ("heifgpu_window_source_rect", "heifgpu_image_tiles_for_rect", "heifgpu_batch_prepare_rects",
                 "heifgpu_batch_count_pictures", "heifgpu_batch_picture_count"):
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.heifgpu_abi_version() == 6 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.Rect) == 16 and ctypes.sizeof(_lib.BatchOpts) == 20


def test_no_rectangles_count_as_prepare_ex_does(halfmoonbay):
    """src NULL, and "everything" rectangles, make the pictures the plain prepare
    makes (the batch builder is shared; the GPU half compares the batches)."""
    imgs = [H.HeifImage.parse(halfmoonbay), H.HeifImage.parse(WC.fixture("rot0"))]
    assert WC.count_pictures(imgs, None) == 48 + 12
    assert WC.count_pictures(imgs, [None, None]) == 60
    assert WC.count_pictures(imgs, [None, (64, 64, 64, 64)]) == 49
    with pytest.raises(H.HeifGpuError):
        WC.count_pictures(imgs, [None, (0, 0, 251, 1)])


def test_prepare_rejects_bad_arguments_without_a_device():
    """The rectangle arguments of prepare are checked on the host."""
    img = H.HeifImage.parse(WC.fixture("rot0"))
    with pytest.raises(ValueError):
        img.source_rect((0, 0, 251, 1))
    with pytest.raises(ValueError):
        H.DecodeContext.prepare(None, [img], windows=[None, None])


def test_grid_heic_defaults_are_unchanged():
    """transforms=, colr= and aux= add to the file only when given."""
    p = WC.PARAMS
    a = S.grid_heic(WC.W, WC.H, p, seed=1)
    assert a == S.grid_heic(WC.W, WC.H, p, seed=1, transforms=(), colr=None, aux=())
    b = S.grid_heic(WC.W, WC.H, p, seed=1, transforms=(S.irot_box(1),), colr=S.nclx_box(1, 13, 1, True))
    img = H.HeifImage.parse(b)
    assert (img.display.out_width, img.display.out_height, img.display.n_transforms) == (WC.H, WC.W, 1)
    assert (img.info.matrix_coeffs, img.info.full_range) == (1, 1)
    assert H.HeifImage.parse(a).display.n_transforms == 0
