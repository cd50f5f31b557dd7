"""Bilinear chroma upsampling on the host (no GPU): heifgpu_chroma_upsample against the
independent numpy statement (chroma_ref), the VUI's sample location and its override, the
source rectangle of a bilinear image against a brute-force union of taps, the ABI, and the
rule's sanitizer driver.  Every comparison is exact."""
import ctypes
import hashlib
import itertools
import pathlib
import subprocess

import numpy as np
import pytest

import chroma_ref
import display_ref
import resample_ref
import window_cases as wc
from conftest import make_emu

import heif_amd as H
from heif_amd import _lib
import heif_amd.synth_encoder as S

ROOT = pathlib.Path(__file__).resolve().parent.parent


def upsample_abi(plane, bits, fmt, loc, x0, y0, w, h, pad=0):
    """heifgpu_chroma_upsample of a 2-D array into a sentinel-filled buffer with `pad` extra
    samples a row; returns (rc, the rectangle, the pad columns)."""
    dt = np.uint8 if bits == 8 else np.uint16
    src = np.ascontiguousarray(plane, dtype=dt)
    out = np.full((h, w + pad), 0xA5, dtype=dt)
    rc = _lib.lib.heifgpu_chroma_upsample(src.ctypes.data, src.shape[1], src.shape[0], src.strides[0], bits, fmt, loc,
                                          x0, y0, w, h, out.ctypes.data, out.strides[0])
    return rc, out[:, :w], out[:, w:]


def contents(hc, wc_, bits, rng):
    top = (1 << bits) - 1
    yy, xx = np.mgrid[0:hc, 0:wc_]
    return {"random": rng.integers(0, top + 1, (hc, wc_)), "zero": np.zeros((hc, wc_), int),
            "max": np.full((hc, wc_), top), "checker": ((xx + yy) & 1) * top, "columns": (xx & 1) * top,
            "rows": (yy & 1) * top}


@pytest.mark.parametrize("fmt, loc", [(1, k) for k in range(6)] + [(2, 0), (2, 3)])
@pytest.mark.parametrize("bits", [8, 12])
def test_upsample_equals_reference(fmt, loc, bits):
    rng = np.random.default_rng(100 * fmt + 10 * loc + bits)
    for hc, wc_ in itertools.product((1, 2, 3, 5), repeat=2):  # every clamp case of either axis
        W, Hh = 2 * wc_, (2 if fmt == 1 else 1) * hc
        for name, c in contents(hc, wc_, bits, rng).items():
            want = chroma_ref.upsample_plane(c, fmt, loc, Hh, W)
            assert want.min() >= 0 and want.max() <= (1 << bits) - 1
            # the whole grid, then rectangles from even and odd offsets
            for x0, y0 in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (W - 1, Hh - 1)):
                if x0 >= W or y0 >= Hh:
                    continue
                w, h = W - x0, Hh - y0
                rc, got, pad = upsample_abi(c, bits, fmt, loc, x0, y0, w, h, pad=3)
                assert rc == 0, _lib.last_error()
                assert np.array_equal(got, want[y0:, x0:]), (name, hc, wc_, x0, y0)
                assert (pad == 0xA5).all()  # the row's padding keeps the sentinel
                # the reference computed for the rectangle alone says the same
                assert np.array_equal(chroma_ref.upsample_plane(c, fmt, loc, h, w, x0, y0), want[y0:, x0:])


def test_rounding_term_matters():
    """Alternating 0 / max columns at the midway phase: sums of 3 * 255 + 8 >> 4 exercise the + 8."""
    c = np.array([[0, 255, 0, 255]])
    rc, got, _ = upsample_abi(c, 8, 2, 0, 0, 0, 8, 1)
    assert rc == 0
    assert got.tolist() == [[0, 128, 255, 128, 0, 128, 255, 255]]  # (2 * 255 * 4 + 8) >> 4 = 128, not 127
    rc, got, _ = upsample_abi(np.array([[0, 255]]), 8, 1, 1, 0, 0, 4, 2)  # px = 1: quarters
    assert got[0].tolist() == [0, 64, 191, 255]  # (255 * 4 + 8) >> 4 = 64, (3 * 255 * 4 + 8) >> 4 = 191


@pytest.mark.parametrize("args", [
    dict(fmt=3), dict(fmt=0), dict(loc=6), dict(bits=7), dict(bits=17), dict(x0=8), dict(w=9), dict(h=0), dict(y0=4),
])
def test_upsample_refuses(args):
    a = dict(bits=8, fmt=1, loc=0, x0=0, y0=0, w=8, h=4)  # a 4 x 2 plane: the luma grid is 8 x 4
    a.update(args)
    src, out = np.zeros((2, 8), np.uint8), np.full((4, 32), 0xA5, np.uint8)
    rc = _lib.lib.heifgpu_chroma_upsample(src.ctypes.data, 4, 2, 8, a["bits"], a["fmt"], a["loc"], a["x0"], a["y0"],
                                          a["w"], a["h"], out.ctypes.data, 32)
    assert rc == _lib.HEIFGPU_E_INVALID
    assert (out == 0xA5).all()  # nothing written


# ---- the VUI's sample location, the override -----------------------------------------------
def stream(loc, **kw):
    return S.single_heic(S.SynthParams(width=64, height=64, chroma_loc=loc, **kw), seed=3)


def test_default_stream_is_unchanged():
    """chroma_loc = -1 writes vui_parameters_present_flag = 0 as ever: the bytes of a
    default stream, hashed at the commit before SynthParams had the field."""
    d = S.single_heic(S.SynthParams(width=64, height=64), seed=3)
    assert len(d) == 722
    assert hashlib.sha256(d).hexdigest() == "c1c8218eb145c9287d8cb7429f2112380452fbf68a3bad0135f36769941c8a53"
    assert stream(-1) == d and stream(0) != d


@pytest.mark.parametrize("loc", [-1, 0, 1, 2, 3, 4, 5])
def test_vui_location_is_kept(loc):
    img = H.HeifImage.parse(stream(loc))
    c = img.chroma
    assert c.signalled == (loc >= 0) and c.loc == max(loc, 0) and c.subsampling == (2, 2)
    assert img.chroma_loc == max(loc, 0) and img.chroma_upsampling == "replicate"
    assert img.info.width == 64  # the rest of the SPS still parses behind the VUI
    # the override wins, None restores the file's value; the mode is kept across both
    img.chroma_upsampling = "bilinear"
    img.chroma_loc = 4
    assert img.chroma_loc == 4 and img.chroma.loc == max(loc, 0) and img.chroma_upsampling == "bilinear"
    img.chroma_loc = None
    assert img.chroma_loc == max(loc, 0) and img.chroma_upsampling == "bilinear"


def test_subsampling_of_the_other_formats():
    for fmt, sub in ((0, (1, 1)), (2, (2, 1)), (3, (1, 1))):
        img = H.HeifImage.parse(stream(2, chroma_format=fmt), chroma="bilinear")  # accepted, no effect
        assert img.chroma.subsampling == sub and img.chroma.loc == 2 and img.chroma_upsampling == "bilinear"


def test_location_six_is_a_parse_error():
    """The ue(v) of chroma_sample_loc_type_top_field hand-patched from 5 (00110) to 6 (00111)."""
    p4, p5 = (S.SynthParams(width=64, height=64, chroma_loc=k) for k in (4, 5))
    sps4, sps5 = S.parameter_sets(p4)[1], S.parameter_sets(p5)[1]
    assert len(sps4) == len(sps5)
    bits4, bits5 = (np.unpackbits(np.frombuffer(s, np.uint8)) for s in (sps4, sps5))
    first = int(np.nonzero(bits4 != bits5)[0][0])  # 00101 / 00110: the fourth bit of the code
    assert bits5[first - 3:first + 2].tolist() == [0, 0, 1, 1, 0]
    bits5 = bits5.copy()
    bits5[first + 1] = 1
    bad = np.packbits(bits5).tobytes()
    good = S.single_heic(p5, seed=3)
    assert good.count(sps5) == 1
    assert H.HeifImage.parse(good).chroma.loc == 5
    with pytest.raises(H.HeifGpuError) as e:
        H.HeifImage.parse(good.replace(sps5, bad))
    assert e.value.code == _lib.HEIFGPU_E_PARSE and "chroma_sample_loc_type_top_field" in str(e.value)


def test_setter_arguments():
    img = H.HeifImage.parse(stream(1))
    with pytest.raises(ValueError):
        img.chroma_upsampling = "bicubic"
    for bad in (-1, 6, 1.5, True):
        with pytest.raises(ValueError):
            img.chroma_loc = bad
    with pytest.raises(ValueError):
        H.HeifImage.parse(stream(1), chroma="nearest")
    with pytest.raises(ValueError):
        H.HeifImage.parse_many([stream(1)], chroma="nearest")
    lib = _lib.lib
    assert lib.heifgpu_image_set_chroma_upsampling(img._h, 2, -1) == _lib.HEIFGPU_E_INVALID
    assert lib.heifgpu_image_set_chroma_upsampling(img._h, 1, 6) == _lib.HEIFGPU_E_INVALID
    assert lib.heifgpu_image_set_chroma_upsampling(img._h, 1, -2) == _lib.HEIFGPU_E_INVALID
    assert img.chroma_upsampling == "replicate" and img.chroma_loc == 1  # a refused call changes nothing
    a, b = H.HeifImage.parse_many([stream(1), stream(4)], chroma="bilinear")
    assert a.chroma_upsampling == b.chroma_upsampling == "bilinear" and (a.chroma_loc, b.chroma_loc) == (1, 4)


def test_grid_tiles_must_agree():
    pn, p0, p1 = (S.SynthParams(width=64, height=64, chroma_loc=k) for k in (-1, 0, 1))
    assert H.HeifImage.parse(S.grid_heic(128, 64, p1, seed=1)).chroma.loc == 1
    # a grid whose tiles carry their own parameter sets: the image keeps its first picture's location
    img = H.HeifImage.parse(S.grid_heic(128, 64, p1, seed=1, tile_params=[p1, p1]))
    assert img.chroma.loc == 1 and img.chroma.signalled
    for pair in ([p0, p1], [p1, p0], [pn, p0]):  # (not signalled and signalled as 0 differ too)
        with pytest.raises(H.UnsupportedError, match="grid tiles with different formats"):
            H.HeifImage.parse(S.grid_heic(128, 64, pair[0], seed=1, tile_params=pair))


# ---- the source rectangle --------------------------------------------------------------------
def shown_box(steps, window, W=wc.W, Hh=wc.H):
    """The decoded luma box (x, y, w, h) a displayed window shows, by gathering coordinates."""
    ys, xs = np.mgrid[0:Hh, 0:W]
    tx, ty = display_ref.apply_transforms(xs, steps), display_ref.apply_transforms(ys, steps)
    x, y, w, h = window if window is not None else (0, 0, tx.shape[1], tx.shape[0])
    sx, sy = tx[y:y + h, x:x + w], ty[y:y + h, x:x + w]
    return int(sx.min()), int(sy.min()), int(sx.max() - sx.min() + 1), int(sy.max() - sy.min() + 1)


def replicate_rect(box, W=wc.W, Hh=wc.H):
    x, y, w, h = box
    x0, y0, x1, y1 = x & ~1, y & ~1, min((x + w - 1) | 1, W - 1), min((y + h - 1) | 1, Hh - 1)
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def windows_of(steps):
    """Displayed windows: those of window_cases, ones touching each edge, odd origins, the whole."""
    out = [wc.displayed_window(steps, s) for s in wc.SOURCE_WINDOWS]
    ys, xs = np.mgrid[0:wc.H, 0:wc.W]
    dh, dw = display_ref.apply_transforms(xs, steps).shape
    out += [None, (0, 0, 7, 5), (dw - 7, dh - 5, 7, 5), (0, dh - 3, 3, 3), (dw - 1, 0, 1, 1), (61, 63, 9, 3), (3, 1, 1, 1)]
    return [w for w in out if w is None or (w[0] + w[2] <= dw and w[1] + w[3] <= dh)], dw, dh


@pytest.mark.parametrize("name", list(wc.VARIANTS))
def test_source_rect_replicate_and_bilinear(name):
    steps = wc.VARIANTS[name]
    data = wc.fixture(name)
    rep, bil = H.HeifImage.parse(data), H.HeifImage.parse(data, chroma="bilinear")
    wins, dw, dh = windows_of(steps)
    grown = 0
    for loc in (None, 1, 2, 5):
        bil.chroma_loc = loc
        for w in wins:
            box = shown_box(steps, w)
            assert rep.source_rect(w) == replicate_rect(box), (w, "replicate")
            want = chroma_ref.tapped_rect(1, loc or 0, wc.W, wc.H, box)
            assert bil.source_rect(w) == want, (w, loc)
            r, a = replicate_rect(box), want
            assert a[0] <= r[0] and a[1] <= r[1] and a[0] + a[2] >= r[0] + r[2] and a[1] + a[3] >= r[1] + r[3]
            grown += a != r
    assert grown > 10
    # the resampled form: the filter's halo first, then the taps of that box
    bil.chroma_loc = 1
    some = [w for w in wins if w is not None]
    for w, size, filt in ((some[0], (7, 5), "bilinear"), (some[-1], (20, 31), "bicubic"), (None, (33, 40), "bicubic")):
        halo = resample_ref.halo_window(dw, dh, w, size[1], size[0], filt)
        box = shown_box(steps, halo)
        assert rep.source_rect(w, size, filt) == replicate_rect(box)
        assert bil.source_rect(w, size, filt) == chroma_ref.tapped_rect(1, 1, wc.W, wc.H, box), (w, filt)


def test_source_rect_422_and_444():
    for fmt in (2, 3, 0):
        p = S.SynthParams(width=64, height=48, chroma_format=fmt)
        d = S.single_heic(p, seed=2)
        rep, bil = H.HeifImage.parse(d), H.HeifImage.parse(d, chroma="bilinear")
        for w in ((5, 3, 9, 7), (0, 0, 1, 1), (62, 46, 2, 2), None):
            box = w if w is not None else (0, 0, 64, 48)
            if fmt == 2:
                want = chroma_ref.tapped_rect(2, 0, 64, 48, box)
                assert want[1] == box[1] and want[3] == box[3]  # no vertical growth
                assert bil.source_rect(w) == want
            else:
                assert bil.source_rect(w) == rep.source_rect(w) == tuple(box)


def test_taps_across_a_tile_seam_select_the_neighbour():
    data = wc.fixture("rot0")
    rep, bil = H.HeifImage.parse(data), H.HeifImage.parse(data, chroma="bilinear")
    w = (64, 64, 6, 6)  # starts on the seam of tiles (1, 1) and its left / upper neighbours
    assert rep.tiles_for(rep.source_rect(w)) == (1, 1, 1, 1)
    bil.chroma_loc = 1  # midway in x: column 64 taps chroma column 31 (luma 62, 63)
    assert bil.source_rect(w)[0] == 62 and bil.tiles_for(bil.source_rect(w)) == (0, 0, 2, 2)
    bil.chroma_loc = 2  # co-sited, top: rows and columns 64.. tap chroma 32 first; the last ones tap the next sample
    assert bil.source_rect(w) == (64, 64, 8, 8) and bil.tiles_for(bil.source_rect(w)) == (1, 1, 1, 1)
    w = (58, 70, 6, 4)  # ends at column 63: the co-sited tap of column 63 is chroma column 32, in the next tile
    assert rep.tiles_for(rep.source_rect(w)) == (0, 1, 1, 1)
    assert bil.tiles_for(bil.source_rect(w)) == (0, 1, 2, 1)


# ---- the ABI ---------------------------------------------------------------------------------
SIZES = {"heifgpu_batch_opts": 20, "heifgpu_color_info": 96, "heifgpu_color_transform": 32860, "heifgpu_display_info": 44,
         "heifgpu_hdr_info": 32, "heifgpu_hdr_transform": 84352, "heifgpu_image_info": 80, "heifgpu_ipc_handle": 72,
         "heifgpu_planes": 40, "heifgpu_rect": 16, "heifgpu_scale": 24, "heifgpu_surface": 16, "heifgpu_tensor_format": 44,
         "heifgpu_tensor_surface": 24, "heifgpu_tile_params": 476}


def test_abi_new_symbols_same_version_same_structs(tmp_path):
    for name in ("heifgpu_image_get_chroma", "heifgpu_image_set_chroma_upsampling", "heifgpu_chroma_upsample"):
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTS
    assert _lib.lib.heifgpu_abi_version() == 6
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "heifgpu.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in SIZES) +
                   '    printf("heifgpu_chroma_info %zu\\n", sizeof(heifgpu_chroma_info));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for n, size in SIZES.items():
        assert int(got[n]) == size, n  # as they were before this entry point was added
    assert int(got["heifgpu_chroma_info"]) == ctypes.sizeof(_lib.ChromaInfo) == 24


# ---- the rule under ASan + UBSan, as a program of its own -----------------------------------
def test_chroma_driver_clean():
    """tests/chroma/chroma_driver.cpp (make chroma-asan): the header's taps and the host hook
    over every clamp case, planes and outputs allocated to the exact size.  Nothing is
    loaded into Python under a sanitizer."""
    make_emu("chroma-asan")
    exe = ROOT / "heif_amd" / "csrc" / "build" / "chroma_asan" / "chroma_driver"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[-2] == "cases 3072"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
