"""The case lists of test_rgb_gather_gpu.py, checked from the models alone: that they hold
what they were drawn up to hold (every store path of k_ycbcr_rgb, every copy path of
k_gather_tiles, clipping at both ends in every channel, bits below the shift), so that a
thinned or softened list fails here, on any machine; and the gather model's own values
by hand."""
import itertools
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import gather_ref
import rgb_gather_cases as C
import rgb_ref

RGB = C.RGB_CASES


def total(counters) -> Counter:
    out = Counter()
    for n in counters:
        out.update(n)
    return out


# ---- the k_ycbcr_rgb list ----------------------------------------------------------------------
def test_rgb_required_combinations():
    assert len({c.name for c in RGB}) == len(RGB)
    have = {(c.w, c.h, c.rot, c.chroma, c.depth) for c in RGB}
    for (w, h), rot, chroma, depth in itertools.product(C.SHAPES, range(4), range(4), (8, 10)):
        assert (w, h, rot, chroma, depth) in have
    for rot in range(4):  # each (matrix, range) pair with each rotation
        assert {(c.matrix, c.full) for c in RGB if c.rot == rot} == set(C.MATRIX_RANGE), rot
    cross = {(c.depth, c.matrix, c.full, c.chroma) for c in RGB if (c.w, c.h, c.rot) == (37, 22, 1)}
    for combo in itertools.product(C.DEPTHS, (1, 2, 6, 9), (False, True), (0, 1, 3)):
        assert combo in cross, combo
    for (w, h), rot in itertools.product(C.SHAPES, range(4)):
        mine = [c for c in RGB if (c.w, c.h, c.rot) == (w, h, rot)]
        assert {c.pad for c in mine} == {0, C.RGB_PAD}, (w, h, rot)
        assert len({c.off for c in mine}) >= 2, (w, h, rot)
    # (how test_rgb_gather_gpu.py splits the list: nothing falls between its two tests)
    assert all(c.depth in (8, 10) or (c.w, c.h, c.rot) == (37, 22, 1) for c in RGB)
    assert {c.off for c in RGB} == {0, 1, 2, 3}
    assert {(c.rot, c.chroma, C.rgb_bps(c)) for c in RGB} == set(itertools.product(range(4), range(4), (1, 2)))


def test_rgb_sources():
    padded = 0
    for c in RGB:
        bps = C.rgb_bps(c)
        assert bps == (1 if c.depth == 8 else 2)
        y, cb, cr = C.rgb_samples(c)
        assert y.shape == (c.h, c.w) and y.dtype == (np.uint8 if bps == 1 else np.uint16)
        assert (cb is None) == (cr is None) == (c.chroma == 0)
        for k, a in enumerate((y, cb, cr)):
            if a is None:
                continue
            pw, ph = C.rgb_plane_dims(c, k)
            assert a.shape == (ph, pw) and int(a.max()) < 1 << c.depth, c.name
            pitch = C.rgb_src_pitch(c, k)
            assert pitch % bps == 0 and pitch >= pw * bps
            buf = C.rgb_source(c, k)
            assert buf.size == 2 * C.GUARD + ph * pitch
            rows = C.rows_of(buf, 0, ph, pitch)
            assert np.array_equal(rows[:, :pw * bps], C.sample_bytes(a))
            assert (rows[:, pw * bps:] == C.SENTINEL).all()
        padded += C.rgb_src_pitch(c, 0) > c.w * bps
        # the kernel's int arithmetic: every sum before the >> 16 fits 32 bits
        assert int(np.abs(C.rgb_unclipped(c)).max()) < 1 << 15, c.name
    assert 2 * padded >= len(RGB)
    c4 = next(c for c in RGB if (c.w, c.h, c.chroma) == (5, 3, 1))  # ceil: 4:2:0 of 5 x 3 is 3 x 2
    assert C.rgb_samples(c4)[1].shape == (2, 3)
    c2 = next(c for c in RGB if (c.w, c.h, c.chroma) == (5, 3, 2))
    assert C.rgb_samples(c2)[1].shape == (3, 3)


def test_rgb_cases_clip_both_ways_in_every_channel():
    seen = 0
    for c in RGB:
        if c.chroma == 0 or (c.w, c.h) in ((1, 1), (5, 3)):  # the two geometry cases
            continue
        u = C.rgb_unclipped(c)
        for ch in range(3):
            assert (u[..., ch] < 0).any(), (c.name, ch, "below")
            assert (u[..., ch] > 255).any(), (c.name, ch, "above")
        assert ((u >= 0) & (u <= 255)).all(axis=-1).any(), c.name
        seen += 1
    assert seen == len([c for c in RGB if c.chroma and (c.w, c.h) not in ((1, 1), (5, 3))])


def test_rgb_limited_range_mono_clips_at_both_ends():
    seen = 0
    for c in RGB:
        if c.chroma or c.full or (c.w, c.h) in ((1, 1), (5, 3)):
            continue
        u = C.rgb_unclipped(c)
        assert (u < 0).any() and (u > 255).any(), c.name
        assert (u[..., 0] == u[..., 1]).all() and (u[..., 0] == u[..., 2]).all()
        seen += 1
    assert seen >= 8


def test_rgb_deep_samples_have_bits_below_the_shift():
    for c in RGB:
        if c.depth > 8:
            mask = (1 << (c.depth - 8)) - 1
            for a in C.rgb_samples(c):
                if a is not None and a.size >= 64:
                    assert (a & mask).any(), c.name
    for depth in C.DEPTHS[1:]:
        assert any(c.depth == depth and (C.rgb_samples(c)[0] & ((1 << (depth - 8)) - 1)).any() for c in RGB)


def test_rgb_store_paths():
    n = total(C.rgb_rows(c) for c in RGB)
    assert n["full_aligned"] > 0 and n["full_unaligned"] > 0
    assert n["partial1"] > 0 and n["partial2"] > 0 and n["partial3"] > 0
    assert max(C.rgb_rows(c)["groups_per_row"] for c in RGB) > 256  # a second workgroup along x
    # for every rotation and sample width, full groups both ways
    for rot, bps in itertools.product(range(4), (1, 2)):
        m = total(C.rgb_rows(c) for c in RGB if c.rot == rot and C.rgb_bps(c) == bps)
        assert m["full_aligned"] > 0 and m["full_unaligned"] > 0, (rot, bps)
    # rows of a multiple of 4 bytes start unaligned only through a base offset or a padded pitch
    even = total(C.rgb_rows(c) for c in RGB if 3 * C.rgb_out_dims(c)[0] % 4 == 0)
    assert even["full_aligned"] > 0 and even["full_unaligned"] > 0
    tight = total(C.rgb_rows(c) for c in RGB if 3 * C.rgb_out_dims(c)[0] % 4 == 0 and not c.pad and not c.off)
    assert tight["full_aligned"] > 0 and tight["full_unaligned"] == 0
    # the wide picture's last group has 2 pixels, at rotations 0 and 2; turned, it is 6 wide
    wide = [c for c in RGB if (c.w, c.h) == (1030, 6)]
    assert {C.rgb_out_dims(c) for c in wide if not c.rot & 1} == {(1030, 6)}
    assert {C.rgb_out_dims(c) for c in wide if c.rot & 1} == {(6, 1030)}
    assert all(C.rgb_rows(c)["partial2"] for c in wide)


def test_rgb_expected_buffers():
    """The buffer's frame, and the rotation stated from the header alone (anticlockwise,
    90 degrees per unit): where the coded picture's corners and one inner sample land."""
    for c in RGB:
        ow, oh = C.rgb_out_dims(c)
        pitch = C.rgb_pitch(c)
        assert pitch == 3 * ow + c.pad and pitch >= 3 * ow
        want = C.rgb_expected(c)
        blank = C.rgb_blank(c)
        assert want.size == blank.size == 2 * C.GUARD + c.off + oh * pitch and (blank == C.SENTINEL).all()
        assert (want[:C.GUARD + c.off] == C.SENTINEL).all() and (want[-C.GUARD:] == C.SENTINEL).all()
        rows = C.rows_of(want, c.off, oh, pitch)
        assert (rows[:, 3 * ow:] == C.SENTINEL).all()
        px = rows[:, :3 * ow].reshape(oh, ow, 3)
        src = np.clip(C.rgb_unclipped(c), 0, 255)
        W, H = c.w - 1, c.h - 1
        for x, y in {(0, 0), (W, 0), (0, H), (W, H), (W // 3, H // 2)}:
            ox, oy = ((x, y), (y, W - x), (W - x, H - y), (H - y, x))[c.rot]
            assert tuple(px[oy, ox]) == tuple(src[y, x]), (c.name, x, y)


def test_rgb_model_by_hand():
    """BT.601 full range: Cr = 255 adds round(1.402 * 127) to R; limited range scales
    luma by 255 / 219 from 16."""
    y = np.array([[100]], np.uint8)
    u = rgb_ref.unclipped(y, np.array([[128]], np.uint8), np.array([[255]], np.uint8), 6, True)
    assert u[0, 0].tolist() == [278, 9, 100]  # 100 + 178.05, 100 - 0.714136 * 127, 100
    assert rgb_ref.unclipped(np.array([[235 << 2 | 3]], np.uint16), None, None, 1, False, 10)[0, 0].tolist() == [255] * 3
    assert rgb_ref.unclipped(np.array([[0]], np.uint8), None, None, 9, False)[0, 0].tolist() == [-19] * 3


# ---- the gather model --------------------------------------------------------------------------
GRID = SimpleNamespace(width=300, height=200, chroma_format_idc=1, bytes_per_sample=1, grid_rows=3, grid_cols=3,
                       tile_width=128, tile_height=96, num_tiles=9)


def test_gather_windows_by_hand():
    assert gather_ref.plane_dims(GRID, 0) == (300, 200) and gather_ref.plane_dims(GRID, 1) == (150, 100)
    assert gather_ref.window(GRID, 4, 0) == (128, 96, 128, 96)
    assert gather_ref.window(GRID, 4, 1) == (64, 48, 64, 48) == gather_ref.window(GRID, 4, 2)
    assert gather_ref.window(GRID, 2, 0) == (256, 0, 44, 96)  # the last column, clipped
    assert gather_ref.window(GRID, 2, 1) == (128, 0, 22, 48)
    assert gather_ref.window(GRID, 8, 0) == (256, 192, 44, 8)  # and the last row
    assert gather_ref.window(GRID, 8, 2) == (128, 96, 22, 4)
    odd = SimpleNamespace(width=37, height=23, chroma_format_idc=1, bytes_per_sample=1, grid_rows=0, grid_cols=0,
                          tile_width=0, tile_height=0, num_tiles=0)
    assert gather_ref.tiles(odd) == 1
    assert gather_ref.window(odd, 0, 0) == (0, 0, 37, 23) and gather_ref.window(odd, 0, 1) == (0, 0, 19, 12)
    g422 = SimpleNamespace(**{**vars(GRID), "chroma_format_idc": 2})
    assert gather_ref.plane_dims(g422, 1) == (150, 200) and gather_ref.window(g422, 8, 1) == (128, 192, 22, 8)
    beyond = C.gather_info(C.GATHER_BY_NAME["beyond"])
    assert gather_ref.window(beyond, 2, 0) is None and gather_ref.window(beyond, 5, 1) is None  # 128 >= 100, 64 >= 50
    assert gather_ref.window(beyond, 4, 0) == (64, 32, 36, 8) and gather_ref.window(beyond, 4, 1) == (32, 16, 18, 4)
    assert gather_ref.selected(GRID, 4, 3) == [3, 7] and gather_ref.selected(GRID, 0, 0) == list(range(9))
    assert gather_ref.selected(GRID, 16, 9) == []
    with pytest.raises(ValueError):
        gather_ref.selected(GRID, 2, 2)


def test_gather_copies_windows_and_nothing_else():
    r = np.random.default_rng(5)
    src = [r.integers(0, 256, size=(200, 310), dtype=np.uint8)] + [r.integers(0, 256, size=(100, 152), dtype=np.uint8)
                                                                  for _ in range(2)]
    dst = [np.full((200, 300), 7, np.uint8), np.full((100, 150), 7, np.uint8), np.full((100, 150), 7, np.uint8)]
    kept = [d.copy() for d in dst]
    got = gather_ref.gather(dst, src, GRID, 16, 9)  # selects no tile
    assert all(np.array_equal(g, k) for g, k in zip(got, kept))
    got = gather_ref.gather(dst, src, GRID, 4, 3)  # tiles 3 and 7
    assert all(np.array_equal(d, k) for d, k in zip(dst, kept))  # the argument is not written
    want = kept[0].copy()
    want[96:192, 0:128] = src[0][96:192, 0:128]
    want[192:200, 128:256] = src[0][192:200, 128:256]
    assert np.array_equal(got[0], want)
    want = kept[2].copy()
    want[48:96, 0:64] = src[2][48:96, 0:64]
    want[96:100, 64:128] = src[2][96:100, 64:128]
    assert np.array_equal(got[2], want)
    full = gather_ref.gather(dst, src, GRID, 0, 0)
    assert np.array_equal(full[0], src[0][:, :300]) and np.array_equal(full[1], src[1][:, :150])
    # 16-bit samples: windows in bytes
    g16 = SimpleNamespace(**{**vars(GRID), "bytes_per_sample": 2, "chroma_format_idc": 0})
    s16, d16 = r.integers(0, 256, size=(200, 600), dtype=np.uint8), np.zeros((200, 640), np.uint8)
    got = gather_ref.gather([d16, None, None], [s16, None, None], g16, 9, 2)
    assert np.array_equal(got[0][0:96, 512:600], s16[0:96, 512:600]) and not got[0][:, 600:].any()
    assert not got[0][:, :512].any() and not got[0][96:].any()


# ---- the k_gather_tiles list -------------------------------------------------------------------
def test_gather_case_list():
    names = [c.name for c in C.GATHER_CASES]
    assert names == ["grid420_8", "grid422_16", "unaligned_x0", "mono", "wide", "odd_nogrid", "beyond", "dst_off3"]
    by = C.GATHER_BY_NAME
    assert set(by["grid420_8"].pairs) >= {(1, 0), (2, 0), (2, 1), (4, 3), (16, 3), (16, 9)}
    assert C.gather_chunks(by["grid420_8"], 16, 9) == Counter()  # nothing selected: no launch
    assert any(s == 0 for c in C.GATHER_CASES for s, _ in c.pairs)
    for c in C.GATHER_CASES:
        assert (1, 0) in c.pairs and all(o < max(s, 1) for s, o in c.pairs)
        info = C.gather_info(c)
        for k in range(C.gather_planes(c)):
            pw, ph = gather_ref.plane_dims(info, k)
            assert c.dpitch[k] >= pw * c.bps and c.spitch[k] >= pw * c.bps
            assert c.dpitch[k] % c.bps == 0 and c.spitch[k] % c.bps == 0
    for name in ("grid422_16", "unaligned_x0", "wide", "dst_off3"):
        assert all(p % 16 == 0 for p in by[name].dpitch + by[name].spitch), name
    assert by["grid422_16"].dpitch != by["grid422_16"].spitch
    assert C.gather_planes(by["mono"]) == 1 and by["dst_off3"].doff == 3


def test_gather_copy_paths():
    by = C.GATHER_BY_NAME
    per = {c.name: total(C.gather_chunks(c, s, o) for s, o in c.pairs) for c in C.GATHER_CASES}
    n = total(per.values())
    assert n["vector"] > 0 and n["bytes"] > 0 and n["tail"] > 0 and n["second_step"] > 0 and n["skipped"] > 0
    # what each case was drawn up for
    g = C.gather_chunks(by["grid422_16"], 9, 2)  # the 88-byte last column: 5 vectors and a tail per row
    assert g["bytes"] == 0 and g["vector"] == 96 * 5 + 2 * 96 * 2 and g["tail"] == 3 * 96
    u = [C.gather_chunks(by["unaligned_x0"], 9, k) for k in range(3)]
    assert u[0]["bytes"] == 0 and u[1]["vector"] == 0 and u[1]["bytes"] > 0 and u[2]["bytes"] == 0
    w = C.gather_chunks(by["wide"], 4, 1)  # column 1 at byte 1150: bytes, over two steps
    assert w["vector"] == 0 and w["second_step"] > 0
    w = C.gather_chunks(by["wide"], 4, 0)
    assert w["bytes"] == 0 and w["vector"] > 0 and w["second_step"] > 0 and w["tail"] > 0
    assert per["beyond"]["skipped"] > 0 and per["grid420_8"]["bytes"] > 0
    assert per["dst_off3"]["vector"] == 0 and per["dst_off3"]["bytes"] > 0
    assert per["mono"]["vector"] > 0 and per["mono"]["bytes"] > 0  # a 260-byte pitch: every fourth row aligned
    assert per["odd_nogrid"]["skipped"] == 0


def test_gather_expected_buffers():
    for c in C.GATHER_CASES:
        src = C.gather_sources(c)
        info = C.gather_info(c)
        for s, o in c.pairs:
            bufs = C.gather_expected(c, s, o)
            copied = 0
            for k, b in enumerate(bufs):
                assert b.size == C.gather_blank(c, k).size
                assert (b[:C.GUARD + c.doff] == C.SENTINEL).all() and (b[-C.GUARD:] == C.SENTINEL).all()
                rows = C.rows_of(b, c.doff, C.gather_rows(c, k), c.dpitch[k])
                pw = gather_ref.plane_dims(info, k)[0] * c.bps
                assert (rows[:, pw:] == C.SENTINEL).all()
                from_src = rows[:, :pw] == C.rows_of(src[k], 0, C.gather_rows(c, k), c.spitch[k])[:, :pw]
                assert (from_src | (rows[:, :pw] == C.SENTINEL)).all()
                copied += int((rows != C.SENTINEL).sum())
            windows = [gather_ref.window(info, k, 0) for k in gather_ref.selected(info, s, o)]
            assert (copied == 0) == (not any(windows)), (c.name, s, o)
    # stride 0 is stride 1, and the whole picture then comes across (but the skipped column of "beyond")
    for c in C.GATHER_CASES:
        a, b = C.gather_expected(c, 0, 0), C.gather_expected(c, 1, 0)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    y = C.rows_of(C.gather_expected(C.GATHER_BY_NAME["odd_nogrid"], 1, 0)[1], 0, 12, 19)
    assert np.array_equal(y, C.rows_of(C.gather_sources(C.GATHER_BY_NAME["odd_nogrid"])[1], 0, 12, 19))
