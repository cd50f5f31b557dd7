"""The PNG output without a GPU: the model (tests/png_ref.py) pinned from outside (zlib inflates
it, a plain reader written here un-filters it to the input samples, zlib.crc32 confirms every
chunk, Pillow opens the 8-bit files and finds the profile), its size against zlib's Huffman-only
coding, and the host restatement (heifgpu_png_encode_host, heifgpu_png_header) and the kernels
under the host emulation (make png-emu, a stand-alone ASan + UBSan program) byte for byte
against the model on every case of tests/png_cases.py."""
import ctypes
import io
import pathlib
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases as pc
import png_ref as ref
from conftest import make_emu
from heif_amd import _lib

CSRC = pathlib.Path(__file__).resolve().parents[1] / "heif_amd" / "csrc"
SENTINEL = 0xA5
NAMES = [c.name for c in pc.CASES]
# The largest ratio of the model's deflate payload to zlib's Z_HUFFMAN_ONLY coding of the same
# pieces over the photo-like cases, as measured: "photo" 336563 / 336225 = 1.00101,
# "photo_rgba" 25647 / 25612 = 1.00137 (what the code lengths cost without repeat codes).
WORST_RATIO = 1.00137


def chunks(data):
    """[(type, data)] of a file, every CRC confirmed by zlib."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack_from(">I", data, at)
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert zlib.crc32(kind + body) == struct.unpack_from(">I", data, at + 8 + n)[0], kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


def unfilter(stream, h, row, bpp):
    """A plain PNG reader's un-filtering: (h, row) uint8."""
    out = np.zeros((h, row), np.uint8)
    for y in range(h):
        line = stream[y * (row + 1):(y + 1) * (row + 1)]
        t, cur = line[0], out[y]
        up = out[y - 1] if y else np.zeros(row, np.uint8)
        for i in range(row):
            a = int(cur[i - bpp]) if i >= bpp else 0
            b = int(up[i])
            c = int(up[i - bpp]) if i >= bpp else 0
            if t == 0:
                pred = 0
            elif t == 1:
                pred = a
            elif t == 2:
                pred = b
            elif t == 3:
                pred = (a + b) // 2
            else:
                assert t == 4
                p = a + b - c
                pa, pb, pcc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pcc else b if pb <= pcc else c
            cur[i] = (line[1 + i] + pred) & 255
    return out


# ---------------------------------------------------------------- the model, pinned from outside
@pytest.mark.parametrize("name", [n for n in NAMES if n != "photo"])
def test_model_inflates_and_unfilters_to_the_input(name):
    check_model_file(name)


def test_model_inflates_and_unfilters_to_the_input_photo():
    """The 512 x 384 crop: its first 24 rows through the plain reader (rows do not depend on later ones)."""
    check_model_file("photo", rows=24)


def check_model_file(name, rows=None):
    c = pc.BY_NAME[name]
    data, head, _ = pc.reference(name)
    h, w, ch = c.px.shape
    cs = chunks(data)
    kinds = [k for k, _ in cs]
    wide = c.fmt.endswith("16")
    want = [b"IHDR"] + ([b"sBIT"] if wide and c.bits < 16 else []) + ([b"sRGB"] if c.srgb else []) + \
        ([b"cICP"] if c.cicp else []) + ([b"iCCP"] if c.icc else [])
    assert kinds[:len(want)] == want and set(kinds[len(want):-1]) == {b"IDAT"}
    assert cs[0][1] == struct.pack(">IIBBBBB", w, h, 16 if wide else 8, 6 if ch == 4 else 2, 0, 0, 0)
    idat = [b for k, b in cs if k == b"IDAT"]
    stream = zlib.decompress(b"".join(idat))
    row = w * c.bpp
    assert len(stream) == h * (row + 1) and len(idat) == -(-len(stream) // ref.BLOCK)
    n = h if rows is None else rows
    raw = unfilter(stream, n, row, c.bpp)
    if wide:
        v = raw.reshape(n, w, ch, 2).astype(np.uint16)
        got = ((v[..., 0] << 8) | v[..., 1]) >> (16 - c.bits)
        assert dict(cs).get(b"sBIT", bytes([16] * ch)) == bytes([c.bits] * ch)
    else:
        got = raw.reshape(n, w, ch)
    assert np.array_equal(got, c.px[:n])
    if c.cicp:
        assert dict(cs)[b"cICP"] == bytes(c.cicp)


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.fmt.endswith("8")])
def test_pillow_opens_model_output(name):
    c = pc.BY_NAME[name]
    im = Image.open(io.BytesIO(pc.reference(name)[0]))
    im.load()
    assert im.mode == ("RGBA" if c.fmt == "rgba8" else "RGB")
    assert np.array_equal(np.asarray(im), c.px)
    if c.icc is not None:
        assert im.info["icc_profile"] == c.icc
    else:
        assert "icc_profile" not in im.info


def huffman_only_size(stream):
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    n = 0
    for at in range(0, len(stream), ref.BLOCK):
        n += len(z.compress(stream[at:at + ref.BLOCK])) + len(z.flush(zlib.Z_SYNC_FLUSH))
    return n + len(z.flush())


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.photo])
def test_size_against_zlibs_huffman_only(name):
    """The deflate payload (the IDAT chunks' data) against zlib's Huffman-only coding of the same
    filtered bytes in the same 32768-byte pieces, a sync flush after each."""
    data, _, facts = pc.reference(name)
    ours = sum(len(b) for k, b in chunks(data) if k == b"IDAT")
    theirs = huffman_only_size(facts["stream"])
    print(f"{name}: deflate payload {ours} bytes, zlib Z_HUFFMAN_ONLY {theirs} bytes, ratio {ours / theirs:.5f}")
    assert ours / theirs <= WORST_RATIO + 0.002


# ---------------------------------------------------------------- the host restatement
def opts_of(c):
    return _lib.PngOpts(pc.FORMAT_CODES[c.fmt], c.bits, c.filt, 0)


def colour_of(c):
    """(heifgpu_png_colour, what must outlive it)"""
    col, keep = _lib.PngColour(), None
    if c.srgb:
        col.kind = _lib.PNG_COLOUR_SRGB
    elif c.cicp:
        col.kind = _lib.PNG_COLOUR_CICP
        col.cicp[:] = c.cicp
    elif c.icc:
        keep = _lib.u8buf(c.icc)
        col.kind, col.icc, col.icc_len = _lib.PNG_COLOUR_ICC, ctypes.cast(keep, ctypes.POINTER(ctypes.c_uint8)), len(c.icc)
    return col, keep


def host_header(c):
    h, w, _ = c.px.shape
    o, (col, keep) = opts_of(c), colour_of(c)
    n = ctypes.c_size_t()
    assert _lib.lib.heifgpu_png_header(w, h, ctypes.byref(o), ctypes.byref(col), None, 0, ctypes.byref(n)) == 0
    buf = (ctypes.c_uint8 * n.value)()
    assert _lib.lib.heifgpu_png_header(w, h, ctypes.byref(o), ctypes.byref(col), buf, n.value, ctypes.byref(n)) == 0
    return bytes(buf)


def host_encode(c):
    buf, pitch = pc.surface(c)
    h, w, _ = c.px.shape
    o, (col, keep) = opts_of(c), colour_of(c)
    n = ctypes.c_size_t()
    args = (ctypes.c_void_p(buf.ctypes.data + c.lead), pitch, w, h, ctypes.byref(o), ctypes.byref(col))
    assert _lib.lib.heifgpu_png_encode_host(*args, None, 0, ctypes.byref(n)) == 0, _lib.last_error()
    out = (ctypes.c_uint8 * (n.value + 16))(*([SENTINEL] * (n.value + 16)))
    assert _lib.lib.heifgpu_png_encode_host(*args, out, n.value, ctypes.byref(n)) == 0
    assert bytes(out[n.value:]) == bytes([SENTINEL]) * 16
    return bytes(out[:n.value])


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_equals_model(name):
    c = pc.BY_NAME[name]
    data, head, _ = pc.reference(name)
    assert host_header(c) == data[:head]
    assert host_encode(c) == data


def test_host_calls_refuse_bad_arguments():
    n = ctypes.c_size_t()
    px = (ctypes.c_uint8 * 256)()
    O = _lib.PngOpts
    good = O(0, 8, 5, 0)
    bad = [(4, 4, O(4, 8, 5, 0)), (4, 4, O(0, 7, 5, 0)), (4, 4, O(0, 9, 5, 0)), (4, 4, O(1, 16, 5, 0)), (4, 4, O(2, 7, 5, 0)),
           (4, 4, O(3, 17, 5, 0)), (4, 4, O(0, 8, 6, 0)), (4, 4, O(0, 8, 5, 1)), (0, 4, good), (4, 0, good), (65536, 4, good),
           (4, 65536, good)]
    for w, h, o in bad:
        assert _lib.lib.heifgpu_png_header(w, h, ctypes.byref(o), None, None, 0, ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID
        assert _lib.lib.heifgpu_png_encode_host(px, 64, w, h, ctypes.byref(o), None, None, 0,
                                                ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID
    for o, pitch in ((good, 11), (O(1, 8, 5, 0), 15), (O(2, 10, 5, 0), 23), (O(3, 16, 5, 0), 31)):  # a pitch one byte short
        assert _lib.lib.heifgpu_png_encode_host(px, pitch, 4, 4, ctypes.byref(o), None, None, 0,
                                                ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID
        assert _lib.lib.heifgpu_png_encode_host(px, pitch + 1, 4, 4, ctypes.byref(o), None, None, 0, ctypes.byref(n)) == 0
    col = _lib.PngColour(_lib.PNG_COLOUR_ICC)  # a profile of no bytes
    assert _lib.lib.heifgpu_png_header(4, 4, ctypes.byref(good), ctypes.byref(col), None, 0, ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID
    col = _lib.PngColour(4)
    assert _lib.lib.heifgpu_png_header(4, 4, ctypes.byref(good), ctypes.byref(col), None, 0, ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_png_header(4, 4, ctypes.byref(good), None, None, 0, ctypes.byref(n)) == 0 and n.value == 33


# ---------------------------------------------------------------- the kernels under the emulation
def case_file(batches, caps):
    """tests/png/png_driver.cpp's input: caps[name] is each picture's output capacity."""
    out = [struct.pack("<2I", 0x31474E50, len(batches))]
    for b in batches:
        fmt, bits, filt = b[0].opts
        assert all(c.opts == b[0].opts for c in b)
        out.append(struct.pack("<8I", len(b), pc.FORMAT_CODES[fmt], bits, filt, SENTINEL, 0, 0, 0))
        for c in b:
            buf, pitch = pc.surface(c)
            h, w, _ = c.px.shape
            out.append(struct.pack("<6I", w, h, pitch, c.lead, len(buf), caps[c.name]))
            out.append(buf.tobytes())
    return b"".join(out)


def run_driver(driver, tmp_path, batches, caps):
    """{name: (size word, the output buffer's bytes)}"""
    cf, rf = tmp_path / "case.bin", tmp_path / "result.bin"
    cf.write_bytes(case_file(batches, caps))
    r = subprocess.run([str(driver), str(cf), str(rf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"driver failed ({r.returncode}): {r.stderr[-4000:]}"
    data, at, res = rf.read_bytes(), 0, {}
    for b in batches:
        for c in b:
            size, = struct.unpack_from("<Q", data, at)
            res[c.name] = (size, data[at + 8:at + 8 + caps[c.name]])
            at += 8 + caps[c.name]
    assert at == len(data)
    return res


@pytest.fixture(scope="module")
def emu_driver():
    make_emu("png-emu")
    return CSRC / "build" / "png_emu" / "png_driver"


def body_of(name):
    data, head, _ = pc.reference(name)
    return data[head:]


def test_kernels_under_emulation_equal_model(emu_driver, tmp_path):
    """Every case, with 7 bytes of room behind the exact size: the IDAT chunks and IEND equal the
    model's, the size is exact and the room keeps the sentinel."""
    bodies = {n: body_of(n) for n in NAMES}
    caps = {n: len(s) + 7 for n, s in bodies.items()}
    res = run_driver(emu_driver, tmp_path, pc.BATCHES, caps)
    for n in NAMES:
        size, buf = res[n]
        assert size == len(bodies[n]), n
        assert buf[:size] == bodies[n], n
        assert buf[size:] == bytes([SENTINEL]) * 7, n


def test_too_small_capacity_under_emulation(emu_driver, tmp_path):
    """Capacities of 0, 1, half the bytes and one byte short, in exact-size heap blocks under ASan,
    for a picture of one block and one of three: the bytes that fit are the first, and the size
    comes back with bit 63 set."""
    batches, caps, want = [], {}, {}
    for base in (pc.BY_NAME["mixed_0"], pc.BY_NAME["stream_65540"]):
        body = body_of(base.name)
        for k, cap in enumerate((0, 1, len(body) // 2, len(body) - 1, len(body))):
            c = pc.Case(f"{base.name}_cap_{k}", base.px, base.fmt, base.bits, base.filt, base.pad, base.lead)
            batches.append([c])
            caps[c.name], want[c.name] = cap, (cap, body)
    res = run_driver(emu_driver, tmp_path, batches, caps)
    for n, (cap, body) in want.items():
        size, buf = res[n]
        assert size == len(body) | (_lib.PNG_TOO_SMALL if cap < len(body) else 0), n
        assert buf == body[:cap], n


# ---------------------------------------------------------------- what the cases reach
def test_case_list_reaches_every_path():
    facts = {n: pc.reference(n)[2] for n in NAMES}
    adaptive = [n for n in NAMES if pc.BY_NAME[n].filt == ref.ADAPTIVE]
    assert set(facts["filter_rows"]["types"][:5]) == {0, 1, 2, 3, 4}           # each type as an adaptive choice
    assert facts["filter_rows"]["types"][:5] == [0, 1, 2, 4, 3]
    assert {0, 2} <= set(facts["filter_rows"]["ties"])                        # a tie between types
    assert {pc.BY_NAME[n].filt for n in NAMES} == {0, 1, 2, 3, 4, 5}
    blocks = {n: f["blocks"] for n, f in facts.items()}
    assert any(b["repair15"] for b in blocks["fibonacci"])                    # the 15-bit repair
    assert max(blocks["fibonacci"][0]["lit"]) == 15
    assert any(b["repair7"] for b in blocks["dyadic"])                        # the 7-bit repair
    assert blocks["zeros"][0]["distinct"] == 1                                # a block of one distinct byte
    assert blocks["ramp256"][0]["distinct"] == 256                            # all 256 values in one block
    assert [len(facts[n]["stream"]) for n in ("stream_32767", "stream_32768", "stream_32769", "stream_65540")] == \
        [32767, 32768, 32769, 65540]
    assert [len(blocks[n]) for n in ("stream_32767", "stream_32768", "stream_32769", "stream_65540")] == [1, 1, 2, 3]
    assert len(blocks["photo"]) > 8                                           # a multi-block picture
    assert {c.fmt for c in pc.CASES} == {"rgb8", "rgba8", "rgb16", "rgba16"}
    assert {(c.fmt, c.bits) for c in pc.CASES} >= {("rgba16", 10), ("rgb16", 12), ("rgba16", 16), ("rgba16", 8)}
    assert {c.px.shape[:2] for c in pc.CASES} >= {(1, 1), (3, 5)}
    assert any(c.pad and c.lead % 4 == 1 for c in pc.CASES)                   # a start address 1 byte past a dword
    assert sorted(len(b) for b in pc.BATCHES)[-1] == 3 and len({c.px.shape for c in pc.BATCHES[0]}) == 3
    assert any(c.srgb for c in pc.CASES) and any(c.cicp for c in pc.CASES) and any(c.icc and len(c.icc) > 65535 for c in pc.CASES)
    assert adaptive
