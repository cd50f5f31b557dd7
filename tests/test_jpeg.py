"""The JPEG output without a GPU: the tables against what Pillow writes, the numpy model
(tests/jpeg_ref.py) against Pillow's decoder and encoder and against an ideal DCT, and
the host restatement (heifgpu_jpeg_encode_host, heifgpu_jpeg_header) and the kernels under
the host emulation (make jpeg-emu, a stand-alone ASan + UBSan program) byte for byte against
the model on every case of tests/jpeg_cases.py."""
import ctypes
import io
import pathlib
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import jpeg_ref as ref
from conftest import make_emu
from heif_amd import _lib

CSRC = pathlib.Path(__file__).resolve().parents[1] / "heif_amd" / "csrc"
SENTINEL = 0xA5
NAMES = [c.name for c in jc.CASES]


def opts_of(quality, sub, restart):
    return _lib.JpegOpts(quality, _lib.JPEG_SUBSAMPLINGS[sub], restart, 0)


def pillow_file(rgb, quality, sub):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=sub, optimize=False)
    return b.getvalue()


def segments(data):
    """(marker, payload) of every segment up to and including SOS."""
    i, out = 2, []
    while True:
        assert data[i] == 0xFF
        n = int.from_bytes(data[i + 2:i + 4], "big")
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        if data[i + 1] == 0xDA:
            return out
        i += 2 + n


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("quality", [1, 10, 25, 50, 75, 90, 95, 100])
def test_quant_tables_equal_pillows(quality):
    luma, chroma = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    assert _lib.lib.heifgpu_jpeg_quant_tables(quality, luma, chroma) == _lib.HEIFGPU_OK
    q = Image.open(io.BytesIO(pillow_file(jc.smooth(16, 16), quality, "4:2:0"))).quantization
    assert list(luma) == list(q[0]) and list(chroma) == list(q[1])
    assert [list(t) for t in ref.quant_tables(quality)] == [list(luma), list(chroma)]


def test_huffman_tables_equal_pillows():
    """The four DHT segments of the header and of the model are those of a file Pillow saves with optimize=False."""
    theirs = {p[0]: bytes(p[1:]) for m, p in segments(pillow_file(jc.smooth(16, 16), 75, "4:2:0")) if m == 0xC4}
    assert sorted(theirs) == [0x00, 0x01, 0x10, 0x11]
    for head in (host_header(16, 16, (75, "4:2:0", 0), None), ref.header(16, 16, 75, "4:2:0")):
        ours = {p[0]: bytes(p[1:]) for m, p in segments(head) if m == 0xC4}
        assert ours == theirs


def test_quant_tables_refuse_bad_quality():
    t = (ctypes.c_uint8 * 64)()
    for q in (0, 101):
        assert _lib.lib.heifgpu_jpeg_quant_tables(q, t, t) == _lib.HEIFGPU_E_INVALID


# ---------------------------------------------------------------- the model against Pillow
@pytest.mark.parametrize("name", NAMES)
def test_pillow_decodes_model_output(name):
    c = jc.BY_NAME[name]
    data, _, _ = jc.reference(name)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (c.rgb.shape[1], c.rgb.shape[0]) and im.mode == "RGB"
    if c.icc is not None:
        assert im.info["icc_profile"] == c.icc
    else:
        assert "icc_profile" not in im.info


@pytest.mark.parametrize("name", NAMES)
def test_vectorised_model_equals_model(name):
    c = jc.BY_NAME[name]
    data, head, _ = jc.reference(name)
    assert ref.scan_fast(c.rgb, c.quality, c.sub, c.restart) == data[head:]


def test_icc_200k_takes_four_chunks():
    data, _, _ = jc.reference("icc_200k")
    assert sum(1 for m, _ in segments(data) if m == 0xE2) == 4


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def quality_picture():
    """256 x 192: gradients under seeded noise whose strength grows from left to right."""
    y, x = np.mgrid[0:192, 0:256]
    rng = np.random.default_rng(2024)
    base = np.stack([x * 0.9 + y * 0.1, 255 - y * 1.2, (x + y) * 0.5], -1)
    tex = rng.normal(0, 1, (192, 256, 3)) * (x[..., None] / 255.0) * 24
    return np.clip(np.rint(base + tex), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("sub", jc.SUBS)
@pytest.mark.parametrize("quality", [50, 90])
def test_quality_against_pillows_encoder(quality, sub):
    """Our file decodes (by Pillow) to within 0.3 dB of what Pillow's own file at the same settings
    decodes to, and is at most 5 % larger once the restart markers are taken off."""
    rgb = quality_picture()
    st = {}
    ours = ref.encode(rgb, quality, sub, 0, stats=st)
    theirs = pillow_file(rgb, quality, sub)
    p_ours = psnr(np.asarray(Image.open(io.BytesIO(ours))), rgb)
    p_theirs = psnr(np.asarray(Image.open(io.BytesIO(theirs))), rgb)
    size_ours = len(ours) - 2 * (st["intervals"] - 1)  # without the RSTm markers
    print(f"Q{quality} {sub}: PSNR ours {p_ours:.3f} dB, Pillow {p_theirs:.3f} dB; bytes ours {size_ours}, Pillow {len(theirs)}")
    assert p_ours >= p_theirs - 0.3
    assert size_ours <= 1.05 * len(theirs)


def test_fdct_accuracy():
    """The unquantised coefficients against scipy's orthonormal DCT in float64: at most 1/4 off."""
    from scipy.fft import dctn, idctn

    rng = np.random.default_rng(7)
    blocks = [rng.integers(0, 256, (2000, 8, 8)), np.zeros((1, 8, 8)), np.full((1, 8, 8), 255)]
    k = np.arange(8)
    checker = np.where((k[:, None] + k[None, :]) % 2 == 0, 255, 0)
    blocks += [checker[None], (255 - checker)[None]]
    for i in range(64):  # each basis function at full amplitude, both signs
        e = np.zeros(64)
        e[i] = 1
        b = idctn(e.reshape(8, 8), norm="ortho")
        b = b / np.abs(b).max()
        blocks += [np.rint(127.5 + 127.5 * b)[None], np.rint(127.5 - 127.5 * b)[None]]
    p = np.concatenate(blocks).astype(np.int64) - 128
    got = ref.fdct(p) / 2.0 ** 20
    want = dctn(p.astype(np.float64), axes=(1, 2), norm="ortho")
    err = np.abs(got - want).max()
    print(f"max |model - ideal| = {err:.4f}")
    assert err <= 0.25


# ---------------------------------------------------------------- the host restatement
def host_header(w, h, opts, icc):
    o = opts_of(*opts)
    n = ctypes.c_size_t()
    icc = icc or b""
    assert _lib.lib.heifgpu_jpeg_header(w, h, ctypes.byref(o), _lib.u8buf(icc), len(icc), None, 0, ctypes.byref(n)) == 0
    buf = (ctypes.c_uint8 * n.value)()
    assert _lib.lib.heifgpu_jpeg_header(w, h, ctypes.byref(o), _lib.u8buf(icc), len(icc), buf, n.value, ctypes.byref(n)) == 0
    return bytes(buf)


def host_encode(c):
    buf, pitch = jc.surface(c)
    h, w, _ = c.rgb.shape
    o = opts_of(*c.opts)
    icc = c.icc or b""
    n = ctypes.c_size_t()
    src = buf.ctypes.data + c.lead
    args = (ctypes.c_void_p(src), pitch, w, h, ctypes.byref(o), _lib.u8buf(icc), len(icc))
    assert _lib.lib.heifgpu_jpeg_encode_host(*args, None, 0, ctypes.byref(n)) == 0, _lib.last_error()
    out = (ctypes.c_uint8 * (n.value + 16))(*([SENTINEL] * (n.value + 16)))
    assert _lib.lib.heifgpu_jpeg_encode_host(*args, out, n.value, ctypes.byref(n)) == 0
    assert bytes(out[n.value:]) == bytes([SENTINEL]) * 16
    return bytes(out[:n.value])


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_equals_model(name):
    c = jc.BY_NAME[name]
    data, head, _ = jc.reference(name)
    assert host_header(c.rgb.shape[1], c.rgb.shape[0], c.opts, c.icc) == data[:head]
    assert host_encode(c) == data


def test_host_calls_refuse_bad_arguments():
    n = ctypes.c_size_t()
    px = (ctypes.c_uint8 * 48)()
    good = opts_of(90, "4:2:0", 0)
    for w, h, o in ((0, 4, good), (4, 0, good), (65536, 4, good), (4, 65536, good), (4, 4, opts_of(0, "4:2:0", 0)),
                    (4, 4, opts_of(101, "4:2:0", 0)), (4, 4, _lib.JpegOpts(90, 2, 0, 0)), (4, 4, opts_of(90, "4:2:0", 65536))):
        assert _lib.lib.heifgpu_jpeg_header(w, h, ctypes.byref(o), None, 0, None, 0, ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID
    assert _lib.lib.heifgpu_jpeg_encode_host(px, 11, 4, 4, ctypes.byref(good), None, 0, None, 0,
                                             ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID  # pitch below 3 * width
    assert _lib.lib.heifgpu_jpeg_header(4, 4, ctypes.byref(good), None, 255 * 65519 + 1, None, 0,
                                        ctypes.byref(n)) == _lib.HEIFGPU_E_INVALID


# ---------------------------------------------------------------- the kernels under the emulation
def case_file(batches, caps):
    """tests/jpeg/jpeg_driver.cpp's input: caps[name] is each picture's output capacity."""
    out = [struct.pack("<2I", 0x3147504A, len(batches))]
    for b in batches:
        q, sub, restart = b[0].opts
        assert all(c.opts == b[0].opts for c in b)
        out.append(struct.pack("<8I", len(b), q, _lib.JPEG_SUBSAMPLINGS[sub], restart, SENTINEL, 0, 0, 0))
        for c in b:
            buf, pitch = jc.surface(c)
            h, w, _ = c.rgb.shape
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
    make_emu("jpeg-emu")
    return CSRC / "build" / "jpeg_emu" / "jpeg_driver"


def test_kernels_under_emulation_equal_model(emu_driver, tmp_path):
    """Every case, with 7 bytes of room behind the exact size: the scan and EOI equal the model's,
    the size is exact and the room keeps the sentinel."""
    scans = {n: jc.reference(n)[0][jc.reference(n)[1]:] for n in NAMES}
    caps = {n: len(s) + 7 for n, s in scans.items()}
    res = run_driver(emu_driver, tmp_path, jc.BATCHES, caps)
    for n in NAMES:
        size, buf = res[n]
        assert size == len(scans[n]), n
        assert buf[:size] == scans[n], n
        assert buf[size:] == bytes([SENTINEL]) * 7, n


def test_too_small_capacity_under_emulation(emu_driver, tmp_path):
    """Capacities of 0, 1, half the scan and one byte short, in exact-size heap blocks under ASan:
    the bytes that fit are the scan's first, and the size comes back with bit 63 set."""
    batches, caps, want = [], {}, {}
    base = jc.BY_NAME["mixed_0"]
    scan = jc.reference(base.name)[0][jc.reference(base.name)[1]:]
    for k, cap in enumerate((0, 1, len(scan) // 2, len(scan) - 1, len(scan))):
        c = jc.Case(f"cap_{k}", base.rgb, base.quality, base.sub, base.restart, base.pad, base.lead)
        batches.append([c])
        caps[c.name], want[c.name] = cap, cap
    res = run_driver(emu_driver, tmp_path, batches, caps)
    for n, cap in want.items():
        size, buf = res[n]
        assert size == len(scan) | (_lib.JPEG_TOO_SMALL if cap < len(scan) else 0), n
        assert buf == scan[:cap], n


# ---------------------------------------------------------------- what the cases reach
def test_case_list_reaches_every_path():
    st = {n: jc.reference(n)[2] for n in NAMES}
    cs = jc.CASES
    for sub in jc.SUBS:
        assert {(c.rgb.shape[1], c.rgb.shape[0]) for c in cs if c.sub == sub} >= set(jc.SIZES)
    assert {c.pad for c in cs} >= {0, 1, 13} and any(c.lead % 2 for c in cs)
    assert any((jc.surface(c)[1] * y + c.lead) % 4 for c in cs for y in range(c.rgb.shape[0]))  # rows off the dword grid
    assert {c.quality for c in cs} >= {1, 50, 75, 100}
    assert {c.restart for c in cs} >= {0, 1, 3}
    assert any(s["intervals"] > 8 for s in st.values())                      # RSTm wraps
    assert sorted(len(b) for b in jc.BATCHES)[-1] == 3 and any(len(b) == 1 for b in jc.BATCHES)
    assert len({c.rgb.shape for c in jc.BATCHES[0]}) == 3
    assert any(c.rgb.shape[1] > 128 for c in cs)                             # more than one group per MCU row
    assert st["zrl_run"]["zrl"] > 0
    assert st["last_coef"]["no_eob"] > 0
    assert st["flat"]["ac_zero"] > 0
    assert st["dc_cat11"]["dc_cat"] == 11
    assert st["ac_cat10"]["ac_cat"] == 10
    assert st["stuffing"]["stuffed"] > 0
    assert st["aligned_end"]["aligned"] > 0
