"""The PNG encoder of heif_amd/csrc/kernels/png.hpp as a plain Python / numpy model, written
from that header's prose (THE FILE, SAMPLES, FILTERING, DEFLATE, CODE LENGTHS, IDAT).  It shares
no code with the library: the host restatement, the kernels under emulation and the kernels on
the GPU are each compared with its bytes.  zlib is used for the two checksums only."""
import struct
import zlib

import numpy as np

BLOCK = 32768
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FORMATS = {"rgb8": (3, False), "rgba8": (4, False), "rgb16": (3, True), "rgba16": (4, True)}
ADAPTIVE = 5


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def raw_rows(px: np.ndarray, fmt: str, bits: int) -> np.ndarray:
    """(h, w * bpp) uint8: the raw rows of an (h, w, C) picture (SAMPLES)."""
    ch, wide = FORMATS[fmt]
    h, w, c = px.shape
    assert c == ch
    if not wide:
        return np.ascontiguousarray(px, dtype=np.uint8).reshape(h, w * ch)
    s = px.astype(np.uint32) & ((1 << bits) - 1)
    v = (s << (16 - bits)) | (s >> (2 * bits - 16))
    out = np.empty((h, w, ch, 2), np.uint8)
    out[..., 0] = v >> 8
    out[..., 1] = v & 255
    return out.reshape(h, w * ch * 2)


def filter_rows(raw: np.ndarray, bpp: int, choice: int):
    """The filtered stream (bytes), the type of every row and the rows whose least sum two
    types share (FILTERING)."""
    h, n = raw.shape
    out = np.empty((h, n + 1), np.uint8)
    types, ties = [], []
    zero = np.zeros(n, np.int32)
    for y in range(h):
        x = raw[y].astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        b = raw[y - 1].astype(np.int32) if y else zero
        c = (np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if n > bpp else np.zeros(n, np.int32)) if y else zero
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        cand = [x & 255, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth) & 255]
        if choice == ADAPTIVE:
            sums = [int(np.minimum(f, 256 - f).sum()) for f in cand]
            t = sums.index(min(sums))  # the lowest type wins a tie
            if sums.count(min(sums)) > 1:
                ties.append(y)
        else:
            t = choice
        types.append(t)
        out[y, 0] = t
        out[y, 1:] = cand[t]
    return out.tobytes(), types, ties


def code_lengths(counts, limit: int):
    """CODE LENGTHS, steps 1 to 3.  Returns (lengths, whether step 2 had to repair)."""
    used = [s for s, c in enumerate(counts) if c]
    assert len(used) >= 2
    leaves = sorted(used, key=lambda s: counts[s])
    # step 1: two queues; a node is (weight, [leaf depths below it])
    q1 = [(counts[s], [0]) for s in leaves]
    q2 = []
    i1 = i2 = 0

    def take():
        nonlocal i1, i2
        if i1 < len(q1) and (i2 >= len(q2) or q1[i1][0] <= q2[i2][0]):
            i1 += 1
            return q1[i1 - 1]
        i2 += 1
        return q2[i2 - 1]

    for _ in range(len(used) - 1):
        a, b = take(), take()
        q2.append((a[0] + b[0], [d + 1 for d in a[1] + b[1]]))
    depths = q2[-1][1]
    n = [0] * (limit + 1)
    for d in depths:
        n[min(d, limit)] += 1
    # step 2
    k = sum(n[l] << (limit - l) for l in range(1, limit + 1))
    repaired = k > 1 << limit
    while k > 1 << limit:
        n[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if n[l]:
                n[l] -= 1
                n[l + 1] += 2
                break
        k -= 1
    # step 3
    by_count = sorted(used, key=lambda s: (-counts[s], s))
    lengths = [0] * len(counts)
    at = 0
    for l in range(1, limit + 1):
        for _ in range(n[l]):
            lengths[by_count[at]] = l
            at += 1
    return lengths, repaired


def canonical(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)}."""
    top = max(lengths)
    count = [0] * (top + 2)
    for l in lengths:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (top + 2)
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


class Bits:
    """Bits into bytes, least significant first."""

    def __init__(self):
        self.done = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v: int, length: int):
        self.acc |= v << self.n
        self.n += length
        if self.n >= 64:  # whole bytes leave the accumulator
            self.done += (self.acc & (2 ** 64 - 1)).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def huff(self, code_len):
        code, length = code_len
        for i in range(length - 1, -1, -1):  # most significant bit first
            self.put(code >> i & 1, 1)

    def bytes(self) -> bytes:
        self.n = (self.n + 7) // 8 * 8
        return bytes(self.done) + self.acc.to_bytes(self.n // 8, "little")


def deflate_block(piece: bytes, final: bool, facts=None) -> bytes:
    counts = np.bincount(np.frombuffer(piece, np.uint8), minlength=257).tolist()
    counts[256] = 1
    lit, rep15 = code_lengths(counts, 15)
    sent = lit + [1]  # the one distance code
    clcount = [0] * 19
    for l in sent:
        clcount[l] += 1
    cl, rep7 = code_lengths(clcount, 7)
    nsent = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
    lit_code, cl_code = canonical(lit), canonical(cl)
    b = Bits()
    b.put(0, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(nsent - 4, 4)
    for s in CL_ORDER[:nsent]:
        b.put(cl[s], 3)
    for l in sent:
        b.huff(cl_code[l])
    # the codes of the bytes, through a table of (reversed code, length) for speed
    rev = {s: (int(format(c, "0%db" % l)[::-1], 2), l) for s, (c, l) in lit_code.items()}
    for d in piece:
        v, l = rev[d]
        b.put(v, l)
    b.put(*rev[256])
    b.put(1 if final else 0, 1), b.put(0, 2)
    if facts is not None:
        facts.append({"repair15": rep15, "repair7": rep7, "distinct": len(set(piece)), "lit": lit})
    return b.bytes() + b"\x00\x00\xff\xff"


def header(w: int, h: int, fmt: str, bits: int, srgb=False, cicp=None, icc=None) -> bytes:
    ch, wide = FORMATS[fmt]
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16 if wide else 8, 6 if ch == 4 else 2, 0, 0, 0))
    if wide and bits < 16:
        out += chunk(b"sBIT", bytes([bits] * ch))
    if srgb:
        out += chunk(b"sRGB", b"\0")
    elif cicp is not None:
        out += chunk(b"cICP", bytes(cicp))
    elif icc is not None:
        z = b"\x78\x01"
        for at in range(0, len(icc), 65535):
            part = icc[at:at + 65535]
            z += bytes([1 if at + len(part) == len(icc) else 0]) + struct.pack("<HH", len(part), len(part) ^ 0xffff) + part
        z += struct.pack(">I", zlib.adler32(icc))
        out += chunk(b"iCCP", b"ICC profile\0\0" + z)
    return out


def body(px: np.ndarray, fmt: str, bits: int = 8, filt: int = ADAPTIVE, facts=None) -> bytes:
    """The IDAT chunks and IEND (what heifgpu_png_encode_batch writes)."""
    ch, wide = FORMATS[fmt]
    stream, types, ties = filter_rows(raw_rows(px, fmt, bits), ch * (2 if wide else 1), filt)
    blocks = []
    pieces = [stream[i:i + BLOCK] for i in range(0, len(stream), BLOCK)]
    out = b""
    for k, piece in enumerate(pieces):
        last = k + 1 == len(pieces)
        blocks_facts = [] if facts is not None else None
        data = (b"\x78\x01" if k == 0 else b"") + deflate_block(piece, last, blocks_facts)
        if last:
            data += struct.pack(">I", zlib.adler32(stream))
        out += chunk(b"IDAT", data)
        if facts is not None:
            blocks.append(blocks_facts[0])
    if facts is not None:
        facts.append({"types": types, "ties": ties, "blocks": blocks, "stream": stream})
    return out + chunk(b"IEND", b"")


def encode(px: np.ndarray, fmt: str, bits: int = 8, filt: int = ADAPTIVE, srgb=False, cicp=None, icc=None, facts=None) -> bytes:
    h, w, _ = px.shape
    return header(w, h, fmt, bits, srgb, cicp, icc) + body(px, fmt, bits, filt, facts)
