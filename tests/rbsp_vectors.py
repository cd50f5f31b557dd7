"""Hand-built inputs of k_rbsp and what tests/rbsp_ref.py makes of them.

Small batches in the product's own structs (SeqParams, PicDesc, the substream
table) as the case file tests/rbsp/rbsp_driver.cpp reads.  Payloads sit at
64-byte-aligned bits_off in an arena that ends in 128 bytes of padding, as
host/batch.cpp lays it out.  The product zero-fills the bytes between a payload
and the next one; here the case file carries the whole arena, so a case can
plant hostile bytes behind a payload (`pad`): the kernel reads the dword after a
payload's last 16-byte chunk and must not let it decide anything.  Where the
payload's length is a multiple of 64 the planted bytes take a 64-byte gap of
their own (in the product the next payload would start there).

Every output arena starts as the sentinel.  Expected: a launched picture's RBSP
bytes at rbsp[bits_off, bits_off + rbsp_len), its remapped words in rsubs, zeros
in its status word and its rows' counters; the sentinel everywhere else, except
rbsp[bits_off + rbsp_len, bits_off + round_up(bits_len, 16)), which the kernel's
16-byte store of an unchanged chunk may fill.
"""
import dataclasses
import functools
import struct

import numpy as np

import rbsp_ref as ref
from rbsp_ref import SUB_CONTINUE, SUB_OFFSET, SUB_SEG_END
from xform_vectors import PD_ASSEMBLY, PIC_DTYPE, SEQ_DTYPE, hash_str

SENTINEL = 0xAA
SENT32 = 0xAAAAAAAA
MAGIC = 0x31535052  # "RPS1"
PD_NMID_SHIFT = 16
OPT_CU, OPT_XPROG, OPT_XNTU, OPT_XJOB = 1, 2, 4, 8
OPT_ALL = 15
CONSTANTS = {"PD_ASSEMBLY": PD_ASSEMBLY, "PD_NMID_SHIFT": PD_NMID_SHIFT, "SUB_OFFSET": SUB_OFFSET,
             "SUB_CONTINUE": SUB_CONTINUE, "SUB_SEG_END": SUB_SEG_END}
MIRRORS = {"SeqParams": SEQ_DTYPE, "PicDesc": PIC_DTYPE}
# the reference's "real SPS" vector (src/hevc/rbsp_reader.rs, its unit tests)
REAL_SPS = bytes([0x01, 0x03, 0x70, 0x00, 0x00, 0x03, 0x00, 0xB0, 0x00, 0x00, 0x03, 0x00, 0x00, 0x03, 0x00, 0x5A, 0xA0,
                  0x04])


def layout_of_mirrors():
    """{name: value} in the form `rbsp_driver --layout` prints."""
    out = dict(CONSTANTS)
    for name, dt in MIRRORS.items():
        out[name] = dt.itemsize
        for f in dt.names:
            out[f"{name}.{f}"] = dt.fields[f][1]
    return out


def _rng(tag):
    return np.random.default_rng(hash_str(tag))


def filler(tag, n):
    """n bytes without a zero: a 03 among them is never removed"""
    return bytearray(_rng(tag).integers(1, 256, size=n, dtype=np.uint8).tobytes())


def planted(tag, n, at, follower=None):
    """filler with 00 00 03 so that the 03 is payload byte p for every p of `at`,
    and `follower` (if given) behind each"""
    b = filler(tag, n)
    for p in at:
        b[p - 2:p + 1] = b"\x00\x00\x03"
        if follower is not None and p + 1 < n:
            b[p + 1] = follower
    return bytes(b)


@dataclasses.dataclass
class Pic:
    name: str
    raw: bytes
    entries: tuple = None     # the words k_rbsp remaps: n_sub starts, the end entry, then the `nmid` segment starts
    nmid: int = 0
    tail: tuple = ()          # raw-only words behind them (WPP: counts per row): rsubs keeps the sentinel there
    pad: bytes = b""          # planted behind the payload
    flags: int = 0
    W: int = 16
    H: int = 16
    log2_ctb: int = 4

    def __post_init__(self):
        self.raw = bytes(self.raw)
        if self.entries is None:
            self.entries = (0, len(self.raw))
        self.n_sub = len(self.entries) - 1 - self.nmid
        assert self.n_sub >= 0
        self.rbsp, self.rentries = ref.remap(self.raw, self.entries)
        self.removed = ref.unescape(self.raw)[1]
        self.hctb = -(-self.H >> self.log2_ctb)


@dataclasses.dataclass
class Batch:
    name: str
    pics: list
    pic0: int = 0
    n_launch: int = None
    opt: int = OPT_ALL
    intra_stream: int = 1

    def __post_init__(self):
        if self.n_launch is None:
            self.n_launch = len(self.pics) - self.pic0
        self._build()

    def launched(self, i):
        return self.pic0 <= i < self.pic0 + self.n_launch

    def _build(self):
        pics = self.pics
        n = len(pics)
        seq_arr = np.zeros(n, dtype=SEQ_DTYPE)
        pic_arr = np.zeros(n, dtype=PIC_DTYPE)
        bits, subs = bytearray(), [0x12345678]  # a word in front that belongs to no picture
        rows = 1  # a guard row in front, one between pictures
        for i, p in enumerate(pics):
            a, pd = seq_arr[i], pic_arr[i]
            a["width"], a["height"], a["log2_ctb"], a["chroma_format"] = p.W, p.H, p.log2_ctb, 1
            a["bit_depth_y"] = a["bit_depth_c"] = 8
            a["out_w"], a["out_h"] = p.W, p.H
            pd["seq"], pd["flags"] = i, p.flags | (p.nmid << PD_NMID_SHIFT)
            pd["bits_off"], pd["bits_len"] = len(bits), len(p.raw)
            pd["sub_first"], pd["n_sub"] = len(subs), p.n_sub
            pd["row_off"] = rows
            rows += p.hctb + 1
            subs += list(p.entries) + list(p.tail) + [0x0BADBEEF]
            bits += p.raw + p.pad
            if p.pad and len(p.raw) % 64 == 0:
                assert len(p.pad) <= 64
            bits += bytes(-len(bits) % 64)
            if not p.raw:
                bits += bytes(64)  # (its own offset, so a stray write shows by picture)
        bits += bytes(128)
        self.bits, self.subs, self.total_rows = bytes(bits), np.array(subs, dtype=np.uint32), rows
        self.pic_arr = pic_arr
        head = struct.pack("<16I", n, n, self.pic0, self.n_launch, len(bits), len(subs), rows, self.opt,
                           self.intra_stream, SENTINEL, 0, 0, 0, 0, 0, 0)
        self.blob = b"".join([head, seq_arr.tobytes(), pic_arr.tobytes(), self.bits, self.subs.tobytes()])
        # ---- expected
        exp = np.full(len(bits), SENTINEL, dtype=np.uint8)
        free = np.zeros(len(bits), dtype=bool)
        rs = np.full(len(subs), SENT32, dtype=np.uint32)
        sizes = {"status": n, "row_counts": 2 * rows, "cu_counts": rows, "xprog": rows, "xntu": rows + n, "xjob": 1}
        words = {k: np.full(v, SENT32, dtype=np.uint32) for k, v in sizes.items()}
        for i, p in enumerate(pics):
            if not self.launched(i):
                continue
            off, ro = int(pic_arr[i]["bits_off"]), int(pic_arr[i]["row_off"])
            exp[off:off + len(p.rbsp)] = np.frombuffer(p.rbsp, dtype=np.uint8)
            free[off + len(p.rbsp):off + (len(p.raw) + 15) // 16 * 16] = True
            s0 = int(pic_arr[i]["sub_first"])
            rs[s0:s0 + len(p.rentries)] = p.rentries
            words["status"][i] = 0
            if self.opt & OPT_XJOB:
                words["xjob"][0] = 0
            if p.flags & PD_ASSEMBLY:
                continue
            words["row_counts"][2 * ro:2 * (ro + p.hctb)] = 0
            if self.opt & OPT_CU:
                words["cu_counts"][ro:ro + p.hctb] = 0
            if self.opt & OPT_XPROG:
                words["xprog"][ro:ro + p.hctb] = 0
            if self.opt & OPT_XNTU and self.intra_stream:
                words["xntu"][ro:ro + p.hctb] = 0
                words["xntu"][rows + i] = 0
        self.expected_rbsp, self.free, self.expected_rsubs, self.expected_words = exp, free, rs, words
        self.out_bytes = len(bits) + 4 * (len(subs) + sum(len(v) for v in words.values()))

    def failures(self, got):
        """Where the driver's buffers (one batch's part of the result file) differ from the model."""
        out, at = [], 0
        rbsp = got[at:at + len(self.bits)]
        at += len(self.bits)
        bad = (rbsp != self.expected_rbsp) & ~self.free
        for i, p in enumerate(self.pics):
            off, ln = int(self.pic_arr[i]["bits_off"]), (len(p.raw) + 63) // 64 * 64
            b = np.flatnonzero(bad[off:off + ln])
            bad[off:off + ln] = False
            if len(b):
                k = int(b[0])
                what = "RBSP byte" if self.launched(i) and k < len(p.rbsp) else "byte that must keep the sentinel"
                out.append(f"{self.name}/{p.name}: {len(b)} bytes differ, first a {what} at RBSP offset {k} of "
                           f"{len(p.rbsp)} (raw length {len(p.raw)}): got {int(rbsp[off + k]):#x}, expected "
                           f"{int(self.expected_rbsp[off + k]):#x}; removed bytes at {p.removed[:8]}")
        if bad.any():
            out.append(f"{self.name}: {int(bad.sum())} bytes outside every payload lost the sentinel, first at "
                       f"{int(np.flatnonzero(bad)[0])}")
        rs = got[at:at + 4 * len(self.subs)].view("<u4")
        at += 4 * len(self.subs)
        for k in np.flatnonzero(rs != self.expected_rsubs)[:8]:
            i = max(j for j in range(len(self.pics)) if int(self.pic_arr[j]["sub_first"]) <= k) \
                if k >= int(self.pic_arr[0]["sub_first"]) else 0
            out.append(f"{self.name}/{self.pics[i].name}: rsubs word {int(k) - int(self.pic_arr[i]['sub_first'])} "
                       f"(raw {int(self.subs[k]):#x}): got {int(rs[k]):#x}, expected {int(self.expected_rsubs[k]):#x}")
        for name, want in self.expected_words.items():
            w = got[at:at + 4 * len(want)].view("<u4")
            at += 4 * len(want)
            for k in np.flatnonzero(w != want)[:4]:
                out.append(f"{self.name}: {name}[{int(k)}]: got {int(w[k]):#x}, expected {int(want[k]):#x}")
        assert at == self.out_bytes
        return out


@dataclasses.dataclass
class Case:
    name: str
    batches: list

    @property
    def blob(self):
        return struct.pack("<II", MAGIC, len(self.batches)) + b"".join(b.blob for b in self.batches)

    def pics(self):
        """the launched pictures"""
        for b in self.batches:
            for i, p in enumerate(b.pics):
                if b.launched(i):
                    yield b, p

    def failures(self, got):
        out, at = [], 0
        want = sum(b.out_bytes for b in self.batches)
        if len(got) != want:
            return [f"{self.name}: result file of {len(got)} bytes, expected {want}"]
        for b in self.batches:
            out += b.failures(got[at:at + b.out_bytes])
            at += b.out_bytes
        return out


# ---------------------------------------------------------------- the cases
BOUNDARY_GROUPS = ((2, 14, 18, 1022, 1026, 2046, 2050), (15, 1023, 2047), (16, 1024, 2048), (17, 1025, 2049))
FOLLOWERS = (0, 1, 2, 3, 4, 0xff)


def case_boundaries():
    """The removable 03 at payload bytes 2, 14..18, 1022..1026, 2046..2050: the two zeros, the 03 and
    the byte behind it on every side of a lane boundary (16 bytes) and a step boundary (1 KiB), each
    with the followers 0..3 (removed) and 4, 0xff (kept).  Then what is no pattern."""
    pics = []
    for g, at in enumerate(BOUNDARY_GROUPS):
        for f in FOLLOWERS:
            pics.append(Pic(f"g{g}_f{f:02x}", planted(f"boundaries/{g}/{f}", 2100, at, f)))
    for name, head in (("00_01_03_00", b"\x00\x01\x03\x00"), ("01_00_03_00", b"\x01\x00\x03\x00"),
                       ("00_03_at_0", b"\x00\x03\x00\x00\x07"), ("03_at_0", b"\x03\x00\x00\x07"),
                       ("03_03_at_0", b"\x03\x03\x01"), ("00_03_03", b"\x00\x03\x03\x00")):
        b = filler(f"boundaries/{name}", 3100)
        # (the 03 at lane bytes 14, 15, 0, 1 and at the last and first byte of a step)
        spread = name[:5] in ("00_01", "01_00")
        for at in (0, 12, 29, 46, 63, 1020, 1037, 1054, 1071, 2045, 2062, 3070) if spread else (0,):
            b[at:at + len(head)] = head
        pics.append(Pic("not_" + name, b))
    return Case("boundaries", [Batch("boundaries", pics)])


END_LENGTHS = (1, 2, 3, 15, 16, 17, 1023, 1024, 1025)


def case_ends():
    """Payloads of 1 .. 1025 bytes.  `end03`: 00 00 03 as the last three bytes with 0xff behind
    them: only `pos + 1 == len` removes it.  `end00`: 00 00 as the last two with 03 00 behind
    them: nothing is removed.  `end04`: 00 00 03 and one more payload byte 04: kept.  The bytes
    behind a payload are planted here; the product zero-fills them."""
    pics = []
    for n in END_LENGTHS:
        body = filler(f"ends/{n}", n)
        if n >= 3:
            pics.append(Pic(f"end03_{n}", body[:n - 3] + b"\x00\x00\x03", pad=b"\xff" * 8))
        else:
            pics.append(Pic(f"end03_{n}", (b"\x00\x03" if n == 2 else b"\x03"), pad=b"\xff" * 8))
        pics.append(Pic(f"end03z_{n}", pics[-1].raw, pad=b"\x00" * 8))
        if n >= 2:
            pics.append(Pic(f"end00_{n}", body[:n - 2] + b"\x00\x00", pad=b"\x03\x00\x00\x03\x00\x00\x03\x00"))
        if n >= 4:
            pics.append(Pic(f"end04_{n}", body[:n - 4] + b"\x00\x00\x03\x04", pad=b"\x00\x00\x03\x00"))
    return Case("ends", [Batch("ends", pics)])


def case_runs():
    r0 = _rng("runs/03").integers(0, 2, size=3000, dtype=np.uint8) * 3
    r1 = _rng("runs/01234").integers(0, 5, size=3000, dtype=np.uint8)
    pics = [Pic("000003_x400", b"\x00\x00\x03" * 400), Pic("00_00_00_03_01", b"\x00\x00\x00\x03\x01"),
            Pic("00_00_03_03_03", b"\x00\x00\x03\x03\x03"), Pic("real_sps", REAL_SPS),
            Pic("random_0_3", r0.tobytes()), Pic("random_0_to_4", r1.tobytes())]
    return Case("runs", [Batch("runs", pics)])


def case_paths():
    """3 KiB payloads.  `late`: the only removed byte is in the last step: unchanged chunks go out
    by the 16-byte store, then the rest byte by byte.  `early`: it is byte 2, so every later chunk
    goes byte by byte, shifted by one.  `none`: 16-byte stores only (some chunks hold a 03)."""
    pics = [Pic("late", planted("paths/late", 3072, (2500,), 0)), Pic("early", planted("paths/early", 3072, (2,), 1)),
            Pic("none", filler("paths/none", 3072))]
    return Case("paths", [Batch("paths", pics)])


def case_entries():
    """Entry points.  An entry at or past the payload's end (a corrupt header) is in bounds by
    construction: the kernel compares it with bits_len before it selects a lane with it and
    writes the RBSP length in its place."""
    at = (40, 47, 300, 1024, 1030, 2047, 2100)
    raw = planted("entries/a", 2200, at, 0)
    n = len(raw)
    ents = [0, 41, 38, 40, 48, 45, 1025, 1022, 2048, 2045, 2101 | SUB_SEG_END, 301 | SUB_CONTINUE,
            39 | SUB_CONTINUE | SUB_SEG_END, 1023 | SUB_SEG_END, n - 1, n | SUB_CONTINUE, n + 5,
            SUB_OFFSET | SUB_SEG_END, n]
    a = Pic("kinds", raw, tuple(ents))
    dense = (_rng("entries/dense").integers(0, 2, size=3000, dtype=np.uint8) * 3).tobytes()
    many = tuple(int(v) for v in np.linspace(0, 2999, 129).astype(int)) + (3000,)
    b = Pic("130_entries", dense, many)
    raw_c = planted("entries/c", 1500, (10, 500, 1100, 1400), 2)
    c = Pic("nmid3", raw_c, (0, 501 | SUB_SEG_END, 1101, 1300 | SUB_CONTINUE, 1500, 11, 1401, 1499), nmid=3,
            tail=(0, 1, 2, 3))
    return Case("entries", [Batch("entries", [a, b, c])])


def _batch_pics(tag):
    dense = lambda t, n: _rng(f"{tag}/{t}").integers(0, 4, size=n, dtype=np.uint8).tobytes()
    return [Pic("before", dense("before", 700), W=64, H=40, log2_ctb=4),
            Pic("a", dense("a", 1100), (0, 400, 800, 1100), W=64, H=40, log2_ctb=4),
            Pic("b", planted(f"{tag}/b", 2500, (5, 1500), 3), W=96, H=72, log2_ctb=5),
            Pic("assembly", b"", (0,), flags=PD_ASSEMBLY, W=96, H=72, log2_ctb=5),
            Pic("c", dense("c", 333), W=128, H=100, log2_ctb=6),
            Pic("after", dense("after", 900), W=64, H=24, log2_ctb=4)]


def case_batch():
    """pic0 = 1 with a picture before and one after the launched range; an assembly picture
    (bits_len 0, one entry); heights that are no multiple of the CTB size, three CTB sizes."""
    return Case("batch", [Batch("batch", _batch_pics("batch"), pic0=1, n_launch=4)])


def case_zeroing():
    """zero_outputs with every optional pointer set and with every one null, intra_stream on and off."""
    bs = [Batch(f"opt{opt}_stream{st}", _batch_pics("zeroing"), pic0=1, n_launch=4, opt=opt, intra_stream=st)
          for opt in (OPT_ALL, 0) for st in (1, 0)]
    return Case("zeroing", bs)


CASES = {"boundaries": case_boundaries, "ends": case_ends, "runs": case_runs, "paths": case_paths,
         "entries": case_entries, "batch": case_batch, "zeroing": case_zeroing}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()
