"""Hand-built inputs of k_transform and an integer model of what it must compute.

Three parts, none of which reads anything from the kernels' sources:

* the reference: H.265 8.6.2 (residual), 8.6.3 (scaling) and 8.6.4.2 (the two
  matrix stages) restated on Python / numpy int64 integers, with full n x n
  products, no extent or DC shortcut, the matrices built from the spec's
  transMatrix and DST-VII tables;
* the encoder: a TB's levels written as the product's TuRec, sub-block records
  (SbRec words), escape list and PCM words, as common/desc.hpp describes them,
  with the 4x4 scans of 6.5.3-6.5.5;
* the cases: pictures of non-overlapping TBs grouped by what they stress, laid
  out as the case file tests/xform/xform_driver.cpp reads, together with the
  expected residual arena (the sentinel wherever no coded TB lies).
"""
import dataclasses
import functools
import struct

import numpy as np

SENTINEL = -21846  # 0xaaaa
MAGIC = 0x31434658

# ---------------------------------------------------------------- layout mirrors
_I, _U = "<i4", "<u4"
SEQ_DTYPE = np.dtype(
    [(k, _I) for k in ("width", "height", "log2_ctb", "log2_min_cb", "log2_min_tb", "log2_max_tb",
                       "max_th_depth_intra", "chroma_format", "bit_depth_y", "bit_depth_c")]
    + [("flags", _U)]
    + [(k, _I) for k in ("diff_cu_qp_delta_depth", "cb_qp_offset", "cr_qp_offset", "log2_min_pcm", "log2_max_pcm",
                         "pcm_bd_y", "pcm_bd_c", "conf_l", "conf_t", "out_w", "out_h")]
    + [("sf_off", _U), ("pad", _I, (3,))], align=True)
PIC_DTYPE = np.dtype(
    [("bits_off", "<u8"), ("bits_len", _U), ("sub_first", _U), ("n_sub", _U), ("seq", _U)]
    + [(k, _I) for k in ("slice_qp", "cb_qp_off", "cr_qp_off", "sao_luma", "sao_chroma", "dbk_disabled", "beta_off",
                         "tc_off")]
    + [("image", _U), ("out_x", _I), ("out_y", _I)]
    + [(k, "<u8") for k in ("recon_off", "resid_off", "map_off", "sao_off", "tu_off", "coef_off")]
    + [("row_off", _U), ("tu_cap_row", _U), ("coef_cap_row", _U), ("flags", _U), ("org_x", _I), ("org_y", _I),
       ("child0", _U), ("nchild", _U)], align=True)
TU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("log2", "u1"), ("flags", "u1"), ("mode", "u1"), ("qp", "u1"),
                     ("coef", _U), ("ncoef", "<u2"), ("ctu", "<u2")], align=True)
MIRRORS = {"SeqParams": SEQ_DTYPE, "PicDesc": PIC_DTYPE, "TuRec": TU_DTYPE}

# the constants of common/desc.hpp the cases use (the layout test compares them too)
SP_SCALING_LIST = 1
PD_ASSEMBLY = 2
TU_CIDX_MASK, TU_CBF, TU_TSKIP, TU_BYPASS, TU_DST, TU_PCM = 3, 4, 8, 16, 32, 64
SF_SIZE_OFFSET = (0, 6 * 16, 6 * (16 + 64), 6 * (16 + 64 + 256))
SF_BLOCK_BYTES = 6 * (16 + 64 + 256 + 1024)
CONSTANTS = {"SP_SCALING_LIST": SP_SCALING_LIST, "PD_ASSEMBLY": PD_ASSEMBLY, "TU_CIDX_MASK": TU_CIDX_MASK,
             "TU_CBF": TU_CBF, "TU_TSKIP": TU_TSKIP, "TU_BYPASS": TU_BYPASS, "TU_DST": TU_DST, "TU_PCM": TU_PCM,
             "kSfBlockBytes": SF_BLOCK_BYTES, "Coef": 4,
             **{f"sf_size_offset.{i}": v for i, v in enumerate(SF_SIZE_OFFSET)}}


def layout_of_mirrors():
    """{name: value} in the form `xform_driver --layout` prints."""
    out = dict(CONSTANTS)
    for name, dt in MIRRORS.items():
        out[name] = dt.itemsize
        for f in dt.names:
            out[f"{name}.{f}"] = dt.fields[f][1]
    return out


# ---------------------------------------------------------------- the reference
# 8.6.4.2: column 0 of transMatrix, transMatrix[k][0] = c(k); every other entry is
# c((2 n + 1) k) continued by the cosine's symmetries, c(j) ~ 64 sqrt(2) cos(j pi / 64)
_COL0 = (64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67,
         64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4)


def _c(j):
    j %= 128
    if j > 64:
        j = 128 - j  # cos(2 pi - a) = cos a
    assert j not in (32, 64)  # (2 n + 1) k never is an odd multiple of 32
    return -_COL0[64 - j] if j > 32 else _COL0[j]  # cos(pi - a) = -cos a


TRANS_MATRIX = np.array([[_c((2 * n + 1) * k) for n in range(32)] for k in range(32)], dtype=np.int64)
DST_MATRIX = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], dtype=np.int64)
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)


def matrix_of(n, dst=False):
    """M[j][i] of the one-dimensional transform y[i] = sum_j M[j][i] x[j] (8.6.4.2)."""
    return DST_MATRIX if dst else TRANS_MATRIX[:: 32 // n, :n]


def clip16(a):
    return np.clip(a, -32768, 32767)


def scale(levels, n, bd, qp, m):
    """8.6.3: d[y][x]; m is the n x n ScalingFactor (or 16)."""
    bd_shift = bd + n.bit_length() - 1 - 5
    v = levels.astype(np.int64) * m * LEVEL_SCALE[qp % 6] * (1 << (qp // 6))
    return clip16((v + (1 << (bd_shift - 1))) >> bd_shift)


def reference(levels, n, bd, qp, m=None, ts=False, bypass=False, dst=False):
    """Residual r[y][x] of a TB with TransCoeffLevel levels[y][x], unclipped, and
    the intermediates {d, e}: e is the first stage before its shift and clip."""
    levels = np.asarray(levels, dtype=np.int64)
    if bypass:
        return levels.copy(), {}
    log2n = n.bit_length() - 1
    mm = 16 if (m is None or (ts and n > 4)) else np.asarray(m, dtype=np.int64)
    d = scale(levels, n, bd, qp, mm)
    if ts:
        r, mid = d * (1 << (5 + log2n)), {"d": d}
    else:
        M = matrix_of(n, dst)
        e = M.T @ d             # columns: e[i][x] = sum_j M[j][i] d[j][x]
        g = clip16((e + 64) >> 7)
        r = g @ M               # rows: r[y][i] = sum_j M[j][i] g[y][j]
        mid = {"d": d, "e": e}
    bd2 = 20 - bd
    return (r + (1 << (bd2 - 1))) >> bd2, mid


# ---------------------------------------------------------------- scans (6.5.3-6.5.5)
def scan_order(blk, scan_idx):
    """[(x, y)] by scan position: 0 up-right diagonal, 1 horizontal, 2 vertical."""
    if scan_idx == 1:
        return [(x, y) for y in range(blk) for x in range(blk)]
    if scan_idx == 2:
        return [(x, y) for x in range(blk) for y in range(blk)]
    out, x, y = [], 0, 0
    while len(out) < blk * blk:
        while y >= 0:
            if x < blk and y < blk:
                out.append((x, y))
            y -= 1
            x += 1
        y, x = x, 0
    return out


# ---------------------------------------------------------------- the encoder
class RowSpace:
    """One CTB row's coefficient words: records and PCM words from the front,
    the escape list down from the end."""

    def __init__(self, cap):
        assert cap % 4 == 0
        self.words = np.zeros(cap, dtype=np.uint32)
        self.front, self.back = 0, cap

    def take(self, n):
        self.front = (self.front + 3) & ~3  # records are read as 16-byte loads
        at = self.front
        self.front += n
        assert self.front <= self.back, "row coefficient space exhausted"
        return at

    def escape(self, value):
        self.back -= 1
        assert self.front <= self.back, "row coefficient space exhausted"
        self.words[self.back] = value
        return self.back


def encode_records(levels, n, scan_idx, hide, row):
    """The TB's sub-block records into `row`; returns (coef, ncoef, levels as a
    decoder reads them).  With `hide`, a sub-block whose first and last
    significant scan positions lie more than 3 apart (9.3.4.3's condition)
    leaves out the sign of its lowest one, which is then the parity of the
    sub-block's sum of absolute levels: the returned levels carry that sign."""
    levels = np.array(levels, dtype=np.int64)
    assert levels.shape == (n, n) and levels.min() >= -32768 and levels.max() <= 32767
    pos4 = scan_order(4, scan_idx)
    recs = []
    for xs, ys in reversed(scan_order(n // 4, scan_idx)):  # decoding order
        vals = [int(levels[4 * ys + py, 4 * xs + px]) for px, py in pos4]
        sig = [k for k in range(16) if vals[k]]
        if not sig:
            continue
        hidden = bool(hide) and sig[-1] - sig[0] > 3
        if hidden:
            k0 = sig[0]
            odd = sum(abs(v) for v in vals) & 1
            assert abs(vals[k0]) <= 32767
            vals[k0] = -abs(vals[k0]) if odd else abs(vals[k0])
            px, py = pos4[k0]
            levels[4 * ys + py, 4 * xs + px] = vals[k0]
        w0, nib, rank, esc0 = sum(1 << k for k in sig), 0, 0, None
        for k in reversed(sig):
            a = abs(vals[k])
            if not (hidden and k == sig[0]):
                if vals[k] < 0:
                    w0 |= 1 << (31 - rank)
            rank += 1
            nib |= min(a - 1, 15) << (4 * k)
            if a >= 16:
                at = row.escape(a)
                esc0 = at if esc0 is None else esc0
        w3 = xs | ys << 3 | scan_idx << 6 | int(hidden) << 8 | (esc0 if esc0 is not None else row.back - 1) << 9
        recs.append((w0, nib & 0xffffffff, nib >> 32, w3))
    at = row.take(4 * len(recs))
    row.words[at:at + 4 * len(recs)] = np.array(recs, dtype=np.uint32).reshape(-1)
    return at, 4 * len(recs), levels


def encode_pcm(levels, n, row):
    """One word per sample: value << 16 | raster position (last sample first: the
    position is the word's own, not its index)."""
    levels = np.asarray(levels, dtype=np.int64)
    at = row.take(n * n)
    row.words[at:at + n * n] = (((levels.reshape(-1) & 0xffff) << 16) | np.arange(n * n))[::-1]
    return at, n * n, levels


# ---------------------------------------------------------------- case description
@dataclasses.dataclass
class TB:
    name: str
    n: int
    cidx: int
    qp: int
    levels: np.ndarray
    ts: bool = False
    bypass: bool = False
    dst: bool = False
    pcm: bool = False
    scan_idx: int = 0
    hide: bool = False
    coded: bool = True
    row: int = 0
    x: int = None
    y: int = None
    outside: bool = False  # lies partly outside its plane: the kernel must leave it alone


@dataclasses.dataclass
class Seq:
    width: int
    height: int
    log2_ctb: int
    chroma_format: int
    bd_y: int
    bd_c: int
    sf: np.ndarray = None  # SF_BLOCK_BYTES of ScalingFactor, or None (flat 16)

    def plane(self, cidx):
        if cidx == 0:
            return self.width, self.height
        assert self.chroma_format
        return (self.width >> (self.chroma_format in (1, 2)), self.height >> (self.chroma_format == 1))

    @property
    def rows(self):
        return -(-self.height >> self.log2_ctb)


@dataclasses.dataclass
class Pic:
    seq: int
    tbs: list
    flags: int = 0
    launched: bool = True


def ramp_sf(salt=0):
    """A ScalingFactor block with its own factor (1..255) at every position, size
    and matrix, and no symmetry between x and y."""
    out = np.zeros(SF_BLOCK_BYTES, dtype=np.uint8)
    for size_id in range(4):
        n = 4 << size_id
        y, x = np.mgrid[0:n, 0:n]
        for mid in range(6):
            at = SF_SIZE_OFFSET[size_id] + mid * n * n
            out[at:at + n * n] = ((13 * x + 29 * y + 57 * size_id + 101 * mid + salt) % 255 + 1).reshape(-1)
    return out


def const_sf(m):
    return np.full(SF_BLOCK_BYTES, m, dtype=np.uint8)


def sf_matrix(sf, n, cidx):
    at = SF_SIZE_OFFSET[n.bit_length() - 3] + cidx * n * n
    return sf[at:at + n * n].reshape(n, n).astype(np.int64)


BOUNDARY_D = (-32768, -32767, -257, -256, -129, -128, -1, 0, 127, 128, 255, 256, 32767)


class Case:
    """A case file and what the transform must make of it."""

    def __init__(self, name, seqs, pics, pic0=0):
        self.name, self.seqs, self.pics, self.pic0 = name, seqs, pics, pic0
        self.regions = []      # (tb name, arena offset of the TB's first sample, pitch, n), coded TBs
        self.d_seen = {}       # n -> set of boundary values among the scaled d
        self.clip_hi, self.clip_lo = set(), set()  # n whose first stage clips at +32767 / -32768
        self.rows_tus = []     # (pic, row, the row's TU records as a TU_DTYPE array)
        self._build()

    def _build(self):
        seqs, pics = self.seqs, self.pics
        max_rows = max(seqs[p.seq].rows for p in pics[self.pic0:])
        sf_blocks, sf_off = [np.zeros(64, np.uint8)], 64  # (a block never starts the arena)
        seq_arr = np.zeros(len(seqs), dtype=SEQ_DTYPE)
        for i, s in enumerate(seqs):
            a = seq_arr[i]
            a["width"], a["height"], a["log2_ctb"], a["chroma_format"] = s.width, s.height, s.log2_ctb, s.chroma_format
            a["bit_depth_y"], a["bit_depth_c"] = s.bd_y, s.bd_c
            a["log2_min_cb"], a["log2_min_tb"], a["log2_max_tb"] = 3, 2, 5
            a["out_w"], a["out_h"] = s.width, s.height
            a["flags"] = SP_SCALING_LIST if s.sf is not None else 0
            a["sf_off"] = sf_off
            blk = s.sf if s.sf is not None else np.full(SF_BLOCK_BYTES, 0xee, np.uint8)  # (never to be read)
            sf_blocks.append(blk)
            sf_off += SF_BLOCK_BYTES
        pic_arr = np.zeros(len(pics), dtype=PIC_DTYPE)
        row_words, tus_all, coefs_all = [7, 7], [np.zeros(3, dtype=TU_DTYPE)], [np.zeros(8, dtype=np.uint32)]
        n_tus, n_coefs, resid_at = 3, 8, 40
        expected = []
        for pi, p in enumerate(pics):
            s = seqs[p.seq]
            live = p.launched and pi >= self.pic0 and not (p.flags & PD_ASSEMBLY)
            rows = s.rows
            by_row = [[t for t in p.tbs if t.row == r] for r in range(rows)]
            assert sum(len(b) for b in by_row) == len(p.tbs)
            tu_cap = max(len(b) for b in by_row) + 2
            need = max(sum((t.n * t.n if t.pcm else t.n * t.n // 4 + int(np.count_nonzero(np.abs(t.levels) >= 16))) + 4
                           for t in b) for b in by_row)
            coef_cap = (need + 16 + 3) & ~3
            planes = [s.plane(0)] + ([s.plane(1)] * 2 if s.chroma_format else [])
            plane_off = np.cumsum([0] + [w * h for w, h in planes])
            occ = [np.zeros((h // 4, w // 4), dtype=bool) for w, h in planes]
            for w, h in planes:
                assert w % 4 == 0 and h % 4 == 0
            arena = np.full(int(plane_off[-1]), SENTINEL, dtype=np.int64)
            pd = pic_arr[pi]
            pd["seq"], pd["flags"], pd["resid_off"] = p.seq, p.flags, resid_at
            pd["tu_off"], pd["coef_off"], pd["row_off"] = n_tus, n_coefs, len(row_words) // 2
            pd["tu_cap_row"], pd["coef_cap_row"] = tu_cap, coef_cap
            for t in sorted(p.tbs, key=lambda t: t.x is None):  # (stable: the given positions first)
                self._place(t, s, occ)
            for r, tbs in enumerate(by_row):
                space = RowSpace(coef_cap)
                recs = np.zeros(tu_cap, dtype=TU_DTYPE)
                for k, t in enumerate(tbs):
                    bd = s.bd_c if t.cidx else s.bd_y
                    if t.pcm:
                        assert t.bypass
                        coef, ncoef, lv = encode_pcm(t.levels, t.n, space)
                    else:
                        coef, ncoef, lv = encode_records(t.levels, t.n, t.scan_idx, t.hide, space)
                    rec = recs[k]
                    rec["x"], rec["y"], rec["log2"], rec["qp"] = t.x, t.y, t.n.bit_length() - 1, t.qp
                    rec["flags"] = t.cidx | sum(f for f, on in ((TU_CBF, t.coded), (TU_TSKIP, t.ts), (TU_BYPASS, t.bypass),
                                                                (TU_DST, t.dst), (TU_PCM, t.pcm)) if on)
                    rec["mode"], rec["ctu"] = (k * 7) % 35, t.x >> s.log2_ctb
                    rec["coef"], rec["ncoef"] = coef, ncoef
                    if not (live and t.coded and not t.outside):
                        continue
                    m = sf_matrix(s.sf, t.n, t.cidx) if s.sf is not None else None
                    res, mid = reference(lv, t.n, bd, t.qp, m, ts=t.ts, bypass=t.bypass, dst=t.dst)
                    pw = planes[t.cidx][0]
                    at = int(plane_off[t.cidx]) + t.y * pw + t.x
                    view = arena[int(plane_off[t.cidx]):int(plane_off[t.cidx + 1])].reshape(planes[t.cidx][1], pw)
                    view[t.y:t.y + t.n, t.x:t.x + t.n] = clip16(res)
                    self.regions.append((t.name, resid_at + at, pw, t.n))
                    if "d" in mid:
                        self.d_seen.setdefault(t.n, set()).update(set(BOUNDARY_D) & set(mid["d"].reshape(-1).tolist()))
                    if "e" in mid:
                        e = (mid["e"] + 64) >> 7
                        if e.max() > 32767:
                            self.clip_hi.add(t.n)
                        if e.min() < -32768:
                            self.clip_lo.add(t.n)
                assert space.front <= space.back
                row_words += [len(tbs), space.front]
                tus_all.append(recs)
                coefs_all.append(space.words)
                self.rows_tus.append((pi, r, recs[:len(tbs)]))
            n_tus += rows * tu_cap
            n_coefs += rows * coef_cap
            expected += [np.full(resid_at - sum(len(e) for e in expected), SENTINEL, dtype=np.int64), arena]
            resid_at += len(arena) + 24
        expected.append(np.full(24, SENTINEL, dtype=np.int64))
        self.expected = np.concatenate(expected).astype(np.int16)
        rows_arr = np.array(row_words + [9, 9], dtype=np.uint32)
        tus = np.concatenate(tus_all)
        coefs = np.concatenate(coefs_all)
        sf = np.concatenate(sf_blocks)
        assert len(tus) == n_tus and len(coefs) == n_coefs and len(sf) == sf_off
        head = struct.pack("<16I", MAGIC, len(seqs), len(pics), self.pic0, len(pics) - self.pic0, max_rows,
                           len(rows_arr), n_tus, n_coefs, len(sf), len(self.expected), SENTINEL & 0xffff, 0, 0, 0, 0)
        self.blob = b"".join([head, seq_arr.tobytes(), pic_arr.tobytes(), rows_arr.tobytes(), tus.tobytes(),
                              coefs.tobytes(), sf.tobytes()])

    @staticmethod
    def _place(t, s, occ):
        """(x, y) for the TB: given, or the first free aligned slot of its plane.
        Coded TBs never overlap (the waves write concurrently)."""
        w, h = s.plane(t.cidx)
        if t.outside or not t.coded:
            if t.x is None:
                t.x, t.y = 0, 0
            return
        o, q = occ[t.cidx], t.n // 4
        if t.x is None:
            for y in range(0, h - t.n + 1, t.n):
                for x in range(0, w - t.n + 1, t.n):
                    if not o[y // 4:y // 4 + q, x // 4:x // 4 + q].any():
                        t.x, t.y = x, y
                        break
                if t.x is not None:
                    break
            assert t.x is not None, f"no room for {t.name}"
        assert t.x % 4 == 0 and t.y % 4 == 0 and t.x + t.n <= w and t.y + t.n <= h, t.name
        assert not o[t.y // 4:t.y // 4 + q, t.x // 4:t.x // 4 + q].any(), f"{t.name} overlaps"
        o[t.y // 4:t.y // 4 + q, t.x // 4:t.x // 4 + q] = True

    def failures(self, got):
        """Names of the TBs whose residual differs, in record order, then a note
        on every sample outside the coded TBs that lost the sentinel."""
        got = np.asarray(got, dtype=np.int16)
        assert got.shape == self.expected.shape
        bad = got != self.expected
        out = []
        if not bad.any():
            return out
        rest = bad.copy()
        for name, at, pitch, n in self.regions:
            idx = at + (np.arange(n)[:, None] * pitch + np.arange(n)[None, :])
            if bad[idx].any():
                yx = np.argwhere(bad[idx])[0]
                out.append(f"{name}: {int(bad[idx].sum())} of {n * n} samples differ, first at (y={yx[0]}, x={yx[1]}): "
                           f"got {got[idx][yx[0], yx[1]]}, expected {self.expected[idx][yx[0], yx[1]]}")
            rest[idx] = False
        if rest.any():
            where = np.flatnonzero(rest)
            out.append(f"{len(where)} samples outside the coded TBs changed, first at arena index {where[0]} "
                       f"(now {got[where[0]]})")
        return out


# ---------------------------------------------------------------- the vector groups
def _rng(tag):
    return np.random.default_rng(abs(hash_str(tag)))


def hash_str(s):
    h = 2166136261
    for ch in s.encode():
        h = ((h ^ ch) * 16777619) & 0xffffffff
    return h


def _full_range(rng, n):
    """Half uniform over the 16 bits, half log-uniform magnitudes."""
    uni = rng.integers(-32768, 32768, size=(n, n))
    mag = (2.0 ** rng.uniform(0, 15, size=(n, n))).astype(np.int64) * rng.choice([-1, 1], size=(n, n))
    return np.where(rng.random((n, n)) < 0.5, uni, mag)


def _single(n, x, y, v):
    a = np.zeros((n, n), dtype=np.int64)
    a[y, x] = v
    return a


def case_sizes():
    """Every size and transform on every component at three bit-depth pairs."""
    seqs, pics = [], []
    for si, (bdy, bdc) in enumerate(((8, 8), (10, 10), (12, 8))):
        seqs.append(Seq(160, 128, 5, 3, bdy, bdc, sf=ramp_sf(si) if bdy == 10 else None))
        tbs = []
        for kind in ("4dct", "4dst", "8", "16", "32"):
            n, dst = int(kind.rstrip("dcst")), kind == "4dst"
            for cidx in range(3):
                tag = f"sizes/bd{bdy}_{bdc}/{kind}/c{cidx}"
                rng = _rng(tag)
                pats = [(f"single_x{x}_y{y}", _single(n, x, y, 53 * (-1) ** (x + y + cidx)))
                        for x, y in ((0, 0), (n - 1, 0), (0, n - 1), (n - 1, n - 1), (4, 0), (0, 4)) if x < n and y < n]
                row0, col0 = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
                row0[0, :] = rng.integers(-40, 41, size=n)
                col0[:, 0] = rng.integers(-40, 41, size=n)
                row0[0, n - 1], col0[n - 1, 0] = 9, -9
                small = rng.integers(-3, 4, size=(n, n)) * (rng.random((n, n)) < 0.5)
                pats += [("row0", row0), ("col0", col0), ("dense_small", small), ("dense_full", _full_range(rng, n))]
                for k, (pn, lv) in enumerate(pats):
                    qp = 4 if pn == "dense_full" else 20 + 3 * cidx + n.bit_length()
                    tbs.append(TB(f"{tag}/{pn}", n, cidx, qp, lv, dst=dst, scan_idx=k % 3, hide=bool(k & 1),
                                  row=len(tbs) % 4))
        pics.append(Pic(si, tbs))
    return Case("sizes", seqs, pics)


def _sign(a):
    return np.where(a < 0, -1, 1)


def _saturation_tbs(tag, n, cidx, qp, row):
    rng = _rng(tag)
    M = matrix_of(n)
    out = []
    # the split boundaries of the MFMA operands as levels, along a column, a row and all over
    bv = np.array(BOUNDARY_D, dtype=np.int64)
    col, rw = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    k = min(n, len(bv))
    col[:k, 1 % n], rw[2 % n, :k] = bv[:k], bv[len(bv) - k:]
    out += [("bound_col", col), ("bound_row", rw), ("bound_all", rng.choice(bv, size=(n, n))),
            ("bound_all2", rng.choice(bv, size=(n, n)))]
    # a full-magnitude column with the signs of matrix column i0: the first stage's sum at row i0
    # is 32767 sum |M[.][i0]|, past the clip; negated in the next column
    i0, i1 = n // 2 - 1, n - 1
    clip = np.zeros((n, n), np.int64)
    clip[:, 0] = 32767 * _sign(M[:, i0])
    clip[:, n - 1] = -32767 * _sign(M[:, i1])
    out.append(("clip_cols", clip))
    # ... in every column, signed so that the second stage adds the clipped values up as well
    out.append(("clip_both", 32767 * np.outer(_sign(M[:, i0]), _sign(M[:, 1]))))
    out.append(("clip_both_neg", -32767 * np.outer(_sign(M[:, 0]), _sign(M[:, i1])) - (rng.random((n, n)) < 0.3)))
    out += [("all_max", np.full((n, n), 32767)), ("all_min", np.full((n, n), -32768)),
            ("checker", np.where(np.add.outer(np.arange(n), np.arange(n)) & 1, -32768, 32767))]
    return [TB(f"{tag}/{pn}", n, cidx, qp, lv, row=row) for pn, lv in out]


def case_saturation():
    """Scaled coefficients on the int8 split's boundaries and both stages' sums at
    their largest, where m levelScale / 2^bdShift is 1, 2, 1/2 and more."""
    seqs = [Seq(224, 192, 6, 3, 10, 10), Seq(160, 128, 6, 3, 10, 10, sf=const_sf(8)), Seq(160, 128, 5, 3, 12, 12)]
    pics = [Pic(0, []), Pic(1, []), Pic(2, [])]
    for qp in (4, 22, 51):
        for n in (4, 8, 16, 32):
            pics[0].tbs += _saturation_tbs(f"sat/bd10_flat/qp{qp}/n{n}", n, (qp + n) % 3, qp, len(pics[0].tbs) % 3)
    for n in (8, 16, 32):
        pics[1].tbs += _saturation_tbs(f"sat/bd10_m8/qp4/n{n}", n, n % 3, 4, (n // 8) % 2)
    for n, qp in ((8, 4), (16, 10), (32, 16), (16, 4)):
        pics[2].tbs += _saturation_tbs(f"sat/bd12_flat/qp{qp}/n{n}", n, (n + qp) % 3, qp, len(pics[2].tbs) % 4)
    return Case("saturation", seqs, pics)


def case_records():
    """The record format: escapes, hidden signs, scan orders, record counts."""
    seqs = [Seq(256, 160, 5, 1, 10, 10)]
    tbs = []

    def add(name, n, lv, **kw):
        for cidx in ((0, 1) if n <= 8 else (0,)):
            tbs.append(TB(f"records/n{n}/c{cidx}/{name}", n, cidx, 17 + cidx, np.array(lv, dtype=np.int64),
                          row=len(tbs) % 3, **kw))

    for n in (4, 8, 32):
        rng = _rng(f"records{n}")

        def blank():
            return np.zeros((n, n), dtype=np.int64)

        def put(a, sb, k, v, scan_idx=0):  # level v at scan position k of sub-block sb = (xS, yS)
            px, py = scan_order(4, scan_idx)[k]
            a[4 * sb[1] + py, 4 * sb[0] + px] = v
            return a

        far = (n // 4 - 1, n // 4 - 1)
        add("esc_none_15_is_no_escape", n, put(put(put(blank(), (0, 0), 0, 15), (0, 0), 5, -15), far, 9, 14))
        add("esc_16_is_the_first_escape", n, put(put(blank(), (0, 0), 3, 16), far, 2, -16))
        add("esc_one", n, put(put(put(blank(), (0, 0), 2, 3), (0, 0), 6, -777), (0, 0), 11, 1))
        a = blank()
        for k, v in ((15, -32768), (12, 5), (7, 32767), (6, -2), (3, 16), (0, 300)):
            put(a, (0, 0), k, v)
        add("esc_several_pos15", n, a)
        add("esc_all16", n, np.pad(rng.integers(16, 32768, size=(4, 4)) * rng.choice([-1, 1], size=(4, 4)),
                                   ((0, n - 4), (0, n - 4))))
        add("pos15_alone", n, put(blank(), far, 15, -7))
        add("pos15_escape_alone", n, put(blank(), (0, 0), 15, 4242))
        if n > 4:
            a = blank()
            for sb in scan_order(n // 4, 0)[:4]:
                for k in (14, 9, 8, 1):
                    put(a, sb, k, int(rng.integers(16, 30000)) * (-1) ** k)
                put(a, sb, 4, 2)
            add("esc_consecutive_subblocks", n, a)
        # hidden signs: first and last significant positions more than 3 apart
        for par, extra in (("even", 1), ("odd", 2)):
            a = put(put(put(blank(), (0, 0), 1, 4), (0, 0), 7, -3), (0, 0), 12, extra)
            add(f"hidden_{par}_sum", n, a, hide=True)
            a = put(put(put(blank(), far, 0, 9), far, 10, -20000 - extra), far, 15, 18)
            add(f"hidden_{par}_sum_with_escapes", n, a, hide=True)
        a = put(put(blank(), (0, 0), 2, 32767), (0, 0), 13, -32768)  # the hidden one an escape itself
        add("hidden_escape_lowest", n, a, hide=True)
        add("hidden_span_3_keeps_its_sign", n, put(put(blank(), (0, 0), 2, -1), (0, 0), 5, 1), hide=True)
        dense = rng.integers(-40, 41, size=(n, n))
        add("hidden_dense", n, dense, hide=True)
        for sc in range(3):
            lv = rng.integers(-20, 21, size=(n, n)) * (rng.random((n, n)) < 0.6)
            lv[1, 3], lv[3, 1], lv[n - 1, n - 2] = 17, -19, 23  # (no symmetry for a swapped scan to hide behind)
            add(f"scan{sc}", n, lv, scan_idx=sc, hide=bool(sc & 1))
        if n == 32:
            add("one_record", n, put(put(blank(), (5, 6), 3, -12), (5, 6), 8, 600))
            lv = rng.integers(-9, 10, size=(n, n)) * (rng.random((n, n)) < 0.4)
            lv[0::4, 0::4] = 11  # every sub-block coded
            add("64_records", n, lv)
            assert all(lv[4 * y:4 * y + 4, 4 * x:4 * x + 4].any() for x in range(8) for y in range(8))
    return Case("records", seqs, [Pic(0, tbs)])


def case_flags():
    """Transform skip, bypass, PCM, scaling lists and the chroma formats' planes."""
    seqs = [Seq(136, 104, 4, 1, 8, 8, sf=ramp_sf(11)), Seq(160, 96, 5, 2, 10, 10, sf=ramp_sf(22)),
            Seq(128, 96, 6, 3, 12, 8, sf=ramp_sf(33)), Seq(200, 72, 5, 0, 10, 10)]
    pics = []
    for si, s in enumerate(seqs):
        tbs = []
        for cidx in range(3 if s.chroma_format else 1):
            w, h = s.plane(cidx)
            for n in (4, 8, 16, 32):
                if n > min(w, h) or (n == 32 and cidx and s.chroma_format != 3):
                    continue
                tag = f"flags/cf{s.chroma_format}_bd{s.bd_y}_{s.bd_c}/n{n}/c{cidx}"
                rng = _rng(tag)
                qp = 10 + 7 * cidx + n.bit_length()
                small = rng.integers(-6, 7, size=(n, n)) * (rng.random((n, n)) < 0.7)
                small[0, n - 1], small[n - 1, 0] = 5, -4
                kw = dict(row=len(tbs) % s.rows)
                tbs.append(TB(f"{tag}/list_dense", n, cidx, qp, small, scan_idx=n % 3, **kw))
                tbs.append(TB(f"{tag}/list_level1_everywhere", n, cidx, 28, np.ones((n, n), np.int64), **kw))
                if n == 4:
                    tbs.append(TB(f"{tag}/list_dst", n, cidx, qp, small[::-1].copy(), dst=True, **kw))
                tbs.append(TB(f"{tag}/tskip", n, cidx, qp, small * 3, ts=True, **kw))
                tbs.append(TB(f"{tag}/tskip_full", n, cidx, 4, _full_range(rng, n), ts=True, hide=True, **kw))
                tbs.append(TB(f"{tag}/bypass", n, cidx, qp, _full_range(rng, n), bypass=True, **kw))
                tbs.append(TB(f"{tag}/pcm", n, cidx, qp, rng.integers(-32768, 32768, size=(n, n)), bypass=True,
                              pcm=True, **kw))
        pics.append(Pic(si, tbs))
    return Case("flags", seqs, pics)


def _dispatch_row0(seed):
    """Row 0 of the dispatch picture: what each record is, in order."""
    rng = np.random.default_rng(seed)
    kinds = ["sat32", "sat32", "u", "c8", "dense16", "dense16", "c4", "u"]  # waves 0 and 1: a 16x16 after a 32x32
    kinds += list(rng.choice(["u", "c4", "c4", "c4", "c8", "c4c", "c8c"], size=300))
    kinds[40], kinds[41], kinds[97], kinds[170] = "c16", "c32", "c16", "c16"
    kinds[301], kinds[306] = "sat32b", "dense16b"  # the second 64-record window of wave 1 and 2
    return kinds


def ballot_counts(recs, waves=4):
    """Coded 4x4 TBs per (wave, 64-record window) of a row's TU records."""
    out = {}
    for t, r in enumerate(recs):
        if (r["flags"] & TU_CBF) and r["log2"] == 2:
            key = (t % waves, t // waves // 64)
            out[key] = out.get(key, 0) + 1
    return out


def case_dispatch():
    """How k_transform hands records to waves: long rows, mixed records, several
    pictures and parameter sets, an assembly picture, plane edges."""
    seqs = [Seq(128, 128, 6, 1, 8, 8), Seq(96, 32, 5, 2, 10, 12, sf=ramp_sf(5))]
    M = matrix_of(32)

    def picture(seed, prefix):
        rng = np.random.default_rng(1000 + seed)
        tbs, kinds = [], _dispatch_row0(seed)
        # the plane edges first, so that the free slots go to the rest
        edge = [("edge/luma4_corner", 4, 0, 124, 124), ("edge/luma8_right", 8, 0, 120, 0),
                ("edge/luma16_bottom", 16, 0, 0, 112), ("edge/luma32_right", 32, 0, 96, 64),
                ("edge/cb4_corner", 4, 1, 60, 60), ("edge/cr8_corner", 8, 2, 56, 56), ("edge/cr16_right", 16, 2, 48, 0)]
        for name, n, cidx, x, y in edge:
            tbs.append(TB(f"{prefix}/{name}", n, cidx, 30, rng.integers(-30, 31, size=(n, n)), row=1, x=x, y=y))
        tbs.append(TB(f"{prefix}/edge/luma4_past_the_right_edge", 4, 0, 30, np.full((4, 4), 99), row=1, x=126, y=8,
                      outside=True))
        tbs.append(TB(f"{prefix}/edge/cb8_past_the_bottom_edge", 8, 1, 30, np.full((8, 8), 99), row=1, x=0, y=60,
                      outside=True))
        for k in range(30):  # the rest of row 1
            n = (4, 8, 4, 16)[k % 4]
            tbs.append(TB(f"{prefix}/row1/{k}_n{n}", n, k % 3 if n < 16 else 0, 26 + k % 9,
                          rng.integers(-60, 61, size=(n, n)), row=1, coded=k % 5 != 4, dst=(n == 4 and k % 3 == 0)))
        for t, kind in enumerate(kinds):
            name = f"{prefix}/row0/{t}_{kind}"
            if kind.startswith("sat32"):
                lv = 32767 * np.outer(_sign(M[:, 15]), _sign(M[:, 3 + t % 5]))
                tbs.append(TB(name, 32, 0, 51, lv))
            elif kind.startswith("dense16") or kind == "c16":
                tbs.append(TB(name, 16, 0, 24, rng.integers(-90, 91, size=(16, 16))))
            elif kind == "c32":
                tbs.append(TB(name, 32, 0, 24, rng.integers(-90, 91, size=(32, 32))))
            elif kind == "u":  # not coded: its words are whatever the row holds
                n = (4, 8, 16, 32)[t % 4]
                tbs.append(TB(name, n, t % 3, 30, rng.integers(-5, 6, size=(n, n)), coded=False))
            else:
                n, cidx = int(kind[1]), (1 + t % 2 if kind.endswith("c") else 0)
                lv = rng.integers(-300, 301, size=(n, n)) * (rng.random((n, n)) < 0.5)
                lv[n - 1, n - 1] = 1 + t
                tbs.append(TB(name, n, cidx, 20 + t % 25, lv, dst=(n == 4 and t % 7 == 0), ts=(t % 11 == 0),
                              scan_idx=t % 3, hide=bool(t & 1)))
        return tbs

    # the first row-0 order whose coded 4x4 counts leave every ballot window a last round that is not full
    for seed in range(64):
        tbs = picture(seed, "dispatch/main")
        recs = [t for t in tbs if t.row == 0]
        counts = {}
        for t, tb in enumerate(recs):
            if tb.coded and tb.n == 4:
                counts[(t % 4, t // 256)] = counts.get((t % 4, t // 256), 0) + 1
        if len(counts) == 8 and all(c % 4 for c in counts.values()):
            break
    else:
        raise AssertionError("no dispatch order with ragged ballot windows")
    rng = np.random.default_rng(77)
    other = [TB(f"dispatch/other_seq/{k}_n{n}", n, k % 3, 22 + k, rng.integers(-200, 201, size=(n, n)),
                scan_idx=k % 3) for k, n in enumerate((32, 16, 4, 8, 4, 8, 4, 16, 4))]
    ghost = [TB(f"dispatch/assembly/{k}", n, 0, 30, rng.integers(-50, 51, size=(n, n)), row=k % 2)
             for k, n in enumerate((32, 4, 8, 16))]
    before = [TB(f"dispatch/before_pic0/{k}", n, 0, 30, rng.integers(-50, 51, size=(n, n)), row=k % 2)
              for k, n in enumerate((4, 16, 8, 32))]
    # picture 0 lies before pic0: not launched.  The one-row picture comes before the rest, so a
    # block of its missing second row would find the next picture's row counters
    pics = [Pic(0, before, launched=False), Pic(1, other), Pic(0, tbs), Pic(0, ghost, flags=PD_ASSEMBLY),
            Pic(1, [dataclasses.replace(t, name=t.name + "/again", x=None, y=None) for t in other])]
    return Case("dispatch", seqs, pics, pic0=1)


CASES = {"sizes": case_sizes, "saturation": case_saturation, "records": case_records, "flags": case_flags,
         "dispatch": case_dispatch}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once (its expected residuals stay as computed)."""
    c = CASES[name]()
    c.expected.setflags(write=False)
    return c
