"""Hand-built inputs of k_assemble / k_deblock / k_sao_out and what they must leave.

A case is one file for tests/loopfilter/lf_driver.cpp: a few batches (one
BatchArgs each: one sample size), each with several small pictures in the
product's own structs.  Every batch's sample arena and output allocation are
pre-filled with a sentinel; `expected` is the two buffers as the model
(tests/loopfilter_ref.py) leaves them, and every picture's events are kept for
the coverage tests.  Nothing here reads the kernels' sources.

The luma decision vectors are steered: a pool of candidate segments (flat,
step, ramp, curvature and small noise, with their own QpY pair) goes through
the model as one tall picture of its own, and for each (event, code) not seen
yet one candidate that shows it is placed on an edge segment.  A steering
picture flags the edges of one direction only, so that what a segment was built
for is what the kernel meets; the `both` pictures flag every edge of both
directions.
"""
import dataclasses
import functools
import struct

import numpy as np

import loopfilter_ref as ref
from xform_vectors import PIC_DTYPE, SEQ_DTYPE

MAGIC = 0x3143464C
SENTINEL = 0xA5
MF_EDGE_V, MF_EDGE_H, MF_NOFILT = ref.MF_EDGE_V, ref.MF_EDGE_H, ref.MF_NOFILT
PD_CHILD, PD_ASSEMBLY = 1, 2

SAO_DTYPE = np.dtype([("type", "i1", (3,)), ("band_eo", "u1", (3,)), ("off", "<i2", (3, 4)), ("pad", "<i2")],
                     align=True)
OUT_DTYPE = np.dtype([("plane", "<u8", (3,)), ("pitch", "<i4", (3,)), ("width", "<i4"), ("height", "<i4")],
                     align=True)
SEQ_FIELDS = ("width", "height", "log2_ctb", "chroma_format", "bit_depth_y", "bit_depth_c", "cb_qp_offset",
              "cr_qp_offset", "conf_l", "conf_t", "out_w", "out_h")
PIC_FIELDS = ("seq", "sao_luma", "sao_chroma", "dbk_disabled", "beta_off", "tc_off", "image", "out_x", "out_y",
              "recon_off", "map_off", "sao_off", "flags", "org_x", "org_y", "child0", "nchild")
CONSTANTS = {"MF_EDGE_V": MF_EDGE_V, "MF_EDGE_H": MF_EDGE_H, "MF_NOFILT": MF_NOFILT, "PD_CHILD": PD_CHILD,
             "PD_ASSEMBLY": PD_ASSEMBLY}


def layout_of_mirrors():
    """{name: value} in the form `lf_driver --layout` prints."""
    out = dict(CONSTANTS)
    for name, dt, fields in (("SeqParams", SEQ_DTYPE, SEQ_FIELDS), ("PicDesc", PIC_DTYPE, PIC_FIELDS),
                             ("SaoParams", SAO_DTYPE, SAO_DTYPE.names), ("OutImage", OUT_DTYPE, OUT_DTYPE.names)):
        out[name] = dt.itemsize
        for f in fields:
            out[f"{name}.{f}"] = dt.fields[f][1]
    return out


def _rng(tag):
    h = 2166136261
    for ch in tag.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return np.random.default_rng(h)


# ---------------------------------------------------------------- pictures, images, batches
@dataclasses.dataclass
class Pic:
    W: int
    H: int
    fmt: int = 0
    bd_y: int = 8
    bd_c: int = 0            # 0: as luma
    log2_ctb: int = 4
    cb_off: int = 0
    cr_off: int = 0
    conf_l: int = 0
    conf_t: int = 0
    out_w: int = 0           # 0: the rest of the picture
    out_h: int = 0
    beta_off: int = 0
    tc_off: int = 0
    sao_luma: int = 0
    sao_chroma: int = 0
    dbk_disabled: int = 0
    flags: int = 0
    image: int = 0
    out_x: int = 0
    out_y: int = 0
    org_x: int = 0
    org_y: int = 0
    children: tuple = ()     # PD_ASSEMBLY: indices of its children in the batch (consecutive)
    skew: int = 0            # samples by which the picture's planes miss the 8-sample alignment of the arena
    name: str = ""
    planes: list = None
    qpy: np.ndarray = None
    flg: np.ndarray = None
    sao: np.ndarray = None

    def __post_init__(self):
        self.bd_c = self.bd_c or self.bd_y
        self.out_w = self.out_w or self.W - self.conf_l
        self.out_h = self.out_h or self.H - self.conf_t
        self.sx, self.sy = ref.subsampling(self.fmt)
        self.cw, self.ch = (self.W >> self.sx, self.H >> self.sy) if self.fmt else (0, 0)
        self.w4, self.h4 = self.W >> 2, self.H >> 2
        ctb = 1 << self.log2_ctb
        self.wctb, self.hctb = (self.W + ctb - 1) >> self.log2_ctb, (self.H + ctb - 1) >> self.log2_ctb
        self.ncomp = 3 if self.fmt else 1
        if self.qpy is None:
            self.qpy = np.full((self.h4, self.w4), 30, dtype=np.int8)
        if self.flg is None:
            self.flg = np.zeros((self.h4, self.w4), dtype=np.uint8)
        if self.sao is None:
            self.sao = np.zeros((self.hctb, self.wctb), dtype=SAO_DTYPE)
        self.events = {}
        self.given = None

    def shape(self, cidx):
        return (self.ch, self.cw) if cidx else (self.H, self.W)

    def bd(self, cidx):
        return self.bd_c if cidx else self.bd_y

    def n_samples(self):
        return self.W * self.H + 2 * self.cw * self.ch

    def sao_fields(self):
        return {k: self.sao[k] for k in ("type", "band_eo", "off")}


@dataclasses.dataclass
class Image:
    width: int
    height: int
    skew: int = 0       # samples between the allocation's 256-byte boundary and each plane's base
    pad: int = 0        # samples of pitch beyond the plane's width


class Batch:
    def __init__(self, sz, fmt, pics, images, pic0=0, n_launch=None, name=""):
        self.sz, self.fmt, self.pics, self.images, self.pic0, self.name = sz, fmt, pics, images, pic0, name
        self.n_launch = len(pics) - pic0 if n_launch is None else n_launch
        self.dt = np.dtype("u1") if sz == 1 else np.dtype("<u2")
        self._layout()
        self._expect()

    def _layout(self):
        sz = self.sz
        cur_r = cur_m = cur_s = 0
        for k, p in enumerate(self.pics):
            assert p.fmt == self.fmt and p.W % 8 == 0 and p.H % 8 == 0
            cur_r = (cur_r + 7 * sz + 8 * sz - 1) // (8 * sz) * (8 * sz)  # a gap, then 8-sample alignment
            p.recon_off = cur_r + p.skew * sz
            cur_r = p.recon_off + p.n_samples() * sz
            cur_m += 5 + (k % 3)
            p.map_off = cur_m
            cur_m += 2 * p.w4 * p.h4
            cur_s += k % 2
            p.sao_off = cur_s
            cur_s += p.wctb * p.hctb
        self.recon_bytes, self.map_bytes, self.n_sao = cur_r + 9 * sz, cur_m + 3, cur_s + 1
        cur = 0
        self.plane_off, self.pitch, self.rows = [], [], []
        sx, sy = ref.subsampling(self.fmt)
        for im in self.images:
            offs, pitches, rows = [0, 0, 0], [0, 0, 0], [0, 0, 0]
            for c in range(3 if self.fmt else 1):
                w = (im.width + (1 << sx) - 1) >> sx if c else im.width
                h = (im.height + (1 << sy) - 1) >> sy if c else im.height
                cur = (cur + 255) // 256 * 256
                offs[c], pitches[c], rows[c] = cur + im.skew * sz, (w + im.pad) * sz, h
                cur = offs[c] + pitches[c] * h
            self.plane_off.append(offs)
            self.pitch.append(pitches)
            self.rows.append(rows)
        self.out_bytes = cur + 16

    # -- the blob
    def blob(self):
        seqs = np.zeros(len(self.pics), dtype=SEQ_DTYPE)
        pics = np.zeros(len(self.pics), dtype=PIC_DTYPE)
        maps = _rng("maps" + self.name).integers(0, 256, self.map_bytes).astype(np.uint8)
        sao = np.zeros(self.n_sao, dtype=SAO_DTYPE)
        sao["type"] = 2  # between the pictures' parameters: would filter if it were read
        sao["off"] = 5
        for k, p in enumerate(self.pics):
            s, d = seqs[k], pics[k]
            s["width"], s["height"], s["log2_ctb"], s["chroma_format"] = p.W, p.H, p.log2_ctb, p.fmt
            s["log2_min_cb"], s["log2_min_tb"], s["log2_max_tb"] = 3, 2, 5
            s["bit_depth_y"], s["bit_depth_c"] = p.bd_y, p.bd_c
            s["cb_qp_offset"], s["cr_qp_offset"] = p.cb_off, p.cr_off
            s["conf_l"], s["conf_t"], s["out_w"], s["out_h"] = p.conf_l, p.conf_t, p.out_w, p.out_h
            d["seq"], d["sao_luma"], d["sao_chroma"], d["dbk_disabled"] = k, p.sao_luma, p.sao_chroma, p.dbk_disabled
            d["beta_off"], d["tc_off"] = p.beta_off, p.tc_off
            d["image"], d["out_x"], d["out_y"] = p.image, p.out_x, p.out_y
            d["recon_off"], d["map_off"], d["sao_off"], d["flags"] = p.recon_off, p.map_off, p.sao_off, p.flags
            d["org_x"], d["org_y"] = p.org_x, p.org_y
            if p.children:
                d["child0"], d["nchild"] = p.children[0], len(p.children)
            n = p.w4 * p.h4
            qpy, flg, prm = p.given or (p.qpy, p.flg, p.sao)  # an assembly: what lay there before k_assemble
            maps[p.map_off:p.map_off + n] = qpy.astype(np.int8).view(np.uint8).ravel()
            maps[p.map_off + n:p.map_off + 2 * n] = flg.ravel()
            sao[p.sao_off:p.sao_off + p.wctb * p.hctb] = prm.ravel()
        outs = np.zeros(len(self.images), dtype=OUT_DTYPE)
        for k, im in enumerate(self.images):
            outs[k]["plane"], outs[k]["pitch"] = self.plane_off[k], self.pitch[k]
            outs[k]["width"], outs[k]["height"] = im.width, im.height
        has_asm = int(any(p.flags & PD_ASSEMBLY for p in self.pics))
        head = struct.pack("<16I", len(seqs), len(pics), self.pic0, self.n_launch, len(outs), self.map_bytes,
                           self.n_sao, self.recon_bytes, self.out_bytes, self.sz, self.fmt, has_asm, SENTINEL, 0, 0, 0)
        return b"".join([head, seqs.tobytes(), pics.tobytes(), outs.tobytes(), maps.tobytes(), sao.tobytes(),
                         self.recon0.tobytes()])

    # -- the arenas
    def _put(self, arena, p, planes):
        off = p.recon_off
        for c, pl in enumerate(planes):
            assert pl.shape == p.shape(c) and pl.min() >= 0 and pl.max() < (1 << (8 * self.sz))
            b = pl.astype(self.dt).tobytes()
            arena[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
            off += len(b)

    def view(self, buf, image, cidx):
        """the caller's plane as (rows, pitch in samples)"""
        return np.ndarray((self.rows[image][cidx], self.pitch[image][cidx] // self.sz), dtype=self.dt, buffer=buf,
                          offset=self.plane_off[image][cidx])

    def _assemble(self, p):
        kids = [self.pics[i] for i in p.children]
        for c in range(p.ncomp):
            kx, ky = (p.sx, p.sy) if c else (0, 0)
            for k in kids:
                h, w = k.shape(c)
                p.planes[c][(k.org_y >> ky):(k.org_y >> ky) + h, (k.org_x >> kx):(k.org_x >> kx) + w] = k.planes[c]
        for k in kids:
            y4, x4, yc, xc = k.org_y >> 2, k.org_x >> 2, k.org_y >> p.log2_ctb, k.org_x >> p.log2_ctb
            p.qpy[y4:y4 + k.h4, x4:x4 + k.w4] = k.qpy
            p.flg[y4:y4 + k.h4, x4:x4 + k.w4] = k.flg
            p.sao[yc:yc + k.hctb, xc:xc + k.wctb] = k.sao if (k.sao_luma or k.sao_chroma) else np.zeros_like(k.sao)

    def _expect(self):
        recon = np.full(self.recon_bytes, SENTINEL, dtype=np.uint8)
        for p in self.pics:
            self._put(recon, p, p.planes)
        self.recon0 = recon.copy()
        out = np.full(self.out_bytes, SENTINEL, dtype=np.uint8)
        for p in self.pics[self.pic0:self.pic0 + self.n_launch]:
            if p.flags & PD_ASSEMBLY:
                p.given = (p.qpy, p.flg, p.sao)  # the case file carries these, the model what k_assemble makes of them
                p.planes = [pl.copy() for pl in p.planes]
                p.qpy, p.flg, p.sao = p.qpy.copy(), p.flg.copy(), p.sao.copy()
                self._assemble(p)
            if p.flags & PD_CHILD:
                continue
            planes = [pl.astype(np.int64) for pl in p.planes]
            if not p.dbk_disabled:
                planes, ev = ref.deblock(planes, p.qpy, p.flg, p.fmt, p.bd_y, p.bd_c, p.cb_off, p.cr_off, p.beta_off,
                                         p.tc_off)
                p.events.update({("dbk",) + k: v for k, v in ev.items()})
            p.deblocked = planes
            self._put(recon, p, planes)
            if p.sao_luma or p.sao_chroma:
                planes, ev = ref.sao(planes, p.flg, p.sao_fields(), p.log2_ctb, p.fmt, p.bd_y, p.bd_c)
                p.events.update({("sao", k): v for k, v in ev.items()})
            im = self.images[p.image]
            views = [self.view(out, p.image, c) for c in range(p.ncomp)]
            ref.place(views, planes, p.conf_l, p.conf_t, p.out_w, p.out_h, im.width, im.height, p.out_x, p.out_y, p.fmt)
        self.expected_recon, self.expected_out = recon, out

    # -- what differs
    def failures(self, recon, out):
        bad = []
        for name, got, want in (("samples", recon, self.expected_recon), ("output", out, self.expected_out)):
            idx = np.flatnonzero(got != want)
            for i in idx[:6]:
                where = ""
                if name == "samples":
                    for k, p in enumerate(self.pics):
                        if p.recon_off <= i < p.recon_off + p.n_samples() * self.sz:
                            s = (int(i) - p.recon_off) // self.sz
                            c = 0 if s < p.W * p.H else 1 + (s - p.W * p.H) // (p.cw * p.ch)
                            s -= 0 if c == 0 else p.W * p.H + (c - 1) * p.cw * p.ch
                            w = p.shape(c)[1]
                            where = f" pic {k} {p.name} c{c} ({s % w}, {s // w})"
                else:
                    for k in range(len(self.images)):
                        for c in range(3 if self.fmt else 1):
                            o = int(i) - self.plane_off[k][c]
                            if 0 <= o < self.pitch[k][c] * self.rows[k][c]:
                                where = f" image {k} c{c} ({o % self.pitch[k][c] // self.sz}, {o // self.pitch[k][c]})"
                bad.append(f"batch {self.name} {name} byte {int(i)}{where}: {int(got[i])} != {int(want[i])}")
            if len(idx) > 6:
                bad.append(f"batch {self.name} {name}: {len(idx)} bytes differ")
        return bad


class Case:
    def __init__(self, name, batches):
        self.name, self.batches = name, batches
        self.blob = struct.pack("<2I", MAGIC, len(batches)) + b"".join(b.blob() for b in batches)
        self.expected = np.concatenate([np.concatenate([b.expected_recon, b.expected_out]) for b in batches])

    def pics(self):
        """(batch, picture) of every launched picture"""
        return [(b, p) for b in self.batches for p in b.pics[b.pic0:b.pic0 + b.n_launch]]

    def failures(self, result):
        if result.size != self.expected.size:
            return [f"result of {result.size} bytes, expected {self.expected.size}"]
        bad, at = [], 0
        for b in self.batches:
            r = result[at:at + b.recon_bytes]
            o = result[at + b.recon_bytes:at + b.recon_bytes + b.out_bytes]
            at += b.recon_bytes + b.out_bytes
            bad += b.failures(r, o)
        return bad

    def seen(self, stage, kind=None, where=lambda b, p: True):
        """{direction or None: set of (event, code)} over the launched pictures"""
        got = {}
        for b, p in self.pics():
            if not where(b, p):
                continue
            for key, ev in p.events.items():
                if key[0] == stage and (kind is None or key[1] == kind):
                    got.setdefault(key[2] if len(key) > 2 else None, set()).update(ref.seen(ev))
        return got


# ---------------------------------------------------------------- content
def blocky(rng, p, amp=2, step=6, lo=None, hi=None):
    """planes of 8x8 (luma) blocks of slowly wandering level plus noise of +-amp, scaled to the bit depth"""
    planes = []
    for c in range(p.ncomp):
        h, w = p.shape(c)
        k = 1 << (p.bd(c) - 8)
        maxv = (1 << p.bd(c)) - 1
        bw, bh = 8 >> (p.sx if c else 0), 8 >> (p.sy if c else 0)
        l0 = 128 if lo is None else None
        base = rng.integers(-step, step + 1, ((h + bh - 1) // bh, (w + bw - 1) // bw)).cumsum(axis=1)
        base = base + rng.integers(-step, step + 1, (base.shape[0], 1)).cumsum(axis=0)
        base = base + (l0 if l0 is not None else rng.integers(lo, hi + 1))
        pl = np.kron(base, np.ones((bh, bw), dtype=np.int64))[:h, :w] * k
        pl = pl + rng.integers(-amp * k, amp * k + 1, (h, w))
        planes.append(np.clip(pl, 0, maxv))
    return planes


def all_edges(p, mask=MF_EDGE_V | MF_EDGE_H):
    f = np.zeros((p.h4, p.w4), dtype=np.uint8)
    f[:, 0::2] |= mask & MF_EDGE_V
    f[0::2, :] |= mask & MF_EDGE_H
    return f


def rand_qpy(rng, p, lo, hi):
    """QpY per 8x8 block, as a coding unit would give it"""
    q = rng.integers(lo, hi + 1, ((p.h4 + 1) // 2, (p.w4 + 1) // 2))
    return np.kron(q, np.ones((2, 2), dtype=np.int64))[:p.h4, :p.w4].astype(np.int8)


def sao_max(bd):
    """largest |SaoOffsetVal| (7.4.9.3.2)"""
    return ((1 << (min(bd, 10) - 5)) - 1) << (bd - min(bd, 10))


BAND_POSITIONS = (0, 28, 29, 30, 31)


def rand_sao(rng, p, luma=True, chroma=True):
    """SaoParams per CTB: type, class / band position and offsets of both signs,
    each drawn per CTB and component; the full offset range in one CTB of four."""
    s = np.zeros((p.hctb, p.wctb), dtype=SAO_DTYPE)
    for c in range(p.ncomp):
        if not (chroma if c else luma):
            continue
        m = sao_max(p.bd(c))
        s["type"][:, :, c] = rng.integers(0, 3, (p.hctb, p.wctb))
        cls = rng.integers(0, 4, (p.hctb, p.wctb))
        pos = rng.choice(BAND_POSITIONS + (8, 15, 16), (p.hctb, p.wctb))
        s["band_eo"][:, :, c] = np.where(s["type"][:, :, c] == 2, cls, pos)
        small = rng.integers(-3, 4, (p.hctb, p.wctb, 4))
        big = rng.choice((-m, m), (p.hctb, p.wctb, 4))
        s["off"][:, :, c, :] = np.where(rng.integers(0, 4, (p.hctb, p.wctb, 1)) == 0, big, small)
    return s


def band_content(rng, p):
    """samples spread over the bands 26..31 and 0..5, where the band positions used put their offsets"""
    planes = []
    for c in range(p.ncomp):
        shift = p.bd(c) - 5
        band = rng.choice(np.r_[26:32, 0:6], p.shape(c))
        planes.append((band << shift) + rng.integers(0, 1 << shift, p.shape(c)))
    return planes


def force_types(s, ncomp, t):
    """no CTB without SAO: type 0 becomes t (an edge class out of what was a band position)"""
    was0 = s["type"] == 0
    s["band_eo"] = np.where(was0 & (t == 2), s["band_eo"] & 3, s["band_eo"])
    s["type"] = np.where(was0, t, s["type"]) * (np.arange(3) < ncomp)


def sao_content(rng, p):
    """per CTB a base level at the bottom, the top or anywhere in the range, samples within 0..3 of it:
    ties between neighbours are common, band 0 and band 31 are populated and the clips at 0 and the
    maximum are reached"""
    planes = []
    for c in range(p.ncomp):
        h, w = p.shape(c)
        maxv = (1 << p.bd(c)) - 1
        cwid, chei = (1 << p.log2_ctb) >> (p.sx if c else 0), (1 << p.log2_ctb) >> (p.sy if c else 0)
        kind = rng.integers(0, 3, (p.hctb, p.wctb))
        base = np.where(kind == 0, 0, np.where(kind == 1, maxv - 3, rng.integers(0, maxv - 2, (p.hctb, p.wctb))))
        pl = np.kron(base, np.ones((chei, cwid), dtype=np.int64))[:h, :w] + rng.integers(0, 4, (h, w))
        planes.append(np.clip(pl, 0, maxv))
    return planes


# ---------------------------------------------------------------- steering the luma decisions
def _candidates(rng, n, bd):
    """n segments as a (4 n, 16) plane with the edge at x = 8, and their QpY pairs"""
    maxv = (1 << bd) - 1
    k = (1 << rng.integers(0, bd - 7, (n, 1, 1)))
    pick = lambda lo, hi, shape=(n, 1, 1): rng.integers(lo, hi + 1, shape)
    x = np.arange(-4, 4)[None, None, :]
    side_q = (x >= 0)
    near = np.where(pick(0, 1) == 0, pick(0, 3), pick(0, 6 * 16))
    level = np.where(pick(0, 2) == 0, np.where(pick(0, 1) == 0, near, maxv - near), pick(0, maxv))
    step = pick(-60, 60) * k
    big = np.where(pick(0, 2) == 0, pick(-400, 400, (n, 4, 1)) * k, 0)   # a step of its own on each line
    big[:, [0, 3], :] = np.where(pick(0, 3) == 0, big[:, [0, 3], :], 0)  # rarely on the deciding lines
    steep = np.where(pick(0, 2) == 0, 8, 1)
    slope_p, slope_q = pick(-3, 3) * k * steep, pick(-3, 3) * k * steep
    curve_p, curve_q = pick(0, 2) * pick(0, 8, (n, 4, 1)) * k, pick(0, 2) * pick(0, 8, (n, 4, 1)) * k
    far_p, far_q = pick(0, 1) * pick(-6, 6, (n, 4, 1)) * k, pick(0, 1) * pick(-6, 6, (n, 4, 1)) * k
    noise = pick(0, 2) * pick(-1, 1, (n, 4, 8)) * np.where(pick(0, 1) == 0, 1, k)
    v = level + np.where(side_q, step + big + slope_q * x, slope_p * (x + 1))
    v = v + np.where(x <= -3, curve_p, 0) + np.where(x >= 2, curve_q, 0)
    v = v + np.where(x == -4, far_p, 0) + np.where(x == 3, far_q, 0) + noise
    plane = np.zeros((4 * n, 16), dtype=np.int64)
    plane[:, 4:12] = np.clip(v, 0, maxv).reshape(4 * n, 8)
    lo = -6 * (bd - 8)
    qp_q = rng.integers(lo, 52, n)
    qp_p = np.where(rng.integers(0, 3, n) == 0, rng.integers(lo, 52, n), np.clip(qp_q + rng.integers(-3, 4, n), lo, 51))
    return plane, qp_p, qp_q


def steer(tag, bd, beta_off, tc_off, n_seg, covered, n=20000):
    """n_seg segments (4 x 8 samples, QpP, QpQ): first one for each event not in
    `covered` that the pool shows (`covered` is updated), the rest as they come."""
    rng = _rng(tag)
    plane, qp_p, qp_q = _candidates(rng, n, bd)
    qpy = np.zeros((n, 4), dtype=np.int64)
    qpy[:, 1], qpy[:, 2] = qp_p, qp_q
    flg = np.zeros((n, 4), dtype=np.uint8)
    flg[:, 2] = MF_EDGE_V
    _, ev = ref.luma_vertical(plane, qpy, flg, bd, beta_off, tc_off)
    chosen = []
    for key, m in sorted(ref.columns(ev).items()):
        m = m[:, 0]
        if m.shape[0] == 4 * n:
            m = m.reshape(n, 4).any(axis=1)
        if key in covered or len(chosen) >= n_seg:
            continue
        i = int(np.flatnonzero(m)[0])
        chosen.append(i)
        for k2, m2 in ref.columns({a: (b[4 * i:4 * i + 4] if b.shape[0] == 4 * n else b[i:i + 1])
                                   for a, b in ev.items()}).items():
            covered.add(k2)
    rest = [int(i) for i in rng.permutation(n)[:n_seg - len(chosen)]]
    return [(plane[4 * i:4 * i + 4, 4:12], int(qp_p[i]), int(qp_q[i])) for i in chosen + rest]


def steered_pic(tag, bd, beta_off, tc_off, covered, W=64, H=32, transpose=False):
    """a luma-only picture whose every vertical-edge segment comes from steer();
    transposed: the same for horizontal edges"""
    ne, ns = W // 8 - 1, H // 4
    segs = steer(tag, bd, beta_off, tc_off, ne * ns, covered)
    rng = _rng(tag + "fill")
    Y = rng.integers(0, 1 << bd, (H, W))
    qpy = np.full((H // 4, W // 4), 26, dtype=np.int8)
    for i, (patch, qp_p, qp_q) in enumerate(segs):
        e, s = i % ne, i // ne
        x = 8 * (e + 1)
        Y[4 * s:4 * s + 4, x - 4:x + 4] = patch
        qpy[s, (x >> 2) - 1], qpy[s, x >> 2] = qp_p, qp_q
    if transpose:
        p = Pic(H, W, bd_y=bd, beta_off=beta_off, tc_off=tc_off, name=tag)
        p.planes, p.qpy = [Y.T.copy()], qpy.T.copy()
        p.flg = all_edges(p, MF_EDGE_H)
    else:
        p = Pic(W, H, bd_y=bd, beta_off=beta_off, tc_off=tc_off, name=tag)
        p.planes, p.qpy = [Y], qpy
        p.flg = all_edges(p, MF_EDGE_V)
    return p


def strong_everywhere(bd, name):
    """64x32, every edge of both directions flagged, flat 8x8 blocks a small step
    apart at a high QpY: the strong filter on every 8-grid line, side by side"""
    p = Pic(64, 32, bd_y=bd, name=name)
    rng = _rng(name)
    k = 1 << (bd - 8)
    base = 100 + rng.integers(-2, 3, (1, 8)).cumsum(axis=1) + rng.integers(-2, 3, (4, 1)).cumsum(axis=0)
    p.planes = [np.kron(base, np.ones((8, 8), dtype=np.int64)) * k]
    p.qpy = np.full((p.h4, p.w4), 45, dtype=np.int8)
    p.flg = all_edges(p)
    return p


def one_image_each(pics, **kw):
    images = []
    for k, p in enumerate(pics):
        p.image = k
        images.append(Image(p.out_x + p.out_w, p.out_y + p.out_h, **kw))
    return images


OFFSETS = ((0, 0), (6, 6), (-6, -6), (6, -6), (-6, 6))


def case_decisions():
    batches = []
    for bd in (8, 10, 12):
        pics = []
        for d in "VH":
            covered = set()
            for bo, to in OFFSETS:
                pics.append(steered_pic(f"steer{bd}{d}{bo}{to}", bd, bo, to, covered, transpose=d == "H"))
        pics.append(strong_everywhere(bd, f"strong{bd}"))
        rng = _rng(f"both{bd}")
        for j, (W, H) in enumerate(((32, 16), (48, 32))):  # both directions on wandering content
            p = Pic(W, H, bd_y=bd, beta_off=(0, 3)[j], tc_off=(0, -2)[j], name=f"both{bd}_{j}")
            p.planes, p.flg = blocky(rng, p, amp=1, step=4), all_edges(p)
            p.qpy = rand_qpy(rng, p, 24 - 6 * (bd - 8), 51)
            pics.append(p)
        batches.append(Batch(1 if bd == 8 else 2, 0, pics, one_image_each(pics), name=f"luma{bd}"))
    return Case("decisions", batches)


# ---------------------------------------------------------------- chroma
CHROMA_OFFSETS = ((-12, 12), (12, -12), (3, -4), (-7, 1))


def chroma_pics(tag, fmt, bd_y, bd_c):
    rng = _rng(tag)
    pics = []
    for k, (W, H) in enumerate(((48, 24), (96, 48), (128, 64), (96, 64), (40, 24), (32, 40))):
        j = k % 4  # 40x24, 32x40: a subsampled cw of 20, no multiple of 8, and of 16, one edge
        cb, cr = CHROMA_OFFSETS[j]
        p = Pic(W, H, fmt=fmt, bd_y=bd_y, bd_c=bd_c, cb_off=cb, cr_off=cr, tc_off=(0, 6, -6, 2)[j],
                beta_off=(0, -2, 3, 0)[j], name=f"{tag}_{k}")
        p.planes = blocky(rng, p, amp=(3, 6, 3, 6)[j], step=(10, 2, 40, 2)[j], lo=(100, 0, 100, 250)[j],
                          hi=(150, 4, 150, 255)[j])
        if j in (1, 3):  # chroma at 0 / at the maximum or up to forty 8-bit steps from it: Clip1 binds
            for c in (1, 2):
                r = rng.integers(0, 40 << (bd_c - 8), p.shape(c)) * rng.integers(0, 2, p.shape(c))
                p.planes[c] = r if j == 1 else (1 << bd_c) - 1 - r
        lo = -6 * (bd_y - 8)
        p.qpy = rand_qpy(rng, p, *((lo, 20), (36, 51), (18, 51), (24, 48))[j])
        # an edge flag per 4x4 block: along one edge a flagged block beside an unflagged one shows
        # how many chroma lines one luma block stands for
        p.flg = (all_edges(p) * (rng.integers(0, 4, (p.h4, p.w4)) > 0)).astype(np.uint8)
        pics.append(p)
    return pics


def case_chroma():
    batches = []
    for fmt in (1, 2, 3):
        p8 = chroma_pics(f"chroma{fmt}_8", fmt, 8, 8)
        batches.append(Batch(1, fmt, p8, one_image_each(p8), name=f"fmt{fmt}_8"))
        p16 = chroma_pics(f"chroma{fmt}_10", fmt, 10, 10) + chroma_pics(f"chroma{fmt}_mixed", fmt, 8, 10)[:2] \
            + chroma_pics(f"chroma{fmt}_mixed2", fmt, 12, 8)[2:3]
        batches.append(Batch(2, fmt, p16, one_image_each(p16), name=f"fmt{fmt}_16"))
    return Case("chroma", batches)


# ---------------------------------------------------------------- flags
def case_flags():
    batches = []
    for sz, fmt, bd in ((1, 0, 8), (1, 1, 8), (2, 1, 10), (2, 2, 10), (1, 3, 8)):
        rng = _rng(f"flags{sz}{fmt}")
        pics = []
        for j, (W, H) in enumerate(((48, 32), (32, 32), (32, 16), (32, 16))):
            # no-filter samples through both SAO paths: picture 0 behind a window offset (every load per
            # sample), picture 1 with a ragged row end behind aligned quads, picture 2 on unaligned planes
            ux, uy = smallest_conf(fmt)
            p = Pic(W, H, fmt=fmt, bd_y=bd, sao_luma=1, sao_chroma=1, conf_l=(ux, 0, 0, 0)[j], conf_t=(uy, 0, 0, 0)[j],
                    out_w=(W - ux - 1, W - 3, 0, 0)[j], skew=(0, 0, 1, 0)[j], name=f"flags{fmt}_{bd}_{j}")
            p.planes = blocky(rng, p, amp=1, step=3)
            p.qpy = rand_qpy(rng, p, 34, 48)
            # every block flagged for both directions: also off the 8x8 grid and along the left and top
            p.flg = np.full((p.h4, p.w4), MF_EDGE_V | MF_EDGE_H, dtype=np.uint8)
            p.flg |= (MF_NOFILT * (rng.integers(0, 3, (p.h4, p.w4)) == 0)).astype(np.uint8)
            p.sao = rand_sao(rng, p)
            force_types(p.sao, p.ncomp, 1 + (j & 1))
            pics.append(p)
        pics[2].dbk_disabled = 1
        pics[3].flags = PD_CHILD  # would be filtered and written out if it ran
        batches.append(Batch(sz, fmt, pics, one_image_each(pics), name=f"flags{fmt}_{bd}"))
    return Case("flags", batches)


# ---------------------------------------------------------------- SAO
def case_sao():
    batches = []
    sizes = {4: ((40, 24), (24, 40)), 5: ((72, 40), (40, 48)), 6: ((136, 72), (72, 24))}
    for fmt in (0, 1, 2, 3):
        for sz, bds in ((1, (8,)), (2, (10, 12))):
            rng = _rng(f"sao{fmt}{sz}")
            pics = []
            for bd in bds:
                for log2_ctb in (4, 5, 6):
                    for j, (W, H) in enumerate(sizes[log2_ctb]):
                        p = Pic(W, H, fmt=fmt, bd_y=bd, log2_ctb=log2_ctb, sao_luma=1, sao_chroma=int(fmt > 0),
                                dbk_disabled=1, out_w=W - 3 * j, name=f"sao{fmt}_{bd}_{log2_ctb}_{j}")
                        p.planes, p.sao = sao_content(rng, p), rand_sao(rng, p)
                        pics.append(p)
                for cls in range(4):  # one edge class on every CTB: all four borders, the corners, CTB seams
                    p = Pic(40, 24, fmt=fmt, bd_y=bd, sao_luma=1, sao_chroma=int(fmt > 0), dbk_disabled=1,
                            name=f"sao{fmt}_{bd}_class{cls}")
                    p.planes, p.sao = sao_content(rng, p), rand_sao(rng, p)
                    p.planes = [pl % 4 + 40 for pl in p.planes]  # four levels: every pair of signs, ties included
                    p.sao["type"], p.sao["band_eo"] = 2 * (np.arange(3) < p.ncomp), cls
                    pics.append(p)
                p = Pic(80, 48, fmt=fmt, bd_y=bd, sao_luma=1, sao_chroma=int(fmt > 0), dbk_disabled=1,
                        name=f"sao{fmt}_{bd}_bands")
                p.planes, p.sao = band_content(rng, p), rand_sao(rng, p)
                p.sao["type"] = 1 * (np.arange(3) < p.ncomp)  # band positions in turn, shifted per component
                turn = (np.arange(p.hctb)[:, None, None] * p.wctb + np.arange(p.wctb)[None, :, None] + np.arange(3))
                p.sao["band_eo"] = np.array(BAND_POSITIONS)[turn % len(BAND_POSITIONS)]
                pics.append(p)
            if sz == 2 and fmt:  # luma and chroma of different depths: the band shift and the clip per component
                for bd_y, bd_c in ((10, 12), (12, 10)):
                    for kind in ("bands", "levels"):
                        p = Pic(48, 32, fmt=fmt, bd_y=bd_y, bd_c=bd_c, sao_luma=1, sao_chroma=1, dbk_disabled=1,
                                name=f"sao{fmt}_mixed{bd_y}_{bd_c}_{kind}")
                        p.planes = band_content(rng, p) if kind == "bands" else sao_content(rng, p)
                        p.sao = rand_sao(rng, p)
                        pics.append(p)
            # luma only, chroma only, neither (the copy path), and one behind a running deblocking
            for j, (lu, chroma, dbk_off) in enumerate(((1, 0, 1), (0, 1, 1), (0, 0, 1), (1, 1, 0))):
                if fmt == 0 and not lu and j == 1:
                    continue
                p = Pic(40, 24, fmt=fmt, bd_y=bds[-1], sao_luma=lu, sao_chroma=chroma if fmt else 0,
                        dbk_disabled=dbk_off, name=f"sao{fmt}_{bds[-1]}_flags{j}")
                p.planes, p.sao = sao_content(rng, p), rand_sao(rng, p, luma=bool(lu), chroma=bool(chroma))
                if not dbk_off:
                    p.planes, p.flg, p.qpy = blocky(rng, p, amp=1, step=3), all_edges(p), rand_qpy(rng, p, 36, 48)
                pics.append(p)
            batches.append(Batch(sz, fmt, pics, one_image_each(pics), name=f"sao{fmt}_{sz}"))
    return Case("sao", batches)


# ---------------------------------------------------------------- placement
def smallest_conf(fmt):
    """the smallest non-zero conformance window offsets in luma samples (SubWidthC, SubHeightC units)"""
    sx, sy = ref.subsampling(fmt)
    return 1 << sx, 1 << sy


def case_placement():
    batches = []
    for sz, bd in ((1, 8), (2, 10)):
        for fmt in (1, 2, 3, 0):
            rng = _rng(f"place{sz}{fmt}")
            ux, uy = smallest_conf(fmt)
            base = Pic(32, 16, fmt=fmt, bd_y=bd, sao_luma=1, sao_chroma=int(fmt > 0))
            planes, params = sao_content(rng, base), rand_sao(rng, base)
            force_types(params, base.ncomp, 2)

            def pic(**kw):
                p = Pic(32, 16, fmt=fmt, bd_y=bd, sao_luma=1, sao_chroma=int(fmt > 0), dbk_disabled=1, **kw)
                p.planes, p.sao = planes, params
                return p
            pics, images = [], []
            k = 0
            for cl, ct in ((0, 0), (ux, uy), (4 + ux, 4 + uy), (8, 4)):
                for mod in range(4):
                    p = pic(conf_l=cl, conf_t=ct, out_w=20 + mod, out_h=9 + (mod & 1), image=len(images),
                            out_x=(0, 2 * ux, 4, 3 * ux)[(k + mod) % 4], out_y=(0, uy, 3 * uy)[k % 3],
                            skew=(0, 1, 3, 4)[(k // 2) % 4] if mod == 3 else 0, name=f"conf{cl}_{ct}_w{20 + mod}")
                    images.append(Image(p.out_x + p.out_w, p.out_y + p.out_h, skew=(0, 1, 3, 0)[(k + mod) % 4],
                                        pad=(0, 1, 2, 3)[(k + 2 * mod + 1) % 4]))
                    pics.append(p)
                k += 1
            # one image of 40x12: two pictures side by side, the second clipped by the image's width and
            # height, a third and a fourth wholly outside it
            shared = len(images)
            images.append(Image(40, 12, skew=1, pad=1))
            pics += [pic(out_w=24, out_h=10, image=shared, name="left"),
                     pic(out_w=24, out_h=14, image=shared, out_x=24, out_y=2, name="clipped"),
                     pic(out_w=24, out_h=10, image=shared, out_x=40, out_y=0, name="outside_x"),
                     pic(out_w=24, out_h=10, image=shared, out_x=0, out_y=12, name="outside_y")]
            off = pic(out_w=23, out_h=11, image=len(images), out_x=2 * ux, name="sao_off")  # the copy path
            off.sao_luma = off.sao_chroma = 0
            off.sao = np.zeros_like(params)
            images.append(Image(off.out_x + 23, 11, skew=3, pad=3))
            pics.append(off)
            batches.append(Batch(sz, fmt, pics, images, name=f"place{fmt}_{sz}"))
    return Case("placement", batches)


# ---------------------------------------------------------------- dispatch
DISPATCH_SIZES = ((32, 16), (48, 24), (64, 40), (272, 16), (136, 24), (1040, 520))


def case_dispatch():
    batches = []
    for sz, fmt, bd, sizes in ((1, 1, 8, DISPATCH_SIZES), (2, 3, 10, DISPATCH_SIZES[:5])):
        rng = _rng(f"dispatch{sz}")
        pics = []
        for j, (W, H) in enumerate(((32, 16), (40, 24)) + sizes):  # the first two lie before pic0
            p = Pic(W, H, fmt=fmt, bd_y=bd, log2_ctb=(4, 5, 6)[j % 3], sao_luma=1, sao_chroma=1, cb_off=2, cr_off=-3,
                    conf_l=(0, 4)[j & 1], out_w=W - (0, 7)[j & 1], name=f"dispatch{W}x{H}")
            p.planes, p.flg = blocky(rng, p, amp=1, step=4), all_edges(p)
            p.qpy, p.sao = rand_qpy(rng, p, 30, 48), rand_sao(rng, p)
            pics.append(p)
        batches.append(Batch(sz, fmt, pics, one_image_each(pics, pad=1), pic0=2, name=f"dispatch{sz}"))
    return Case("dispatch", batches)


# ---------------------------------------------------------------- assembly
def case_assembly():
    batches = []
    for sz, fmt, bd in ((1, 1, 8), (2, 2, 10)):
        rng = _rng(f"assembly{sz}")
        kids = []
        for j, (W, H, ox, oy) in enumerate(((32, 48, 0, 0), (32, 32, 32, 0), (32, 16, 32, 32))):
            p = Pic(W, H, fmt=fmt, bd_y=bd, flags=PD_CHILD, org_x=ox, org_y=oy, sao_luma=int(j < 2),
                    sao_chroma=int(j == 0), cb_off=1, cr_off=-2, name=f"child{j}")
            p.planes, p.flg = blocky(rng, p, amp=1, step=3), all_edges(p)
            # a child's own left and top are picture borders to its parse but seams of the assembly
            p.flg[:, 0] |= MF_EDGE_V
            p.flg[0, :] |= MF_EDGE_H
            p.qpy = rand_qpy(rng, p, 34, 48)
            # a component whose flag is off carries type 0; child 2, SAO off altogether, wrote nothing: garbage
            p.sao = rand_sao(rng, p, luma=True, chroma=j != 1)
            kids.append(p)
        asm = Pic(64, 48, fmt=fmt, bd_y=bd, flags=PD_ASSEMBLY, children=(1, 2, 3), sao_luma=1, sao_chroma=1, cb_off=1,
                  cr_off=-2, conf_t=0, out_w=61, out_h=47, image=0, name="assembly")
        asm.planes = [rng.integers(0, 1 << bd, asm.shape(c)) for c in range(3)]   # all of it is overwritten
        asm.qpy = rng.integers(0, 50, (asm.h4, asm.w4)).astype(np.int8)
        asm.flg = rng.integers(0, 8, (asm.h4, asm.w4)).astype(np.uint8)
        asm.sao = rand_sao(rng, asm)
        plain = Pic(32, 16, fmt=fmt, bd_y=bd, sao_luma=1, sao_chroma=1, image=1, name="plain")
        plain.planes, plain.flg = blocky(rng, plain, amp=1, step=3), all_edges(plain)
        plain.qpy, plain.sao = rand_qpy(rng, plain, 34, 48), rand_sao(rng, plain)
        pics = [plain] + kids + [asm]
        batches.append(Batch(sz, fmt, pics, [Image(61, 47, pad=3), Image(32, 16)], name=f"assembly{sz}"))
    return Case("assembly", batches)


CASES = {"decisions": case_decisions, "chroma": case_chroma, "flags": case_flags, "sao": case_sao,
         "placement": case_placement, "dispatch": case_dispatch, "assembly": case_assembly}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()
