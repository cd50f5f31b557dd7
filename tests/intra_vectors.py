"""Hand-built inputs of k_intra and what tests/intra_ref.py makes of them.

Pictures are described as quadtrees of transform units and written in the
product's own structs (SeqParams, PicDesc, per-row TU counts, TuRec, residual
planes) as the case file tests/intra/intra_driver.cpp reads.  Two facts about
the kernel shape them: a CTU that any record opens is written back whole, so
every such CTU is tiled completely by records of every component, in z-order,
luma then Cb then Cr per TU as the parse writes them; and neighbour samples are
planted exactly with PCM records (prediction 0, reconstruction = residual),
which is how a threshold is hit on the nose.
"""
import dataclasses
import functools
import struct

import numpy as np

import intra_ref as ref
from xform_vectors import (MIRRORS, PD_ASSEMBLY, PIC_DTYPE, SEQ_DTYPE, TU_BYPASS, TU_CBF, TU_CIDX_MASK, TU_DTYPE,
                           TU_PCM, hash_str)

SENTINEL = 0xAA
MAGIC = 0x31435049
SP_STRONG_INTRA = 64
CONSTANTS = {"SP_STRONG_INTRA": SP_STRONG_INTRA, "PD_ASSEMBLY": PD_ASSEMBLY, "TU_CIDX_MASK": TU_CIDX_MASK,
             "TU_CBF": TU_CBF, "TU_BYPASS": TU_BYPASS, "TU_PCM": TU_PCM}


def layout_of_mirrors():
    """{name: value} in the form `intra_driver --layout` prints."""
    out = dict(CONSTANTS)
    for name, dt in MIRRORS.items():
        out[name] = dt.itemsize
        for f in dt.names:
            out[f"{name}.{f}"] = dt.fields[f][1]
    return out


def _rng(tag):
    return np.random.default_rng(hash_str(tag))


# ---------------------------------------------------------------- pictures
@dataclasses.dataclass
class VTB(ref.TB):
    tag: str = ""
    ctu: int = 0
    res: object = None   # None: the picture's random residual; else a scalar or an n x n array
    tu: tuple = ()       # (x, y, log2) of the luma node the TB came from


def tile(g, split, stop_at=None):
    """The picture's TBs per CTB row: the quadtree in z-order, a node split while
    it crosses the picture's edge, is larger than 32 or split(x, y, log2) says
    so; an 8x8 node that splits becomes four 4x4 luma TBs with the chroma of the
    8x8 (4:4:4: chroma with each).  stop_at = (row, ctu): that row ends before
    that CTU."""
    cf = g.chroma_format
    rows = []

    def chroma(out, x, y, log2, c):
        if cf == 1:
            for k in (1, 2):
                out.append(VTB(k, x // 2, y // 2, log2 - 1, 0, ctu=c, tu=(x, y, log2)))
        elif cf == 2:
            h = 1 << (log2 - 1)
            for k in (1, 2):
                out.append(VTB(k, x // 2, y, log2 - 1, 0, ctu=c, tu=(x, y, log2)))
                out.append(VTB(k, x // 2, y + h, log2 - 1, 0, ctu=c, tu=(x, y, log2)))
        elif cf == 3:
            for k in (1, 2):
                out.append(VTB(k, x, y, log2, 0, ctu=c, tu=(x, y, log2)))

    def node(out, x, y, log2, c):
        n = 1 << log2
        if x >= g.W or y >= g.H:
            return
        if x + n > g.W or y + n > g.H or log2 > 5 or (log2 >= 3 and split(x, y, log2)):
            h = n // 2
            if log2 == 3:
                for dy, dx in ((0, 0), (0, 4), (4, 0), (4, 4)):
                    out.append(VTB(0, x + dx, y + dy, 2, 0, ctu=c, tu=(x + dx, y + dy, 2)))
                    if cf == 3:
                        chroma(out, x + dx, y + dy, 2, c)
                if cf in (1, 2):
                    chroma(out, x, y, 3, c)
                return
            for dy, dx in ((0, 0), (0, h), (h, 0), (h, h)):
                node(out, x + dx, y + dy, log2 - 1, c)
            return
        out.append(VTB(0, x, y, log2, 0, ctu=c, tu=(x, y, log2)))
        chroma(out, x, y, log2, c)

    ctb = 1 << g.log2_ctb
    for r in range(-(-g.H // ctb)):
        out = []
        for c in range(-(-g.W // ctb)):
            if stop_at == (r, c):
                break
            node(out, c * ctb, r * ctb, g.log2_ctb, c)
        rows.append(out)
    return rows


def uniform(log2):
    return lambda x, y, l: l > log2


def random_tree(tag, p=(0.0, 0.0, 0.0, 0.45, 0.55, 0.7, 1.0)):
    """split with probability p[log2], from a hash of the node"""
    return lambda x, y, l: (hash_str(f"{tag}/{x}/{y}/{l}") % 1000) < 1000 * p[l]


class Pic:
    """One picture: geometry, quadtree, and how each TB is coded.

    style(tb) sets mode / cbf / pcm / res / tag of a TB (the default: a mode
    drawn per TU and shared by its Cb and Cr TBs, cbf on half of them, a small
    random residual).  plant(pic) then edits `want`, the planes whose samples
    the PCM TBs carry.  mangle(r, recs) edits a row's packed records (dicts)."""

    def __init__(self, name, g, split, style=None, plant=None, mangle=None, flags=0, launched=True, stop_at=None,
                 res_amp=24):
        self.name, self.g, self.flags, self.launched, self.mangle = name, g, flags, launched, mangle
        rng = _rng(name)
        self.rows = tile(g, split, stop_at)
        self.tbs = [t for row in self.rows for t in row]
        bds = [g.bd_y, g.bd_c, g.bd_c][:g.ncomp]
        self.want = [rng.integers(0, 1 << bd, size=g.plane(k)[::-1]) for k, bd in enumerate(bds)]
        self.resid = [rng.integers(-res_amp, res_amp + 1, size=g.plane(k)[::-1]) for k in range(g.ncomp)]
        for t in self.tbs:
            h = hash_str(f"{name}/{t.tu}")
            t.mode = (h // 35) % 35 if t.cidx else h % 35
            t.cbf = bool((hash_str(f"{name}/{t.tu}/{t.cidx}/{t.x}/{t.y}") >> 9) & 1)
            if style:
                style(t)
        if plant:
            plant(self)
        for t in self.tbs:
            n = 1 << t.log2
            if t.pcm:
                t.cbf = True
                self.resid[t.cidx][t.y:t.y + n, t.x:t.x + n] = self.want[t.cidx][t.y:t.y + n, t.x:t.x + n]
            elif t.res is not None:
                self.resid[t.cidx][t.y:t.y + n, t.x:t.x + n] = t.res
        self.live = launched and not (flags & PD_ASSEMBLY)
        if self.live:
            self.planes, self.infos, self.agree = ref.predict_picture(g, self.tbs, self.resid, fill=-1)
        else:
            self.planes, self.infos, self.agree = None, [], True

    def records(self, r):
        recs = [dict(x=t.x, y=t.y, log2=t.log2, mode=t.mode, ctu=t.ctu,
                     flags=t.cidx | (TU_CBF if t.cbf else 0) | ((TU_PCM | TU_BYPASS) if t.pcm else 0))
                for t in self.rows[r]]
        return self.mangle(r, recs) if self.mangle else recs


@dataclasses.dataclass
class Batch:
    pics: list
    pic0: int = 0

    def __post_init__(self):
        gs = [p.g for p in self.pics]
        assert len({g.chroma_format for g in gs}) == 1
        self.chroma_format = gs[0].chroma_format
        self.bps = 2 if max(gs[0].bd_y, gs[0].bd_c) > 8 else 1
        assert all((min(g.bd_y, g.bd_c) > 8) == (max(g.bd_y, g.bd_c) > 8) == (self.bps == 2) for g in gs)
        self._build()

    def _build(self):
        pics, bps = self.pics, self.bps
        seq_arr = np.zeros(len(pics), dtype=SEQ_DTYPE)
        pic_arr = np.zeros(len(pics), dtype=PIC_DTYPE)
        row_words, tus_all, n_tus = [7, 7], [np.zeros(3, dtype=TU_DTYPE)], 3
        resid_all, resid_at = [np.full(40, 0x5555, dtype=np.int64)], 40
        recon_at, expected = 256, [np.full(256, SENTINEL, dtype=np.uint8)]
        self.where = []  # (pic index, byte offset of the picture's samples)
        launched = [p for p in pics[self.pic0:] if not (p.flags & PD_ASSEMBLY)]
        for i, p in enumerate(pics):
            g, a = p.g, seq_arr[i]
            a["width"], a["height"], a["log2_ctb"], a["chroma_format"] = g.W, g.H, g.log2_ctb, g.chroma_format
            a["bit_depth_y"], a["bit_depth_c"] = g.bd_y, g.bd_c
            a["log2_min_cb"], a["log2_min_tb"], a["log2_max_tb"] = 3, g.log2_min_tb, 5
            a["out_w"], a["out_h"] = g.W, g.H
            a["flags"] = SP_STRONG_INTRA if g.strong else 0
            nrows = len(p.rows)
            recs = [p.records(r) for r in range(nrows)]
            cap = max(len(x) for x in recs) + 2
            pd = pic_arr[i]
            pd["seq"], pd["flags"], pd["recon_off"], pd["resid_off"] = i, p.flags, recon_at, resid_at
            pd["tu_off"], pd["row_off"], pd["tu_cap_row"] = n_tus, len(row_words) // 2, cap
            for rr in recs:
                arr = np.zeros(cap, dtype=TU_DTYPE)
                for k, q in enumerate(rr):
                    for f in ("x", "y", "log2", "mode", "ctu", "flags"):
                        arr[k][f] = q[f]
                arr["qp"] = 26
                tus_all.append(arr)
                row_words += [len(rr), 0]
            n_tus += nrows * cap
            res = np.concatenate([x.reshape(-1) for x in p.resid])
            resid_all += [res, np.full(24, 0x5555, dtype=np.int64)]
            resid_at += len(res) + 24
            live = p.live and i >= self.pic0
            if live:
                flat = np.concatenate([x.reshape(-1) for x in p.planes])
                sent = SENTINEL | (SENTINEL << 8) if bps == 2 else SENTINEL
                flat = np.where(flat < 0, sent, flat)
                buf = flat.astype("<u2" if bps == 2 else np.uint8).view(np.uint8)
            else:
                buf = np.full(len(res) * bps, SENTINEL, dtype=np.uint8)
            self.where.append((i, recon_at))
            pad = (-len(buf)) % 256 + 256
            expected += [buf, np.full(pad, SENTINEL, dtype=np.uint8)]
            recon_at += len(buf) + pad
        self.expected = np.concatenate(expected)
        self.expected.setflags(write=False)
        assert len(self.expected) == recon_at
        rows_arr = np.array(row_words + [9, 9], dtype=np.uint32)
        tus = np.concatenate(tus_all)
        resid = np.concatenate(resid_all).astype(np.int16)
        max_rows = max(len(p.rows) for p in launched)
        max_log2ctb = max(p.g.log2_ctb for p in pics)
        head = struct.pack("<16I", len(pics), len(pics), self.pic0, len(pics) - self.pic0, max_rows, len(rows_arr),
                           len(tus), len(resid), recon_at, bps, self.chroma_format, max_log2ctb, SENTINEL, 0, 0, 0)
        self.blob = b"".join([head, seq_arr.tobytes(), pic_arr.tobytes(), rows_arr.tobytes(), tus.tobytes(),
                              resid.tobytes()])
        self.out_bytes = recon_at + 4 * len(pics)

    def failures(self, got):
        """Where the arena differs from the model, by picture, component and TB; then the status words."""
        arena, status = got[:len(self.expected)], got[len(self.expected):].view("<u4")
        out = []
        bad = arena != self.expected
        if bad.any():
            rest = bad.copy()
            for i, at in self.where:
                p = self.pics[i]
                g = p.g
                for k in range(g.ncomp):
                    w, h = g.plane(k)
                    nb = w * h * self.bps
                    b = bad[at:at + nb].reshape(h, w * self.bps)
                    rest[at:at + nb] = False
                    if b.any():
                        y, xb = (int(v) for v in np.argwhere(b)[0])
                        x = xb // self.bps
                        view = lambda a: a[at:at + nb].view("<u2" if self.bps == 2 else np.uint8).reshape(h, w)
                        tb = [t for t in p.tbs if t.cidx == k and t.x <= x < t.x + (1 << t.log2)
                              and t.y <= y < t.y + (1 << t.log2)]
                        what = (f"TB {tb[0].tag or '-'} at ({tb[0].x}, {tb[0].y}) n {1 << tb[0].log2} mode {tb[0].mode}"
                                f" cbf {int(tb[0].cbf)} pcm {int(tb[0].pcm)}") if tb else "no TB"
                        out.append(f"{p.name} c{k}: {int(b.sum()) // self.bps}+ samples differ, first at (x={x}, y={y}): "
                                   f"got {view(arena)[y, x]}, expected {view(self.expected)[y, x]}; {what}")
                    at += nb
            if rest.any():
                first = int(np.flatnonzero(rest)[0])
                out.append(f"{int(rest.sum())} bytes between the pictures lost the sentinel, first at {first}")
        for i, s in enumerate(status):
            if s:
                out.append(f"{self.pics[i].name}: status {int(s):#x}")
        return out


class Case:
    def __init__(self, name, batches):
        self.name, self.batches = name, batches
        self.blob = struct.pack("<2I", MAGIC, len(batches)) + b"".join(b.blob for b in batches)

    @property
    def pics(self):
        return [p for b in self.batches for p in b.pics]

    @property
    def has_chroma(self):
        return any(b.chroma_format for b in self.batches)

    def failures(self, got):
        got = np.asarray(got, dtype=np.uint8)
        assert len(got) == sum(b.out_bytes for b in self.batches), "result file size"
        out, at = [], 0
        for b in self.batches:
            out += b.failures(got[at:at + b.out_bytes])
            at += b.out_bytes
        return out


def batches_of(pics):
    """one batch per (chroma format, sample size), in order of first appearance"""
    groups = {}
    for p in pics:
        groups.setdefault((p.g.chroma_format, max(p.g.bd_y, p.g.bd_c) > 8), []).append(p)
    return [Batch(v) for v in groups.values()]


# ---------------------------------------------------------------- helpers of the cases
def pattern(info, n):
    """(left, below-left, above, above-right): each 'none', 'all' or 'part'"""
    a = info.avail

    def cls(v):
        return "all" if v.all() else ("part" if v.any() else "none")
    return cls(a[n:2 * n]), cls(a[0:n]), cls(a[2 * n + 1:3 * n + 1]), cls(a[3 * n + 1:4 * n + 1])


def substitution_arms(avail, chunk=64):
    """The arms of the chunked substitution a TB's availability drives: for each
    unavailable search position, where its value comes from, by chunk of search
    positions (64 a wave, 32 a half-wave of a Cb / Cr pair)."""
    arms = set()
    idx = np.flatnonzero(avail)
    if len(idx) == 0:
        return {"no_sample"}
    for s in np.flatnonzero(~avail):
        before = idx[idx < s]
        if len(before):
            arms.add("same_chunk" if before[-1] // chunk == s // chunk else "earlier_chunk")
        else:
            arms.add("first_same_chunk" if idx[0] // chunk == s // chunk else "first_later_chunk")
    return arms


def neighbour_positions(pic, t):
    """the TB's neighbour positions inside its plane"""
    n = 1 << t.log2
    w, h = pic.g.plane(t.cidx)
    return [(t.x + dx, t.y + dy) for dx, dy in ref.search_positions(n) if 0 <= t.x + dx < w and 0 <= t.y + dy < h]


def plant_distinct(pic, probes, rng):
    """pairwise distinct pseudo-random values on each probe's neighbours: first the
    positions two probes share (the corners between CTUs), distinct among themselves,
    then each probe's own"""
    for k in range(pic.g.ncomp):
        mine = [t for t in probes if t.cidx == k]
        bd = pic.g.bd_c if k else pic.g.bd_y
        count = {}
        for t in mine:
            for q in neighbour_positions(pic, t):
                count[q] = count.get(q, 0) + 1
        shared = [q for q, c in count.items() if c > 1]
        assert len(shared) + max((4 << t.log2) + 1 for t in mine) <= 1 << bd if mine else True
        pool = [int(v) for v in rng.permutation(1 << bd)]
        taken = {q: pool.pop() for q in shared}
        for t in mine:
            pos = neighbour_positions(pic, t)
            free = [v for v in rng.permutation(pool)]
            for q in pos:
                if q not in taken:
                    taken[q] = int(free.pop())
        for (x, y), v in taken.items():
            pic.want[k][y, x] = v


def covering_pcm(pic, t):
    """every neighbour of t lies in a PCM TB (so what plant() wrote is what t reads)"""
    pcm = np.zeros(pic.g.plane(t.cidx)[::-1], dtype=bool)
    for o in pic.tbs:
        if o.cidx == t.cidx and o.pcm:
            pcm[o.y:o.y + (1 << o.log2), o.x:o.x + (1 << o.log2)] = True
    return all(pcm[y, x] for x, y in neighbour_positions(pic, t))


def probe_pic(name, g, n, probe_of, plant_probe=None, **kw):
    """A picture of PCM TBs with one probe TU of luma size n at the origin of CTU
    (r, c) wherever probe_of(r, c) returns a dict of TB attributes per cidx class
    ({0: {...}, 1: {...}}; Cb and Cr share class 1).  CTB = 2n or more, so a probe
    in row >= 1 and column >= 1 has all five neighbour groups."""
    ctb, log2n = 1 << g.log2_ctb, n.bit_length() - 1

    def at_origin(x, y):
        return x % ctb == 0 and y % ctb == 0 and probe_of(y // ctb, x // ctb) is not None

    def split(x, y, l):
        return l > log2n and at_origin(x, y)

    probes = []

    def style(t):
        x, y, l = t.tu
        first = t.cidx == 0 or (t.x * g.sub_w == x and t.y * g.sub_h == y)  # (4:2:2: the upper chroma TB)
        if n == 4 and t.cidx and g.chroma_format in (1, 2):  # the chroma of the 8x8 around the four 4x4s
            l = 2
        if at_origin(x, y) and l == log2n and first:
            attrs = probe_of(y // ctb, x // ctb).get(1 if t.cidx else 0)
            if attrs is not None:
                t.pcm = False
                t.tag = f"{name}/r{y // ctb}c{x // ctb}/c{t.cidx}n{1 << t.log2}"
                for k, v in attrs.items():
                    setattr(t, k, v)
                probes.append(t)
                return
        t.pcm = True

    def plant(pic):
        rng = _rng(name + "/plant")
        plant_distinct(pic, probes, rng)
        if plant_probe:
            for t in probes:
                plant_probe(pic, t)
        for t in probes:
            assert covering_pcm(pic, t), t.tag

    return Pic(name, g, split, style, plant, **kw)


# ---------------------------------------------------------------- the cases
def _modes_pics(cf, bd, tag):
    pics = []
    for n, log2ctb, (W, H) in ((4, 4, (128, 128)), (8, 4, (128, 128)), (16, 5, (256, 192)), (32, 6, (256, 192))):
        ctb = 1 << log2ctb
        inner = [(r, c) for r in range(1, H // ctb) for c in range(1, W // ctb)]
        for k0 in range(0, 35, len(inner)):
            slot = {rc: k0 + i for i, rc in enumerate(inner) if k0 + i < 35}

            def probe_of(r, c, slot=slot):
                if (r, c) not in slot:
                    return None
                k = slot[(r, c)]
                mc = (k + 17) % 35  # (DC without a residual: the edge filter, or its absence, is the sample)
                return {0: dict(mode=k, cbf=bool(k & 1) and k != 1), 1: dict(mode=mc, cbf=bool(k & 2) and mc != 1)}
            g = ref.Geom(W, H, cf, bd, bd, log2ctb, 2 if n == 4 else 3, strong=False)
            pics.append(probe_pic(f"{tag}/n{n}/m{k0}", g, n, probe_of))
    return pics


def case_modes():
    """Every mode at every TB size of every component class and format, all five
    neighbour groups available and pairwise distinct."""
    return Case("modes", batches_of(_modes_pics(1, 8, "modes/420") + _modes_pics(2, 10, "modes/422")
                                    + _modes_pics(3, 8, "modes/444")))


# 72 x 40, 88 x 40, 72 x 72: the bottom and right edges cut below-left and above-right part-way;
# 80 x 72: a 16x16 TB in the last column beside a 32x32 one; 192 x 128: a 64 CTB with all its
# neighbours; 8, 16, 32, 64 wide: a TB as wide as the picture, whose above-right lies outside
AVAIL_SIZES = ((72, 40), (88, 40), (72, 72), (80, 72), (192, 128), (8, 40), (16, 40), (32, 72), (64, 72))


def _avail_pics(cf, bd, tag):
    pics = []
    for W, H in AVAIL_SIZES:
        for log2ctb in (4, 5, 6):
            for kind in ("u2", "u3", "u4", "u5", "rnd"):
                if kind != "rnd" and int(kind[1]) > log2ctb:
                    continue
                name = f"{tag}/{W}x{H}/ctb{1 << log2ctb}/{kind}"
                split = random_tree(name) if kind == "rnd" else uniform(int(kind[1]))
                min_tb = 2 if kind in ("u2", "rnd") else min(int(kind[1]), 3)
                g = ref.Geom(W, H, cf, bd, bd, log2ctb, min_tb)

                def style(t):
                    t.tag = f"c{t.cidx}n{1 << t.log2}@{t.x},{t.y}"
                pics.append(Pic(name, g, split, style))
    return pics


def case_availability():
    """Every reachable pattern of (left, below-left, above, above-right) for every
    TB size, by each of its causes, on pictures whose edges cut the groups part-way."""
    return Case("availability", batches_of(_avail_pics(1, 8, "avail/420")))


def _strong_plant(top, left):
    """plant p[-1][-1], p[31] and p[63] on both sides of a 32x32 probe so that the top
    expression of biIntFlag is `top` and the left one `left`"""
    def plant(pic, t):
        if t.log2 != 5:
            return
        w = pic.want[t.cidx]
        hi = (1 << (pic.g.bd_c if t.cidx else pic.g.bd_y)) - 1
        c = hi // 2 + 3
        w[t.y - 1, t.x - 1] = c
        for val, (dx, dy) in ((top, (1, 0)), (left, (0, 1))):
            m = hi // 2 + (7 if dx else -9)
            w[t.y - 1 + dy * 32, t.x - 1 + dx * 32] = m
            w[t.y - 1 + dy * 64, t.x - 1 + dx * 64] = 2 * m - c + (val if dx else -val)
    return plant


def case_filter():
    """The strong-smoothing decision with planted neighbours: each expression at
    threshold - 1 and at the threshold while the other passes, at 8 and 10 bits,
    the flag on and off; a 4:4:4 chroma 32x32 TB that passes both."""
    pics = []
    for bd in (8, 10):
        thr = 1 << (bd - 5)
        for k, (top, left) in enumerate(((thr - 1, thr - 1), (thr, thr - 1), (thr - 1, thr), (0, 0))):
            for strong in (True, False):
                g = ref.Geom(128, 128, 1, bd, bd, 6, 3, strong=strong)
                mode = (0, 2, 34, 18)[k]
                probe_of = lambda r, c, mode=mode: {0: dict(mode=mode, cbf=False), 1: dict(cbf=True)} \
                    if (r, c) == (1, 1) else None
                pics.append(probe_pic(f"filter/bd{bd}/top{top}_left{left}/strong{int(strong)}", g, 32, probe_of,
                                      _strong_plant(top, left)))
    for bd in (8, 10):
        g = ref.Geom(128, 128, 3, bd, bd, 6, 3, strong=True)
        probe_of = lambda r, c: {0: dict(mode=0, cbf=False), 1: dict(mode=0, cbf=False)} if (r, c) == (1, 1) else None
        pics.append(probe_pic(f"filter/444/bd{bd}", g, 32, probe_of, _strong_plant(0, 0)))
    return Case("filter", batches_of(pics))


def _edge_plant(kind, bd):
    """neighbours that drive the mode 26 / 10 boundary filter below 0 ('lo') or above the
    maximum ('hi') on two samples of three, and inside the range on the third"""
    def plant(pic, t):
        if t.cidx or t.mode not in (10, 26):
            return
        w, n, hi = pic.want[0], 1 << t.log2, (1 << bd) - 1
        # mode 26: p[0][-1] + ((p[-1][y] - p[-1][-1]) >> 1); mode 10: the transpose
        along = [(t.x - 1, t.y + i) for i in range(n)] if t.mode == 26 else [(t.x + i, t.y - 1) for i in range(n)]
        base = (t.x, t.y - 1) if t.mode == 26 else (t.x - 1, t.y)
        corner = (t.x - 1, t.y - 1)
        w[base[1], base[0]] = 3 if kind == "lo" else hi - 3
        w[corner[1], corner[0]] = hi - 5 if kind == "lo" else 5
        for i, (x, y) in enumerate(along):
            if (x, y) == base:
                continue
            if i % 3 == 1:
                w[y, x] = hi if kind == "lo" else 0   # 3 + (5 >> 1), hi - 3 + (-5 >> 1): inside
            else:
                w[y, x] = i if kind == "lo" else hi - i
    return plant


def case_edges():
    """The DC / mode 26 / mode 10 edge filters and their Clip1, Clip1(pred + res)
    both ways, and a picture whose luma and chroma depths differ."""
    pics = []
    for bd in (8, 10):
        hi = (1 << bd) - 1
        for n, log2ctb in ((4, 4), (8, 4), (16, 5), (32, 6)):
            ctb = 1 << log2ctb
            W, H = 4 * ctb, 3 * ctb
            for kind in ("lo", "hi"):
                def probe_of(r, c, kind=kind, n=n, hi=hi):
                    if r < 1 or c < 1:
                        return None
                    mode = (10, 26, 1)[(c - 1) % 3]
                    # row 2: a residual that brings a boundary sample the filter's Clip1 bound back inside the
                    # range (without that Clip1 another sample), and on every other sample one that makes
                    # Clip1(pred + res) bind
                    sgn = 1 if kind == "hi" else -1
                    yy, xx = np.mgrid[0:n, 0:n]
                    res = None if r == 1 else np.where((xx + yy) & 1, sgn * hi, -sgn * (hi // 3))
                    # chroma: the same modes, where no edge filter may run
                    return {0: dict(mode=mode, cbf=res is not None, res=res), 1: dict(mode=mode, cbf=c == 2, res=None)}
                g = ref.Geom(W, H, 3 if n == 8 else 1, bd, bd, log2ctb, 2 if n == 4 else 3)
                pics.append(probe_pic(f"edges/bd{bd}/n{n}/{kind}", g, n, probe_of, _edge_plant(kind, bd)))
    # luma and chroma depths differ: the default value of the nothing-available TB, the clip
    # and the strong threshold each from the right depth
    for bdy, bdc in ((10, 12), (12, 10)):
        thr = 1 << (bdy - 5)
        for top in (thr - 1, thr):
            g = ref.Geom(128, 128, 3, bdy, bdc, 6, 3, strong=True)

            def probe_of(r, c, bdy=bdy, bdc=bdc):
                if (r, c) == (0, 0):  # nothing available: 1 << (bd - 1) everywhere
                    return {0: dict(mode=1, cbf=False), 1: dict(mode=26, cbf=False)}
                if (r, c) == (1, 1):
                    return {0: dict(mode=0, cbf=True, res=(1 << bdy)), 1: dict(mode=0, cbf=True, res=-(1 << bdc))}
                if (r, c) == (0, 1):
                    return {0: dict(mode=2, cbf=True, res=-(1 << bdy)), 1: dict(mode=2, cbf=True, res=(1 << bdc) - 200)}
                return {0: dict(mode=0, cbf=False), 1: dict(mode=34, cbf=False)}
            pics.append(probe_pic(f"edges/bd{bdy}_{bdc}/top{top}", g, 32, probe_of, None))
            pics.append(probe_pic(f"edges/bd{bdy}_{bdc}/strong_top{top}", g, 32,
                                  lambda r, c: {0: dict(mode=0, cbf=False), 1: dict(mode=0, cbf=False)}
                                  if (r, c) == (1, 1) else None, _strong_plant(top, thr - 1)))
        # ... and in 4:2:0, where Cb / Cr pairs take the chroma depth: residuals large enough to clip
        name = f"edges/bd{bdy}_{bdc}/420"
        pics.append(Pic(name, ref.Geom(72, 72, 1, bdy, bdc, 5, 2), random_tree(name), res_amp=1 << max(bdy, bdc)))
    return Case("edges", batches_of(pics))


def formed_pairs(recs):
    """Indices of the Cb records the walk predicts together with their Cr record: a 4x4 or
    8x8 Cb TB whose next record is the Cr TB of the same position, size, mode and CTU, not
    in lane 63 of its 64-record block (4:2:0 only)."""
    out = []
    for i in range(len(recs) - 1):
        a, b = recs[i], recs[i + 1]
        if (a["flags"] & 3) == 1 and a["log2"] <= 3 and (b["flags"] & 3) == 2 and i % 64 != 63 and all(
                a[f] == b[f] for f in ("x", "y", "log2", "mode", "ctu")):
            out.append(i)
    return out


def case_pairs():
    """4:2:0 Cb / Cr pairs of 4x4 and 8x8 TBs across all modes, availability patterns and
    cbf / PCM combinations, and the pairs the walk must not form."""
    pics = []
    for bd in (8, 10):
        for (W, H), log2ctb, kind in (((72, 72), 5, "u4m34"), ((192, 40), 4, "u3"), ((72, 40), 4, "u4"), ((88, 40), 4, "u2"), ((88, 40), 6, "u4"), ((72, 72), 6, "rnd"),
                                      ((192, 64), 5, "rnd"), ((128, 64), 6, "u5"), ((256, 64), 5, "u4")):
            name = f"pairs/bd{bd}/{W}x{H}/{kind}"
            split = random_tree(name, (0, 0, 0, 0.3, 0.7, 0.9, 1.0)) if kind == "rnd" else uniform(int(kind[1]))
            # u4m34: every chroma TB mode 34, the one mode that reads p[2n - 1][-1], the 33rd neighbour of an
            # 8x8 pair (its half-wave's second chunk), here also where it is substituted
            turn = {}

            def style(t, name=name, turn=turn, kind=kind):
                h = hash_str(f"{name}/{t.tu}/style")
                t.tag = f"c{t.cidx}n{1 << t.log2}@{t.x},{t.y}"
                if t.cidx == 1:  # the modes in turn per size; Cr as its Cb
                    turn[t.log2] = turn.get(t.log2, 5 * t.log2) + 1
                if t.cidx:
                    t.mode = 34 if kind.endswith("m34") else turn[t.log2] % 35
                    if kind.endswith("m34"):
                        return
                if t.cidx and h % 11 == 0:
                    t.pcm = True          # a PCM pair
                if t.cidx == 2 and h % 13 == 1:
                    t.mode = (t.mode + 1) % 35  # the follower differs in mode: no pair
                if t.cidx == 2 and h % 17 == 2:
                    t.pcm = True          # PCM on Cr alone
            pics.append(Pic(name, ref.Geom(W, H, 1, bd, bd, log2ctb, 2), split, style))
    return Case("pairs", batches_of(pics))


def case_formats():
    """4:0:0, 4:2:2 and 4:4:4 at 8 and 10 bits: what is special to each."""
    pics = []
    for cf in (0, 2, 3):
        for bd in (8, 10):
            for (W, H), log2ctb, kind in (((72, 72), 6, "rnd"), ((88, 40), 5, "rnd"), ((72, 40), 4, "u3"),
                                          ((128, 128), 6, "u5"), ((72, 72), 5, "u4")):
                name = f"formats/cf{cf}/bd{bd}/{W}x{H}/{kind}"
                split = random_tree(name) if kind == "rnd" else uniform(int(kind[1]))

                def style(t):
                    t.tag = f"c{t.cidx}n{1 << t.log2}@{t.x},{t.y}"
                pics.append(Pic(name, ref.Geom(W, H, cf, bd, bd, log2ctb, 2 if kind == "rnd" else 3,
                                               strong=kind == "u5"), split, style))
    return Case("formats", batches_of(pics))


def _garbage(kind, g):
    """mangle(): records that do not pack, among a row's valid ones; each would write
    PCM samples if it ran"""
    def mangle(r, recs):
        if r != 0:
            return recs
        out = []
        for i, q in enumerate(recs):
            out.append(q)
            bad = dict(q, flags=(q["flags"] & 3) | TU_CBF | TU_PCM | TU_BYPASS)
            if kind == "mode35" and i % 5 == 1:
                out.append(dict(bad, mode=35))
            if kind == "edge" and i % 7 == 2 and (q["flags"] & 3) == 0:
                out.append(dict(bad, x=g.W - 4, log2=3, ctu=q["ctu"]))  # across the right edge (and outside its CTB)
                out.append(dict(bad, x=q["x"], y=g.H - 4, log2=3))      # across the bottom edge
            if kind == "outside" and i % 6 == 3 and (q["flags"] & 3) == 0:
                out.append(dict(bad, x=(q["x"] + (1 << g.log2_ctb)) % g.W))  # another CTB's samples
                out.append(dict(bad, log2=6))
                out.append(dict(bad, flags=bad["flags"] | 3))
        return out
    return mangle


def case_dispatch():
    """pic0 > 0, an assembly picture, mixed CTB sizes, fewer and more CTB rows than
    waves, records that do not pack, a record that ends its row."""
    def style(t):
        t.tag = f"c{t.cidx}n{1 << t.log2}@{t.x},{t.y}"
    G = lambda W, H, l, **kw: ref.Geom(W, H, 1, 10, 10, l, 2, **kw)
    pics = [Pic("dispatch/before_pic0", G(64, 64, 4), random_tree("d0"), style, launched=False),
            Pic("dispatch/ctb64", G(192, 128, 6, strong=True), random_tree("d1"), style),
            Pic("dispatch/tall_ctb16", G(64, 192, 4), random_tree("d2"), style),
            Pic("dispatch/assembly", G(128, 64, 5), random_tree("d3"), style, flags=PD_ASSEMBLY),
            Pic("dispatch/one_row", G(136, 24, 5), random_tree("d4"), style)]
    for kind in ("mode35", "edge", "outside"):
        g = G(96, 64, 5)
        pics.append(Pic(f"dispatch/garbage_{kind}", g, random_tree("d5" + kind), style, mangle=_garbage(kind, g)))
    # a record naming CTU wctb ends row 1 before its last two CTUs; what follows it must not run
    g = G(128, 64, 5)

    def stop(r, recs):
        if r != 1:
            return recs
        tail = [dict(x=96, y=32, log2=5, mode=1, ctu=3, flags=TU_CBF | TU_PCM | TU_BYPASS),
                dict(x=64, y=32, log2=5, mode=1, ctu=2, flags=TU_CBF | TU_PCM | TU_BYPASS)]
        return recs + [dict(x=64, y=32, log2=5, mode=1, ctu=4, flags=0)] + tail
    pics.append(Pic("dispatch/stop", g, random_tree("d6"), style, mangle=stop, stop_at=(1, 2)))
    return Case("dispatch", [Batch(pics, pic0=1)])


CASES = {"modes": case_modes, "availability": case_availability, "filter": case_filter, "edges": case_edges,
         "pairs": case_pairs, "formats": case_formats, "dispatch": case_dispatch}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once (its expectation stays as computed)."""
    return CASES[name]()
