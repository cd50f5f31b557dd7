"""Cases for what k_transform reads off a TB's records instead of its tile: the DC-only
test, the extents of the dot-product stages, the scaling and pass A's rounds.

Everything is built with the encoder and checked against the integer model of
tests/xform_vectors.py, unchanged; pictures are at most 64x64.  One thing the encoder
cannot write is added here: a hidden sign on a sub-block with a single coefficient
(`hide="force"`), which 9.3.4.3 never produces but the record format can hold, so the
DC shortcut has to honour it like any other path.
"""
import contextlib
import functools
import itertools

import numpy as np

import xform_vectors as xv
from xform_vectors import TB, Case, Pic, Seq

SIZE = 64


# ---------------------------------------------------------------- a forced hidden sign
def _encode_forced(levels, n, scan_idx, hide, row):
    if hide != "force":
        return _encode_plain(levels, n, scan_idx, hide, row)
    levels = np.array(levels, dtype=np.int64)
    ys, xs = np.nonzero(levels)
    assert len(ys) == 1, "a forced hidden sign is for a single coefficient"
    at, ncoef, lv = _encode_plain(levels, n, scan_idx, False, row)
    assert ncoef == 4
    row.words[at] &= 0xffff       # no sign bin: the sign is the level's parity
    row.words[at + 3] |= 1 << 8
    v = abs(int(levels[ys[0], xs[0]]))
    lv[ys[0], xs[0]] = -v if v & 1 else v
    return at, ncoef, lv


_encode_plain = xv.encode_records


@contextlib.contextmanager
def _forced_hidden_signs():
    xv.encode_records = _encode_forced
    try:
        yield
    finally:
        xv.encode_records = _encode_plain


# ---------------------------------------------------------------- helpers
def at_scan(n, sb, k, v, scan_idx=0, base=None):
    """Level v at scan position k of sub-block sb = (xS, yS) of an n x n TB."""
    a = np.zeros((n, n), dtype=np.int64) if base is None else base
    px, py = xv.scan_order(4, scan_idx)[k]
    a[4 * sb[1] + py, 4 * sb[0] + px] = v
    return a


def pictures(seq_index, seq, tbs):
    """The TBs spread over as many pictures of `seq` as their planes need, the large
    ones first in each (first-fit placement of aligned power-of-two blocks)."""
    pics, cur, used = [], [], [0, 0, 0]

    def area(cidx):
        w, h = seq.plane(min(cidx, 2) if seq.chroma_format else 0)
        return w * h

    for t in tbs:
        takes = t.coded and not t.outside and t.x is None
        c = min(t.cidx, 2)
        if takes and used[c] + t.n * t.n > area(c):
            pics.append(cur)
            cur, used = [], [0, 0, 0]
        if takes:
            used[c] += t.n * t.n
        cur.append(t)
    pics.append(cur)
    out = []
    for group in pics:
        group = sorted(group, key=lambda t: -t.n)
        for k, t in enumerate(group):
            t.row = k % seq.rows
        out.append(Pic(seq_index, group))
    return out


# ---------------------------------------------------------------- the cases
def case_dc():
    """The DC shortcut's boundary: every TB that must take it, in all three scans, as a
    negative, a hidden-sign and an escape level, and the near misses that must not."""
    seqs = [Seq(SIZE, SIZE, 5, 3, 8, 8), Seq(SIZE, SIZE, 5, 3, 10, 12), Seq(SIZE, SIZE, 5, 3, 8, 8, sf=xv.ramp_sf(7)),
            Seq(SIZE, SIZE, 5, 3, 8, 8, sf=xv.const_sf(255))]
    by_seq = [[] for _ in seqs]
    for n, cidx in itertools.product((8, 16, 32), (0, 1)):
        far = n // 4 - 1
        for si in (0, 1):
            for sc in range(3):
                tag = f"dc/yes/s{si}/n{n}/c{cidx}/scan{sc}"
                for name, v, hide in (("pos", 7, False), ("neg", -9, False), ("hidden_odd", 11, "force"),
                                      ("hidden_even", 12, "force"), ("escape", 300, False),
                                      ("escape_neg_hidden", 20001, "force"), ("escape_max", -32768, False)):
                    if si == 1 and name in ("pos", "hidden_even"):
                        continue
                    by_seq[si].append(TB(f"{tag}/{name}", n, cidx, 22 + 3 * sc + cidx, at_scan(n, (0, 0), 0, v, sc),
                                         scan_idx=sc, hide=hide))
        tag = f"dc/no/n{n}/c{cidx}"
        miss = by_seq[0]
        miss.append(TB(f"{tag}/sig2", n, cidx, 27, at_scan(n, (0, 0), 1, -3, base=at_scan(n, (0, 0), 0, 5))))
        miss.append(TB(f"{tag}/scan1_alone", n, cidx, 27, at_scan(n, (0, 0), 1, 6)))
        miss.append(TB(f"{tag}/subblock_1_0", n, cidx, 27, at_scan(n, (1, 0), 0, 6)))
        miss.append(TB(f"{tag}/subblock_0_1", n, cidx, 27, at_scan(n, (0, 1), 0, -6, 2), scan_idx=2))
        miss.append(TB(f"{tag}/subblock_far", n, cidx, 27, at_scan(n, (far, far), 0, 6, 1), scan_idx=1))
        for sc in range(3):  # sub-block (0, 0) is decoded last in every scan: the DC in the second record
            other = ((1, 0), (0, 1), (1, 1))[sc]
            miss.append(TB(f"{tag}/two_records_scan{sc}", n, cidx, 27,
                           at_scan(n, other, 0, 4, sc, base=at_scan(n, (0, 0), 0, -5, sc)), scan_idx=sc))
        miss.append(TB(f"{tag}/tskip", n, cidx, 27, at_scan(n, (0, 0), 0, 9), ts=True))
        miss.append(TB(f"{tag}/bypass", n, cidx, 27, at_scan(n, (0, 0), 0, -9), bypass=True))
        for si in (2, 3):  # under a scaling list the factor at (0, 0) is not 16
            by_seq[si].append(TB(f"dc/list/s{si}/n{n}/c{cidx}", n, cidx, 30, at_scan(n, (0, 0), 0, -13)))
            by_seq[si].append(TB(f"dc/list/s{si}/n{n}/c{cidx}/tskip", n, cidx, 30, at_scan(n, (0, 0), 0, 13), ts=True))
    # a 4x4 chroma DC and a luma DST one beside them (pass A, untouched by the shortcut)
    by_seq[0].append(TB("dc/pass_a/c1", 4, 1, 30, at_scan(4, (0, 0), 0, 40)))
    by_seq[0].append(TB("dc/pass_a/dst", 4, 0, 30, at_scan(4, (0, 0), 0, 40), dst=True))
    pics = [p for si, s in enumerate(seqs) for p in pictures(si, s, by_seq[si])]
    with _forced_hidden_signs():
        return Case("dc", seqs, pics)


def case_extents():
    """The dot products' extents from the records: every non-empty set of an 8x8 TB's
    four sub-blocks with its coefficient at the sub-block's last and first scan
    position, and single far sub-blocks of the larger sizes (the emulation's stages)."""
    seqs = [Seq(SIZE, SIZE, 5, 3, 8, 8)]
    tbs = []
    sbs = ((0, 0), (1, 0), (0, 1), (1, 1))
    for mask in range(1, 16):
        for k in (15, 0):
            sc = (mask + k) % 3
            lv = np.zeros((8, 8), dtype=np.int64)
            for b, sb in enumerate(sbs):
                if mask >> b & 1:
                    at_scan(8, sb, k, (-1) ** b * (20 + 7 * b + mask), sc, base=lv)
            tbs.append(TB(f"extents/n8/mask{mask}/scan_pos{k}", 8, mask % 3, 24 + mask, lv, scan_idx=sc))
    for n in (16, 32):
        f = n // 4 - 1
        for sb in ((f, 0), (0, f), (f, f), (f - 1, 1), (1, f - 1)):
            for k in (15, 0):
                tbs.append(TB(f"extents/n{n}/sb{sb[0]}_{sb[1]}/scan_pos{k}", n, (sb[0] + k) % 3, 26,
                              at_scan(n, sb, k, 33 - 2 * k, k % 3), scan_idx=k % 3))
        both = at_scan(n, (f, 0), 15, -21, base=at_scan(n, (0, f), 15, 19))
        tbs.append(TB(f"extents/n{n}/two_far_corners", n, 0, 26, both))
    return Case("extents", seqs, pictures(0, seqs[0], tbs))


SCALING_LEVELS = (1, -1, 255, -255, 32767, -32767, -32768, 32767)


def _scaling_levels(n, salt):
    """The levels at eight positions of the TB, (0, 0) and the far corner among them."""
    spots = [(0, 0), (1, 0), (0, 1), (n - 1, n - 1), (n - 1, 0), (0, n - 1), (2, 3), (n - 2, n - 3)]
    lv = np.zeros((n, n), dtype=np.int64)
    for k, (x, y) in enumerate(spots):
        lv[y, x] = SCALING_LEVELS[(k + salt) % len(SCALING_LEVELS)]
    return lv


def case_scaling():
    """8.6.3 at the ends of its operands: at 8 bits every TB size at qp 0, 5, 6 and 51,
    flat and under lists of 1, 16 and 255; at 10 and 12 bits the largest legal qP."""
    seqs = [Seq(SIZE, SIZE, 5, 3, 8, 8), Seq(SIZE, SIZE, 5, 3, 8, 8, sf=xv.const_sf(1)),
            Seq(SIZE, SIZE, 5, 3, 8, 8, sf=xv.const_sf(16)), Seq(SIZE, SIZE, 5, 3, 8, 8, sf=xv.const_sf(255)),
            Seq(SIZE, SIZE, 5, 3, 10, 10), Seq(SIZE, SIZE, 5, 3, 12, 12), Seq(SIZE, SIZE, 5, 3, 12, 8)]
    pics = []
    for si, s in enumerate(seqs):
        tbs = []
        qps = (0, 5, 6, 51) if s.bd_y == 8 else ((63, 4) if s.bd_y == 10 else (75, 51))
        for qi, qp in enumerate(qps):
            for n in (4, 8, 16, 32):
                cidx = (qi + n.bit_length()) % 3
                if s.bd_c != s.bd_y and cidx and qp > 51 + 6 * (s.bd_c - 8):
                    cidx = 0  # (legal for the luma depth only)
                tag = f"scaling/s{si}_bd{s.bd_y}_{s.bd_c}/qp{qp}/n{n}/c{cidx}"
                tbs.append(TB(tag, n, cidx, qp, _scaling_levels(n, qi + si), scan_idx=qi % 3))
                if n == 4:
                    tbs.append(TB(tag + "/dst", n, 0, qp, _scaling_levels(n, qi + si + 3), dst=True))
                if n == 8:
                    tbs.append(TB(tag + "/dc", n, cidx, qp, at_scan(n, (0, 0), 0, SCALING_LEVELS[(4 + qi) % 8])))
        pics += pictures(si, s, tbs)
    return Case("scaling", seqs, pics)


def case_pass_a():
    """Pass A's rounds of four: rows that give every wave one to seven coded 4x4 TBs, the
    members of a round differing in qp, cIdx and the DST, uncoded and larger records
    between them."""
    seqs = [Seq(SIZE, SIZE, 4, 3, 8, 8), Seq(SIZE, SIZE, 4, 3, 8, 8, sf=xv.ramp_sf(3))]
    rng = np.random.default_rng(2404)
    pics = []
    for si, counts in ((0, (1, 2, 3, 4)), (0, (5, 6, 7, 1)), (1, (3, 1, 4, 2))):
        tbs = []
        for row, per_wave in enumerate(counts):
            for t in range(4 * per_wave):  # record t goes to wave t % 4
                cidx = (t + row) % 3
                lv = rng.integers(-300, 301, size=(4, 4)) * (rng.random((4, 4)) < 0.6)
                lv[(t >> 2) & 3, t & 3] = 1 + t
                tbs.append(TB(f"pass_a/s{si}/row{row}_{per_wave}_per_wave/{t}", 4, cidx, (7 * t + 13 * row) % 52, lv,
                              dst=(cidx == 0 and t % 2 == 0), scan_idx=t % 3, hide=bool(t & 1), row=row))
                if t % 5 == 2:  # an uncoded 4x4 and a coded 8x8 record in between: the waves' lists shift
                    tbs.append(TB(f"pass_a/s{si}/row{row}/{t}_uncoded", 4, 0, 30, lv, coded=False, row=row))
                    tbs.append(TB(f"pass_a/s{si}/row{row}/{t}_n8", 8, t % 3, 30, rng.integers(-50, 51, size=(8, 8)), row=row))
        pics.append(Pic(si, tbs))
    return Case("pass_a", seqs, pics)


def ballot_rounds(case):
    """{coded 4x4 TBs of one wave in one row} over the case's launched pictures."""
    out = set()
    for _, _, recs in case.rows_tus:
        out |= set(xv.ballot_counts(recs).values())
    return out


def case_no_write():
    """Records that must write nothing: sizes outside 4..32, cIdx 3, a TB one sample
    over its plane's right and bottom edge, an assembly picture's records."""
    seqs = [Seq(SIZE, SIZE, 5, 1, 8, 8)]
    rng = np.random.default_rng(2405)

    def lv(n):
        a = rng.integers(-40, 41, size=(n, n))
        a[0, 0] = 17
        return a

    tbs = [TB("no_write/live/n8", 8, 0, 30, lv(8)), TB("no_write/live/n4", 4, 1, 30, lv(4)),
           TB("no_write/live/n32", 32, 0, 30, lv(32)), TB("no_write/live/dc16", 16, 2, 30, at_scan(16, (0, 0), 0, 50))]
    dead = [TB("no_write/log2_1", 2, 0, 30, np.full((2, 2), 9), x=8, y=40, outside=True),
            TB("no_write/log2_6", 64, 0, 30, at_scan(64, (0, 0), 0, 9), x=0, y=0, outside=True),
            TB("no_write/log2_6_dense", 64, 1, 30, lv(64), x=0, y=0, outside=True)]
    for n in (4, 8, 16, 32):
        for cidx in (0, 1, 2):
            w, h = seqs[0].plane(cidx)
            if n > w:
                continue
            full, dc = lv(n), at_scan(n, (0, 0), 0, 21)
            dead.append(TB(f"no_write/cidx3/n{n}", n, 3, 30, full, x=0, y=0, outside=True))
            dead.append(TB(f"no_write/right/n{n}/c{cidx}", n, cidx, 30, full, x=w - n + 1, y=0, outside=True))
            dead.append(TB(f"no_write/bottom/n{n}/c{cidx}", n, cidx, 30, full, x=0, y=h - n + 1, outside=True))
            dead.append(TB(f"no_write/corner_dc/n{n}/c{cidx}", n, cidx, 30, dc, x=w - n + 1, y=h - n + 1, outside=True))
    order = []
    for k, t in enumerate(dead):  # the live TBs between the dead ones
        order.append(t)
        if k % 9 == 4 and tbs:
            order.append(tbs.pop())
    order += tbs
    for k, t in enumerate(order):
        t.row = k % 2
    ghost = [TB(f"no_write/assembly/{k}_n{n}", n, k % 3 if n < 32 else 0, 30,
                at_scan(n, (0, 0), 0, 25) if k & 1 else lv(n), row=k % 2) for k, n in enumerate((4, 8, 16, 32, 4, 8, 16))]
    return Case("no_write", seqs, [Pic(0, order), Pic(0, ghost, flags=xv.PD_ASSEMBLY)])


CASES = {"dc": case_dc, "extents": case_extents, "scaling": case_scaling, "pass_a": case_pass_a,
         "no_write": case_no_write}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once (its expected residuals stay as computed)."""
    c = CASES[name]()
    c.expected.setflags(write=False)
    return c
