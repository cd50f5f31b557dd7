"""A model of H.265 intra sample prediction and reconstruction on whole pictures.

Written from the clause text, on numpy int64, importing nothing of the product
or the oracle:

* 6.5.2  MinTbAddrZs for the whole picture (one slice, one tile: CtbAddrRsToTs
         is the identity), from the real log2 of the minimum TB size;
* 6.4.1  z-scan availability, the picture-bounds test first;
* 8.4.4.2.2  the neighbour search and substitution as worded;
* 8.4.4.2.3  filterFlag, intraHorVerDistThres, biIntFlag, [1 2 1] and bilinear;
* 8.4.4.2.4-6  planar, DC with its edge filter, angular over an explicit
         extended ref[] with the mode 26 / 10 boundary filters;
* 8.6.7  recSamples = Clip1(predSamples + resSamples).

predict_picture() takes the picture's geometry, the TB records in decoding
order and the residual planes and returns the reconstructed planes with, per
TB, a record of what happened (for the coverage tests of
tests/test_intra_predict.py).
"""
import dataclasses

import numpy as np

PLANAR, DC = 0, 1
# Table 8-5: intraPredAngle for predModeIntra 2..34
INTRA_PRED_ANGLE = {m: a for m, a in zip(range(2, 35), (
    32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26,
    -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32))}
# Table 8-6: invAngle for predModeIntra 11..25
INV_ANGLE = {m: a for m, a in zip(range(11, 26), (
    -4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096))}
# 8.4.4.2.3: intraHorVerDistThres[nTbS]
DIST_THRES = {8: 7, 16: 1, 32: 0}


@dataclasses.dataclass(frozen=True)
class Geom:
    W: int
    H: int
    chroma_format: int
    bd_y: int
    bd_c: int
    log2_ctb: int
    log2_min_tb: int = 2
    strong: bool = False

    @property
    def sub_w(self):  # SubWidthC (Table 6-1)
        return 2 if self.chroma_format in (1, 2) else 1

    @property
    def sub_h(self):  # SubHeightC
        return 2 if self.chroma_format == 1 else 1

    def plane(self, cidx):
        if cidx == 0:
            return self.W, self.H
        assert self.chroma_format
        return self.W // self.sub_w, self.H // self.sub_h

    @property
    def ncomp(self):
        return 3 if self.chroma_format else 1


@dataclasses.dataclass
class TB:
    cidx: int
    x: int       # component samples
    y: int
    log2: int
    mode: int    # the final predModeIntra of the component
    cbf: bool = False
    pcm: bool = False


@dataclasses.dataclass
class TBInfo:
    avail: np.ndarray          # 4n + 1 flags in the search order of 8.4.4.2.2
    filt: int = 0              # 0 no filtering, 1 [1 2 1], 2 bilinear
    strong_terms: tuple = ()   # luma 32x32, filtered: (top expression, left expression, threshold)
    clips: frozenset = frozenset()  # of "edge_lo", "edge_hi", "edge_mid", "rec_lo", "rec_hi", "rec_mid"
    min_ref: int = 0           # the smallest ref[] index read (angular)
    ifact_zero: bool = False
    ifact_nonzero: bool = False


# ---------------------------------------------------------------- 6.5.2, 6.4.1
def min_tb_addr_zs(g):
    """MinTbAddrZs[x][y] (6.5.2, equation 6-10), CtbAddrRsToTs the identity."""
    ctb = g.log2_ctb
    wctb = -(-g.W >> ctb)
    hctb = -(-g.H >> ctb)
    d = ctb - g.log2_min_tb
    out = np.zeros((wctb << d, hctb << d), dtype=np.int64)
    for y in range(hctb << d):
        for x in range(wctb << d):
            tb_x = (x << g.log2_min_tb) >> ctb
            tb_y = (y << g.log2_min_tb) >> ctb
            ctb_addr_rs = wctb * tb_y + tb_x
            v = ctb_addr_rs << (d * 2)
            for i in range(d):
                m = 1 << i
                v += (m * m if m & x else 0) + (2 * m * m if m & y else 0)
            out[x, y] = v
    return out


def available_zscan(g, zs, x_curr, y_curr, x_nb, y_nb):
    """6.4.1 for luma locations, one slice and one tile."""
    if x_nb < 0 or y_nb < 0 or x_nb >= g.W or y_nb >= g.H:
        return False
    s = g.log2_min_tb
    if zs[x_nb >> s, y_nb >> s] > zs[x_curr >> s, y_curr >> s]:
        return False
    return True


def search_positions(n):
    """(x, y) relative to the TB of the 4n + 1 neighbours in the search order of
    8.4.4.2.2: from p[-1][2n-1] upwards to p[-1][-1], then along the top."""
    return [(-1, y) for y in range(2 * n - 1, -2, -1)] + [(x, -1) for x in range(0, 2 * n)]


def avail_by_zscan(g, zs, tb):
    n = 1 << tb.log2
    sw, sh = (g.sub_w, g.sub_h) if tb.cidx else (1, 1)
    x_tb_y, y_tb_y = tb.x * sw, tb.y * sh
    return np.array([available_zscan(g, zs, x_tb_y, y_tb_y, (tb.x + dx) * sw, (tb.y + dy) * sh)
                     for dx, dy in search_positions(n)], dtype=bool)


def avail_by_mask(done, tb):
    """"Already reconstructed", from the mask painted as the records are processed."""
    n = 1 << tb.log2
    h, w = done.shape
    out = []
    for dx, dy in search_positions(n):
        x, y = tb.x + dx, tb.y + dy
        out.append(0 <= x < w and 0 <= y < h and bool(done[y, x]))
    return np.array(out, dtype=bool)


# ---------------------------------------------------------------- 8.4.4.2.2
class Neigh:
    """p[x][y] for x = -1, y = -1..2n-1 and x = 0..2n-1, y = -1."""

    def __init__(self, n):
        self.n = n
        self.left = np.zeros(2 * n + 1, dtype=np.int64)  # [y + 1] = p[-1][y]
        self.top = np.zeros(2 * n + 1, dtype=np.int64)   # [x + 1] = p[x][-1]

    def get(self, x, y):
        if x == -1:
            return int(self.left[y + 1])
        assert y == -1
        return int(self.top[x + 1])

    def put(self, x, y, v):
        if x == -1:
            self.left[y + 1] = v
            if y == -1:
                self.top[0] = v
        else:
            assert y == -1
            self.top[x + 1] = v


def substitute(plane, tb, avail, bd):
    n = 1 << tb.log2
    p = Neigh(n)
    pos = search_positions(n)
    if not avail.any():
        for x, y in pos:
            p.put(x, y, 1 << (bd - 1))
        return p
    av = {}
    for (x, y), a in zip(pos, avail):
        av[(x, y)] = bool(a)
        if a:
            p.put(x, y, int(plane[tb.y + y, tb.x + x]))
    # 1. p[-1][2n-1] from the first available sample of the search
    if not av[(-1, 2 * n - 1)]:
        for x, y in pos:
            if av[(x, y)]:
                p.put(-1, 2 * n - 1, p.get(x, y))
                break
    # 2. upwards: p[-1][y] from p[-1][y+1]
    for y in range(2 * n - 2, -2, -1):
        if not av[(-1, y)]:
            p.put(-1, y, p.get(-1, y + 1))
    # 3. along the top: p[x][-1] from p[x-1][-1]
    for x in range(0, 2 * n):
        if not av[(x, -1)]:
            p.put(x, -1, p.get(x - 1, -1))
    return p


# ---------------------------------------------------------------- 8.4.4.2.3
def filter_neighbours(g, tb, p, info):
    n = 1 << tb.log2
    if not (tb.cidx == 0 or g.chroma_format == 3):
        return p
    if tb.mode == DC or n == 4:
        return p
    min_dist = min(abs(tb.mode - 26), abs(tb.mode - 10))
    if not min_dist > DIST_THRES[n]:
        return p
    bd = g.bd_y  # (biIntFlag is for cIdx 0 only)
    bi = False
    if tb.cidx == 0 and n == 32:
        e_top = abs(p.get(-1, -1) + p.get(2 * n - 1, -1) - 2 * p.get(n - 1, -1))
        e_left = abs(p.get(-1, -1) + p.get(-1, 2 * n - 1) - 2 * p.get(-1, n - 1))
        info.strong_terms = (e_top, e_left, 1 << (bd - 5))
        bi = g.strong and e_top < (1 << (bd - 5)) and e_left < (1 << (bd - 5))
    f = Neigh(n)
    if bi:
        info.filt = 2
        f.put(-1, -1, p.get(-1, -1))
        for y in range(0, 63):
            f.put(-1, y, ((63 - y) * p.get(-1, -1) + (y + 1) * p.get(-1, 63) + 32) >> 6)
        f.put(-1, 63, p.get(-1, 63))
        for x in range(0, 63):
            f.put(x, -1, ((63 - x) * p.get(-1, -1) + (x + 1) * p.get(63, -1) + 32) >> 6)
        f.put(63, -1, p.get(63, -1))
    else:
        info.filt = 1
        f.put(-1, -1, (p.get(-1, 0) + 2 * p.get(-1, -1) + p.get(0, -1) + 2) >> 2)
        for y in range(0, 2 * n - 1):
            f.put(-1, y, (p.get(-1, y + 1) + 2 * p.get(-1, y) + p.get(-1, y - 1) + 2) >> 2)
        f.put(-1, 2 * n - 1, p.get(-1, 2 * n - 1))
        for x in range(0, 2 * n - 1):
            f.put(x, -1, (p.get(x - 1, -1) + 2 * p.get(x, -1) + p.get(x + 1, -1) + 2) >> 2)
        f.put(2 * n - 1, -1, p.get(2 * n - 1, -1))
    return f


# ---------------------------------------------------------------- 8.4.4.2.4-6
def _clip1(v, bd):
    return np.clip(v, 0, (1 << bd) - 1)


def _edge_clip(v, bd, clips):
    lo, hi = v < 0, v > (1 << bd) - 1
    if lo.any():
        clips.add("edge_lo")
    if hi.any():
        clips.add("edge_hi")
    if (~lo & ~hi).any():
        clips.add("edge_mid")
    return _clip1(v, bd)


def predict(g, tb, p, info, clips):
    """predSamples[y][x] (rows y) of the TB from its (filtered) neighbours."""
    n, k = 1 << tb.log2, tb.log2
    bd = g.bd_c if tb.cidx else g.bd_y
    left, top = p.left, p.top  # [i + 1] = p[-1][i], p[i][-1]
    x = np.arange(n)[None, :]
    y = np.arange(n)[:, None]
    if tb.mode == PLANAR:
        return ((n - 1 - x) * left[1 + y] + (x + 1) * top[1 + n] + (n - 1 - y) * top[1 + x] + (y + 1) * left[1 + n]
                + n) >> (k + 1)
    if tb.mode == DC:
        dc = (int(top[1:n + 1].sum()) + int(left[1:n + 1].sum()) + n) >> (k + 1)
        pred = np.full((n, n), dc, dtype=np.int64)
        if tb.cidx == 0 and n < 32:
            pred[0, 0] = (left[1] + 2 * dc + top[1] + 2) >> 2
            pred[0, 1:] = (top[2:n + 1] + 3 * dc + 2) >> 2
            pred[1:, 0] = (left[2:n + 1] + 3 * dc + 2) >> 2
        return pred
    ang = INTRA_PRED_ANGLE[tb.mode]
    vertical = tb.mode >= 18
    main, side = (top, left) if vertical else (left, top)  # [i + 1] = the side at i
    # ref[] as the text builds it: an explicit array from its lowest index up
    ref = {i: int(main[i]) for i in range(0, n + 1)}  # ref[x] = p[-1 + x][-1], x = 0..nTbS
    if ang < 0:
        last = (n * ang) >> 5
        if last < -1:
            inv = INV_ANGLE[tb.mode]
            for i in range(last, 0):  # x = (nTbS * intraPredAngle) >> 5 .. -1
                ref[i] = int(side[((i * inv + 128) >> 8)])  # p[-1][-1 + ((x * invAngle + 128) >> 8)]
    else:
        for i in range(n + 1, 2 * n + 1):
            ref[i] = int(main[i])
    lo = min(ref)
    arr = np.array([ref[i] for i in range(lo, max(ref) + 1)], dtype=np.int64)
    a, b = (x, y) if vertical else (y, x)  # a runs along the main side
    idx = ((b + 1) * ang) >> 5
    fact = ((b + 1) * ang) & 31
    i0 = a + idx + 1
    need_hi = np.where(fact != 0, i0 + 1, i0)
    assert i0.min() >= lo and need_hi.max() <= max(ref), "a ref[] index the text does not build"
    info.min_ref = int(i0.min())
    info.ifact_zero = bool((fact == 0).any())
    info.ifact_nonzero = bool((fact != 0).any())
    r0 = arr[i0 - lo]
    r1 = arr[np.minimum(i0 + 1, max(ref)) - lo]
    pred = np.where(fact != 0, ((32 - fact) * r0 + fact * r1 + 16) >> 5, r0)
    if tb.cidx == 0 and n < 32:
        if tb.mode == 26:  # predSamples[0][y] = Clip1Y(p[0][-1] + ((p[-1][y] - p[-1][-1]) >> 1))
            pred[:, 0] = _edge_clip(top[1] + ((left[1:n + 1] - left[0]) >> 1), bd, clips)
        if tb.mode == 10:  # predSamples[x][0] = Clip1Y(p[-1][0] + ((p[x][-1] - p[-1][-1]) >> 1))
            pred[0, :] = _edge_clip(left[1] + ((top[1:n + 1] - top[0]) >> 1), bd, clips)
    return pred


# ---------------------------------------------------------------- the picture
def predict_tb(g, tb, plane, res, avail):
    """(reconstructed n x n samples, TBInfo) of one TB; plane holds the decoded neighbours."""
    n = 1 << tb.log2
    bd = g.bd_c if tb.cidx else g.bd_y
    info = TBInfo(avail=avail)
    clips = set()
    if tb.pcm:
        pred = np.zeros((n, n), dtype=np.int64)
    else:
        p = substitute(plane, tb, avail, bd)
        p = filter_neighbours(g, tb, p, info)
        pred = predict(g, tb, p, info, clips)
    v = pred + (res[tb.y:tb.y + n, tb.x:tb.x + n] if tb.cbf else 0)
    if not tb.pcm:
        if (v < 0).any():
            clips.add("rec_lo")
        if (v > (1 << bd) - 1).any():
            clips.add("rec_hi")
        if ((v >= 0) & (v <= (1 << bd) - 1)).any():
            clips.add("rec_mid")
    info.clips = frozenset(clips)
    return _clip1(v, bd), info


def predict_picture(g, tbs, resid, fill=0, check_mask=True):
    """Reconstructed planes (samples no TB covers hold `fill`), the TBInfo of
    every TB, and whether the two availability functions agreed on every
    neighbour of every TB."""
    zs = min_tb_addr_zs(g)
    planes = [np.full(g.plane(k)[::-1], fill, dtype=np.int64) for k in range(g.ncomp)]
    done = [np.zeros(g.plane(k)[::-1], dtype=bool) for k in range(g.ncomp)]
    infos, agree = [], True
    for tb in tbs:
        n = 1 << tb.log2
        w, h = g.plane(tb.cidx)
        assert 0 <= tb.x and tb.x + n <= w and 0 <= tb.y and tb.y + n <= h and 0 <= tb.mode <= 34
        avail = avail_by_zscan(g, zs, tb)
        if check_mask:
            agree = agree and bool((avail == avail_by_mask(done[tb.cidx], tb)).all())
        rec, info = predict_tb(g, tb, planes[tb.cidx], resid[tb.cidx], avail)
        planes[tb.cidx][tb.y:tb.y + n, tb.x:tb.x + n] = rec
        done[tb.cidx][tb.y:tb.y + n, tb.x:tb.x + n] = True
        infos.append(info)
    return planes, infos, agree
