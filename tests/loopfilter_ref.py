"""An integer model of H.265 8.7.2 (deblocking) and 8.7.3 (SAO) plus the output
placement of k_sao_out, on numpy int64, written from the clause text.

Its inputs are the loop-filter kernels' contract (common/desc.hpp): the QpY
map (one int8 per 4x4 luma block), the flag map (MF_EDGE_V / MF_EDGE_H /
MF_NOFILT per 4x4 luma block), one SaoParams per CTB and the PicDesc /
SeqParams fields the kernels read.  bS is 2 wherever an edge flag is set on
the 8x8 luma grid away from the picture's left / top; there is no bS 1 (intra
pictures only).  The maps are finer than the coding-unit grid a real stream
gives them, so chroma takes bS, QpY and the no-filter flag per chroma line
from the 4x4 luma block that line lies in: 4 >> log2(SubHeightC) lines per
block along a vertical edge, 4 >> log2(SubWidthC) along a horizontal one.

Shape: the whole picture at once.  All p3..q3 lines of one direction are
gathered into arrays, the decisions dE / dEp / dEq and then nDp / nDq are taken
with np.where and applied in one step; horizontal edges are the vertical-edge
code on the transposed plane and maps.  Every function also returns what each
segment, line or sample did (`ev`, name -> array of small codes, NA where the
question does not arise), from which the coverage tests are asserted.
"""
import numpy as np

MF_EDGE_V, MF_EDGE_H, MF_NOFILT = 1, 2, 4
NA = -9


# ---------------------------------------------------------------- tables
def beta_prime(q):
    """Table 8-12, beta' of Q = 0..51, by its closed form."""
    q = np.asarray(q, dtype=np.int64)
    return np.where(q < 16, 0, np.where(q < 29, q - 10, 2 * q - 38))


# Table 8-12, tC' of Q = 0..53, as (run length, value)
_TC_RUNS = ((18, 0), (9, 1), (4, 2), (4, 3), (3, 4), (2, 5), (2, 6)) + tuple(
    (1, v) for v in (7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24))
TC_PRIME = np.array([v for n, v in _TC_RUNS for _ in range(n)], dtype=np.int64)
assert TC_PRIME.size == 54

# Table 8-10 (ChromaArrayType 1), qPi 30..43
_QPC_1 = {30: 29, 31: 30, 32: 31, 33: 32, 34: 33, 35: 33, 36: 34, 37: 34, 38: 35, 39: 35, 40: 36, 41: 36, 42: 37,
          43: 37}


def qp_chroma(qpi, chroma_array_type):
    qpi = np.asarray(qpi, dtype=np.int64)
    if chroma_array_type != 1:
        return np.minimum(qpi, 51)
    mid = np.vectorize(lambda v: _QPC_1.get(int(v), 0), otypes=[np.int64])(qpi)
    return np.where(qpi < 30, qpi, np.where(qpi >= 44, qpi - 6, mid))


def subsampling(fmt):
    """log2 SubWidthC, log2 SubHeightC (Table 6-1)"""
    return {0: (0, 0), 1: (1, 1), 2: (1, 0), 3: (0, 0)}[fmt]


def clip3(lo, hi, v):
    return np.minimum(np.maximum(v, lo), hi)


def _sgn(a, b):
    """-1 / 0 / 1: a below, at, above b"""
    return np.sign(np.asarray(a, dtype=np.int64) - b).astype(np.int64)


def _lines(seg):
    """a per-segment array (n, e) as per-line (4 n, e)"""
    return np.repeat(seg, 4, axis=0)


# ---------------------------------------------------------------- deblocking, luma
def luma_vertical(P, qpy, flg, bd, beta_off, tc_off):
    """8.7.2.5.3 / .6 / .7 on every vertical edge of the luma plane P (H, W):
    the filtered plane and the events (per segment (H / 4, ne), per line (H, ne))."""
    H, W = P.shape
    xs = np.arange(8, W, 8)
    out = P.copy()
    if xs.size == 0 or H < 4:
        return out, {}
    rows = (np.arange(H) >> 2)[:, None]
    cq, cp = (xs >> 2)[None, :], ((xs - 1) >> 2)[None, :]
    fq, fp = flg[rows, cq].astype(np.int64), flg[rows, cp].astype(np.int64)
    bs = np.where(fq & MF_EDGE_V, 2, 0)
    qpq, qpp = qpy[rows, cq].astype(np.int64), qpy[rows, cp].astype(np.int64)
    p = [P[:, xs - 1 - i] for i in range(4)]
    q = [P[:, xs + i] for i in range(4)]
    # 8.7.2.5.3: beta and tC of the segment
    qpl = (qpq + qpp + 1) >> 1
    qb_raw = qpl + (beta_off << 1)
    qb = clip3(0, 51, qb_raw)
    beta = beta_prime(qb) * (1 << (bd - 8))
    qt_raw = qpl + 2 * (bs - 1) + (tc_off << 1)
    qt = clip3(0, 53, qt_raw)
    tc = TC_PRIME[qt] * (1 << (bd - 8))
    dpl = np.abs(p[2] - 2 * p[1] + p[0])
    dql = np.abs(q[2] - 2 * q[1] + q[0])
    dp0, dp3, dq0, dq3 = dpl[0::4], dpl[3::4], dql[0::4], dql[3::4]
    dpq0, dpq3 = dp0 + dq0, dp3 + dq3
    dp, dq, d = dp0 + dp3, dq0 + dq3, dpq0 + dpq3
    sbeta, stc, sbs = beta[0::4], tc[0::4], bs[0::4]
    edge = sbs == 2
    on = edge & (d < sbeta)
    # 8.7.2.5.6 for line 0 and line 3
    conds = {}
    for k, dpq in ((0, 2 * dpq0), (3, 2 * dpq3)):
        p0, p3, q0, q3 = p[0][k::4], p[3][k::4], q[0][k::4], q[3][k::4]
        conds[k, "a"] = (dpq, sbeta >> 2)
        conds[k, "b"] = (np.abs(p3 - p0) + np.abs(q0 - q3), sbeta >> 3)
        conds[k, "c"] = (np.abs(p0 - q0), (5 * stc + 1) >> 1)
    holds = {key: a < b for key, (a, b) in conds.items()}
    dsam0 = holds[0, "a"] & holds[0, "b"] & holds[0, "c"]
    dsam3 = holds[3, "a"] & holds[3, "b"] & holds[3, "c"]
    side = (sbeta + (sbeta >> 1)) >> 3
    dE = np.where(on, np.where(dsam0 & dsam3, 2, 1), 0)
    dEp = np.where(on & (dp < side), 1, 0)
    dEq = np.where(on & (dq < side), 1, 0)
    lE, lEp, lEq = _lines(dE), _lines(dEp), _lines(dEq)
    # 8.7.2.5.7: both filters for every line, then chosen by dE
    p0, p1, p2, p3 = p
    q0, q1, q2, q3 = q
    strong_raw = {"p0": (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, "p1": (p2 + p1 + p0 + q0 + 2) >> 2,
                  "p2": (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3,
                  "q0": (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, "q1": (p0 + q0 + q1 + q2 + 2) >> 2,
                  "q2": (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3}
    cur = {"p0": p0, "p1": p1, "p2": p2, "q0": q0, "q1": q1, "q2": q2}
    strong = {n: clip3(cur[n] - 2 * tc, cur[n] + 2 * tc, v) for n, v in strong_raw.items()}
    maxv = (1 << bd) - 1
    delta_raw = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
    weak = (lE == 1) & (np.abs(delta_raw) < tc * 10)
    delta = clip3(-tc, tc, delta_raw)
    dlt_p_raw = (((p2 + p0 + 1) >> 1) - p1 + delta) >> 1
    dlt_q_raw = (((q2 + q0 + 1) >> 1) - q1 - delta) >> 1
    dlt_p, dlt_q = clip3(-(tc >> 1), tc >> 1, dlt_p_raw), clip3(-(tc >> 1), tc >> 1, dlt_q_raw)
    normal_raw = {"p0": p0 + delta, "q0": q0 - delta, "p1": p1 + dlt_p, "q1": q1 + dlt_q}
    normal = {n: clip3(0, maxv, v) for n, v in normal_raw.items()}
    normal["p2"], normal["q2"] = p2, q2
    nDp = np.where(lE == 2, 3, np.where(weak, lEp + 1, 0))
    nDq = np.where(lE == 2, 3, np.where(weak, lEq + 1, 0))
    nfp, nfq = (fp & MF_NOFILT) != 0, (fq & MF_NOFILT) != 0
    nDp, nDq = np.where(nfp, 0, nDp), np.where(nfq, 0, nDq)
    for i in range(3):
        out[:, xs - 1 - i] = np.where(nDp > i, np.where(lE == 2, strong[f"p{i}"], normal[f"p{i}"]), p[i])
        out[:, xs + i] = np.where(nDq > i, np.where(lE == 2, strong[f"q{i}"], normal[f"q{i}"]), q[i])
    # ---- what happened: only where both sides are filtered, so every event shows in the samples
    free = edge & ~nfp[0::4] & ~nfq[0::4]
    lfree = _lines(free)

    def where(mask, v):
        return np.where(mask, v, NA)

    ev = {"d": where(free, _sgn(d, sbeta)),
          "dE": where(free, dE * 4 + dEp * 2 + dEq),
          "dp": where(free & (dE == 1), _sgn(dp, side)),
          "dq": where(free & (dE == 1), _sgn(dq, side)),
          "Qbeta": where(free, _sgn(qb_raw, qb)[0::4]),
          "QtC": where(free, _sgn(qt_raw, qt)[0::4]),
          "qp_odd": where(free & (d < sbeta), ((qpq + qpp) & 1)[0::4]),
          # 0: neither QpY negative, 1: one is, 2: one is -QpBdOffsetY, the least there is
          "qp_neg": where(free & (d < sbeta), ((np.minimum(qpq, qpp) < 0) * 1
                                               + ((np.minimum(qpq, qpp) == -6 * (bd - 8)) & (bd > 8)) * 1)[0::4]),
          "nofilt": where(edge & (d < sbeta), (nfp * 2 + nfq)[0::4]),
          "delta": where(lfree & (lE == 1), _sgn(np.abs(delta_raw), tc * 10)),
          "clip_delta": where(lfree & weak, _sgn(delta_raw, delta)),
          "clip_dp": where(lfree & weak & (lEp == 1), _sgn(dlt_p_raw, dlt_p)),
          "clip_dq": where(lfree & weak & (lEq == 1), _sgn(dlt_q_raw, dlt_q))}
    for key, (a, b) in conds.items():  # a condition counts where the other five hold: there it decides dE
        others = np.ones_like(on)
        for k2, h in holds.items():
            if k2 != key:
                others &= h
        ev[f"dsam{key[0]}{key[1]}"] = where(free & on & others, _sgn(a, b))
    for n in ("p0", "q0"):
        ev[f"clip1_{n}"] = where(lfree & weak, _sgn(normal_raw[n], normal[n]))
    ev["clip1_p1"] = where(lfree & weak & (lEp == 1), _sgn(normal_raw["p1"], normal["p1"]))
    ev["clip1_q1"] = where(lfree & weak & (lEq == 1), _sgn(normal_raw["q1"], normal["q1"]))
    for n in strong:
        ev[f"strong_{n}"] = where(lfree & (lE == 2), _sgn(strong_raw[n], strong[n]))
    return out, ev


# ---------------------------------------------------------------- deblocking, chroma
def chroma_vertical(C, qpy, flg, sx, sy, chroma_array_type, bd, qp_offset, tc_off):
    """8.7.2.5.5 / .8 on every vertical edge of the 8x8 chroma-sample grid of
    the plane C (ch, cw), per chroma line."""
    ch, cw = C.shape
    xs = np.arange(8, cw, 8)
    out = C.copy()
    if xs.size == 0:
        return out, {}
    rows = ((np.arange(ch) << sy) >> 2)[:, None]
    xl = xs << sx
    cq, cp = (xl >> 2)[None, :], ((xl - 1) >> 2)[None, :]
    fq, fp = flg[rows, cq].astype(np.int64), flg[rows, cp].astype(np.int64)
    bs = np.where(fq & MF_EDGE_V, 2, 0)
    qpq, qpp = qpy[rows, cq].astype(np.int64), qpy[rows, cp].astype(np.int64)
    qpi = ((qpq + qpp + 1) >> 1) + qp_offset
    qpc = qp_chroma(qpi, chroma_array_type)
    qt_raw = qpc + 2 * (bs - 1) + (tc_off << 1)
    qt = clip3(0, 53, qt_raw)
    tc = TC_PRIME[qt] * (1 << (bd - 8))
    p0, p1, q0, q1 = C[:, xs - 1], C[:, xs - 2], C[:, xs], C[:, xs + 1]
    delta_raw = (((q0 - p0) << 2) + p1 - q1 + 4) >> 3
    delta = clip3(-tc, tc, delta_raw)
    maxv = (1 << bd) - 1
    np0, nq0 = clip3(0, maxv, p0 + delta), clip3(0, maxv, q0 - delta)
    edge = bs == 2
    nfp, nfq = (fp & MF_NOFILT) != 0, (fq & MF_NOFILT) != 0
    out[:, xs - 1] = np.where(edge & ~nfp, np0, p0)
    out[:, xs] = np.where(edge & ~nfq, nq0, q0)
    free = edge & ~nfp & ~nfq
    ev = {"qpi": np.where(free, np.where(qpi < 0, -1, np.where(qpi > 51, 52, np.where((qpi >= 30) & (qpi <= 43), qpi,
                                                                                   NA))), NA),
          "QtC": np.where(free, _sgn(qt_raw, qt), NA),
          "clip_delta": np.where(free & (tc > 0), _sgn(delta_raw, delta), NA),
          "clip1_p0": np.where(free, _sgn(p0 + delta, np0), NA),
          "clip1_q0": np.where(free, _sgn(q0 - delta, nq0), NA),
          "nofilt": np.where(edge, nfp * 2 + nfq, NA)}
    return out, ev


# ---------------------------------------------------------------- deblocking, the picture
def _swap_dirs(flg):
    """the flag map of the transposed picture"""
    f = flg.T
    return ((f & MF_EDGE_V) << 1) | ((f & MF_EDGE_H) >> 1) | (f & MF_NOFILT)


def deblock(planes, qpy, flg, fmt, bd_y, bd_c, cb_qp_offset, cr_qp_offset, beta_off, tc_off):
    """8.7.2: all vertical edges of the picture, then all horizontal ones on the
    result.  planes: [Y] or [Y, Cb, Cr] (int64, (rows, columns)); returns the
    new planes and {(component kind, "V" | "H"): events}."""
    sx, sy = subsampling(fmt)
    events = {}
    cur = [pl.astype(np.int64) for pl in planes]
    for d in "VH":
        t = d == "H"
        m_qpy, m_flg = (qpy.T, _swap_dirs(flg)) if t else (qpy, flg)
        ssx, ssy = (sy, sx) if t else (sx, sy)
        y, ev = luma_vertical(cur[0].T if t else cur[0], m_qpy, m_flg, bd_y, beta_off, tc_off)
        events["luma", d] = ev
        nxt = [y.T if t else y]
        for cidx in (1, 2) if fmt else ():
            c, ev = chroma_vertical(cur[cidx].T if t else cur[cidx], m_qpy, m_flg, ssx, ssy, fmt, bd_c,
                                    cb_qp_offset if cidx == 1 else cr_qp_offset, tc_off)
            events["cb" if cidx == 1 else "cr", d] = ev
            nxt.append(c.T if t else c)
        cur = nxt
    return cur, events


# ---------------------------------------------------------------- SAO
# Table 8-13
H_POS = {0: (-1, 1), 1: (0, 0), 2: (-1, 1), 3: (1, -1)}
V_POS = {0: (0, 0), 1: (-1, 1), 2: (-1, 1), 3: (-1, 1)}


def band_table(band_position):
    """8.7.3.2: bandTable[(k + sao_band_position) & 31] = k + 1 for k = 0..3"""
    t = [0] * 32
    for k in range(4):
        t[(k + band_position) & 31] = k + 1
    return t


_BAND_TABLES = np.array([band_table(b) for b in range(32)], dtype=np.int64)


def sao_plane(P, cidx, sx, sy, prm, log2ctb, flg, bd):
    """8.7.3 of one component's deblocked plane P (rows, columns); sx, sy: that
    component's subsampling.  prm: type / band_eo (hctb, wctb, 3), off (hctb, wctb, 3, 4)."""
    H, W = P.shape
    P = P.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = yy >> (log2ctb - sy), xx >> (log2ctb - sx)
    typ = prm["type"][cy, cx, cidx].astype(np.int64)
    pos = prm["band_eo"][cy, cx, cidx].astype(np.int64)
    val = np.concatenate([np.zeros((H, W, 1), dtype=np.int64), prm["off"][cy, cx, cidx, :].astype(np.int64)], axis=2)
    nofilt = (flg[(yy << sy) >> 2, (xx << sx) >> 2] & MF_NOFILT) != 0
    band_idx = _BAND_TABLES[pos & 31, P >> (bd - 5)]
    edge_idx = np.zeros((H, W), dtype=np.int64)
    signs = np.full((H, W), NA, dtype=np.int64)
    border = np.full((H, W), NA, dtype=np.int64)
    for cls in range(4):
        s, inside = [], np.ones((H, W), dtype=bool)
        for k in range(2):
            nx, ny = xx + H_POS[cls][k], yy + V_POS[cls][k]
            ok = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
            inside &= ok
            s.append(np.sign(P - P[np.where(ok, ny, 0), np.where(ok, nx, 0)]))
        e = 2 + s[0] + s[1]
        e = np.where(e <= 2, np.where(e == 2, 0, e + 1), e)
        m = (typ == 2) & (pos == cls)
        edge_idx = np.where(m, np.where(inside, e, 0), edge_idx)
        live = m & ~nofilt
        signs = np.where(live & inside, cls * 9 + (s[0] + 1) * 3 + (s[1] + 1), signs)
        at = (yy == 0) * 1 + (yy == H - 1) * 2 + (xx == 0) * 4 + (xx == W - 1) * 8
        border = np.where(live & ~inside, cls * 16 + at, border)
    idx = np.where(typ == 2, edge_idx, np.where(typ == 1, band_idx, 0))
    raw = P + np.take_along_axis(val, idx[:, :, None], axis=2)[:, :, 0]
    res = clip3(0, (1 << bd) - 1, raw)
    out = np.where(nofilt | (typ == 0), P, res)
    live = ~nofilt & (typ != 0)
    ev = {"eo": signs, "eo_border": border,
          "band": np.where(live & (typ == 1) & (band_idx > 0), pos * 4 + band_idx - 1, NA),
          "band_wrap": np.where(live & (typ == 1) & (band_idx > 0), ((P >> (bd - 5)) < pos).astype(np.int64), NA),
          "band_miss": np.where(live & (typ == 1), (band_idx == 0).astype(np.int64), NA),
          "clip": np.where(live & (idx > 0), _sgn(raw, res), NA),
          "type": np.where(nofilt, 3, typ)}
    return out, ev


def sao(planes, flg, prm, log2ctb, fmt, bd_y, bd_c):
    """8.7.3 of every component, each from the deblocked planes only."""
    sx, sy = subsampling(fmt)
    out, events = [], {}
    for cidx, P in enumerate(planes):
        o, ev = sao_plane(P, cidx, sx if cidx else 0, sy if cidx else 0, prm, log2ctb, flg, bd_c if cidx else bd_y)
        out.append(o)
        events[("luma", "cb", "cr")[cidx]] = ev
    return out, events


# ---------------------------------------------------------------- output placement
def visible(out_w, out_h, img_w, img_h, out_x, out_y, fmt):
    """The size k_sao_out writes, per component: the conformance-cropped
    picture clipped by the output image; chroma is the ceiling."""
    sx, sy = subsampling(fmt)
    vw, vh = min(out_w, img_w - out_x), min(out_h, img_h - out_y)
    if vw <= 0 or vh <= 0:
        return [(0, 0)] * (3 if fmt else 1)
    vis = [(vw, vh)]
    if fmt:
        vis += [((vw + (1 << sx) - 1) >> sx, (vh + (1 << sy) - 1) >> sy)] * 2
    return vis


def place(views, planes, conf_l, conf_t, out_w, out_h, img_w, img_h, out_x, out_y, fmt):
    """Writes the visible window of each SAO'ed plane into views[cidx] (the
    caller's plane as a 2-D array of samples, pitch included)."""
    sx, sy = subsampling(fmt)
    for cidx, (vw, vh) in enumerate(visible(out_w, out_h, img_w, img_h, out_x, out_y, fmt)):
        if not vw:
            continue
        kx, ky = (sx, sy) if cidx else (0, 0)
        x0, y0, ox, oy = conf_l >> kx, conf_t >> ky, out_x >> kx, out_y >> ky
        views[cidx][oy:oy + vh, ox:ox + vw] = planes[cidx][y0:y0 + vh, x0:x0 + vw]


def columns(ev):
    """{(name, code): per-unit mask} of an event dict; a per-line event (4 n rows
    against n segments) is not reduced here."""
    cols = {}
    for name, arr in ev.items():
        for code in np.unique(arr):
            if code != NA:
                cols[name, int(code)] = arr == code
    return cols


def seen(ev):
    """the set of (name, code) an event dict holds"""
    return {(name, int(code)) for name, arr in ev.items() for code in np.unique(arr) if code != NA}
