"""Cases for the wide paths of k_sao_out (16-byte groups, packed arithmetic) and k_deblock.

Built from the parts of tests/loopfilter_vectors.py (Pic, Image, Batch, Case and the content
helpers, unchanged); expected bytes come from tests/loopfilter_ref.py alone.  Pictures are at
most 64x48.  `group_paths` restates the rule k_sao_out documents for which samples go through
a 16-byte group, from the case's own layout; nothing here reads the kernels' sources.

  groups  every combination of source aligned or not, destination aligned or not and a ragged
          row end, in each component: widths 32..56, all four chroma formats, 8 and 10 bits,
          conformance-left 0, 2, 4, 8, 16, out_x 0, 4, 8, 16, one picture and one image off the
          16-byte grid
  params  log2_ctb 4, 5, 6; horizontally adjacent CTBs of different kinds (off, band, the four
          edge classes); MF_NOFILT on the first, the last and an inner block of a group
  packs   0 and the maximum side by side, offsets at +-sao_max, 8 / 10 / 12 bits
  words   deblocking: strong filtering everywhere, the normal filter's side decisions,
          MF_NOFILT on one side of every edge, chroma in the three formats
"""
import functools

import numpy as np

import loopfilter_ref as ref
import loopfilter_vectors as lv
from loopfilter_vectors import Batch, Case, Image, Pic

IMAGE_W = 96  # every image: a pitch of 96 samples keeps 16 bytes in luma and in subsampled chroma


def aligned(pics, sz, skews=None):
    """sets each picture's `skew` so that its planes start `skews[k]` samples past a 16-byte
    boundary of the arena (Batch._layout puts a picture on an 8-sample boundary plus its skew)"""
    cur = 0
    for k, p in enumerate(pics):
        cur = (cur + 7 * sz + 8 * sz - 1) // (8 * sz) * (8 * sz)
        want = (skews or {}).get(k, 0)
        p.skew = next(s for s in range(16) if (cur + s * sz) % 16 == (want * sz) % 16)
        cur += p.skew * sz + p.n_samples() * sz
    return pics


def group_paths(b, p):
    """Per component a mask over the picture's samples: 1 through a 16-byte group, 2 through the
    quads and single samples, 0 not visible.  By k_sao_out's rule: a component of a picture is
    eligible when its rows and the caller's pitch are multiples of 16 bytes, the first visible
    column is a multiple of the group (16 bytes of samples), its address and the address it is
    written to are 16-byte aligned, and a CTB of the component is at least a group wide; then
    every whole group of a visible row is wide and the rest of the row is not."""
    im = b.images[p.image]
    g = 16 // b.sz
    masks, base = [], p.recon_off
    for cidx, (vw, vh) in enumerate(ref.visible(p.out_w, p.out_h, im.width, im.height, p.out_x, p.out_y, p.fmt)):
        kx, ky = (p.sx, p.sy) if cidx else (0, 0)
        h, w = p.shape(cidx)
        m = np.zeros((h, w), dtype=np.int8)
        cx0, cy0 = p.conf_l >> kx, p.conf_t >> ky
        src = base + cx0 * b.sz
        dst = b.plane_off[p.image][cidx] + (p.out_y >> ky) * b.pitch[p.image][cidx] + (p.out_x >> kx) * b.sz
        ok = (w * b.sz) % 16 == 0 and b.pitch[p.image][cidx] % 16 == 0 and cx0 % g == 0 and src % 16 == 0 \
            and dst % 16 == 0 and (1 << p.log2_ctb) >> kx >= g and p.bd(cidx) <= 12
        if vw:
            m[cy0:cy0 + vh, cx0:cx0 + vw] = 2
            if ok:
                m[cy0:cy0 + vh, cx0:cx0 + vw // g * g] = 1
        masks.append(m)
        base += h * w * b.sz
    return masks


def alignment_of(b, p, cidx):
    """(source aligned, destination aligned, ragged row end) of a component, as the test counts them"""
    im = b.images[p.image]
    g = 16 // b.sz
    kx, ky = (p.sx, p.sy) if cidx else (0, 0)
    h, w = p.shape(cidx)
    base = p.recon_off + (0 if cidx == 0 else (p.W * p.H + (cidx - 1) * p.cw * p.ch) * b.sz)
    cx0 = p.conf_l >> kx
    src = (base + cx0 * b.sz) % 16 == 0 and cx0 % g == 0 and (w * b.sz) % 16 == 0
    dst = (b.plane_off[p.image][cidx] + (p.out_y >> ky) * b.pitch[p.image][cidx] + (p.out_x >> kx) * b.sz) % 16 == 0 \
        and b.pitch[p.image][cidx] % 16 == 0
    vw = ref.visible(p.out_w, p.out_h, im.width, im.height, p.out_x, p.out_y, p.fmt)[cidx][0]
    return src, dst, vw % g != 0


# ---------------------------------------------------------------- groups
CONF_L = (0, 2, 4, 8, 16)
OUT_X = (0, 4, 8, 16)


def case_groups():
    batches = []
    for fmt in (0, 1, 2, 3):
        for sz, bd in ((1, 8), (2, 10)):
            rng = lv._rng(f"groups{fmt}{sz}")
            pics, images = [], []
            for W in (32, 40, 48, 56):
                # 32 and 48 (whole groups in luma, 32 also in subsampled chroma at 8 bits): every pair, with a
                # whole and with a ragged last group; 40 and 56: a few
                pairs = [(c, o, r) for c in CONF_L for o in OUT_X for r in (0, 3)] if W in (32, 48) else \
                    [(0, 0, 0), (16, 16, 0), (2, 4, 0), (8, 8, 3), (16, 0, 3)]
                for j, (cl, ox, rag) in enumerate(pairs):
                    # (a whole last group in every component: 32 luma samples, or 16 where the window leaves fewer)
                    p = Pic(W, 16, fmt=fmt, bd_y=bd, log2_ctb=5, sao_luma=1, sao_chroma=int(fmt > 0), dbk_disabled=1,
                            conf_l=cl, out_w=W - cl - rag if rag else (32 if W - cl >= 32 else 16), out_x=ox,
                            out_y=(0, 2)[j % 7 == 3],
                            image=len(images), name=f"w{W}_c{cl}_x{ox}_r{rag}")
                    p.planes, p.sao = lv.sao_content(rng, p), lv.rand_sao(rng, p)
                    lv.force_types(p.sao, p.ncomp, 1 + (j & 1))
                    images.append(Image(IMAGE_W, p.out_y + p.out_h))
                    pics.append(p)
            # off the 16-byte grid: one picture's planes, one image's plane pointers, one image's pitch
            odd = []
            for j in range(3):
                p = Pic(48, 16, fmt=fmt, bd_y=bd, sao_luma=1, sao_chroma=int(fmt > 0), dbk_disabled=1,
                        image=len(images), name=f"odd{j}")
                p.planes, p.sao = lv.sao_content(rng, p), lv.rand_sao(rng, p)
                images.append(Image(IMAGE_W, 16, skew=(0, 4, 0)[j], pad=(0, 0, 4)[j]))
                odd.append(len(pics))
                pics.append(p)
            for t in (1, 2):  # one type on every CTB of every component, all of it in whole groups
                p = Pic(32, 16, fmt=fmt, bd_y=bd, log2_ctb=5, sao_luma=1, sao_chroma=int(fmt > 0), dbk_disabled=1,
                        image=len(images), name=f"all{t}")
                p.planes, p.sao = lv.sao_content(rng, p), lv.rand_sao(rng, p)
                p.sao["type"], p.sao["band_eo"] = t * (np.arange(3) < p.ncomp), p.sao["band_eo"] & (3 if t == 2 else 31)
                images.append(Image(IMAGE_W, 16))
                pics.append(p)
            aligned(pics, sz, {odd[0]: 4})
            batches.append(Batch(sz, fmt, pics, images, name=f"groups{fmt}_{bd}"))
    return Case("groups", batches)


# ---------------------------------------------------------------- params
KINDS = ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (2, 3))  # (type, edge class): off, band, the four classes


def kind_params(rng, p, turn):
    """CTB (cy, cx) of component c takes KINDS[(cx + 2 cy + c + turn) % 6]: horizontally adjacent
    CTBs differ, and over six turns every ordered pair of neighbours with step 1 appears"""
    s = lv.rand_sao(rng, p)
    for c in range(p.ncomp):
        for cy in range(p.hctb):
            for cx in range(p.wctb):
                t, cls = KINDS[(cx + 2 * cy + c + turn) % 6]
                s["type"][cy, cx, c] = t
                s["band_eo"][cy, cx, c] = cls if t == 2 else lv.BAND_POSITIONS[(cx + cy + turn) % 5]
    return s


def case_params():
    batches = []
    for sz, bd in ((1, 8), (2, 10)):
        for fmt in (0, 1, 2, 3):
            rng = lv._rng(f"params{fmt}{sz}")
            pics, images = [], []
            for log2_ctb in (4, 5, 6):
                for turn in range(12):  # the second six behind a window offset of 4: no group is aligned
                    p = Pic(64, 48 if log2_ctb == 5 else 16, fmt=fmt, bd_y=bd, log2_ctb=log2_ctb, sao_luma=1,
                            sao_chroma=int(fmt > 0), dbk_disabled=1, conf_l=4 * (turn // 6), image=len(images),
                            name=f"ctb{log2_ctb}_t{turn}")
                    p.planes = lv.sao_content(rng, p) if turn & 1 else lv.band_content(rng, p)
                    p.sao = kind_params(rng, p, turn)
                    # MF_NOFILT on single blocks, about one in five: first, last and inner blocks of groups
                    p.flg = (lv.MF_NOFILT * (rng.integers(0, 5, (p.h4, p.w4)) == 0)).astype(np.uint8)
                    images.append(Image(IMAGE_W, p.out_h))
                    pics.append(p)
            aligned(pics, sz)
            batches.append(Batch(sz, fmt, pics, images, name=f"params{fmt}_{bd}"))
    return Case("params", batches)


# ---------------------------------------------------------------- packs
def extremes(rng, p):
    """0, 1, the maximum and the one below it, drawn per sample: both ends side by side in a pack,
    every sign pair against the neighbours, bands 0 and 31; and the first sample of band 1, which the
    largest offset moves either way without a clip"""
    planes = []
    for c in range(p.ncomp):
        maxv = (1 << p.bd(c)) - 1
        planes.append(rng.choice(np.array([0, 1, maxv - 1, maxv, 1 << (p.bd(c) - 5)]), p.shape(c),
                                 p=(0.3, 0.15, 0.15, 0.3, 0.1)))
    return planes


def case_packs():
    batches = []
    for sz, bds in ((1, (8,)), (2, (10, 12))):
        for fmt in (0, 1, 3):
            rng = lv._rng(f"packs{fmt}{sz}")
            pics, images = [], []
            for bd in bds:
                m = lv.sao_max(bd)
                for j, (t, cls) in enumerate(KINDS[1:] + KINDS[1:]):
                    p = Pic((32, 48)[j & 1], 16, fmt=fmt, bd_y=bd, log2_ctb=4 + (j % 3), sao_luma=1, sao_chroma=int(fmt > 0),
                            dbk_disabled=1, image=len(images), name=f"packs{bd}_{t}{cls}_{j}")
                    p.planes = extremes(rng, p)
                    s = np.zeros((p.hctb, p.wctb), dtype=lv.SAO_DTYPE)
                    s["type"] = t * (np.arange(3) < p.ncomp)
                    # band positions 31 and 0: the bands of 0 and of the maximum carry offsets
                    s["band_eo"] = cls if t == 2 else (31, 0)[j >= 5]
                    # signs so that the clip binds at 0 and at the maximum: edgeIdx 1, 2 (a valley) push a 0
                    # further down in the second half of the pictures, edgeIdx 3, 4 a maximum further up
                    s["off"] = np.array([m, -m, m, -m]) * (1 if j < 5 else -1)
                    p.sao = s
                    images.append(Image(IMAGE_W, 16))
                    pics.append(p)
            aligned(pics, sz)
            batches.append(Batch(sz, fmt, pics, images, name=f"packs{fmt}_{sz}"))
    return Case("packs", batches)


# ---------------------------------------------------------------- words
def one_sided(p):
    """MF_NOFILT on a checkerboard of 8x8 blocks: every edge has exactly one protected side,
    the P side on one edge and the Q side on the next"""
    yy, xx = np.mgrid[0:p.h4, 0:p.w4]
    return (lv.MF_NOFILT * (((yy >> 1) + (xx >> 1)) & 1)).astype(np.uint8)


def case_words():
    batches = []
    for sz, bd in ((1, 8), (2, 10)):
        pics = [lv.strong_everywhere(bd, f"wstrong{bd}")]
        for d in "VH":  # the normal filter's decisions, dEp only and dEq only among them
            pics.append(lv.steered_pic(f"wsteer{bd}{d}", bd, 0, 0, set(), W=(64, 48)[d == "H"], H=32, transpose=d == "H"))
        rng = lv._rng(f"words{bd}")
        for j in range(2):  # one protected side per edge: on strong filtering and on wandering content
            p = lv.strong_everywhere(bd, f"wside{bd}_{j}") if j == 0 else Pic(64, 32, bd_y=bd, name=f"wside{bd}_{j}")
            if j:
                p.planes, p.qpy = lv.blocky(rng, p, amp=1, step=4), lv.rand_qpy(rng, p, 34, 48)
            p.flg = lv.all_edges(p) | one_sided(p)
            pics.append(p)
        batches.append(Batch(sz, 0, pics, lv.one_image_each(pics), name=f"words_luma{bd}"))
        for fmt in (1, 2, 3):
            rng = lv._rng(f"wordsc{fmt}{bd}")
            cp = []
            for j, (W, H) in enumerate(((64, 48), (40, 24), (64, 32))):
                p = Pic(W, H, fmt=fmt, bd_y=bd, cb_off=(3, -4, 0)[j], cr_off=(-2, 5, 1)[j], name=f"wchroma{fmt}_{bd}_{j}")
                p.planes = lv.blocky(rng, p, amp=(3, 6, 3)[j], step=(10, 2, 40)[j], lo=100, hi=150)
                p.qpy = lv.rand_qpy(rng, p, 30, 51)
                # (picture 1: half of the blocks without an edge flag, so that some segments stay as they are)
                p.flg = (lv.all_edges(p) * (rng.integers(0, 2, (p.h4, p.w4)) | (j != 1))).astype(np.uint8) \
                    | (one_sided(p) if j == 2 else 0)
                cp.append(p)
            batches.append(Batch(sz, fmt, cp, lv.one_image_each(cp), name=f"words_c{fmt}_{bd}"))
    return Case("words", batches)


CASES = {"groups": case_groups, "params": case_params, "packs": case_packs, "words": case_words}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()
