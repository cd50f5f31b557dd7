// intra_rec.hpp — a TB record's facts as packed words (k_intra's block walk).
//
// When a wave loads 64 TuRecs, one per lane, each lane forms everything a TB's
// prediction needs that depends only on the record and on constants of the CTB
// row; the TB loop then reads the words of one lane (a v_readlane each) and
// extracts fields from them, and no TuRec field is decoded on the scalar unit.
//
//   word A  bits  0-5   x of the TB inside its CTB, component samples
//                 6-11  y (a 4:2:2 chroma CTB is 64 high)
//                12-13  log2 size - 2
//                14-19  intra prediction mode (0-34)
//                20-21  cIdx
//                22     cbf          23  PCM
//                24     the neighbours are filtered (8.4.4.2.3)
//                25     a Cb TB whose next record is its Cr TB (set by the caller)
//                26     OK: a valid TB of CTB `ctu` of the row
//                27-28  cbf, PCM of the pair's Cr TB (set by the caller)
//   word B  bits  0-7   zc, the z-order index of the TB's first luma 4x4 block in its CTU (6.4.1)
//                 8-15  intraPredAngle (signed)   16-31  invAngle (signed)
//   word C        the element offset of the TB's first residual from the picture's Y residual plane
//   word D  the TB's neighbours (6.4.1): which of its 4n + 1 reference samples are decoded.  The
//           per-sample rule reduces to five facts (tests/intra_avail/avail_driver.cpp holds them
//           against it over every format, CTB size, TB, picture extent and picture edge):
//           bits  0-3   below-left samples available, in fours (0-8): a prefix, nearest the TB first
//                 4-7   above-right samples available, in fours (0-8): a prefix, left to right
//                 8     the left column (all of it or none)    9  the row above (likewise)
//                10     the corner             (bits 0-10 all zero: nothing is available)
//                11-18  the first available position in the search order of 8.4.4.2.2 (0-128)
//                19-30  the TB's first sample in its window, y * CTB width + x
//
// A record that is not OK packs to zero words: no field of a damaged record
// reaches an index.  Plain inline functions, so the host emulation and a
// stand-alone sanitizer driver run the same bit-fields as the kernel.
#pragma once
#include <stdint.h>

#include "../common/desc.hpp"

#if defined(__HIPCC__) && !defined(HG_HOST_EMU)
#define HG_REC_FN __host__ __device__ __forceinline__
#else
#define HG_REC_FN inline
#endif

namespace hg {

enum : uint32_t {
    TBA_LX_SHIFT = 0, TBA_LY_SHIFT = 6, TBA_LOG2_SHIFT = 12, TBA_MODE_SHIFT = 14, TBA_CIDX_SHIFT = 20,
    TBA_CBF = 1u << 22, TBA_PCM = 1u << 23, TBA_FILT = 1u << 24, TBA_PAIR = 1u << 25, TBA_OK = 1u << 26,
    TBA_CBF2 = 1u << 27, TBA_PCM2 = 1u << 28,
};

// constants of a picture that the pack needs
struct TbGeom {
    int log2ctb;  // CTB size
    int chroma;   // chroma_format_idc
    int W, H;     // luma plane
    int cw, ch;   // chroma planes (0 x 0 for 4:0:0)
};

// bits of bx, by interleaved (bx, by < 16): the z-scan index of a 4x4 block in a CTB of up to 64
HG_REC_FN int tb_zidx(int bx, int by) {
    bx = (bx | (bx << 2)) & 0x33;
    bx = (bx | (bx << 1)) & 0x55;
    by = (by | (by << 2)) & 0x33;
    by = (by | (by << 1)) & 0x55;
    return bx | (by << 1);
}

// Word A of record q in CTB row r (without the pair bits), or 0 where the
// record is not a TB of 8.4.4.2 inside the picture and inside CTB q.ctu.
HG_REC_FN uint32_t tb_pack_a(const TuRec &q, const TbGeom &g, int r) {
    const int k = q.flags & TU_CIDX_MASK;
    const int log2 = q.log2 <= 5 ? q.log2 : 0, n = 1 << log2;  // (a size above 5 never forms a shift)
    const int subx = k ? chroma_sx(g.chroma) : 0, suby = k ? chroma_sy(g.chroma) : 0;
    const int lcx = g.log2ctb - subx, lcy = g.log2ctb - suby;
    const int cx0 = (int)q.ctu << lcx, cy0 = r << lcy;
    const int PW = k ? g.cw : g.W, PH = k ? g.ch : g.H;
    const int lx = (int)q.x - cx0, ly = (int)q.y - cy0;
    const bool ok = k < (g.chroma ? 3 : 1) && q.mode <= 34 && q.log2 >= 2 && q.log2 <= 5 && g.log2ctb <= 6 &&
                    q.x + n <= PW && q.y + n <= PH && lx >= 0 && ly >= 0 && lx + n <= (1 << lcx) &&
                    ly + n <= (1 << lcy);
    if (!ok) return 0u;
    const int m = q.mode;
    const int d26 = m > 26 ? m - 26 : 26 - m, d10 = m > 10 ? m - 10 : 10 - m;
    const int dist = d26 < d10 ? d26 : d10;
    const int thr = n == 8 ? 7 : (n == 16 ? 1 : 0);
    const bool filt = (k == 0 || g.chroma == 3) && m != 1 && n != 4 && dist > thr;
    return ((uint32_t)lx << TBA_LX_SHIFT) | ((uint32_t)ly << TBA_LY_SHIFT) | ((uint32_t)(log2 - 2) << TBA_LOG2_SHIFT) |
           ((uint32_t)m << TBA_MODE_SHIFT) | ((uint32_t)k << TBA_CIDX_SHIFT) | ((q.flags & TU_CBF) ? TBA_CBF : 0u) |
           ((q.flags & TU_PCM) ? TBA_PCM : 0u) | (filt ? TBA_FILT : 0u) | TBA_OK;
}

// the Cr TB's cbf and PCM bits and the pair mark, added to a Cb TB's word A
HG_REC_FN uint32_t tb_pack_pair(uint32_t a, uint32_t cr_flags) {
    return a | TBA_PAIR | ((cr_flags & TU_CBF) ? TBA_CBF2 : 0u) | ((cr_flags & TU_PCM) ? TBA_PCM2 : 0u);
}

// Word B: from word A (zc needs the position and cIdx) and the mode's angles
HG_REC_FN uint32_t tb_pack_b(uint32_t a, const TbGeom &g, int ang, int inv) {
    if (!(a & TBA_OK)) return 0u;
    const int k = (int)((a >> TBA_CIDX_SHIFT) & 3u);
    const int subx = k ? chroma_sx(g.chroma) : 0, suby = k ? chroma_sy(g.chroma) : 0;
    const int lx = (int)((a >> TBA_LX_SHIFT) & 63u), ly = (int)((a >> TBA_LY_SHIFT) & 63u);
    const int zc = tb_zidx((lx << subx) >> 2, (ly << suby) >> 2);
    return (uint32_t)zc | ((uint32_t)(uint8_t)(int8_t)ang << 8) | ((uint32_t)(uint16_t)(int16_t)inv << 16);
}

// Word C: the TB's first residual, in elements from the picture's Y residual
// plane (Cb and Cr follow it).  *fits: the offset is below 2^32.
HG_REC_FN uint32_t tb_pack_c(const TuRec &q, uint32_t a, const TbGeom &g, bool *fits) {
    const int k = (int)((a >> TBA_CIDX_SHIFT) & 3u);
    const uint64_t ysz = (uint64_t)g.W * (uint64_t)g.H, csz = (uint64_t)g.cw * (uint64_t)g.ch;
    const uint64_t plane = k ? ysz + (k == 2 ? csz : 0u) : 0u;
    const uint64_t off = plane + (uint64_t)q.y * (uint64_t)(k ? g.cw : g.W) + q.x;
    *fits = off < (1ull << 32);
    return (a & TBA_OK) ? (uint32_t)off : 0u;
}

enum : uint32_t {
    TBD_BL_SHIFT = 0, TBD_AR_SHIFT = 4, TBD_LEFT = 1u << 8, TBD_ABOVE = 1u << 9, TBD_CORNER = 1u << 10,
    TBD_FACTS = 0x7ffu, TBD_FIRST_SHIFT = 11, TBD_OFF_SHIFT = 19,
};

// word D of a TB of size n from its facts (bl4, ar4: available below-left / above-right samples in fours)
HG_REC_FN uint32_t tbd_make(int n, int bl4, int ar4, bool left, bool above, bool corner, int off) {
    const int first = bl4 ? n - 4 * bl4 : (left ? n : (corner ? 2 * n : (above ? 2 * n + 1 : (ar4 ? 3 * n + 1 : 0))));
    return ((uint32_t)bl4 << TBD_BL_SHIFT) | ((uint32_t)ar4 << TBD_AR_SHIFT) | (left ? TBD_LEFT : 0u) |
           (above ? TBD_ABOVE : 0u) | (corner ? TBD_CORNER : 0u) | ((uint32_t)first << TBD_FIRST_SHIFT) |
           ((uint32_t)off << TBD_OFF_SHIFT);
}

// Word D: from word A (position, size, cIdx), the record's CTB column and the row.  A group of
// neighbours lies in one decoded or undecoded block of the TB's size or in another CTB, so one
// sample decides it; the picture's edge and the CTB's lower and right edges then cut below-left
// and above-right to a prefix (extents are multiples of 8 luma samples: whole fours).
HG_REC_FN uint32_t tb_pack_d(uint32_t a, const TbGeom &g, int ctu, int r) {
    if (!(a & TBA_OK)) return 0u;
    const int k = (int)((a >> TBA_CIDX_SHIFT) & 3u);
    const int subx = k ? chroma_sx(g.chroma) : 0, suby = k ? chroma_sy(g.chroma) : 0;
    const int lsx = g.log2ctb - subx, csx = 1 << lsx, csy = 1 << (g.log2ctb - suby), csl = 1 << g.log2ctb;
    const int x0 = (int)((a >> TBA_LX_SHIFT) & 63u), y0 = (int)((a >> TBA_LY_SHIFT) & 63u);
    const int n = 4 << ((a >> TBA_LOG2_SHIFT) & 3u);
    // columns, rows from the CTB's origin to the picture's edge; -1 where the picture goes on left of / above it
    const int vw = (g.W - (ctu << g.log2ctb)) >> subx, vh = (g.H - (r << g.log2ctb)) >> suby;
    const int minx = ctu > 0 ? -1 : 0, miny = r > 0 ? -1 : 0;
    const int zc = tb_zidx((x0 << subx) >> 2, (y0 << suby) >> 2);
    // 6.4.1 for the neighbour (xn, yn): inside the picture; the CTB row above is decoded up to the CTB
    // above-right and the CTB to the left is decoded, those below and to the right are not; inside the
    // CTB, a 4x4 luma block that precedes the TB's first in z-scan order
    auto avail = [&](int xn, int yn) {
        if (xn < minx || yn < miny || xn >= vw || yn >= vh) return false;
        const int lx = xn * (1 << subx), ly = yn * (1 << suby);
        if (ly < 0) return true;
        if (ly >= csl || lx >= csl) return false;
        if (lx < 0) return true;
        return tb_zidx(lx >> 2, ly >> 2) < zc;
    };
    const int yend = vh < csy ? vh : csy;               // below-left ends at the picture's or the CTB's edge
    const int xend = (y0 == 0 || vw < csx) ? vw : csx;  // above-right: the CTB's edge unless it is the row above
    int bl = avail(x0 - 1, y0 + n) ? yend - (y0 + n) : 0, ar = avail(x0 + n, y0 - 1) ? xend - (x0 + n) : 0;
    bl = bl < n ? bl : n;
    ar = ar < n ? ar : n;
    return tbd_make(n, bl >> 2, ar >> 2, avail(x0 - 1, y0), avail(x0, y0 - 1), avail(x0 - 1, y0 - 1),
                    (y0 << lsx) + x0);
}

// the fields of the words
HG_REC_FN int tbd_bl(uint32_t d) { return (int)((d >> TBD_BL_SHIFT) & 15u) << 2; }  // samples
HG_REC_FN int tbd_ar(uint32_t d) { return (int)((d >> TBD_AR_SHIFT) & 15u) << 2; }
HG_REC_FN int tbd_first(uint32_t d) { return (int)((d >> TBD_FIRST_SHIFT) & 0xffu); }
HG_REC_FN int tbd_off(uint32_t d) { return (int)((d >> TBD_OFF_SHIFT) & 0xfffu); }

// 8.4.4.2.2 on the facts.  Search position s runs 0 .. 4n: the column left of the TB bottom-up
// (below-left first), the corner at 2n, the row above left to right.  The available positions are
// at most three runs: one that ends at n - 1 or 2n - 1, the corner, and one from 2n + 1 or 3n + 1
// to 3n + ar.  The position whose sample stands at s after the substitution is the last
// available position at or below s, or the first available one where there is none: s clamped
// into the run it lies in or behind, then to the first position.  No branch and no lane other
// than s itself.  -1: nothing is available (every sample is 1 << (bitDepth - 1)).
HG_REC_FN int tb_subst_src(int s, int n, uint32_t d) {
    if (!(d & TBD_FACTS)) return -1;
    const int never = 1 << 20, ar = tbd_ar(d);
    const int h1 = ((d & TBD_LEFT) ? 2 * n : n) - 1;  // (an empty first run ends below the first position)
    const int c = (d & TBD_CORNER) ? 2 * n : never;
    const int lo3 = (d & TBD_ABOVE) ? 2 * n + 1 : (ar ? 3 * n + 1 : never), h3 = 3 * n + ar;
    int t = s < h1 ? s : h1;
    t = s >= c ? c : t;
    const int t3 = s < h3 ? s : h3;
    t = s >= lo3 ? t3 : t;
    const int first = tbd_first(d);
    return t > first ? t : first;
}

// the neighbour at search position s, relative to the TB's first sample
HG_REC_FN void tb_search_pos(int s, int n, int *dx, int *dy) {
    *dx = s <= 2 * n ? -1 : s - 2 * n - 1;
    *dy = s < 2 * n ? 2 * n - 1 - s : -1;
}

// Where a TB's neighbours stand in its component's window, as element offsets from the window's
// first sample: the window is the CTB's samples (pitch 1 << lsx), then somewhere behind them the
// column left of the CTB (from row 0) and the row above it (from the corner); `left` and `above`
// are those arrays' offsets.  The column left of the TB is the CTB's left column or the TB's
// neighbour column, the row above it the CTB's row above or the TB's neighbour row.  Positions
// below `split` are on the column, cbase - (s << cshift), the others on the row, rbase + s; the
// corner goes with the column below the CTB's first row (the row above the CTB begins with it).
struct TbSrcAddr {
    int cbase, cshift, rbase, split;
};
HG_REC_FN TbSrcAddr tb_src_addr(int x0, int y0, int n, int lsx, int left, int above) {
    TbSrcAddr a;
    a.cshift = x0 == 0 ? 0 : lsx;
    a.cbase = (x0 == 0 ? left + y0 : (y0 << lsx) + x0 - 1) + ((2 * n - 1) << a.cshift);
    a.rbase = (y0 == 0 ? above + x0 + 1 : ((y0 - 1) << lsx) + x0) - (2 * n + 1);
    a.split = y0 == 0 ? 2 * n : 2 * n + 1;
    return a;
}
HG_REC_FN int tb_src_at(const TbSrcAddr &a, int s) {
    const int c = a.cbase - (s << a.cshift), t = a.rbase + s;
    return s < a.split ? c : t;
}

HG_REC_FN int tba_lx(uint32_t a) { return (int)((a >> TBA_LX_SHIFT) & 63u); }
HG_REC_FN int tba_ly(uint32_t a) { return (int)((a >> TBA_LY_SHIFT) & 63u); }
HG_REC_FN int tba_log2(uint32_t a) { return (int)((a >> TBA_LOG2_SHIFT) & 3u) + 2; }
HG_REC_FN int tba_mode(uint32_t a) { return (int)((a >> TBA_MODE_SHIFT) & 63u); }
HG_REC_FN int tba_cidx(uint32_t a) { return (int)((a >> TBA_CIDX_SHIFT) & 3u); }
HG_REC_FN int tbb_zc(uint32_t b) { return (int)(b & 0xffu); }
HG_REC_FN int tbb_ang(uint32_t b) { return (int)(int8_t)((b >> 8) & 0xffu); }
HG_REC_FN int tbb_inv(uint32_t b) { return (int)(int16_t)(b >> 16); }

}  // namespace hg
