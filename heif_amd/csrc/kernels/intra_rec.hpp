// intra_rec.hpp — a TB record's facts as packed words (k_intra's block walk).
//
// When a wave loads 64 TuRecs, one per lane, each lane forms everything a TB's
// prediction needs that depends only on the record and on constants of the CTB
// row; the TB loop then reads the words of one lane (three v_readlane) and
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

// the fields of the words
HG_REC_FN int tba_lx(uint32_t a) { return (int)((a >> TBA_LX_SHIFT) & 63u); }
HG_REC_FN int tba_ly(uint32_t a) { return (int)((a >> TBA_LY_SHIFT) & 63u); }
HG_REC_FN int tba_log2(uint32_t a) { return (int)((a >> TBA_LOG2_SHIFT) & 3u) + 2; }
HG_REC_FN int tba_mode(uint32_t a) { return (int)((a >> TBA_MODE_SHIFT) & 63u); }
HG_REC_FN int tba_cidx(uint32_t a) { return (int)((a >> TBA_CIDX_SHIFT) & 3u); }
HG_REC_FN int tbb_zc(uint32_t b) { return (int)(b & 0xffu); }
HG_REC_FN int tbb_ang(uint32_t b) { return (int)(int8_t)((b >> 8) & 0xffu); }
HG_REC_FN int tbb_inv(uint32_t b) { return (int)(int16_t)(b >> 16); }

}  // namespace hg
