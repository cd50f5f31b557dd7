// parse_units.hpp — the syntax units of the CABAC slice-data parse (H.265
// 7.3.8.2-14 with the derivations below them: 8.4.2 MPM, 8.6.1 QP, 6.5.3-5
// scans, 9.3.4.2 ctxInc), written once over the engine type EG
// (parse_engine.hpp) and run by every parse kernel and by the host emulation
// through run_unit; then the picture and lane setup (pic_init, lane_init).
#pragma once
#include "parse_engine.hpp"

namespace hg {
namespace {

// ------------------------------------------------------------------ derivations
// Table 8-3: IntraPredModeC of 4:2:2 from the 4:2:0-style derivation, 35 modes
// packed four per word as bytes
HG_HD inline int mode422(int m) {
    constexpr uint32_t t[9] = {0x02020100u, 0x05030202u, 0x0b0a0807u, 0x12100f0du, 0x16151413u,
                               0x18181717u, 0x1b1a1919u, 0x1d1c1c1bu, 0x001f1e1du};
    return (int)((t[m >> 2] >> (8 * (m & 3))) & 0xffu);
}

HG_HD inline int chroma_qp_map(int qpi, int chroma) {
    if (chroma != 1) return qpi < 51 ? qpi : 51;
    if (qpi < 30) return qpi;
    if (qpi > 43) return qpi - 6;
    // Table 8-10 for qPi 30..43 (29 30 31 32 33 33 34 34 35 35 36 36 37 37), without a private array
    return qpi < 34 ? qpi - 1 : 33 + ((qpi - 34) >> 1);
}

HG_HD inline void update_qpy(Lane &L, const LanePic &P) {
    L.qpy_cur = ((L.qp_pred + L.cu_qp_delta_val + 52 + 2 * P.qpbdY) % (52 + P.qpbdY)) - P.qpbdY;
}

// 8.6.1 qPY_PRED of the current quantization group
HG_HD inline void derive_qp_pred(Lane &L, const LaneLds &ld, const LanePic &P) {
    int prev;
    const bool first_in_ctb = L.qg_x == L.ctbx && L.qg_y == L.ctby;
    if (L.fl & F_FIRST_QG) {
        prev = P.sliceQp;
        L.fl &= ~F_FIRST_QG;
    } else if ((L.fl & F_WPP) && first_in_ctb && L.c == 0) {
        prev = P.sliceQp;
    } else {
        prev = L.qp_prev_last;
    }
    const int mask = (1 << P.log2ctb) - 1;
    const int qa = (L.qg_x & mask) ? ld.qL[(L.qg_y - L.ctby) >> 3] : prev;
    const int qb = (L.qg_y & mask) ? ld.qA[(L.qg_x - L.ctbx) >> 3] : prev;
    L.qp_pred = (qa + qb + 1) >> 1;
}

// 8.4.2 luma intra prediction mode of the PB at (xPb, yPb), its neighbours read from the lines
HG_HD inline int derive_luma_mode(const Lane &L, const LaneLds &ld, int xPb, int yPb, int prev, int mpm_idx,
                                  int rem) {
    const int ca = xPb <= 0 ? 1 : ld.ipmL[(yPb - L.ctby) >> 2];
    const int cb = (yPb - 1 < L.ctby) ? 1 : ld.ipmA[(xPb - L.ctbx) >> 2];  // above CTB (or picture edge) → DC
    int l0, l1, l2;
    if (ca == cb) {
        if (ca < 2) {
            l0 = 0;
            l1 = 1;
            l2 = 26;
        } else {
            l0 = ca;
            l1 = 2 + ((ca + 29) % 32);
            l2 = 2 + ((ca - 2 + 1) % 32);
        }
    } else {
        l0 = ca;
        l1 = cb;
        if (ca != 0 && cb != 0) l2 = 0;
        else if (ca != 1 && cb != 1) l2 = 1;
        else l2 = 26;
    }
    if (prev) return mpm_idx == 0 ? l0 : (mpm_idx == 1 ? l1 : l2);
    int t;
    if (l0 > l1) { t = l0; l0 = l1; l1 = t; }
    if (l0 > l2) { t = l0; l0 = l2; l2 = t; }
    if (l1 > l2) { t = l1; l1 = l2; l2 = t; }
    int m = rem;
    if (m >= l0) ++m;
    if (m >= l1) ++m;
    if (m >= l2) ++m;
    return m;
}
// the same from candIntraPredModeA / B themselves (the vector engines keep a CU's neighbours in
// registers).  A copy, not the function above calling this one: its code in the scalar kernels changes otherwise
HG_HD inline int luma_mode(int ca, int cb, int prev, int mpm_idx, int rem) {
    int l0, l1, l2;
    if (ca == cb) {
        if (ca < 2) {
            l0 = 0;
            l1 = 1;
            l2 = 26;
        } else {
            l0 = ca;
            l1 = 2 + ((ca + 29) % 32);
            l2 = 2 + ((ca - 2 + 1) % 32);
        }
    } else {
        l0 = ca;
        l1 = cb;
        if (ca != 0 && cb != 0) l2 = 0;
        else if (ca != 1 && cb != 1) l2 = 1;
        else l2 = 26;
    }
    if (prev) return mpm_idx == 0 ? l0 : (mpm_idx == 1 ? l1 : l2);
    int t;
    if (l0 > l1) { t = l0; l0 = l1; l1 = t; }
    if (l0 > l2) { t = l0; l0 = l2; l2 = t; }
    if (l1 > l2) { t = l1; l1 = l2; l2 = t; }
    int m = rem;
    if (m >= l0) ++m;
    if (m >= l1) ++m;
    if (m >= l2) ++m;
    return m;
}

// The vector engines update a CU's or PB's segment of the CtDepth and IntraPredModeY lines
// (an aligned run of 1, 2, 4, 8 or 16 bytes) as a masked 64-bit word, not byte by byte: a
// byte loop's trip count differs by lane, and every lane of the unit run waits for the
// longest (the QpY lines stay byte loops, cu_done).  HG_LINE_BYTES (tuning
// builds) keeps the byte loops of the lines named in its bits: 1 CtDepth, 2 IntraPredModeY.
#if !defined(HG_LINE_BYTES)
#define HG_LINE_BYTES 0
#endif
template <class EG>
constexpr bool kLineWords(int which) { return !EG::kSolo && !(HG_LINE_BYTES & which); }
HG_HD inline uint64_t line_ld(const void *line) {
    uint64_t w;
    __builtin_memcpy(&w, line, 8);
    return w;
}
HG_HD inline void line_st(void *line, uint64_t w) { __builtin_memcpy(line, &w, 8); }
// bytes [b0, b0 + nb) of an 8-byte line := v; nb = 1, 2, 4 or 8
// (~0 >> (64 - 8 nb): no shift by 64 when the run fills the word)
HG_HD inline void line8_fill(void *line, int b0, int nb, int v) {
    const uint64_t m = (~0ull >> (64 - 8 * nb)) << (8 * b0);
    line_st(line, (line_ld(line) & ~m) | ((0x0101010101010101ull * (uint8_t)v) & m));
}
// bytes [b0, b0 + nb / 2) of a 16-byte line := lo, [b0 + nb / 2, b0 + nb) := hi; nb = 2, 4, 8 or 16;
// w: the word holding byte b0 as it is now (a 16-byte run fills both words)
HG_HD inline void line16_fill(uint8_t *line, uint64_t w, int b0, int nb, int lo, int hi) {
    const uint64_t rl = 0x0101010101010101ull * (uint8_t)lo, rh = 0x0101010101010101ull * (uint8_t)hi;
    if (nb == 16) {
        line_st(line, rl);
        line_st(line + 8, rh);
        return;
    }
    const int h = 4 * nb, sh = 8 * (b0 & 7);  // bits of a half (at most 32), of the run's offset
    const uint64_t hm = (1ull << h) - 1, m = ~0ull >> (64 - 8 * nb);
    line_st(line + (b0 & 8), (w & ~(m << sh)) | (((rl & hm) | ((rh & hm) << h)) << sh));
}

// 6.5.3-6.5.5 scans.  Packed 4-bit 2x2 / 4x4 scans (entry x | (y << 2)) are
// selected, not indexed, so they stay immediates; the 8x8 sub-block scan of
// 32x32 TBs comes from the table.  scan_pos returns x | (y << 4).
HG_HD inline uint64_t scan4_word(int scan) { return scan == 0 ? kScan4Pos[0] : (scan == 1 ? kScan4Pos[1] : kScan4Pos[2]); }
template <class EG>
HG_HD inline int scan_pos(const EG &G, int l, int scan, int i) {
    if (l == 3) return G.scan8(scan, i);
    if (l == 0) return 0;
    const uint64_t t = l == 2 ? scan4_word(scan) : (scan == 0 ? kScan2Pos[0] : (scan == 1 ? kScan2Pos[1] : kScan2Pos[2]));
    const uint32_t e = (uint32_t)(t >> (4 * i)) & 15u;
    return (int)((e & 3) | ((e >> 2) << 4));
}
template <class EG>
HG_HD inline int scan_inv(const EG &G, int l, int scan, int raster) {
    if (l == 3) return G.scan8_inv(scan, raster);
    if (l == 0) return 0;
    const uint64_t t = l == 2 ? (scan == 0 ? kScan4Inv[0] : (scan == 1 ? kScan4Inv[1] : kScan4Inv[2]))
                              : (scan == 0 ? kScan2Inv[0] : (scan == 1 ? kScan2Inv[1] : kScan2Inv[2]));
    return (int)((uint32_t)(t >> (4 * raster)) & 15u);
}

// sig_coeff_flag ctxInc patterns (9.3.4.2.5) per prevCsbf, as one nibble per raster position
// e = x | (y << 2), each + 1 (slot of the sub-block's context cache)
constexpr uint64_t sig_pat_nib(int pc) {
    uint64_t w = 0;
    for (int e = 0; e < 16; ++e) {
        const int x = e & 3, y = e >> 2;
        const int v = pc == 0 ? (x + y == 0 ? 2 : (x + y < 3 ? 1 : 0))
                    : pc == 1 ? (y == 0 ? 2 : (y == 1 ? 1 : 0))
                    : pc == 2 ? (x == 0 ? 2 : (x == 1 ? 1 : 0)) : 2;
        w |= (uint64_t)(v + 1) << (4 * e);
    }
    return w;
}
HG_HD inline uint64_t sig_slots(int pcs) {
    return pcs == 0 ? sig_pat_nib(0) : pcs == 1 ? sig_pat_nib(1) : pcs == 2 ? sig_pat_nib(2) : sig_pat_nib(3);
}
HG_HD inline int msb32(uint32_t m) { return 31 - __builtin_clz(m); }

// context slot of sig_coeff_flag per scan position n of a 4x4 sub-block
// (nibble n), for scanIdx 0..2 and slot pattern 0..3 (prevCsbf, sizes > 4x4)
// or 4 (ctxIdxMap, 4x4 TBs): 15 words, computed into LDS at kernel start
HG_HD inline uint64_t sig_seq(int idx) {
    const int scan = idx / 5, pat = idx % 5;
    const uint64_t slots = pat == 4 ? kSigCtxMap4 : sig_slots(pat);
    const uint64_t sw = scan4_word(scan);
    uint64_t q = 0;
    for (int n = 0; n < 16; ++n) {
        const int e = (int)((sw >> (4 * n)) & 15u);
        q |= ((slots >> (4 * e)) & 15u) << (4 * n);
    }
    return q;
}

// the 8x8 diagonal scan of 32x32 TBs (kScanPos[3][0]) and its inverse into LDS, one entry per lane
HG_HD inline void scan8_tables(uint8_t *t, int lane) {
    t[lane] = kScanPos[3][0][lane];
    t[64 + lane] = kScanInv[3][0][lane];
}

struct Env {
    const BatchArgs *a;
    LaneLds *lds;    // the wave's 64 lane blocks
    uint32_t *prog;  // [64] row * wctb + CTUs finished in the lane's current row
    uint8_t *wctx;   // [64][CTX_PAD] WPP context staging of wrapping pictures (null when none wraps)
    int lane;
};

// WPP context staging block read at the start of substream `row` (written
// after CTU 1 of row - 1): per picture with job lanes (one block is enough:
// row r + 1 writes it only after its own start, and row r + 2 cannot start
// before that), else per row slot (lane / wave / spread row)
HG_HD inline uint8_t *wpp_stage(const Env &E, const LanePic &P, int row) {
    return E.wctx + (size_t)(P.lane0 + row % P.R) * CTX_PAD;
}
// progress word of substream `row` (monotone row * wctb + CTUs done, so a
// slot shared by rows r and r + R never runs backwards)
HG_HD inline uint32_t *prog_word(const Env &E, const LanePic &P, int row) { return &E.prog[P.lane0 + row % P.R]; }

// WPP, for parsing: a row's first CTU needs the contexts stored after CTU 1
// of the row above (9.3.1), so two CTUs of it done; CTU c > 0 only reads the
// CTU above it (split_cu_flag's CtDepth, sao_merge_up_flag; intra modes and
// QP prediction stay inside the CTB row), so one CTU ahead is enough.  The
// 2-CTU lag of the reconstruction (above-right neighbours) is k_intra's.
template <class EG>
HG_HD inline bool wpp_ready(const Lane &L, const LanePic &P, const Env &E) {
    if (!(L.fl & F_WPP) || L.row == 0) return true;
    const int ahead = L.c == 0 ? 2 : L.c + 1;
    const uint32_t need = (uint32_t)(L.row - 1) * (uint32_t)P.wctb + (uint32_t)(ahead < P.wctb ? ahead : P.wctb);
    const uint32_t *pw = prog_word(E, P, L.row - 1);
    return (EG::kSpread ? load_agent(pw) : prog_load(pw)) >= need;
}

// RBSP offset (absolute) at which a lane about to run U_CTU starts its
// substream (engine and context initialisation, unit_ctu), or ~0u
// dependent slice segments starting inside a CTB row of picture P (PicDesc.flags)
template <class EG>
HG_HD inline uint32_t lanes_nmid(const LanePic &P) { return (pic_flags<EG>(P) >> PD_NMID_SHIFT) & PD_NMID_MAX; }

// (Mid: the lanes engine, which takes dependent segments starting inside a
// row; the scalar engines do not, parse_mode_for gives such batches the lanes parse)
template <class EG>
HG_HD inline uint32_t substream_start(const Lane &L, const LanePic &P, const BatchArgs &a) {
    if (L.c != 0) {
        if constexpr (!EG::kSolo && !EG::kLean) {
            if (L.status & ST_SEGSW) {
                // a dependent segment starting inside the row (the picture's row
                // entries, the end entry, then these); past the picture's
                // list (a corrupt stream, flagged by unit_ctu): the RBSP end
                const uint32_t m = L.fl >> kMsegShift;
                return P.bits_off +
                       (a.rsubs[P.sub_first + (uint32_t)P.hctb + (m < lanes_nmid<EG>(P) ? 1u + m : 0u)] & SUB_OFFSET);
            }
        }
        return ~0u;
    }
    if ((L.fl & F_WPP) || L.row == 0)
        return P.bits_off + (a.rsubs[P.sub_first + ((L.fl & F_WPP) ? L.row : 0)] & SUB_OFFSET);
    if (pic_flags<EG>(P) & SP_ROW_SEGMENTS) {  // no WPP: a dependent slice segment may start at this row
        const uint32_t e = a.rsubs[P.sub_first + L.row];
        if (!(e & SUB_CONTINUE)) return P.bits_off + (e & SUB_OFFSET);
    }
    return ~0u;
}

HG_HD inline void row_outputs(Lane &L, const LanePic &P) {
    L.tu_row = (uint32_t)L.row * P.tu_cap;
    L.coef_row = (uint32_t)L.row * P.coef_cap;
    L.ntu = L.ncoef = L.nesc = 0;
}

// one coefficient, one 4-byte store.  (Grouping four into a 16-byte store
// through registers measured 5 % slower: the selects run on every lane of
// every coefficient step, the saved stores were cheap.)
template <class EG>
HG_HD inline void coef_push(Lane &L, const LanePic &P, uint32_t w) {
    if (pic_flags<EG>(P) & PF_COHERENT) store_word_agent((uint32_t *)(P.coef_base + L.coef_row + L.ncoef++), w);
    else P.coef_base[L.coef_row + L.ncoef++] = w;
}

// ------------------------------------------------------------------ units
// U_CTU: CTU start (7.3.8.2) and sao() (7.3.8.3).  Returns without a state
// change while the row above is less than two CTUs ahead (WPP).
template <class EG>
HG_HD inline void unit_ctu(Lane &L, LaneLds &ld, LanePic &P, const Env &E, const EG &G) {
    if (!wpp_ready<EG>(L, P, E)) return;
    L.ctbx = L.c << P.log2ctb;
    L.ctby = L.row << P.log2ctb;
    const uint32_t start = substream_start<EG>(L, P, *E.a);
    if (HG_UNLIKELY(start != ~0u)) {
        // substream start: contexts (init; the WPP copy already in ld.ctx; or, a
        // dependent slice segment without WPP, the previous segment's final
        // state, which the lane still holds: 9.3.2.4) + engine.  A dependent
        // segment starting inside a row (ST_SEGSW) keeps the contexts and qPY_PREV
        const bool segsw = !EG::kSolo && !EG::kLean && (L.status & ST_SEGSW) != 0;
        const bool init = !segsw && (L.row == 0 || ((L.fl & F_WPP) && P.wctb < 2));
        const bool wpp_copy = !init && (L.fl & F_WPP);
        if constexpr (EG::kCtxReg) {
#if !defined(HG_HOST_EMU)
            // every lane its dword of the contexts: initialised, or the row above's copy
            const int ln = (int)__lane_id();
            uint32_t w = L.cx;
            if (init) {
                w = 0;
                for (int b = 0; b < 4; ++b) {
                    const int i = 4 * ln + b;
                    if (i < CTX_NUM) w |= (uint32_t)ctx_init_state(c_ctx_init_l[i], P.sliceQp) << (8 * b);
                }
            } else if (wpp_copy) {
                w = 0;
                if (ln < CTX_PAD / 4) {
                    const uint8_t *src = (EG::kSpread || pic_ring<EG>(P)) ? wpp_stage(E, P, L.row) : ld.ctx;
                    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src) + ln;
                    w = EG::kSpread ? load_agent(sw) : *sw;
                }
            }
            L.cx = w;
#endif
        } else if (init) {
#pragma nounroll
            for (int i = 0; i < CTX_NUM; ++i) ld.ctx[i] = ctx_init_state(c_ctx_init_l[i], P.sliceQp);
        } else if (wpp_copy && (EG::kSpread || pic_ring<EG>(P))) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(wpp_stage(E, P, L.row));
            uint32_t *dst = reinterpret_cast<uint32_t *>(ld.ctx);
#pragma nounroll
            for (int k = 0; k < CTX_PAD / 4; ++k) dst[k] = EG::kSpread ? load_agent(src + k) : src[k];
        }
        engine_init(L, G, start, P.bits_end);
        if (segsw) {
            L.status &= ~ST_SEGSW;
            if ((L.fl >> kMsegShift) >= lanes_nmid<EG>(P)) L.status |= ST_SUBSTREAM_END;  // no such segment
            L.fl += kMsegOne;
        } else {
            if (L.row == 0) L.fl |= F_FIRST_QG;
            if constexpr (!EG::kSolo) {
                // WPP: this row's lane counts the segments started inside rows from
                // those of earlier rows (batch.cpp: after the picture's mid list)
                const uint32_t nm = lanes_nmid<EG>(P);
                if ((L.fl & F_WPP) && nm)
                    L.fl = (L.fl & (kMsegOne - 1)) |
                           (E.a->subs[P.sub_first + (uint32_t)P.hctb + 1u + nm + L.row] << kMsegShift);
            }
        }
    }
    if (P.saoL || P.saoC) {
        int ml = 0, mu = 0;
        if (L.c > 0) ml = dec(L, G, CTX_SAO_MERGE);
        if (L.row > 0 && !ml) mu = dec(L, G, CTX_SAO_MERGE);
        // the CTB's SaoParams as 8 words (desc.hpp layout), built in registers:
        // no per-lane LDS copy (merge-left re-reads the left CTB's entry, which
        // this lane stored one CTU earlier)
        uint32_t *dst = reinterpret_cast<uint32_t *>(P.gsao + (size_t)L.row * P.wctb + L.c);
        uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, w6 = 0, w7 = 0;
        if (ml || mu) {
            const uint32_t *src = ml ? dst - 8 : reinterpret_cast<const uint32_t *>(P.gsao + (size_t)(L.row - 1) * P.wctb + L.c);
            w0 = load_word_coherent(src + 0);
            w1 = load_word_coherent(src + 1);
            w2 = load_word_coherent(src + 2);
            w3 = load_word_coherent(src + 3);
            w4 = load_word_coherent(src + 4);
            w5 = load_word_coherent(src + 5);
            w6 = load_word_coherent(src + 6);
            w7 = load_word_coherent(src + 7);
        } else {
            // byte b of the 32-byte record (every offset below is a constant after unrolling)
            auto put8 = [&](int b, uint32_t v) {
                const uint32_t m = (v & 0xffu) << (8 * (b & 3));
                switch (b >> 2) {
                case 0: w0 |= m; break;
                case 1: w1 |= m; break;
                case 2: w2 |= m; break;
                case 3: w3 |= m; break;
                case 4: w4 |= m; break;
                case 5: w5 |= m; break;
                case 6: w6 |= m; break;
                default: w7 |= m; break;
                }
            };
            auto put16 = [&](int b, int v) {
                put8(b, (uint32_t)v);
                put8(b + 1, (uint32_t)v >> 8);
            };
            const int ncomp = HG_PIC_CHROMA(P) ? 3 : 1;
            int type1 = 0, eo1 = 0;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                if (cc >= ncomp) break;
                if (!((P.saoL && cc == 0) || (P.saoC && cc > 0))) continue;
                const int type = cc < 2 ? (dec(L, G, CTX_SAO_TYPE) ? (byp(L, G) ? 2 : 1) : 0) : type1;
                if (cc == 1) type1 = type;
                put8(cc, (uint32_t)type);
                if (!type) continue;
                const int bd = cc ? P.bdC : P.bdY;
                const int cmax = (1 << ((bd < 10 ? bd : 10) - 5)) - 1;
                int o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {  // TR(cMax), bypass
                    int v = 0;
                    while (v < cmax && byp(L, G)) ++v;
                    o[i] = v;
                }
                int band_eo;
                if (type == 1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (o[i] && byp(L, G)) o[i] = -o[i];
                    band_eo = (int)byp_bits(L, G, 5);
                } else {
                    band_eo = cc < 2 ? (int)byp_bits(L, G, 2) : eo1;
                    if (cc == 1) eo1 = band_eo;
                    o[2] = -o[2];
                    o[3] = -o[3];
                }
                put8(3 + cc, (uint32_t)band_eo);
#pragma unroll
                for (int i = 0; i < 4; ++i) put16(6 + 8 * cc + 2 * i, o[i]);
            }
        }
        const uint32_t w[8] = {w0, w1, w2, w3, w4, w5, w6, w7};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if constexpr (EG::kSpread) store_agent(dst + k, w[k]);
            else dst[k] = w[k];
        }
    }
    L.qx = L.ctbx, L.qy = L.ctby, L.ql = P.log2ctb, L.qd = 0;
    L.st = U_CQT;
}

// U_CQT: split_cu_flag descent (7.3.8.4) from the current node to a CU
template <class EG>
HG_HD inline void unit_cqt(Lane &L, LaneLds &ld, LanePic &P, const EG &G) {
    HG_CU_T0(tcq);
    for (;;) {
        const int n = 1 << L.ql;
        bool split;
        if (L.qx + n <= P.W && L.qy + n <= P.H && L.ql > P.minCb) {
            int cond = 0;  // 9.3.4.2.2 ctxInc of split_cu_flag
            if (L.qx > 0 && ld.dL[(L.qy - L.ctby) >> 3] > L.qd) ++cond;
            if (L.qy > 0) {
                const int ad = (L.qy - 1 < L.ctby)
                                   ? load_byte_coherent(P.gdepth + (size_t)(L.row - 1) * P.w8 + (L.qx >> 3))
                                   : ld.dA[(L.qx - L.ctbx) >> 3];
                if (ad > L.qd) ++cond;
            }
            split = dec(L, G, CTX_SPLIT_CU + cond) != 0;
        } else {
            split = L.ql > P.minCb;
        }
        if (L.ql >= P.log2qg) {
            L.fl = (L.fl & ~F_DQP_CODED) | F_QG_NEW;
            L.cu_qp_delta_val = 0;
            L.qg_x = L.qx;
            L.qg_y = L.qy;
        }
        if (!split) break;
        --L.ql;  // child 0 (always inside the picture)
        ++L.qd;
    }
    HG_CU_T(L, 0, tcq);
    L.st = U_CU;
}

template <class EG>
HG_HD inline void cu_done(Lane &L, LaneLds &ld, LanePic &P);
template <class EG>
HG_HD inline void tu_emit(Lane &L, const LanePic &P);

// pcm_flag = 1 (7.3.8.7 pcm_sample(); the reference parses the SPS PCM fields,
// parameter_set_reader.rs:107-125): the decoder has consumed through the
// codeword's final 1 bit, the samples start at the next byte boundary
// (pcm_alignment_zero_bits).  They are recorded as bypass TBs (TU_PCM) whose
// "coefficients" are the samples << (BitDepth - PcmBitDepth) in raster order:
// k_transform copies them and k_intra adds them to a zero prediction.  The
// engine restarts at the byte after them (9.3.2.5).  The CU counts as
// INTRA_DC for later MPM derivations (8.4.2) and is one deblocking block,
// unfiltered with pcm_loop_filter_disabled_flag.
template <class EG>
HG_HD inline void pcm_cu(Lane &L, LaneLds &ld, LanePic &P, const EG &G) {
    const int n = 1 << L.ql;
    {
        const int nb = n >> 2, by = (L.qy - L.ctby) >> 2, bx = (L.qx - L.ctbx) >> 2;
        if constexpr (kLineWords<EG>(2)) {
            line16_fill(ld.ipmL, line_ld(ld.ipmL + (by & 8)), by, nb, 1, 1);
            line16_fill(ld.ipmA, line_ld(ld.ipmA + (bx & 8)), bx, nb, 1, 1);
        } else {
            for (int k = 0; k < nb; ++k) {
                ld.ipmL[by + k] = 1;
                ld.ipmA[bx + k] = 1;
            }
        }
    }
    // bits consumed so far: 8 * end - budget - k (absolute RBSP bit position)
    uint32_t bit = (uint32_t)(8 * (int32_t)P.bits_end - L.budget - L.k + 7) & ~7u;
    L.fl = (L.fl | F_PCM | F_TB_CBF) & ~F_TS;
    // luma, then Cb and Cr; a 4:2:2 chroma block (raster, m wide, 2m tall) is
    // two stacked square TBs
    const int ntb = HG_PIC_CHROMA(P) == 0 ? 1 : (HG_PIC_CHROMA(P) == 2 ? 5 : 3), nh = HG_PIC_CHROMA(P) == 2 ? 2 : 1;
    for (int t = 0; t < ntb; ++t) {
        const int c = t == 0 ? 0 : 1 + (t - 1) / nh, h = t == 0 ? 0 : (t - 1) % nh;
        const int l2 = (c && HG_PIC_CHROMA(P) != 3) ? L.ql - 1 : L.ql, m = 1 << l2;
        const int pbd = c ? P.pcmBdC : P.pcmBdY, sh = (c ? P.bdC : P.bdY) - pbd;
        L.tb_cidx = c;
        L.tb_x = c ? L.qx >> HG_PIC_SUBX(P) : L.qx;
        L.tb_y = c ? (L.qy >> HG_PIC_SUBY(P)) + (h << l2) : L.qy;
        L.tb_log2 = l2;
        L.tb_mode = 1;
        L.tb_coef0 = L.ncoef;
#pragma nounroll
        for (int i = 0; i < m * m; ++i) {
            // clamped to the substream's padded end: a truncated stream reads padding
            // (and reports ST_OVERRUN below), never past the arena
            const uint32_t b = (bit >> 3) < G.lim ? bit >> 3 : G.lim;
            const uint32_t w = ((uint32_t)G.rbsp[b] << 16) | ((uint32_t)G.rbsp[b + 1] << 8) | (uint32_t)G.rbsp[b + 2];
            const uint32_t v = (w >> (24u - (bit & 7u) - (uint32_t)pbd)) & ((1u << pbd) - 1u);
            bit += (uint32_t)pbd;
            if (L.ncoef + L.nesc < P.coef_cap) coef_push<EG>(L, P, ((v << sh) << 16) | (uint32_t)i);
            else L.status |= ST_CAPACITY;
        }
        tu_emit<EG>(L, P);
    }
    L.fl &= ~(F_PCM | F_TB_CBF);
    {  // the CU's 4x4 blocks: one block for the deblocking edges
        const int nb = n >> 2, gx0 = L.qx >> 2, gy0 = L.qy >> 2;
        const int wx = gx0 + nb <= P.w4 ? nb : P.w4 - gx0, hy = gy0 + nb <= P.h4 ? nb : P.h4 - gy0;
        const uint64_t nf = ((L.fl & F_BYPASS) || (pic_flags<EG>(P) & SP_PCM_LOOP_FILTER_DISABLED)) ? MF_NOFILT : 0;
        const uint64_t rep = 0x0101010101010101ull;
        for (int y = 0; y < hy; ++y) {
            uint8_t *row = P.gflags + (size_t)(gy0 + y) * P.w4 + gx0;
            const uint64_t h = (y == 0 ? (uint64_t)MF_EDGE_H : 0u) | nf;
            store_bytes(row, wx, (rep * h) | (uint64_t)MF_EDGE_V);
        }
    }
    const uint32_t next = bit >> 3;  // the samples end on a byte boundary
    if (next > P.bits_end) L.status |= ST_OVERRUN;
    if constexpr (EG::kSolo) {  // the driver moves the window first (run_unit re-initialises)
        L.reinit = next;
        L.lb = next >> 2;
        L.fl |= F_REINIT;
    } else {
        engine_init(L, G, next, P.bits_end);
    }
    cu_done<EG>(L, ld, P);
}

// U_CU: coding_unit (7.3.8.5) up to its transform_tree
template <class EG>
HG_HD inline void unit_cu(Lane &L, LaneLds &ld, LanePic &P, const EG &G) {
    HG_CU_T0(tcu);
    if (L.fl & F_QG_NEW) {
        derive_qp_pred(L, ld, P);
        L.fl &= ~F_QG_NEW;
    }
    update_qpy(L, P);
    L.fl &= ~(F_BYPASS | F_NXN);
    if ((pic_flags<EG>(P) & SP_TQ_BYPASS) && dec(L, G, CTX_TQ_BYPASS)) L.fl |= F_BYPASS;
    if (L.ql == P.minCb && !dec(L, G, CTX_PART_MODE)) L.fl |= F_NXN;
    const bool nxn = (L.fl & F_NXN) != 0;
    const bool pcm = !nxn && (pic_flags<EG>(P) & SP_PCM) && L.ql >= P.pcmMin && L.ql <= P.pcmMax && term(L, G);
    HG_CU_T(L, 1, tcu);
    {  // CtDepth of the CU
        const int nd = 1 << (L.ql - 3);
        const int dy = (L.qy - L.ctby) >> 3, dx = (L.qx - L.ctbx) >> 3;
        if constexpr (kLineWords<EG>(1)) {
            line8_fill(ld.dL, dy, nd, L.qd);
            line8_fill(ld.dA, dx, nd, L.qd);
        } else {
            for (int k = 0; k < nd; ++k) {
                ld.dL[dy + k] = (uint8_t)L.qd;
                ld.dA[dx + k] = (uint8_t)L.qd;
            }
        }
    }
    HG_CU_T(L, 2, tcu);
    if constexpr (!EG::kLean) {
        if (pcm) {
            pcm_cu(L, ld, P, G);
            return;
        }
    }
    const int np = nxn ? 4 : 1;
    const int pb = nxn ? 1 << (L.ql - 1) : 1 << L.ql;
    if (nxn) HG_COV(COV_NXN);
    int prev = 0;
    if constexpr (!EG::kSolo) {
        // the 1 or 4 bins share one context: read once, decided in a register, stored once
        uint32_t t = ctx_ld(L, G, CTX_PREV_INTRA);
        for (int i = 0; i < np; ++i) prev |= dec_t(L, G, t & 0x7fu, t) << i;
        ctx_st(L, G, CTX_PREV_INTRA, t & 0x7fu);
    } else {
        for (int i = 0; i < np; ++i) prev |= dec(L, G, CTX_PREV_INTRA) << i;
    }
    int modes = 0;
    // vector engines: the CU's words of the two lines, read once.  PB i + 1's neighbours inside
    // the CU are PB i's modes (in `modes`), so no PB waits for an LDS round trip of the one
    // before; the lines are written back once, after the last PB
    const int nbc = 1 << (L.ql - 2), byc = (L.qy - L.ctby) >> 2, bxc = (L.qx - L.ctbx) >> 2;
    uint64_t wl = 0, wa = 0;
    int nl1 = 1, na1 = 1;  // the lower PBs' left and the right PBs' above neighbour (NxN)
    if constexpr (kLineWords<EG>(2)) {
        wl = line_ld(ld.ipmL + (byc & 8));
        wa = line_ld(ld.ipmA + (bxc & 8));
        if (nxn) {  // (a 64x64 NxN CU's second halves lie in the lines' second words)
            nl1 = nbc == 16 ? ld.ipmL[8] : (int)(wl >> (8 * ((byc & 7) + (nbc >> 1)))) & 0xff;
            na1 = nbc == 16 ? ld.ipmA[8] : (int)(wa >> (8 * ((bxc & 7) + (nbc >> 1)))) & 0xff;
        }
    }
    for (int i = 0; i < np; ++i) {
        const int p = (prev >> i) & 1;
        int mpm = 0, rem = 0;
        if constexpr (EG::kSolo) {
            if (p) mpm = byp(L, G) ? (byp(L, G) ? 2 : 1) : 0;
            else rem = (int)byp_bits(L, G, 5);
        } else {
            mpm = rem = byp_luma_mode(L, G, p);
        }
        if (nxn) HG_COV(p ? COV_NXN_MPM + mpm : COV_NXN_REM);
        HG_CU_T(L, 3, tcu);
        if constexpr (kLineWords<EG>(2)) {
            // left: PB i - 1 (right column), else the line (DC at the picture's edge);
            // above: PB i - 2 (lower row), else the line (DC above the CTB)
            const int ca = (i & 1) ? (modes >> (8 * (i - 1))) & 0xff
                                   : (L.qx <= 0 ? 1 : (i ? nl1 : (int)(wl >> (8 * (byc & 7))) & 0xff));
            const int cb = (i & 2) ? (modes >> (8 * (i - 2))) & 0xff
                                   : (L.qy - 1 < L.ctby ? 1 : (i ? na1 : (int)(wa >> (8 * (bxc & 7))) & 0xff));
            modes |= luma_mode(ca, cb, p, mpm, rem) << (8 * i);
        } else {
            const int xPb = L.qx + (i & 1) * pb, yPb = L.qy + (i >> 1) * pb;
            const int m = derive_luma_mode(L, ld, xPb, yPb, p, mpm, rem);
            modes |= m << (8 * i);
            const int nb = pb >> 2, by = (yPb - L.ctby) >> 2, bx = (xPb - L.ctbx) >> 2;
            for (int k = 0; k < nb; ++k) {
                ld.ipmL[by + k] = (uint8_t)m;
                ld.ipmA[bx + k] = (uint8_t)m;
            }
        }
        HG_CU_T(L, 4, tcu);
    }
    if constexpr (kLineWords<EG>(2)) {
        // last written per row: the right PBs (1, 3); per column: the lower PBs (2, 3)
        const int m0 = modes & 0xff;
        line16_fill(ld.ipmL, wl, byc, nbc, nxn ? (modes >> 8) & 0xff : m0, nxn ? (modes >> 24) & 0xff : m0);
        line16_fill(ld.ipmA, wa, bxc, nbc, nxn ? (modes >> 16) & 0xff : m0, nxn ? (modes >> 24) & 0xff : m0);
        HG_CU_T(L, 4, tcu);
    }
    L.cu_modes = modes;
    if (HG_PIC_CHROMA(P)) {  // intra_chroma_pred_mode: per PB with 4:4:4, else per CU; 8.4.3
        const int nc = HG_PIC_CHROMA(P) == 3 ? np : 1;
        int cms = 0;
        for (int i = 0; i < nc; ++i) {
            const int icpm = dec(L, G, CTX_CHROMA_MODE) ? (int)byp_bits(L, G, 2) : 4;
            const int lm = (modes >> (8 * i)) & 0xff;
            int cm;
            if (icpm == 4) {
                cm = lm;
            } else {
                cm = icpm == 0 ? 0 : (icpm == 1 ? 26 : (icpm == 2 ? 10 : 1));
                if (cm == lm) cm = 34;
            }
            if (HG_PIC_CHROMA(P) == 2) cm = mode422(cm);
            cms |= cm << (8 * i);
        }
        L.cu_chroma = nc == 1 ? (int)((uint32_t)cms * 0x01010101u) : cms;  // byte k: PB k
    }
    HG_CU_T(L, 5, tcu);
    L.tx = L.qx, L.ty = L.qy, L.tl = L.ql, L.td = 0, L.tcbf = 0;
    L.st = U_TT;
}

// The scalar engines write the edge / no-filter map's rows as the tree's leaves
// are parsed.  The vector engines leave them to k_paint_flags (transform.hip),
// which paints the map from the luma TB records after the parse
// (BatchArgs::flags_from_recs): the per-lane row loop held every lane of the unit
// run for its largest TB in nearly every pass.  A PCM CU's block
// stays with pcm_cu in every engine: its record cannot tell the CU's own bypass flag.
// (HG_FLAGS_IN_PARSE: written by every engine too, for same-box pairs; harmless
// beside the painting, which writes the same bytes later.)
#if defined(HG_FLAGS_IN_PARSE)
template <class EG>
constexpr bool kFlagsInParse = true;
#else
template <class EG>
constexpr bool kFlagsInParse = EG::kSolo;
#endif
// The QpY map likewise: the scalar engines write a finished CU's rows in cu_done.
// The vector engines append one word per CU (cu_word, kernels.hpp) to the CTB row's
// CU list instead, and k_paint_flags paints the rows from the words after the parse:
// the row loop ran up to 16 stores on every lane of nearly every completion step
// (DESIGN 5.24).  (HG_QPY_IN_PARSE: every engine writes the rows too, for same-box pairs.)
#if defined(HG_QPY_IN_PARSE)
template <class EG>
constexpr bool kQpyInParse = true;
#else
template <class EG>
constexpr bool kQpyInParse = EG::kSolo;
#endif
// the QpY map itself (the vector engines' slot of its pointer holds their CU list,
// lane_cus: the map lies before the flag map)
template <class EG>
HG_HD inline int8_t HG_GAS *qpy_map(const LanePic &P) {
    if constexpr (EG::kSolo) return P.gqpy;
    else return (int8_t HG_GAS *)(P.gflags - (size_t)P.w4 * P.h4);
}

// U_TT: transform_tree descent (7.3.8.8) from the current node to a leaf,
// then transform_unit (7.3.8.10) up to its first TB
template <class EG>
HG_HD inline void unit_tt(Lane &L, LaneLds &ld, LanePic &P, const EG &G) {
    HG_TB_T0(ttt);
    const bool nxn = (L.fl & F_NXN) != 0;
    const int max_depth = P.maxDepthIntra + (nxn ? 1 : 0);
    for (;;) {
        bool split;
        if (L.tl <= P.maxTb && L.tl > P.minTb && L.td < max_depth && !(nxn && L.td == 0))
            split = dec(L, G, CTX_SPLIT_TF + 5 - L.tl) != 0;
        else
            split = L.tl > P.maxTb || (nxn && L.td == 0);
        uint32_t cbf = 0;  // cbf_cb | cbf_cr << 1, 4:2:2 lower TBs << 2 / << 3 (7.3.8.8)
        if ((L.tl > 2 && HG_PIC_CHROMA(P)) || HG_PIC_CHROMA(P) == 3) {
            const uint32_t pc = L.td == 0 ? 3u : (L.tcbf >> (4 * (L.td - 1))) & 3u;
            const bool two = HG_PIC_CHROMA(P) == 2 && (!split || L.tl == 3);
            if (pc & 1) {
                cbf |= (uint32_t)dec(L, G, CTX_CBF_CHROMA + L.td);
                if (two) cbf |= (uint32_t)dec(L, G, CTX_CBF_CHROMA + L.td) << 2;
            }
            if (pc & 2) {
                cbf |= (uint32_t)dec(L, G, CTX_CBF_CHROMA + L.td) << 1;
                if (two) cbf |= (uint32_t)dec(L, G, CTX_CBF_CHROMA + L.td) << 3;
            }
        }
        L.tcbf = (L.tcbf & ~(15u << (4 * L.td))) | (cbf << (4 * L.td));
        if (!split) break;
        --L.tl;  // child 0
        ++L.td;
    }
    const uint32_t cbf = (L.tcbf >> (4 * L.td)) & 15u;
    L.fl &= ~F_CBF_L;
    if (dec(L, G, CTX_CBF_LUMA + (L.td == 0 ? 1 : 0))) L.fl |= F_CBF_L;
    // transform_unit
    const bool chroma4 = (HG_PIC_CHROMA(P) == 1 || HG_PIC_CHROMA(P) == 2) && L.tl == 2;
    const uint32_t pc = L.td > 0 ? (L.tcbf >> (4 * (L.td - 1))) & 15u : 0u;  // the parent's chroma cbfs
    const bool cbf_c = HG_PIC_CHROMA(P) == 0 ? false : (chroma4 ? pc != 0 : cbf != 0);
    if (((L.fl & F_CBF_L) || cbf_c) && (pic_flags<EG>(P) & SP_CU_QP_DELTA) && !(L.fl & F_DQP_CODED)) {
        int v = 0;  // cu_qp_delta_abs: TR prefix (cMax 5), EG0 suffix
        if constexpr (!EG::kSolo) {
            // the first bin's context, then one context for bins 2 to 5: read once, stored once
            v = dec(L, G, CTX_CU_QP_DELTA);
            if (v) {
                uint32_t t = ctx_ld(L, G, CTX_CU_QP_DELTA + 1);
                while (v < 5 && dec_t(L, G, t & 0x7fu, t)) ++v;
                ctx_st(L, G, CTX_CU_QP_DELTA + 1, t & 0x7fu);
            }
        } else {
            while (v < 5 && dec(L, G, CTX_CU_QP_DELTA + (v == 0 ? 0 : 1))) ++v;
        }
        HG_COV(COV_DQP);
        if (v == 5) {
            HG_COV(COV_DQP_EG0);
            int ones = 0;
            bool bad = false;
            while (byp(L, G)) {
                if (++ones > 31) {
                    bad = true;
                    break;
                }
            }
            if (bad) L.status |= ST_SYNTAX;
            else v += (int)(((1u << ones) - 1u) + byp_bits(L, G, ones));
        }
        if (v && byp(L, G)) v = -v;
        // 7.4.9.14: CuQpDeltaVal in [-(26 + QpBdOffsetY / 2), 25 + QpBdOffsetY / 2]
        // (outside it, QpY and the scaling shift would leave their ranges)
        const int vlo = -(26 + P.qpbdY / 2), vhi = 25 + P.qpbdY / 2;
        if (HG_UNLIKELY(v < vlo || v > vhi)) {
            L.status |= ST_SYNTAX;
            v = v < vlo ? vlo : vhi;
        }
        L.fl |= F_DQP_CODED;
        L.cu_qp_delta_val = v;
        update_qpy(L, P);
    }
    if constexpr (kFlagsInParse<EG>) {  // edge / no-filter flags of every 4x4 luma block of the TB (MF_*)
        const int nb = 1 << (L.tl - 2), gx0 = L.tx >> 2, gy0 = L.ty >> 2;
        const int wx = gx0 + nb <= P.w4 ? nb : P.w4 - gx0, hy = gy0 + nb <= P.h4 ? nb : P.h4 - gy0;
        const uint64_t nf = (lane_fl<EG>(L) & F_BYPASS) ? MF_NOFILT : 0;
        const uint64_t rep = 0x0101010101010101ull;
        for (int y = 0; y < hy; ++y) {
            uint8_t *row = P.gflags + (size_t)(gy0 + y) * P.w4 + gx0;
            const uint64_t h = (y == 0 ? (uint64_t)MF_EDGE_H : 0u) | nf;
            store_bytes(row, wx, (rep * h) | (uint64_t)MF_EDGE_V);
        }
    }
    HG_TB_T(L, 3, ttt);
    const int blk = L.td == 0 ? 0 : (((L.tx >> L.tl) & 1) | (((L.ty >> L.tl) & 1) << 1));
    // luma, then Cb and Cr (two each with 4:2:2: upper, lower)
    L.tb_n = (HG_PIC_CHROMA(P) != 0 && (!chroma4 || blk == 3)) ? (HG_PIC_CHROMA(P) == 2 ? 5 : 3) : 1;
    L.tb_t = 0;
    L.st = U_TB;
}

// record of the current TB (TuRec, desc.hpp)
template <class EG>
HG_HD inline void tu_emit(Lane &L, const LanePic &P) {
    const uint32_t fl = lane_fl<EG>(L);
    int qp;
    if (L.tb_cidx == 0) {
        qp = L.qpy_cur + P.qpbdY;
    } else {
        const int off = L.tb_cidx == 1 ? P.cbOff : P.crOff;
        int qpi = L.qpy_cur + off;
        qpi = qpi < -P.qpbdC ? -P.qpbdC : (qpi > 57 ? 57 : qpi);
        qp = chroma_qp_map(qpi, HG_PIC_CHROMA(P)) + P.qpbdC;
    }
    uint32_t f = (uint32_t)L.tb_cidx;
    if (fl & F_TB_CBF) f |= TU_CBF;
    if (fl & F_TS) f |= TU_TSKIP;
    if (fl & F_BYPASS) f |= TU_BYPASS;
    if (fl & F_PCM) f |= TU_PCM | TU_BYPASS;
    if (L.tb_cidx == 0 && L.tb_log2 == 2) f |= TU_DST;
    if (HG_LIKELY(L.ntu < P.tu_cap)) {
        const uint32_t w0 = (uint32_t)L.tb_x | ((uint32_t)L.tb_y << 16);
        const uint32_t w1 = (uint32_t)L.tb_log2 | (f << 8) | ((uint32_t)L.tb_mode << 16) | ((uint32_t)(uint8_t)qp << 24);
        const uint32_t w3 = (L.ncoef - L.tb_coef0) | ((uint32_t)L.c << 16);
        if (pic_flags<EG>(P) & PF_COHERENT) store_tu_agent(P.tu_base + L.tu_row + L.ntu, w0, w1, L.tb_coef0, w3);
        else store_tu(P.tu_base + L.tu_row + L.ntu, w0, w1, L.tb_coef0, w3);
        ++L.ntu;
    } else {
        L.status |= ST_CAPACITY;
    }
}

template <class EG>
HG_HD inline void cu_done(Lane &L, LaneLds &ld, LanePic &P);

// After a TB: its record, then the next TB of the TU, the next transform-tree
// node, or (tree done) the CU's QpY and the next coding-quadtree node / CTU end.
// (Vector engines: the U_TBD step of the pass; scalar engines: from U_TB / U_SB.)
template <class EG>
HG_HD inline void tb_done(Lane &L, LaneLds &ld, LanePic &P) {
    tu_emit<EG>(L, P);
    if (++L.tb_t < L.tb_n) {
        L.st = U_TB;
        return;
    }
    // next transform-tree node in z-order (nodes are aligned to their size)
    while (L.td > 0) {
        const int s = 1 << L.tl;
        const int b = ((L.tx >> L.tl) & 1) | (((L.ty >> L.tl) & 1) << 1);
        if (b < 3) {
            const int px = L.tx & ~(2 * s - 1), py = L.ty & ~(2 * s - 1);
            L.tx = px + ((b + 1) & 1) * s;
            L.ty = py + ((b + 1) >> 1) * s;
            L.st = U_TT;
            return;
        }
        L.tx &= ~(2 * s - 1);
        L.ty &= ~(2 * s - 1);
        ++L.tl;
        --L.td;
    }
    cu_done<EG>(L, ld, P);
}

// end of a CU: QpY for qPY_A/B and the 4x4 map (deblocking: the scalar engines
// write its rows, the vector engines one word for the CU in the CTB row's CU
// list, kQpyInParse), then the next coding-quadtree node in z-order (skipping
// children outside the picture) or the CTU end
template <class EG>
HG_HD inline void cu_done(Lane &L, LaneLds &ld, LanePic &P) {
    HG_TB_T0(tcu);
    HG_COV(COV_CU_DONE + L.ql - 3);
    {
        const int n = 1 << L.ql, nd = n >> 3;
        const int dy = (L.qy - L.ctby) >> 3, dx = (L.qx - L.ctbx) >> 3;
        // (byte loops in every engine: as words beside the other two lines they lost)
        for (int k = 0; k < nd; ++k) {
            ld.qL[dy + k] = (int8_t)L.qpy_cur;
            ld.qA[dx + k] = (int8_t)L.qpy_cur;
        }
        HG_TB_T(L, 4, tcu);
        if constexpr (!EG::kSolo) {
            // geometric capacity (CUs are at least 8x8 and disjoint): a stream cannot exceed it
            if (HG_LIKELY(L.ncu < cu_cap_row(P.wctb, P.log2ctb)))
                lane_cus(P)[(uint32_t)L.row * cu_cap_row(P.wctb, P.log2ctb) + L.ncu++] =
                    cu_word(L.qx, L.qy - L.ctby, L.ql, L.qpy_cur);
            else
                L.status |= ST_CAPACITY;
        }
        if constexpr (kQpyInParse<EG>) {
            const int nb = n >> 2, gx0 = L.qx >> 2, gy0 = L.qy >> 2;
            const int wx = gx0 + nb <= P.w4 ? nb : P.w4 - gx0, hy = gy0 + nb <= P.h4 ? nb : P.h4 - gy0;
            for (int y = 0; y < hy; ++y) {
                int8_t *row = qpy_map<EG>(P) + (size_t)(gy0 + y) * P.w4 + gx0;
                store_bytes(reinterpret_cast<uint8_t *>(row), wx, 0x0101010101010101ull * (uint8_t)L.qpy_cur);
            }
        }
        L.qp_prev_last = L.qpy_cur;
    }
    HG_TB_T(L, 5, tcu);
    // next coding-quadtree node in z-order, skipping children outside the picture
    while (L.qd > 0) {
        const int s = 1 << L.ql;
        const int px = L.qx & ~(2 * s - 1), py = L.qy & ~(2 * s - 1);
        for (int b = (((L.qx >> L.ql) & 1) | (((L.qy >> L.ql) & 1) << 1)) + 1; b < 4; ++b) {
            const int cx = px + (b & 1) * s, cy = py + (b >> 1) * s;
            if (cx < P.W && cy < P.H) {
                L.qx = cx;
                L.qy = cy;
                L.st = U_CQT;
                return;
            }
        }
        L.qx = px;
        L.qy = py;
        ++L.ql;
        --L.qd;
    }
    L.st = U_CTU_END;
}

// U_TB: TB tb_t of the TU; without coefficients it is done (vector engines: it
// goes to the pass's U_TBD step), otherwise residual_coding's header
// (transform_skip_flag, last position) is parsed
template <class EG>
HG_HD inline void unit_tb(Lane &L, LaneLds &ld, LanePic &P, const EG &G) {
    HG_TB_T0(ttb);
    const int t = L.tb_t;
    const bool chroma4 = (HG_PIC_CHROMA(P) == 1 || HG_PIC_CHROMA(P) == 2) && L.tl == 2;
    // component and (4:2:2) upper / lower half of TB t: luma, Cb (, Cb lower), Cr (, Cr lower)
    const bool c422 = HG_PIC_CHROMA(P) == 2;
    const int comp = t == 0 ? 0 : (c422 ? 1 + ((t - 1) >> 1) : t), half = (c422 && t > 0) ? (t - 1) & 1 : 0;
    bool cbf;
    L.tb_cidx = comp;
    if (t == 0) {
        L.tb_x = L.tx;
        L.tb_y = L.ty;
        L.tb_log2 = L.tl;
        int k = 0;  // IntraPredModeY of the PB the TB lies in
        if (L.fl & F_NXN) {
            const int half = 1 << (L.ql - 1);
            k = ((L.ty - L.qy) >= half ? 2 : 0) + ((L.tx - L.qx) >= half ? 1 : 0);
        }
        L.tb_mode = (L.cu_modes >> (8 * k)) & 0xff;
        cbf = (L.fl & F_CBF_L) != 0;
    } else if (!chroma4) {
        L.tb_log2 = HG_PIC_CHROMA(P) == 3 ? L.tl : L.tl - 1;  // log2TrafoSizeC
        L.tb_x = L.tx >> HG_PIC_SUBX(P);
        L.tb_y = (L.ty >> HG_PIC_SUBY(P)) + (half << L.tb_log2);
        int k = 0;  // IntraPredModeC of the PB (4:4:4 NxN: four)
        if (HG_PIC_CHROMA(P) == 3 && (L.fl & F_NXN)) {
            const int hp = 1 << (L.ql - 1);
            k = ((L.ty - L.qy) >= hp ? 2 : 0) + ((L.tx - L.qx) >= hp ? 1 : 0);
        }
        L.tb_mode = (L.cu_chroma >> (8 * k)) & 0xff;
        cbf = ((L.tcbf >> (4 * L.td + (comp - 1) + 2 * half)) & 1u) != 0;
    } else {  // 4:2:0 / 4:2:2, 4x4 luma TBs: the chroma TBs of the 8x8 parent, after its 4th luma TB
        const int s = 1 << (L.tl + 1);
        L.tb_x = (L.tx & ~(s - 1)) >> 1;
        L.tb_y = ((L.ty & ~(s - 1)) >> HG_PIC_SUBY(P)) + 4 * half;
        L.tb_log2 = 2;
        L.tb_mode = L.cu_chroma & 0xff;
        cbf = ((L.tcbf >> (4 * (L.td - 1) + (comp - 1) + 2 * half)) & 1u) != 0;
    }
    L.fl = (L.fl & ~(F_TS | F_TB_CBF)) | (cbf ? F_TB_CBF : 0u);
    L.tb_coef0 = L.ncoef;
    if (!cbf) {
        if constexpr (EG::kSolo) tb_done<EG>(L, ld, P);
        else L.st = U_TBD;
        return;
    }
    // residual_coding header (7.3.8.11)
    const int l2 = L.tb_log2, n = 1 << l2, cidx = comp;
    HG_COV((cidx ? COV_TB_CHROMA : COV_TB_LUMA) + l2 - 2);
    if (t == 1 && !(L.fl & F_CBF_L)) HG_COV(COV_CODED_AFTER_EMPTY);
    if ((pic_flags<EG>(P) & SP_TRANSFORM_SKIP) && !(L.fl & F_BYPASS) && l2 == 2 && dec(L, G, CTX_TS_FLAG + (cidx ? 1 : 0)))
        L.fl |= F_TS;
    if (L.fl & F_TS) HG_COV(COV_TSKIP);
    // last_sig_coeff_{x,y}_prefix (decoder.rs:109-130), suffixes
    const int cmax = (l2 << 1) - 1;
    const int off = cidx == 0 ? 3 * (l2 - 2) + ((l2 - 1) >> 2) : 15;
    const int shift = cidx == 0 ? (l2 + 1) >> 2 : l2 - 2;
    int px = 0, py = 0;
    HG_TB_T(L, 0, ttb);
    // (a register word of the prefix's up to five contexts, read and stored once,
    // measured no faster than these per-bin LDS bytes: DESIGN 5.18)
    while (px < cmax && dec(L, G, CTX_LAST_X + off + (px >> shift))) ++px;
    while (py < cmax && dec(L, G, CTX_LAST_Y + off + (py >> shift))) ++py;
    HG_TB_T(L, 1, ttb);
    int lx = px, ly = py;
    if (px > 3 || py > 3) HG_COV(COV_LAST_SUFFIX);
    if (px > 8 || py > 8) HG_COV(COV_LAST_CTX5);
    if ((px == 0 || px == cmax) && (py == 0 || py == cmax)) HG_COV(COV_LAST_00 + (px ? 2 : 0) + (py ? 1 : 0));
    if ((px > 3) != (py > 3)) HG_COV(px > 3 ? COV_LAST_SUFFIX_X_ONLY : COV_LAST_SUFFIX_Y_ONLY);
    if (px > 3) {
        const int k = (px >> 1) - 1;
        lx = (1 << k) * (2 + (px & 1)) + (int)byp_bits(L, G, k);
    }
    if (py > 3) {
        const int k = (py >> 1) - 1;
        ly = (1 << k) * (2 + (py & 1)) + (int)byp_bits(L, G, k);
    }
    int scan = 0;  // 7.4.9.11 scanIdx
    if (l2 == 2 || (l2 == 3 && (cidx == 0 || HG_PIC_CHROMA(P) == 3))) {
        if (L.tb_mode >= 6 && L.tb_mode <= 14) scan = 2;
        else if (L.tb_mode >= 22 && L.tb_mode <= 30) scan = 1;
    }
    if (scan == 2) {
        HG_COV(COV_LAST_SWAP);
        const int tt = lx;
        lx = ly;
        ly = tt;
    }
    if (HG_UNLIKELY(lx >= n || ly >= n)) {
        L.status |= ST_SYNTAX;
        lx &= n - 1;
        ly &= n - 1;
    }
    const int sbl = l2 - 2, sbw = 1 << sbl;
    L.rc_scan = scan;
    L.rc_last_sub = scan_inv(G, sbl, scan, (ly >> 2) * sbw + (lx >> 2));
    L.rc_last_pos = scan_inv(G, 2, scan, (ly & 3) * 4 + (lx & 3));
    L.rc_csbf = 0;
    L.rc_prev_c1 = 1;
    L.fl &= ~F_ANY_SB;
    L.rc_i = L.rc_last_sub;
    L.st = U_SB;
    HG_TB_T(L, 2, ttb);
}

// bit n of a 16-bit mask to bit 4n (a nibble per scan position).  Scalar
// engine: two s_bitreplicate_b64_b32 (each bit doubled) and a mask, three
// SALU ops instead of the twelve of the shift-and-mask ladder
template <bool Scalar = false>
HG_HD inline uint64_t spread16_nib(uint32_t m) {
#if !defined(HG_HOST_EMU) && defined(__HIP_DEVICE_COMPILE__)
    if constexpr (Scalar) {
        uint64_t x2, x4;
        asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(x2) : "s"(uni32(m & 0xffffu)));
        asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(x4) : "s"((uint32_t)x2));
        return x4 & 0x1111111111111111ull;
    }
#endif
    uint64_t x = m & 0xffffu;
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

// the vector engines' sub-block unit (the greater1 context selector,
// the remainder phase's carried Rice parameter and in-place nibble update, the
// record's nibble spread and escape slot); the scalar engines keep their code
template <class EG>
constexpr bool kSbVec = !EG::kSolo;

// (vector engines) the same in 32-bit halves, eight positions each: the record
// stores the nibbles as two dwords anyway, and a step is a shift-or and a mask
// where the 64-bit ladder takes a 64-bit shift, two ORs and two masks
HG_HD inline uint64_t spread16_nib_halves(uint32_t m) {
    auto half = [](uint32_t x) {
        x = (x | (x << 12)) & 0x000f000fu;
        x = (x | (x << 6)) & 0x03030303u;
        x = (x | (x << 3)) & 0x11111111u;
        return x;
    };
    return (uint64_t)half(m & 0xffu) | ((uint64_t)half((m >> 8) & 0xffu) << 32);
}

// (nesc0, vector engines: L.nesc when the sub-block started; every nibble of 15
// is an escape that the remainder loop counted into L.nesc, so the scalar
// engines' count of those nibbles is L.nesc - nesc0)
template <class EG, class L_, class P_>
HG_HD inline void sb_store(L_ &L, const P_ &P, uint32_t sig, uint32_t signs, uint64_t nib, int xS, int yS, bool hide,
                           uint32_t nesc0) {
    uint32_t esc0;  // row-relative index of its first escape
    if constexpr (kSbVec<EG>) {
        esc0 = P.coef_cap - 1 - nesc0;
    } else {
        const uint32_t nesc_sb =
            (uint32_t)__builtin_popcountll(nib & (nib >> 1) & (nib >> 2) & (nib >> 3) & 0x1111111111111111ull);
        esc0 = P.coef_cap - 1 - (L.nesc - nesc_sb);
    }
    const uint32_t w0 = (sig & 0xffffu) | (signs & 0xffff0000u);
    const uint32_t w3 = (uint32_t)xS | ((uint32_t)yS << 3) | ((uint32_t)L.rc_scan << 6) | (hide ? 1u << 8 : 0u) |
                        (esc0 << 9);
    if (HG_LIKELY(L.ncoef + L.nesc + 4 <= P.coef_cap)) {
        TuRec *d = (TuRec *)(P.coef_base + L.coef_row + L.ncoef);
        if (pic_flags<EG>(P) & PF_COHERENT) store_tu_agent(d, w0, (uint32_t)nib, (uint32_t)(nib >> 32), w3);
        else store_tu(d, w0, (uint32_t)nib, (uint32_t)(nib >> 32), w3);
        L.ncoef += 4;
    } else {
        L.status |= ST_CAPACITY;
    }
}

// U_SB: sub-block rc_i of residual_coding (7.3.8.11, 9.3.4.2.5-7)
template <class EG>
HG_HD inline void unit_sb(Lane &L, LaneLds &ld, LanePic &P, const EG &G) {
#if defined(HG_PARSE_PROF_SB) && !defined(HG_HOST_EMU)
    uint64_t tsb = __builtin_amdgcn_s_memtime();
#endif
    const int l2 = L.tb_log2, cidx = L.tb_cidx, i = L.rc_i;
    const int sbl = l2 - 2, sbw = 1 << sbl;
    const int sp = scan_pos(G, sbl, L.rc_scan, i);
    const int xS = sp & 15, yS = sp >> 4;
    int pcs = 0;  // prevCsbf
    if (xS < sbw - 1) pcs |= (int)((L.rc_csbf >> (yS * 8 + xS + 1)) & 1);
    if (yS < sbw - 1) pcs |= (int)((L.rc_csbf >> ((yS + 1) * 8 + xS)) & 1) << 1;
    bool coded = true, infer_dc = false;
    if (i < L.rc_last_sub && i > 0) {
        coded = dec(L, G, CTX_CSBF + ((pcs & 1) | (pcs >> 1)) + (cidx ? 2 : 0)) != 0;
        infer_dc = true;
    }
    uint32_t sig = 0;
    if (coded) {
        L.rc_csbf |= 1ull << (yS * 8 + xS);
        int nstart = 15;
        if (i == L.rc_last_sub) {
            sig = 1u << L.rc_last_pos;
            nstart = L.rc_last_pos - 1;
        }
        // sig_coeff_flag contexts of the sub-block (9.3.4.2.5) in a register
        // cache: a 4x4 TB uses sigCtx 0..8 (ctxIdxMap, slots 0..8); larger TBs
        // use sigCtx 0 at the TB's DC (slot 0) and off + 0..2 (slots 1..3)
        const int cbase = CTX_SIG + (cidx ? 27 : 0);
        auto cb = [&](int i) { return ctx_ld(L, G, cbase + i); };
        uint64_t seq = G.seqw(L.rc_scan * 5 + (l2 == 2 ? 4 : pcs));  // slot per scan position
        uint32_t c0 = 0, c1 = 0, c2 = 0;
        // vector engines: the sub-block's (up to 9) context states as 7-bit fields
        // of one 64-bit word, slot k at bit 7k (a state byte is below 128:
        // pStateIdx << 1 | valMps), so a slot is one 64-bit shift and mask each way.
        // The 3-word byte cache the scalar engine keeps took two compares, two
        // selects and a bit-field extract to read a slot and three selects to
        // write it back.  r06 A/B (profiles/r06/ab/ab_cc7.txt): 22,805 -> 23,052
        // Mpix/s at 128 images; in the scalar engine's 4x4 loop the same fields
        // cost one image 24.88 -> 25.2 ms, so it keeps its byte word and slot 8
        constexpr bool kCc7 = !EG::kSolo;
        uint64_t cc = 0;
        int off = 0;
        if (l2 == 2) {
            if constexpr (kCc7) {
                for (int k = 0; k < 9; ++k) cc |= (uint64_t)cb(k) << (7 * k);
            } else {
                c0 = cb(0) | (cb(1) << 8) | (cb(2) << 16) | (cb(3) << 24);
                c1 = cb(4) | (cb(5) << 8) | (cb(6) << 16) | (cb(7) << 24);
                c2 = cb(8);
            }
        } else {
            off = cidx == 0 ? ((xS | yS) ? 3 : 0) + (l2 == 3 ? (L.rc_scan == 0 ? 9 : 15) : 21) : (l2 == 3 ? 9 : 12);
            if ((xS | yS) == 0) seq &= ~0xfull;  // DC of the TB (scan position 0 of sub-block 0): sigCtx 0
            if constexpr (kCc7)
                cc = (uint64_t)cb(0) | ((uint64_t)cb(off) << 7) | ((uint64_t)cb(off + 1) << 14) |
                     ((uint64_t)cb(off + 2) << 21);
            else
                c0 = cb(0) | (cb(off) << 8) | (cb(off + 1) << 16) | (cb(off + 2) << 24);
        }
        HG_SB_T(L, 0, tsb);
        if constexpr (EG::kSolo) {
          if (l2 > 2) {
            // scalar engine, TBs above 4x4: the four slots in one 32-bit word
            // (a byte shift reads or writes a slot), no slot 8 to select
            auto dec_slot4 = [&](uint32_t slot) -> uint32_t {
                const uint32_t sh = slot * 8u;
                uint32_t cs = (c0 >> sh) & 0xffu;
                const uint32_t bin = (uint32_t)dec_s(L, G, cs);
                c0 = (c0 & ~(0xffu << sh)) | (cs << sh);
                return bin;
            };
            uint32_t sg = sig;
            for (int nn = nstart; nn > 0; --nn) sg |= dec_slot4((uint32_t)(seq >> (4 * nn)) & 3u) << nn;
            if (nstart >= 0) sg |= (infer_dc && sg == 0) ? 1u : dec_slot4((uint32_t)seq & 3u);
            sig = sg;
          } else {
            // scalar engine: slots 0..7 as one 64-bit word (a shift reads or
            // writes a slot), slot 8 apart; every select branch-free, the bin
            // an integer, so an iteration is one scalar chain
            uint64_t cc = (uint64_t)c0 | ((uint64_t)c1 << 32);
            auto dec_slot = [&](uint32_t slot) -> uint32_t {
                const uint32_t sh = (slot & 7u) * 8u;
                const bool hi = slot >= 8u;
                uint32_t cs = hi ? c2 : (uint32_t)(cc >> sh) & 0xffu;
                const uint32_t bin = (uint32_t)dec_s(L, G, cs);
                const uint64_t ncc = (cc & ~(0xffull << sh)) | ((uint64_t)cs << sh);
                cc = hi ? cc : ncc;
                c2 = hi ? cs : c2;
                return bin;
            };
            // positions nstart .. 1 are always decoded; only position 0 of a
            // coded sub-block with no other significant coefficient is inferred
            uint32_t sg = sig;
            for (int nn = nstart; nn > 0; --nn) sg |= dec_slot((uint32_t)(seq >> (4 * nn)) & 15u) << nn;
            if (nstart >= 0) sg |= (infer_dc && sg == 0) ? 1u : dec_slot((uint32_t)seq & 15u);
            sig = sg;
            c0 = (uint32_t)cc;
            c1 = (uint32_t)(cc >> 32);
          }
        } else {
            // positions nstart .. 1 without a per-position branch (the bin is or-ed
            // in), position 0 apart: inferred in a coded sub-block with no other
            // significant coefficient (r05 A/B against the r04 loop, which tested
            // for the inferred DC at every position: parse alone 63.1 -> 59.9 ms,
            // 18,770 -> 19,260 Mpix/s at 128 images)
            auto dec_slot = [&](int slot) -> uint32_t {
                if constexpr (kCc7) {
                    // the new byte goes in under the field's mask (v_bfi), which
                    // also drops dec_t's bin bit
                    const uint32_t sh = (uint32_t)slot * 7u;
                    const uint64_t m = 0x7full << sh;
                    uint32_t t;
                    const uint32_t bin = (uint32_t)dec_t(L, G, (uint32_t)(cc >> sh) & 0x7fu, t);
                    const uint64_t tv = (uint64_t)t << sh;
                    cc = (uint64_t)bfi32((uint32_t)m, (uint32_t)tv, (uint32_t)cc) |
                         ((uint64_t)bfi32((uint32_t)(m >> 32), (uint32_t)(tv >> 32), (uint32_t)(cc >> 32)) << 32);
                    return bin;
                } else {
                    uint32_t cs = cache_get(c0, c1, c2, slot);
                    const uint32_t bin = (uint32_t)dec_s(L, G, cs);
                    cache_put(c0, c1, c2, slot, cs);
                    return bin;
                }
            };
            if constexpr (kCc7) {
                // the slot of position nn taken from the top nibble of a copy of
                // seq shifted left one nibble per position (no per-lane shift count)
                uint64_t sq = nstart > 0 ? seq << (4 * (15 - nstart)) : 0ull;
                for (int nn = nstart; nn > 0; --nn) {
                    sig |= dec_slot((int)(uint32_t)(sq >> 60)) << nn;
                    sq <<= 4;
                }
            } else {
                for (int nn = nstart; nn > 0; --nn) sig |= dec_slot((int)((seq >> (4 * nn)) & 15u)) << nn;
            }
            if (nstart >= 0) {
                HG_COV(l2 == 2 ? COV_SB_SIG4 : COV_SB_SIG);
                if (infer_dc && sig == 0) {
                    HG_COV(COV_SB_INFER_DC);
                    sig |= 1u;
                } else {
                    sig |= dec_slot((int)(seq & 15u));
                }
            } else {
                HG_COV(COV_SB_LAST_POS0);
            }
        }
        auto cw = [&](int i, uint32_t v) { ctx_st(L, G, cbase + i, v & 0xffu); };
        if constexpr (kCc7) {
            if (l2 == 2) {
                for (int k = 0; k < 9; ++k) cw(k, (uint32_t)(cc >> (7 * k)) & 0x7fu);
            } else {
                cw(0, (uint32_t)cc & 0x7fu);
                cw(off, (uint32_t)(cc >> 7) & 0x7fu);
                cw(off + 1, (uint32_t)(cc >> 14) & 0x7fu);
                cw(off + 2, (uint32_t)(cc >> 21) & 0x7fu);
            }
        } else if (l2 == 2) {
            for (int k = 0; k < 4; ++k) cw(k, c0 >> (8 * k));
            for (int k = 0; k < 4; ++k) cw(4 + k, c1 >> (8 * k));
            cw(8, c2);
        } else {
            cw(0, c0);
            cw(off, c0 >> 8);
            cw(off + 1, c0 >> 16);
            cw(off + 2, c0 >> 24);
        }
#if defined(HG_PARSE_PROF_SB) && !defined(HG_PARSE_PROF_TB) && !defined(HG_PARSE_PROF_CU) && !defined(HG_HOST_EMU)
        L.psb[4] += (uint64_t)(nstart + 1);
#endif
        HG_SB_T(L, 1, tsb);
    }
    if (sig) {
        // greater1 / greater2 (9.3.4.2.6-7)
        int ctx_set = (i == 0 || cidx > 0) ? 0 : 2;
        if ((L.fl & F_ANY_SB) && L.rc_prev_c1 == 0) {
            HG_COV(COV_SB_CTXSET_INC);
            ++ctx_set;
        }
        L.fl |= F_ANY_SB;
        int c1 = 1;
        uint32_t g1 = 0, g2 = 0;
        // the ctxSet's four greater1 contexts (9.3.4.2.6) in one register
        const int gbase = CTX_GT1 + ctx_set * 4 + (cidx ? 16 : 0);
        uint32_t gc = ctx_ld(L, G, gbase) | (ctx_ld(L, G, gbase + 1) << 8) | (ctx_ld(L, G, gbase + 2) << 16) |
                      (ctx_ld(L, G, gbase + 3) << 24);
        const int first_sig = 31 - __builtin_clz(sig & (0u - sig));
        const int last_sig = msb32(sig);
        int num_g1 = 0, last_g1 = -1;
        uint32_t beyond8 = sig;  // after the greater1 loop: the significant positions past the first eight
        if constexpr (EG::kSolo) {
            // scalar engine: the first 8 significant positions, every update a
            // select on integers (no boolean carried across the engine's refill branch)
            uint32_t &m = beyond8;
            for (int j = 0; j < 8 && m; ++j) {
                const int nn = msb32(m);
                m ^= 1u << nn;
                const uint32_t gs = (uint32_t)(c1 < 3 ? c1 : 3) * 8u;
                uint32_t cs = (gc >> gs) & 0xffu;
                const uint32_t f = (uint32_t)dec_s(L, G, cs);
                gc = (gc & ~(0xffu << gs)) | (cs << gs);
                g1 |= f << nn;
                c1 = (c1 > 0 && !f) ? c1 + 1 : 0;
            }
            // the first greater1 flag set in decoding order: positions decode from the highest down
            last_g1 = g1 ? msb32(g1) : -1;
        } else {
            for (uint32_t &m = beyond8; m && num_g1 < 8;) {
                const int nn = msb32(m);
                m &= ~(1u << nn);
                // greater1Ctx (9.3.4.2.6) is 0 from the first flag set on and
                // grows by one per flag before it, from 1.  The lanes in the loop
                // step together, so the count is the wave's and only the test of
                // g1 is per lane; c1 itself is put together after the loop
                const int gs = g1 ? 0 : (num_g1 < 2 ? num_g1 + 1 : 3) * 8;
                const uint32_t gm = 0x7fu << gs;  // (bit 7 of every byte of gc stays 0)
                uint32_t t;
                const int f = dec_t(L, G, (gc >> gs) & 0xffu, t);
                gc = bfi32(gm, t << gs, gc);
                ++num_g1;
                g1 |= (uint32_t)f << nn;
            }
            c1 = g1 ? 0 : 1 + num_g1;
            last_g1 = g1 ? msb32(g1) : -1;  // the first set in decoding order (positions decode downwards)
        }
        L.rc_prev_c1 = c1;
        for (int k = 0; k < 4; ++k) ctx_st(L, G, gbase + k, (gc >> (8 * k)) & 0xffu);
        if (last_g1 >= 0 && dec(L, G, CTX_GT2 + ctx_set + (cidx ? 4 : 0))) g2 = 1u << last_g1;
        if (g2) HG_COV(COV_SB_GT2);
        if (beyond8) HG_COV(COV_SB_BEYOND8);
        HG_SB_T(L, 2, tsb);
        const bool sign_hidden = !(lane_fl<EG>(L) & F_BYPASS) && (last_sig - first_sig > 3);
        const bool hide = (pic_flags<EG>(P) & SP_SIGN_HIDING) && sign_hidden;
        if (pic_flags<EG>(P) & SP_SIGN_HIDING) HG_COV(hide ? COV_SB_HIDE : COV_SB_NO_HIDE);
        const int nsign = __builtin_popcount(sig) - (hide ? 1 : 0);
        uint32_t signs = byp_bits(L, G, nsign);
        signs = nsign ? signs << (32 - nsign) : 0u;  // first decoded sign in bit 31
        // The sub-block leaves as one 16-byte record (SbRec, desc.hpp): the
        // significance map, the signs in decoding order, and abs - 1 of every
        // scan position as a nibble (15: the level is in the row's escape list,
        // which grows down from the end of the row's coefficient space).  abs - 1
        // is greater1 + greater2 (bit masks spread to nibbles) plus
        // coeff_abs_level_remaining where one is coded, so only those levels
        // are visited, one at a time (their Rice parameters chain); the r03
        // layout stored every coefficient with its own 4-byte store.
        // (vector engines) the row's escape count before this sub-block: the
        // record's first escape slot, without counting the nibbles of 15 afterwards
        [[maybe_unused]] const uint32_t nesc0 = L.nesc;
        uint64_t nib;
        if constexpr (kSbVec<EG>) {
            // greater1 alone: the position with a greater2 flag always has a
            // remainder, and the remainder loop adds the flag with it
            nib = spread16_nib_halves(g1);
        } else {
            nib = spread16_nib<EG::kSolo>(g1) + (g2 ? 1ull << (4 * last_g1) : 0ull);  // (g2: at most the one bit)
        }
        {
            // the levels with a coded remainder: greater1 set but not the one with a
            // greater2 flag, greater2 set, and every position past the first eight
            const uint32_t lastb = last_g1 >= 0 ? 1u << last_g1 : 0u;
            uint32_t need = (g1 & ~lastb) | g2 | beyond8;
            int last_abs = 0, last_rice = 0;
            bool first_rem = true;
            // (vector engines) cRiceParam of the next remainder, carried: min(4, k + (abs > 3 << k))
            // after every level (9.3.3.11), 0 for the first
            [[maybe_unused]] int rice = 0;
            while (need) {
                const int nn = msb32(need);
                need ^= 1u << nn;
                const int g1b = (int)((g1 >> nn) & 1);
                const int base = 1 + g1b + (int)((g2 >> nn) & 1);
                int k;
                if constexpr (kSbVec<EG>) {
                    k = rice;
                } else if (first_rem) {
                    k = 0;
                    first_rem = false;
                } else {
                    k = last_rice + (last_abs > 3 * (1 << last_rice) ? 1 : 0);
                    k = k < 4 ? k : 4;
                }
                // coeff_abs_level_remaining (decoder.rs:230-261): TR(4 << k, k) prefix, EG(k + 1) escape
                int rem = byp_rem(L, G, k);
                if (HG_UNLIKELY(rem < 0)) {
                    // EG(k + 1) prefix: unary ones, up to 8 per division, at most 31 - (k + 1)
                    const int lim = 31 - (k + 1);
                    int ones = 0;
                    for (;;) {
                        const int mm = lim + 1 - ones < 8 ? lim + 1 - ones : 8;
                        const int pz = byp_unary(L, G, mm);
                        ones += pz;
                        if (pz < mm || ones > lim) break;  // the terminating 0 read, or too many ones
                    }
                    if (ones > lim) {
                        L.status |= ST_SYNTAX;
                        rem = 0;
                    } else {
                        rem = (int)((4u << k) + (((1u << ones) - 1u) << (k + 1)) + byp_bits(L, G, ones + k + 1));
                    }
                    HG_COV(COV_SB_EGK);
                }
                if (k == 4) HG_COV(COV_SB_RICE4);
                last_abs = base + rem;
                last_rice = k;
                const int am1 = base - 1 + rem;  // abs - 1
                if constexpr (kSbVec<EG>) {
                    const int inc = last_abs > (3 << k) ? 1 : 0;
                    rice = k + inc < 4 ? k + inc : 4;
                    // The nibble holds the greater1 flag g1b (0 or 1) and has to
                    // become min(abs - 1, 15), which is at least g1b: abs - 1 =
                    // g1b + greater2 + rem.  So the difference is added in place,
                    // with no carry into the next nibble and nothing to clear first
                    nib += (uint64_t)(uint32_t)((am1 < 15 ? am1 : 15) - g1b) << (4 * nn);
                } else {
                    nib = (nib & ~(0xfull << (4 * nn))) | ((uint64_t)(am1 < 15 ? am1 : 15) << (4 * nn));
                }
                if (HG_UNLIKELY(am1 >= 15)) {  // escape: the whole level, in descending scan order from the row's end
                    HG_COV(COV_SB_ESCAPE);
                    if (L.ncoef + L.nesc + 4 < P.coef_cap) {
                        Coef HG_GAS *e = P.coef_base + L.coef_row + P.coef_cap - 1 - L.nesc;
                        if (pic_flags<EG>(P) & PF_COHERENT) store_word_agent((uint32_t *)e, (uint32_t)last_abs);
                        else *e = (uint32_t)last_abs;
                    } else {
                        L.status |= ST_CAPACITY;
                    }
                    ++L.nesc;
                }
            }
        }
        HG_SB_T(L, 3, tsb);
        sb_store<EG>(L, P, sig, signs, nib, xS, yS, hide, nesc0);
    }
    if (--L.rc_i < 0) {
        // (the TU at the CU's bottom right corner, its last TB)
        if (L.tb_t + 1 >= L.tb_n && L.tx + (1 << L.tl) == L.qx + (1 << L.ql) && L.ty + (1 << L.tl) == L.qy + (1 << L.ql))
            HG_COV(COV_CU_ENDS_IN_SB);
        if constexpr (EG::kSolo) tb_done<EG>(L, ld, P);
        else L.st = U_TBD;
    }
}

// U_CTU_END: WPP context storage, the depth line, end_of_slice_segment_flag /
// end_of_subset_one_bit (slice.rs:214-227), progress, next CTU / row
template <class EG>
HG_HD inline void unit_ctu_end(Lane &L, LaneLds &ld, LanePic &P, const Env &E, const EG &G) {
    if ((L.fl & F_WPP) && L.c == 1 && L.row + 1 < P.hctb) {
        // 9.3.2.4 storage for the next row's substream: into its lane's block, or
        // its staging block when that lane may still be parsing an earlier row
        uint32_t *dst = reinterpret_cast<uint32_t *>((EG::kSpread || pic_ring<EG>(P)) ? wpp_stage(E, P, L.row + 1)
                                                                              : E.lds[P.lane0 + (L.row + 1) % P.R].ctx);
        if constexpr (EG::kCtxReg) {
#if !defined(HG_HOST_EMU)
            const int ln = (int)__lane_id();  // every lane stores its dword
            if (ln < CTX_PAD / 4) {
                if constexpr (EG::kSpread) store_agent(dst + ln, L.cx);
                else dst[ln] = L.cx;
            }
#endif
        } else {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(ld.ctx);
#pragma nounroll
            for (int k = 0; k < CTX_PAD / 4; ++k) {
                if constexpr (EG::kSpread) store_agent(dst + k, src[k]);
                else dst[k] = src[k];
            }
        }
    }
    {  // bottom CtDepth of this CTB for the row below
        const int nb8 = 1 << (P.log2ctb - 3), col0 = L.ctbx >> 3;
        uint8_t *line = P.gdepth + (size_t)L.row * P.w8;
        for (int k = 0; k < nb8 && col0 + k < P.w8; ++k) {
            if constexpr (EG::kSpread) store_agent(line + col0 + k, ld.dA[k]);
            else line[col0 + k] = ld.dA[k];
        }
    }
    const bool last_in_pic = L.row == P.hctb - 1 && L.c == P.wctb - 1;
    // end_of_slice_segment_flag = 1 at the picture's last CTU (unless a tile's
    // substream goes on: SP_SUBSET_END) and at the end of a row that ends a slice segment
    const bool seg_end = !last_in_pic && L.c == P.wctb - 1 && (pic_flags<EG>(P) & SP_ROW_SEGMENTS) &&
                         (E.a->rsubs[P.sub_first + L.row] & SUB_SEG_END);
    const bool eos = (last_in_pic && !(pic_flags<EG>(P) & SP_SUBSET_END)) || seg_end;
    // inside a row of a picture with dependent segments starting inside rows,
    // end_of_slice_segment_flag = 1 ends one: the next starts at the next CTU
    if (term(L, G) != (eos ? 1 : 0)) {
        // end_of_slice_segment_flag = 1 inside a row of a picture that has
        // dependent segments starting there: the next starts at the next CTU
        // (unit_ctu checks that one is left).  A picture without any (always so
        // in the lean body) has no entries for them after its substream table:
        // the mismatch is an error at once
        if constexpr (EG::kSolo || EG::kLean) L.status |= ST_SUBSTREAM_END;
        else L.status |= (!eos && L.c < P.wctb - 1 && lanes_nmid<EG>(P)) ? ST_SEGSW : (uint32_t)ST_SUBSTREAM_END;
    }
    if (!eos && (last_in_pic || ((L.fl & F_WPP) && L.c == P.wctb - 1)) && !term(L, G)) L.status |= ST_SUBSTREAM_END;
    if (L.budget + L.k < 0) L.status |= ST_OVERRUN;  // read past the NAL unit
    ++L.c;
    const uint32_t pv = (L.fl & F_STOP) ? kProgDone : (uint32_t)L.row * (uint32_t)P.wctb + (uint32_t)L.c;
    if constexpr (EG::kSpread) {
        if (E.a->xntu) {  // k_intra's streaming mode reads this row's records as they appear
            // the records (agent-scope stores: PF_COHERENT) before the count: an
            // agent release, which k_intra_stream's acquire after its poll pairs with
            HG_REL_AGENT();
            store_agent(E.a->xntu + P.row_off + L.row, L.ntu);
        }
        // The rule that makes vmcnt(0) enough here: every word the row below
        // reads after this progress word (the context hand-off, SAO parameters,
        // the depth line) went out above as an agent-scope store (store_agent,
        // coherent at L2 across XCDs), so completing them orders them.  A plain
        // store into hand-off data would need HG_REL_AGENT() (L2 write-back) here.
        stores_done();
        store_agent(prog_word(E, P, L.row), pv);
    } else {
        release_fence();
        prog_store(prog_word(E, P, L.row), pv);
    }
    if (!(L.fl & F_STOP) && L.c < P.wctb) {
        L.st = U_CTU;
        return;
    }
    uint32_t *rc = E.a->row_counts + 2 * (size_t)(P.row_off + L.row);
    rc[0] = L.ntu;
    rc[1] = L.ncoef;
    if constexpr (!EG::kSolo) E.a->cu_counts[P.row_off + L.row] = L.ncu;
    const int step = (L.fl & F_WPP) ? P.R : 1;  // one substream (no WPP): walk on to the next row
    if (!(L.fl & F_STOP) && L.row + step < P.hctb) {
        L.row += step;
        L.c = 0;
        row_outputs(L, P);
        if constexpr (!EG::kSolo) L.ncu = 0;  // (not in row_outputs: the scalar engines' code would change)
        L.st = U_CTU;
        return;
    }
    // (ST_SEGSW: never reported; the scalar engines never set it)
    const uint32_t st_rep = EG::kSolo ? L.status : (L.status & ~ST_SEGSW);
    if (st_rep) atomicOr(&E.a->status[P.pic], st_rep);
    L.st = U_DONE;
}

// Runs unit `kind` on this lane (the caller passes a wave-uniform kind and
// only lanes in that unit).  One unit kind per pass keeps the dispatch a
// uniform branch: a divergent switch over the units would linearise them, and
// every L field a unit updates would then need a register per unit.
template <class EG>
HG_HD inline void run_unit(int kind, Lane &L, LaneLds &ld, LanePic &P, const Env &E, const EG &G) {
    if constexpr (EG::kSolo) {
        if (L.fl & F_REINIT) {  // after PCM samples: the driver has moved the window to L.reinit
            engine_init(L, G, L.reinit, P.bits_end);
            L.fl &= ~F_REINIT;
        }
    }
    switch (kind) {
    case U_SB: unit_sb(L, ld, P, G); break;
    case U_TB: unit_tb(L, ld, P, G); break;
    case U_TT: unit_tt(L, ld, P, G); break;
    case U_CU: unit_cu(L, ld, P, G); break;
    case U_CQT: unit_cqt(L, ld, P, G); break;
    case U_CTU: unit_ctu(L, ld, P, E, G); break;
    case U_CTU_END: unit_ctu_end(L, ld, P, E, G); break;
    case U_TBD:  // (vector engines only: the scalar ones finish a TB inside U_TB / U_SB)
        if constexpr (!EG::kSolo) tb_done<EG>(L, ld, P);
        break;
    default: break;
    }
}

// a lane in U_CTU can start its CTU (WPP: the row above is two CTUs ahead)
template <class EG = Eng>
HG_HD inline bool ctu_ready(const Lane &L, const LanePic &P, const Env &E) { return wpp_ready<EG>(L, P, E); }

// lane setup: picture constants, outputs, first state.  Returns false for an idle lane.
// `cap` lanes (waves, solo mode) at most per picture.
// (Mid: the lanes engine, which keeps the picture's count of segment starts
// inside rows in P.flags; the scalar engines do not take such pictures)
template <bool Mid = true>
HG_HD inline bool pic_init(LanePic &P, const BatchArgs &a, int pic, int lane0, int cap) {
    const PicDesc &pd = a.pics[pic];
    if (pd.flags & PD_ASSEMBLY) return false;  // no coded data of its own
    const SeqParams &sp = a.seqs[pd.seq];
    const int log2ctb = sp.log2_ctb, ctb = 1 << log2ctb;
    const int hctb = (sp.height + ctb - 1) >> log2ctb;
    const bool wpp = (sp.flags & SP_WPP) != 0;
    const int R = wpp ? (hctb < cap ? hctb : cap) : 1;
    P.R = R;
    P.lane0 = lane0;
    P.ring = wpp && hctb > R;
    P.W = sp.width;
    P.H = sp.height;
    P.log2ctb = log2ctb;
    P.wctb = (sp.width + ctb - 1) >> log2ctb;
    P.hctb = hctb;
    P.minCb = sp.log2_min_cb;
    P.minTb = sp.log2_min_tb;
    P.maxTb = sp.log2_max_tb;
    P.maxDepthIntra = sp.max_th_depth_intra;
    P.chroma = sp.chroma_format;
    P.subx = (sp.chroma_format == 1 || sp.chroma_format == 2) ? 1 : 0;
    P.suby = sp.chroma_format == 1 ? 1 : 0;
    P.log2qg = log2ctb - sp.diff_cu_qp_delta_depth;
    P.bdY = sp.bit_depth_y;
    P.bdC = sp.bit_depth_c;
    P.qpbdY = 6 * (sp.bit_depth_y - 8);
    P.qpbdC = 6 * (sp.bit_depth_c - 8);
    P.pcmMin = sp.log2_min_pcm;
    P.pcmMax = sp.log2_max_pcm;
    P.pcmBdY = sp.pcm_bd_y;
    P.pcmBdC = sp.pcm_bd_c;
    P.cbOff = sp.cb_qp_offset + pd.cb_qp_off;
    P.crOff = sp.cr_qp_offset + pd.cr_qp_off;
    P.sliceQp = pd.slice_qp;
    P.w4 = (sp.width + 3) >> 2;
    P.h4 = (sp.height + 3) >> 2;
    P.w8 = (sp.width + 7) >> 3;
    P.saoL = pd.sao_luma;
    P.saoC = pd.sao_chroma;
    // (bits 16-30: the picture's segment starts inside rows, PicDesc.flags; lanes_nmid)
    P.flags = sp.flags | (a.xntu ? PF_COHERENT : 0u) | (Mid ? pd.flags & (PD_NMID_MAX << PD_NMID_SHIFT) : 0u);
    P.bits_off = (uint32_t)pd.bits_off;
    P.bits_end = (uint32_t)pd.bits_off + a.rsubs[pd.sub_first + pd.n_sub];  // RBSP end (k_rbsp)
    P.sub_first = pd.sub_first;
    P.row_off = pd.row_off;
    P.tu_cap = pd.tu_cap_row;
    P.coef_cap = pd.coef_cap_row;
    P.pic = (uint32_t)pic;
    // (Mid: the vector engines; their slot of the QpY map's pointer holds the picture's CU list)
    if constexpr (Mid) P.gqpy = (int8_t HG_GAS *)(a.cus + cu_list_off(pd.sao_off, a.max_log2ctb));
    else P.gqpy = (int8_t HG_GAS *)(a.maps + pd.map_off);
    P.gflags = (uint8_t HG_GAS *)(a.maps + pd.map_off + (size_t)P.w4 * P.h4);
    P.gdepth = (uint8_t HG_GAS *)(a.maps + pd.map_off + 2 * (size_t)P.w4 * P.h4);
    P.gsao = (SaoParams HG_GAS *)(a.sao + pd.sao_off);
    P.tu_base = (TuRec HG_GAS *)(a.tus + pd.tu_off);
    P.coef_base = (Coef HG_GAS *)(a.coefs + pd.coef_off);
    return true;
}

// lane state at the start of substream `row` of picture P
HG_HD inline void lane_start(Lane &L, const LanePic &P, LaneLds &ld, int row) {
    L.status = 0;
    L.cn = 0;
    L.k = 8;
    L.ai = L.bv = L.fp = 0;
    L.lb = 0;
    L.fl = (P.flags & SP_WPP) ? F_WPP : 0u;  // (no segment started inside a row yet: bits 16-31)
    L.row = row;
    L.c = 0;
    L.qp_prev_last = P.sliceQp;
    row_outputs(L, P);
    L.st = U_CTU;
}

template <bool Mid = true>
HG_HD inline bool lane_init(Lane &L, LanePic &P, LaneLds &ld, const BatchArgs &a, int pic, int row, int lane0,
                            int cap) {
    if (!pic_init<Mid>(P, a, pic, lane0, cap) || row >= P.R) return false;
    lane_start(L, P, ld, row);
    if constexpr (Mid) L.ncu = 0;  // the vector engines' CU words of the row
    return true;
}

}  // namespace
}  // namespace hg
