// emu_parse.cpp — the host emulation's drivers of the CABAC parse (HG_HOST_EMU,
// test only): the syntax units of kernels/parse_units.hpp on the CPU, in the
// order the kernels of kernels/parse_*.hip run them.  HEIFGPU_LANES_STATS
// prints the lanes driver's per-wave counts, HEIFGPU_EMU_PASS_ORDER reorders
// the unit kinds of its pass.
#include "../kernels/parse_units.hpp"

#include <cstdio>
#include <string>
#include <vector>

namespace hg {

// one wave at a time, one unit per live lane per pass, lanes in order
template <class EG>
void emu_parse_lanes(const BatchArgs &a) {
    const int ppw = a.parse_order && a.parse_group > 0 ? a.parse_group : lanes_pics_per_wave(a.lane_rows, a.n_pics);
    const int n_slots = a.parse_order ? a.n_slots : a.n_pics;
    const int waves = (n_slots + ppw - 1) / ppw;
    uint64_t tab[kTabRows], seq[15];
    uint8_t scan8[128];
    for (int i = 0; i < 64; ++i) scan8_tables(scan8, i);
    for (int i = 0; i < kTabRows; ++i) tab[i] = state_row_ctx(i);
    for (int i = 0; i < 15; ++i) seq[i] = sig_seq(i);
    std::vector<LaneLds> lds(64);
    std::vector<LanePic> pics(64);
    std::vector<Lane> lanes(64);
    std::vector<uint8_t> wctx(a.wpp_ring ? 64 * CTX_PAD : 0);
    uint32_t prog[64];
    static const bool stats = std::getenv("HEIFGPU_LANES_STATS") != nullptr;
    // modelling knob (emulation only): the unit kinds of one pass, in order, as
    // digits (default "12345687", pass_kind: U_CTU .. U_SB, U_TBD, U_CTU_END once);
    // characters that name no unit kind are ignored
    static const std::string order = [] {
        const char *e = std::getenv("HEIFGPU_EMU_PASS_ORDER");
        std::string o;
        if (e && *e) {
            for (const char *c = e; *c; ++c)
                if (*c >= '0' + U_CTU && *c <= '0' + U_TBD) o += *c;
        } else {
            for (int i = 0; i < kPassKinds; ++i) o += (char)('0' + pass_kind(i));
        }
        return o;
    }();
    for (int w = 0; w < waves; ++w) {
        for (int l = 0; l < 64; ++l) {
            prog[l] = 0;
            const int pl = l / a.lane_rows, row = l % a.lane_rows;
            const int slot = w * ppw + pl;
            const bool in = pl < ppw && slot < n_slots && (!a.parse_order || a.parse_order[slot] != ~0u);
            const int pic = a.pic0 + (in && a.parse_order ? (int)a.parse_order[slot] : slot);
            const bool live = in && lane_init(lanes[l], pics[pl], lds[l], a, pic, row, pl * a.lane_rows, a.lane_rows);
            if (!live) lanes[l].st = U_DONE;
        }
        Env E{&a, lds.data(), prog, a.wpp_ring ? wctx.data() : nullptr, 0};
        long passes = 0, units = 0, kruns = 0, kr[U_TBD + 1] = {}, ku[U_TBD + 1] = {};
        for (;; ++passes) {
            bool any = false, progressed = false;
            for (int l = 0; l < 64; ++l) any |= lanes[l].st != U_DONE;
            if (!any) break;
            for (int l = 0; l < 64; ++l)
                if (lanes[l].st != U_DONE) {
                    const LanePic &P = pics[l / a.lane_rows];
                    const EG G{lds[l].ctx, tab, seq, a.rbsp, (P.bits_end + 64u) & ~3u, scan8, scan8 + 64};
                    q_refill(lanes[l], G);
                }
            // the kernel's pass: every unit kind in syntax order, each on the lanes in it
            for (const char ch : order) {
                const int kind = ch - '0';
                bool mine[64], anym = false;
                int cnt = 0;
                for (int l = 0; l < 64; ++l) {
                    E.lane = l;
                    mine[l] = lanes[l].st == kind && (kind != U_CTU || ctu_ready<EG>(lanes[l], pics[l / a.lane_rows], E));
                    anym |= mine[l];
                    cnt += mine[l] ? 1 : 0;
                }
                if (!anym) continue;
                ++kruns;
                ++kr[kind];
                ku[kind] += cnt;
                if (kind == U_SB) {
                    bool any4 = false;
                    for (int l = 0; l < 64; ++l) any4 |= mine[l] && lanes[l].tb_log2 == 2;
                    HG_COV(any4 ? COV_SB_RUN_ANY4 : COV_SB_RUN_NO4);
                }
                for (int l = 0; l < 64; ++l) {
                    Lane &L = lanes[l];
                    E.lane = l;
                    LanePic &P = pics[l / a.lane_rows];
                    if (!mine[l]) continue;
                    progressed = true;
                    ++units;
                    const EG G{lds[l].ctx, tab, seq, a.rbsp, (P.bits_end + 64u) & ~3u, scan8, scan8 + 64};
                    run_unit(kind, L, lds[l], P, E, G);
                }
            }
            if (!progressed) {  // every live lane waits: cannot happen (the top row never waits)
                for (int l = 0; l < 64; ++l)
                    if (lanes[l].st != U_DONE) {
                        lanes[l].status |= ST_SUBSTREAM_END;
                        atomicOr(&a.status[pics[l / a.lane_rows].pic], lanes[l].status & ~ST_SEGSW);
                        lanes[l].st = U_DONE;
                    }
                break;
            }
        }
        if (stats) {
            printf("wave %d: %ld passes, %.1f units per pass, %ld kind runs, %.2f units per kind run\n", w, passes,
                   (double)units / passes, kruns, (double)units / kruns);
            printf("  runs");
            for (int k = U_CTU; k <= U_TBD; ++k) printf(" %ld", kr[k]);
            printf("\n  units");
            for (int k = U_CTU; k <= U_TBD; ++k) printf(" %ld", ku[k]);
            printf("\n  paths");  // (Cov, counted since the last wave)
            for (int k = 0; k < COV_N; ++k) printf(" %ld", g_cov[k]), g_cov[k] = 0;
            printf("\n  sb_paths");
            for (int k = COV_N; k < COV_SB_END; ++k) printf(" %ld", g_cov[k]), g_cov[k] = 0;
            printf("\n  tb_paths");
            for (int k = COV_SB_END; k < COV_TB_END; ++k) printf(" %ld", g_cov[k]), g_cov[k] = 0;
            printf("\n  cu_paths");
            for (int k = COV_TB_END; k < COV_ALL; ++k) printf(" %ld", g_cov[k]), g_cov[k] = 0;
            printf("\n");
        }
    }
}

// solo mode: each picture's rows (waves) round-robin, one unit per ready wave
// per round, with the GPU driver's window logic (SoloWin) per wave
template <bool Spread>
void emu_parse_solo(const BatchArgs &a) {
    using EG = EngSoloT<Spread>;
    const int NW = Spread ? a.max_rows : a.solo_waves;  // spread: every row of a picture its own wave
    const int n_slots = a.parse_order ? a.n_slots : a.n_pics;
    uint64_t seq[15];
    for (int i = 0; i < 15; ++i) seq[i] = sig_seq(i);
    std::vector<LaneLds> lds((size_t)NW);
    std::vector<Lane> lanes((size_t)NW);
    std::vector<uint8_t> wctx((size_t)NW * CTX_PAD);
    std::vector<uint32_t> wbuf((size_t)NW * 192);
    std::vector<SoloWin> wins((size_t)NW);
    LanePic P;
    uint32_t prog[64];
    for (int slot = 0; slot < n_slots; ++slot) {
        const bool in = !a.parse_order || a.parse_order[slot] != ~0u;
        if (!in) continue;
        // spread: one entry per row (row << 20 | picture); the picture's row-0 entry runs all its rows here
        const uint32_t ent = a.parse_order ? a.parse_order[slot] : (uint32_t)slot;
        if (Spread && (ent >> 20) != 0) continue;
        const int pic = a.pic0 + (int)(Spread ? (ent & 0xfffffu) : ent);
        for (int w = 0; w < NW; ++w) {
            prog[w] = 0;
            if (!lane_init<false>(lanes[(size_t)w], P, lds[(size_t)w], a, pic, w, 0, Spread ? (1 << 20) : NW))
                lanes[(size_t)w].st = U_DONE;
            wins[(size_t)w].w = &wbuf[(size_t)w * 192];
            wins[(size_t)w].f = &wbuf[(size_t)w * 192 + 128];
        }
        const uint32_t lim = (P.bits_end + 64u) & ~3u;
        if (Spread)
            for (int w = 0; w < P.R; ++w) a.xprog[P.row_off + (uint32_t)w] = 0;  // this picture's words only
        Env E = Spread ? Env{&a, lds.data(), a.xprog + P.row_off, a.xctx + (size_t)P.row_off * CTX_PAD, 0}
                       : Env{&a, lds.data(), prog, wctx.data(), 0};
        for (;;) {
            bool any = false, progressed = false;
            for (int w = 0; w < NW; ++w) {
                Lane &L = lanes[(size_t)w];
                if (L.st == U_DONE) continue;
                any = true;
                E.lane = w;
                if (L.st == U_CTU && !ctu_ready<EG>(L, P, E)) continue;
                progressed = true;
                SoloWin &sw = wins[(size_t)w];
                const uint32_t start = L.st == U_CTU ? substream_start<EG>(L, P, a) : ~0u;
                if (start != ~0u) sw.restart(a.rbsp, start, lim, 0);
                else sw.advance(a.rbsp, L.lb, lim, 0);
                const EG G{lds[(size_t)w].ctx, 0u, 0u, seq, a.rbsp, lim, sw.view(), 0u, 0u, 0u};
                run_unit(L.st, L, lds[(size_t)w], P, E, G);
            }
            if (!any) break;
            if (!progressed) {
                for (int w = 0; w < NW; ++w)
                    if (lanes[(size_t)w].st != U_DONE) {
                        lanes[(size_t)w].status |= ST_SUBSTREAM_END;
                        atomicOr(&a.status[P.pic], lanes[(size_t)w].status);
                        lanes[(size_t)w].st = U_DONE;
                    }
                break;
            }
        }
    }
}

void emu_parse(const BatchArgs &a) {
    if (a.parse_mode == PARSE_SOLO) emu_parse_solo<false>(a);
    else if (a.parse_mode == PARSE_SPREAD) emu_parse_solo<true>(a);
    else if (a.lanes_lean) emu_parse_lanes<EngLean>(a);  // the body launch_parse would run
    else emu_parse_lanes<Eng>(a);
}

}  // namespace hg
