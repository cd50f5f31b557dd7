// parse_lanes_body.hpp — CABAC slice-data parser (pipeline stage 1), one
// substream per LANE: the body of k_parse_lanes (parse_lanes.hip, every coding
// tool) and k_parse_lean (parse_lean.hip, the lean tool set), over the syntax
// units of parse_units.hpp.
//
// Replaces SliceSegmentReader::read_data / read_coding_tree_unit and the
// todo!() sao() / coding_quadtree() of src/hevc/slice.rs:206-256, with the
// engine of src/cabac/arithmetic.rs and the binarizations of
// src/cabac/decoder.rs, plus everything H.265 needs below them (7.3.8.3-14,
// 9.3.4.2 ctxInc, 8.4.2 MPM, 8.6.1 QP).  Outputs: TU records, coefficients,
// the QP / edge maps, SAO parameters and per-row counts (desc.hpp).
//
// Every lane of a wave runs its own substream: with WPP a lane is one CTB
// row of a picture and a picture's rows sit in consecutive lanes (R =
// min(rows, 64) lanes; a picture with more than 64 rows wraps round them, lane
// r taking rows r, r + R, r + 2R, ...); without WPP the slice is one
// substream and one lane walks all of its rows.  Each lane walks its substream as a sequence of
// syntax units (CTU start + SAO, coding-quadtree descent, coding-unit header,
// transform-tree descent + transform_unit, residual header, one 4x4
// sub-block, CTU end); one pass of the kernel loop runs one unit on every
// live lane, the lanes in the same kind of unit sharing its instructions, and
// the arithmetic decoder (context bytes in the lane's LDS block) runs inline
// inside the units.  So up to 64 substreams share each engine instruction,
// where k_parse spends a whole wave on one.
//
// WPP (9.3.1) inside the wave: row r+1 starts CTU c once row r has finished
// CTU c+1 (per-lane progress words in LDS, counting r * wctb + CTUs done so
// they stay monotone when a lane wraps to a later row); row r writes its
// contexts after CTU 1 straight into row r+1's lane block, or, when rows wrap
// (that lane may still be parsing an earlier row), into its staging block.  The CtDepth of a CTB's bottom
// 8x8 row and its SAO parameters reach the row below through global memory
// (maps arena / SAO array), read with L1-bypassing loads.
//
// Left / above neighbour state (IntraPredModeY, CtDepth, QpY) needs no CTB
// map: in z-order the last block written in a 4x4 (8x8) row of the CTB row is
// always the left neighbour of the next block in that row, and likewise for
// columns within a CTB, so a "last written" value per row and per column is
// enough (ipmL/ipmA, dL/dA, qL/qA).
#pragma once
#include "parse_units.hpp"

#include <type_traits>

namespace hg {

// a register budget of 256 (2 waves per SIMD, the occupancy the VGPR floor
// below fixes anyway); 0 leaves it to the compiler
#if !defined(HG_PARSE_WPE)
#define HG_PARSE_WPE 2
#endif
#if HG_PARSE_WPE > 0
#define HG_PARSE_ATTR __attribute__((amdgpu_waves_per_eu(HG_PARSE_WPE)))
#else
#define HG_PARSE_ATTR
#endif
// the lanes parse with engine EG (Eng: every tool, k_parse_lanes; EngLean: k_parse_lean)
template <class EG>
__device__ __forceinline__ void parse_lanes_body(const BatchArgs &a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int ppw = a.parse_group;  // pictures per wave (launch_parse)
    const int nl = ppw * a.lane_rows;
    LaneLds *s_lds = reinterpret_cast<LaneLds *>(smem);
    LanePic *s_pic = reinterpret_cast<LanePic *>(smem + lane_blocks_bytes(nl));
    uint32_t *s_prog = reinterpret_cast<uint32_t *>(s_pic + ppw);
    uint64_t *s_tab = reinterpret_cast<uint64_t *>(s_prog + 64);
    uint64_t *s_seq = s_tab + kTabRows;
    uint8_t *s_scan = reinterpret_cast<uint8_t *>(s_seq + 16);
    uint8_t *s_wctx = !EG::kLean && a.wpp_ring ? s_scan + 128 : nullptr;
    const int lane = threadIdx.x;
#if HG_PARSE_SETPRIO > 0
    // the parse is the latency-critical stream: win issue arbitration against
    // the reconstruction kernels of the previous decode sharing the SIMD
    __builtin_amdgcn_s_setprio(HG_PARSE_SETPRIO);
#endif
#if !defined(HG_PARSE_NO_VGPR_FLOOR)
    // at least 176 VGPRs, so at most 2 parse waves per SIMD whatever the allocator
    // needs: at <= 168 a SIMD takes 3, the reconstruction kernels beside them find no
    // room and the step loses 7 % (A/B in DESIGN 5.11)
    asm volatile("" ::: "v175");
#endif
    for (int i = lane; i < kTabRows; i += 64) s_tab[i] = state_row_ctx(i);
    if (lane < 15) s_seq[lane] = sig_seq(lane);
    scan8_tables(s_scan, lane);
    const int pl = lane / a.lane_rows, row = lane % a.lane_rows;
    const int slot = (int)blockIdx.x * ppw + pl;
    const int n_slots = a.parse_order ? a.n_slots : a.n_pics;
    const bool in = pl < ppw && slot < n_slots && (!a.parse_order || a.parse_order[slot] != ~0u);
    const int pic = a.pic0 + (in && a.parse_order ? (int)a.parse_order[slot] : slot);
    Lane L;
    LaneLds &ld = s_lds[lane < nl ? lane : 0];
    LanePic &P = s_pic[pl < ppw ? pl : 0];
    s_prog[lane] = 0;
    const bool live = in && lane_init(L, P, ld, a, pic, row, pl * a.lane_rows, a.lane_rows);
    if (!live) L.st = U_DONE;
#if defined(HG_PARSE_PROF_SB)
    for (int k = 0; k < 6; ++k) L.psb[k] = 0;
#endif
    __syncthreads();
    const Env E{&a, s_lds, s_prog, s_wctx, lane};
    const EG G{ld.ctx, s_tab, s_seq, a.rbsp, live ? (P.bits_end + 64u) & ~3u : 0u, s_scan, s_scan + 64};
#if defined(HG_PARSE_PROF)
    uint64_t pf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t t_start = __builtin_amdgcn_s_memtime();
    const uint64_t rt_start = __builtin_amdgcn_s_memrealtime();
#endif
#if defined(HG_PARSE_PROF)
    uint64_t pw = 0;                                // the passes' start (pass_wait, q_refill)
    uint32_t kc[U_TBD] = {0, 0, 0, 0, 0, 0, 0, 0};  // passes that ran each unit kind
#endif
    for (uint32_t pass = 0;; ++pass) {
        if (!__any(L.st != U_DONE)) break;
#if defined(HG_PARSE_PROF)
        const uint64_t t0 = __builtin_amdgcn_s_memtime();
#endif
        pass_wait();
        if (live) q_refill(L, G);
#if defined(HG_PARSE_PROF)
        pw += __builtin_amdgcn_s_memtime() - t0;
#endif
        // one pass: every unit kind in syntax order, each run by the lanes in it
        // (a uniform loop: the units are never linearised into one divergent region)
        bool progressed = false;
        // (a lambda per step, not a loop over pass_kind: each step's kind has to be a
        // constant, and the optimizer does not unroll the loop once it has eight steps)
        auto step = [&](auto kind_c) __attribute__((always_inline)) {
            constexpr int kind = decltype(kind_c)::value;
            const bool mine = L.st == kind && (kind != U_CTU || ctu_ready<EG>(L, P, E));
            if (!__any(mine)) return;
            progressed = true;
#if defined(HG_PARSE_PROF)
            ++kc[kind - 1];
            const uint64_t t1 = __builtin_amdgcn_s_memtime();
            pf[7] += (uint64_t)__popcll(__ballot(mine));  // lanes running a unit
#endif
            if (mine) run_unit(kind, L, ld, P, E, G);
#if defined(HG_PARSE_PROF)
            const uint64_t t2 = __builtin_amdgcn_s_memtime();
            // (U_TBD with the TB unit: its no-cbf path held that code before)
            pf[kind <= U_CTU ? 2 : kind <= U_TT ? 3 : kind == U_TBD ? 4 : kind - 1] += t2 - t1;
#endif
        };
        step(std::integral_constant<int, pass_kind(0)>{});
        step(std::integral_constant<int, pass_kind(1)>{});
        step(std::integral_constant<int, pass_kind(2)>{});
        step(std::integral_constant<int, pass_kind(3)>{});
        step(std::integral_constant<int, pass_kind(4)>{});
        step(std::integral_constant<int, pass_kind(5)>{});
        step(std::integral_constant<int, pass_kind(6)>{});
        step(std::integral_constant<int, pass_kind(7)>{});
        static_assert(kPassKinds == 8, "one step per kind of the pass");
#if defined(HG_PARSE_PROF)
        ++pf[1];
#endif
        if (!progressed || pass > (1u << 30)) {  // every live lane waits: cannot happen (the top row never waits)
            if (L.st != U_DONE) {
                L.status |= ST_SUBSTREAM_END;
                atomicOr(&a.status[P.pic], L.status & ~ST_SEGSW);
            }
            break;
        }
    }
#if defined(HG_PARSE_PROF)
    pf[0] = __builtin_amdgcn_s_memtime() - t_start;
    if (lane == 0)
        for (int k = 0; k < 8; ++k) atomicAdd((unsigned long long *)&g_prof_lanes[k], (unsigned long long)pf[k]);
#if defined(HG_PARSE_PROF_SB)
    // the sub-block unit's phases (slots 8..13: header, sig loop, greater1/2,
    // signs + remainders + record, sig bins, -; `make prof-tb`: the tree / TB units' six,
    // HG_TB_T of parse_state.hpp), the wave's time: one lane per run
    if (live) {
        for (int k = 0; k < 6; ++k) atomicAdd((unsigned long long *)&g_prof_lanes[8 + k], (unsigned long long)L.psb[k]);
        if (blockIdx.x < (unsigned)kWaveRecCap)  // and per wave (records 3 and 4 of the wave's breakdown)
            for (int k = 0; k < 6; ++k)
                atomicAdd((unsigned long long *)&g_ctu_t[kWaveRec + (3 + k / 3) * kWaveRecCap + blockIdx.x][k % 3],
                          (unsigned long long)L.psb[k]);
    }
#endif
    // per wave (the CTU-time slots, unused by this kernel): s_memrealtime at its start, its
    // duration and place, then the passes and its first three pictures (16 bits each; 0xffff: none)
    if (blockIdx.x < (unsigned)kCtuTimeCap) {
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane(in ? pic : 0xffff, 0);
        const uint32_t p1 = (uint32_t)__builtin_amdgcn_readlane(in ? pic : 0xffff, a.lane_rows < 64 ? a.lane_rows : 0);
        const uint32_t p2 =
            (uint32_t)__builtin_amdgcn_readlane(in ? pic : 0xffff, 2 * a.lane_rows < 64 ? 2 * a.lane_rows : 0);
        uint32_t hwid, xcc;  // where the wave ran: HW_ID (SIMD, CU, SH, SE) and the XCD
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if (lane == 0) {
            g_ctu_t[blockIdx.x][0] = rt_start;
            // the wave's duration (low 32 bits), then HW_ID[15:0] and XCC_ID[3:0]
            g_ctu_t[blockIdx.x][1] = ((__builtin_amdgcn_s_memrealtime() - rt_start) & 0xffffffffu) |
                                     ((uint64_t)((hwid & 0xffffu) | ((xcc & 0xfu) << 16)) << 32);
            g_ctu_t[blockIdx.x][2] = (pf[1] & 0xffffu) | ((uint64_t)(p0 & 0xffffu) << 16) |
                                     ((uint64_t)(p1 & 0xffffu) << 32) | ((uint64_t)(p2 & 0xffffu) << 48);
            // the wave's own breakdown (tools/wave_times.py): s_memtime cycles of the
            // wave, per unit kind group (pf[2..6]), of the pass starts, the lanes x
            // units / 4, and the passes that ran each unit kind (16 bits each; U_TBD's
            // above the pass starts' 48 bits)
            if (blockIdx.x < (unsigned)kWaveRecCap) {
                uint64_t *r = &g_ctu_t[kWaveRec + blockIdx.x][0];
                uint64_t *r2 = &g_ctu_t[kWaveRec + kWaveRecCap + blockIdx.x][0];
                uint64_t *r3 = &g_ctu_t[kWaveRec + 2 * kWaveRecCap + blockIdx.x][0];
                r[0] = pf[0], r[1] = pf[2], r[2] = pf[3];
                r2[0] = pf[4], r2[1] = pf[5], r2[2] = pf[6];
                r3[0] = (pw & 0xffffffffffffull) | ((uint64_t)std::min<uint32_t>(kc[7], 0xffffu) << 48);
                r3[1] = (uint64_t)kc[0] | ((uint64_t)kc[1] << 16) | ((uint64_t)kc[2] << 32) | ((uint64_t)kc[3] << 48);
                r3[2] = (uint64_t)kc[4] | ((uint64_t)kc[5] << 16) | ((uint64_t)kc[6] << 32) |
                        (std::min<uint64_t>(pf[7] >> 2, 0xffffu) << 48);
            }
        }
    }
#endif
}

}  // namespace hg
