// parse_state.hpp — what every CABAC parse kernel and the host emulation's
// drivers share below the engines: the engine tables, the per-lane LDS block,
// the picture constants, the syntax-unit and flag enums, the lane state, the
// emulation's path counters and the tuning builds' counters with their read-out.
// (parse_engine.hpp: the engines; parse_units.hpp: the syntax units)
#pragma once
#include "cabac.hpp"
#include "kernels.hpp"
#include "tables.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(HG_HOST_EMU)
#include <cstdio>
#endif

#if !defined(HG_HOST_EMU)
// v_writelane_b32 (this clang exposes no builtin for it): lane `lane` of `old` := src
extern "C" __device__ int hg_writelane(int src, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
#endif
// branches a conforming stream of ordinary content almost never takes (substream
// starts, the escape form of coeff_abs_level_remaining, capacity and syntax
// errors): laid out after the units' hot blocks (HG_NO_COLD_HINTS turns the
// hints off; A/B in DESIGN 5.15)
#if !defined(HG_NO_COLD_HINTS)
#define HG_UNLIKELY(x) __builtin_expect(!!(x), 0)
#define HG_LIKELY(x) __builtin_expect(!!(x), 1)
#else
#define HG_UNLIKELY(x) (x)
#define HG_LIKELY(x) (x)
#endif

namespace hg {

namespace {
__constant__ uint8_t c_lps_l[256] = {HG_LPS_TABLE};
__constant__ uint8_t c_trans_l[64] = {HG_TRANS_LPS};
__constant__ uint8_t c_ctx_init_l[CTX_NUM] = {HG_CTX_INIT_VALUES};
}  // namespace
#if defined(HG_PARSE_PROF) && !defined(HG_HOST_EMU)
// s_memtime cycles per wave: [0] kernel, [1] passes, [2..6] unit kinds CTU, tree (CQT+CU+TT), TB, SB,
// CTU_END; [7] units run (lanes x unit executions) (tuning build only; heifgpu_debug_counters slots 8..15)
__device__ uint64_t g_prof_lanes[16];  // 8 used; 16 in the prof-sb build
// solo / spread: per CTU (index (global CTB row) * 128 + column) s_memrealtime of
// the first time its wave wanted to start it, the start of its U_CTU unit and
// the end of its U_CTU_END unit (heifgpu_debug_counters slots 8 on)
constexpr int kCtuTimeCap = 1 << 17;
__device__ uint64_t g_ctu_t[kCtuTimeCap][3];
// k_parse_lanes (one wave per workgroup): records kWaveRec.. of g_ctu_t hold
// each wave's own cycle breakdown, three records per wave (five in prof-sb)
constexpr int kWaveRec = 4096, kWaveRecCap = 4096;
#endif

namespace {

// engine row of pStateIdx st (Eng::tab): rangeTabLps[st][0..3], then the
// next context byte (pStateIdx << 1 | valMps) to XOR with valMps after an LPS
// (transIdxLps << 1, | 1 at pStateIdx 0 where valMps flips) and after an MPS
// (transIdxMps << 1)
HG_HD inline uint64_t state_row(int st) {
    uint64_t r = 0;
    for (int q = 0; q < 4; ++q) r |= (uint64_t)c_lps_l[(st << 2) | q] << (8 * q);
    const uint64_t lps_next = ((uint64_t)c_trans_l[st] << 1) | (st == 0 ? 1u : 0u);
    const uint64_t mps_next = (uint64_t)(st < 62 ? st + 1 : st) << 1;
    return r | (lps_next << 32) | (mps_next << 40);
}

// Vector engines (lanes): one row per context byte s = pStateIdx << 1 |
// valMps, valMps folded in: rangeTabLps[4], then the next context byte after
// an LPS (bits 32-38) and after an MPS (bits 40-46), each with the bin that
// path decodes to in its bit 7.  A decision indexes it by the byte itself and
// reads the new byte and the bin from one shift (no valMps extraction, XOR or
// row-index masking; r05 A/B at 128 images: 18,770 vs 18,590 Mpix/s); a
// register cache inserts the shifted byte under a 7-bit mask (v_bfi), so the
// bin bit costs no extra mask there (dec_t; r06 A/B: VALU 19.92 -> 19.60 G per
// launch, 23,056 -> 23,108 Mpix/s, profiles/r06/ab/ab_bfi.txt).
// (A/B r05: the decoded bin in bit 7 of the context byte itself, 256 rows:
// 19,020 vs 19,200 Mpix/s, rejected)
constexpr int kTabRows = 128;
HG_HD inline uint64_t state_row_ctx(int s) {
    const uint64_t r = state_row(s >> 1);
    const uint64_t mps = (uint64_t)(s & 1);
    return (r & 0xffffffffull) | (((((r >> 32) & 0xffu) ^ mps) | ((mps ^ 1u) << 7)) << 32) |
           (((((r >> 40) & 0xffu) ^ mps) | (mps << 7)) << 40);
}

constexpr uint32_t kProgDone = 0x7fffffffu;
// (parse waves at issue priority HG_PARSE_SETPRIO: wave.hpp)
// LanePic.flags bit above the SP_ flags: k_intra_stream reads this picture's TU
// and coefficient records while the parse writes them (agent-scope stores)
constexpr uint32_t PF_COHERENT = 1u << 31;

// per-lane LDS block (208 bytes: lanes l and l + 16 share a bank for one
// context byte; an odd 212-byte block, 64 banks, measured 76.8 vs 76.3 ms, r04)
struct alignas(16) LaneLds {
    uint8_t ctx[CTX_PAD];
    uint8_t ipmL[16], ipmA[16];  // IntraPredModeY (4x4 units): last written per row / per column
    uint8_t dL[8], dA[8];        // CtDepth (8x8 units)
    int8_t qL[8], qA[8];         // QpY (8x8 units)
};
// (the vector engines update a CU's or PB's segment of these lines as a masked 64-bit word)
static_assert(offsetof(LaneLds, ipmL) % 8 == 0 && offsetof(LaneLds, ipmA) % 8 == 0, "64-bit line updates");
static_assert(offsetof(LaneLds, dL) % 8 == 0 && offsetof(LaneLds, dA) % 8 == 0, "64-bit line updates");

// picture constants and output pointers (LDS, one per picture of the wave)
struct LanePic {
    int W, H, log2ctb, wctb, hctb, minCb, minTb, maxTb, maxDepthIntra, chroma;
    int log2qg, bdY, bdC, qpbdY, qpbdC, pcmMin, pcmMax, pcmBdY, pcmBdC, cbOff, crOff, sliceQp;
    int subx, suby;  // log2 SubWidthC, SubHeightC (Table 6-1)
    int w4, h4, w8, saoL, saoC;
    int R, lane0, ring;  // lanes of the picture, its first lane, rows wrap round the lanes (WPP rows > R)
    uint32_t flags, bits_off, bits_end, sub_first, row_off, tu_cap, coef_cap, pic;
    // global memory, said so in the type: a generic pointer loaded from LDS
    // would make every store through it a flat store, and flat stores count in
    // lgkmcnt, so each later LDS read of the wave would wait for them
    // (gqpy: the scalar engines' QpY map, whose rows they write.  The vector engines keep
    // the picture's CU list in the slot instead, lane_cus: they append a word per CU and
    // k_paint_flags paints the rows from the words.  One slot, one type: the struct, and
    // with it the scalar engines' code, stay what they were)
    int8_t HG_GAS *gqpy;
    uint8_t HG_GAS *gflags;
    uint8_t HG_GAS *gdepth;
    SaoParams HG_GAS *gsao;
    TuRec HG_GAS *tu_base;
    Coef HG_GAS *coef_base;
};
HG_HD inline uint32_t HG_GAS *lane_cus(const LanePic &P) { return (uint32_t HG_GAS *)P.gqpy; }

// syntax units (Lane.st)
enum Unit : int {
    U_DONE = 0,
    U_CTU,      // WPP wait, substream start, sao()                      7.3.8.2-3
    U_CQT,      // coding_quadtree descent from the current node         7.3.8.4
    U_CU,       // coding_unit up to transform_tree                      7.3.8.5
    U_TT,       // transform_tree descent + transform_unit               7.3.8.8-10
    U_TB,       // next TB of the TU: record, or residual_coding header  7.3.8.11
    U_SB,       // one 4x4 sub-block of residual_coding                  7.3.8.11
    U_CTU_END,  // end_of_slice_segment_flag / end_of_subset_one_bit     7.3.8.1
    // (vector engines) a finished TB: its record, then the next TB / tree node /
    // CU end (tb_done).  Numbered last, so the kinds before it keep their counter
    // slots; it runs between U_SB and U_CTU_END (pass_kind)
    U_TBD,
};
// One pass of the lanes parse: every unit kind in syntax order.  U_TB (a TB
// without coefficients) and U_SB (a TB's last sub-block) only mark the lane
// U_TBD, so the record store, the tree walks and the CU's QpY rows run once per
// pass for the lanes of both origins, not once inside each unit.  tb_done
// leaves a lane in U_TB, U_TT or U_CQT (all earlier in the order: the next
// pass, as when the units called it) or in U_CTU_END (later: the same pass).
constexpr int kPassKinds = 8;
// kind of the pass's step i: U_CTU .. U_SB, U_TBD, U_CTU_END (arithmetic, not a
// table: the kernel's unrolled pass loop needs each step's kind as a constant)
HG_HD constexpr int pass_kind(int i) { return i < U_SB ? i + 1 : (i == U_SB ? (int)U_TBD : (int)U_CTU_END); }

// Lane.fl bits
enum : uint32_t {
    F_WPP = 1u << 0,
    F_FIRST_QG = 1u << 1,
    F_QG_NEW = 1u << 2,
    F_DQP_CODED = 1u << 3,
    F_BYPASS = 1u << 4,   // cu_transquant_bypass_flag
    F_NXN = 1u << 5,      // PART_NxN
    F_CBF_L = 1u << 6,
    F_CBF_CB = 1u << 7,
    F_CBF_CR = 1u << 8,
    F_TS = 1u << 9,       // transform_skip_flag of the current TB
    F_TB_CBF = 1u << 10,
    F_ANY_SB = 1u << 11,  // a sub-block of the TB had significant coefficients
    F_STOP = 1u << 12,
    F_PCM = 1u << 13,     // the TB being recorded is a PCM block
    F_REINIT = 1u << 14,  // solo modes: engine re-initialisation at byte L.reinit before the next unit
    // bits 16-31: the dependent segments started inside a row so far (kMsegOne
    // each; in fl, not a register of its own: the lanes parse sits at its VGPR floor)
};
constexpr uint32_t kMsegShift = 16, kMsegOne = 1u << kMsegShift;
// Lane.status bit, never reported (unit_ctu clears it): a dependent slice
// segment starts at the next CTU, inside the row (lanes_nmid).  Carried in
// status, which the CTU end's error branch writes anyway: set in fl there, the
// flag cost the lanes parse 16 VGPRs of allocation (160 -> 176)
constexpr uint32_t ST_SEGSW = 1u << 30;

struct Lane {
    // arithmetic decoder (9.3.4.3): ivlOffset carried with k look-ahead bits,
    // value = ivlOffset * 2^k + next k bits of the substream, so a renormalisation
    // only lowers k; a bit window tops value up 16 bits at a time
    uint32_t range, value;
    int k;
    uint64_t cur;     // next bits of the substream, MSB first (cn valid)
    int cn;
    // RBSP queue, dwords as loaded (little endian): a (ai consumed), then b (valid: bv), then f (in
    // flight: fp); lb = offset of the 16 bytes after the last loaded block.  f is issued at a pass
    // start and lands at the next one, after the pass's one memory wait, so refills inside a pass
    // never wait on memory (a wait for a load also waits for every older store)
    uint32_t a0, a1, a2, a3, b0, b1, b2, b3, f0, f1, f2, f3;
    int ai, bv, fp;
    uint32_t lb;
    int32_t budget;   // 8 * (bytes from the substream start to the picture's RBSP end) - bits moved into value
    uint32_t status;
    int st;
    uint32_t fl;
    int row, c, ctbx, ctby;
    // coding quadtree / transform tree node
    int qx, qy, ql, qd;
    int tx, ty, tl, td;
    uint32_t tcbf;  // cbf_cb | cbf_cr << 1 (| the 4:2:2 lower TBs' << 2, << 3) of the node at depth d, at bit 4d
    // quantization (8.6.1)
    int qp_prev_last, qp_pred, cu_qp_delta_val, qpy_cur, qg_x, qg_y;
    // coding unit: IntraPredModeY of PB k in byte k, IntraPredModeC
    int cu_modes, cu_chroma;
    // transform block
    int tb_t, tb_n, tb_cidx, tb_x, tb_y, tb_log2, tb_mode;
    uint32_t tb_coef0;
    // residual_coding state carried across sub-blocks
    int rc_scan, rc_last_sub, rc_last_pos, rc_i, rc_prev_c1;
    uint64_t rc_csbf;  // coded_sub_block_flag, bit yS * 8 + xS
    uint32_t ntu, ncoef;
    uint32_t ncu;               // vector engines: CU words of the row (the picture's CU list, cu_done)
    uint32_t nesc;              // escape levels of the row (stored down from the end of its coefficient space)
    uint32_t tu_row, coef_row;  // TuRec / Coef index of the current row's outputs
    // solo mode on the GPU: the context states, byte i of the LDS layout at
    // byte i & 3 of lane i >> 2 (35 lanes), read / written with v_readlane /
    // v_writelane; the one field whose lanes differ
    uint32_t cx;
    uint32_t reinit;  // F_REINIT: RBSP byte (absolute) where the engine restarts after PCM samples
#if defined(HG_PARSE_PROF_SB)
    // solo tuning build: s_memtime cycles of unit_sb's phases (header, sig loop,
    // greater1/2, signs + levels + coefficient stores) and sig bins / coefficients;
    // lanes kernels of the prof-tb build: the tree / TB units' phases (HG_TB_T below)
    uint64_t psb[6];
#endif
};
#if defined(HG_PARSE_PROF_SB) && !defined(HG_HOST_EMU)
// (the lowest active lane accumulates: in the lanes kernel the lanes running
// the unit share one timeline, so the psb sums over lanes are the wave's time)
#define HG_PHASE_T(L, i, t0)                                                         \
    do {                                                                             \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                            \
        if ((int)__lane_id() == __builtin_ctzll(__ballot(1))) (L).psb[i] += t_ - (t0); \
        (t0) = t_;                                                                   \
    } while (0)
#endif
// `make prof-tb` (HG_PARSE_PROF_TB on top of the prof-sb build) times the tree and
// TB units' phases into the same six slots instead of the sub-block unit's: 0 the
// TB unit up to the last position, 1 the last-position prefix bins, 2 suffixes and
// scan set-up, 3 the transform-tree unit (its map rows included: nothing in the
// vector engines since r13), 4 the QpY lines of a finished CU (LDS), 5 its QpY map
// rows or CU word (global) (tools/wave_times.py names them)
// `make prof-cu` (HG_PARSE_PROF_CU on top of the prof-sb build) times the coding
// quadtree and CU units there instead: 0 the quadtree unit, 1 the CU unit up to its
// CtDepth lines, 2 the CtDepth lines, 3 the prev_intra and mode bins, 4 the luma
// mode derivations with the IntraPredModeY lines, 5 the chroma mode
#if defined(HG_PARSE_PROF_TB) && defined(HG_PARSE_PROF_CU)
#error "prof-tb and prof-cu share the six phase slots: one of them per build"
#endif
#if defined(HG_PARSE_PROF_SB) && !defined(HG_HOST_EMU) && !defined(HG_PARSE_PROF_TB) && !defined(HG_PARSE_PROF_CU)
#define HG_SB_T(L, i, t0) HG_PHASE_T(L, i, t0)
#elif (defined(HG_PARSE_PROF_TB) || defined(HG_PARSE_PROF_CU)) && !defined(HG_HOST_EMU)
#define HG_SB_T(L, i, t0) ((void)(t0))
#else
#define HG_SB_T(L, i, t0) ((void)0)
#endif
#if defined(HG_PARSE_PROF_TB) && !defined(HG_HOST_EMU)
#define HG_TB_T0(t0) uint64_t t0 = __builtin_amdgcn_s_memtime()
#define HG_TB_T(L, i, t0) HG_PHASE_T(L, i, t0)
#else
#define HG_TB_T0(t0) ((void)0)
#define HG_TB_T(L, i, t0) ((void)0)
#endif
#if defined(HG_PARSE_PROF_CU) && !defined(HG_HOST_EMU)
#define HG_CU_T0(t0) uint64_t t0 = __builtin_amdgcn_s_memtime()
#define HG_CU_T(L, i, t0) HG_PHASE_T(L, i, t0)
#else
#define HG_CU_T0(t0) ((void)0)
#define HG_CU_T(L, i, t0) ((void)0)
#endif

// Emulation only (HEIFGPU_LANES_STATS prints them per wave): how often the parse
// took the paths that the small pictures of tests/lanes_units_cases.py are
// chosen for, so the test can tell that a picture reaches the path it names
enum Cov : int {
    COV_TB_LUMA,                      // + log2 - 2: coded luma TBs of 4, 8, 16, 32
    COV_TB_CHROMA = COV_TB_LUMA + 4,  // + log2 - 2: coded chroma TBs
    COV_NXN = COV_TB_CHROMA + 4,      // NxN CUs (four PBs)
    COV_NXN_MPM,                      // their PBs with an MPM: + mpm_idx (0, 1, 2)
    COV_NXN_REM = COV_NXN_MPM + 3,    // and with rem_intra_luma_pred_mode
    COV_DQP,                          // cu_qp_delta_abs
    COV_DQP_EG0,                      // with the EG0 suffix
    COV_LAST_SUFFIX,                  // last_sig_coeff_{x,y}_suffix
    COV_CODED_AFTER_EMPTY,            // a coded Cb TB after the TU's coefficient-free luma TB
    COV_CU_ENDS_IN_SB,                // a CU's last TB ending in a sub-block (not in U_TB)
    COV_TSKIP,                        // transform_skip_flag = 1
    COV_LAST_CTX5,                    // a last_sig_coeff prefix of 9 (32x32 luma: its fifth context)
    COV_N,
    // the sub-block unit's paths (tests/lanes_sb_cases.py), on a `sb_paths` line of their own
    COV_SB_SIG4 = COV_N,  // sub-blocks of 4x4 TBs through the sig_coeff_flag loop (nine context slots)
    COV_SB_SIG,           // and of larger TBs (four slots)
    COV_SB_BEYOND8,       // more than eight significant coefficients
    COV_SB_RICE4,         // a remainder decoded with Rice parameter 4
    COV_SB_ESCAPE,        // an escape level (abs - 1 >= 15)
    COV_SB_EGK,           // a remainder with the EG(k + 1) suffix
    COV_SB_HIDE,          // a hidden sign
    COV_SB_NO_HIDE,       // sign hiding enabled, but first and last too close
    COV_SB_CTXSET_INC,    // ctxSet raised by rc_prev_c1 == 0
    COV_SB_INFER_DC,      // the DC inferred in a coded sub-block
    COV_SB_LAST_POS0,     // a last sub-block with last_pos 0 (no sig_coeff_flag decoded)
    COV_SB_GT2,           // coeff_abs_level_greater2_flag set
    COV_SB_RUN_ANY4,      // unit runs of a wave with a 4x4 TB's lane among them
    COV_SB_RUN_NO4,       // and without one
    COV_SB_END,
    // the residual header's last-position prefixes (tests/lanes_tbhdr_cases.py), on a `tb_paths` line
    COV_LAST_00 = COV_SB_END,  // both prefixes 0 (one bin each)
    COV_LAST_0M,               // x prefix 0, y prefix cMax (no terminating bin)
    COV_LAST_M0,               // x prefix cMax, y prefix 0
    COV_LAST_MM,               // both cMax
    COV_LAST_SUFFIX_X_ONLY,    // a suffix on the x axis alone
    COV_LAST_SUFFIX_Y_ONLY,    // and on the y axis alone
    COV_LAST_SWAP,             // vertical scan: the two positions swapped
    COV_TB_END,
    // the end of a CU (tests/lanes_culist_cases.py), on a `cu_paths` line
    COV_CU_DONE = COV_TB_END,  // + log2 - 3: CUs of 8, 16, 32 and 64 samples that reached cu_done
    COV_ALL = COV_CU_DONE + 4
};
#if defined(HG_HOST_EMU)
long g_cov[COV_ALL];
#define HG_COV(i) (++g_cov[i])
#else
#define HG_COV(i) ((void)0)
#endif

// bytes of n lane blocks, rounded up so the LanePic after them stays 16-byte aligned
HG_HD inline size_t lane_blocks_bytes(int n) { return (sizeof(LaneLds) * (size_t)n + 15) & ~(size_t)15; }

#if !defined(HG_HOST_EMU) && defined(HG_PARSE_PROF)
// (tuning builds) each parse translation unit's device globals are its code
// object's own, so each reads its own out through an entry of its own
// (heifgpu_debug_counters adds them up): this translation unit's counters
// (g_prof_lanes, g_ctu_t) copied out and zeroed
int prof_read(uint64_t *out, int n) {
    uint64_t tmp[16] = {};
    if (hipMemcpyFromSymbol(tmp, HIP_SYMBOL(hg::g_prof_lanes), sizeof(tmp)) != hipSuccess) return -1;
    const uint64_t zero[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(hg::g_prof_lanes), zero, sizeof(zero)) != hipSuccess) return -1;
#if defined(HG_PARSE_PROF_SB)
    const int head = 16;  // slots 16 on: g_ctu_t as in the prof build (the per-wave records)
#else
    const int head = 8;   // slots 8 on: the per-CTU times (3 per CTU) and the per-wave records
#endif
    for (int k = 0; k < n && k < head; ++k) out[k] = tmp[k];
    if (n <= head) return n < head ? n : head;
    const size_t m = std::min((size_t)(n - head), (size_t)hg::kCtuTimeCap * 3);
    if (hipMemcpyFromSymbol(out + head, HIP_SYMBOL(hg::g_ctu_t), m * sizeof(uint64_t)) != hipSuccess) return -1;
    std::vector<uint64_t> z((size_t)hg::kCtuTimeCap * 3, 0);
    if (hipMemcpyToSymbol(HIP_SYMBOL(hg::g_ctu_t), z.data(), z.size() * sizeof(uint64_t)) != hipSuccess) return -1;
    return (int)(head + m);
}
#endif

}  // namespace
}  // namespace hg
