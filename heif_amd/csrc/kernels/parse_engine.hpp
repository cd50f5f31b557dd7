// parse_engine.hpp — the CABAC engines of the parse kernels, both families:
// vector (EngT: one substream per lane; k_parse_lanes, k_parse_lean) and scalar
// (EngSoloT: one substream per wave; k_parse_solo), with the tool-set
// accessors, the memory helpers, the RBSP queue and the arithmetic decoder
// (9.3.4.3) the syntax units of parse_units.hpp run on.
#pragma once
#include "parse_state.hpp"

namespace hg {
namespace {

// engine context of one lane (lanes mode: every lane its own substream; a
// picture's WPP rows are lanes of one wave, so no hand-off leaves the wave).
// (r05's row waves, k_parse_rows, were this engine with spread mode's
// hand-offs; removed in r06, their A/B record is DESIGN 5.4)
//
// Tool set (Lean): the general body keeps every coding tool of every chroma
// format at run time; the lean body is compiled for the set nearly every HEIC
// still uses (lanes_lean_eligible: 4:2:0, no PCM, transform_skip or
// cu_transquant_bypass, no slice segments inside a picture's rows or between
// them, no wrapping rows), with those picture constants and per-CU / per-TB
// flags folded (HG_PIC_CHROMA .. lane_fl below).  Sign hiding, cu_qp_delta, WPP,
// SAO and the bit depth stay run-time values in both.
template <bool Lean>
struct EngT {
    static constexpr bool kSolo = false;
    static constexpr bool kSpread = false;
    static constexpr bool kLean = Lean;
    static constexpr bool kCtxReg = false;  // contexts in LDS (ctx)
    static constexpr bool kRowCtx = true;
    uint8_t *ctx;
    const uint64_t *tab;  // engine_row of every context byte (LDS)
    const uint64_t *seq;  // sig_seq(scan, pattern): slot of every scan position of a sub-block (LDS)
    const uint8_t *rbsp;  // BatchArgs::rbsp (emulation prevention removed by k_rbsp)
    uint32_t lim;         // no loads at or past this offset (the picture's RBSP end + 64)
    // the 8x8 up-right diagonal scan of 32x32 TBs' sub-blocks and its inverse in
    // LDS (null: the constant tables).  A lane-varying index into constant memory
    // is a vector load, and its wait would drain the wave's record stores too
    const uint8_t *sp8 = nullptr, *inv8 = nullptr;
    HG_HD uint64_t row(uint32_t st) const { return tab[st]; }
    HG_HD uint64_t seqw(int idx) const { return seq[idx]; }
    HG_HD int scan8(int scan, int i) const { return sp8 && scan == 0 ? sp8[i] : kScanPos[3][scan][i]; }
    HG_HD int scan8_inv(int scan, int r) const { return inv8 && scan == 0 ? inv8[r] : kScanInv[3][scan][r]; }
};
using Eng = EngT<false>;
using EngLean = EngT<true>;

// Solo mode (k_parse_solo): one substream per WAVE, run by its lane 0 alone,
// so the engine state is wave-uniform.  The state rows live in two VGPRs
// across the lanes (lane s = pStateIdx s) and are read with v_readlane, and
// the RBSP comes from a 512-byte window in two VGPRs (dword d of the arena at
// lane d % 64 of register (d / 64) % 2), filled between units by whole-wave
// coalesced 256-byte loads through a staging VGPR: a chunk is loaded one
// chunk ahead of use and copied into the window (the copy is where the
// compiler waits for it) only when the reader enters the chunk before it, so
// a bin never waits on LDS for its state row and a refill almost never waits
// on memory.
#if defined(HG_HOST_EMU)
struct Win {
    const uint32_t *w;  // [2 * 64]
    uint32_t get(uint32_t d) const { return w[d & 127u]; }
};
#else
struct Win {
    uint32_t r0, r1;
    // both registers read and the result selected: a select of the register
    // (or of its address) becomes a dynamically indexed array in scratch
    __device__ __forceinline__ uint32_t get(uint32_t d) const {
        const int ln = __builtin_amdgcn_readfirstlane((int)(d & 63u));
        const uint32_t v0 = (uint32_t)__builtin_amdgcn_readlane((int)r0, ln);
        const uint32_t v1 = (uint32_t)__builtin_amdgcn_readlane((int)r1, ln);
        return (d & 64u) ? v1 : v0;
    }
};
#endif
template <bool Spread>
struct EngSoloT {
    static constexpr bool kSolo = true;
    static constexpr bool kLean = false;    // every tool at run time
    static constexpr bool kRowCtx = false;  // rows per pStateIdx (tlo / thi)
    // one wave per workgroup: the rows of a picture on different CUs, their
    // WPP progress, context hand-off, SAO and depth lines in coherent global
    // memory.  Rule: hand-off data goes out only through store_agent, so the
    // progress word needs vmcnt(0) only, not an L2 write-back (unit_ctu_end)
    static constexpr bool kSpread = Spread;
#if defined(HG_HOST_EMU)
    static constexpr bool kCtxReg = false;  // one lane per wave: contexts stay in the LDS block
#else
    static constexpr bool kCtxReg = true;   // contexts in Lane::cx
#endif
    uint8_t *ctx;
    uint32_t tlo, thi;    // lane s: state_row(s) (GPU); unused under emulation
    const uint64_t *seq;  // sig_seq(i), i < 15, in LDS (seqw)
    const uint8_t *rbsp;
    uint32_t lim;
    Win win;
    // lane i < 15: sig_seq(i).  Nothing reads them: seqw reads LDS (`seq`); the
    // v_readlane form over these two (removed) measured 26.7 against 25.7 ms
    // for one image (r05 same-box A/B, profiles/r05/ab/b1_engine_variants.txt);
    // the two builds differ mostly in where the register allocator put its
    // SGPR spills (89 here against 138).  The fields and their values in
    // k_parse_solo stay all the same: without them the register allocator
    // places the solo and spread kernels' SGPR spills differently again
    // (102,348 -> 99,212 B of code), and that is a change to measure
    uint32_t sqlo, sqhi;
    // lane i: kScanPos[3][0][i] | kScanInv[3][0][i] << 8 (a byte of constant memory
    // is a vector load even at a uniform index: v_readlane instead)
    uint32_t scan8v;
#if defined(HG_HOST_EMU)
    int scan8(int scan, int i) const { return kScanPos[3][scan][i]; }
    int scan8_inv(int scan, int r) const { return kScanInv[3][scan][r]; }
#else
    __device__ __forceinline__ int scan8(int scan, int i) const {
        if (scan != 0) return kScanPos[3][scan][i];
        return __builtin_amdgcn_readlane((int)scan8v, __builtin_amdgcn_readfirstlane(i)) & 0xff;
    }
    __device__ __forceinline__ int scan8_inv(int scan, int r) const {
        if (scan != 0) return kScanInv[3][scan][r];
        return (__builtin_amdgcn_readlane((int)scan8v, __builtin_amdgcn_readfirstlane(r)) >> 8) & 0xff;
    }
#endif
#if defined(HG_HOST_EMU)
    uint64_t row(uint32_t st) const { return state_row((int)st); }
    uint64_t seqw(int idx) const { return seq[idx]; }
#else
    __device__ __forceinline__ uint64_t seqw(int idx) const { return seq[idx]; }
    __device__ __forceinline__ uint64_t row(uint32_t st) const {
        const int s = __builtin_amdgcn_readfirstlane((int)st);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)tlo, s);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)thi, s);
        return (uint64_t)lo | ((uint64_t)hi << 32);
    }
#endif
};
using EngSolo = EngSoloT<false>;
using EngSpread = EngSoloT<true>;

#if !defined(HG_HOST_EMU)
// Solo mode: the wave's substream state is equal in every lane; say so to the
// compiler (v_readfirstlane), so the units keep it in SGPRs and branch on it
// with s_cbranch instead of exec masks.
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int uni32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return (uint64_t)uni32((uint32_t)v) | ((uint64_t)uni32((uint32_t)(v >> 32)) << 32);
}
[[maybe_unused]] __device__ __forceinline__ void uni_state(Lane &L) {
#define HG_U(f) L.f = uni32(L.f)
    // the engine and the tree / residual state the units branch on; the other
    // fields stay in VGPRs (all 64 lanes alike) and are read where used.  r05
    // A/B, one image, same box: 27.2 ms against 28.1 with every field scalar
    // (r04; that list left 134 SGPRs spilled into VGPR lanes, reloaded at
    // every unit) and 29.5 with the engine alone (profiles/r05/ab/b1_engine_select_uni.txt;
    // those lists, and the ones with the TB unit's fields added or the tree
    // positions left out, were compile-time variants: removed)
    HG_U(range); HG_U(value); HG_U(k); HG_U(cn); HG_U(lb); HG_U(budget); HG_U(st); HG_U(fl);
    HG_U(qx); HG_U(qy); HG_U(ql); HG_U(qd); HG_U(tx); HG_U(ty); HG_U(tl); HG_U(td); HG_U(tcbf);
    HG_U(ctbx); HG_U(ctby); HG_U(tb_log2); HG_U(tb_cidx); HG_U(rc_i); HG_U(rc_scan); HG_U(rc_last_sub);
    HG_U(rc_last_pos); HG_U(rc_prev_c1);
#undef HG_U
    L.cur = uni64(L.cur);
    L.rc_csbf = uni64(L.rc_csbf);
}
#endif

#if !defined(HG_SOLO_SLEEP)
#define HG_SOLO_SLEEP 1
#endif

// driver side of a solo wave's RBSP window: chunks (64 dwords, 256 bytes) c
// and c + 1 of the reader in the window, c + 2 staged (in flight)
struct SoloWin {
#if defined(HG_HOST_EMU)
    uint32_t *w, *f;  // [128], [64]
    void load(const uint8_t *rbsp, uint32_t chunk, uint32_t lim, int) {
        for (int l = 0; l < 64; ++l) {  // big-endian words (as the GPU window holds them)
            const uint32_t o = std::min((chunk * 64u + (uint32_t)l) * 4u, lim);
            f[l] = ((uint32_t)rbsp[o] << 24) | ((uint32_t)rbsp[o + 1] << 16) | ((uint32_t)rbsp[o + 2] << 8) |
                   (uint32_t)rbsp[o + 3];
        }
    }
    void commit(uint32_t chunk) {
        for (int l = 0; l < 64; ++l) w[(chunk & 1u) * 64u + (uint32_t)l] = f[l];
    }
    Win view() const { return Win{w}; }
#else
    uint32_t r0, r1, f;
    // every lane loads its dword of the chunk (one coalesced 256-byte load)
    __device__ __forceinline__ void load(const uint8_t *rbsp, uint32_t chunk, uint32_t lim, int lane) {
        const uint32_t o = (chunk * 64u + (uint32_t)lane) * 4u;
        f = *reinterpret_cast<const uint32_t *>(rbsp + (o < lim ? o : lim));
    }
    // the copy is the first use of the staged load: the compiler waits for it
    // here.  The window holds big-endian words (byte-swapped once per dword, by
    // the lanes in parallel), so the engine's bit refill is scalar shifts only
    __device__ __forceinline__ void commit(uint32_t chunk) {
        const bool odd = (chunk & 1u) != 0;  // both written: no address select
        const uint32_t be = __builtin_bswap32(f);
        r1 = odd ? be : r1;
        r0 = odd ? r0 : be;
    }
    __device__ __forceinline__ Win view() const { return Win{r0, r1}; }
#endif
    uint32_t ck;  // the staged chunk
    // a substream (re)starts at byte `start`
    HG_HD void restart(const uint8_t *rbsp, uint32_t start, uint32_t lim, int lane) {
        const uint32_t c0 = start >> 8;
        load(rbsp, c0, lim, lane);
        commit(c0);
        load(rbsp, c0 + 1, lim, lane);
        commit(c0 + 1);
        load(rbsp, c0 + 2, lim, lane);
        ck = c0 + 2;
    }
    // before a unit, the reader at dword rd: keep its chunk and the next in the window
    HG_HD void advance(const uint8_t *rbsp, uint32_t rd, uint32_t lim, int lane) {
        const uint32_t cc = rd >> 6;
        if (cc + 1 < ck) return;
        if (cc >= ck) {  // a unit ran past the window (corrupt stream): reload
            restart(rbsp, cc << 8, lim, lane);
            return;
        }
        commit(ck);
        load(rbsp, ck + 1, lim, lane);
        ++ck;
    }
};

// ------------------------------------------------------------------ tool set
// The picture constants and flags the units test, through the engine's tool
// set: run-time values of the picture (LDS reads, divergent branches) in the
// general bodies, constants in the lean one.  PF_COHERENT is the streaming
// spread parse's alone (BatchArgs::xntu): neither lanes body tests it.
constexpr uint32_t kLeanOffFlags = SP_TRANSFORM_SKIP | SP_TQ_BYPASS | SP_PCM | SP_PCM_LOOP_FILTER_DISABLED |
                                   SP_ROW_SEGMENTS | ((uint32_t)PD_NMID_MAX << PD_NMID_SHIFT);
// (the chroma format's three as in-place constant selections, not functions:
// written as accessor functions, or read once into a local, they moved the
// code generation of the solo / spread kernels, which this tool set leaves
// alone: the spread kernel 52,940 -> 48,952 B and one image 24.8 -> 25.8 ms,
// DESIGN 5.15; so every read stands where the general body had it)
#define HG_PIC_CHROMA(P) (EG::kLean ? 1 : (P).chroma)
#define HG_PIC_SUBX(P) (EG::kLean ? 1 : (P).subx)
#define HG_PIC_SUBY(P) (EG::kLean ? 1 : (P).suby)
template <class EG>
HG_HD inline uint32_t pic_flags(const LanePic &P) {
    uint32_t f = P.flags;
    if constexpr (!EG::kSolo) f &= ~PF_COHERENT;
    if constexpr (EG::kLean) f &= ~kLeanOffFlags;
    return f;
}
// rows wrap round the picture's lanes (WPP context staging)
template <class EG>
HG_HD inline bool pic_ring(const LanePic &P) {
    if constexpr (EG::kLean) return false;
    else return P.ring != 0;
}
// Lane.fl as the units test it: cu_transquant_bypass, transform_skip and PCM never set in the lean body
template <class EG>
HG_HD inline uint32_t lane_fl(const Lane &L) {
    if constexpr (EG::kLean) return L.fl & ~(uint32_t)(F_BYPASS | F_TS | F_PCM);
    else return L.fl;
}

// ------------------------------------------------------------------ memory helpers
#if defined(HG_HOST_EMU)
inline uint32_t prog_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline void prog_store(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
inline uint32_t load_word_coherent(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline void release_fence() { std::atomic_thread_fence(std::memory_order_release); }
inline void store_tu(TuRec *d, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    uint32_t *p = reinterpret_cast<uint32_t *>(d);
    p[0] = x;
    p[1] = y;
    p[2] = z;
    p[3] = w;
}
inline void store_tu_agent(TuRec *d, uint32_t x, uint32_t y, uint32_t z, uint32_t w) { store_tu(d, x, y, z, w); }
inline void store_word_agent(uint32_t *p, uint32_t v) { *p = v; }
#else
__device__ __forceinline__ uint32_t prog_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void prog_store(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// 4-byte load that bypasses the L1: the word was written by another lane of
// this wave (same CU, so the L2 of this XCD has it)
__device__ __forceinline__ uint32_t load_word_coherent(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// drain this wave's global stores (SAO parameters, depth line) before the
// progress word that lets the lane below read them
__device__ __forceinline__ void release_fence() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }
__device__ __forceinline__ void store_tu(TuRec *d, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    *reinterpret_cast<uint4 *>(d) = make_uint4(x, y, z, w);
}
// the same as agent-scope (sc1) stores: coherent across the XCDs' L2s once
// complete, so the spread parse publishes them with a wait, not an L2 write-back
__device__ __forceinline__ void store_tu_agent(TuRec *d, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    uint64_t *q = reinterpret_cast<uint64_t *>(d);
    __hip_atomic_store(q, (uint64_t)x | ((uint64_t)y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, (uint64_t)z | ((uint64_t)w << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_word_agent(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

// n bytes of v at p (v's 8-byte pattern repeats for n > 8: a 64x64 CU's
// 16-byte QpY row): one store when n is 2, 4 or 8 and p is n-aligned
HG_HD inline void store_bytes(uint8_t *p, int n, uint64_t v) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (n == 8 && !(a & 7)) {
        *reinterpret_cast<uint64_t *>(p) = v;
    } else if (n == 4 && !(a & 3)) {
        *reinterpret_cast<uint32_t *>(p) = (uint32_t)v;
    } else if (n == 2 && !(a & 1)) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    } else {
        for (int i = 0; i < n; ++i) p[i] = (uint8_t)(v >> (8 * (i & 7)));
    }
}

// Spread mode: words another CU reads (agent-scope atomics: sc1 accesses,
// coherent across the XCDs' L2s without whole-cache write-backs), and the
// wait that makes this wave's earlier such stores visible before a progress word
#if defined(HG_HOST_EMU)
template <class T>
inline void store_agent(T *p, T v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
inline uint32_t load_agent(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline void stores_done() { std::atomic_thread_fence(std::memory_order_release); }
#else
template <class T>
__device__ __forceinline__ void store_agent(T *p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t load_agent(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// s_waitcnt vmcnt(0): every store of this wave has completed
__device__ __forceinline__ void stores_done() { __builtin_amdgcn_s_waitcnt(0x0f70); }
#endif

HG_HD inline uint8_t load_byte_coherent(const uint8_t *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t w = load_word_coherent(reinterpret_cast<const uint32_t *>(a & ~uintptr_t(3)));
    return (uint8_t)(w >> ((a & 3) * 8));
}

// ------------------------------------------------------------------ bytes
// Each lane reads its substream straight from the RBSP arena, which k_rbsp
// (rbsp.hip) filled with emulation prevention removed (rbsp_reader.rs:11-39).
// The bit window refills from a per-lane queue of up to 8 dwords in registers;
// 16 more bytes are loaded at each pass start and used from the next pass on,
// after the pass's single s_waitcnt, so no refill inside a pass waits on
// memory (a wait for a load also drains every older store of the wave: with a
// one-dword prefetch it cost ~5 % of the parse).  Loads stop 64 bytes past
// the picture's end (arena padding); an overrun of a corrupt stream shows as
// budget + k < 0 at the CTU end (ST_OVERRUN).
// 16 bytes at `off` (dword aligned), clamped to `lim` (inside the arena's padding)
#if defined(HG_HOST_EMU)
inline void load_x4(const uint8_t *p, uint32_t off, uint32_t lim, uint32_t &x, uint32_t &y, uint32_t &z, uint32_t &w) {
    uint32_t v[4];
    for (int i = 0; i < 4; ++i) {
        const uint32_t o = std::min(off + 4u * (uint32_t)i, lim);
        v[i] = (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16) | ((uint32_t)p[o + 3] << 24);
    }
    x = v[0], y = v[1], z = v[2], w = v[3];
}
// the pass start's one memory wait (host emulation: nothing in flight)
inline void pass_wait() {}
#else
__device__ __forceinline__ void load_x4(const uint8_t *p, uint32_t off, uint32_t lim, uint32_t &x, uint32_t &y,
                                        uint32_t &z, uint32_t &w) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p + (off < lim ? off : lim));
    x = v.x, y = v.y, z = v.z, w = v.w;
}
// s_waitcnt vmcnt(0) expcnt(7) lgkmcnt(15): every global access of this wave so far
__device__ __forceinline__ void pass_wait() { __builtin_amdgcn_s_waitcnt(0x0f70); }
#endif
HG_HD inline uint32_t bswap32(uint32_t w) {
    return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24);
}

// next RBSP dword of the queue.  Normally a or b; a lane that drained both
// inside one pass takes f (waiting for it) or loads synchronously.  Solo
// mode: dword L.lb of the register window (filled between units), already
// big-endian (be_pop).
template <class EG>
HG_HD inline uint32_t q_pop(Lane &L, const EG &G) {
    if constexpr (EG::kSolo) return G.win.get(L.lb++);
#if !defined(HG_HOST_EMU) && defined(__HIP_DEVICE_COMPILE__)
    // the dword at index ai as three v_cndmask.  Written in C++ the selection
    // compiles to nested exec-mask branches (a dozen SALU instructions at every
    // refill site), and as bit tests into a dynamically indexed scratch array;
    // r05 A/B at 128 images: 19,490 against 19,200 (branches) and 17,520
    // (scratch) Mpix/s; 17 % fewer static instructions in k_parse_lanes
    uint32_t w;
    asm("v_cmp_eq_u32 vcc, 1, %1\n\t"
        "v_cndmask_b32 %0, %2, %3, vcc\n\t"
        "v_cmp_eq_u32 vcc, 2, %1\n\t"
        "v_cndmask_b32 %0, %0, %4, vcc\n\t"
        "v_cmp_eq_u32 vcc, 3, %1\n\t"
        "v_cndmask_b32 %0, %0, %5, vcc"
        : "=&v"(w)
        : "v"(L.ai), "v"(L.a0), "v"(L.a1), "v"(L.a2), "v"(L.a3)
        : "vcc");
#else
    const uint32_t w = L.ai == 0 ? L.a0 : (L.ai == 1 ? L.a1 : (L.ai == 2 ? L.a2 : L.a3));
#endif
    if (++L.ai == 4) {
        L.ai = 0;
        if (L.bv) {
            L.a0 = L.b0, L.a1 = L.b1, L.a2 = L.b2, L.a3 = L.b3;
            L.bv = 0;
        } else if (L.fp) {
            L.a0 = L.f0, L.a1 = L.f1, L.a2 = L.f2, L.a3 = L.f3;
            L.fp = 0;
        } else {
            load_x4(G.rbsp, L.lb, G.lim, L.a0, L.a1, L.a2, L.a3);
            L.lb += 16;
        }
    }
    return w;
}

// the next 32 bits of the substream, MSB first
template <class EG>
HG_HD inline uint32_t be_pop(Lane &L, const EG &G) {
    if constexpr (EG::kSolo) return q_pop(L, G);
    return bswap32(q_pop(L, G));
}

// pass start (after pass_wait): land f, issue the next block
template <class EG>
HG_HD inline void q_refill(Lane &L, const EG &G) {
    if (L.fp && !L.bv) {
        L.b0 = L.f0, L.b1 = L.f1, L.b2 = L.f2, L.b3 = L.f3;
        L.bv = 1;
        L.fp = 0;
    }
    if (!L.fp && L.lb) {
        load_x4(G.rbsp, L.lb, G.lim, L.f0, L.f1, L.f2, L.f3);
        L.lb += 16;
        L.fp = 1;
    }
    // top the bit window up to more than 32 bits once per pass, so that inside
    // the pass vfill's pop (the queue select and its reload branches, run by
    // the whole wave whenever one lane needs it) is rarely reached
    if (L.cn <= 32) {
        L.cur |= (uint64_t)be_pop(L, G) << (32 - L.cn);
        L.cn += 32;
    }
}

// value += 16 more look-ahead bits (k < 8 on entry, so k <= 23 and value < 2^32 after).
// (A/B r03: comparisons as sign masks with k <= 22 and v_bfi selects instead
// of compares into VCC: parse 94 vs 91 ms at 128 images, 37.9 vs 36.1 ms for
// one image in spread mode — the compares stay.)
template <class EG>
HG_HD inline void vfill(Lane &L, const EG &G) {
    if (L.cn < 16) {
        L.cur |= (uint64_t)be_pop(L, G) << (32 - L.cn);
        L.cn += 32;
    }
#if !defined(HG_HOST_EMU) && defined(__HIP_DEVICE_COMPILE__)
    if constexpr (EG::kSolo) {
        // scalar: the compiler turns this into a funnel shift, which only the VALU has
        const uint32_t top = (uint32_t)(L.cur >> 48);
        uint32_t nv;
        asm("s_lshl_b32 %0, %1, 16\n\ts_or_b32 %0, %0, %2" : "=&s"(nv) : "s"(uni32(L.value)), "s"(uni32(top)) : "scc");
        L.value = nv;
    } else
#endif
    {
        L.value = (L.value << 16) | (uint32_t)(L.cur >> 48);
    }
    L.cur <<= 16;
    L.cn -= 16;
    L.k += 16;
    L.budget -= 16;
}

// 9.3.2.5: engine initialisation at RBSP offset `start` (absolute), picture RBSP end `end`
// (solo mode: the driver has filled the window from `start` on)
template <class EG>
HG_HD inline void engine_init(Lane &L, const EG &G, uint32_t start, uint32_t end) {
    const uint32_t a0 = start & ~3u, sh = (start & 3u) * 8u;
    if constexpr (EG::kSolo) {
        L.lb = a0 >> 2;
    } else {
        load_x4(G.rbsp, a0, G.lim, L.a0, L.a1, L.a2, L.a3);
        load_x4(G.rbsp, a0 + 16, G.lim, L.b0, L.b1, L.b2, L.b3);
        L.ai = 0;
        L.bv = 1;
        L.fp = 0;
        L.lb = a0 + 32;
    }
    L.cur = (uint64_t)be_pop(L, G) << (32 + sh);
    L.cn = 32 - (int)sh;
    L.budget = 8 * (int32_t)(end - start);
    L.value = 0;
    L.k = -9;  // the first 9 bits are ivlOffset itself
    vfill(L, G);
    vfill(L, G);
    L.range = 510;
    if ((L.value >> L.k) >= 510) {
        // ivlOffset 510 / 511 (9.3.2.5 forbids it): flagged, and clamped so that
        // value < range << k holds and every later bin stays in range (a bypass
        // run of n bins < 2^n, so no syntax element leaves its domain)
        L.status |= ST_CABAC_INIT;
        L.value = (509u << L.k) | ((1u << L.k) - 1u);
    }
}

// ------------------------------------------------------------------ engine (9.3.4.3)
// DecodeDecision (arithmetic.rs:97-144), branch-free: one row per pStateIdx
// gives rangeTabLps and both transitions; the renormalisation of either path
// is a shift by clz and lowers k.
// (a & m) | (b & ~m) as one v_bfi_b32: written as C the compiler re-masks the
// inserted value first (a bit-field extract of the row, then the OR)
HG_HD inline uint32_t bfi32(uint32_t m, uint32_t a, uint32_t b) {
#if !defined(HG_HOST_EMU) && defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
#else
    return (a & m) | (b & ~m);
#endif
}

// (vector engines, state_row_ctx) a decision on context byte s; t receives
// the new byte in bits 0-6 and the bin in bit 7, bits above are not cleared
template <class EG>
HG_HD inline int dec_t(Lane &L, const EG &G, uint32_t s, uint32_t &t) {
    const uint64_t row = G.row(s);
    const uint32_t lps = ((uint32_t)row >> ((L.range >> 3) & 24u)) & 0xffu;
    const uint32_t rm = L.range - lps;
    const uint32_t sr = rm << L.k;
    const bool isl = L.value >= sr;
    L.value -= isl ? sr : 0u;
    const uint32_t rn = isl ? lps : rm;
    const int nb = __builtin_clz(rn) - 23;
    L.range = rn << nb;
    L.k -= nb;
    t = (uint32_t)(row >> (isl ? 32 : 40));
    if (L.k < 8) vfill(L, G);
    return (int)((t >> 7) & 1u);
}

template <class EG>
HG_HD inline int dec_s(Lane &L, const EG &G, uint32_t &s) {
    if constexpr (EG::kRowCtx) {
        uint32_t t;
        const int bin = dec_t(L, G, s, t);
        s = t & 0x7fu;
        return bin;
    }
    const uint32_t st = s >> 1, mps = s & 1u;
    const uint64_t row = G.row(st);
    const uint32_t hi = (uint32_t)(row >> 32);  // next byte after an LPS | after an MPS << 8
    const uint32_t lps = ((uint32_t)row >> ((L.range >> 3) & 24u)) & 0xffu;
    const uint32_t rm = L.range - lps;
    const uint32_t sr = rm << L.k;
#if !defined(HG_HOST_EMU) && defined(__HIP_DEVICE_COMPILE__)
    if constexpr (EG::kSolo) {
        // scalar engine: the LPS test as an integer straight from SCC (as a
        // boolean the compiler carries a lane mask and rebuilds the bin
        // through a VALU select and v_readfirstlane), then mask arithmetic.
        // (uni32: the lanes are identical, but where the compiler cannot
        // prove it, e.g. at engine start, the operands must be made scalar)
        // one compare, every choice an s_cselect on its SCC: the bin, the new
        // range, what leaves the offset and the shift that picks the next state
        uint32_t lp, rn, d, sh;
        asm("s_cmp_ge_u32 %4, %5\n\t"
            "s_cselect_b32 %0, 1, 0\n\t"
            "s_cselect_b32 %1, %6, %7\n\t"
            "s_cselect_b32 %2, %5, 0\n\t"
            "s_cselect_b32 %3, 0, 8"
            : "=&s"(lp), "=&s"(rn), "=&s"(d), "=&s"(sh)
            : "s"(uni32(L.value)), "s"(uni32(sr)), "s"(uni32(lps)), "s"(uni32(rm))
            : "scc");
        s = ((hi >> sh) & 0xffu) ^ mps;
        L.value -= d;
        const int nb = __builtin_clz(rn) - 23;
        L.range = rn << nb;
        L.k -= nb;
        if (L.k < 8) vfill(L, G);
        return (int)(mps ^ lp);
    }
#endif
    const bool isl = L.value >= sr;
    L.value -= isl ? sr : 0u;
    const uint32_t rn = isl ? lps : rm;
    const int nb = __builtin_clz(rn) - 23;
    L.range = rn << nb;
    L.k -= nb;
    s = ((hi >> (isl ? 0 : 8)) & 0xffu) ^ mps;
    if (L.k < 8) vfill(L, G);
    return (int)(mps ^ (isl ? 1u : 0u));
}

// context state ci: a byte of the LDS block, or (solo on the GPU) of Lane::cx
template <class EG>
HG_HD inline uint32_t ctx_ld(const Lane &L, const EG &G, int ci) {
#if !defined(HG_HOST_EMU)
    if constexpr (EG::kCtxReg) {
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)L.cx, ci >> 2);
        return (w >> ((ci & 3) * 8)) & 0xffu;
    }
#endif
    return G.ctx[ci];
}
template <class EG>
HG_HD inline void ctx_st(Lane &L, const EG &G, int ci, uint32_t v) {
#if !defined(HG_HOST_EMU)
    if constexpr (EG::kCtxReg) {
        const int sh = (ci & 3) * 8;
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)L.cx, ci >> 2);
        L.cx = (uint32_t)hg_writelane((int)((w & ~(0xffu << sh)) | (v << sh)), ci >> 2, (int)L.cx);
        return;
    }
#endif
    G.ctx[ci] = (uint8_t)v;
}

// the same on context ci
template <class EG>
HG_HD inline int dec(Lane &L, const EG &G, int ci) {
#if !defined(HG_HOST_EMU)
    if constexpr (EG::kCtxReg) {  // one v_readlane serves the read and the write back
        const int sh = (ci & 3) * 8;
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)L.cx, ci >> 2);
        uint32_t s = (w >> sh) & 0xffu;
        const int bin = dec_s(L, G, s);
        L.cx = (uint32_t)hg_writelane((int)((w & ~(0xffu << sh)) | (s << sh)), ci >> 2, (int)L.cx);
        return bin;
    }
#endif
    uint32_t s = G.ctx[ci];
    const int bin = dec_s(L, G, s);
    G.ctx[ci] = (uint8_t)s;
    return bin;
}

// byte `slot` (0..11) of a 3-word register cache of context states
HG_HD inline uint32_t cache_get(uint32_t c0, uint32_t c1, uint32_t c2, int slot) {
    const uint32_t w = slot < 4 ? c0 : (slot < 8 ? c1 : c2);
    return (w >> ((slot & 3) * 8)) & 0xffu;
}
HG_HD inline void cache_put(uint32_t &c0, uint32_t &c1, uint32_t &c2, int slot, uint32_t s) {
    const int sh = (slot & 3) * 8;
    const uint32_t w = slot < 4 ? c0 : (slot < 8 ? c1 : c2);
    const uint32_t nw = (w & ~(0xffu << sh)) | (s << sh);
    c0 = slot < 4 ? nw : c0;
    c1 = (slot >> 2) == 1 ? nw : c1;
    c2 = slot >= 8 ? nw : c2;
}

// DecodeBypass (arithmetic.rs:146-157)
template <class EG>
HG_HD inline int byp(Lane &L, const EG &G) {
    L.k -= 1;
    const uint32_t sr = L.range << L.k;
    const bool one = L.value >= sr;
    L.value -= one ? sr : 0u;
    if (L.k < 8) vfill(L, G);
    return one ? 1 : 0;
}

// floor(top / r) for top < 2^24 and 256 <= r <= 510: f32 reciprocal estimate, then one correction
HG_HD inline uint32_t div_range(uint32_t top, uint32_t r) {
#if defined(HG_HOST_EMU)
    return top / r;
#else
    const uint32_t q = (uint32_t)((float)top * __builtin_amdgcn_rcpf((float)r));
    const int32_t rem = (int32_t)top - (int32_t)(q * r);
    // the correction as sign bits (|rem| < 2r): compares and selects here become
    // a lane-mask boolean that the scalar engine rebuilds through the VALU
    return q + ((uint32_t)((int32_t)r - 1 - rem) >> 31) - ((uint32_t)rem >> 31);
#endif
}

// n (0..8) bypass bins in one step.  n successive DecodeBypass steps are the
// long division of ivlOffset * 2^n + (the next n bits) by ivlCurrRange: the
// quotient is the n bins, the remainder the new ivlOffset.
template <class EG>
HG_HD inline uint32_t byp_n(Lane &L, const EG &G, int n) {
    L.k -= n;  // k >= 8 >= n on entry
    const uint32_t q = div_range(L.value >> L.k, L.range);
    L.value -= (q * L.range) << L.k;
    if (L.k < 8) vfill(L, G);
    return q;
}

template <class EG>
HG_HD inline uint32_t byp_bits(Lane &L, const EG &G, int n) {
    uint32_t v = 0;
    while (n > 0) {
        const int c = n < 8 ? n : 8;
        v = (v << c) | byp_n(L, G, c);
        n -= c;
    }
    return v;
}

// coeff_abs_level_remaining's non-escape part (decoder.rs:230-261: prefix
// TR(cMax 4 << k, k), i.e. up to 4 one-bins, a 0, then k suffix bins) in ONE
// division: the next 8 bins are divided out without consuming them, the
// prefix p is their leading ones (at most 4), and when p < 4 the whole code
// (p + 1 + k <= 8 bins) is a prefix of those 8, consumed at once (a prefix of
// a long-division quotient is the quotient of the shorter division).  Returns
// the value, or -1 after consuming the 4 ones of an escape.
template <class EG>
HG_HD inline int byp_rem(Lane &L, const EG &G, int k) {
    const uint32_t q8 = div_range(L.value >> (L.k - 8), L.range);  // k >= 8 on entry
    const int p = __builtin_clz(((~q8) << 24) | (1u << 27));        // leading ones, at most 4
    const int used = p < 4 ? p + 1 + k : 4;
    const uint32_t q = q8 >> (8 - used);
    L.k -= used;
    L.value -= (q * L.range) << L.k;
    if (L.k < 8) vfill(L, G);
    return p < 4 ? (p << k) + (int)(q & ((1u << k) - 1u)) : -1;
}

// a unary bypass prefix of at most m (1..8) bins: the number p of 1-bins
// before the first 0, consuming min(p + 1, m) bins
template <class EG>
HG_HD inline int byp_unary(Lane &L, const EG &G, int m) {
    const uint32_t q = div_range(L.value >> (L.k - m), L.range);
    const int p = __builtin_clz(((~q) << (32 - m)) | (1u << (31 - m)));
    const int used = p < m ? p + 1 : m;
    L.k -= used;
    L.value -= ((q >> (m - used)) * L.range) << L.k;
    if (L.k < 8) vfill(L, G);
    return p;
}

// (vector engines) one PB's mode bins in ONE division, without a branch on
// prev_intra_luma_pred_flag: the next 5 bypass bins are divided out unconsumed;
// rem_intra_luma_pred_mode is all five, mpm_idx (TR, cMax 2: 0, 10, 11) the
// first one or two (a prefix of a long-division quotient is the quotient of
// the shorter division, as in byp_rem).  Returns mpm_idx or the remainder.
template <class EG>
HG_HD inline int byp_luma_mode(Lane &L, const EG &G, int prev) {
    const uint32_t q5 = div_range(L.value >> (L.k - 5), L.range);  // k >= 8 on entry
    const int used = prev ? 1 + (int)(q5 >> 4) : 5;
    const uint32_t q = q5 >> (5 - used);
    L.k -= used;
    L.value -= (q * L.range) << L.k;
    if (L.k < 8) vfill(L, G);
    return (int)(prev ? q - (q >> 1) : q);  // mpm_idx: bins 0 -> 0, 10 -> 1, 11 -> 2
}

// DecodeTerminate (arithmetic.rs:159-169)
template <class EG>
HG_HD inline int term(Lane &L, const EG &G) {
    L.range -= 2;
    const uint32_t sr = L.range << L.k;
    if (L.value >= sr) {
        // 1 ends the engine's run (end of a segment / subset, pcm_flag: a new
        // initialisation follows).  A corrupt stream may read on: keep
        // value < range << k, so later bins stay in their domains
        L.value = sr - 1u;
        return 1;
    }
    if (L.range < 256) {
        L.range <<= 1;
        L.k -= 1;
        if (L.k < 8) vfill(L, G);
    }
    return 0;
}

}  // namespace
}  // namespace hg
