// parse_solo.hip — the solo / spread parse kernels (k_parse_solo, one image's
// substreams on scalar engines, EngSoloT, over the syntax units of
// parse_units.hpp) and their launch, as a translation unit of their own, so
// that the lanes kernels and these get the code-generation flags each is
// fastest with (Makefile PARSE_SCHED / SOLO_SCHED; A/B in DESIGN 5.11).
// (the lanes units' cold-branch hints stay out of the scalar engines: their code is the one before the
// lean body, instruction for instruction)
#define HG_NO_COLD_HINTS 1
#include "parse_units.hpp"

namespace hg {

// the job counter: lane 0 takes the next number, the wave shares it
__device__ __forceinline__ uint32_t dequeue_job(uint32_t *ctr) {
    uint32_t j = 0;
    if (__lane_id() == 0) j = atomicAdd(ctr, 1u);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
}

// Solo mode: one workgroup per picture, one wave per WPP row (rows beyond 16
// wrap round the waves).  All 64 lanes of a wave run the same substream in
// lockstep (identical state in every lane, so exec stays full: the window and
// state-row registers read with v_readlane are never left stale in inactive
// lanes by a copy the compiler placed inside a divergent region), and the
// lanes differ only in the window refill, where each loads its own dword.  WPP
// progress words and the row-to-row context copies are in the workgroup's
// LDS, so the 2-CTU lag needs no memory traffic; waves waiting for the row
// above sleep.
inline size_t solo_lds_bytes(int nw, bool ring) {
    return lane_blocks_bytes(nw) + sizeof(LanePic) + 64 * sizeof(uint32_t) + 16 * sizeof(uint64_t) +
           (ring ? (size_t)nw * CTX_PAD : 0);
}

// (r06: a 6-waves-per-SIMD register budget, 80 VGPRs with 36 B/lane of
// scratch, lost 4 % at 16 and 32 images and 0.5 % at one: DESIGN 5.13)
template <bool Spread>
__global__ void __launch_bounds__(Spread ? 64 : 64 * kSoloMaxWaves) k_parse_solo(BatchArgs a) {
    using EG = EngSoloT<Spread>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NW = Spread ? 1 : a.solo_waves;
    LaneLds *s_lds = reinterpret_cast<LaneLds *>(smem);
    LanePic *s_pic = reinterpret_cast<LanePic *>(smem + lane_blocks_bytes(NW));
    uint32_t *s_prog = reinterpret_cast<uint32_t *>(s_pic + 1);
    uint64_t *s_seq = reinterpret_cast<uint64_t *>(s_prog + 64);
    uint8_t *s_wctx = a.wpp_ring ? reinterpret_cast<uint8_t *>(s_seq + 16) : nullptr;
    // wave index made scalar: every value of the substream state derives from uniform inputs, so the
    // compiler can keep the engine in SGPRs and branch with s_cbranch
    const int w = Spread ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
#if HG_PARSE_SETPRIO > 0
    // the substream chain wins issue arbitration against k_intra_stream's waves on its SIMD
    __builtin_amdgcn_s_setprio(HG_PARSE_SETPRIO);
#endif
    if (threadIdx.x < 15) s_seq[threadIdx.x] = sig_seq((int)threadIdx.x);
    if (threadIdx.x < 64) s_prog[threadIdx.x] = 0;
    const uint64_t trow = state_row(lane);
    const uint32_t tlo = (uint32_t)trow, thi = (uint32_t)(trow >> 32);
    const uint32_t scan8v = (uint32_t)kScanPos[3][0][lane] | ((uint32_t)kScanInv[3][0][lane] << 8);
    const uint64_t sq = lane < 15 ? sig_seq(lane) : 0;
    const uint32_t sqlo = (uint32_t)sq, sqhi = (uint32_t)(sq >> 32);
    // spread: the slot from the job counter (a row's predecessor is the slot
    // before it, so it is already held by a running wave whatever order the
    // workgroups are dispatched in); solo: the workgroup's own picture
    const int slot = Spread ? (int)dequeue_job(a.xjob) : (int)blockIdx.x;
    const int n_slots = a.parse_order ? a.n_slots : a.n_pics;
    const uint32_t ent = slot < n_slots ? (a.parse_order ? a.parse_order[slot] : (uint32_t)slot) : ~0u;
    const bool in = ent != ~0u;
    // spread: entry = row << 20 | picture, one wave per WPP row
    const int pic = a.pic0 + (int)(Spread ? (ent & 0xfffffu) : ent), row = Spread ? (int)(ent >> 20) : w;
    Lane L;
    LaneLds &ld = s_lds[w < NW ? w : 0];
    LanePic &P = s_pic[0];
    const bool live = in && w < NW && lane_init<false>(L, P, ld, a, pic, row, 0, Spread ? (1 << 20) : NW);  // every lane alike
    if (!live) L.st = U_DONE;
#if defined(HG_PARSE_PROF_SB)
    for (int k = 0; k < 6; ++k) L.psb[k] = 0;
#endif
    __syncthreads();
    if (!__builtin_amdgcn_readfirstlane(live ? 1 : 0)) return;
    const Env E = Spread ? Env{&a, s_lds, a.xprog + P.row_off, a.xctx + (size_t)P.row_off * CTX_PAD, row}
                         : Env{&a, s_lds, s_prog, s_wctx, w};
    const uint32_t lim = (P.bits_end + 64u) & ~3u;
    SoloWin sw;
    sw.r0 = sw.r1 = sw.f = 0;
    sw.ck = 0;
#if defined(HG_PARSE_PROF)
    uint64_t pf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t t_start = __builtin_amdgcn_s_memtime();
    int want_seen = -1;  // the CTU whose want time is recorded
#endif
#if defined(HG_PARSE_PROF_SB)
    uint64_t pw[2] = {0, 0};  // cycles of not-run iterations (WPP polls + sleeps); driver cycles of run ones
#endif
    uint32_t stalled = 0;  // consecutive not-run iterations (bounded: never hang the device)
    for (;;) {
#if defined(HG_PARSE_PROF_SB)
        const uint64_t t_top = __builtin_amdgcn_s_memtime();
#endif
        // the wave's state (equal in every lane), made scalar
        int st = L.st, run = st != U_DONE && (st != U_CTU || ctu_ready<EG>(L, P, E));
#if defined(HG_PARSE_PROF)
        const int tix = (P.row_off + L.row) * 128 + L.c;
        if (st == U_CTU && L.c < 128 && tix < kCtuTimeCap) {
            const uint64_t now = __builtin_amdgcn_s_memrealtime();  // chip-wide 100 MHz clock
            if (want_seen != tix && lane == 0) g_ctu_t[tix][0] = now;
            want_seen = tix;
            if (run && lane == 0) g_ctu_t[tix][1] = now;
        }
#endif
        uint32_t start = run && st == U_CTU ? substream_start<EG>(L, P, a) : ~0u;
        const uint32_t rd = L.lb;
        st = __builtin_amdgcn_readfirstlane(st);
        if (st == U_DONE) break;
        if (!__builtin_amdgcn_readfirstlane(run)) {
            // the row above is not 2 CTUs ahead: sleep (~64 cycles a unit), so the
            // busy waves on this SIMD keep the issue slots
            __builtin_amdgcn_s_sleep(HG_SOLO_SLEEP);
#if defined(HG_PARSE_PROF_SB)
            pw[0] += __builtin_amdgcn_s_memtime() - t_top;
#endif
            // a row waits at most one picture's parse (~1e6 iterations); far past
            // that the row above can never arrive (a dispatch-order assumption
            // broken): flag the picture and stop instead of spinning forever
            if (++stalled > (1u << 25)) {
                if (lane == 0) atomicOr(&a.status[P.pic], L.status | ST_SUBSTREAM_END);
                // publish the row as finished (the TU count as it stands), so the
                // rows below and k_intra_stream stop waiting on it at once
                if (Spread) {
                    if (a.xntu) store_agent(a.xntu + P.row_off + L.row, L.ntu);
                    stores_done();
                    store_agent(prog_word(E, P, L.row), kProgDone);
                }
                break;
            }
            continue;
        }
        stalled = 0;
        start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
        if (start != ~0u) sw.restart(a.rbsp, start, lim, lane);
        else sw.advance(a.rbsp, (uint32_t)__builtin_amdgcn_readfirstlane((int)rd), lim, lane);
        // the rows above (contexts, SAO parameters, depth line: other workgroups'
        // agent-scope stores) after their progress words, before their readers
        if (st == U_CTU) {
            if (Spread) HG_ACQ_AGENT();
            else HG_FENCE_ACQ();
        }
#if defined(HG_PARSE_PROF)
        const uint64_t t1 = __builtin_amdgcn_s_memtime();
        ++pf[7];
#endif
        {
            uni_state(L);
            const EG G{ld.ctx, tlo, thi, s_seq, a.rbsp, lim, sw.view(), sqlo, sqhi, scan8v};
#if defined(HG_PARSE_PROF)
            const int eix = (P.row_off + L.row) * 128 + L.c;
#endif
            run_unit(st, L, ld, P, E, G);
#if defined(HG_PARSE_PROF)
            if (st == U_CTU_END && eix < kCtuTimeCap && lane == 0) g_ctu_t[eix][2] = __builtin_amdgcn_s_memrealtime();
#endif
        }
#if defined(HG_PARSE_PROF)
#if defined(HG_PARSE_PROF_SB)
        pw[1] += t1 - t_top;
#else
        pf[st <= U_CTU ? 2 : st <= U_TT ? 3 : st - 1] += __builtin_amdgcn_s_memtime() - t1;
        ++pf[1];
#endif
#endif
    }
#if defined(HG_PARSE_PROF_SB)
    for (int k = 0; k < 6; ++k) pf[2 + k] = L.psb[k];
    pf[1] = pw[0];
    if (lane == 0) atomicAdd((unsigned long long *)&g_prof_lanes[8], (unsigned long long)pw[1]);
#endif
#if defined(HG_PARSE_PROF)
    pf[0] = __builtin_amdgcn_s_memtime() - t_start;
    if (lane == 0)
        for (int k = 0; k < 8; ++k) atomicAdd((unsigned long long *)&g_prof_lanes[k], (unsigned long long)pf[k]);
#endif
}

// the solo and spread modes (launch_parse)
hipError_t launch_parse_solo(const BatchArgs &a, hipStream_t s) {
    if (a.parse_mode == PARSE_SOLO) {
        if (a.solo_waves < 1 || a.solo_waves > kSoloMaxWaves) return hipErrorInvalidValue;
        const int n = a.parse_order ? a.n_slots : a.n_pics;
        if (n <= 0) return hipSuccess;
        hipLaunchKernelGGL(k_parse_solo<false>, dim3(n), dim3(64 * a.solo_waves),
                           solo_lds_bytes(a.solo_waves, a.wpp_ring != 0), s, a);
        return hipGetLastError();
    }
    if (!a.parse_order || !a.xprog || !a.xctx || !a.xjob) return hipErrorInvalidValue;
    if (a.n_slots <= 0) return hipSuccess;
    // (the progress words start at 0: k_rbsp of this decode cleared them)
    hipLaunchKernelGGL(k_parse_solo<true>, dim3(a.n_slots), dim3(64), solo_lds_bytes(1, false), s, a);
    return hipGetLastError();
}

}  // namespace hg

#if defined(HG_PARSE_PROF)
extern "C" int hg_debug_counters_solo(uint64_t *out, int n) { return hg::prof_read(out, n); }
#endif
