// intra.hip — intra sample prediction + reconstruction (pipeline stage 3).
//
// H.265 8.4.4.2.1-8.4.4.2.6 (neighbour availability via z-scan order 6.4.1,
// substitution, [1 2 1] / strong smoothing, planar, DC with edge filter,
// 33 angular modes with the mode-10/26 boundary filters) and 8.6.7
// (recSamples = Clip1(pred + res)).  The reference stops before any of this
// (src/hevc/slice.rs:253-255).
//
// Mapping: the serial part of HEVC intra decoding is the TB-to-TB
// dependency inside a CTU row.  One workgroup per picture, one wave per CTB
// row; row r starts CTU c once row r-1 has finished CTU c+1 (every
// above-right neighbour lies in CTU c+1 at most), signalled through per-wave
// progress counters in LDS with workgroup-scope release/acquire.
//
// Each wave reconstructs its current CTU in an LDS window: the CTU's samples,
// the column left of it (kept from the previous CTU), the row above it
// (2*ctb+1 samples incl. the corner and above-right, loaded once per CTU from
// the picture after the progress wait) and the CTU's residuals (one coalesced
// load per CTU).  Every TB then works on LDS only — neighbour gather with
// the substitution (each lane reads the sample that stands at its search
// position after 8.4.4.2.2, a closed form on the record's five availability
// facts: intra_rec.hpp word D), filtering, prediction and residual add run
// one sample per lane — and the finished CTU is written to the picture once.
#include "kernels.hpp"
#include "intra_rec.hpp"
#include "xform.hpp"
#if defined(HG_HOST_EMU)
#include <cstdio>
#include <cstdlib>
#endif

namespace hg {

namespace {

constexpr int kMaxWaves = 16;
constexpr int kResidentIntraWaves = 4096;  // ~16 per CU: enough pictures in flight to hide TB latency
constexpr size_t kIntraLdsBudget = 128 * 1024;

__constant__ int8_t c_angle[35] = {0, 0, 32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26,
                                   -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32};
__constant__ int16_t c_inv_angle[35] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -4096, -1638, -910, -630, -482, -390, -315,
                                        -256, -315, -390, -482, -630, -910, -1638, -4096, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct alignas(16) IntraScratch {
    // TBs are at most 32x32 (MaxTbLog2SizeY <= 5): 2n + 1 <= 65 reference samples
    // per side.  Sized to that, not to the CTB, so more workgroups fit beside the
    // next decode's k_parse_lanes (which holds ~120 KB of each CU's LDS).
    int16_t left[66];  // [0] = p[-1][-1], [1+y] = p[-1][y]
    int16_t top[66];   // [0] = p[-1][-1], [1+x] = p[x][-1]
    int16_t fl[66];
    int16_t ft[66];
};

// Per-wave LDS block: scratch, then per component the CTU window.
struct WinLayout {
    int csx[3], csy[3];                          // component CTB width, height
    uint32_t cur[3], left[3], above[3], res[3];  // byte offsets in the block
    uint32_t bytes;                              // block size (16-aligned)
};

#if defined(HG_HOST_EMU)
inline
#else
__host__ __device__ inline
#endif
WinLayout win_layout(int log2ctb, int chroma, int bps) {
    WinLayout L{};
    uint32_t o = (uint32_t)((sizeof(IntraScratch) + 15) & ~size_t(15));
    const int ncomp = chroma ? 3 : 1;
    for (int k = 0; k < 3; ++k) {
        const int cx = k == 0 ? (1 << log2ctb) : (chroma ? (1 << log2ctb) >> chroma_sx(chroma) : 0);
        const int cy = k == 0 ? (1 << log2ctb) : (chroma ? (1 << log2ctb) >> chroma_sy(chroma) : 0);
        L.csx[k] = cx;
        L.csy[k] = cy;
        if (k >= ncomp) continue;
        L.cur[k] = o;
        o += (uint32_t)(cx * cy * bps + 15) & ~15u;
        L.left[k] = o;
        o += (uint32_t)(cy * bps + 15) & ~15u;
        L.above[k] = o;
        o += (uint32_t)((2 * cx + 1) * bps + 15) & ~15u;
        // residuals are read from the k_transform planes, not staged here: half
        // the block, so twice the workgroups fit beside the next decode's k_parse
        L.res[k] = 0;
    }
    L.bytes = o;
    return L;
}

int intra_waves(int log2ctb, int chroma, int bps, int max_rows) {
    const WinLayout L = win_layout(log2ctb, chroma, bps);
    int nw = (int)((kIntraLdsBudget - 64) / L.bytes);
    nw = nw < kMaxWaves ? nw : kMaxWaves;
    nw = nw < max_rows ? nw : max_rows;
    return nw < 1 ? 1 : nw;
}

#define wave_sync() HG_WAVE_SYNC()
// k_intra_stream's wait for the parse (tuning: HG_STREAM_SLEEP_N, s_sleep units of 64 clocks)
#if defined(HG_HOST_EMU) || !defined(HG_STREAM_SLEEP_N)
#define HG_STREAM_SLEEP() HG_SLEEP()
#else
#define HG_STREAM_SLEEP() __builtin_amdgcn_s_sleep(HG_STREAM_SLEEP_N)
#endif


// 6.4.1 availability of a TB's neighbours is decided where the wave loads the
// records (tb_pack_d, intra_rec.hpp): everything in the CTU row above (up to the
// above-right CTU, which the wavefront has finished) and in the CTU to the left
// is decoded; the CTUs below-left and right are not; inside the CTU a block is
// available iff it precedes the TB in z-scan order (MinTbAddrZs of 6.5.2 at 4x4
// granularity).  Per group of neighbours that is one fact, not one per sample.

// ref[k] of 8.4.4.2.6 read in place: the main-side neighbour for k >= 0, the
// projected side-side neighbour for k < 0 (only reached when
// (nTbS * intraPredAngle) >> 5 < -1, exactly where the spec extends ref)
// (r06 A/B: as an element index from one base, an integer select before one
// load: VALU +0.18 G with the two rows below, the step -0.3 %; not taken)
__device__ __forceinline__ const int16_t *ang_ref(const int16_t *main_, const int16_t *side, int inv, int k) {
    return k >= 0 ? main_ + k : side + ((k * inv + 128) >> 8);
}

// four samples as one store unit
template <typename Pel>
struct QuadT;
template <>
struct QuadT<uint8_t> {
    using type = uint32_t;
};
template <>
struct QuadT<uint16_t> {
    using type = uint64_t;
};
template <typename Pel>
using Quad = typename QuadT<Pel>::type;

// One component's CTU window in LDS and its place in the picture (the CTU
// write-back and the load of the row above; a TB works on a TbWin)
template <typename Pel>
struct Win {
    Pel *cur, *left, *above;
    int csx, csy;  // CTB width, height in component samples (4:2:2 chroma: csy = 2 csx)
    int cx0, cy0;  // CTB origin in component samples
};

// What a TB's prediction reads of its component's window: the CTB's samples
// (the TB's own position in them is in the record's word D), where the column
// left of the CTB and the row above it stand behind them, and the TB's residual.
template <typename Pel>
struct TbWin {
    Pel *cur;
    int dl, da;          // the left column and the row above, in samples from cur
    int lsx;             // log2 of the window's pitch (the component CTB's width)
    const int16_t *rt;   // the TB's first residual: in the component's residual plane (k_transform), or in
                         // streaming mode the TB's residual tile in LDS
    int rp;              // residual pitch (the plane width; streaming mode: the TB width)
#if defined(HG_HOST_EMU)
    // emulation only: the LDS objects the pointers must stay inside (the r04
    // gain-map fault was a residual pointer moved before its LDS buffer, which
    // the host build could not see): the wave's window block, and the residual's
    // object when it is an LDS tile (null: a residual plane in global memory)
    const unsigned char *blk_lo = nullptr, *blk_hi = nullptr;
    const int16_t *res_lo = nullptr, *res_hi = nullptr;
    void check_blk(const void *p, size_t bytes) const {
        const unsigned char *q = static_cast<const unsigned char *>(p);
        if (blk_lo && (q < blk_lo || q + bytes > blk_hi)) {
            fprintf(stderr, "k_intra: window access %td bytes outside the wave's LDS block\n",
                    q < blk_lo ? q - blk_lo : q + bytes - blk_hi);
            abort();
        }
    }
    void check_res(const int16_t *p, size_t elems) const {
        if (res_lo && (p < res_lo || p + elems > res_hi)) {
            fprintf(stderr, "k_intra: residual access %td elements outside its LDS tile\n",
                    p < res_lo ? p - res_lo : p + elems - res_hi);
            abort();
        }
    }
#endif
};

// One picture's CTU windows, from which a component's Win is formed where it
// is used (a few scalar operations on the wave-uniform CTU and component)
// instead of being held: three Win and six plane pointers live across the TB
// loop kept k_intra at the 106-SGPR cap with 120-190 SGPRs spilled into VGPR
// lanes, a v_writelane / v_readlane per use.  The block
// layout is win_layout's: scratch, then per component the window, the left
// column and the row above, each 16-byte aligned.
template <typename Pel, int CF>
struct Frame {
    unsigned char *blk;    // the wave's window block (LDS)
    Pel *recon;            // the picture's Y plane; Cb, Cr follow
    const int16_t *resid;  // its Y residual plane (k_transform); Cb, Cr follow
    int W, H, cw, ch, log2ctb;
    uint32_t b0, b1;       // bytes of the Y and of one chroma component's part of the block
    static constexpr uint32_t al16(uint32_t v) { return (v + 15u) & ~15u; }
    static constexpr uint32_t kS0 = (uint32_t)((sizeof(IntraScratch) + 15) & ~size_t(15));
    __device__ __forceinline__ int csx(int k) const { return k ? (1 << log2ctb) >> chroma_sx(CF) : 1 << log2ctb; }
    __device__ __forceinline__ int csy(int k) const { return k ? (1 << log2ctb) >> chroma_sy(CF) : 1 << log2ctb; }
    __device__ __forceinline__ int pw(int k) const { return k ? cw : W; }
    __device__ __forceinline__ int ph(int k) const { return k ? ch : H; }
    __device__ __forceinline__ size_t plane_off(int k) const {
        return k ? (size_t)W * H + (k == 2 ? (size_t)cw * ch : 0) : 0;
    }
    __device__ __forceinline__ Pel *plane(int k) const { return recon + plane_off(k); }
    __device__ __forceinline__ void init(int log2, int w_, int h_, int cw_, int ch_) {
        log2ctb = log2, W = w_, H = h_, cw = cw_, ch = ch_;
        const uint32_t bps = sizeof(Pel), c0 = 1u << log2;
        b0 = al16(c0 * c0 * bps) + al16(c0 * bps) + al16((2 * c0 + 1) * bps);
        const uint32_t cx = CF ? c0 >> chroma_sx(CF) : 0, cy = CF ? c0 >> chroma_sy(CF) : 0;
        b1 = al16(cx * cy * bps) + al16(cy * bps) + al16((2 * cx + 1) * bps);
    }
    // component k's window at CTU column c of CTB row r
    __device__ __forceinline__ Win<Pel> win(int k, int c, int r) const {
        Win<Pel> w;
        const int sx = csx(k), sy = csy(k);
        const uint32_t cur = kS0 + (k ? b0 + (uint32_t)(k - 1) * b1 : 0u);
        const uint32_t left = cur + al16((uint32_t)(sx * sy) * sizeof(Pel));
        const uint32_t above = left + al16((uint32_t)sy * sizeof(Pel));
        w.cur = reinterpret_cast<Pel *>(blk + cur);
        w.left = reinterpret_cast<Pel *>(blk + left);
        w.above = reinterpret_cast<Pel *>(blk + above);
        w.csx = sx;
        w.csy = sy;
        w.cx0 = c * sx;
        w.cy0 = r * sy;
        return w;
    }
};

// The byte offsets of the luma and of the Cb window parts in a wave's block
// (Cr: Cb's + Frame::b1): constants of a CTB row, so a TB's window is a select
// on cIdx and an add.
struct WinOffs {
    uint32_t cur[2];
    int dl[2], da[2];  // from a window's samples to its left column and its row above, in samples
};
template <typename Pel, int CF>
__device__ __forceinline__ WinOffs win_offs(const Frame<Pel, CF> &F) {
    WinOffs o;
    const uint32_t bps = sizeof(Pel);
    const int l2 = F.log2ctb, lx = l2 - chroma_sx(CF), ly = l2 - chroma_sy(CF);
    o.cur[0] = F.kS0;
    o.dl[0] = (int)(F.al16(bps << (2 * l2)) / bps);
    o.da[0] = o.dl[0] + (int)(F.al16(bps << l2) / bps);
    o.cur[1] = F.kS0 + F.b0;
    o.dl[1] = (int)(F.al16(bps << (lx + ly)) / bps);
    o.da[1] = o.dl[1] + (int)(F.al16(bps << ly) / bps);
    return o;
}

// The facts of a TB record that depend on the record and on constants of its
// CTB row are formed for 64 records at once, one per lane, when the wave loads
// them, as the packed words of intra_rec.hpp (the per-TB checks and field
// extracts on the scalar unit were a large part of k_intra's instructions).
// intraPredAngle and invAngle (8.4.4.2.6) of a mode, for word B: one vector
// load per 64 records instead of two scalar loads from constant memory per TB.
__device__ __forceinline__ uint32_t tb_word_b(uint32_t a, const TbGeom &g) {
    const int m = (a & TBA_OK) ? tba_mode(a) : 0;
    return tb_pack_b(a, g, c_angle[m], c_inv_angle[m]);
}

#if !defined(HG_HOST_EMU)
// the sum over the lanes of each aligned group of m (2 <= m <= 64, a power of
// two) lanes, in every lane of the group: ds_swizzle xor steps inside 32-lane
// halves (one LDS-crossbar instruction each, against __shfl_xor's address
// arithmetic and bounds select), ds_bpermute across them
__device__ __forceinline__ int group_sum(int v, int m) {
    if (m >= 64) v += __builtin_amdgcn_ds_bpermute(((int)__lane_id() ^ 32) << 2, v);
    if (m >= 32) v += __builtin_amdgcn_ds_swizzle(v, 0x1f | (16 << 10));
    if (m >= 16) v += __builtin_amdgcn_ds_swizzle(v, 0x1f | (8 << 10));
    if (m >= 8) v += __builtin_amdgcn_ds_swizzle(v, 0x1f | (4 << 10));
    if (m >= 4) v += __builtin_amdgcn_ds_swizzle(v, 0x1f | (2 << 10));
    return v + __builtin_amdgcn_ds_swizzle(v, 0x1f | (1 << 10));
}
#endif

// The sample that stands at search position s of a TB's neighbours after the
// substitution of 8.4.4.2.2, read from the window: the lane's own source
// position by the closed form on the record's facts (no ballot and no cross-lane
// read), then one LDS read.  Only called where something is available.
template <typename Pel>
__device__ __forceinline__ int gather_at(const TbWin<Pel> &w, const Pel *cur, const TbSrcAddr &sa, int s, int n,
                                         uint32_t wd) {
    const int e = tb_src_at(sa, tb_subst_src(s, n, wd));
#if defined(HG_HOST_EMU)
    w.check_blk(cur + e, sizeof(Pel));
#endif
    return (int)cur[e];
}

// One TB from its record's words A, B and D (intra_rec.hpp) and its component's window.
template <typename Pel, int CF>
__device__ __attribute__((always_inline)) inline void predict_tb(IntraScratch *L, uint32_t wa, uint32_t wb,
                                                                 uint32_t wd, const TbWin<Pel> &w, int bd,
                                                                 bool strong, int lane) {
    const int log2n = tba_log2(wa), n = 1 << log2n, mode = tba_mode(wa), cidx = tba_cidx(wa);
    const int x0 = tba_lx(wa), y0 = tba_ly(wa);  // relative to the CTB's origin
    const int off = tbd_off(wd);                 // the TB's first sample in the window
    const bool filt = (wa & TBA_FILT) != 0;
    const int ns = 4 * n + 1;
    const bool cbf = (wa & TBA_CBF) != 0;
    // residual of a 4x4 / 8x8 TB (one sample per lane): loaded now, used after
    // the neighbour and filter phases, so the load latency hides behind them
    // (w.rt is the TB's first residual, formed by the caller only where it is in bounds: a pointer moved
    // before an LDS buffer is out of the object, and its flat address lost the aperture on the GPU)
    const int16_t *rt = w.rt;
#if defined(HG_HOST_EMU)
    if (cbf) w.check_res(rt, (size_t)(n - 1) * w.rp + n);
    w.check_blk(w.cur + off, ((size_t)((n - 1) << w.lsx) + n) * sizeof(Pel));
#endif
    const int r0 = (cbf && n <= 8 && lane < n * n) ? rt[(lane >> log2n) * w.rp + (lane & (n - 1))] : 0;
#if defined(HG_IABL_TB)  // measurement builds only (wrong pixels): the TB's work dropped
    if (r0 != 12345) return;
#endif
    // 1. + 2. the neighbours in search order with the substitution (8.4.4.2.2): s < 2n left
    //    column bottom-up, s == 2n corner, s > 2n top row left-to-right.  The record's word D says
    //    which groups are available; every position reads the sample that stands there afterwards.
    const TbSrcAddr sa = tb_src_addr(x0, y0, n, w.lsx, w.dl, w.da);
    const bool none = tb_subst_src(0, n, wd) < 0;  // nothing available (uniform): 1 << (bitDepth - 1)
    auto put = [&](int s, int v) {
        int16_t *dp = s < 2 * n ? L->left + (2 * n - s) : L->top + (s - 2 * n);  // (a select, not two exec regions)
        *dp = (int16_t)v;
        if (s == 2 * n) L->left[0] = (int16_t)v;
    };
#if defined(HG_HOST_EMU)
    for (int s = 0; s < ns; ++s) {  // (one lane: every position in turn, the kernel's arithmetic)
        const int sp = tb_subst_src(s, n, wd);
        if (sp >= 0) {  // the source is the window's sample at the position of search index sp
            int dx, dy;
            tb_search_pos(sp, n, &dx, &dy);
            const int xn = x0 + dx, yn = y0 + dy;
            const int e = yn < 0 ? w.da + xn + 1 : (xn < 0 ? w.dl + yn : (yn << w.lsx) + xn);
            if (e != tb_src_at(sa, sp)) {
                fprintf(stderr, "k_intra: search position %d of a TB at (%d, %d) n %d read at %d, not %d\n", sp, x0,
                        y0, n, tb_src_at(sa, sp), e);
                abort();
            }
        }
        put(s, none ? 1 << (bd - 1) : gather_at(w, w.cur, sa, s, n, wd));
    }
#elif defined(HG_IABL_GATHER)  // measurement builds only: no neighbour gather
#else
    if (ns <= 64) {  // 4x4 and 8x8 TBs (most of them): one chunk of 4n + 1 <= 33 samples
        // (lanes past the last position read its source: every lane's address is a sample's)
        const int v = none ? 1 << (bd - 1) : gather_at(w, w.cur, sa, min(lane, 4 * n), n, wd);
        if (lane < ns) put(lane, v);
    } else {
        // 16x16 (65 samples) needs two chunks, 32x32 (129) three
        const int nch = ns <= 128 ? 2 : 3;
        for (int k = 0; k < nch; ++k) {
            const int s = lane + 64 * k;
            const int v = none ? 1 << (bd - 1) : gather_at(w, w.cur, sa, min(s, 4 * n), n, wd);
            if (s < ns) put(s, v);
        }
    }
#endif
    wave_sync();
    // 3. filtering (8.4.4.2.3): luma, and chroma with 4:4:4
    const int16_t *lf = L->left, *tp = L->top;
    {
        if (filt) {  // (word A: luma or 4:4:4 chroma, not DC, not 4x4, the mode past the threshold)
            const int c = L->left[0];
            const bool bi = strong && cidx == 0 && n == 32 && abs(c + L->top[64] - 2 * L->top[32]) < (1 << (bd - 5)) &&
                            abs(c + L->left[64] - 2 * L->left[32]) < (1 << (bd - 5));
            // (selects, not a lane-dependent if / else chain: one exec-mask region
            // per arm cost more scalar instructions than the arithmetic)
            const int corner = (L->left[1] + 2 * c + L->top[1] + 2) >> 2;
            for (int i = lane; i <= 2 * n; i += kWave) {
                int a, b;
                if (bi) {  // (uniform; i == 0 and i == 64 are the interpolation's end points)
                    a = ((64 - i) * c + i * L->left[64] + 32) >> 6;
                    b = ((64 - i) * c + i * L->top[64] + 32) >> 6;
                } else {
                    const int im = i > 0 ? i - 1 : 0, ip = i < 2 * n ? i + 1 : i;
                    const int li = L->left[i], ti = L->top[i];
                    a = (L->left[ip] + 2 * li + L->left[im] + 2) >> 2;
                    b = (L->top[ip] + 2 * ti + L->top[im] + 2) >> 2;
                    a = i == 0 ? corner : (i == 2 * n ? li : a);
                    b = i == 0 ? corner : (i == 2 * n ? ti : b);
                }
                L->fl[i] = (int16_t)a;
                L->ft[i] = (int16_t)b;
            }
            wave_sync();
            lf = L->fl;
            tp = L->ft;
        }
    }
    const int maxv = (1 << bd) - 1;
    // 4. prediction (+ residual)
    int dc = 0;
    if (mode == 1) {  // DC: the 2n <= 64 references summed over lanes 0 .. 2n - 1, then broadcast
#if !defined(HG_HOST_EMU)
        int sum = lane < 2 * n ? (lane < n ? tp[1 + lane] : lf[1 + lane - n]) : 0;
        sum = __builtin_amdgcn_readlane(group_sum(sum, 2 * n), 0);
#else
        int sum = 0;
        for (int i = lane; i < 2 * n; i += kWave) sum += i < n ? tp[1 + i] : lf[1 + i - n];
#endif
        dc = (sum + n) >> (log2n + 1);
    }
    const int ang = tbb_ang(wb), inv = tbb_inv(wb);
    const bool pcm = (wa & TBA_PCM) != 0;
    auto predict_sample = [&](int o) {
        const int x = o & (n - 1), y = o >> log2n;
        int pv;
        if (mode == 0) {
            pv = ((n - 1 - x) * lf[1 + y] + (x + 1) * tp[1 + n] + (n - 1 - y) * tp[1 + x] + (y + 1) * lf[1 + n] + n) >>
                 (log2n + 1);
        } else if (mode == 1) {
            pv = dc;
            if (cidx == 0 && n < 32) {
                // the DC edge filter as selects over both reference reads (the
                // lane-dependent if / else chain cost an exec-mask region per arm)
                const int t = tp[1 + x], l = lf[1 + y];
                const int e = (x == 0 ? l : t) + (x == 0 && y == 0 ? t : dc) + 2 * dc + 2;
                pv = (x == 0 || y == 0) ? e >> 2 : dc;
            }
        } else {
            const int16_t *main_ = mode >= 18 ? tp : lf, *side = mode >= 18 ? lf : tp;
            const int a = mode >= 18 ? x : y, b = mode >= 18 ? y : x;  // a along the main direction
            const int idx = ((b + 1) * ang) >> 5, fact = ((b + 1) * ang) & 31;
            // both references read unconditionally (the second index is at most
            // 2n + 1, inside the 66-entry arrays): with iFact 0 the weighted sum
            // is the first reference exactly, so no lane-dependent branch
            const int p0 = *ang_ref(main_, side, inv, a + idx + 1), p1 = *ang_ref(main_, side, inv, a + idx + 2);
            pv = ((32 - fact) * p0 + fact * p1 + 16) >> 5;
            if (cidx == 0 && n < 32) {
                if (mode == 26) {
                    const int v = min(max(tp[1] + ((lf[1 + y] - lf[0]) >> 1), 0), maxv);
                    pv = x == 0 ? v : pv;
                }
                if (mode == 10) {
                    const int v = min(max(lf[1] + ((tp[1 + x] - tp[0]) >> 1), 0), maxv);
                    pv = y == 0 ? v : pv;
                }
            }
        }
        const int li = off + (y << w.lsx) + x;
        if (pcm) pv = 0;  // the residual is the PCM sample itself
        if (cbf) pv += (n <= 8 && o == lane) ? r0 : rt[y * w.rp + x];
        pv = min(max(pv, 0), maxv);
        w.cur[li] = (Pel)pv;
    };
#if defined(HG_IABL_PRED)  // measurement builds only: no prediction
    if (lane == 1000) predict_sample(0);
    if (false)
#elif !defined(HG_HOST_EMU)
    if (n <= 8) {  // one sample per lane: no loop
        if (lane < n * n) predict_sample(lane);
    } else
#endif
    {
        for (int o = lane; o < n * n; o += kWave) predict_sample(o);
    }
    wave_sync();
}

#if !defined(HG_HOST_EMU)
// The Cb and Cr TBs of one 4:2:0 chroma TU (n = 4 or 8) in one pass: lanes
// 0-31 predict Cb, lanes 32-63 Cr.  The two TBs share position, size,
// IntraPredModeC and neighbour availability, and chroma has no reference
// filtering (8.4.4.2.3) and no DC / angular edge filters (8.4.4.2.6, cIdx 0
// only), so each step of predict_tb runs once for both: 4n + 1 <= 33
// neighbours per half (a second chunk for the 33rd of an 8x8), a 32-lane DC
// reduction, and n * n <= 64 samples in two rounds of 32.  Scratch halves:
// left / top at + 33 * h.
template <typename Pel>
__device__ __attribute__((always_inline)) inline void predict_pair(IntraScratch *L, uint32_t wa, uint32_t wb,
                                                                   uint32_t wd, const TbWin<Pel> &wc, uint32_t dwin,
                                                                   uint32_t dres, int bd, int lane) {
    // lanes 0-31 predict Cb and 32-63 Cr: the pairing needs a full 64-lane wave
    static_assert(kWave == 64, "predict_pair splits a 64-lane wave into two halves");
    const int log2n = tba_log2(wa), n = 1 << log2n, mode = tba_mode(wa);
    const int x0 = tba_lx(wa), y0 = tba_ly(wa);  // relative to the CTB's origin
    const int off = tbd_off(wd);                 // the TB's first sample in the window
    const int h = lane >> 5, sl = lane & 31;
    // wc is the Cb window; Cr's lies dwin samples behind it, its residual dres elements behind Cb's
    // (a per-lane offset: a lane-dependent reference into an array of windows would put it in scratch)
    const TbWin<Pel> &w = wc;
    Pel *const cur = wc.cur + (h ? dwin : 0u);
    const int16_t *rt = wc.rt + (h ? dres : 0u);
    const bool cbf = (wa & (h ? TBA_CBF2 : TBA_CBF)) != 0;
    const bool pcm = (wa & (h ? TBA_PCM2 : TBA_PCM)) != 0;
    const int ns = 4 * n + 1, nch = n == 8 ? 2 : 1;
    // residuals (sample sl and sl + 32 of this half), used after the neighbour phase
    int r0 = 0, r1 = 0;
    if (cbf && sl < n * n) r0 = rt[(sl >> log2n) * w.rp + (sl & (n - 1))];
    if (cbf && sl + 32 < n * n) r1 = rt[((sl + 32) >> log2n) * w.rp + ((sl + 32) & (n - 1))];
    int16_t *left = L->left + 33 * h, *top = L->top + 33 * h;
    // 1. + 2. neighbours in search order with the substitution (8.4.4.2.2), as predict_tb: each half's
    // lane sl reads the sample that stands at position sl; the 33rd of an 8x8 (position 32, the last
    // above-right sample) is a second read, the same position in every lane
    {
        const TbSrcAddr sa = tb_src_addr(x0, y0, n, w.lsx, w.dl, w.da);
        const bool none = tb_subst_src(0, n, wd) < 0;  // (uniform)
        const int v = none ? 1 << (bd - 1) : gather_at(w, cur, sa, min(sl, 4 * n), n, wd);
        int16_t *dp = sl < 2 * n ? left + (2 * n - sl) : top + (sl - 2 * n);
        if (sl < ns) *dp = (int16_t)v;
        if (sl == 2 * n) left[0] = (int16_t)v;
        if (n == 8) {
            const int v32 = none ? 1 << (bd - 1) : gather_at(w, cur, sa, 32, n, wd);
            if (sl == 0) top[16] = (int16_t)v32;
        }
    }
    wave_sync();
    const int16_t *lf = left, *tp = top;
    const int maxv = (1 << bd) - 1;
    int dc = 0;
    const int ang = tbb_ang(wb), inv = tbb_inv(wb);
    const int16_t *main_ = mode >= 18 ? tp : lf, *side = mode >= 18 ? lf : tp;
    if (mode == 1) {  // each half sums its 2n <= 16 references in its lanes 0 .. 2n - 1
        const int sum = group_sum(sl < 2 * n ? (sl < n ? tp[1 + sl] : lf[1 + sl - n]) : 0, 2 * n);
        const int s0 = __builtin_amdgcn_readlane(sum, 0), s1 = __builtin_amdgcn_readlane(sum, 32);
        dc = ((h ? s1 : s0) + n) >> (log2n + 1);
    }
    for (int it = 0; it < nch; ++it) {
        const int o = sl + 32 * it;
        if (o < n * n) {
            const int x = o & (n - 1), y = o >> log2n;
            int pv;
            if (mode == 0) {
                pv = ((n - 1 - x) * lf[1 + y] + (x + 1) * tp[1 + n] + (n - 1 - y) * tp[1 + x] + (y + 1) * lf[1 + n] +
                      n) >> (log2n + 1);
            } else if (mode == 1) {
                pv = dc;
            } else {
                const int a = mode >= 18 ? x : y, b = mode >= 18 ? y : x;
                const int idx = ((b + 1) * ang) >> 5, fact = ((b + 1) * ang) & 31;
                // (both references unconditionally, as predict_tb: index <= 2n + 1 inside the half's 33)
                const int p0 = *ang_ref(main_, side, inv, a + idx + 1), p1 = *ang_ref(main_, side, inv, a + idx + 2);
                pv = ((32 - fact) * p0 + fact * p1 + 16) >> 5;
            }
            if (pcm) pv = 0;  // the residual is the PCM sample itself
            if (cbf) pv += it ? r1 : r0;
            pv = min(max(pv, 0), maxv);
            cur[off + (y << w.lsx) + x] = (Pel)pv;
        }
    }
    wave_sync();
}
#endif

}  // namespace

// Register budget: at most 5 waves per SIMD (<= 102 VGPRs, 76 used).  r04
// measured 7 (72 VGPRs) best against 8 and the compiler's own; with r05's
// lighter parse and transform, same-box pairs at 128 images gave 7: 19,690,
// 5: 20,210, 4: 20,020 Mpix/s (profiles/r05/ab/ab_b128_dot4.txt): fewer
// resident k_intra waves take less issue from the parse beside them.
// HG_INTRA_WPE=0 leaves it to the compiler.
#ifndef HG_INTRA_WPE
#define HG_INTRA_WPE 5
#endif
#if HG_INTRA_WPE > 0
#define HG_INTRA_ATTR __attribute__((amdgpu_waves_per_eu(HG_INTRA_WPE)))
#else
#define HG_INTRA_ATTR
#endif
// CF: the batch's chroma_format_idc (a compile-time constant: the 4:2:0 build
// carries no per-format arithmetic)
// LDS of k_intra's streaming mode beyond the windows: the transform tables
// (workgroup) and per wave the transform tiles (transform_tb, xform.hpp)
// (the transposed matrices s_mt; per wave the d tile 32 x 34, the g tile 32 x 32)
constexpr size_t kXfTablesBytes = sizeof(XfTab);
constexpr size_t kXfDBytes = 32 * kXfDStride32 * sizeof(int16_t), kXfGBytes = 32 * 32 * sizeof(int16_t);
constexpr size_t kXfWaveBytes = kXfDBytes + kXfGBytes;
static_assert(kXfTablesBytes % 16 == 0 && kXfWaveBytes % 16 == 0, "transform scratch alignment");
constexpr int kIntraPlanes = 0, kIntraStream = 1;

// One word per record of a wave's 64-record block, lane l holding record
// base + l's: read back for the TB at hand with one v_readlane (the emulation's
// single lane holds all 64).
#if defined(HG_HOST_EMU)
struct LaneWord {
    uint32_t v[64];
    uint32_t at(int l) const { return v[l]; }
};
// The block walk's events, counted by the emulation (HEIFGPU_INTRA_STATS=1: emu_intra
// prints them on an `intra_walk` line): what tests/test_intra_walk.py asserts its pictures reach.
struct WalkStats {
    std::atomic<uint64_t> records{0}, ok{0}, pairs{0}, ctus{0}, blocks{0};
    std::atomic<uint64_t> pair_splits{0};    // a Cb TB in lane 63 whose Cr TB opens the next block
    std::atomic<uint64_t> ctu_lane0{0};      // a CTU start at lane 0 of a block after the row's first
    std::atomic<uint64_t> blocks_no_ctu{0};  // a block without a CTU start
    std::atomic<uint64_t> rows_lt64{0}, rows_gt128{0};
    std::atomic<uint64_t> second_rows{0};    // a row that is not its wave's first
    // TBs predicted: 32x32 luma with filtered neighbours under strong smoothing, 4x4 luma, PCM
    std::atomic<uint64_t> tb32_strong{0}, luma4{0}, pcm{0};
};
static WalkStats g_walk;
static bool walk_stats_on() {
    static const bool on = [] {
        const char *e = std::getenv("HEIFGPU_INTRA_STATS");
        return e && std::atoi(e) != 0;
    }();
    return on;
}
#else
struct LaneWord {
    uint32_t v = 0;
    __device__ __forceinline__ uint32_t at(int l) const { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
};
#endif
constexpr uint32_t kGaveUp = ~0u;                 // a wave's progress word: it gave its rows up
constexpr uint64_t kRedoPatience = 200000000ull;  // 2 s (10 ns ticks): the parse is over by then

// Mode kIntraPlanes: k_intra, residuals from k_transform's planes.
// Mode kIntraStream: k_intra_stream, launched beside the spread parse of the same decode:
// each row's TU records are consumed as the parse publishes them (agent-scope
// per-row TU counts behind its progress words) and every coded TB is
// transformed by the wave itself (transform_tb into LDS) right before its
// prediction, so no k_transform pass and no residual planes; the
// reconstruction trails the parse by a CTU instead of starting after it.
// (r04's third mode, k_intra_fused: the in-line transform after the parse
// instead of k_transform + k_intra, lost beside the next parse, 12.2-12.9
// against 18.6 Gpix/s; removed in r05)
template <typename Pel, int CF, int Mode>
__device__ __attribute__((always_inline)) inline void intra_body(const BatchArgs &a, unsigned char *smem) {
    constexpr bool Poll = Mode == kIntraStream;       // rows consumed while the parse writes them
    constexpr bool XfInline = Poll;                   // each TB transformed by the wave (no k_transform)
    const int nw = (int)HG_UNI(blockDim.x >> 6);
    const int pic = a.pic0 + blockIdx.x;
    const int wave = (int)HG_UNI(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const PicDesc pd = a.pics[pic];
    if (pd.flags & PD_ASSEMBLY) return;  // no coded data of its own (uniform: the whole workgroup leaves)
    // second launch: only the pictures the first gave up (its done word, after the TU counts)
    if (Poll && a.stream_redo && hg_load_agent(a.xntu + a.total_rows + pic) != 0) return;
    const SeqParams sp = a.seqs[pd.seq];
    const int W = sp.width, H = sp.height, log2ctb = sp.log2_ctb;
    const int wctb = (W + (1 << log2ctb) - 1) >> log2ctb, hctb = (H + (1 << log2ctb) - 1) >> log2ctb;
    constexpr int chroma = CF;  // = sp.chroma_format (launch_intra picks the instantiation)
    const int cw = chroma ? W >> chroma_sx(chroma) : 0, ch = chroma ? H >> chroma_sy(chroma) : 0;
    const int ncomp = chroma ? 3 : 1;
    const bool strong = (sp.flags & SP_STRONG_INTRA) != 0;
    const WinLayout lay = win_layout(log2ctb, chroma, (int)sizeof(Pel));
    uint32_t *progress = reinterpret_cast<uint32_t *>(smem);  // [nw], 64 B reserved
    Frame<Pel, CF> F;
    F.blk = smem + 64 + (size_t)wave * lay.bytes;
    F.recon = reinterpret_cast<Pel *>(a.recon + pd.recon_off);
    F.resid = a.resid + pd.resid_off;
    F.init(log2ctb, W, H, cw, ch);
    XfScratch X{};
    if constexpr (XfInline) {
        unsigned char *tab = smem + 64 + (size_t)nw * lay.bytes;
        unsigned char *xw = tab + kXfTablesBytes + (size_t)wave * kXfWaveBytes;
        X = XfScratch{reinterpret_cast<int16_t *>(xw), reinterpret_cast<int16_t *>(xw + kXfDBytes),
                      reinterpret_cast<const XfTab *>(tab)};
        xf_tables(reinterpret_cast<XfTab *>(tab), lane);
    }
    IntraScratch *S = reinterpret_cast<IntraScratch *>(F.blk);
    progress[wave] = 0;  // every lane writes the same value
    __syncthreads();
    const uint32_t stride = (uint32_t)wctb + 1;
    // split (a.intra_split): waves in pairs per CTB row, luma on the even one and
    // Cb, Cr on the odd one.  Chroma prediction reads chroma neighbours only, so
    // the two TB chains of a CTU run side by side instead of one after the other
    const bool split = a.intra_split != 0 && ncomp == 3;
    const int cls = split ? (wave & 1) : 0, rw = split ? wave >> 1 : wave, nrw = split ? nw >> 1 : nw;
    const int k0 = split && cls ? 1 : 0, k1 = split && !cls ? 1 : ncomp;  // this wave's components
    const int prev_wave = split ? ((rw + nrw - 1) % nrw) * 2 + cls : (wave + nw - 1) % nw;
    const bool wpp = (sp.flags & SP_WPP) != 0;
    bool gave_up = false;  // (streaming, first launch: no parse progress for a while)
    const TbGeom G{log2ctb, chroma, W, H, cw, ch};
    const WinOffs wo = win_offs(F);  // constants of the picture: a TB's window is a select on cIdx and an add
    constexpr int SX = chroma_sx(CF);
    const uint32_t dwin = F.b1 / (uint32_t)sizeof(Pel);  // from a Cb window part to Cr's, samples
    const uint32_t dres = (uint32_t)cw * (uint32_t)ch;   // from a Cb residual to Cr's, elements
#if defined(HG_HOST_EMU)
    // (split: the records and the walk's events by the luma wave, the pairs by the chroma wave)
    const bool stats = walk_stats_on() && cls == 0 && !(Poll && a.stream_redo);
    const bool stats_c = walk_stats_on() && k0 <= 1 && k1 > 1;
#endif
    for (int r = rw; r < hctb; r += nrw) {
        // streaming: TUs [0, ntu) of the row are known written; `done` once the parse finished the row
        uint32_t ntu = Poll ? 0u : a.row_counts[2 * (pd.row_off + r)];
        bool row_done = !Poll;
        const TuRec *tus = a.tus + pd.tu_off + (uint64_t)r * pd.tu_cap_row;
        const CoefSrc<Poll> coefs{a.coefs + pd.coef_off + (uint64_t)r * pd.coef_cap_row};
        int cur = -1;
        // finish CTU `cur`: write the window back, keep its last column as `left`
        auto finish_ctu = [&]() {
#if !defined(HG_IABL_CTU)  // (HG_IABL_CTU, measurement builds only, wrong pixels: the per-CTU copies dropped)
            _Pragma("nounroll") for (int k = 0; k < 3; ++k) {
                if (k >= ncomp) break;
                if (k < k0 || k >= k1) continue;
                const Win<Pel> w = F.win(k, cur, r);
                Pel *const plane = F.plane(k);
                const int PW = F.pw(k), PH = F.ph(k);
                const int vw = min(w.csx, PW - w.cx0), vh = min(w.csy, PH - w.cy0);
                if (vw == w.csx && !(PW & 3) && !(reinterpret_cast<uintptr_t>(plane) & (4 * sizeof(Pel) - 1))) {
                    // full-width CTU: four samples per lane, one 4- (8-) byte store
                    const int lq = __builtin_ctz((unsigned)w.csx) - 2;
                    for (int o = lane; o < (vh << lq); o += kWave) {
                        const int x = (o & ((1 << lq) - 1)) << 2, y = o >> lq;
                        *reinterpret_cast<Quad<Pel> *>(plane + (size_t)(w.cy0 + y) * PW + w.cx0 + x) =
                            *reinterpret_cast<const Quad<Pel> *>(w.cur + y * w.csx + x);
                    }
                } else {
                    for (int o = lane; o < vw * vh; o += kWave) {
                        const int x = o % vw, y = o / vw;
                        plane[(size_t)(w.cy0 + y) * PW + w.cx0 + x] = w.cur[y * w.csx + x];
                    }
                }
                for (int y = lane; y < w.csy; y += kWave) w.left[y] = w.cur[y * w.csx + w.csx - 1];
            }
#endif
            wave_sync();
            HG_FENCE_REL();
            hg_atomic_store(&progress[wave], (uint32_t)r * stride + (uint32_t)cur + 1u);
        };
        // start CTU c (after the row above has finished CTU c + 1): the row above, corner .. above-right;
        // false: the row above was given up
        auto start_ctu = [&](int c) -> bool {
            if (r > 0) {
                const uint32_t need = (uint32_t)(r - 1) * stride + (uint32_t)min(c + 2, wctb);
                for (uint32_t spin = 0;; ++spin) {
                    const uint32_t v = (uint32_t)HG_UNI(hg_atomic_load(&progress[prev_wave]));
                    if (Poll && v == kGaveUp) return false;  // the row above was given up: so is this one
                    if (v >= need) break;
                    if (spin > (1u << 24)) {  // bounded: never hang the device
                        if (lane == 0) atomicOr(&a.status[pic], ST_SUBSTREAM_END);
                        break;
                    }
                    HG_SLEEP();
                }
                HG_FENCE_ACQ();
            }
#if !defined(HG_IABL_CTU)
            _Pragma("nounroll") for (int k = 0; k < 3; ++k) {
                if (k >= ncomp) break;
                if (k < k0 || k >= k1) continue;
                const Win<Pel> w = F.win(k, c, r);
                const Pel *const plane = F.plane(k);
                const int PW = F.pw(k);
                const int yg = w.cy0 - 1;
                for (int i = lane; i <= 2 * w.csx; i += kWave) {
                    const int xg = w.cx0 - 1 + i;
                    w.above[i] = (yg >= 0 && xg >= 0 && xg < PW) ? plane[(size_t)yg * PW + xg] : (Pel)0;
                }
            }
#endif
            wave_sync();
            return true;
        };
#if defined(HG_HOST_EMU)
        if (stats) {
            g_walk.rows_lt64 += ntu < 64 && !Poll;
            g_walk.rows_gt128 += ntu > 128 && !Poll;
            g_walk.second_rows += r != rw;
        }
#endif
        bool stop = false;  // a record names a CTU outside the row: the row ends there
        for (uint32_t t = 0; !stop;) {  // t: the row's first record not consumed yet
            if constexpr (Poll) {
                if (t >= ntu && !row_done) {
                    // wait until the parse has published TU t of this row or finished the row
                    const uint32_t *pw = a.xprog + pd.row_off + (wpp ? r : 0);
                    const uint32_t *nw_ = a.xntu + pd.row_off + r;
                    const uint32_t fin = (uint32_t)(r + 1) * (uint32_t)wctb;
                    // Patience: nothing guarantees that the parse runs beside this kernel (a
                    // profiler that serialises dispatches, a busy device), so after `patience`
                    // without progress the first launch gives the picture up, and the second
                    // launch (after the parse) reconstructs it; there a stall is an error.
                    const uint64_t patience = (uint64_t)a.stream_patience_us * 100u;
                    uint32_t seen_n = ~0u, seen_p = ~0u;
                    uint64_t t_last = 0;
                    for (;;) {
                        if (!a.stream_redo && !patience) {  // (test knob: every picture to the second launch)
                            gave_up = true;
                            break;
                        }
                        const uint32_t n_ = (uint32_t)HG_UNI(hg_load_agent(nw_));
                        if (n_ > t) {
                            ntu = n_;
                            break;
                        }
                        const uint32_t pv = (uint32_t)HG_UNI(hg_load_agent(pw));
                        if (pv >= fin) {  // row finished (or stopped: kProgDone)
                            ntu = (uint32_t)HG_UNI(hg_load_agent(nw_));
                            row_done = true;
                            break;
                        }
                        const uint64_t now = hg_clock_10ns();
                        if (n_ != seen_n || pv != seen_p) {
                            seen_n = n_;
                            seen_p = pv;
                            t_last = now;
                        } else if (now - t_last > (a.stream_redo ? kRedoPatience : patience)) {
                            if (!a.stream_redo) {
                                gave_up = true;
                            } else {  // bounded: never hang the device
                                if (lane == 0) atomicOr(&a.status[pic], ST_SUBSTREAM_END);
                                row_done = true;
                            }
                            break;
                        }
                        HG_STREAM_SLEEP();
                    }
                    if (gave_up) break;
                    // the records behind the count / progress word: formally ordered
                    // after the poll (the parse published them with an agent release)
                    HG_ACQ_AGENT();
                }
            }
            if (t >= ntu) break;  // the row's last record is consumed (or the parse stalled: the status says so)
            // ---- the block of up to 64 records that holds record t, one per lane: the packed
            // words (intra_rec.hpp) and the two masks the walk below follows
            const uint32_t base = t & ~63u;
            LaneWord wa, wb, wc, wd, wctu;
#if !defined(HG_HOST_EMU)
            uint4 tblk = make_uint4(0, 0, 0, 0);  // (streaming: the record itself, for transform_tb)
#endif
            // lane l's words of record base + l (zero where the block has no such record yet)
            auto form = [&](int l, uint32_t &A, uint32_t &B, uint32_t &C, uint32_t &D, uint32_t &ctu) {
                A = B = C = D = ctu = 0;
                const uint32_t i = base + (uint32_t)l;
                if (i < t || i >= ntu) return;
                TuRec q;
#if defined(HG_HOST_EMU)
                q = tus[i];
#else
                if constexpr (Poll) {
                    const uint64_t *p = reinterpret_cast<const uint64_t *>(tus + i);
                    const uint64_t lo = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint64_t hi = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    tblk = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
                } else {
                    tblk = *reinterpret_cast<const uint4 *>(tus + i);
                }
                __builtin_memcpy(&q, &tblk, sizeof(q));
#endif
                ctu = q.ctu;
                A = tb_pack_a(q, G, r);
                bool fits = true;
                C = tb_pack_c(q, A, G, &fits);
                if (!fits) A = C = 0;
#if !defined(HG_INTRA_NO_PAIR)
                if constexpr (!XfInline && CF == 1) {
                    // a 4x4 / 8x8 Cb TB whose next record is its Cr TB (same TU): both in one pass,
                    // unless the Cr record opens the next block (a pair never spans two blocks)
                    if ((A & TBA_OK) && tba_cidx(A) == 1 && tba_log2(A) <= 3 && i + 1 < ntu) {
                        TuRec nq;
#if defined(HG_HOST_EMU)
                        nq = tus[i + 1];
#else
                        const uint4 nb = *reinterpret_cast<const uint4 *>(tus + i + 1);
                        __builtin_memcpy(&nq, &nb, sizeof(nq));
#endif
                        const bool cr = (nq.flags & TU_CIDX_MASK) == 2 && nq.x == q.x && nq.y == q.y &&
                                        nq.log2 == q.log2 && nq.mode == q.mode && nq.ctu == q.ctu;
                        if (cr && l < 63) A = tb_pack_pair(A, nq.flags);
#if defined(HG_HOST_EMU)
                        if (stats_c) g_walk.pairs += cr && l < 63, g_walk.pair_splits += cr && l == 63;
#endif
                    }
                }
#endif
                B = tb_word_b(A, G);
                D = tb_pack_d(A, G, (int)q.ctu, r);  // (the neighbours: of the record's CTB column and this row)
            };
            // a record is this wave's where it is OK, of the wave's components, and not the Cr TB of a
            // pair; it opens a CTU where its CTU is not the record's before it (the first one: not `cur`)
            auto is_mine = [&](uint32_t A, uint32_t prevA) {
                const int k = tba_cidx(A);
                return (A & TBA_OK) && k >= k0 && k < k1 && !(prevA & TBA_PAIR);
            };
            uint64_t mine_m, nctu_m;
#if defined(HG_HOST_EMU)
            mine_m = nctu_m = 0;
            {
                uint32_t prevA = 0, prevc = (uint32_t)cur;
                for (int l = 0; l < 64; ++l) {
                    form(l, wa.v[l], wb.v[l], wc.v[l], wd.v[l], wctu.v[l]);
                    const uint32_t i = base + (uint32_t)l;
                    const bool valid = i >= t && i < ntu;
                    if (valid && is_mine(wa.v[l], prevA)) mine_m |= 1ull << l;
                    if (valid && wctu.v[l] != prevc) nctu_m |= 1ull << l;
                    if (valid) prevA = wa.v[l], prevc = wctu.v[l];
                }
            }
            if (stats) {
                g_walk.blocks += 1;
                g_walk.blocks_no_ctu += nctu_m == 0;
                g_walk.ctu_lane0 += base > 0 && (nctu_m & 1ull);
                g_walk.ctus += (uint64_t)__builtin_popcountll(nctu_m);
                for (int l = 0; l < 64; ++l) {
                    const uint32_t i = base + (uint32_t)l;
                    if (i < t || i >= ntu) continue;
                    g_walk.records += 1;
                    g_walk.ok += (wa.v[l] & TBA_OK) != 0;
                }
            }
#else
            {
                form(lane, wa.v, wb.v, wc.v, wd.v, wctu.v);
                const uint32_t i = base + (uint32_t)lane;
                const bool valid = i >= t && i < ntu;
                const int pl = max(lane - 1, 0);
                const uint32_t pA = (uint32_t)__shfl((int)wa.v, pl, 64), pc = (uint32_t)__shfl((int)wctu.v, pl, 64);
                const uint32_t prevA = lane == 0 ? 0u : pA;  // (a lane before record t holds zero words)
                const uint32_t prevc = (i == t) ? (uint32_t)cur : pc;
                mine_m = __ballot(valid && is_mine(wa.v, prevA));
                nctu_m = __ballot(valid && wctu.v != prevc);
            }
#endif
            // ---- the walk: TBs at the set bits of mine_m, CTU finish / start at those of nctu_m
            // (the two masks are the loop's state, their lowest bits cleared as the walk passes them:
            // a third mask of both would be two more live SGPRs)
            while (mine_m | nctu_m) {
                const int l = __builtin_ctzll(mine_m | nctu_m);
                const uint64_t bit = 1ull << l;
                const bool tb = (mine_m & bit) != 0;
                mine_m &= ~bit;
                if (nctu_m & bit) {
                    nctu_m &= ~bit;
                    const int c = (int)wctu.at(l);
                    if (cur >= 0) finish_ctu();
                    cur = -1;
                    if (c >= wctb) {
                        stop = true;
                        break;
                    }
                    if (!start_ctu(c)) {
                        gave_up = true;
                        break;
                    }
                    cur = c;
                }
                if (!tb) continue;
                const uint32_t A = wa.at(l), B = wb.at(l), D = wd.at(l);
                const int cidx = tba_cidx(A), kc = cidx ? 1 : 0;
#if defined(HG_HOST_EMU)
                if (walk_stats_on() && !(Poll && a.stream_redo)) {
                    g_walk.tb32_strong += cidx == 0 && tba_log2(A) == 5 && (A & TBA_FILT) && strong;
                    g_walk.luma4 += cidx == 0 && tba_log2(A) == 2;
                    g_walk.pcm += (A & TBA_PCM) != 0;
                }
#endif
                // the TB's component window: a select on cIdx and an add
                TbWin<Pel> w;
                unsigned char *const wbase = F.blk + (cidx == 2 ? F.b1 : 0u);
                w.cur = reinterpret_cast<Pel *>(wbase + wo.cur[kc]);
                w.dl = wo.dl[kc];
                w.da = wo.da[kc];
                w.lsx = log2ctb - (cidx ? SX : 0);
                w.rp = cidx ? cw : W;
#if defined(HG_HOST_EMU)
                w.blk_lo = F.blk;
                w.blk_hi = F.blk + F.kS0 + F.b0 + (CF ? 2 * F.b1 : 0u);
#endif
                if constexpr (XfInline) {
                    // the TB's residual, transformed by this wave into LDS (pitch n)
                    w.rt = X.d;
                    if (A & TBA_CBF) {
                        TuRec tu;
#if defined(HG_HOST_EMU)
                        tu = tus[base + (uint32_t)l];
#else
                        const uint4 rr = make_uint4((uint32_t)__builtin_amdgcn_readlane((int)tblk.x, l),
                                                    (uint32_t)__builtin_amdgcn_readlane((int)tblk.y, l),
                                                    (uint32_t)__builtin_amdgcn_readlane((int)tblk.z, l),
                                                    (uint32_t)__builtin_amdgcn_readlane((int)tblk.w, l));
                        __builtin_memcpy(&tu, &rr, sizeof(tu));
#endif
                        const int n = 1 << tba_log2(A);
                        transform_tb<Poll>(tu, coefs, sp, a.sf, X, X.d, n, lane);
                        w.rp = n;
#if defined(HG_HOST_EMU)
                        w.res_lo = X.d;
                        w.res_hi = X.d + 32 * 32;  // (the 2 KB residual tile of XfScratch)
#endif
                    }
                } else {
                    w.rt = F.resid + wc.at(l);  // (word C: inside the picture's residual planes for an OK record)
                }
                if (!XfInline && (A & TBA_PAIR)) {
#if defined(HG_HOST_EMU)
                    // (one lane: the Cb TB, then the Cr TB from the pair's bits, each as a TB of its own)
                    predict_tb<Pel, CF>(S, A, B, D, w, sp.bit_depth_c, strong, lane);
                    const uint32_t A2 = (A & ~((3u << TBA_CIDX_SHIFT) | TBA_CBF | TBA_PCM)) | (2u << TBA_CIDX_SHIFT) |
                                        ((A & TBA_CBF2) ? TBA_CBF : 0u) | ((A & TBA_PCM2) ? TBA_PCM : 0u);
                    w.cur += dwin;
                    w.rt += dres;
                    predict_tb<Pel, CF>(S, A2, B, D, w, sp.bit_depth_c, strong, lane);
#else
                    predict_pair<Pel>(S, A, B, D, w, dwin, dres, sp.bit_depth_c, lane);
#endif
                    continue;
                }
                predict_tb<Pel, CF>(S, A, B, D, w, cidx ? sp.bit_depth_c : sp.bit_depth_y, strong, lane);
            }
            if (gave_up) break;
            t = min(ntu, base + 64u);
        }
        if (!gave_up && !stop && cur >= 0) finish_ctu();  // after the row's last record: the open CTU
        if (gave_up) {  // (the waves below see it and give up too)
            hg_atomic_store(&progress[wave], kGaveUp);
            break;
        }
        HG_FENCE_REL();
        hg_atomic_store(&progress[wave], (uint32_t)r * stride + (uint32_t)wctb);
    }
    if constexpr (Poll) {
        // first launch: the picture is done unless a wave gave up (its words then say kGaveUp)
        __syncthreads();
        if (!a.stream_redo && wave == 0) {
            bool ok = true;
            for (int w = 0; w < nw; ++w) ok = ok && hg_atomic_load(&progress[w]) != kGaveUp;
            if (lane == 0) a.xntu[a.total_rows + pic] = ok ? 1u : 0u;
        }
    }
}

template <typename Pel, int CF>
__global__ void __launch_bounds__(kMaxWaves * 64) HG_INTRA_ATTR k_intra(BatchArgs a) {
#if defined(HG_HOST_EMU)
    unsigned char *smem = g_emu.smem;
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#endif
    intra_body<Pel, CF, kIntraPlanes>(a, smem);
}

// (no waves-per-EU cap: the transform's registers come on top of the prediction's)
template <typename Pel, int CF>
__global__ void __launch_bounds__(kMaxWaves * 64) k_intra_stream(BatchArgs a) {
#if defined(HG_HOST_EMU)
    unsigned char *smem = g_emu.smem;
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#endif
    intra_body<Pel, CF, kIntraStream>(a, smem);
}

// luma / chroma wave pairs (k_intra's split): for batches of few pictures,
// where the per-picture TB chain is the latency (HEIFGPU_INTRA_SPLIT=0/1 forces it)
static bool intra_split_for(const BatchArgs &a, int nw) {
    static const int forced = [] {
        const char *e = std::getenv("HEIFGPU_INTRA_SPLIT");
        return e ? std::atoi(e) : -1;
    }();
    if (a.chroma_format == 0) return false;
    if (forced >= 0) return forced != 0;
    return nw >= 4 && (long)a.n_pics * a.max_rows <= 4096;
}

// waves of a split workgroup: two per row in flight, within the LDS budget and kMaxWaves
static int intra_split_waves(const BatchArgs &a, int nw) {
    int cap = intra_waves(a.max_log2ctb, a.chroma_format, a.bytes_per_sample, 2 * a.max_rows);
    int w = 2 * nw < cap ? 2 * nw : cap;
    w &= ~1;
    return w < 2 ? 2 : w;
}

static int intra_launch_waves(const BatchArgs &a) {
    // all pictures of a batch share bit depth and chroma format; the CTB size
    // may differ, so size for the largest one.  HEIFGPU_INTRA_WAVES caps the
    // waves per picture (tuning: fewer waves = more pictures per CU).
    // Measured (128 x 48 tiles): 16 waves/picture 142 ms, 8: 71, 4: 48, 1: 61 —
    // many pictures per CU beat deep per-picture row parallelism, so waves per
    // picture shrink as the batch grows.  Floor 2: alone 4 and 2 waves tie
    // (~40 ms), but beside the next decode's k_parse (pipelined) the smaller
    // workgroup fits the LDS that k_parse leaves free (bench 12.0 -> 12.5-13.0 Gpix/s).
    static const int forced = [] {
        const char *e = std::getenv("HEIFGPU_INTRA_WAVES");
        return e ? std::atoi(e) : 0;
    }();
    int cap = forced > 0 ? forced : kResidentIntraWaves / (a.n_pics > 0 ? a.n_pics : 1);
    if (forced <= 0) cap = cap < 2 ? 2 : cap;
    const int nw = intra_waves(a.max_log2ctb, a.chroma_format, a.bytes_per_sample, a.max_rows);
    return cap < nw ? cap : nw;
}

// k_intra_stream: four waves per picture (rows r, r + 4, ...), no luma / chroma
// split.  It only has to keep up with the parse, and its waves share the CUs
// with the parse's: one image, same box, 4 waves 28.2-28.3 ms per pipelined
// step against 28.9-29.4 with 16 (latency 28.0-28.1 either way, the parse's)
static int stream_waves(int nw) {
    static const int forced = [] {
        const char *e = std::getenv("HEIFGPU_INTRA_WAVES");
        return e ? std::atoi(e) : 0;
    }();
    if (forced > 0) return nw;
    return nw < 4 ? nw : 4;
}

static size_t intra_lds_bytes(const BatchArgs &a, int nw) {
    size_t b = 64 + (size_t)nw * win_layout(a.max_log2ctb, a.chroma_format, a.bytes_per_sample).bytes;
    if (a.intra_stream) b += kXfTablesBytes + (size_t)nw * kXfWaveBytes;
    return b;
}

// waves of a launch, the streaming mode's extra LDS included (pairs stay pairs)
static int intra_fit_waves(const BatchArgs &a, int nw) {
    while (nw > 1 && intra_lds_bytes(a, nw) > kIntraLdsBudget) nw -= a.intra_split ? 2 : 1;
    return nw < 1 ? 1 : nw;
}

#if defined(HG_HOST_EMU)
template <int CF>
static void emu_intra_cf(const BatchArgs &a, int nw) {
    const size_t lds = intra_lds_bytes(a, nw);
    if (a.intra_stream) {
        if (a.bytes_per_sample == 1) emu_launch(k_intra_stream<uint8_t, CF>, a.n_pics, 1, nw, a, false, lds);
        else emu_launch(k_intra_stream<uint16_t, CF>, a.n_pics, 1, nw, a, false, lds);
        return;
    }
    if (a.bytes_per_sample == 1) emu_launch(k_intra<uint8_t, CF>, a.n_pics, 1, nw, a, false, lds);
    else emu_launch(k_intra<uint16_t, CF>, a.n_pics, 1, nw, a, false, lds);
}
void emu_intra(const BatchArgs &a0) {
    BatchArgs a = a0;
    int nw = intra_launch_waves(a);
    if (a.intra_stream) nw = stream_waves(nw);
    a.intra_split = !a.intra_stream && intra_split_for(a, nw) ? 1 : 0;
    if (a.intra_split) nw = intra_split_waves(a, nw);
    nw = intra_fit_waves(a, nw);
    switch (a.chroma_format) {
    case 0: emu_intra_cf<0>(a, nw); break;
    case 2: emu_intra_cf<2>(a, nw); break;
    case 3: emu_intra_cf<3>(a, nw); break;
    default: emu_intra_cf<1>(a, nw); break;
    }
    if (walk_stats_on())  // (totals of the process so far)
        printf("intra_walk records %llu ok %llu pairs %llu ctus %llu blocks %llu pair_splits %llu ctu_lane0 %llu "
               "blocks_no_ctu %llu rows_lt64 %llu rows_gt128 %llu second_rows %llu tb32_strong %llu luma4 %llu pcm %llu\n",
               (unsigned long long)g_walk.records, (unsigned long long)g_walk.ok, (unsigned long long)g_walk.pairs,
               (unsigned long long)g_walk.ctus, (unsigned long long)g_walk.blocks,
               (unsigned long long)g_walk.pair_splits, (unsigned long long)g_walk.ctu_lane0,
               (unsigned long long)g_walk.blocks_no_ctu, (unsigned long long)g_walk.rows_lt64,
               (unsigned long long)g_walk.rows_gt128, (unsigned long long)g_walk.second_rows,
               (unsigned long long)g_walk.tb32_strong, (unsigned long long)g_walk.luma4, (unsigned long long)g_walk.pcm);
}
#else
template <int CF>
static void launch_intra_cf(const BatchArgs &a, int nw, size_t lds, hipStream_t s) {
    if (a.intra_stream) {
        if (a.bytes_per_sample == 1)
            hipLaunchKernelGGL((k_intra_stream<uint8_t, CF>), dim3(a.n_pics), dim3(nw * 64), lds, s, a);
        else
            hipLaunchKernelGGL((k_intra_stream<uint16_t, CF>), dim3(a.n_pics), dim3(nw * 64), lds, s, a);
        return;
    }
    if (a.bytes_per_sample == 1)
        hipLaunchKernelGGL((k_intra<uint8_t, CF>), dim3(a.n_pics), dim3(nw * 64), lds, s, a);
    else
        hipLaunchKernelGGL((k_intra<uint16_t, CF>), dim3(a.n_pics), dim3(nw * 64), lds, s, a);
}
hipError_t launch_intra(const BatchArgs &a0, hipStream_t s) {
    BatchArgs a = a0;
    int nw = intra_launch_waves(a);
    if (a.intra_stream) nw = stream_waves(nw);
    a.intra_split = !a.intra_stream && intra_split_for(a, nw) ? 1 : 0;
    if (a.intra_split) nw = intra_split_waves(a, nw);
    nw = intra_fit_waves(a, nw);
    const size_t lds = intra_lds_bytes(a, nw);
    switch (a.chroma_format) {
    case 0: launch_intra_cf<0>(a, nw, lds, s); break;
    case 2: launch_intra_cf<2>(a, nw, lds, s); break;
    case 3: launch_intra_cf<3>(a, nw, lds, s); break;
    default: launch_intra_cf<1>(a, nw, lds, s); break;
    }
    return hipGetLastError();
}
#endif

// The streaming knobs, read from the environment when a context is created
// (heifgpu_create; the emulation driver reads them once per run):
// HEIFGPU_STREAM=0 turns k_intra_stream off, HEIFGPU_STREAM_MAX_PICS moves its
// batch limit (tuning), HEIFGPU_STREAM_PATIENCE_US is how long the first
// launch waits without parse progress before it gives a picture up to the
// second launch (0: every picture, a test knob).
StreamKnobs stream_knobs_from_env() {
    StreamKnobs k;
    const char *e = std::getenv("HEIFGPU_STREAM");
    k.enabled = !(e && std::atoi(e) == 0);
    const char *m = std::getenv("HEIFGPU_STREAM_MAX_PICS");
    k.max_pics = m && *m ? std::atoi(m) : kStreamMaxPics;
    const char *p = std::getenv("HEIFGPU_STREAM_PATIENCE_US");
    k.patience_us = p && *p ? (uint32_t)std::strtoul(p, nullptr, 10) : 200000u;
    return k;
}

// Streaming reconstruction (k_intra_stream beside the spread parse) for the
// small batches (up to 192 pictures: four 4032x3024 images, kStreamMaxPics)
bool intra_stream_for(int parse_mode, int n_pics, bool has_assembly, const StreamKnobs &k) {
    return k.enabled && parse_mode == PARSE_SPREAD && !has_assembly && n_pics > 0 && n_pics <= k.max_pics;
}

}  // namespace hg
