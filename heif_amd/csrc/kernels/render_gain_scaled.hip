// render_gain_scaled.hip — k_render_gain_scaled: a window of a batch of SDR base pictures with
// their gain maps → the HDR rendition on another grid, interleaved RGB(A) as linear half-float
// or PQ codes, in one launch (heifgpu_render_batch_gain_scaled; include/heifgpu.h "Gain-map HDR
// render", the scaled call).  The full-size HDR surface is never written: the base's depth-B
// integers, the alpha samples and the Q8 gain codes are area-averaged, each exactly, and the HDR
// formula runs once per OUTPUT pixel on the averages.
//
// The kernel has k_render_scaled's shape (render.hip): grid (tile, image), 256 threads, a
// workgroup owns na x nb output pixels in the source's axes (8 x 64..256 for maps that keep the
// axes, 64 x 16..64 for maps that swap them), and walks every a-line's source footprint in
// chunks of 512 source columns:
//   1. lanes along the source's x, two columns per thread: beside scale_acc's converted channels
//      (render_px.hpp) a thread accumulates the gain code of its positions.  The map's column
//      taps and fx are the thread's, found once per workgroup for the first chunk; its row taps
//      and fy are uniform per source row and walked with the rows in integers (GainTapWalk,
//      gain_xform.hpp: no double-precision quotient per row).  A map row (four samples: two taps
//      of either column) is loaded when the walk enters it, with its group's luma loads, is kept
//      as the weighted sum of its taps per column (gain_sample_row) and serves the base rows
//      that follow in it: two 24-bit products per source pixel (gain_sample_rows); row r waits
//      in slot r & 1 (the two rows a base row taps are equal or consecutive), as the chroma
//      rows of scale_columns_up do.  The map's sample width is a uniform branch.
//      A code is summed as its parts g >> 8 and g & 255 (gain_scale.hpp): two more planes of
//      32-bit column sums beside the four of the channels, 12 KiB in all.
//   2. lanes along b, the channels spread over the waves, the gain code being a fifth channel
//      with two 64-bit sums; the channels' quotient is k_render_scaled's, the gain code's the
//      two-step quotient of gain_scale.hpp.
// The result tile holds, per output pixel, the packed channels (two dwords) and the averaged
// gain code (a third: 12 + 12 + 12 + 12 + 21 bits do not fit two), 48.75 KiB.  The epilogue runs
// there, where k_render_scaled's XF runs: one gain_px (gain_xform.hpp) per output pixel, the
// alpha encoded by k_render_gain's rules, then store_row.  The image's GainRef (tables, matrix,
// offsets) is read in the epilogue only, field by field: nothing of it is held across the walk.
#include "gain_scale.hpp"
#include "gain_xform.hpp"
#include "kernels.hpp"
#include "render_px.hpp"  // Px, sample_g, scale_acc, store_row

namespace hg {

#if !defined(HG_HOST_EMU)
namespace {

typedef uint32_t GainPair __attribute__((ext_vector_type(2)));
typedef const GainPair __attribute__((address_space(1))) *GainPairs;

// a gain-map row as loaded: the two taps of either of the thread's columns
struct GainMapRow {
    int g[2][2];  // [column][tap]
};

// Stage 1 for one thread: scale_columns (render.hip) with the gain code beside the channels.
// tx: the map's column taps of x0 and x1; wy: the map's row taps, walked with the source rows
// (uniform; its state outlives the call: the next a-line goes on where this one ended).  A map
// row in use is kept as gain_sample_row of its taps, one value per column.
template <typename Pel, int FMT>
__device__ __forceinline__ void gain_scale_columns(const GainScaleDesc &gd, const GainTap (&tx)[2], GainTapWalk &wy, int x0,
                                                   int x1, int ka0, int ka1, uint32_t alo, uint32_t ahi,
                                                   uint32_t (&sum)[2][4], GsCol (&gsum)[2]) {
    constexpr int G = kScaleRowGroup;
    const ScaleDesc &s = gd.s;
    const RenderDesc &d = s.r;
    const int sx = chroma_sx(d.chroma), sy = chroma_sy(d.chroma);
    const uint32_t oa = (uint32_t)s.oa;
    ScaleChroma cc = {{0, 0}, {0, 0}};  // the chroma row in use
    int in_yc = -1;                      // its number
    uint32_t cur[2][2] = {{0, 0}, {0, 0}};  // the map rows in use, by parity: [slot][column]
    int in_row[2] = {-1, -1};               // their numbers
    auto load_row = [&](int yg) {
        GainMapRow r;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (gd.gain_bps == 2) {  // (uniform)
                r.g[c][0] = sample_g<uint16_t>(gd.gain, gd.gain_pitch, tx[c].i0, yg);
                r.g[c][1] = sample_g<uint16_t>(gd.gain, gd.gain_pitch, tx[c].i1, yg);
            } else {
                r.g[c][0] = sample_g<uint8_t>(gd.gain, gd.gain_pitch, tx[c].i0, yg);
                r.g[c][1] = sample_g<uint8_t>(gd.gain, gd.gain_pitch, tx[c].i1, yg);
            }
        }
        return r;
    };
    for (int k0 = ka0; k0 < ka1; k0 += G) {
        int ly[G][2], la[G][2];
        ScaleChroma lc[G];
        bool enter[G];
        GainMapRow lg[G][2];
        bool genter[G][2];
        GainTap ty[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int y = s.ma * min(k0 + g, ka1 - 1) + s.ta;
            ly[g][0] = sample_g<Pel>(d.plane[0], d.pitch[0], x0, y);
            ly[g][1] = sample_g<Pel>(d.plane[0], d.pitch[0], x1, y);
            enter[g] = false;
            lc[g] = ScaleChroma{{0, 0}, {0, 0}};
            if (d.chroma) {
                const int yc = y >> sy;
                enter[g] = yc != in_yc;  // (uniform)
                if (enter[g]) {
                    in_yc = yc;
                    lc[g].cb[0] = sample_g<Pel>(d.plane[1], d.pitch[1], x0 >> sx, yc);
                    lc[g].cr[0] = sample_g<Pel>(d.plane[2], d.pitch[2], x0 >> sx, yc);
                    if (!sx) {
                        lc[g].cb[1] = sample_g<Pel>(d.plane[1], d.pitch[1], x1, yc);
                        lc[g].cr[1] = sample_g<Pel>(d.plane[2], d.pitch[2], x1, yc);
                    }
                }
            }
            gain_walk_seek(wy, y, gd.h, gd.hg, gd.inv_h);  // (uniform; a step, but for the walk's first row)
            ty[g] = gain_tap_of(wy.q, gd.hg);
            genter[g][0] = genter[g][1] = false;
            lg[g][0] = lg[g][1] = GainMapRow{};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int yg = e ? ty[g].i1 : ty[g].i0;
#pragma unroll
                for (int slot = 0; slot < 2; ++slot)  // (constant indices: nothing goes to scratch)
                    if ((yg & 1) == slot && yg != in_row[slot]) {  // (uniform)
                        in_row[slot] = yg;
                        genter[g][slot] = true;
                        lg[g][slot] = load_row(yg);
                    }
            }
            la[g][0] = la[g][1] = 0;
            if ((FMT & 1) && d.alpha) {
                if (d.alpha_bps == 2) {
                    la[g][0] = sample_g<uint16_t>(d.alpha, d.alpha_pitch, x0, y);
                    la[g][1] = sample_g<uint16_t>(d.alpha, d.alpha_pitch, x1, y);
                } else {
                    la[g][0] = sample_g<uint8_t>(d.alpha, d.alpha_pitch, x0, y);
                    la[g][1] = sample_g<uint8_t>(d.alpha, d.alpha_pitch, x1, y);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int k = k0 + g;
            if (k >= ka1) break;  // (uniform; the repeated rows past the end were loaded for nothing)
            if (enter[g]) cc = lc[g];
#pragma unroll
            for (int slot = 0; slot < 2; ++slot)
                if (genter[g][slot]) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        cur[slot][c] = gain_sample_row((uint32_t)lg[g][slot].g[c][0], (uint32_t)lg[g][slot].g[c][1],
                                                       (uint32_t)tx[c].f);
                }
            const uint32_t w = gs_weight((uint32_t)k, oa, alo, ahi);
            scale_acc<FMT>(d, ly[g], cc, la[g], w, sum);
            const bool odd0 = ty[g].i0 & 1, odd1 = ty[g].i1 & 1;  // (uniform)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t gq = gain_sample_rows(odd0 ? cur[1][c] : cur[0][c], odd1 ? cur[1][c] : cur[0][c],
                                                     (uint32_t)ty[g].f);
                gs_col_add(gsum[c], w, min(gq, gd.gmax));
            }
        }
    }
}

// HF: GAIN_* (bit 0 alpha, bit 1 PQ)
template <typename Pel, int HF>
__global__ void __launch_bounds__(256) k_render_gain_scaled(const GainScaleDesc *__restrict__ descs) {
    constexpr int FMT = (HF & 1) ? RENDER_RGBA16 : RENDER_RGB16;
    constexpr int NCH = (HF & 1) ? 4 : 3;
    constexpr int CG = 4;                               // the gain code's channel number in stage 2
    constexpr int RES = kScaleTile * (kScaleTile + 1);  // dwords: 64 lines of pitch 65 (>= 8 lines of pitch 256)
    __shared__ uint32_t colsum[6 * kScaleCols];         // R, G, B, A, then the two parts of the gain code
    __shared__ uint32_t res[3 * RES];                   // Px lo, Px hi, the gain code
    // (read where it lies, through scalar loads: a copy of its 68 dwords up front spills a quarter more SGPRs)
    const GainScaleDesc &gd = descs[blockIdx.y];
    const ScaleDesc &s = gd.s;
    const RenderDesc &d = s.r;
    if ((int)blockIdx.x >= d.tiles) return;  // (a smaller image of the batch: the whole workgroup leaves)
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int a0 = ((int)blockIdx.x / d.tiles_x) * s.na, b0 = ((int)blockIdx.x % d.tiles_x) * s.nb;
    const int a1 = min(a0 + s.na, s.oa), b1 = min(b0 + s.nb, s.ob);
    const uint32_t ca = (uint32_t)s.ca, cb = (uint32_t)s.cb, oa = (uint32_t)s.oa, ob = (uint32_t)s.ob;
    const int lp = d.swap ? kScaleTile + 1 : 256;  // pitch of the result tile in dwords
    // the tile's footprint along b: window indices [kb0, kb1), source columns [xmin, xmax)
    // (products of two sides stay below 2^32: every side is at most 65535)
    const int kb0 = (int)((uint32_t)b0 * cb / ob), kb1 = (int)(((uint32_t)b1 * cb + ob - 1) / ob);
    const int xmin = s.mb > 0 ? s.tb + kb0 : s.tb - (kb1 - 1);
    const int xmax = s.mb > 0 ? s.tb + kb1 : s.tb - kb0 + 1;
    // stage 2: this thread's output line along b and its channels c0, c0 + cstep, ... of R, G, B, A, gain
    const int bl = t & (s.nb - 1), c0 = t >> s.nb_log2, cstep = 256 >> s.nb_log2;
    const bool bvalid = b0 + bl < b1;
    const uint32_t blo = (uint32_t)(b0 + bl) * cb, bhi = blo + cb;  // its interval on the grid of 1 / (ob * cb)
    const int kl = bvalid ? (int)(blo / ob) : 0, kh = bvalid ? (int)((bhi + ob - 1) / ob) : 0;

    // the map's column taps of this thread's two columns in the first chunk (all there is, unless the
    // tile's footprint is wider than a chunk), and the walk of the map's row taps down the source rows
    const int xs0 = xmin & ~1;
    GainTap tx0[2];
    {
        const int x0 = xs0 + 2 * t, x0c = min(max(x0, xmin), xmax - 1), x1c = min(max(x0 + 1, xmin), xmax - 1);
        tx0[0] = gain_tap(x0c, gd.w, gd.wg, gd.inv_w);
        tx0[1] = gain_tap(x1c, gd.w, gd.wg, gd.inv_w);
    }
    GainTapWalk wy;
    gain_walk_start(wy, s.ma * (int)((uint32_t)a0 * ca / oa) + s.ta, gd.h, gd.hg, gd.inv_h);

    for (int a = a0; a < a1; ++a) {
        const uint32_t alo = (uint32_t)a * ca, ahi = alo + ca;
        const int ka0 = (int)(alo / oa), ka1 = (int)((ahi + oa - 1) / oa);
        uint64_t acc[5] = {0, 0, 0, 0, 0};
        uint64_t accl = 0;  // the gain code's low part (one of the thread's channels at most is the gain code)
        for (int xs = xmin & ~1; xs < xmax; xs += kScaleCols) {
            const int x0 = xs + 2 * t;
            if (x0 < xmax) {
                // a column outside the footprint repeats its neighbour and is never read back
                const int x0c = max(x0, xmin), x1c = min(x0 + 1, xmax - 1);
                uint32_t sum[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
                GsCol gsum[2] = {{0, 0}, {0, 0}};
                GainTap tx[2] = {tx0[0], tx0[1]};
                if (xs != xs0) {  // (uniform)
                    tx[0] = gain_tap(x0c, gd.w, gd.wg, gd.inv_w);
                    tx[1] = gain_tap(x1c, gd.w, gd.wg, gd.inv_w);
                }
                gain_scale_columns<Pel, FMT>(gd, tx, wy, x0c, x1c, ka0, ka1, alo, ahi, sum, gsum);
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    reinterpret_cast<uint2 *>(colsum + c * kScaleCols)[t] = make_uint2(sum[0][c], sum[1][c]);
                reinterpret_cast<uint2 *>(colsum + 4 * kScaleCols)[t] = make_uint2(gsum[0].hi, gsum[1].hi);
                reinterpret_cast<uint2 *>(colsum + 5 * kScaleCols)[t] = make_uint2(gsum[0].lo, gsum[1].lo);
            }
            __syncthreads();
            if (bvalid) {
                // the chunk's columns as window indices: [kc, kc + 512)
                const int kc = s.mb > 0 ? xs - s.tb : s.tb - xs - (kScaleCols - 1);
                const int k_lo = max(kl, kc), k_hi = min(kh, kc + kScaleCols);
                for (int k = k_lo; k < k_hi; ++k) {
                    const uint32_t w = gs_weight((uint32_t)k, ob, blo, bhi);
                    const int idx = s.mb * k + s.tb - xs;
#pragma unroll
                    for (int ci = 0; ci < 5; ++ci) {
                        const int c = c0 + ci * cstep;
                        if (c < NCH) {
                            acc[ci] += (uint64_t)w * colsum[c * kScaleCols + idx];
                        } else if (c == CG) {
                            acc[ci] += (uint64_t)w * colsum[4 * kScaleCols + idx];
                            accl += (uint64_t)w * colsum[5 * kScaleCols + idx];
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (bvalid) {
            const int at = (a - a0) * lp + bl;
#pragma unroll
            for (int ci = 0; ci < 5; ++ci) {
                const int c = c0 + ci * cstep;
                if (c > CG) continue;
                if (c == CG) {
                    const GsSum gs = {acc[ci], accl};
                    res[2 * RES + at] = gs_average(gs, s.den, s.inv_den);
                } else {
                    // (the RGB formats keep a zero where alpha would be: store_row packs over it)
                    const uint32_t q = c < NCH ? gs_average_small(acc[ci], s.den, s.inv_den) : 0;
                    reinterpret_cast<uint16_t *>(res)[2 * ((c >> 1) * RES + at) + (c & 1)] = (uint16_t)q;
                }
            }
        }
    }
    __syncthreads();
    {
        // the HDR formula on the tile's averages, in place in the result tile
        const GainRef &g = reinterpret_cast<const GainRef *>(descs + gridDim.y)[blockIdx.y];
        GainParams gp;
#pragma unroll
        for (int k = 0; k < 9; ++k) gp.m[k] = g.m[k];
        gp.k_b = g.k_b, gp.k_a = g.k_a;
        gp.encoding = (HF & 2) ? GAIN_ENC_PQ : GAIN_ENC_LINEAR;
        const uint64_t lut = g.lut;
        const int n = g.n;
        const XfLut in = (XfLut)lut;
        const XfTonePairs<GainPairs> T{(GainPairs)(lut + (uint64_t)g.t_off)}, E{(GainPairs)(lut + (uint64_t)g.e_off)};
        const int32_t alpha_shift = g.alpha_shift, maxp = g.maxp;
        const float alpha_scale = g.alpha_scale;
        const int nbv = b1 - b0, cnt = (a1 - a0) * nbv;
        for (int idx = t; idx < cnt; idx += 256) {
            const int al = idx / nbv, at = al * lp + (idx - al * nbv);
            const uint32_t lo = res[at], hi = res[RES + at];
            uint32_t R = lo & 0xffffu, G = lo >> 16, B = hi & 0xffffu, A = hi >> 16;
            gain_px(in, n, T, E, gp, res[2 * RES + at], R, G, B);
            if (HF & 1) {
                if (HF & 2) A = !d.alpha ? (uint32_t)maxp : alpha_shift >= 0 ? A >> alpha_shift : A << -alpha_shift;
                else A = !d.alpha ? 0x3c00u : gain_encode_linear(A, alpha_scale);  // (binary16 1.0 for an opaque pixel)
            }
            res[at] = R | (G << 16);
            res[RES + at] = B | (A << 16);
        }
        __syncthreads();
    }
    // write: lanes along the output's x, 64 pixels of a row per wave and step
    const Px none = {0, 0};
    if (!d.swap) {
        const int segs = s.nb >> 6;
        for (int u = wave; u < (a1 - a0) * segs; u += 4) {
            const int al = u / segs, oxw = b0 + (u % segs) * 64;
            if (oxw >= d.out_w) continue;
            const uint32_t *line = res + al * lp + (oxw - b0);
            const bool valid = oxw + lane < d.out_w;
            Px p = none;
            if (valid) p = {line[lane], line[RES + lane]};
            store_row<FMT>(d, a0 + al, oxw, lane, p, valid);
        }
    } else {
        const bool valid = a0 + lane < d.out_w;
        for (int oy = b0 + wave; oy < b1; oy += 4) {
            const uint32_t *col = res + (oy - b0);
            Px p = none;
            if (valid) p = {col[lane * lp], col[RES + lane * lp]};
            store_row<FMT>(d, oy, a0, lane, p, valid);
        }
    }
}

template <typename Pel>
void launch_gain_scaled_fmt(const GainScaleDesc *descs, dim3 grid, int format, hipStream_t s) {
    switch (format) {
    case GAIN_RGB16F: hipLaunchKernelGGL((k_render_gain_scaled<Pel, GAIN_RGB16F>), grid, dim3(256), 0, s, descs); break;
    case GAIN_RGBA16F: hipLaunchKernelGGL((k_render_gain_scaled<Pel, GAIN_RGBA16F>), grid, dim3(256), 0, s, descs); break;
    case GAIN_RGB16PQ: hipLaunchKernelGGL((k_render_gain_scaled<Pel, GAIN_RGB16PQ>), grid, dim3(256), 0, s, descs); break;
    default: hipLaunchKernelGGL((k_render_gain_scaled<Pel, GAIN_RGBA16PQ>), grid, dim3(256), 0, s, descs); break;
    }
}

}  // namespace

hipError_t launch_render_gain_scaled(const GainScaleDesc *descs, int n_images, int max_tiles, int format,
                                     int bytes_per_sample, hipStream_t s) {
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_gain_scaled_fmt<uint8_t>(descs, grid, format, s);
    else launch_gain_scaled_fmt<uint16_t>(descs, grid, format, s);
    return hipGetLastError();
}
#endif

}  // namespace hg
