// render.hip — k_render: a batch of decoded images → display-ready interleaved
// RGB(A), 8 or 16 bits per sample, in one launch (heifgpu_render_batch).
//
// Every image brings a RenderDesc: its planes, its output surface and the
// folded map of its clap / irot / imir properties, output pixel → decoded
// sample (one of the eight signed permutations plus a translation).  The
// kernel knows that one general case and nothing about box order.  The
// arithmetic is color.hip's (H.273 in 16.16 fixed point, round half up, clip,
// chroma by replication), at 8 bits for the 8-bit formats and at the image's
// own depth for the 16-bit ones; at 12 bits the largest sum, ys * 4095 +
// cr_r * 2048 + 32768 < 2^30, still fits int32.  Chroma is addressed from the
// absolute source position, so an odd clap offset keeps the right phase.
//
// Mapping: grid (tile, image), 256 threads, one pixel per lane, lanes along
// the source's x when reading and along the output's x when writing:
// - maps that keep the axes (identity, mirrors, 180 degrees): a workgroup
//   takes 256 x 16 output pixels, a wave 64 pixels of a row at a time; a
//   mirrored row is read backwards inside the same cache lines;
// - maps that swap them (90, 270 degrees, the transposes): a workgroup takes
//   64 x 64 output pixels, converts them with lanes along the output's y (the
//   source's x) into an LDS tile of packed pixels, and writes them with lanes
//   along the output's x.  The tile's pitch is 65 dwords: both the row-wise
//   write and the column-wise read touch 32 different banks per 32 lanes (at
//   64 the read would hit one bank 32 times).
// RGB8 keeps color.hip's packing, 4 pixels → 3 dwords: a lane fetches its
// right neighbour's pixel across the wave and lanes 0..2 of every four store
// one dword each (bytes when the row is not 4-byte aligned or the four are
// incomplete).  RGB16 packs 2 pixels → 3 dwords the same way; RGBA stores its
// own 4 or 8 bytes.
//
// k_render_scaled (heifgpu_render_batch_scaled), further down, writes the exact
// area average of a window of the same picture onto another grid; it shares
// convert()'s arithmetic and store_row.  With a TensorDesc the same kernel ends in
// store_tensor instead (heifgpu_render_batch_tensor): the same integers, scaled
// and biased per channel, as f32 / f16 / bf16, planar or interleaved.
//
// The colour-managed calls (heifgpu_render_batch_color and its kin) run the same
// bodies compiled with XF: a ColorRef per image names the transform's tables in
// device memory (out_lut as pairs: six gathers per pixel), and color_xform_px
// (color_xform.hpp) turns every RGB triple
// into the destination space: behind convert() in k_render, on the rounded
// averages in the result tile of k_render_scaled, before either store.  The
// tables are read where they lie (global loads that the L1 / L2 serve, out of
// 17.5 KiB at 8 bits, 40 KiB at 12), not staged
// through LDS: k_render's axis-keeping path has no barrier to stage behind, and
// the 16-bit formats already sit at the LDS occupancy limit.  The unmanaged
// kernels are the XF = false instantiations under their old names and arguments.
//
// The HDR render adds one more bit, kRenderTone: the instantiations that a call launches
// when one of its images has a tone transform (ColorRef::tone; include/heifgpu.h "HDR
// render").  Such an image's RGB triples go through color_tone_px (wide input table,
// luminance, one 8-byte gather of the gain pair, three 64-bit products, then the same
// matrix and out_lut); the others of the batch take the managed or unmanaged path by a
// uniform branch.  Those instantiations are compiled from this file as render_tone.hip.
//
// Bilinear chroma upsampling adds a third bit, kRenderChromaUp: the instantiations (with
// all three bits, render_chroma.hip) that a call launches when one of its images is set to
// it.  A ChromaRef per image follows the ColorRefs; for such an image (a uniform branch)
// convert() forms C' from the clamped 2 x 2 neighbourhood of Cb and of Cr (chroma_up.hpp)
// in place of the one replicated sample, and k_render_scaled walks its columns with
// scale_columns_up; everything behind that is unchanged.
//
// The linear-light scaled render adds a fourth bit, kRenderLinear, read by k_render_scaled
// only: the instantiations (kRenderXf | kRenderLinear | kRenderChromaUp, render_linear.hip)
// that heifgpu_render_batch_scaled_linear and _tensor_linear launch whatever the batch's mix.
// Stage 1 sends every clipped R, G, B through the image's in_lut before the weighted add (three
// table reads per source sample; alpha not), the quotients are 16-bit levels in the wide tile
// layout for every format, and the pass behind them runs the matrix and out_lut and packs the
// codes as the stores read them (include/heifgpu.h "Linear-light scaled render").
#include <type_traits>

// where the linear instantiations read in_lut in stage 1: LDS (1) or global gathers (0); both
// staged, as measured on the MI355X
#if !defined(HG_LIN_LDS8)
#define HG_LIN_LDS8 1
#endif
#if !defined(HG_LIN_LDS16)
#define HG_LIN_LDS16 1
#endif

#include "color_xform.hpp"
#include "kernels.hpp"
#include "render_px.hpp"  // Px, convert, xform_rgb, store_row, store_tensor (shared with resample.hip)

namespace hg {

#if !defined(HG_HOST_EMU)
namespace {

// FMTX: the pixel format, plus kRenderXf for the colour-managed instantiations, whose
// ColorRefs lie behind the call's gridDim.y descriptors
template <typename Pel, int FMTX>
__global__ void __launch_bounds__(256) k_render(const RenderDesc *descs) {
    constexpr int FMT = FMTX & 3;
    constexpr bool XF = (FMTX & kRenderXf) != 0;
    constexpr bool TONE = (FMTX & kRenderTone) != 0;  // (with XF: an image's ColorRef may carry a tone stage)
    constexpr bool CUP = (FMTX & kRenderChromaUp) != 0;  // (with XF: a ChromaRef per image behind the ColorRefs)
    constexpr bool WIDE = FMT >= RENDER_RGB16;
    constexpr int T = kRenderTile, LP = kRenderTile + 1;  // LDS pitch in dwords: 65, not 64 (bank conflicts)
    __shared__ uint32_t tile_lds[(WIDE ? 2 : 1) * T * LP];
    const RenderDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x >= d.tiles) return;  // (a smaller image of the batch: the whole workgroup leaves)
    ColorRef x{};
    if constexpr (XF) x = reinterpret_cast<const ColorRef *>(descs + gridDim.y)[blockIdx.y];
    const uint16_t *staged = nullptr;
#if defined(HG_XF_LDS)
    // the A/B of DESIGN 5.25: every workgroup copies its image's tables (1.5 + 16 KiB at 8 bits,
    // 24 + 16 KiB at 12) into LDS first and reads them there
    __shared__ uint32_t xf_lds[XF ? (3 * (WIDE ? 4096 : 256)) / 2 + kXfPairEntries : 1];
    if constexpr (XF) {
        if (x.lut) {  // (uniform)
            const uint32_t __attribute__((address_space(1))) *src = (const uint32_t __attribute__((address_space(1))) *)x.lut;
            for (int i = (int)threadIdx.x; i < 3 * x.n / 2 + kXfPairEntries; i += 256) xf_lds[i] = src[i];
            __syncthreads();
            staged = reinterpret_cast<const uint16_t *>(xf_lds);
        }
    }
#endif
    const ToneW tw = tone_weights<TONE>(x);
    const ChromaRef cu = chroma_ref_of<CUP>(descs);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int tx = (int)blockIdx.x % d.tiles_x, ty = (int)blockIdx.x / d.tiles_x;
    const Px none = {0, 0};
    if (!d.swap) {
        const int oxw = tx * kRenderRowW + wave * 64, ox = oxw + lane;
        if (oxw >= d.out_w) return;  // (no barrier on this path)
        const bool valid = ox < d.out_w;
        for (int r = 0; r < kRenderRowH; ++r) {
            const int oy = ty * kRenderRowH + r;
            if (oy >= d.out_h) break;
            Px p = valid ? convert<Pel, FMT, CUP>(d, ox, oy, cu) : none;
            if constexpr (XF) {
                if (x.lut) xform_pixel<FMT, TONE>(x, p, staged, tw);  // (uniform: the image's transform, or none)
            }
            store_row<FMT>(d, oy, oxw, lane, p, valid);
        }
        return;
    }
    const int ox0 = tx * T, oy0 = ty * T;
    // convert: lanes along the output's y, which is the source's x
    for (int i = 0; i < T / 4; ++i) {
        const int oxl = wave * (T / 4) + i, ox = ox0 + oxl, oy = oy0 + lane;
        if (ox < d.out_w && oy < d.out_h) {
            Px p = convert<Pel, FMT, CUP>(d, ox, oy, cu);
            if constexpr (XF) {
                if (x.lut) xform_pixel<FMT, TONE>(x, p, staged, tw);
            }
            tile_lds[oxl * LP + lane] = p.lo;
            if (WIDE) tile_lds[T * LP + oxl * LP + lane] = p.hi;
        }
    }
    __syncthreads();
    // write: lanes along the output's x
    const bool valid = ox0 + lane < d.out_w;
    for (int i = 0; i < T / 4; ++i) {
        const int oyl = wave * (T / 4) + i, oy = oy0 + oyl;
        if (oy >= d.out_h) break;
        Px p = none;
        if (valid) {
            p.lo = tile_lds[lane * LP + oyl];
            if (WIDE) p.hi = tile_lds[T * LP + lane * LP + oyl];
        }
        store_row<FMT>(d, oy, ox0, lane, p, valid);
    }
}

// XF: kRenderXf for the colour-managed instantiations, else 0
template <typename Pel, int XF>
void launch_fmt(const RenderDesc *descs, dim3 grid, int format, hipStream_t s) {
    switch (format) {
    case RENDER_RGB8: hipLaunchKernelGGL((k_render<Pel, RENDER_RGB8 | XF>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGBA8: hipLaunchKernelGGL((k_render<Pel, RENDER_RGBA8 | XF>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGB16: hipLaunchKernelGGL((k_render<Pel, RENDER_RGB16 | XF>), grid, dim3(256), 0, s, descs); break;
    default: hipLaunchKernelGGL((k_render<Pel, RENDER_RGBA16 | XF>), grid, dim3(256), 0, s, descs); break;
    }
}

// ---- k_render_scaled: the same pictures, area-averaged onto a smaller (or any
// other) grid in the same launch (heifgpu_render_batch_scaled) -----------------
// R = round_half_up(sum_j sum_i wy(Y,j) wx(X,i) D[j][i] / (cw ch)) over the
// converted pixels D of the window (include/heifgpu.h states the weights), all
// in integers.  The sum is separable and is taken in the source's axes, so the
// same code serves the eight orientations: axis a is the output axis the
// source's y runs along, axis b the one its x runs along (ScaleDesc).
//
// A workgroup (256 threads) owns na x nb output pixels: 8 rows x 64 / 128 / 256
// columns for maps that keep the axes, 64 columns x 16 / 32 / 64 rows for maps
// that swap them (nb picked by the host so that the tile's footprint along b
// comes close to one chunk below; store_row wants 64 pixels along the output's x).  For every a-line of its tile it walks the line's source footprint in
// chunks of 512 source columns:
//   1. lanes along the source's x, two adjacent columns (one 4:2:0 / 4:2:2
//      chroma sample) per thread, mirrored or not: a thread walks its columns
//      down the line's source rows, converts each sample with convert()'s
//      arithmetic and adds weight_a * channel into 32-bit sums (at most
//      65535 * 4095).  The loads of four rows are issued before the first is
//      used; a chroma row is fetched once for the luma rows it serves.  The
//      sums go to LDS, one plane of 512 dwords per channel.
//   2. lanes along b, the channels spread over the waves: an output pixel adds
//      weight_b * column sum over its columns of the chunk into a 64-bit sum
//      kept across chunks (the whole sum reaches 4095 * cw * ch > 2^32).
// Both footprints are walked by loops, so LDS (8 KiB of column sums, 16.25 or
// 32.5 KiB of results) does not depend on the ratio.  The rounded quotient
// comes from a double-precision estimate corrected exactly in integers.  The
// tile's pixels wait in LDS, packed as Px, and leave through store_row with
// lanes along the output's x (for swapped axes that read is the transpose,
// pitch 65 dwords as in k_render).
// (kScaleRowGroup, ScaleChroma and scale_acc, convert()'s arithmetic for a thread's two columns, are in
// render_px.hpp: k_render_gain_scaled walks its columns with them too)

// Stage 1 for one thread: its two source columns x0, x1 down the window rows [ka0, ka1)
// of output line a, weighted.  The loads of kScaleRowGroup rows are issued before the
// first of them is used (rows past the end load the last one again and are skipped); a chroma
// row is loaded when the walk enters it and serves the luma rows that follow in it.
// (LIN, lin: scale_acc's, for the kRenderLinear instantiations)
template <typename Pel, int FMT, bool LIN = false, typename Lin = NoLin>
__device__ __forceinline__ void scale_columns(const ScaleDesc &s, int x0, int x1, int ka0, int ka1, uint32_t alo,
                                              uint32_t ahi, uint32_t (&sum)[2][4], const Lin &lin = Lin{}) {
    constexpr int G = kScaleRowGroup;
    const RenderDesc &d = s.r;
    const int sx = chroma_sx(d.chroma), sy = chroma_sy(d.chroma);
    const uint32_t oa = (uint32_t)s.oa;
    ScaleChroma cc = {{0, 0}, {0, 0}};  // the chroma row in use
    int in_yc = -1;                      // its number
    for (int k0 = ka0; k0 < ka1; k0 += G) {
        int ly[G][2], la[G][2];
        ScaleChroma lc[G];
        bool enter[G];
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
            const uint32_t w = min((uint32_t)(k + 1) * oa, ahi) - max((uint32_t)k * oa, alo);
            scale_acc<FMT, false, LIN>(d, ly[g], cc, la[g], w, sum, lin);
        }
    }
}

// scale_columns for an image with bilinear chroma upsampling (cu.mode != 0).  A chroma row
// in use holds, per plane, the two taps of either luma column (neighbouring columns share
// samples: up to three different ones); row r waits in slot r & 1, and the two rows a
// luma row taps are equal or consecutive, so they never share a slot.  A row is loaded
// when the walk first needs it, with its group's luma loads; C' is formed and rounded per
// luma sample in front of scale_acc's products.
struct ScaleChromaRow {
    int cb[2][2], cr[2][2];  // [column][tap], as loaded
};

template <typename Pel, int FMT, bool LIN = false, typename Lin = NoLin>
__device__ __forceinline__ void scale_columns_up(const ScaleDesc &s, const ChromaRef &cu, int x0, int x1, int ka0, int ka1,
                                                 uint32_t alo, uint32_t ahi, uint32_t (&sum)[2][4], const Lin &lin = Lin{}) {
    constexpr int G = kScaleRowGroup;
    const RenderDesc &d = s.r;
    const uint32_t oa = (uint32_t)s.oa;
    const ChromaTap tx[2] = {chroma_tap(x0, cu.px, cu.wc), chroma_tap(x1, cu.px, cu.wc)};
    ScaleChromaRow cur[2] = {};     // the chroma rows in use, by parity
    int in_row[2] = {-1, -1};       // their numbers
    auto load_row = [&](int yc) {
        ScaleChromaRow r;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            r.cb[c][0] = sample_g<Pel>(d.plane[1], d.pitch[1], tx[c].i0, yc);
            r.cb[c][1] = sample_g<Pel>(d.plane[1], d.pitch[1], tx[c].i1, yc);
            r.cr[c][0] = sample_g<Pel>(d.plane[2], d.pitch[2], tx[c].i0, yc);
            r.cr[c][1] = sample_g<Pel>(d.plane[2], d.pitch[2], tx[c].i1, yc);
        }
        return r;
    };
    for (int k0 = ka0; k0 < ka1; k0 += G) {
        int ly[G][2], la[G][2];
        ScaleChromaRow lc[G][2];
        bool enter[G][2];
        ChromaTap ty[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int y = s.ma * min(k0 + g, ka1 - 1) + s.ta;
            ly[g][0] = sample_g<Pel>(d.plane[0], d.pitch[0], x0, y);
            ly[g][1] = sample_g<Pel>(d.plane[0], d.pitch[0], x1, y);
            ty[g] = chroma_tap(y, cu.py, cu.hc);
            enter[g][0] = enter[g][1] = false;
            lc[g][0] = lc[g][1] = ScaleChromaRow{};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int yc = e ? ty[g].i1 : ty[g].i0;
#pragma unroll
                for (int slot = 0; slot < 2; ++slot)  // (constant indices: nothing goes to scratch)
                    if ((yc & 1) == slot && yc != in_row[slot]) {  // (uniform)
                        in_row[slot] = yc;
                        enter[g][slot] = true;
                        lc[g][slot] = load_row(yc);
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
            if (enter[g][0]) cur[0] = lc[g][0];
            if (enter[g][1]) cur[1] = lc[g][1];
            const ScaleChromaRow r0 = (ty[g].i0 & 1) ? cur[1] : cur[0], r1 = (ty[g].i1 & 1) ? cur[1] : cur[0];
            ScaleChroma cc;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                cc.cb[c] = chroma_value(r0.cb[c][0], r0.cb[c][1], r1.cb[c][0], r1.cb[c][1], tx[c], ty[g]);
                cc.cr[c] = chroma_value(r0.cr[c][0], r0.cr[c][1], r1.cr[c][0], r1.cr[c][1], tx[c], ty[g]);
            }
            const uint32_t w = min((uint32_t)(k + 1) * oa, ahi) - max((uint32_t)k * oa, alo);
            scale_acc<FMT, true, LIN>(d, ly[g], cc, la[g], w, sum, lin);
        }
    }
}

__device__ __forceinline__ const ScaleDesc &scale_of(const ScaleDesc &s) { return s; }
__device__ __forceinline__ const ScaleDesc &scale_of(const TensorDesc &t) { return t.s; }

template <typename Pel, int FMTX, typename Desc>
__global__ void __launch_bounds__(256) k_render_scaled(const Desc *descs) {
    constexpr int FMT = FMTX & 3;
    constexpr bool XF = (FMTX & kRenderXf) != 0;  // (as k_render's)
    constexpr bool TONE = (FMTX & kRenderTone) != 0;
    constexpr bool CUP = (FMTX & kRenderChromaUp) != 0;
    constexpr bool TENSOR = std::is_same<Desc, TensorDesc>::value;  // (else ScaleDesc: the integer surfaces)
    constexpr bool WIDE = FMT >= RENDER_RGB16;
    // the linear-light instantiations (render_linear.hip): stage 1 sums in_lut's levels, the
    // quotients are 16-bit levels for every format (WRES: two dwords per pixel in the result
    // tile), and the pass behind them encodes into the format's own layout
    constexpr bool LIN = (FMTX & kRenderLinear) != 0;
    constexpr bool WRES = WIDE || LIN;
    // in_lut staged into LDS (HG_LIN_LDS8: the 1.5 KiB of the 8-bit formats; HG_LIN_LDS16: the 6 to
    // 24 KiB of the 16-bit ones) or gathered where it lies in global memory; DESIGN 5.38 has the A/B
    constexpr bool STAGE = LIN && (WIDE ? HG_LIN_LDS16 != 0 : HG_LIN_LDS8 != 0);
    constexpr int NCH = (FMT & 1) ? 4 : 3;
    constexpr int RES = kScaleTile * (kScaleTile + 1);  // dwords: 64 lines of pitch 65 (>= 8 lines of pitch 256)
    __shared__ uint32_t colsum[4 * kScaleCols];
    __shared__ uint32_t res[(WRES ? 2 : 1) * RES];
    const Desc dd = descs[blockIdx.y];
    const ScaleDesc &s = scale_of(dd);
    const RenderDesc &d = s.r;
    if ((int)blockIdx.x >= d.tiles) return;  // (a smaller image of the batch: the whole workgroup leaves)
    const ChromaRef cu = chroma_ref_of<CUP>(descs);
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    // a linear call's ColorRef always has a table (an identity transform is applied here)
    ColorRef lx{};
    if constexpr (LIN) lx = reinterpret_cast<const ColorRef *>(descs + gridDim.y)[blockIdx.y];
    __shared__ uint32_t lin_lds[STAGE ? 3 * (WIDE ? 4096 : 256) / 2 : 1];
    if constexpr (STAGE) {
        // once per workgroup, before the first a-line: 3 * n entries of 16 bits, n a multiple of 256
        const uint32_t __attribute__((address_space(1))) *src = (const uint32_t __attribute__((address_space(1))) *)lx.lut;
        for (int i = t; i < 3 * lx.n / 2; i += 256) lin_lds[i] = src[i];
        __syncthreads();
    }
    const int a0 = ((int)blockIdx.x / d.tiles_x) * s.na, b0 = ((int)blockIdx.x % d.tiles_x) * s.nb;
    const int a1 = min(a0 + s.na, s.oa), b1 = min(b0 + s.nb, s.ob);
    const uint32_t ca = (uint32_t)s.ca, cb = (uint32_t)s.cb, oa = (uint32_t)s.oa, ob = (uint32_t)s.ob;
    const int lp = d.swap ? kScaleTile + 1 : 256;  // pitch of the result tile in dwords
    // the tile's footprint along b: window indices [kb0, kb1), source columns [xmin, xmax)
    // (products of two sides stay below 2^32: every side is at most 65535)
    const int kb0 = (int)((uint32_t)b0 * cb / ob), kb1 = (int)(((uint32_t)b1 * cb + ob - 1) / ob);
    const int xmin = s.mb > 0 ? s.tb + kb0 : s.tb - (kb1 - 1);
    const int xmax = s.mb > 0 ? s.tb + kb1 : s.tb - kb0 + 1;
    // stage 2: this thread's output line along b and its channels c0, c0 + cstep, ...
    const int bl = t & (s.nb - 1), c0 = t >> s.nb_log2, cstep = 256 >> s.nb_log2;
    const bool bvalid = b0 + bl < b1;
    const uint32_t blo = (uint32_t)(b0 + bl) * cb, bhi = blo + cb;  // its interval on the grid of 1 / (ob * cb)
    const int kl = bvalid ? (int)(blo / ob) : 0, kh = bvalid ? (int)((bhi + ob - 1) / ob) : 0;

    for (int a = a0; a < a1; ++a) {
        const uint32_t alo = (uint32_t)a * ca, ahi = alo + ca;
        const int ka0 = (int)(alo / oa), ka1 = (int)((ahi + oa - 1) / oa);
        uint64_t acc[4] = {0, 0, 0, 0};
        for (int xs = xmin & ~1; xs < xmax; xs += kScaleCols) {
            const int x0 = xs + 2 * t;
            if (x0 < xmax) {
                // a column outside the footprint repeats its neighbour and is never read back
                const int x0c = max(x0, xmin), x1c = min(x0 + 1, xmax - 1);
                uint32_t sum[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
                bool up = false;
                if constexpr (CUP) up = cu.mode != 0;  // (uniform)
                if constexpr (STAGE) {
                    const LinLut<const uint16_t *> lin{reinterpret_cast<const uint16_t *>(lin_lds), lx.n};
                    if (up) scale_columns_up<Pel, FMT, true>(s, cu, x0c, x1c, ka0, ka1, alo, ahi, sum, lin);
                    else scale_columns<Pel, FMT, true>(s, x0c, x1c, ka0, ka1, alo, ahi, sum, lin);
                } else if constexpr (LIN) {
                    const LinLut<XfLut> lin{(XfLut)lx.lut, lx.n};
                    if (up) scale_columns_up<Pel, FMT, true>(s, cu, x0c, x1c, ka0, ka1, alo, ahi, sum, lin);
                    else scale_columns<Pel, FMT, true>(s, x0c, x1c, ka0, ka1, alo, ahi, sum, lin);
                } else {
                    if (up) scale_columns_up<Pel, FMT>(s, cu, x0c, x1c, ka0, ka1, alo, ahi, sum);
                    else scale_columns<Pel, FMT>(s, x0c, x1c, ka0, ka1, alo, ahi, sum);
                }
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    reinterpret_cast<uint2 *>(colsum + c * kScaleCols)[t] = make_uint2(sum[0][c], sum[1][c]);
            }
            __syncthreads();
            if (bvalid) {
                // the chunk's columns as window indices: [kc, kc + 512)
                const int kc = s.mb > 0 ? xs - s.tb : s.tb - xs - (kScaleCols - 1);
                const int k_lo = max(kl, kc), k_hi = min(kh, kc + kScaleCols);
                for (int k = k_lo; k < k_hi; ++k) {
                    const uint32_t w = min((uint32_t)(k + 1) * ob, bhi) - max((uint32_t)k * ob, blo);
                    const int idx = s.mb * k + s.tb - xs;
#pragma unroll
                    for (int ci = 0; ci < 4; ++ci) {
                        const int c = c0 + ci * cstep;
                        if (c < NCH) acc[ci] += (uint64_t)w * colsum[c * kScaleCols + idx];
                    }
                }
            }
            __syncthreads();
        }
        if (bvalid) {
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                const int c = c0 + ci * cstep;
                if (c >= 4) continue;
                uint32_t q = 0;  // (the RGB formats keep a zero where alpha would be: store_row packs over it)
                if (c < NCH) {
                    const uint64_t num = 2 * acc[ci] + (s.den >> 1);
                    q = (uint32_t)((double)num * s.inv_den);
                    const int64_t rem = (int64_t)(num - (uint64_t)q * s.den);
                    if (rem < 0) --q;
                    else if (rem >= (int64_t)s.den) ++q;
                }
                const int at = (a - a0) * lp + bl;
                if (WRES) reinterpret_cast<uint16_t *>(res)[2 * ((c >> 1) * RES + at) + (c & 1)] = (uint16_t)q;
                else reinterpret_cast<uint8_t *>(res)[4 * at + c] = (uint8_t)q;
            }
        }
    }
    __syncthreads();
    if constexpr (LIN) {
        // the tile holds mean levels Lm_0..2 and alpha's mean code, 16 bits each: the matrix and
        // out_lut (color_linear_encode), then the packed codes where store_row / store_tensor
        // read them for this format; alpha's quotient passes through
        typedef const uint32_t __attribute__((address_space(1))) *XfWords;
        const XfOutPairs<XfWords> out{(XfWords)(lx.lut + 6 * (uint64_t)lx.n)};
        const int nbv = b1 - b0, cnt = (a1 - a0) * nbv;
        for (int idx = t; idx < cnt; idx += 256) {
            const int al = idx / nbv, at = al * lp + (idx - al * nbv);
            const uint32_t lo = res[at], hi = res[RES + at];
            uint32_t R, G, B;
            color_linear_encode(out, lx.m, lo & 0xffffu, lo >> 16, hi & 0xffffu, R, G, B);
            if (WIDE) {
                res[at] = R | (G << 16);
                res[RES + at] = B | (hi & 0xffff0000u);
            } else {
                res[at] = R | (G << 8) | (B << 16) | ((hi >> 16) << 24);
            }
        }
        __syncthreads();
    } else if constexpr (XF) {
        // the transform of the tile's rounded averages, in place in the result tile
        const ColorRef x = reinterpret_cast<const ColorRef *>(descs + gridDim.y)[blockIdx.y];
        if (x.lut) {  // (uniform)
            const ToneW tw = tone_weights<TONE>(x);
            const int nbv = b1 - b0, cnt = (a1 - a0) * nbv;
            for (int idx = t; idx < cnt; idx += 256) {
                const int al = idx / nbv, at = al * lp + (idx - al * nbv);
                Px p = {res[at], WIDE ? res[RES + at] : 0u};
                uint32_t R = px_channel<FMT>(p, 0), G = px_channel<FMT>(p, 1), B = px_channel<FMT>(p, 2);
                xform_any<TONE>(x, tw, R, G, B);
                if (WIDE) {
                    res[at] = R | (G << 16);
                    res[RES + at] = B | (p.hi & 0xffff0000u);
                } else {
                    res[at] = R | (G << 8) | (B << 16) | (p.lo & 0xff000000u);
                }
            }
            __syncthreads();
        }
    }
    // write: lanes along the output's x, 64 pixels of a row per wave and step
    const Px none = {0, 0};
    if (!d.swap) {
        const int segs = s.nb >> 6;
        for (int u = wave; u < (a1 - a0) * segs; u += 4) {
            const int al = u / segs, oxw = b0 + (u % segs) * 64;
            if (oxw >= d.out_w) continue;
            const uint32_t *line = res + al * lp + (oxw - b0);
            if constexpr (TENSOR) {
                store_tensor<FMT>(dd, a0 + al, oxw, lane, [&](int i) {
                    return Px{line[i], WIDE ? line[RES + i] : 0u};
                });
            } else {
                const bool valid = oxw + lane < d.out_w;
                Px p = none;
                if (valid) {
                    p.lo = line[lane];
                    if (WIDE) p.hi = line[RES + lane];
                }
                store_row<FMT>(d, a0 + al, oxw, lane, p, valid);
            }
        }
    } else {
        const bool valid = a0 + lane < d.out_w;
        for (int oy = b0 + wave; oy < b1; oy += 4) {
            const uint32_t *col = res + (oy - b0);
            if constexpr (TENSOR) {
                store_tensor<FMT>(dd, oy, a0, lane, [&](int i) {
                    return Px{col[i * lp], WIDE ? col[RES + i * lp] : 0u};
                });
            } else {
                Px p = none;
                if (valid) {
                    p.lo = col[lane * lp];
                    if (WIDE) p.hi = col[RES + lane * lp];
                }
                store_row<FMT>(d, oy, a0, lane, p, valid);
            }
        }
    }
}

// Desc = ScaleDesc: the integer surfaces; TensorDesc: the tensor epilogue (element type
// and layout are uniform branches in store_tensor, so the heavy body is compiled once
// per sample width and source format for each of the two).  The overload for the two
// descriptors of k_render_scaled; a RenderDesc takes the one above.
template <typename Pel, int XF, typename Desc>
void launch_fmt(const Desc *descs, dim3 grid, int format, hipStream_t s) {
    switch (format) {
    case RENDER_RGB8: hipLaunchKernelGGL((k_render_scaled<Pel, RENDER_RGB8 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGBA8: hipLaunchKernelGGL((k_render_scaled<Pel, RENDER_RGBA8 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGB16: hipLaunchKernelGGL((k_render_scaled<Pel, RENDER_RGB16 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    default: hipLaunchKernelGGL((k_render_scaled<Pel, RENDER_RGBA16 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    }
}

// The kernels lie in the code object in the order of these instantiations: the order the
// six launchers before this one gave them, so that a build still compares byte for
// byte with the earlier ones (tools/kernel_text_diff.py).  The tone
// instantiations are a code object of their own, render_tone.hip, which is this file
// compiled with HG_RENDER_TONE_UNIT: this unit's kernels stay what they were.
#define HG_LAUNCH_FMT(XF, Desc)                                                   \
    template void launch_fmt<uint8_t, XF>(const Desc *, dim3, int, hipStream_t); \
    template void launch_fmt<uint16_t, XF>(const Desc *, dim3, int, hipStream_t)
#if defined(HG_RENDER_LINEAR_UNIT)
HG_LAUNCH_FMT(kRenderXf | kRenderLinear | kRenderChromaUp, ScaleDesc);
HG_LAUNCH_FMT(kRenderXf | kRenderLinear | kRenderChromaUp, TensorDesc);
#elif defined(HG_RENDER_CHROMA_UNIT)
HG_LAUNCH_FMT(kRenderXf | kRenderTone | kRenderChromaUp, RenderDesc);
HG_LAUNCH_FMT(kRenderXf | kRenderTone | kRenderChromaUp, ScaleDesc);
HG_LAUNCH_FMT(kRenderXf | kRenderTone | kRenderChromaUp, TensorDesc);
#elif defined(HG_RENDER_TONE_UNIT)
HG_LAUNCH_FMT(kRenderXf | kRenderTone, RenderDesc);
HG_LAUNCH_FMT(kRenderXf | kRenderTone, ScaleDesc);
HG_LAUNCH_FMT(kRenderXf | kRenderTone, TensorDesc);
#else
HG_LAUNCH_FMT(0, ScaleDesc);
HG_LAUNCH_FMT(0, TensorDesc);
HG_LAUNCH_FMT(kRenderXf, RenderDesc);
HG_LAUNCH_FMT(kRenderXf, ScaleDesc);
HG_LAUNCH_FMT(kRenderXf, TensorDesc);
HG_LAUNCH_FMT(0, RenderDesc);
#endif
#undef HG_LAUNCH_FMT

}  // namespace

#if defined(HG_RENDER_LINEAR_UNIT)
// (render_linear.hip: k_render_scaled averaging in linear light; no RenderDesc, no tone)
template <typename Desc>
hipError_t launch_render_linear(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                                hipStream_t s) {
    constexpr int LINEAR = kRenderXf | kRenderLinear | kRenderChromaUp;
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_fmt<uint8_t, LINEAR>(descs, grid, format, s);
    else launch_fmt<uint16_t, LINEAR>(descs, grid, format, s);
    return hipGetLastError();
}
template hipError_t launch_render_linear(const ScaleDesc *, int, int, int, int, hipStream_t);
template hipError_t launch_render_linear(const TensorDesc *, int, int, int, int, hipStream_t);
#elif defined(HG_RENDER_CHROMA_UNIT)
// (render_chroma.hip: the instantiations that know everything, bilinear chroma upsampling included)
template <typename Desc>
hipError_t launch_render_chroma(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                                hipStream_t s) {
    constexpr int ALL = kRenderXf | kRenderTone | kRenderChromaUp;
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_fmt<uint8_t, ALL>(descs, grid, format, s);
    else launch_fmt<uint16_t, ALL>(descs, grid, format, s);
    return hipGetLastError();
}
template hipError_t launch_render_chroma(const RenderDesc *, int, int, int, int, hipStream_t);
template hipError_t launch_render_chroma(const ScaleDesc *, int, int, int, int, hipStream_t);
template hipError_t launch_render_chroma(const TensorDesc *, int, int, int, int, hipStream_t);
#elif defined(HG_RENDER_TONE_UNIT)
template <typename Desc>
hipError_t launch_render_tone(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                              hipStream_t s) {
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_fmt<uint8_t, kRenderXf | kRenderTone>(descs, grid, format, s);
    else launch_fmt<uint16_t, kRenderXf | kRenderTone>(descs, grid, format, s);
    return hipGetLastError();
}
template hipError_t launch_render_tone(const RenderDesc *, int, int, int, int, hipStream_t);
template hipError_t launch_render_tone(const ScaleDesc *, int, int, int, int, hipStream_t);
template hipError_t launch_render_tone(const TensorDesc *, int, int, int, int, hipStream_t);
#else
template <typename Desc>
hipError_t launch_render(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample, int color,
                         hipStream_t s) {
    if (color == RENDER_CHROMA) return launch_render_chroma(descs, n_images, max_tiles, format, bytes_per_sample, s);
    if (color == RENDER_TONE) return launch_render_tone(descs, n_images, max_tiles, format, bytes_per_sample, s);
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) {
        if (color) launch_fmt<uint8_t, kRenderXf>(descs, grid, format, s);
        else launch_fmt<uint8_t, 0>(descs, grid, format, s);
    } else {
        if (color) launch_fmt<uint16_t, kRenderXf>(descs, grid, format, s);
        else launch_fmt<uint16_t, 0>(descs, grid, format, s);
    }
    return hipGetLastError();
}
template hipError_t launch_render(const RenderDesc *, int, int, int, int, int, hipStream_t);
template hipError_t launch_render(const ScaleDesc *, int, int, int, int, int, hipStream_t);
template hipError_t launch_render(const TensorDesc *, int, int, int, int, int, hipStream_t);
#endif
#endif

}  // namespace hg
