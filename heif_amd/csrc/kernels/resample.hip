// resample.hip — k_render_resampled: a window of the displayed picture D through Pillow's
// antialiased bilinear or bicubic filter onto another grid, for a batch in one launch
// (heifgpu_render_batch_resampled, heifgpu_render_batch_tensor_resampled).  The arithmetic
// is kernels/resample.hpp's (include/heifgpu.h states it): coefficients in binary64 with
// P fractional bits, a pass along D's x into rounded and clipped intermediates, then a
// pass along D's y over those.  D's pixels are convert()'s (render_px.hpp), so the
// identity window is heifgpu_render_batch's bytes.
//
// A workgroup (256 threads) owns 64 x 16 STORED pixels (a flip reverses which output a
// stored pixel shows, nothing else: coefficients are always those of D's coordinates).
// Wave 0 finds every column's taps [lo, hi), centre and weight sum (the sum is a pass of
// its own over the taps, in the order Pillow adds them), wave 1 every row's.  The tile's
// columns are then taken `sw` at a time (the host picks sw so that the footprint of sw
// columns fits one chunk of 256 columns of D and their coefficients fit the table):
//   for each chunk of 16 rows of D inside the tile's vertical footprint
//     for each chunk of 256 columns of D inside the sub-tile's horizontal footprint
//       1. every sample of the chunk is converted once (lanes along the source's x:
//          along D's x, or along D's y for the maps that swap the axes; the global
//          loads of four pixels are issued before the first is used) into LDS,
//          packed as Px, pitch 257 dwords (the swapped write walks a column);
//       2. a thread (column, row) adds coefficient * channel over the column's taps in
//          the chunk into int32 sums; the coefficients come from an LDS table filled
//          once per sub-tile when one chunk holds the footprint, else per chunk;
//     the 16 x sw sums are rounded and clipped into LDS (the intermediate T), the 16 x 16
//     vertical coefficients of the chunk's rows are computed, one per thread, and
//     a thread (column, output row) adds coefficient * T into its int32 sums.
// Footprints of any width and height are walked by these loops: LDS and registers do not
// depend on the ratio.  The results wait in LDS as Px, are colour-transformed there
// (XF, as k_render_scaled) and leave through store_row or store_tensor.
#include <type_traits>

#include "kernels.hpp"
#include "render_px.hpp"
#include "resample.hpp"

namespace hg {

#if !defined(HG_HOST_EMU)
namespace {

__device__ __forceinline__ const RenderDesc &render_of(const ResampleDesc &s) { return s.r; }
__device__ __forceinline__ const RenderDesc &render_of(const ResampleTensorDesc &s) { return s.t.s.r; }

template <int FMT>
__device__ __forceinline__ Px px_pack(const int32_t (&v)[4]) {
    if (FMT >= RENDER_RGB16) return {(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16)};
    return {(uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24), 0};
}

// convert() in two steps, so that the loads of several pixels can be issued before the
// first is used: the samples of D's pixel (ox, oy) as loaded (global loads, sample_g), and
// convert()'s arithmetic over them, operation for operation.
struct RawPx {
    int y, cb, cr, a;
};

// (CUP, cu.mode != 0: cb and cr are C' of the pixel's position, chroma_up.hpp, as convert()'s)
template <typename Pel, int FMT, bool CUP = false>
__device__ __forceinline__ RawPx load_raw(const RenderDesc &d, int ox, int oy, const ChromaRef &cu = ChromaRef{}) {
    const int x = d.m[0] * ox + d.m[1] * oy + d.t[0], y = d.m[2] * ox + d.m[3] * oy + d.t[1];
    RawPx r = {sample_g<Pel>(d.plane[0], d.pitch[0], x, y), 0, 0, 0};
    if constexpr (CUP) {
        if (d.chroma && cu.mode) {  // (uniform)
            chroma_up_pair(d, cu, x, y, [](uint64_t p, int32_t pitch, int cx, int cy) { return sample_g<Pel>(p, pitch, cx, cy); },
                           r.cb, r.cr);
        } else if (d.chroma) {
            const int xc = x >> chroma_sx(d.chroma), yc = y >> chroma_sy(d.chroma);
            r.cb = sample_g<Pel>(d.plane[1], d.pitch[1], xc, yc);
            r.cr = sample_g<Pel>(d.plane[2], d.pitch[2], xc, yc);
        }
    } else if (d.chroma) {
        const int xc = x >> chroma_sx(d.chroma), yc = y >> chroma_sy(d.chroma);
        r.cb = sample_g<Pel>(d.plane[1], d.pitch[1], xc, yc);
        r.cr = sample_g<Pel>(d.plane[2], d.pitch[2], xc, yc);
    }
    if ((FMT & 1) && d.alpha)
        r.a = d.alpha_bps == 2 ? sample_g<uint16_t>(d.alpha, d.alpha_pitch, x, y) : sample_g<uint8_t>(d.alpha, d.alpha_pitch, x, y);
    return r;
}

template <int FMT>
__device__ __forceinline__ Px convert_raw(const RenderDesc &d, const RawPx &r) {
    const int ys = r.y >> d.shift;
    int cb = 0, cr = 0;
    if (d.chroma) {
        cb = (r.cb >> d.shift) - d.cmid;
        cr = (r.cr >> d.shift) - d.cmid;
    }
    const int yv = d.ys * (ys - d.yoff);
    const uint32_t R = (uint32_t)min(max((yv + d.cr_r * cr + 32768) >> 16, 0), d.maxv);
    const uint32_t G = (uint32_t)min(max((yv - d.cb_g * cb - d.cr_g * cr + 32768) >> 16, 0), d.maxv);
    const uint32_t B = (uint32_t)min(max((yv + d.cb_b * cb + 32768) >> 16, 0), d.maxv);
    uint32_t A = 0;
    if (FMT & 1) {
        A = (uint32_t)d.maxv;  // opaque
        if (d.alpha) A = (uint32_t)(d.alpha_shift >= 0 ? r.a >> d.alpha_shift : r.a << -d.alpha_shift);
    }
    if (FMT >= RENDER_RGB16) return {R | (G << 16), B | (A << 16)};
    return {R | (G << 8) | (B << 16) | (A << 24), 0};
}

constexpr int kRsLoadGroup = 4;  // pixels whose loads are issued together

template <typename Pel, int FMTX, typename Desc>
__global__ void __launch_bounds__(256) k_render_resampled(const Desc *descs) {
    constexpr int FMT = FMTX & 3;
    constexpr bool XF = (FMTX & kRenderXf) != 0;  // (as k_render's)
    constexpr bool TONE = (FMTX & kRenderTone) != 0;
    constexpr bool CUP = (FMTX & kRenderChromaUp) != 0;
    constexpr bool TENSOR = std::is_same<Desc, ResampleTensorDesc>::value;
    constexpr bool WIDE = FMT >= RENDER_RGB16;
    constexpr int NCH = (FMT & 1) ? 4 : 3;
    constexpr int TW = kRsTileW, TH = kRsTileH, RC = kRsRows, CC = kRsCols, DP = kRsCols + 1;
    constexpr int NJ = 4;  // rows (or output rows) per thread: 16 over the 256 / sw >= 4 threads of a column
    static_assert(TH == RC && TH * TW == 4 * 256 && TW == 64, "the thread maps below");
    __shared__ uint32_t dpx[(WIDE ? 2 : 1) * RC * DP];
    __shared__ uint32_t tmid[(WIDE ? 2 : 1) * RC * TW];
    __shared__ uint32_t res[(WIDE ? 2 : 1) * TH * TW];
    __shared__ int32_t ktab[kRsCoefCap];
    __shared__ int32_t kytab[TH * RC];
    __shared__ double cen[TW + TH], wsum[TW + TH];  // columns, then rows
    __shared__ int32_t tlo[TW + TH], thi[TW + TH];
    const Desc dd = descs[blockIdx.y];
    const RenderDesc &d = render_of(dd);
    const RsParams &p = dd.p;
    if ((int)blockIdx.x >= d.tiles) return;  // (a smaller image of the batch: the whole workgroup leaves)
    const ChromaRef cu = chroma_ref_of<CUP>(descs);
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int sx0 = ((int)blockIdx.x % d.tiles_x) * TW, sy0 = ((int)blockIdx.x / d.tiles_x) * TH;
    const int nx = min(TW, d.out_w - sx0), ny = min(TH, d.out_h - sy0);
    const int P = p.P, maxv = d.maxv;

    // the taps of the tile's columns (wave 0) and rows (wave 1)
    if (t < TW + TH) {
        const bool col = t < TW;
        const int i = col ? t : t - TW;
        if (i < (col ? nx : ny)) {
            const RsAxis &a = col ? p.ax : p.ay;
            const int s = (col ? sx0 : sy0) + i;  // stored index
            const int o = (p.flip & (col ? 1 : 2)) ? a.out - 1 - s : s;
            int lo, hi;
            rs_bounds(a, o, lo, hi);
            const double c = rs_center(a, o);
            tlo[t] = lo;
            thi[t] = hi;
            cen[t] = c;
            wsum[t] = rs_weight_sum(a, c, lo, hi);
        }
    }
    __syncthreads();
    const int fy0 = min(tlo[TW], tlo[TW + ny - 1]), fy1 = max(thi[TW], thi[TW + ny - 1]);
    const int kw = min(p.ax.ksize, CC);  // table entries per column
    const int sw = p.sw, nq = 256 / sw;
    const int xi = t % sw, q = t / sw;

    for (int i0 = 0; i0 < nx; i0 += sw) {
        const int n = min(sw, nx - i0);
        const int fx0 = min(tlo[i0], tlo[i0 + n - 1]), fx1 = max(thi[i0], thi[i0 + n - 1]);
        const bool single = fx1 - fx0 <= CC;  // (uniform)
        const bool mine = xi < n && q < nq;
        const int xlo = mine ? tlo[i0 + xi] : 0, xhi = mine ? thi[i0 + xi] : 0;
        // coefficients of the sub-tile's columns for their taps in D columns [c0, c1)
        auto fill_ktab = [&](int c0, int c1) {
            for (int e = t; e < n * kw; e += 256) {
                const int ci = e / kw, at = max(tlo[i0 + ci], c0) + (e - ci * kw);
                if (at < min(thi[i0 + ci], c1))
                    ktab[e] = rs_coeff(rs_weight(p.ax, cen[i0 + ci], at), wsum[i0 + ci], P);
            }
        };
        if (single) fill_ktab(fx0, fx1);  // (read behind the chunk's barrier below)
        int32_t vacc[NJ][4];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) vacc[j][c] = rs_half(P);

        for (int ry = fy0; ry < fy1; ry += RC) {
            const int nr = min(RC, fy1 - ry);
            int32_t hacc[NJ][4];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) hacc[j][c] = rs_half(P);
            for (int cx = fx0; cx < fx1; cx += CC) {
                const int nc = min(CC, fx1 - cx);
                // 1. the chunk's pixels
                // (a pixel past the chunk's end loads the last one again and is not stored)
                constexpr int G = kRsLoadGroup;
                if (!d.swap) {
                    if (t < nc)
                        for (int r0 = 0; r0 < nr; r0 += G) {
                            RawPx raw[G];
#pragma unroll
                            for (int g = 0; g < G; ++g) raw[g] = load_raw<Pel, FMT, CUP>(d, cx + t, ry + min(r0 + g, nr - 1), cu);
#pragma unroll
                            for (int g = 0; g < G; ++g) {
                                const int r = r0 + g;
                                if (r >= nr) break;
                                const Px v = convert_raw<FMT>(d, raw[g]);
                                dpx[r * DP + t] = v.lo;
                                if (WIDE) dpx[RC * DP + r * DP + t] = v.hi;
                            }
                        }
                } else {
                    const int r = t & (RC - 1);
                    if (r < nr)
                        for (int c0 = t >> 4; c0 < nc; c0 += G * (256 / RC)) {
                            RawPx raw[G];
#pragma unroll
                            for (int g = 0; g < G; ++g)
                                raw[g] = load_raw<Pel, FMT, CUP>(d, cx + min(c0 + g * (256 / RC), nc - 1), ry + r, cu);
#pragma unroll
                            for (int g = 0; g < G; ++g) {
                                const int c = c0 + g * (256 / RC);
                                if (c >= nc) break;
                                const Px v = convert_raw<FMT>(d, raw[g]);
                                dpx[r * DP + c] = v.lo;
                                if (WIDE) dpx[RC * DP + r * DP + c] = v.hi;
                            }
                        }
                }
                if (!single) fill_ktab(cx, cx + nc);
                __syncthreads();
                // 2. along D's x
                if (mine) {
                    const int base = max(xlo, single ? fx0 : cx);
                    const int lo = max(xlo, cx), hi = min(xhi, cx + nc);
                    const int32_t *kt = ktab + xi * kw - base;
                    for (int at = lo; at < hi; ++at) {
                        const int32_t k = kt[at];
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int r = q + nq * j;
                            if (r < nr) {
                                const int w = r * DP + (at - cx);
                                const Px v = {dpx[w], WIDE ? dpx[RC * DP + w] : 0u};
#pragma unroll
                                for (int c = 0; c < NCH; ++c) hacc[j][c] += __mul24(k, (int)px_channel<FMT>(v, c));
                            }
                        }
                    }
                }
                __syncthreads();
            }
            // the intermediate of the chunk's rows, and the rows' vertical coefficients
            if (mine) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int r = q + nq * j;
                    if (r < nr) {
                        int32_t v[4] = {0, 0, 0, 0};
#pragma unroll
                        for (int c = 0; c < NCH; ++c) v[c] = rs_round(hacc[j][c], P, maxv);
                        const Px m = px_pack<FMT>(v);
                        tmid[r * TW + xi] = m.lo;
                        if (WIDE) tmid[RC * TW + r * TW + xi] = m.hi;
                    }
                }
            }
            {
                const int yi = t >> 4, r = t & (RC - 1), at = ry + r;
                int32_t k = 0;
                if (yi < ny && r < nr && at >= tlo[TW + yi] && at < thi[TW + yi])
                    k = rs_coeff(rs_weight(p.ay, cen[TW + yi], at), wsum[TW + yi], P);
                kytab[t] = k;
            }
            __syncthreads();
            // along D's y
            if (mine) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int yi = q + nq * j;
                    if (yi < ny) {
                        const int r0 = max(tlo[TW + yi] - ry, 0), r1 = min(thi[TW + yi] - ry, nr);
                        for (int r = r0; r < r1; ++r) {
                            const int32_t k = kytab[yi * RC + r];
                            const Px v = {tmid[r * TW + xi], WIDE ? tmid[RC * TW + r * TW + xi] : 0u};
#pragma unroll
                            for (int c = 0; c < NCH; ++c) vacc[j][c] += __mul24(k, (int)px_channel<FMT>(v, c));
                        }
                    }
                }
            }
            // (tmid and kytab are written again behind the next chunk's barriers)
        }
        if (mine) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int yi = q + nq * j;
                if (yi < ny) {
                    int32_t v[4] = {0, 0, 0, 0};  // (the RGB formats keep a zero where alpha would be)
#pragma unroll
                    for (int c = 0; c < NCH; ++c) v[c] = rs_round(vacc[j][c], P, maxv);
                    const Px m = px_pack<FMT>(v);
                    res[yi * TW + i0 + xi] = m.lo;
                    if (WIDE) res[TH * TW + yi * TW + i0 + xi] = m.hi;
                }
            }
        }
        __syncthreads();  // the next sub-tile's table and chunks
    }
    if constexpr (XF) {
        // the transform of the tile's rounded results, in place (as k_render_scaled's)
        const ColorRef x = reinterpret_cast<const ColorRef *>(descs + gridDim.y)[blockIdx.y];
        if (x.lut) {  // (uniform)
            const ToneW tw = tone_weights<TONE>(x);
            for (int idx = t; idx < ny * TW; idx += 256) {
                if ((idx & (TW - 1)) >= nx) continue;
                Px v = {res[idx], WIDE ? res[TH * TW + idx] : 0u};
                uint32_t R = px_channel<FMT>(v, 0), G = px_channel<FMT>(v, 1), B = px_channel<FMT>(v, 2);
                xform_any<TONE>(x, tw, R, G, B);
                if (WIDE) {
                    res[idx] = R | (G << 16);
                    res[TH * TW + idx] = B | (v.hi & 0xffff0000u);
                } else {
                    res[idx] = R | (G << 8) | (B << 16) | (v.lo & 0xff000000u);
                }
            }
            __syncthreads();
        }
    }
    // write: lanes along the stored x, a row of the tile per wave and step
    for (int u = wave; u < ny; u += 4) {
        const uint32_t *line = res + u * TW;
        if constexpr (TENSOR) {
            store_tensor<FMT>(dd.t, sy0 + u, sx0, lane, [&](int i) { return Px{line[i], WIDE ? line[TH * TW + i] : 0u}; });
        } else {
            const bool valid = lane < nx;
            Px v = {0, 0};
            if (valid) {
                v.lo = line[lane];
                if (WIDE) v.hi = line[TH * TW + lane];
            }
            store_row<FMT>(d, sy0 + u, sx0, lane, v, valid);
        }
    }
}

template <typename Pel, int XF, typename Desc>
void launch_fmt(const Desc *descs, dim3 grid, int format, hipStream_t s) {
    switch (format) {
    case RENDER_RGB8: hipLaunchKernelGGL((k_render_resampled<Pel, RENDER_RGB8 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGBA8: hipLaunchKernelGGL((k_render_resampled<Pel, RENDER_RGBA8 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGB16: hipLaunchKernelGGL((k_render_resampled<Pel, RENDER_RGB16 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    default: hipLaunchKernelGGL((k_render_resampled<Pel, RENDER_RGBA16 | XF, Desc>), grid, dim3(256), 0, s, descs); break;
    }
}

#if defined(HG_RENDER_CHROMA_UNIT)
// (resample_chroma.hip: this file compiled with HG_RENDER_CHROMA_UNIT, the instantiations that
// know everything, bilinear chroma upsampling included, as a code object of their own)
template <typename Desc>
hipError_t launch_resampled_chroma(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                                   hipStream_t s) {
    constexpr int ALL = kRenderXf | kRenderTone | kRenderChromaUp;
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_fmt<uint8_t, ALL>(descs, grid, format, s);
    else launch_fmt<uint16_t, ALL>(descs, grid, format, s);
    return hipGetLastError();
}
#elif !defined(HG_RENDER_TONE_UNIT)
template <typename Desc>
hipError_t launch_resampled(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample, int color,
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
#else
// (resample_tone.hip: this file compiled with HG_RENDER_TONE_UNIT, the tone instantiations
// as a code object of their own, so that this unit's kernels stay what they were)
template <typename Desc>
hipError_t launch_resampled_tone(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                                 hipStream_t s) {
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_fmt<uint8_t, kRenderXf | kRenderTone>(descs, grid, format, s);
    else launch_fmt<uint16_t, kRenderXf | kRenderTone>(descs, grid, format, s);
    return hipGetLastError();
}
#endif

}  // namespace

#if defined(HG_RENDER_CHROMA_UNIT)
template <>
hipError_t launch_render_chroma<ResampleDesc>(const ResampleDesc *descs, int n_images, int max_tiles, int format,
                                              int bytes_per_sample, hipStream_t s) {
    return launch_resampled_chroma(descs, n_images, max_tiles, format, bytes_per_sample, s);
}
template <>
hipError_t launch_render_chroma<ResampleTensorDesc>(const ResampleTensorDesc *descs, int n_images, int max_tiles,
                                                    int format, int bytes_per_sample, hipStream_t s) {
    return launch_resampled_chroma(descs, n_images, max_tiles, format, bytes_per_sample, s);
}
#elif !defined(HG_RENDER_TONE_UNIT)
template <>
hipError_t launch_render<ResampleDesc>(const ResampleDesc *descs, int n_images, int max_tiles, int format,
                                       int bytes_per_sample, int color, hipStream_t s) {
    return launch_resampled(descs, n_images, max_tiles, format, bytes_per_sample, color, s);
}
template <>
hipError_t launch_render<ResampleTensorDesc>(const ResampleTensorDesc *descs, int n_images, int max_tiles, int format,
                                             int bytes_per_sample, int color, hipStream_t s) {
    return launch_resampled(descs, n_images, max_tiles, format, bytes_per_sample, color, s);
}
#else
template <>
hipError_t launch_render_tone<ResampleDesc>(const ResampleDesc *descs, int n_images, int max_tiles, int format,
                                            int bytes_per_sample, hipStream_t s) {
    return launch_resampled_tone(descs, n_images, max_tiles, format, bytes_per_sample, s);
}
template <>
hipError_t launch_render_tone<ResampleTensorDesc>(const ResampleTensorDesc *descs, int n_images, int max_tiles,
                                                  int format, int bytes_per_sample, hipStream_t s) {
    return launch_resampled_tone(descs, n_images, max_tiles, format, bytes_per_sample, s);
}
#endif
#endif

}  // namespace hg
