// render_gain.hip — k_render_gain: a batch of decoded SDR base pictures with their gain maps →
// the HDR rendition, interleaved RGB(A) as linear half-float or PQ codes, in one launch
// (heifgpu_render_batch_gain; include/heifgpu.h "Gain-map HDR render").
//
// The kernel keeps k_render's shape (render.hip): grid (tile, image), 256 threads, one pixel per
// lane; 256 x 16 tiles with lanes along the row for maps that keep the axes, 64 x 64 tiles
// through the 65-dword LDS tile for maps that swap them; convert() and store_row of
// render_px.hpp unchanged.  Between the two sits the gain stage of gain_xform.hpp, per pixel:
//   - the pixel's decoded position → two taps per axis (one double-precision product and an
//     exact correction each: no 64-bit division);
//   - four gain-map sample loads (neighbouring lanes share them: at the usual 2:1 map the 64
//     pixels of a wave's row touch 33 bytes of each of two map rows);
//   - three in_lut gathers, one 8-byte gather of the pair T[i], T[i + 1], three 64-bit products,
//     the Q14 matrix in 64 bits;
//   - the encode: a product and a conversion per channel (linear), or one 8-byte gather of
//     E's pair and a 64-bit interpolation per channel (PQ).
// The tables are read where they lie, in the context's cache (global loads served by L1 / L2:
// 1.5 to 24 KiB of in_lut, 2 to 32 KiB of T pairs, 5 KiB of E pairs), as DESIGN 5.25 found
// best for the colour-managed render: the axis-keeping path has no barrier to stage them behind.
// A GainRef per image follows the descriptors.  The base's sample width is the template's Pel;
// the gain plane's and the alpha plane's are uniform branches.
#include "gain_xform.hpp"
#include "kernels.hpp"
#include "render_px.hpp"  // Px, sample, convert, store_row

namespace hg {

#if !defined(HG_HOST_EMU)
namespace {

typedef const uint32_t __attribute__((address_space(1))) *GainWords;
typedef uint32_t GainPair __attribute__((ext_vector_type(2)));
typedef const GainPair __attribute__((address_space(1))) *GainPairs;

// the Q8 gain code at decoded base position (x, y)
__device__ __forceinline__ uint32_t gain_at(const GainRef &g, int x, int y) {
    const GainTap tx = gain_tap(x, g.w, g.wg, g.inv_w), ty = gain_tap(y, g.h, g.hg, g.inv_h);
    uint32_t g00, g01, g10, g11;
    if (g.gain_bps == 2) {  // (uniform)
        g00 = (uint32_t)sample_g<uint16_t>(g.gain, g.gain_pitch, tx.i0, ty.i0);
        g01 = (uint32_t)sample_g<uint16_t>(g.gain, g.gain_pitch, tx.i1, ty.i0);
        g10 = (uint32_t)sample_g<uint16_t>(g.gain, g.gain_pitch, tx.i0, ty.i1);
        g11 = (uint32_t)sample_g<uint16_t>(g.gain, g.gain_pitch, tx.i1, ty.i1);
    } else {
        g00 = (uint32_t)sample_g<uint8_t>(g.gain, g.gain_pitch, tx.i0, ty.i0);
        g01 = (uint32_t)sample_g<uint8_t>(g.gain, g.gain_pitch, tx.i1, ty.i0);
        g10 = (uint32_t)sample_g<uint8_t>(g.gain, g.gain_pitch, tx.i0, ty.i1);
        g11 = (uint32_t)sample_g<uint8_t>(g.gain, g.gain_pitch, tx.i1, ty.i1);
    }
    return gain_sample(g00, g01, g10, g11, (uint32_t)tx.f, (uint32_t)ty.f);
}

// the gain stage of output pixel (ox, oy), in place on convert()'s 16-bit pixel
template <int HF>
__device__ __forceinline__ void gain_pixel(const RenderDesc &d, const GainRef &g, const GainParams &gp, int ox, int oy,
                                           Px &p) {
    const int x = d.m[0] * ox + d.m[1] * oy + d.t[0], y = d.m[2] * ox + d.m[3] * oy + d.t[1];
    const uint32_t gq = min(gain_at(g, x, y), g.gmax);
    uint32_t R = p.lo & 0xffffu, G = p.lo >> 16, B = p.hi & 0xffffu, A = p.hi >> 16;
    const XfLut in = (XfLut)g.lut;
    const XfTonePairs<GainPairs> T{(GainPairs)(g.lut + (uint64_t)g.t_off)}, E{(GainPairs)(g.lut + (uint64_t)g.e_off)};
    gain_px(in, g.n, T, E, gp, gq, R, G, B);
    if (HF & 1) {
        if (HF & 2) A = !d.alpha ? (uint32_t)g.maxp : g.alpha_shift >= 0 ? A >> g.alpha_shift : A << -g.alpha_shift;
        else A = !d.alpha ? 0x3c00u : gain_encode_linear(A, g.alpha_scale);  // (binary16 1.0 for an opaque pixel)
    }
    p = {R | (G << 16), B | (A << 16)};
}

// HF: GAIN_* (bit 0 alpha, bit 1 PQ)
template <typename Pel, int HF>
__global__ void __launch_bounds__(256) k_render_gain(const RenderDesc *descs) {
    constexpr int FMT = (HF & 1) ? RENDER_RGBA16 : RENDER_RGB16;
    constexpr int T = kRenderTile, LP = kRenderTile + 1;  // LDS pitch in dwords: 65, not 64 (bank conflicts)
    __shared__ uint32_t tile_lds[2 * T * LP];
    const RenderDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x >= d.tiles) return;  // (a smaller image of the batch: the whole workgroup leaves)
    const GainRef g = reinterpret_cast<const GainRef *>(descs + gridDim.y)[blockIdx.y];
    GainParams gp;
#pragma unroll
    for (int k = 0; k < 9; ++k) gp.m[k] = g.m[k];
    gp.k_b = g.k_b, gp.k_a = g.k_a;
    gp.encoding = (HF & 2) ? GAIN_ENC_PQ : GAIN_ENC_LINEAR;
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
            Px p = none;
            if (valid) {
                p = convert<Pel, FMT>(d, ox, oy);
                gain_pixel<HF>(d, g, gp, ox, oy, p);
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
            Px p = convert<Pel, FMT>(d, ox, oy);
            gain_pixel<HF>(d, g, gp, ox, oy, p);
            tile_lds[oxl * LP + lane] = p.lo;
            tile_lds[T * LP + oxl * LP + lane] = p.hi;
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
            p.hi = tile_lds[T * LP + lane * LP + oyl];
        }
        store_row<FMT>(d, oy, ox0, lane, p, valid);
    }
}

template <typename Pel>
void launch_gain_fmt(const RenderDesc *descs, dim3 grid, int format, hipStream_t s) {
    switch (format) {
    case GAIN_RGB16F: hipLaunchKernelGGL((k_render_gain<Pel, GAIN_RGB16F>), grid, dim3(256), 0, s, descs); break;
    case GAIN_RGBA16F: hipLaunchKernelGGL((k_render_gain<Pel, GAIN_RGBA16F>), grid, dim3(256), 0, s, descs); break;
    case GAIN_RGB16PQ: hipLaunchKernelGGL((k_render_gain<Pel, GAIN_RGB16PQ>), grid, dim3(256), 0, s, descs); break;
    default: hipLaunchKernelGGL((k_render_gain<Pel, GAIN_RGBA16PQ>), grid, dim3(256), 0, s, descs); break;
    }
}

}  // namespace

hipError_t launch_render_gain(const RenderDesc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                              hipStream_t s) {
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_gain_fmt<uint8_t>(descs, grid, format, s);
    else launch_gain_fmt<uint16_t>(descs, grid, format, s);
    return hipGetLastError();
}
#endif

}  // namespace hg
