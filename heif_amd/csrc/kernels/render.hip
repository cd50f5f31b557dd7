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
#include "kernels.hpp"

namespace hg {

#if !defined(HG_HOST_EMU)
namespace {

struct Px {
    uint32_t lo, hi;  // 8-bit formats: lo = R | G << 8 | B << 16 | A << 24; 16-bit: lo = R | G << 16, hi = B | A << 16
};

template <typename T>
__device__ __forceinline__ int sample(uint64_t plane, int32_t pitch, int x, int y) {
    return (int)*reinterpret_cast<const T *>(reinterpret_cast<const uint8_t *>(plane) + (size_t)y * (size_t)pitch +
                                             (size_t)x * sizeof(T));
}

template <typename Pel, int FMT>
__device__ __forceinline__ Px convert(const RenderDesc &d, int ox, int oy) {
    const int x = d.m[0] * ox + d.m[1] * oy + d.t[0], y = d.m[2] * ox + d.m[3] * oy + d.t[1];
    const int ys = sample<Pel>(d.plane[0], d.pitch[0], x, y) >> d.shift;
    int cb = 0, cr = 0;
    if (d.chroma) {
        const int xc = x >> chroma_sx(d.chroma), yc = y >> chroma_sy(d.chroma);
        cb = (sample<Pel>(d.plane[1], d.pitch[1], xc, yc) >> d.shift) - d.cmid;
        cr = (sample<Pel>(d.plane[2], d.pitch[2], xc, yc) >> d.shift) - d.cmid;
    }
    const int yv = d.ys * (ys - d.yoff);
    const uint32_t R = (uint32_t)min(max((yv + d.cr_r * cr + 32768) >> 16, 0), d.maxv);
    const uint32_t G = (uint32_t)min(max((yv - d.cb_g * cb - d.cr_g * cr + 32768) >> 16, 0), d.maxv);
    const uint32_t B = (uint32_t)min(max((yv + d.cb_b * cb + 32768) >> 16, 0), d.maxv);
    uint32_t A = 0;
    if (FMT & 1) {
        A = (uint32_t)d.maxv;  // opaque
        if (d.alpha) {
            const int a = d.alpha_bps == 2 ? sample<uint16_t>(d.alpha, d.alpha_pitch, x, y)
                                           : sample<uint8_t>(d.alpha, d.alpha_pitch, x, y);
            A = (uint32_t)(d.alpha_shift >= 0 ? a >> d.alpha_shift : a << -d.alpha_shift);
        }
    }
    if (FMT >= RENDER_RGB16) return {R | (G << 16), B | (A << 16)};
    return {R | (G << 8) | (B << 16) | (A << 24), 0};
}

// One wave stores 64 pixels of output row oy starting at oxw (a multiple of 64);
// every lane of the wave calls it (lanes past the row's end with valid = false).
template <int FMT>
__device__ __forceinline__ void store_row(const RenderDesc &d, int oy, int oxw, int lane, Px p, bool valid) {
    uint8_t *row = reinterpret_cast<uint8_t *>(d.out) + (size_t)oy * (size_t)d.out_pitch;
    const bool al4 = !(reinterpret_cast<uintptr_t>(row) & 3);  // (64 pixels of any format are a multiple of 4 bytes)
    const int ox = oxw + lane;
    if (FMT == RENDER_RGB8) {
        const uint32_t nxt = __shfl_down(p.lo, 1);
        const int q = lane & 3;
        if (al4 && (ox | 3) < d.out_w) {
            const uint32_t w = q == 0 ? p.lo | (nxt << 24) : q == 1 ? (p.lo >> 8) | (nxt << 16) : (p.lo >> 16) | (nxt << 8);
            if (q < 3) reinterpret_cast<uint32_t *>(row + (size_t)oxw * 3)[lane - (lane >> 2)] = w;
        } else if (valid) {
            uint8_t *o = row + (size_t)ox * 3;
            o[0] = (uint8_t)p.lo;
            o[1] = (uint8_t)(p.lo >> 8);
            o[2] = (uint8_t)(p.lo >> 16);
        }
    } else if (FMT == RENDER_RGBA8) {
        if (!valid) return;
        if (al4) {
            reinterpret_cast<uint32_t *>(row)[ox] = p.lo;
        } else {
            uint8_t *o = row + (size_t)ox * 4;
            o[0] = (uint8_t)p.lo;
            o[1] = (uint8_t)(p.lo >> 8);
            o[2] = (uint8_t)(p.lo >> 16);
            o[3] = (uint8_t)(p.lo >> 24);
        }
    } else if (FMT == RENDER_RGB16) {
        const uint32_t nxt = __shfl_down(p.lo, 1);
        if (al4 && (ox | 1) < d.out_w) {
            uint32_t *w = reinterpret_cast<uint32_t *>(row + (size_t)oxw * 6) + 3 * (lane >> 1);
            if (lane & 1) {
                w[2] = (p.lo >> 16) | (p.hi << 16);
            } else {
                w[0] = p.lo;
                w[1] = (p.hi & 0xffffu) | (nxt << 16);
            }
        } else if (valid) {  // (the API requires 2-byte alignment of the 16-bit formats)
            uint16_t *o = reinterpret_cast<uint16_t *>(row) + (size_t)ox * 3;
            o[0] = (uint16_t)p.lo;
            o[1] = (uint16_t)(p.lo >> 16);
            o[2] = (uint16_t)p.hi;
        }
    } else {
        if (!valid) return;
        if (!(reinterpret_cast<uintptr_t>(row) & 7)) {
            reinterpret_cast<uint2 *>(row)[ox] = make_uint2(p.lo, p.hi);
        } else if (al4) {
            reinterpret_cast<uint32_t *>(row)[2 * (size_t)ox] = p.lo;
            reinterpret_cast<uint32_t *>(row)[2 * (size_t)ox + 1] = p.hi;
        } else {
            uint16_t *o = reinterpret_cast<uint16_t *>(row) + (size_t)ox * 4;
            o[0] = (uint16_t)p.lo;
            o[1] = (uint16_t)(p.lo >> 16);
            o[2] = (uint16_t)p.hi;
            o[3] = (uint16_t)(p.hi >> 16);
        }
    }
}

template <typename Pel, int FMT>
__global__ void __launch_bounds__(256) k_render(const RenderDesc *descs) {
    constexpr bool WIDE = FMT >= RENDER_RGB16;
    constexpr int T = kRenderTile, LP = kRenderTile + 1;  // LDS pitch in dwords: 65, not 64 (bank conflicts)
    __shared__ uint32_t tile_lds[(WIDE ? 2 : 1) * T * LP];
    const RenderDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x >= d.tiles) return;  // (a smaller image of the batch: the whole workgroup leaves)
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
            store_row<FMT>(d, oy, oxw, lane, valid ? convert<Pel, FMT>(d, ox, oy) : none, valid);
        }
        return;
    }
    const int ox0 = tx * T, oy0 = ty * T;
    // convert: lanes along the output's y, which is the source's x
    for (int i = 0; i < T / 4; ++i) {
        const int oxl = wave * (T / 4) + i, ox = ox0 + oxl, oy = oy0 + lane;
        if (ox < d.out_w && oy < d.out_h) {
            const Px p = convert<Pel, FMT>(d, ox, oy);
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

template <typename Pel>
void launch_fmt(const RenderDesc *descs, dim3 grid, int format, hipStream_t s) {
    switch (format) {
    case RENDER_RGB8: hipLaunchKernelGGL((k_render<Pel, RENDER_RGB8>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGBA8: hipLaunchKernelGGL((k_render<Pel, RENDER_RGBA8>), grid, dim3(256), 0, s, descs); break;
    case RENDER_RGB16: hipLaunchKernelGGL((k_render<Pel, RENDER_RGB16>), grid, dim3(256), 0, s, descs); break;
    default: hipLaunchKernelGGL((k_render<Pel, RENDER_RGBA16>), grid, dim3(256), 0, s, descs); break;
    }
}

}  // namespace

hipError_t launch_render(const RenderDesc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                         hipStream_t s) {
    const dim3 grid((unsigned)max_tiles, (unsigned)n_images);
    if (bytes_per_sample == 1) launch_fmt<uint8_t>(descs, grid, format, s);
    else launch_fmt<uint16_t>(descs, grid, format, s);
    return hipGetLastError();
}
#endif

}  // namespace hg
