// render_px.hpp — what the render kernels share (render.hip: k_render, k_render_scaled;
// resample.hip: k_render_resampled): a packed pixel, convert()'s arithmetic from the
// decoded planes, the colour transform of a pixel, and the two stores, store_row
// (interleaved integers) and store_tensor (scaled and biased floats).  render.hip's
// opening comment describes them.  Device code only; every kernel's unit gets its own copy.
#pragma once
#include <cstddef>
#include <type_traits>

#include "chroma_up.hpp"
#include "color_xform.hpp"
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

// the transform's tables through global-address-space pointers (global_load, not flat_load)
typedef const uint16_t __attribute__((address_space(1))) *XfLut;

// the transform of one RGB triple, in place (x.lut != 0); staged: the same tables copied
// to LDS (the HG_XF_LDS build, an A/B of where the tables are read from), else null
__device__ __forceinline__ void xform_rgb(const ColorRef &x, uint32_t &R, uint32_t &G, uint32_t &B,
                                          const uint16_t *staged = nullptr) {
    if (staged) {
        const XfOutPairs<const uint32_t *> out{reinterpret_cast<const uint32_t *>(staged + 3 * x.n)};
        color_xform_px(staged, x.n, out, x.m, R, G, B);
        return;
    }
    typedef const uint32_t __attribute__((address_space(1))) *XfWords;
    const XfLut in = (XfLut)x.lut;
    const XfOutPairs<XfWords> out{(XfWords)(x.lut + 6 * (uint64_t)x.n)};
    color_xform_px(in, x.n, out, x.m, R, G, B);
}

// ---- the tone stage (the kRenderTone instantiations; x.tone != 0) ----
// what a workgroup keeps of its image's ToneBlock in registers: the luminance weights,
// read once before the workgroup's first store (scalar loads)
struct ToneW {
    int32_t w[3];
};
template <bool TONE>
__device__ __forceinline__ ToneW tone_weights(const ColorRef &x) {
    ToneW t = {{0, 0, 0}};
    if constexpr (TONE) {
        if (x.tone) {  // (uniform)
            typedef const int32_t __attribute__((address_space(1))) *Words;
            const Words p = (Words)(x.lut + (uint64_t)x.tone_off);
            t.w[0] = p[0], t.w[1] = p[1], t.w[2] = p[2];
        }
    }
    return t;
}

// xform_rgb for an image with a tone stage: in_lut32, the luminance, the gain pair
// (one 8-byte gather), then the matrix and out_lut as ever: seven gathers per pixel
__device__ __forceinline__ void tone_rgb(const ColorRef &x, const ToneW &tw, uint32_t &R, uint32_t &G, uint32_t &B) {
    typedef const uint32_t __attribute__((address_space(1))) *XfWords;
    typedef uint32_t XfPair __attribute__((ext_vector_type(2)));
    typedef const XfPair __attribute__((address_space(1))) *XfPairs;
    const XfWords in = (XfWords)x.lut;
    const XfOutPairs<XfWords> out{(XfWords)(x.lut + 12 * (uint64_t)x.n)};
    const XfTonePairs<XfPairs> tone{(XfPairs)(x.lut + (uint64_t)x.tone_off + offsetof(ToneBlock, pairs))};
    color_tone_px(in, x.n, tw.w, tone, out, x.m, R, G, B);
}

// the transform of one RGB triple by whichever of the two the image has (a uniform branch)
template <bool TONE>
__device__ __forceinline__ void xform_any(const ColorRef &x, const ToneW &tw, uint32_t &R, uint32_t &G, uint32_t &B,
                                          const uint16_t *staged = nullptr) {
    if constexpr (TONE) {
        if (x.tone) {
            tone_rgb(x, tw, R, G, B);
            return;
        }
    }
    xform_rgb(x, R, G, B, staged);
}

// ---- bilinear chroma upsampling (the kRenderChromaUp instantiations; cu.mode != 0) ----
// a call's ChromaRefs lie behind its gridDim.y descriptors and as many ColorRefs
template <bool CUP, typename Desc>
__device__ __forceinline__ ChromaRef chroma_ref_of(const Desc *descs) {
    ChromaRef cu{};
    if constexpr (CUP)
        cu = reinterpret_cast<const ChromaRef *>(reinterpret_cast<const ColorRef *>(descs + gridDim.y) + gridDim.y)[blockIdx.y];
    return cu;
}

// C' of Cb and Cr at decoded luma position (x, y), samples as decoded (chroma_up.hpp): the
// clamped 2 x 2 neighbourhood of each plane, 1 x 2 without a vertical filter (uniform).
// Load: sample<Pel> or sample_g<Pel>.
template <typename Load>
__device__ __forceinline__ void chroma_up_pair(const RenderDesc &d, const ChromaRef &cu, int x, int y, Load load, int &cb,
                                               int &cr) {
    const ChromaTap tx = chroma_tap(x, cu.px, cu.wc), ty = chroma_tap(y, cu.py, cu.hc);
    const int b00 = load(d.plane[1], d.pitch[1], tx.i0, ty.i0), b01 = load(d.plane[1], d.pitch[1], tx.i1, ty.i0);
    const int r00 = load(d.plane[2], d.pitch[2], tx.i0, ty.i0), r01 = load(d.plane[2], d.pitch[2], tx.i1, ty.i0);
    int b10 = b00, b11 = b01, r10 = r00, r11 = r01;
    if (cu.py >= 0) {
        b10 = load(d.plane[1], d.pitch[1], tx.i0, ty.i1), b11 = load(d.plane[1], d.pitch[1], tx.i1, ty.i1);
        r10 = load(d.plane[2], d.pitch[2], tx.i0, ty.i1), r11 = load(d.plane[2], d.pitch[2], tx.i1, ty.i1);
    }
    cb = chroma_value(b00, b01, b10, b11, tx, ty);
    cr = chroma_value(r00, r01, r10, r11, tx, ty);
}

template <typename Pel, int FMT, bool CUP = false>
__device__ __forceinline__ Px convert(const RenderDesc &d, int ox, int oy, const ChromaRef &cu = ChromaRef{}) {
    const int x = d.m[0] * ox + d.m[1] * oy + d.t[0], y = d.m[2] * ox + d.m[3] * oy + d.t[1];
    const int ys = sample<Pel>(d.plane[0], d.pitch[0], x, y) >> d.shift;
    int cb = 0, cr = 0;
    if constexpr (CUP) {
        if (d.chroma && cu.mode) {  // (uniform)
            chroma_up_pair(d, cu, x, y, [](uint64_t p, int32_t pitch, int cx, int cy) { return sample<Pel>(p, pitch, cx, cy); },
                           cb, cr);
            cb = (cb >> d.shift) - d.cmid;
            cr = (cr >> d.shift) - d.cmid;
        } else if (d.chroma) {
            const int xc = x >> chroma_sx(d.chroma), yc = y >> chroma_sy(d.chroma);
            cb = (sample<Pel>(d.plane[1], d.pitch[1], xc, yc) >> d.shift) - d.cmid;
            cr = (sample<Pel>(d.plane[2], d.pitch[2], xc, yc) >> d.shift) - d.cmid;
        }
    } else if (d.chroma) {
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

// the transform of a converted pixel, in place (alpha kept)
template <int FMT, bool TONE = false>
__device__ __forceinline__ void xform_pixel(const ColorRef &x, Px &p, const uint16_t *staged, const ToneW &tw = ToneW{}) {
    uint32_t R, G, B;
    if (FMT >= RENDER_RGB16) R = p.lo & 0xffffu, G = p.lo >> 16, B = p.hi & 0xffffu;
    else R = p.lo & 0xffu, G = (p.lo >> 8) & 0xffu, B = (p.lo >> 16) & 0xffu;
    xform_any<TONE>(x, tw, R, G, B, staged);
    if (FMT >= RENDER_RGB16) p = {R | (G << 16), B | (p.hi & 0xffff0000u)};
    else p = {R | (G << 8) | (B << 16) | (p.lo & 0xff000000u), 0};
}

// sample() through a global-address-space pointer (global_load, not flat_load: its
// wait does not also count LDS traffic)
template <typename T>
__device__ __forceinline__ int sample_g(uint64_t plane, int32_t pitch, int x, int y) {
    typedef const T __attribute__((address_space(1))) *gptr;
    return (int)*(gptr)(plane + (size_t)y * (size_t)pitch + (size_t)x * sizeof(T));
}

// ---- the tensor epilogue (heifgpu_render_batch_tensor) ------------------------
// F = fadd_rn(fmul_rn(float(R), a[c]), b[c]) in binary32, then rounded to the
// element type.  Two roundings: the pair must not become a fused multiply-add.
// __fmul_rn / __fadd_rn would not keep it apart: they are a plain product and sum
// in the header, compiled under -ffp-contract=fast, and the compiler fuses them.
// The product and the sum are written out here under a pragma that takes
// the contraction flag off both, so nothing later can fuse them.  f16 is the hardware's
// round-to-nearest-even conversion with gradual underflow (the f16 denormal mode
// is on by default), bf16 round-to-nearest-even on the bits (the inputs are finite).
__device__ __forceinline__ uint32_t tensor_elem(uint32_t level, float a, float b, int elem) {
#pragma clang fp contract(off)
    const float m = (float)level * a;
    const float f = m + b;
    const uint32_t u = __float_as_uint(f);
    if (elem == TENSOR_F32) return u;
    if (elem == TENSOR_F16) return (uint32_t) __builtin_bit_cast(uint16_t, (_Float16)f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <int FMT>
__device__ __forceinline__ uint32_t px_channel(Px p, int c) {
    if (FMT >= RENDER_RGB16) return (((c & 2) ? p.hi : p.lo) >> (16 * (c & 1))) & 0xffffu;
    return (p.lo >> (8 * c)) & 0xffu;
}

// v[c] for a c that differs between lanes (selects, not an indexed array: no scratch)
__device__ __forceinline__ float pick4(const float (&v)[4], int c) {
    return c == 0 ? v[0] : c == 1 ? v[1] : c == 2 ? v[2] : v[3];
}

// One wave stores pixels oxw .. oxw + 63 (oxw a multiple of 64) of output row oy; every
// lane of the wave calls it.  px(i) reads pixel oxw + i of that row from the result
// tile in LDS, for any i below the row's end (not only the lane's own), which is how
// the interleaved layout gets whole dwords without an exchange between lanes:
// - CHW: per channel 64 consecutive elements of one plane row.  f32 is a dword per
//   lane; f16 / bf16 pack two pixels into a dword through the right neighbour, even
//   lanes store (single elements where the plane row is not 4-byte aligned and for a
//   ragged last pixel);
// - HWC: the segment is 64 * C consecutive elements, written as consecutive dwords,
//   lane l taking dwords l, 64 + l, ...: it converts the one or two elements of its
//   dword, whichever pixels they belong to.  Lanes that read the same pixel read the
//   same LDS word (a broadcast), neighbours read neighbouring pixels, so the tile's
//   pitch (1 or 65 dwords per pixel) keeps the banks apart as in store_row's read.
//   Single elements per pixel where the row is not 4-byte aligned, and for an odd last one.
template <int FMT, typename Load>
__device__ __forceinline__ void store_tensor(const TensorDesc &td, int oy, int oxw, int lane, Load px) {
    constexpr int C = (FMT & 1) ? 4 : 3;
    const RenderDesc &d = td.s.r;
    const int elem = td.elem;
    const int nv = min(64, d.out_w - oxw);  // the segment's pixels (at least 1)
    uint8_t *row = reinterpret_cast<uint8_t *>(d.out) + (int64_t)oy * td.stride_y;
    if (td.layout == TENSOR_CHW) {
        const bool valid = lane < nv;
        const Px p = valid ? px(lane) : Px{0, 0};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint32_t e = tensor_elem(px_channel<FMT>(p, c), td.a[c], td.b[c], elem);
            uint8_t *pl = row + (int64_t)c * td.stride_c;
            if (elem == TENSOR_F32) {
                if (valid) reinterpret_cast<uint32_t *>(pl)[oxw + lane] = e;
            } else {
                const uint32_t nxt = __shfl_down(e, 1);
                if (!(reinterpret_cast<uintptr_t>(pl) & 3) && (lane | 1) < nv) {
                    if (!(lane & 1)) reinterpret_cast<uint32_t *>(pl)[(oxw + lane) >> 1] = e | (nxt << 16);
                } else if (valid) {
                    reinterpret_cast<uint16_t *>(pl)[oxw + lane] = (uint16_t)e;
                }
            }
        }
        return;
    }
    const int ne = nv * C;  // the segment's elements
    auto element = [&](int k) {  // element k of the segment
        const int i = k / C, c = k - i * C;
        return tensor_elem(px_channel<FMT>(px(i), c), pick4(td.a, c), pick4(td.b, c), elem);
    };
    if (elem == TENSOR_F32) {
        uint32_t *seg = reinterpret_cast<uint32_t *>(row) + (size_t)oxw * C;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int k = j * 64 + lane;
            if (k < ne) seg[k] = element(k);
        }
    } else if (!(reinterpret_cast<uintptr_t>(row) & 3)) {  // (64 pixels are a multiple of 4 bytes)
        uint16_t *seg = reinterpret_cast<uint16_t *>(row) + (size_t)oxw * C;
#pragma unroll
        for (int j = 0; j < 2; ++j) {  // 32 * C dwords
            const int k = 2 * (j * 64 + lane);
            if (k + 1 < ne) reinterpret_cast<uint32_t *>(seg)[k >> 1] = element(k) | (element(k + 1) << 16);
            else if (k < ne) seg[k] = (uint16_t)element(k);
        }
    } else if (lane < nv) {
        uint16_t *o = reinterpret_cast<uint16_t *>(row) + (size_t)(oxw + lane) * C;
        const Px p = px(lane);
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = (uint16_t)tensor_elem(px_channel<FMT>(p, c), td.a[c], td.b[c], elem);
    }
}

// ---- the scaled renders' first stage (k_render_scaled, render.hip; k_render_gain_scaled,
// render_gain_scaled.hip): what a thread does with the samples of its two source columns ----
constexpr int kScaleRowGroup = 4;  // source rows whose loads are issued together

struct ScaleChroma {
    int cb[2], cr[2];  // as loaded, for a thread's two columns
};

// convert()'s arithmetic for the two columns of one source row (samples as loaded),
// weighted into the column sums; every product has factors below 2^23
// (UP: cc holds C' of either column, chroma_up.hpp: two sets of products whatever the format)
// (LIN: the kRenderLinear instantiations: each clipped R, G, B goes through the image's in_lut,
// read through lin, before the weighted add, color_linear_level; alpha does not.  A level is at
// most 65535 and a line's weights sum to a window side, so the sums still fit 32 bits.)
struct NoLin {};
template <typename Lut>
struct LinLut {
    Lut t;  // in_lut[3][n], in LDS or in global memory
    int n;
};
template <int FMT, bool UP = false, bool LIN = false, typename Lin = NoLin>
__device__ __forceinline__ void scale_acc(const RenderDesc &d, const int (&ys)[2], const ScaleChroma &cc,
                                          const int (&al)[2], uint32_t w, uint32_t (&acc)[2][4], const Lin &lin = Lin{}) {
    int tr[2] = {0, 0}, tg[2] = {0, 0}, tb[2] = {0, 0};  // the chroma terms of R, G, B
    if (d.chroma) {
        const int n = !UP && chroma_sx(d.chroma) ? 1 : 2;  // a subsampled pair shares its sample: one set of products
        for (int c = 0; c < n; ++c) {
            const int cb = (cc.cb[c] >> d.shift) - d.cmid, cr = (cc.cr[c] >> d.shift) - d.cmid;
            tr[c] = __mul24(d.cr_r, cr);
            tg[c] = __mul24(d.cb_g, cb) + __mul24(d.cr_g, cr);
            tb[c] = __mul24(d.cb_b, cb);
        }
        if (n == 1) tr[1] = tr[0], tg[1] = tg[0], tb[1] = tb[0];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int yv = __mul24(d.ys, (ys[c] >> d.shift) - d.yoff) + 32768;
        const int R = min(max((yv + tr[c]) >> 16, 0), d.maxv);
        const int G = min(max((yv - tg[c]) >> 16, 0), d.maxv);
        const int B = min(max((yv + tb[c]) >> 16, 0), d.maxv);
        if constexpr (LIN) {
            acc[c][0] += __umul24(w, color_linear_level(lin.t, lin.n, 0, (uint32_t)R));
            acc[c][1] += __umul24(w, color_linear_level(lin.t, lin.n, 1, (uint32_t)G));
            acc[c][2] += __umul24(w, color_linear_level(lin.t, lin.n, 2, (uint32_t)B));
        } else {
            acc[c][0] += __umul24(w, (uint32_t)R);
            acc[c][1] += __umul24(w, (uint32_t)G);
            acc[c][2] += __umul24(w, (uint32_t)B);
        }
        if (FMT & 1) {
            int A = d.maxv;  // opaque
            if (d.alpha) A = d.alpha_shift >= 0 ? al[c] >> d.alpha_shift : al[c] << -d.alpha_shift;
            acc[c][3] += __umul24(w, (uint32_t)A);
        }
    }
}

}  // namespace
#endif

}  // namespace hg
