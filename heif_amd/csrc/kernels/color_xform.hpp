// color_xform.hpp — the colour-managed render's per-pixel arithmetic, the one
// statement of it in code: k_render / k_render_scaled (render.hip) and
// heifgpu_color_apply (api/image.cpp) both call color_xform_px, so the CPU suite runs
// the very function the GPU runs.  include/heifgpu.h states the contract
// (heifgpu_color_transform); tests/color_ref.py restates it in numpy.
//
//   L_c  = in_lut[c][code_c]                                     (u16, linear light * 65535)
//   L'_k = clamp((m[3k] L_0 + m[3k+1] L_1 + m[3k+2] L_2 + 8192) >> 14, 0, 65535)
//          (Q14 matrix, 64-bit sum, arithmetic shift)
//   i = L'_k >> 4, f = L'_k & 15
//   out_k = (out_lut[i] (16 - f) + out_lut[i + 1] f + 128) >> 8   (out_lut in 1/16 code)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HG_XF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HG_XF_HD inline
#endif

namespace hg {

constexpr int kXfOutEntries = 4097;  // out_lut: one entry per 16 levels of L', and the end
constexpr int kXfMatrixOne = 16384;  // Q14

// How out_lut[i] and out_lut[i + 1] are fetched.  XfOutLut reads the table as the
// transform holds it.  XfOutPairs reads the device's copy, one 32-bit word per i
// holding out_lut[i] | out_lut[i + 1] << 16 (xf_out_pair), so a pixel costs six
// gathers, not nine; the values, and so the result, are the same.
template <typename Lut>
struct XfOutLut {
    Lut t;
    HG_XF_HD void operator()(uint32_t i, uint32_t &lo, uint32_t &hi) const { lo = t[i], hi = t[i + 1]; }
};
template <typename Words>
struct XfOutPairs {
    Words t;
    HG_XF_HD void operator()(uint32_t i, uint32_t &lo, uint32_t &hi) const {
        const uint32_t w = t[i];
        lo = w & 0xffffu, hi = w >> 16;
    }
};
constexpr int kXfPairEntries = kXfOutEntries - 1;  // i = L' >> 4 is at most 4095
inline uint32_t xf_out_pair(const uint16_t *out_lut, int i) { return (uint32_t)out_lut[i] | ((uint32_t)out_lut[i + 1] << 16); }

// the encoding half: the clamped L' through the interpolated table
template <typename Out>
HG_XF_HD uint32_t color_xform_encode(const Out &out, uint32_t L) {
    const uint32_t i = L >> 4, f = L & 15u;
    uint32_t lo, hi;
    out(i, lo, hi);
    return (lo * (16u - f) + hi * f + 128u) >> 8;
}

// L' of a matrix sum (64 bits wide: a row of a wide-gamut matrix times 65535 can pass 2^31;
// sums kept in 32 bits where they provably fit measured slower on the MI355X)
HG_XF_HD uint32_t color_xform_level(int64_t sum) {
    const int64_t v = (sum + 8192) >> 14;
    return (uint32_t)(v < 0 ? 0 : v > 65535 ? 65535 : v);
}

// One pixel in place.  in_lut: three tables of n = 1 << B entries, one after the
// other; r, g, b: codes 0 .. n - 1 in, codes 0 .. n - 1 out.
template <typename Lut, typename Out>
HG_XF_HD void color_xform_px(Lut in_lut, int n, const Out &out_lut, const int32_t (&m)[9], uint32_t &r, uint32_t &g,
                             uint32_t &b) {
    const int64_t l0 = in_lut[r], l1 = in_lut[n + g], l2 = in_lut[2 * n + b];
    r = color_xform_encode(out_lut, color_xform_level(m[0] * l0 + m[1] * l1 + m[2] * l2));
    g = color_xform_encode(out_lut, color_xform_level(m[3] * l0 + m[4] * l1 + m[5] * l2));
    b = color_xform_encode(out_lut, color_xform_level(m[6] * l0 + m[7] * l1 + m[8] * l2));
}

}  // namespace hg
