// color_xform.hpp — the colour-managed render's per-pixel arithmetic, the one
// statement of it in code: k_render / k_render_scaled (render.hip) and
// heifgpu_color_apply (api/image.cpp) both call color_xform_px, so the CPU suite runs
// the very function the GPU runs.  include/heifgpu.h states the contract
// (heifgpu_color_transform); tests/color_ref.py restates it in numpy.  The tone stage
// of an HDR source (color_tone_px, further down; tests/tone_ref.py) puts itself between
// in_lut and the matrix and shares everything from the matrix on.
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

// the matrix and the encoding of three linear levels
template <typename Out>
HG_XF_HD void color_xform_linear(const Out &out_lut, const int32_t (&m)[9], int64_t l0, int64_t l1, int64_t l2, uint32_t &r,
                                 uint32_t &g, uint32_t &b) {
    r = color_xform_encode(out_lut, color_xform_level(m[0] * l0 + m[1] * l1 + m[2] * l2));
    g = color_xform_encode(out_lut, color_xform_level(m[3] * l0 + m[4] * l1 + m[5] * l2));
    b = color_xform_encode(out_lut, color_xform_level(m[6] * l0 + m[7] * l1 + m[8] * l2));
}

// One pixel in place.  in_lut: three tables of n = 1 << B entries, one after the
// other; r, g, b: codes 0 .. n - 1 in, codes 0 .. n - 1 out.
template <typename Lut, typename Out>
HG_XF_HD void color_xform_px(Lut in_lut, int n, const Out &out_lut, const int32_t (&m)[9], uint32_t &r, uint32_t &g,
                             uint32_t &b) {
    const int64_t l0 = in_lut[r], l1 = in_lut[n + g], l2 = in_lut[2 * n + b];
    color_xform_linear(out_lut, m, l0, l1, l2, r, g, b);
}

// ---- the linear-light scaled render (include/heifgpu.h, "Linear-light scaled render") ----
// The order is the other one: every source sample of the window goes through in_lut BEFORE
// the area sum (color_linear_level, three table reads per sample), the rounded mean levels
// Lm go through the matrix and out_lut AFTER the quotient (color_linear_encode).  Called by
// k_render_scaled's kRenderLinear instantiations and by heifgpu_linear_average_apply
// (api/image.cpp); tests/linear_ref.py restates the whole in numpy.
//   S_c  = sum_j sum_i wy(Y,j) wx(X,i) in_lut[c][code_c(j,i)]     (below 2^48: sides and levels at most 65535)
//   Lm_c = floor((2 S_c + cw ch) / (2 cw ch))                     (round half up; 0..65535)

// the per-sample step: channel c's code as its linear level
template <typename Lut>
HG_XF_HD uint32_t color_linear_level(Lut in_lut, int n, int c, uint32_t code) {
    return in_lut[c * n + (int)code];
}

// the rounded mean level of a full sum S over a window of cwch = cw * ch pixels, in plain
// integers (the kernel takes the same quotient from a double estimate corrected exactly)
HG_XF_HD uint32_t color_linear_mean(uint64_t S, uint64_t cwch) { return (uint32_t)((2 * S + cwch) / (2 * cwch)); }

// the level-to-code step: three mean levels through the matrix and out_lut
template <typename Out>
HG_XF_HD void color_linear_encode(const Out &out_lut, const int32_t (&m)[9], uint32_t lm0, uint32_t lm1, uint32_t lm2,
                                  uint32_t &r, uint32_t &g, uint32_t &b) {
    color_xform_linear(out_lut, m, (int64_t)lm0, (int64_t)lm1, (int64_t)lm2, r, g, b);
}

// ---- the tone stage of an HDR source (include/heifgpu.h, "HDR render") ----------
//   L_c   = in_lut32[c][code_c]                       (u32 below 2^22; 65535 = 203 cd/m2)
//   Y     = (w0 L_0 + w1 L_1 + w2 L_2 + 8192) >> 14   (w in Q14, sum 16384: Y below 2^22 too)
//   g     = the gain table T at Y, 32 nodes per octave, interpolated (tone_gain)
//   L''_c = min((L_c g + 2^23) >> 24, 65535)          (g has kXfToneShift = 24 fractional bits)
// and then color_xform_linear on L''.
constexpr int kXfToneEntries = 577;                   // T's nodes: Y = 0 .. 63, then 32 per octave up to 2^22
constexpr int kXfTonePairs = kXfToneEntries - 1;      // the index is at most 575
constexpr uint32_t kXfToneMaxLevel = (1u << 22) - 1;  // the largest in_lut32 entry the index has nodes for
constexpr int kXfToneShift = 24;                      // T's fractional bits: a gain of 1 is 1 << 24

// the level of node k of T
inline uint32_t xf_tone_node(int k) { return k < 64 ? (uint32_t)k : (uint32_t)(32 + ((k - 32) & 31)) << ((k - 32) >> 5); }

// How T[idx] and T[idx + 1] are fetched: as the transform holds them, or from the
// device's copy, one 8-byte pair per idx (as XfOutLut / XfOutPairs above).
template <typename Lut>
struct XfToneLut {
    Lut t;
    HG_XF_HD void operator()(uint32_t i, uint32_t &lo, uint32_t &hi) const { lo = t[i], hi = t[i + 1]; }
};
template <typename Pairs>
struct XfTonePairs {
    Pairs t;  // of a two-word vector type with .x and .y
    HG_XF_HD void operator()(uint32_t i, uint32_t &lo, uint32_t &hi) const {
        const auto p = t[i];
        lo = p.x, hi = p.y;
    }
};

HG_XF_HD uint32_t xf_bitlength(uint32_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 32u - (uint32_t)__builtin_clz(v);
#else
    uint32_t n = 0;
    for (; v; v >>= 1) ++n;
    return n;
#endif
}

// the gain at luminance Y (Y <= kXfToneMaxLevel), kXfToneShift fractional bits, at most 1 << kXfToneShift
template <typename Tone>
HG_XF_HD uint32_t color_tone_gain(const Tone &tone, uint32_t Y) {
    uint32_t lo, hi;
    if (Y < 64) {
        tone(Y, lo, hi);
        return lo;
    }
    const uint32_t e = xf_bitlength(Y) - 6, idx = 32 * e + (Y >> e), frac = Y & ((1u << e) - 1);
    tone(idx, lo, hi);
    return (uint32_t)(((uint64_t)lo * ((1u << e) - frac) + (uint64_t)hi * frac + (1u << (e - 1))) >> e);
}

// One pixel of an HDR source in place.  in_lut32: three tables of n entries, one
// after the other; w: the luminance weights; the rest as color_xform_px.
template <typename Lut32, typename Tone, typename Out>
HG_XF_HD void color_tone_px(Lut32 in_lut32, int n, const int32_t (&w)[3], const Tone &tone, const Out &out_lut,
                            const int32_t (&m)[9], uint32_t &r, uint32_t &g, uint32_t &b) {
    const uint32_t l0 = in_lut32[r], l1 = in_lut32[n + g], l2 = in_lut32[2 * n + b];
    const uint64_t ysum = (uint64_t)(uint32_t)w[0] * l0 + (uint64_t)(uint32_t)w[1] * l1 + (uint64_t)(uint32_t)w[2] * l2;
    const uint32_t gain = color_tone_gain(tone, (uint32_t)((ysum + 8192) >> 14));
    auto scaled = [gain](uint32_t l) {
        const uint64_t v = ((uint64_t)l * gain + (1u << (kXfToneShift - 1))) >> kXfToneShift;
        return (int64_t)(v > 65535 ? 65535 : v);
    };
    color_xform_linear(out_lut, m, scaled(l0), scaled(l1), scaled(l2), r, g, b);
}

}  // namespace hg
