// gain_xform.hpp — the gain-map HDR render's per-pixel arithmetic, the one statement of it
// in code: k_render_gain (render_gain.hip) and heifgpu_gain_apply (api/gain.cpp) both call
// gain_px, and both sample the gain map through gain_tap / gain_sample, so the CPU suite
// runs the very functions the GPU runs.  include/heifgpu.h states the contract ("Gain-map
// HDR render"); tests/gain_ref.py restates it in numpy.
//
//   position   t = floor(128 (2 s + 1) Wg / W) - 128,  i = t >> 8 (arithmetic), f = t & 255
//              (which are floor(n / d) and floor(256 (n - i d) / d) of n = (2 s + 1) Wg - W, d = 2 W)
//   sample     g = ((256 - fy) ((256 - fx) G00 + fx G01) + fy ((256 - fx) G10 + fx G11) + 128) >> 8
//   multiplier M = (T[g >> 8] (256 - (g & 255)) + T[(g >> 8) + 1] (g & 255) + 128) >> 8
//   apply      H_c = clamp((((L_c + k_b) M + 2^15) >> 16) - k_a, 0, 2^24 - 1),  L_c = in_lut[c][code_c]
//   matrix     H'_k = clamp((m[3k] H_0 + m[3k+1] H_1 + m[3k+2] H_2 + 8192) >> 14, 0, 2^24 - 1)
//   encode     linear: binary16(fmul(float(H'), c));  PQ: (E at H' on the floating index + 128) >> 8
#pragma once
#include <cstdint>
#include <cstring>

#include "color_xform.hpp"

namespace hg {

constexpr int kGainEEntries = 641;                   // E's nodes: 0 .. 63, then 32 per octave up to 2^24 (xf_tone_node)
constexpr int kGainEPairs = kGainEEntries - 1;       // the index is at most 639
constexpr uint32_t kGainMaxLevel = (1u << 24) - 1;   // the largest H and H'
constexpr uint32_t kGainTOne = 1u << 16;             // T's fractional bits: a multiplier of 1
constexpr uint32_t kGainTMax = 1u << 24;             // the largest T entry (a multiplier of 256)
constexpr int kGainMaxSide = 65535;                  // W, H, Wg, Hg: 128 (2 s + 1) Wg stays below 2^40
enum : int { GAIN_ENC_LINEAR = 0, GAIN_ENC_PQ = 1 };

// what the per-pixel formula reads beside the tables
struct GainParams {
    int32_t m[9];      // Q14
    int32_t k_b, k_a;  // the offsets in units of 1 / 65535 of SDR white, |k| <= 16 * 65535
    int32_t encoding;  // GAIN_ENC_*
};

// the two gain-map columns (or rows) that decoded base column (row) s reads, and the weight of the second
struct GainTap {
    int32_t i0, i1, f;
};

// s in [0, W), W and Wg in [1, kGainMaxSide], inv_w = 1.0 / W.  The quotient is a
// double-precision estimate (A < 2^40 is exact in a double, the product is off by less
// than one) corrected exactly in integers, as k_render_scaled's quotient is.
// (in two steps, which a walk shares: q = floor(A / W) and its remainder, then the taps of q)
HG_XF_HD uint32_t gain_tap_quotient(int s, int W, int Wg, double inv_w, uint32_t &rem_out) {
    const uint64_t A = (uint64_t)(128u * (2u * (uint32_t)s + 1u)) * (uint32_t)Wg;
    uint64_t q = (uint64_t)((double)A * inv_w);
    int64_t rem = (int64_t)(A - q * (uint32_t)W);
    if (rem < 0) --q, rem += W;
    else if (rem >= (int64_t)W) ++q, rem -= W;
    rem_out = (uint32_t)rem;
    return (uint32_t)q;  // q <= 256 Wg < 2^24
}
HG_XF_HD GainTap gain_tap_of(uint32_t q, int Wg) {
    const int32_t t = (int32_t)q - 128;
    const int32_t i = t >> 8;
    GainTap r;
    r.f = t & 255;
    r.i0 = i < 0 ? 0 : i > Wg - 1 ? Wg - 1 : i;
    r.i1 = i + 1 < 0 ? 0 : i + 1 > Wg - 1 ? Wg - 1 : i + 1;
    return r;
}
HG_XF_HD GainTap gain_tap(int s, int W, int Wg, double inv_w) {
    uint32_t rem;
    return gain_tap_of(gain_tap_quotient(s, W, Wg, inv_w, rem), Wg);
}

// gain_tap along a walk that mostly moves to a neighbouring position (the source rows of
// k_render_gain_scaled's first stage): A = 128 (2 s + 1) Wg = q W + rem is kept exactly, and
// a step of s by one adds or takes 256 Wg = dq W + dr.  Integers only after the first position.
struct GainTapWalk {
    int32_t s;        // the position the state is at
    uint32_t q, rem;  // floor(A / W) and A mod W
    uint32_t dq, dr;
};
HG_XF_HD void gain_walk_start(GainTapWalk &w, int s, int W, int Wg, double inv_w) {
    w.s = s;
    w.q = gain_tap_quotient(s, W, Wg, inv_w, w.rem);
    w.dq = 256u * (uint32_t)Wg / (uint32_t)W;
    w.dr = 256u * (uint32_t)Wg - w.dq * (uint32_t)W;
}
// the state at s: a step from a neighbouring position, a fresh start from anywhere else
HG_XF_HD void gain_walk_seek(GainTapWalk &w, int s, int W, int Wg, double inv_w) {
    if (s == w.s + 1) {
        w.q += w.dq, w.rem += w.dr;
        if (w.rem >= (uint32_t)W) w.rem -= (uint32_t)W, ++w.q;
        w.s = s;
    } else if (s == w.s - 1) {
        w.q -= w.dq;
        if (w.rem < w.dr) w.rem += (uint32_t)W, --w.q;
        w.rem -= w.dr;
        w.s = s;
    } else if (s != w.s) {
        gain_walk_start(w, s, W, Wg, inv_w);
    }
}

// the Q8 gain code, 0 .. 256 maxg, of the four samples (at most 4095 each: below 2^28 + 128)
HG_XF_HD uint32_t gain_sample(uint32_t g00, uint32_t g01, uint32_t g10, uint32_t g11, uint32_t fx, uint32_t fy) {
    const uint32_t top = (256u - fx) * g00 + fx * g01, bot = (256u - fx) * g10 + fx * g11;
    return ((256u - fy) * top + fy * bot + 128u) >> 8;
}
// gain_sample in its two steps, for a walk that keeps a map row's two taps as their weighted
// sum: gain_sample(g00, g01, g10, g11, fx, fy) == gain_sample_rows(gain_sample_row(g00, g01, fx),
// gain_sample_row(g10, g11, fx), fy).  Every factor is below 2^24 even for samples of 16 bits
// (256 * 65535 < 2^24), and is written so: the masks change nothing and let the device's
// compiler take its 24-bit multiplier (a quarter of the 32-bit one's cycles).
HG_XF_HD uint32_t gain_mul24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }
HG_XF_HD uint32_t gain_sample_row(uint32_t g0, uint32_t g1, uint32_t fx) {
    return gain_mul24(256u - fx, g0) + gain_mul24(fx, g1);
}
HG_XF_HD uint32_t gain_sample_rows(uint32_t top, uint32_t bot, uint32_t fy) {
    return (gain_mul24(256u - fy, top) + gain_mul24(fy, bot) + 128u) >> 8;
}

// M of T[i], T[i + 1] (each at most kGainTMax) and f = g & 255
HG_XF_HD uint32_t gain_multiplier(uint32_t lo, uint32_t hi, uint32_t f) {
    return (uint32_t)(((uint64_t)lo * (256u - f) + (uint64_t)hi * f + 128u) >> 8);
}

HG_XF_HD int64_t gain_level(int64_t L, uint32_t M, int32_t k_b, int32_t k_a) {
    const int64_t v = (((L + k_b) * (int64_t)M + 32768) >> 16) - k_a;
    return v < 0 ? 0 : v > (int64_t)kGainMaxLevel ? (int64_t)kGainMaxLevel : v;
}

HG_XF_HD uint32_t gain_matrix_row(const int32_t *m, int64_t h0, int64_t h1, int64_t h2) {
    const int64_t v = (m[0] * h0 + m[1] * h1 + m[2] * h2 + 8192) >> 14;
    return (uint32_t)(v < 0 ? 0 : v > (int64_t)kGainMaxLevel ? (int64_t)kGainMaxLevel : v);
}

// binary32 -> binary16 bits, round to nearest even, gradual underflow; f finite and not negative
// and below 65520 (the callers give at most 256).  In integers on the bits, on the device too:
// with the hardware's conversion behind the product 2 samples in 46080 differed from numpy's
// two roundings on the MI355X (a product rounded once to binary16 would explain it); nothing
// can merge this conversion into the product.
HG_XF_HD uint32_t gain_half_bits(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    const int32_t e = (int32_t)(u >> 23) - 127 + 15;  // the half's biased exponent
    uint32_t man = u & 0x7fffffu;
    if (e <= 0) {  // a subnormal half (or zero): the 24-bit significand shifted down by 14 - e
        if (e < -10) return 0;
        man |= 0x800000u;
        const int sh = 14 - e;  // 14 .. 24
        const uint32_t q = man >> sh, r = man & ((1u << sh) - 1), half = 1u << (sh - 1);
        return q + ((r > half || (r == half && (q & 1u))) ? 1u : 0u);
    }
    const uint32_t q = ((uint32_t)e << 10) | (man >> 13), r = man & 0x1fffu;
    return q + ((r > 0x1000u || (r == 0x1000u && (q & 1u))) ? 1u : 0u);  // (a carry runs into the exponent: right)
}

// the linear encoding of a level: 1.0 is SDR white (level 65535)
HG_XF_HD uint32_t gain_encode_linear(uint32_t level, float scale) {
#pragma clang fp contract(off)
    return gain_half_bits((float)level * scale);
}
// c, the binary32 nearest to 1 / 65535
constexpr float kGainLinearScale = 1.0f / 65535.0f;

// the PQ code of a level: E on the floating index (color_tone_gain's interpolation), 8 fractional bits
template <typename Pairs>
HG_XF_HD uint32_t gain_encode_pq(const Pairs &E, uint32_t level) {
    return (color_tone_gain(E, level) + 128u) >> 8;
}

// One pixel in place.  in_lut: three tables of n = 1 << B entries, one after the other; T and E
// fetch an entry and its successor (XfToneLut / XfTonePairs); r, g, b: codes 0 .. n - 1 in,
// binary16 bits or PQ codes out; gq: the pixel's Q8 gain code (gain_sample).
template <typename Lut, typename TFetch, typename EFetch>
HG_XF_HD void gain_px(Lut in_lut, int n, const TFetch &T, const EFetch &E, const GainParams &p, uint32_t gq, uint32_t &r,
                      uint32_t &g, uint32_t &b) {
    uint32_t lo, hi;
    T(gq >> 8, lo, hi);
    const uint32_t M = gain_multiplier(lo, hi, gq & 255u);
    const int64_t h0 = gain_level(in_lut[r], M, p.k_b, p.k_a), h1 = gain_level(in_lut[n + g], M, p.k_b, p.k_a),
                  h2 = gain_level(in_lut[2 * n + b], M, p.k_b, p.k_a);
    const uint32_t o0 = gain_matrix_row(p.m, h0, h1, h2), o1 = gain_matrix_row(p.m + 3, h0, h1, h2),
                   o2 = gain_matrix_row(p.m + 6, h0, h1, h2);
    if (p.encoding == GAIN_ENC_PQ) {
        r = gain_encode_pq(E, o0), g = gain_encode_pq(E, o1), b = gain_encode_pq(E, o2);
    } else {
        r = gain_encode_linear(o0, kGainLinearScale), g = gain_encode_linear(o1, kGainLinearScale),
        b = gain_encode_linear(o2, kGainLinearScale);
    }
}

}  // namespace hg
