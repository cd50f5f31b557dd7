// gain_scale.hpp — the scaled gain-map HDR render's averaging of Q8 gain codes, the one
// statement of it in code: k_render_gain_scaled (render_gain_scaled.hip) and
// heifgpu_gain_average (api/gain.cpp) accumulate and divide through these functions, so the
// CPU suite runs the very arithmetic the GPU runs.  include/heifgpu.h states the contract
// ("Gain-map HDR render", the scaled call); tests/gain_scale_ref.py restates it in numpy.
//
//   avg(g) = floor((2 sum_j sum_i wy(Y, j) wx(X, i) g[cy + j][cx + i] + cw ch) / (2 cw ch))
//
// with the area weights of the scaled render and g a Q8 gain code, 0 .. 256 * 4095 < 2^20.
// The ranges are above what the colour channels' sums hold (samples of at most 12 bits):
// the weights of one output line add up to the window's side, so a line's column sum of g
// reaches 65535 * 256 * 4095 > 2^35, the whole sum 2^52 and the numerator 2^53.  A code is
// therefore carried as its two parts, g >> 8 (at most 4095) and g & 255, each of which is a
// sample of at most 12 bits and fits the sums a colour channel uses:
//   column sums   32 bits each:  at most 65535 * 4095 < 2^28
//   whole sums    64 bits each:  at most 65535^2 * 4095 < 2^44
// and the quotient is taken in two steps that each stay in the regime where a
// double-precision estimate corrected once in integers is exact (numerator below 2^46,
// quotient below 2^12: the estimate is off by less than 2^-39):
//   2 SH = qh den + rh                          (qh <= 4095)
//   256 rh + 2 SL + cw ch = ql den + rl         (below 512 den <= 2^42: ql <= 511)
//   avg = 256 qh + ql                           (num = 256 (2 SH) + 2 SL + cw ch)
// Nothing here is the colour channels' quotient with a wider type: no step leaves that regime.
#pragma once
#include <cstddef>
#include <cstdint>

#include "color_xform.hpp"  // HG_XF_HD

namespace hg {

constexpr uint32_t kGainScaleMaxCode = 256u * 4095u;  // the largest Q8 gain code (a 12-bit map)
constexpr uint32_t kGainScaleMaxSide = 65535;         // window and rendered sides

// the two parts of weighted gain codes: a thread's column sums (one output line, 32 bits)
// and an output pixel's whole sums (64 bits)
struct GsCol {
    uint32_t hi, lo;
};
struct GsSum {
    uint64_t hi, lo;
};

// The weight of window index k in an output index whose interval on the grid of
// 1 / (o * c) is [lo, hi) (lo = X * c, hi = lo + c): the overlap with [k o, (k + 1) o).
// Sides at most 65535: every product stays below 2^32.
HG_XF_HD uint32_t gs_weight(uint32_t k, uint32_t o, uint32_t lo, uint32_t hi) {
    const uint32_t a = (k + 1) * o, b = k * o;
    return (a < hi ? a : hi) - (b > lo ? b : lo);
}
// the window indices [k0, k1) that output index X of o reads from a window of c
HG_XF_HD void gs_footprint(uint32_t X, uint32_t c, uint32_t o, uint32_t &k0, uint32_t &k1) {
    k0 = X * c / o;
    k1 = ((X + 1) * c + o - 1) / o;
}

// w * g into a column sum (the weights of a line add up to at most 65535; g <= kGainScaleMaxCode:
// the masks change nothing and let the device's compiler take its 24-bit multiplier)
HG_XF_HD void gs_col_add(GsCol &s, uint32_t w, uint32_t g) {
    s.hi += (w & 0xffffu) * ((g >> 8) & 0xfffu);
    s.lo += (w & 0xffffu) * (g & 255u);
}
// w * column sum into the whole sum
HG_XF_HD void gs_add(GsSum &s, uint32_t w, uint32_t col_hi, uint32_t col_lo) {
    s.hi += (uint64_t)w * col_hi;
    s.lo += (uint64_t)w * col_lo;
}

// floor(num / den) and the remainder, for num < 2^46, 1 <= den <= 2^33 and a quotient below
// 2^12; inv_den = 1.0 / den.  num is exact in a double, inv_den and the product are each off
// by a relative 2^-53, so the estimate is off by less than 2^-39 and its floor by at most one.
HG_XF_HD uint32_t gs_div_small(uint64_t num, uint64_t den, double inv_den, uint64_t &rem) {
    uint32_t q = (uint32_t)((double)num * inv_den);
    int64_t r = (int64_t)(num - (uint64_t)q * den);
    if (r < 0) --q, r += (int64_t)den;
    else if (r >= (int64_t)den) ++q, r -= (int64_t)den;
    rem = (uint64_t)r;
    return q;
}

// The rounded average of a colour sample's whole sum (at most 4095 * cw * ch), den = 2 cw ch:
// k_render_scaled's quotient, here for the channels that ride beside the gain code.
HG_XF_HD uint32_t gs_average_small(uint64_t sum, uint64_t den, double inv_den) {
    uint64_t rem;
    return gs_div_small(2 * sum + (den >> 1), den, inv_den, rem);
}

// The rounded average of the gain codes of one output pixel: den = 2 cw ch.
HG_XF_HD uint32_t gs_average(const GsSum &s, uint64_t den, double inv_den) {
    uint64_t rh, rl;
    const uint32_t qh = gs_div_small(2 * s.hi, den, inv_den, rh);
    const uint32_t ql = gs_div_small(256 * rh + 2 * s.lo + (den >> 1), den, inv_den, rl);
    return 256u * qh + ql;
}

// Host: the averages of the window (cx, cy, cw, ch) of a W-wide array of codes (pitch
// entries a row) on an ow x oh grid, in the kernel's order: per output line the column
// sums over its rows, then per output pixel the sum over its columns, then the quotient.
// The caller has checked the window, the sizes (1 .. 65535) and the codes (<= kGainScaleMaxCode);
// col: cw entries of scratch.
inline void gs_average_window(const uint32_t *g, size_t pitch, uint32_t cx, uint32_t cy, uint32_t cw, uint32_t ch,
                              uint32_t ow, uint32_t oh, GsCol *col, uint32_t *out) {
    const uint64_t den = 2 * (uint64_t)cw * ch;
    const double inv_den = 1.0 / (double)den;
    for (uint32_t Y = 0; Y < oh; ++Y) {
        const uint32_t alo = Y * ch, ahi = alo + ch;
        uint32_t j0, j1;
        gs_footprint(Y, ch, oh, j0, j1);
        for (uint32_t i = 0; i < cw; ++i) col[i] = GsCol{0, 0};
        for (uint32_t j = j0; j < j1; ++j) {
            const uint32_t w = gs_weight(j, oh, alo, ahi);
            const uint32_t *row = g + (size_t)(cy + j) * pitch + cx;
            for (uint32_t i = 0; i < cw; ++i) gs_col_add(col[i], w, row[i]);
        }
        for (uint32_t X = 0; X < ow; ++X) {
            const uint32_t blo = X * cw, bhi = blo + cw;
            uint32_t i0, i1;
            gs_footprint(X, cw, ow, i0, i1);
            GsSum s = {0, 0};
            for (uint32_t i = i0; i < i1; ++i) gs_add(s, gs_weight(i, ow, blo, bhi), col[i].hi, col[i].lo);
            out[(size_t)Y * ow + X] = gs_average(s, den, inv_den);
        }
    }
}

}  // namespace hg
