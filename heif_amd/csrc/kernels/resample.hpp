// resample.hpp — the bilinear / bicubic resampling of the filtered renders, stated once.
// k_render_resampled (resample.hip) and the host hooks heifgpu_resample_coeffs /
// heifgpu_resample_apply (api/resample.cpp) both call these functions, so the CPU suite
// runs the arithmetic the GPU runs.  include/heifgpu.h has the contract: Pillow's
// precompute_coeffs in binary64, operation for operation, coefficients normalised by a
// division and rounded to P fractional bits, then two integer passes (along D's x, then
// along its y) with a rounding and a clip after each.
//
// Every product that feeds a sum is rounded on its own: the functions run with
// floating-point contraction off (device code would otherwise fuse a * b + c into one
// rounding and part from Pillow in the last bit of a coefficient).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ inline
#else
#define RS_HD inline
#endif
#if defined(__clang__)
#define RS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RS_NO_CONTRACT  // (ISO mode of the other compilers contracts nothing)
#endif

namespace hg {

enum : int { RS_AREA = 0, RS_BILINEAR = 1, RS_BICUBIC = 2 };

// the fractional bits of a coefficient at depth B (8: Pillow's PRECISION_BITS)
RS_HD int rs_precision(int bits) { return 32 - 2 - (bits > 8 ? bits : 8); }

// One axis of a resampling: window [in0, in1) of a side of in_size samples onto out samples.
struct RsAxis {
    double in0, scale, ss, support;
    int32_t in_size, out, filter, ksize;  // ksize: Pillow's row length, (int)ceil(support) * 2 + 1
};

RS_HD RsAxis rs_axis(int in_size, int in0, int in1, int out, int filter) {
    RS_NO_CONTRACT
    RsAxis a;
    a.in0 = (double)in0;
    a.scale = (double)(in1 - in0) / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = (filter == RS_BICUBIC ? 2.0 : 1.0) * fs;
    a.ss = 1.0 / fs;
    a.in_size = in_size;
    a.out = out;
    a.filter = filter;
    int c = (int)a.support;
    if ((double)c < a.support) ++c;
    a.ksize = 2 * c + 1;
    return a;
}

RS_HD double rs_center(const RsAxis &a, int X) {
    RS_NO_CONTRACT
    const double step = ((double)X + 0.5) * a.scale;
    return a.in0 + step;
}

// the taps of output X: samples [lo, hi) of the side
RS_HD void rs_bounds(const RsAxis &a, int X, int &lo, int &hi) {
    RS_NO_CONTRACT
    const double center = rs_center(a, X);
    lo = (int)(center - a.support + 0.5);
    if (lo < 0) lo = 0;
    hi = (int)(center + a.support + 0.5);
    if (hi > a.in_size) hi = a.in_size;
}

RS_HD double rs_filter(int filter, double x) {
    RS_NO_CONTRACT
    if (x < 0.0) x = -x;
    if (filter == RS_BICUBIC) {
        const double a = -0.5;
        if (x < 1.0) {
            const double p = (a + 2.0) * x;
            const double q = (p - (a + 3.0)) * x;
            const double r = q * x;
            return r + 1.0;
        }
        if (x < 2.0) {
            const double p = (x - 5.0) * x;
            const double q = (p + 8.0) * x;
            return (q - 4.0) * a;
        }
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

// the weight of sample `at` for an output centred at `center`, before normalisation
RS_HD double rs_weight(const RsAxis &a, double center, int at) {
    RS_NO_CONTRACT
    const double d = (double)at - center + 0.5;
    return rs_filter(a.filter, d * a.ss);
}

// the sum of an output's weights, left to right
RS_HD double rs_weight_sum(const RsAxis &a, double center, int lo, int hi) {
    RS_NO_CONTRACT
    double ww = 0.0;
    for (int at = lo; at < hi; ++at) ww += rs_weight(a, center, at);
    return ww;
}

// the integer coefficient of a weight: normalised (a division), P fractional bits, rounded half away
RS_HD int32_t rs_coeff(double w, double ww, int P) {
    RS_NO_CONTRACT
    if (ww != 0.0) w = w / ww;
    const double s = w * (double)(1 << P);
    return w < 0.0 ? (int32_t)(-0.5 + s) : (int32_t)(0.5 + s);
}

// a pass's sum starts at rs_half(P), takes k * sample per tap and ends in rs_round
RS_HD int32_t rs_half(int P) { return (int32_t)1 << (P - 1); }
RS_HD int32_t rs_round(int32_t acc, int P, int32_t maxv) {
    const int32_t v = acc >> P;  // arithmetic
    return v < 0 ? 0 : v > maxv ? maxv : v;
}

}  // namespace hg
