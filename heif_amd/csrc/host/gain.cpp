// gain.cpp — see gain.hpp.
#include "gain.hpp"

#include <cmath>
#include <cstring>
#include <memory>

#include "../kernels/gain_xform.hpp"

namespace hg {
namespace {

int fail(int code, std::string &err, const char *msg) {
    err = msg;
    return code;
}
uint32_t be32(const uint8_t *p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }
uint32_t be16(const uint8_t *p) { return (uint32_t(p[0]) << 8) | p[1]; }
double rhu(double v) { return std::floor(v + 0.5); }

// the ST 2084 inverse EOTF of y = cd/m2 / 10000 in [0, 1]
double pq_inverse(double y) {
    const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0;
    const double c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
    const double p = std::pow(y > 0.0 ? y : 0.0, m1);
    return std::pow((c1 + c2 * p) / (1.0 + c3 * p), m2);
}
// the BT.709 inverse OETF
double f709(double v) { return v < 0.081 ? v / 4.5 : std::pow((v + 0.099) / 1.099, 1.0 / 0.45); }

bool invert3(const double (&a)[9], double (&o)[9]) {
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
    if (!(std::fabs(det) > 1e-12)) return false;
    const double c[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                         a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                         a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    for (int k = 0; k < 9; ++k) o[k] = c[k] / det;
    return true;
}

// color_transform_build's matrix recipe for the BT.2020 destination: inv(Dst) Src in double,
// rows normalised, Q14 rounded to nearest, the largest entry of a row adjusted to the sum 16384
int matrix_bt2020(const ColorSource &src, int32_t (&m)[9], std::string &err) {
    if (src.nclx && src.primaries == 9) {
        for (int k = 0; k < 9; ++k) m[k] = (k % 4 == 0) ? kXfMatrixOne : 0;
        return HEIFGPU_OK;
    }
    ColorSource dst;
    if (int rc = nclx_source(9, 8, dst, err)) return rc;
    double S[9], D[9], Di[9], M[9];
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) S[3 * k + c] = src.col[3 * c + k], D[3 * k + c] = dst.col[3 * c + k];
    if (!invert3(D, Di)) return fail(HEIFGPU_E_INVALID, err, "destination colourants");
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[3 * r + c] = Di[3 * r] * S[c] + Di[3 * r + 1] * S[3 + c] + Di[3 * r + 2] * S[6 + c];
    for (int r = 0; r < 3; ++r) {
        const double sum = M[3 * r] + M[3 * r + 1] + M[3 * r + 2];
        if (!(sum > 0.25 && sum < 4.0)) return fail(HEIFGPU_E_UNSUPPORTED, err, "source colourants out of range");
        for (int c = 0; c < 3; ++c) M[3 * r + c] /= sum;
    }
    for (int k = 0; k < 9; ++k) {
        if (!(std::fabs(M[k]) < 64.0)) return fail(HEIFGPU_E_UNSUPPORTED, err, "source colourants out of range");
        m[k] = int32_t(rhu(M[k] * kXfMatrixOne));
    }
    for (int r = 0; r < 3; ++r) {
        int big = 0;
        for (int c = 1; c < 3; ++c)
            if (m[3 * r + c] > m[3 * r + big]) big = c;
        m[3 * r + big] += kXfMatrixOne - (m[3 * r] + m[3 * r + 1] + m[3 * r + 2]);
    }
    return HEIFGPU_OK;
}

constexpr double kMaxLog2 = 8.0, kMaxOffset = 16.0;

}  // namespace

int gain_read(const uint8_t *p, size_t len, GainMeta &out, std::string &err) {
    out = GainMeta{};
    if (len < 5) return fail(HEIFGPU_E_PARSE, err, "tmap: payload shorter than its version fields");
    out.version = p[0];
    out.minimum_version = be16(p + 1);
    out.writer_version = be16(p + 3);
    if (out.version != 0) return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: version other than 0");
    if (out.minimum_version != 0) return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: minimum_version other than 0");
    if (len < 6) return fail(HEIFGPU_E_PARSE, err, "tmap: payload shorter than its flags");
    out.multichannel = (p[5] >> 7) & 1u;
    out.use_base_colour_space = (p[5] >> 6) & 1u;
    const size_t channels = out.multichannel ? 3 : 1;
    if (len < 22 + 40 * channels) return fail(HEIFGPU_E_PARSE, err, "tmap: payload shorter than its fields");
    // 2 headrooms, then five fractions of channel 0 (the other channels' denominators are checked too)
    bool zero_den = false;
    auto frac = [&](const uint8_t *q, bool is_signed) {
        const uint32_t n = be32(q), d = be32(q + 4);
        if (!d) {
            zero_den = true;
            return 0.0;
        }
        return (is_signed ? double(int32_t(n)) : double(n)) / double(d);
    };
    out.base_headroom = frac(p + 6, false);
    out.alternate_headroom = frac(p + 14, false);
    for (size_t c = 0; c < channels; ++c) {
        const uint8_t *q = p + 22 + 40 * c;
        const double v[5] = {frac(q, true), frac(q + 8, true), frac(q + 16, false), frac(q + 24, true), frac(q + 32, true)};
        if (c == 0) out.gain_min = v[0], out.gain_max = v[1], out.gamma = v[2], out.base_offset = v[3], out.alternate_offset = v[4];
    }
    if (zero_den) return fail(HEIFGPU_E_PARSE, err, "tmap: zero denominator");
    if (out.multichannel) return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: multichannel gain map");
    if (!out.use_base_colour_space) return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: gain applied in the alternate colour space");
    if (out.alternate_headroom <= out.base_headroom) return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: an HDR base image");
    if (!(out.gamma > 0.0)) return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: gamma not above 0");
    if (std::fabs(out.gain_min) > kMaxLog2 || std::fabs(out.gain_max) > kMaxLog2 || out.base_headroom > kMaxLog2 ||
        out.alternate_headroom > kMaxLog2)
        return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: |min|, |max| or a headroom above 8");
    if (std::fabs(out.base_offset) > kMaxOffset || std::fabs(out.alternate_offset) > kMaxOffset)
        return fail(HEIFGPU_E_UNSUPPORTED, err, "tmap: an offset above 16 in magnitude");
    return HEIFGPU_OK;
}

int gain_transform_build(const GainDesc &g, const ColorDesc &color, uint32_t gain_bits, uint32_t dst, uint32_t bits,
                         uint32_t encoding, uint32_t pq_bits, double headroom, double display_headroom,
                         double sdr_white, heifgpu_gain_transform &t, std::string &err) {
    if (dst > HEIFGPU_CS_BT2020) return fail(HEIFGPU_E_INVALID, err, "destination colour space");
    if (bits < 8 || bits > 12) return fail(HEIFGPU_E_INVALID, err, "transform depth outside 8..12");
    if (gain_bits < 8 || gain_bits > 12) return fail(HEIFGPU_E_UNSUPPORTED, err, "gain map depth outside 8..12");
    if (encoding > HEIFGPU_GAIN_PQ) return fail(HEIFGPU_E_INVALID, err, "encoding");
    if (encoding == HEIFGPU_GAIN_PQ && pq_bits != 10 && pq_bits != 12 && pq_bits != 16)
        return fail(HEIFGPU_E_INVALID, err, "pq_bits other than 10, 12, 16");
    if (!std::isfinite(headroom) || !std::isfinite(display_headroom) || !std::isfinite(sdr_white) || sdr_white > 10000.0)
        return fail(HEIFGPU_E_INVALID, err, "headroom, display_headroom or sdr_white not finite, or sdr_white above 10000");
    ColorSource src;
    if (int rc = color_source(color, src, err)) return rc;
    auto ct = std::make_unique<heifgpu_color_transform>();
    if (int rc = color_transform_build(src, dst == HEIFGPU_CS_BT2020 ? uint32_t(HEIFGPU_CS_SRGB) : dst, bits, *ct, err)) return rc;
    std::memset(&t, 0, sizeof(t));
    t.bits = bits, t.gain_bits = gain_bits, t.dst = dst, t.encoding = encoding;
    t.pq_bits = encoding == HEIFGPU_GAIN_PQ ? pq_bits : 0;
    std::memcpy(t.in_lut, ct->in_lut, sizeof(t.in_lut));
    if (dst == HEIFGPU_CS_BT2020) {
        if (int rc = matrix_bt2020(src, t.m, err)) return rc;
    } else {
        for (int k = 0; k < 9; ++k) t.m[k] = ct->m[k];
    }
    const int maxg = (1 << gain_bits) - 1;
    if (g.kind == HEIFGPU_GAIN_ISO) {
        GainMeta gm;
        if (int rc = gain_read(g.tmap.data(), g.tmap.size(), gm, err)) return rc;
        double w = 1.0;
        if (display_headroom > 0.0) {
            w = (std::log2(display_headroom) - gm.base_headroom) / (gm.alternate_headroom - gm.base_headroom);
            w = w >= 0.0 ? (w <= 1.0 ? w : 1.0) : 0.0;
        }
        t.kind = HEIFGPU_GAIN_ISO;
        t.weight = w;
        for (int v = 0; v <= maxg; ++v) {
            const double x = std::pow(double(v) / double(maxg), 1.0 / gm.gamma);
            const double tv = rhu(65536.0 * std::exp2(w * (gm.gain_min + (gm.gain_max - gm.gain_min) * x)));
            t.T[v] = uint32_t(tv <= double(kGainTMax) ? tv : double(kGainTMax));
        }
        t.k_b = int32_t(rhu(65535.0 * gm.base_offset));
        t.k_a = int32_t(rhu(65535.0 * gm.alternate_offset));
    } else {
        if (!(headroom >= 1.0 && headroom <= 256.0))
            return fail(HEIFGPU_E_INVALID, err, "an Apple gain map needs the caller's headroom, in [1, 256]");
        double hr = headroom;
        if (display_headroom > 0.0) hr = std::fmin(headroom, std::fmax(display_headroom, 1.0));
        t.kind = HEIFGPU_GAIN_APPLE;
        t.weight = 1.0;
        t.headroom = hr;
        for (int v = 0; v <= maxg; ++v) t.T[v] = uint32_t(rhu(65536.0 * (1.0 + (hr - 1.0) * f709(double(v) / double(maxg)))));
    }
    t.T[maxg + 1] = t.T[maxg];
    if (encoding == HEIFGPU_GAIN_PQ) {
        const double white = sdr_white > 0.0 ? sdr_white : 203.0, maxp = double((1u << pq_bits) - 1);
        t.sdr_white = white;
        for (int k = 0; k < kGainEEntries; ++k) {
            const double nits = std::fmin(white * double(xf_tone_node(k)) / 65535.0, 10000.0);
            t.E[k] = uint32_t(rhu(256.0 * maxp * pq_inverse(nits / 10000.0)));
        }
    }
    return HEIFGPU_OK;
}

const char *gain_transform_invalid(const heifgpu_gain_transform &t) {
    if (t.bits < 8 || t.bits > 12 || t.gain_bits < 8 || t.gain_bits > 12) return "gain transform: depth outside 8..12";
    if (t.encoding > HEIFGPU_GAIN_PQ) return "gain transform: encoding";
    if (t.encoding == HEIFGPU_GAIN_PQ && t.pq_bits != 10 && t.pq_bits != 12 && t.pq_bits != 16) return "gain transform: pq_bits";
    const int32_t kmax = 16 * 65535;
    if (t.k_b > kmax || t.k_b < -kmax || t.k_a > kmax || t.k_a < -kmax) return "gain transform: an offset above 16 * 65535";
    for (uint32_t v = 0; v < (1u << t.gain_bits) + 1; ++v)
        if (t.T[v] > kGainTMax) return "gain transform: a T entry above 2^24";
    if (t.encoding == HEIFGPU_GAIN_PQ)
        for (int k = 0; k < kGainEEntries; ++k)
            if (t.E[k] > kGainTMax) return "gain transform: an E entry above 2^24";
    for (int k = 0; k < 9; ++k)
        if (t.m[k] > 64 * kXfMatrixOne || t.m[k] < -64 * kXfMatrixOne) return "gain transform: a matrix entry above 64";
    return nullptr;
}

}  // namespace hg
