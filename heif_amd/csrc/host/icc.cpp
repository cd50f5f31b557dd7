// icc.cpp — ICC matrix/TRC profile reader, nclx colour descriptions and the
// tables of heifgpu_color_transform (include/heifgpu.h states every formula).
#include "icc.hpp"

#include <cmath>
#include <cstring>

#include "../kernels/color_xform.hpp"

namespace hg {
namespace {

uint32_t be32(const uint8_t *p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }
uint32_t be16(const uint8_t *p) { return (uint32_t(p[0]) << 8) | p[1]; }
double s15f16(const uint8_t *p) { return double(int32_t(be32(p))) / 65536.0; }
constexpr uint32_t tag(char a, char b, char c, char d) {
    return (uint32_t(uint8_t(a)) << 24) | (uint32_t(uint8_t(b)) << 16) | (uint32_t(uint8_t(c)) << 8) | uint8_t(d);
}

int fail(int code, std::string &err, const char *msg) {
    err = msg;
    return code;
}

// IEC 61966-2-1 as an ICC 'para' type 3 would state it
Trc srgb_trc() {
    Trc t;
    t.kind = Trc::PARA;
    t.para_type = 3;
    t.g = 2.4, t.a = 1.0 / 1.055, t.b = 0.055 / 1.055, t.c = 1.0 / 12.92, t.d = 0.04045;
    return t;
}

double srgb_encode(double x) { return x <= 0.0031308 ? 12.92 * x : 1.055 * std::pow(x, 1.0 / 2.4) - 0.055; }

double pow_pos(double base, double g) { return base > 0.0 ? std::pow(base, g) : 0.0; }

bool invert3(const double (&a)[9], double (&o)[9]) {
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
    if (!(std::fabs(det) > 1e-12) || !std::isfinite(det)) return false;
    o[0] = c0 / det, o[1] = (a[2] * a[7] - a[1] * a[8]) / det, o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = c1 / det, o[4] = (a[0] * a[8] - a[2] * a[6]) / det, o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = c2 / det, o[7] = (a[1] * a[6] - a[0] * a[7]) / det, o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
    return true;
}

void mul3(const double (&a)[9], const double (&b)[9], double (&o)[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[3 * r + c] = a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c];
}

// the destinations' colourants, X Y Z of R, G, B in s15.16 (include/heifgpu.h)
const int32_t kDst[2][9] = {
    {0x6FA2, 0x38F5, 0x0390, 0x6299, 0xB785, 0x18DA, 0x24A0, 0x0F84, 0xB6CF},
    {0x83DF, 0x3DBF, int32_t(0xFFFFFFBB), 0x4ABF, 0xB137, 0x0AB9, 0x2838, 0x110B, 0xC8B9},
};

int read_trc(const uint8_t *p, size_t len, Trc &t, std::string &err) {
    if (len < 12) return fail(HEIFGPU_E_PARSE, err, "ICC: TRC tag shorter than its header");
    const uint32_t type = be32(p);
    if (type == tag('c', 'u', 'r', 'v')) {
        const uint32_t n = be32(p + 8);
        if (n > (len - 12) / 2) return fail(HEIFGPU_E_PARSE, err, "ICC: curv count beyond its tag");
        if (n == 0) {
            t.kind = Trc::IDENTITY;
        } else if (n == 1) {
            t.kind = Trc::GAMMA;
            t.g = double(be16(p + 12)) / 256.0;
        } else {
            t.kind = Trc::TABLE;
            t.table.resize(n);
            for (uint32_t i = 0; i < n; ++i) t.table[i] = uint16_t(be16(p + 12 + 2 * size_t(i)));
        }
        return HEIFGPU_OK;
    }
    if (type == tag('p', 'a', 'r', 'a')) {
        const uint32_t fn = be16(p + 8);
        if (fn > 4) return fail(HEIFGPU_E_UNSUPPORTED, err, "ICC: para function type above 4");
        static const int count[5] = {1, 3, 4, 5, 7};
        if (len < 12 + 4 * size_t(count[fn])) return fail(HEIFGPU_E_PARSE, err, "ICC: para parameters beyond their tag");
        double v[7] = {1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < count[fn]; ++i) v[i] = s15f16(p + 12 + 4 * i);
        t.kind = Trc::PARA;
        t.para_type = int(fn);
        t.g = v[0], t.a = v[1], t.b = v[2];
        // table 68: type 2 has c as its offset; types 3, 4 have c, d (and e, f)
        t.c = v[3], t.d = v[4], t.e = v[5], t.f = v[6];
        return HEIFGPU_OK;
    }
    return fail(HEIFGPU_E_UNSUPPORTED, err, "ICC: TRC tag is neither curv nor para");
}

}  // namespace

double Trc::eval(double x) const {
    switch (kind) {
    case IDENTITY: return x;
    case GAMMA: return pow_pos(x, g);
    case TABLE: {
        const size_t n = table.size();
        const double pos = std::fmin(std::fmax(x, 0.0), 1.0) * double(n - 1);
        size_t i = size_t(pos);
        if (i >= n - 1) i = n - 2;
        const double fr = pos - double(i);
        return (double(table[i]) * (1.0 - fr) + double(table[i + 1]) * fr) / 65535.0;
    }
    default: break;
    }
    const double lin = pow_pos(a * x + b, g);
    switch (para_type) {
    case 0: return pow_pos(x, g);
    case 1: return a != 0.0 && x >= -b / a ? lin : 0.0;
    case 2: return a != 0.0 && x >= -b / a ? lin + c : c;
    case 3: return x >= d ? lin : c * x;
    default: return x >= d ? lin + e : c * x + f;
    }
}

int icc_read(const uint8_t *p, size_t len, ColorSource &out, std::string &err) {
    if (!p || len < 132) return fail(HEIFGPU_E_PARSE, err, "ICC: profile shorter than its header");
    const size_t size = be32(p);
    if (size > len) return fail(HEIFGPU_E_PARSE, err, "ICC: size field beyond the box");
    if (size < 132) return fail(HEIFGPU_E_PARSE, err, "ICC: size field below the header");
    if (be32(p + 36) != tag('a', 'c', 's', 'p')) return fail(HEIFGPU_E_PARSE, err, "ICC: no acsp signature");
    if (be32(p + 16) != tag('R', 'G', 'B', ' ')) return fail(HEIFGPU_E_UNSUPPORTED, err, "ICC: data space is not RGB");
    if (be32(p + 20) != tag('X', 'Y', 'Z', ' ')) return fail(HEIFGPU_E_UNSUPPORTED, err, "ICC: PCS is not XYZ");
    const size_t count = be32(p + 128);
    if (count > (size - 132) / 12) return fail(HEIFGPU_E_PARSE, err, "ICC: tag table beyond the profile");
    static const uint32_t want[6] = {tag('r', 'X', 'Y', 'Z'), tag('g', 'X', 'Y', 'Z'), tag('b', 'X', 'Y', 'Z'),
                                     tag('r', 'T', 'R', 'C'), tag('g', 'T', 'R', 'C'), tag('b', 'T', 'R', 'C')};
    size_t off[6] = {}, ln[6] = {};
    bool have[6] = {}, lut = false;
    for (size_t k = 0; k < count; ++k) {
        const uint8_t *e = p + 132 + 12 * k;
        const uint32_t sig = be32(e);
        const size_t o = be32(e + 4), l = be32(e + 8);
        if (o > size || l > size - o) return fail(HEIFGPU_E_PARSE, err, "ICC: tag offset or length outside the profile");
        if (sig == tag('A', '2', 'B', '0')) lut = true;
        for (int w = 0; w < 6; ++w)
            if (sig == want[w] && !have[w]) have[w] = true, off[w] = o, ln[w] = l;
    }
    for (int w = 0; w < 6; ++w)
        if (!have[w])
            return fail(HEIFGPU_E_UNSUPPORTED, err,
                        lut ? "ICC: LUT-based profile (A2B0 without colourants)" : "ICC: not a matrix/TRC profile");
    out = ColorSource{};
    for (int c = 0; c < 3; ++c) {
        if (ln[c] < 20) return fail(HEIFGPU_E_PARSE, err, "ICC: colourant tag shorter than an XYZType");
        const uint8_t *q = p + off[c];
        if (be32(q) != tag('X', 'Y', 'Z', ' ')) return fail(HEIFGPU_E_PARSE, err, "ICC: colourant tag is not an XYZType");
        for (int k = 0; k < 3; ++k) out.col[3 * c + k] = s15f16(q + 8 + 4 * k);
    }
    for (int c = 0; c < 3; ++c)
        if (int rc = read_trc(p + off[3 + c], ln[3 + c], out.trc[c], err)) return rc;
    return HEIFGPU_OK;
}

// chromaticities x y of R, G, B (H.273 table 2; primaries 1, 9 or 12); the white is D65 for all three
static bool nclx_xy(uint32_t primaries, double (&xy)[6]) {
    if (primaries == 1) {
        const double v[6] = {0.640, 0.330, 0.300, 0.600, 0.150, 0.060};
        std::memcpy(xy, v, sizeof(xy));
    } else if (primaries == 9) {
        const double v[6] = {0.708, 0.292, 0.170, 0.797, 0.131, 0.046};
        std::memcpy(xy, v, sizeof(xy));
    } else if (primaries == 12) {
        const double v[6] = {0.680, 0.320, 0.265, 0.690, 0.150, 0.060};
        std::memcpy(xy, v, sizeof(xy));
    } else {
        return false;
    }
    return true;
}

// chromaticities to XYZ: the columns P (x/y, 1, z/y), and the scales S that make R = G = B = 1
// the D65 white W (the Y row of the RGB -> XYZ matrix is S itself)
static bool nclx_xyz(const double (&xy)[6], double (&P)[9], double (&S)[3], double (&W)[3]) {
    const double wx = 0.3127, wy = 0.3290;
    W[0] = wx / wy, W[1] = 1.0, W[2] = (1.0 - wx - wy) / wy;
    double Pi[9];
    for (int c = 0; c < 3; ++c) {
        const double x = xy[2 * c], y = xy[2 * c + 1];
        P[c] = x / y, P[3 + c] = 1.0, P[6 + c] = (1.0 - x - y) / y;
    }
    if (!invert3(P, Pi)) return false;
    for (int c = 0; c < 3; ++c) S[c] = Pi[3 * c] * W[0] + Pi[3 * c + 1] * W[1] + Pi[3 * c + 2] * W[2];
    return true;
}

int nclx_source(uint32_t primaries, uint32_t transfer, ColorSource &out, std::string &err) {
    out = ColorSource{};
    out.nclx = true;
    if (primaries == 2) primaries = 1;  // unspecified: sRGB
    if (transfer == 2) transfer = 13;
    double xy[6];
    if (!nclx_xy(primaries, xy)) return fail(HEIFGPU_E_UNSUPPORTED, err, "nclx: colour_primaries other than 1, 2, 9, 12");
    out.primaries = primaries;
    switch (transfer) {
    case 1: case 6: case 13: case 14: case 15:
        for (Trc &t : out.trc) t = srgb_trc();
        break;
    case 8: break;  // linear: the identity
    case 4:
        for (Trc &t : out.trc) t.kind = Trc::GAMMA, t.g = 2.2;
        break;
    case 16: case 18:
        return fail(HEIFGPU_E_UNSUPPORTED, err,
                    "nclx: PQ / HLG transfer needs tone mapping (heifgpu_color_transform_make_hdr, tone_map=\"bt2390\")");
    default: return fail(HEIFGPU_E_UNSUPPORTED, err, "nclx: transfer_characteristics not supported");
    }
    double P[9], S[3], W[3];
    if (!nclx_xyz(xy, P, S, W)) return fail(HEIFGPU_E_PARSE, err, "nclx: singular primaries");
    // Bradford from D65 to the ICC D50 white
    const double B[9] = {0.8951, 0.2664, -0.1614, -0.7502, 1.7135, 0.0367, 0.0389, -0.0685, 1.0296};
    const double D50[3] = {double(0xF6D6) / 65536.0, 1.0, double(0xD32D) / 65536.0};
    double Bi[9], ls[3], ld[3];
    invert3(B, Bi);
    for (int r = 0; r < 3; ++r) {
        ls[r] = B[3 * r] * W[0] + B[3 * r + 1] * W[1] + B[3 * r + 2] * W[2];
        ld[r] = B[3 * r] * D50[0] + B[3 * r + 1] * D50[1] + B[3 * r + 2] * D50[2];
    }
    double scaled[9], A[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) scaled[3 * r + c] = ld[r] / ls[r] * B[3 * r + c];
    mul3(Bi, scaled, A);
    for (int c = 0; c < 3; ++c) {
        const double X = P[c] * S[c], Y = P[3 + c] * S[c], Z = P[6 + c] * S[c];
        for (int k = 0; k < 3; ++k) out.col[3 * c + k] = A[3 * k] * X + A[3 * k + 1] * Y + A[3 * k + 2] * Z;
    }
    return HEIFGPU_OK;
}

int color_source(const ColorDesc &c, ColorSource &out, std::string &err) {
    if (c.has_icc) return icc_read(c.icc.data(), c.icc.size(), out, err);
    return nclx_source(c.has_nclx ? c.primaries : 2, c.has_nclx ? c.transfer : 2, out, err);
}

int color_transform_build(const ColorSource &src, uint32_t dst, uint32_t bits, heifgpu_color_transform &t,
                          std::string &err) {
    if (dst > HEIFGPU_CS_DISPLAY_P3) return fail(HEIFGPU_E_INVALID, err, "destination colour space");
    if (bits < 8 || bits > 12) return fail(HEIFGPU_E_INVALID, err, "transform depth outside 8..12");
    std::memset(&t, 0, sizeof(t));
    t.bits = bits;
    t.dst = dst;
    const int n = 1 << bits, maxv = n - 1;
    auto rhu = [](double v) { return std::floor(v + 0.5); };
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < n; ++v) {
            double f = src.trc[c].eval(double(v) / double(maxv));
            f = f >= 0.0 ? (f <= 1.0 ? f : 1.0) : 0.0;  // (a NaN becomes 0)
            t.in_lut[c][v] = uint16_t(rhu(65535.0 * f));
        }
    for (int i = 0; i < kXfOutEntries; ++i) {
        const int l = 16 * i < 65535 ? 16 * i : 65535;
        t.out_lut[i] = uint16_t(rhu(16.0 * maxv * srgb_encode(double(l) / 65535.0)));
    }
    const bool own = src.nclx && src.primaries == (dst == HEIFGPU_CS_SRGB ? 1u : 12u);
    if (own) {
        for (int k = 0; k < 9; ++k) t.m[k] = t.m_rounded[k] = (k % 4 == 0) ? kXfMatrixOne : 0;
    } else {
        double S[9], D[9], Di[9], M[9];
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) {
                S[3 * k + c] = src.col[3 * c + k];
                D[3 * k + c] = double(kDst[dst][3 * c + k]) / 65536.0;
            }
        if (!invert3(D, Di)) return fail(HEIFGPU_E_INVALID, err, "destination colourants");
        mul3(Di, S, M);
        // the source's white onto the destination's: the s15.16 colourants of two spaces do not sum
        // to the same white (sRGB's to F6DB FFFE D339, Display P3's to F6D6 10001 D32D), which
        // would leave row sums of 1 +- 3e-4 and a fix-up of up to 5 units on one entry
        for (int r = 0; r < 3; ++r) {
            const double sum = M[3 * r] + M[3 * r + 1] + M[3 * r + 2];
            if (!(sum > 0.25 && sum < 4.0)) return fail(HEIFGPU_E_UNSUPPORTED, err, "source colourants out of range");
            for (int c = 0; c < 3; ++c) M[3 * r + c] /= sum;
        }
        for (int k = 0; k < 9; ++k) {
            if (!(std::fabs(M[k]) < 64.0)) return fail(HEIFGPU_E_UNSUPPORTED, err, "source colourants out of range");
            t.m_rounded[k] = t.m[k] = int32_t(rhu(M[k] * kXfMatrixOne));
        }
        for (int r = 0; r < 3; ++r) {
            int big = 0;
            for (int c = 1; c < 3; ++c)
                if (t.m[3 * r + c] > t.m[3 * r + big]) big = c;
            t.m[3 * r + big] += kXfMatrixOne - (t.m[3 * r] + t.m[3 * r + 1] + t.m[3 * r + 2]);
        }
    }
    bool ident = true;
    for (int k = 0; k < 9; ++k) ident = ident && t.m[k] == ((k % 4 == 0) ? kXfMatrixOne : 0);
    for (int c = 0; c < 3 && ident; ++c)
        for (int v = 0; v < n && ident; ++v)
            ident = color_xform_encode(XfOutLut<const uint16_t *>{t.out_lut},
                                       color_xform_level(int64_t(kXfMatrixOne) * t.in_lut[c][v])) == uint32_t(v);
    t.identity = ident ? 1 : 0;
    return HEIFGPU_OK;
}

// ---- the tone stage of PQ / HLG sources (include/heifgpu.h, "HDR render") ----
uint32_t hdr_transfer(const ColorDesc &c) {
    return !c.has_icc && c.has_nclx && (c.transfer == 16 || c.transfer == 18) ? c.transfer : 0;
}

int hdr_read(const ColorDesc &c, HdrMeta &out, std::string &err) {
    out = HdrMeta{};
    int rc = HEIFGPU_OK;
    if (c.has_clli) {
        if (c.clli.size() < 4) {
            rc = fail(HEIFGPU_E_PARSE, err, "clli: box shorter than its two fields");
        } else {
            out.max_cll = be16(c.clli.data());
            out.max_fall = be16(c.clli.data() + 2);
        }
    }
    if (c.has_mdcv) {
        if (c.mdcv.size() < 24) {
            rc = fail(HEIFGPU_E_PARSE, err, "mdcv: box shorter than its fields");
        } else {
            out.mastering_max = be32(c.mdcv.data() + 16);
            out.mastering_min = be32(c.mdcv.data() + 20);
        }
    }
    return rc;
}

double hdr_source_peak(uint32_t transfer, const HdrMeta &m, double peak_nits) {
    if (transfer == 18) return 1000.0;  // HLG: the BT.2100 nominal display
    double l = 1000.0;
    if (peak_nits > 0.0) l = peak_nits;  // (a NaN is not: the file's then)
    else if (m.max_cll) l = double(m.max_cll);
    else if (m.mastering_max) l = double(m.mastering_max) * 1e-4;
    return l < 203.0 ? 203.0 : l > 10000.0 ? 10000.0 : l;
}

namespace {
// SMPTE ST 2084
constexpr double kPqM1 = 2610.0 / 16384.0, kPqM2 = 2523.0 / 4096.0 * 128.0;
constexpr double kPqC1 = 3424.0 / 4096.0, kPqC2 = 2413.0 / 4096.0 * 32.0, kPqC3 = 2392.0 / 4096.0 * 32.0;
double pq_eotf(double e) {  // code value in [0, 1] to cd/m2
    const double p = std::pow(e > 0.0 ? e : 0.0, 1.0 / kPqM2);
    const double num = p - kPqC1 > 0.0 ? p - kPqC1 : 0.0;
    return 10000.0 * std::pow(num / (kPqC2 - kPqC3 * p), 1.0 / kPqM1);
}
double pq_inverse(double nits) {
    const double y = std::pow((nits > 0.0 ? nits : 0.0) / 10000.0, kPqM1);
    return std::pow((kPqC1 + kPqC2 * y) / (1.0 + kPqC3 * y), kPqM2);
}
// BT.2100 HLG inverse OETF: signal in [0, 1] to scene light in [0, 1]
double hlg_inverse_oetf(double x) {
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * std::log(4.0 * a);
    return x <= 0.5 ? x * x / 3.0 : (std::exp((x - c) / a) + b) / 12.0;
}
}  // namespace

double hdr_eetf(double x, double lsrc) {
    if (x > lsrc) x = lsrc;
    const double n0 = pq_inverse(0.0), span = pq_inverse(lsrc) - n0;
    const double e1 = (pq_inverse(x) - n0) / span, max_lum = (pq_inverse(203.0) - n0) / span;
    const double ks = 1.5 * max_lum - 0.5;
    if (e1 <= ks) return x;
    const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
    const double e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (3.0 * t2 - 2.0 * t3) * max_lum;
    return pq_eotf(e2 * span + n0);
}

int hdr_transform_build(uint32_t primaries, uint32_t transfer, double lsrc, uint32_t dst, uint32_t bits,
                        heifgpu_hdr_transform &out, std::string &err) {
    if (transfer != 16 && transfer != 18) return fail(HEIFGPU_E_INVALID, err, "tone transform of a transfer other than 16, 18");
    if (!(lsrc >= 203.0 && lsrc <= 10000.0)) return fail(HEIFGPU_E_INVALID, err, "source peak outside 203..10000 cd/m2");
    std::memset(&out, 0, sizeof(out));
    // the matrix and out_lut: those of the same primaries coded linearly
    ColorSource src;
    if (int rc = nclx_source(primaries, 8, src, err)) return rc;
    if (int rc = color_transform_build(src, dst, bits, out.base, err)) return rc;
    std::memset(out.base.in_lut, 0, sizeof(out.base.in_lut));
    out.base.identity = 0;
    out.base.tone = HEIFGPU_TONE_BT2390;
    out.transfer = transfer;
    out.Lsrc = transfer == 18 ? 1000.0 : lsrc;
    auto rhu = [](double v) { return std::floor(v + 0.5); };
    const int n = 1 << bits, maxv = n - 1;
    const double U = 65535.0;
    for (int v = 0; v < n; ++v) {
        const double x = double(v) / double(maxv);
        const double nits = transfer == 16 ? pq_eotf(x) : 1000.0 * hlg_inverse_oetf(x);
        const uint32_t l = uint32_t(rhu(U * nits / 203.0));
        for (int c = 0; c < 3; ++c) out.in_lut32[c][v] = l < kXfToneMaxLevel ? l : kXfToneMaxLevel;
    }
    double xy[6], P[9], S[3], W[3];
    if (!nclx_xy(src.primaries, xy) || !nclx_xyz(xy, P, S, W)) return fail(HEIFGPU_E_UNSUPPORTED, err, "nclx: primaries");
    const double ssum = S[0] + S[1] + S[2];
    int big = 0;
    for (int c = 0; c < 3; ++c) {
        out.w[c] = int32_t(rhu(S[c] / ssum * kXfMatrixOne));
        if (out.w[c] > out.w[big]) big = c;
    }
    out.w[big] += kXfMatrixOne - (out.w[0] + out.w[1] + out.w[2]);
    for (int k = 0; k < kXfToneEntries; ++k) {
        const double yn = 203.0 * double(xf_tone_node(k)) / U;
        double g;
        if (transfer == 16) {
            g = k == 0 ? 1.0 : hdr_eetf(yn, out.Lsrc) / yn;
        } else if (k == 0) {
            g = 0.0;
        } else {
            const double ys = yn / 1000.0, yd = 1000.0 * std::pow(ys, 1.2);
            g = std::pow(ys, 0.2) * hdr_eetf(yd, 1000.0) / yd;
        }
        out.T[k] = uint32_t(rhu(double(1u << kXfToneShift) * (g < 1.0 ? g : 1.0)));
    }
    return HEIFGPU_OK;
}

int hdr_transform_make(const ColorDesc &c, uint32_t dst, uint32_t bits, uint32_t tone_map, double peak_nits,
                       heifgpu_hdr_transform &out, std::string &err) {
    if (tone_map > HEIFGPU_TONE_BT2390) return fail(HEIFGPU_E_INVALID, err, "tone_map");
    const uint32_t transfer = tone_map ? hdr_transfer(c) : 0;
    if (!transfer) {
        std::memset(&out, 0, sizeof(out));
        ColorSource src;
        if (int rc = color_source(c, src, err)) return rc;
        return color_transform_build(src, dst, bits, out.base, err);
    }
    HdrMeta meta;
    if (int rc = hdr_read(c, meta, err)) return rc;
    return hdr_transform_build(c.primaries, transfer, hdr_source_peak(transfer, meta, peak_nits), dst, bits, out, err);
}

bool hdr_transform_valid(const heifgpu_hdr_transform &t) {
    if (t.base.bits < 8 || t.base.bits > 12) return false;
    int64_t sum = 0;
    for (int c = 0; c < 3; ++c) {
        if (t.w[c] < 0) return false;
        sum += t.w[c];
        for (uint32_t v = 0; v < (1u << t.base.bits); ++v)
            if (t.in_lut32[c][v] > kXfToneMaxLevel) return false;
    }
    return sum == kXfMatrixOne;
}

}  // namespace hg
