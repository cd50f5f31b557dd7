// hdr_driver.cpp — the host reader of clli / mdcv and the tone-table builder
// (heif_amd/csrc/host/icc.cpp) as a stand-alone program built with ASan + UBSan
// (`make tone-asan`; tests/test_tone.py runs it).  Nothing here touches a device.
//
//   hdr_driver
//
// answers one line per case:
//   clli N / mdcv N            the box cut to its first N payload bytes, for every N up to
//                              its size and a few beyond (OK from 4 / 24 bytes on, else E_PARSE)
//   fields V                   every field of both boxes set to V = 0, 0xFFFF / 0xFFFFFFFF
//   build TRANSFER PEAK ...    the tables at that source peak, to both destinations at 8, 10
//                              and 12 bits: every entry inside the range the kernels rely on,
//                              and the per-pixel formula over the corners of the code cube
// Each payload is a heap copy of exactly its own length, so a read past its end is an
// ASan report.  Exit status 1 if any case answers what it must not.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "host/icc.hpp"
#include "kernels/color_xform.hpp"

static int bad = 0;

static const char *name_of(int rc) {
    switch (rc) {
    case HEIFGPU_OK: return "OK";
    case HEIFGPU_E_PARSE: return "E_PARSE";
    case HEIFGPU_E_UNSUPPORTED: return "E_UNSUPPORTED";
    case HEIFGPU_E_INVALID: return "E_INVALID";
    default: return "OTHER";
    }
}

static void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED %s\n", what);
        ++bad;
    }
}

static std::vector<uint8_t> clli_payload(uint32_t cll, uint32_t fall) {
    return {uint8_t(cll >> 8), uint8_t(cll), uint8_t(fall >> 8), uint8_t(fall)};
}

static std::vector<uint8_t> mdcv_payload(uint32_t xy, uint32_t lmax, uint32_t lmin) {
    std::vector<uint8_t> p;
    for (int k = 0; k < 8; ++k) p.push_back(uint8_t(xy >> 8)), p.push_back(uint8_t(xy));
    for (uint32_t v : {lmax, lmin})
        for (int s = 24; s >= 0; s -= 8) p.push_back(uint8_t(v >> s));
    return p;
}

static hg::ColorDesc desc(uint32_t transfer, const std::vector<uint8_t> *clli, const std::vector<uint8_t> *mdcv) {
    hg::ColorDesc c;
    c.has_nclx = true;
    c.primaries = 9;
    c.transfer = transfer;
    if (clli) c.has_clli = true, c.clli = std::vector<uint8_t>(clli->begin(), clli->end());  // capacity == size
    if (mdcv) c.has_mdcv = true, c.mdcv = std::vector<uint8_t>(mdcv->begin(), mdcv->end());
    return c;
}

static heifgpu_hdr_transform g_t;  // (134 KB: not on the stack)

// the tables of one transform inside the range the kernels rely on, and the formula over
// the corners and the grey axis of the code cube
static void check_tables(const heifgpu_hdr_transform &t, uint32_t bits) {
    expect(hg::hdr_transform_valid(t), "hdr_transform_valid");
    expect(t.base.tone == HEIFGPU_TONE_BT2390 && t.base.identity == 0 && t.base.bits == bits, "tags");
    for (int k = 0; k < hg::kXfToneEntries; ++k) expect(t.T[k] <= (1u << hg::kXfToneShift), "T entry above a gain of 1");
    const int n = 1 << bits;
    std::vector<uint32_t> in(size_t(3) * n);
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < n; ++v) in[size_t(c) * n + v] = t.in_lut32[c][v];
    const hg::XfToneLut<const uint32_t *> tone{t.T};
    const hg::XfOutLut<const uint16_t *> out{t.base.out_lut};
    const uint32_t ends[3] = {0u, uint32_t(n / 2), uint32_t(n - 1)};
    for (uint32_t r0 : ends)
        for (uint32_t g0 : ends)
            for (uint32_t b0 : ends) {
                uint32_t r = r0, g = g0, b = b0;
                hg::color_tone_px(in.data(), n, t.w, tone, out, t.base.m, r, g, b);
                expect(r < uint32_t(n) && g < uint32_t(n) && b < uint32_t(n), "output code above maxv");
            }
    for (uint32_t v = 0; v < uint32_t(n); ++v) {
        uint32_t r = v, g = v, b = v;
        hg::color_tone_px(in.data(), n, t.w, tone, out, t.base.m, r, g, b);
        expect(r < uint32_t(n) && g < uint32_t(n) && b < uint32_t(n), "grey output above maxv");
    }
}

int main() {
    std::string err;
    hg::HdrMeta m;
    // every truncation length
    const std::vector<uint8_t> clli = clli_payload(400, 100), mdcv = mdcv_payload(15000, 10000000u, 50u);
    for (size_t n = 0; n <= clli.size() + 3; ++n) {
        std::vector<uint8_t> p(clli.begin(), clli.begin() + long(std::min(n, clli.size())));
        p.resize(n, 0xAB);
        const hg::ColorDesc c = desc(16, &p, nullptr);
        const int rc = hg::hdr_read(c, m, err);
        std::printf("clli %zu %s\n", n, name_of(rc));
        expect(rc == (n >= 4 ? HEIFGPU_OK : HEIFGPU_E_PARSE), "clli truncation");
        expect(n < 4 || (m.max_cll == 400 && m.max_fall == 100), "clli values");
        const int mk = hg::hdr_transform_make(c, 0, 8, HEIFGPU_TONE_BT2390, 0.0, g_t, err);
        expect(mk == rc, "make follows the reader (clli)");
        expect(hg::hdr_transform_make(c, 0, 8, HEIFGPU_TONE_NONE, 0.0, g_t, err) == HEIFGPU_E_UNSUPPORTED, "untoned PQ is refused");
    }
    for (size_t n = 0; n <= mdcv.size() + 3; ++n) {
        std::vector<uint8_t> p(mdcv.begin(), mdcv.begin() + long(std::min(n, mdcv.size())));
        p.resize(n, 0xAB);
        const hg::ColorDesc c = desc(16, nullptr, &p);
        const int rc = hg::hdr_read(c, m, err);
        std::printf("mdcv %zu %s\n", n, name_of(rc));
        expect(rc == (n >= 24 ? HEIFGPU_OK : HEIFGPU_E_PARSE), "mdcv truncation");
        expect(n < 24 || (m.mastering_max == 10000000u && m.mastering_min == 50u), "mdcv values");
        expect(hg::hdr_transform_make(c, 1, 10, HEIFGPU_TONE_BT2390, 0.0, g_t, err) == rc, "make follows the reader (mdcv)");
    }
    // extreme field values: the peak stays inside [203, 10000] and the tables inside their ranges
    const uint32_t ext16[2] = {0u, 0xFFFFu}, ext32[2] = {0u, 0xFFFFFFFFu};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const std::vector<uint8_t> cl = clli_payload(ext16[a], ext16[a]), md = mdcv_payload(ext16[b], ext32[b], ext32[b]);
            const hg::ColorDesc c = desc(16, &cl, &md);
            int rc = hg::hdr_read(c, m, err);
            const double peak = hg::hdr_source_peak(16, m, 0.0);
            std::printf("fields %u %u %s peak %.1f\n", ext16[a], ext32[b], name_of(rc), peak);
            expect(rc == HEIFGPU_OK && peak >= 203.0 && peak <= 10000.0, "extreme fields");
            expect(peak == (a ? 10000.0 : b ? 10000.0 : 1000.0), "the Lsrc rule at the extremes");
            rc = hg::hdr_transform_make(c, 0, 12, HEIFGPU_TONE_BT2390, 0.0, g_t, err);
            expect(rc == HEIFGPU_OK, "make at extreme fields");
            if (rc == HEIFGPU_OK) check_tables(g_t, 12);
        }
    // peak_nits: negative, zero, tiny, huge, infinite, NaN
    for (double pk : {-1.0, 0.0, 1e-300, 5.0, 203.0, 1e9, double(INFINITY), double(NAN)}) {
        const double peak = hg::hdr_source_peak(16, hg::HdrMeta{}, pk);
        std::printf("peak_nits %g -> %.1f\n", pk, peak);
        expect(peak >= 203.0 && peak <= 10000.0, "peak_nits clamp");
        expect(hg::hdr_source_peak(18, hg::HdrMeta{}, pk) == 1000.0, "HLG peak");
    }
    // the builder over peaks, transfers, primaries, destinations and depths
    for (uint32_t transfer : {16u, 18u})
        for (double peak : {203.0, 203.5, 400.0, 1000.0, 4000.0, 10000.0})
            for (uint32_t prim : {1u, 2u, 9u, 12u})
                for (uint32_t dst = 0; dst < 2; ++dst)
                    for (uint32_t bits = 8; bits <= 12; bits += 2) {
                        const int rc = hg::hdr_transform_build(prim, transfer, peak, dst, bits, g_t, err);
                        if (dst == 0 && bits == 8 && prim == 9) std::printf("build %u %.1f %s\n", transfer, peak, name_of(rc));
                        expect(rc == HEIFGPU_OK, "build");
                        if (rc == HEIFGPU_OK) check_tables(g_t, bits);
                    }
    // what the builder refuses
    expect(hg::hdr_transform_build(9, 13, 1000.0, 0, 8, g_t, err) == HEIFGPU_E_INVALID, "transfer 13");
    expect(hg::hdr_transform_build(9, 16, 100.0, 0, 8, g_t, err) == HEIFGPU_E_INVALID, "peak below 203");
    expect(hg::hdr_transform_build(9, 16, double(NAN), 0, 8, g_t, err) == HEIFGPU_E_INVALID, "peak NaN");
    expect(hg::hdr_transform_build(5, 16, 1000.0, 0, 8, g_t, err) == HEIFGPU_E_UNSUPPORTED, "primaries 5");
    expect(hg::hdr_transform_build(9, 16, 1000.0, 2, 8, g_t, err) == HEIFGPU_E_INVALID, "destination 2");
    expect(hg::hdr_transform_build(9, 16, 1000.0, 0, 13, g_t, err) == HEIFGPU_E_INVALID, "13 bits");
    expect(hg::hdr_transform_make(desc(16, nullptr, nullptr), 0, 8, 2, 0.0, g_t, err) == HEIFGPU_E_INVALID, "tone_map 2");
    // a transform whose tables leave the range is told apart
    expect(hg::hdr_transform_build(9, 16, 1000.0, 0, 8, g_t, err) == HEIFGPU_OK && hg::hdr_transform_valid(g_t), "valid");
    g_t.in_lut32[1][7] = hg::kXfToneMaxLevel + 1;
    expect(!hg::hdr_transform_valid(g_t), "level above 2^22 - 1");
    g_t.in_lut32[1][7] = 0, g_t.w[0] += 1;
    expect(!hg::hdr_transform_valid(g_t), "weights not summing to 16384");
    std::printf("%s\n", bad ? "BAD" : "ALL OK");
    return bad ? 1 : 0;
}
