// gain_driver.cpp — the 'tmap' reader and the table builder (host/gain.cpp) with the per-pixel
// formula and the sampler (kernels/gain_xform.hpp) as a stand-alone program for ASan + UBSan
// (make -C heif_amd/csrc gain-asan; tests/test_gain.py runs it): a valid payload at every
// truncation length, every byte of it set to 00, 7F, 80 and FF in turn, random payloads, the
// tables over kinds, depths, destinations and encodings, and the formula and the sampler over
// extreme inputs.  Prints one line per truncation length and per build, then ALL OK.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "host/gain.hpp"
#include "kernels/gain_xform.hpp"

using namespace hg;

static void be32(std::vector<uint8_t> &v, uint32_t x) {
    for (int s = 24; s >= 0; s -= 8) v.push_back(uint8_t(x >> s));
}
static std::vector<uint8_t> payload(bool multichannel) {
    std::vector<uint8_t> v = {0, 0, 0, 0, 0, uint8_t((multichannel ? 0x80 : 0) | 0x40)};
    be32(v, 0), be32(v, 1), be32(v, 3), be32(v, 1);
    for (int c = 0; c < (multichannel ? 3 : 1); ++c) {
        be32(v, uint32_t(-1)), be32(v, 2), be32(v, 3), be32(v, 1), be32(v, 5), be32(v, 4);
        be32(v, 1), be32(v, 64), be32(v, 1), be32(v, 32);
    }
    return v;
}
static const char *name(int rc) {
    return rc == HEIFGPU_OK ? "OK" : rc == HEIFGPU_E_PARSE ? "E_PARSE" : rc == HEIFGPU_E_UNSUPPORTED ? "E_UNSUPPORTED" : "E_INVALID";
}

// the formula over the corners of its domain, through the tables a transform holds
static uint64_t run_formula(const heifgpu_gain_transform &t) {
    const int n = 1 << t.bits;
    std::vector<uint16_t> in(size_t(3) * n);
    for (int c = 0; c < 3; ++c) std::memcpy(in.data() + size_t(c) * n, t.in_lut[c], size_t(n) * 2);
    GainParams gp;
    for (int k = 0; k < 9; ++k) gp.m[k] = t.m[k];
    gp.k_b = t.k_b, gp.k_a = t.k_a, gp.encoding = int(t.encoding);
    const XfToneLut<const uint32_t *> T{t.T}, E{t.E};
    const uint32_t gmax = 256u * ((1u << t.gain_bits) - 1);
    uint64_t sum = 0;
    const uint32_t codes[4] = {0, 1, uint32_t(n / 2), uint32_t(n - 1)};
    for (uint32_t gq : {0u, 1u, 255u, 256u, gmax / 2 + 77, gmax - 1, gmax})
        for (uint32_t a : codes)
            for (uint32_t b : codes) {
                uint32_t r = a, g = b, bl = codes[(a + b) & 3];
                gain_px(in.data(), n, T, E, gp, gq, r, g, bl);
                sum += r + g + bl;
            }
    return sum;
}

int main() {
    int failed = 0;
    std::string err;
    GainMeta gm;
    const std::vector<uint8_t> good = payload(false);
    for (size_t n = 0; n <= good.size(); ++n) {
        std::vector<uint8_t> cut(good.begin(), good.begin() + long(n));  // an exact-size heap copy: a read past it is caught
        const int rc = gain_read(cut.data(), cut.size(), gm, err);
        std::printf("tmap %zu %s\n", n, name(rc));
    }
    const std::vector<uint8_t> multi = payload(true);
    for (size_t n : {size_t(62), multi.size() - 1, multi.size()}) {
        std::vector<uint8_t> cut(multi.begin(), multi.begin() + long(n));
        std::printf("multi %zu %s\n", n, name(gain_read(cut.data(), cut.size(), gm, err)));
    }
    auto t = std::make_unique<heifgpu_gain_transform>();
    ColorDesc color;  // no colr: sRGB
    // every byte hostile in turn; whatever reads OK must also build and run
    int ok = 0, refused = 0;
    for (size_t i = 0; i < good.size(); ++i)
        for (uint8_t v : {uint8_t(0x00), uint8_t(0x7f), uint8_t(0x80), uint8_t(0xff)}) {
            GainDesc g;
            g.kind = HEIFGPU_GAIN_ISO;
            g.tmap = good;
            g.tmap[i] = v;
            const int rc = gain_transform_build(g, color, 8, HEIFGPU_CS_BT2020, 8, HEIFGPU_GAIN_PQ, 10, 0.0, 3.0, 203.0, *t, err);
            if (rc == HEIFGPU_OK) {
                if (gain_transform_invalid(*t)) ++failed, std::printf("FAILED byte %zu %02x: built an invalid transform\n", i, v);
                run_formula(*t);
                ++ok;
            } else {
                ++refused;
            }
        }
    std::printf("bytes ok %d refused %d\n", ok, refused);
    std::mt19937 rng(21496);
    for (int k = 0; k < 2000; ++k) {
        GainDesc g;
        g.kind = HEIFGPU_GAIN_ISO;
        g.tmap.resize(rng() % 160);
        for (uint8_t &b : g.tmap) b = uint8_t(rng());
        if ((k & 1) && !g.tmap.empty()) std::memcpy(g.tmap.data(), good.data(), std::min<size_t>(6, g.tmap.size()));
        if (gain_transform_build(g, color, 10, HEIFGPU_CS_SRGB, 10, HEIFGPU_GAIN_LINEAR, 0, 0.0, 0.0, 0.0, *t, err) == HEIFGPU_OK) {
            if (gain_transform_invalid(*t)) ++failed, std::printf("FAILED random %d: built an invalid transform\n", k);
            run_formula(*t);
        }
    }
    // the builds: kinds x depths x destinations x encodings
    for (uint32_t kind : {uint32_t(HEIFGPU_GAIN_APPLE), uint32_t(HEIFGPU_GAIN_ISO)})
        for (uint32_t bits : {8u, 12u})
            for (uint32_t dst : {uint32_t(HEIFGPU_CS_SRGB), uint32_t(HEIFGPU_CS_DISPLAY_P3), uint32_t(HEIFGPU_CS_BT2020)})
                for (uint32_t pq : {0u, 10u, 16u}) {
                    GainDesc g;
                    g.kind = kind;
                    g.tmap = good;
                    const int rc = gain_transform_build(g, color, bits == 8 ? 12 : 8, dst, bits, pq ? HEIFGPU_GAIN_PQ : HEIFGPU_GAIN_LINEAR,
                                                        pq, 256.0, 0.0, 10000.0, *t, err);
                    const bool fine = rc == HEIFGPU_OK && !gain_transform_invalid(*t);
                    if (fine) run_formula(*t);
                    else ++failed;
                    std::printf("build %u %u %u %u %s\n", kind, bits, dst, pq, fine ? "OK" : "FAILED");
                }
    // the refusals of the builder's own arguments
    {
        GainDesc g;
        g.kind = HEIFGPU_GAIN_APPLE;
        const int a = gain_transform_build(g, color, 8, 0, 8, 0, 0, 0.0, 0.0, 0.0, *t, err);      // no headroom
        const int b = gain_transform_build(g, color, 8, 0, 8, 1, 11, 2.0, 0.0, 0.0, *t, err);     // pq_bits
        const int c = gain_transform_build(g, color, 8, 3, 8, 0, 0, 2.0, 0.0, 0.0, *t, err);      // destination
        const int d = gain_transform_build(g, color, 8, 0, 8, 0, 0, 2.0, 0.0, std::numeric_limits<double>::infinity(), *t, err);  // infinite sdr_white
        std::printf("refuse %s %s %s %s\n", name(a), name(b), name(c), name(d));
    }
    // the sampler at the extremes of its domain: taps inside the map, weights in 0 .. 255
    for (int W : {1, 2, 3, 255, 4032, 65535})
        for (int Wg : {1, 2, 3, 97, 2016, 65535}) {
            const double inv = 1.0 / double(W);
            for (int s : {0, 1, W / 2, W - 2, W - 1}) {
                if (s < 0 || s >= W) continue;
                const GainTap tp = gain_tap(s, W, Wg, inv);
                const int64_t nn = (2 * int64_t(s) + 1) * Wg - W, dd = 2 * int64_t(W);
                int64_t i = nn / dd;
                if (nn % dd < 0) --i;
                const int64_t f = 256 * (nn - i * dd) / dd;
                const int64_t i0 = i < 0 ? 0 : i > Wg - 1 ? Wg - 1 : i, i1 = i + 1 < 0 ? 0 : i + 1 > Wg - 1 ? Wg - 1 : i + 1;
                if (tp.i0 != i0 || tp.i1 != i1 || tp.f != f) ++failed, std::printf("FAILED tap %d %d %d\n", s, W, Wg);
            }
        }
    if (gain_sample(4095, 4095, 4095, 4095, 255, 255) != 256u * 4095u) ++failed, std::printf("FAILED sample\n");
    std::printf(failed ? "FAILED %d\n" : "ALL OK\n", failed);
    return failed ? 1 : 0;
}
