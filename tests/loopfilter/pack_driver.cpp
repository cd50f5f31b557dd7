// pack_driver.cpp — TEST-ONLY: the loop filter's packed helpers (kernels/lf_pack.hpp) alone, as
// a stand-alone ASan + UBSan program (make lf-pack-asan; tests/test_loopfilter_wide.py runs it).
//
// The host twins are run over every pair of 8-bit samples in both lanes of a pack and every
// SAO offset of the 8-bit range, against the clause text of 8.7.3 written out per sample; the
// byte permute over every selector value; the 16-bit helpers over the ends of the 10- and
// 12-bit ranges.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kernels/lf_pack.hpp"

namespace hg {
thread_local EmuCtx g_emu;
}
using namespace hg::lfp;

namespace {

int fails = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond) && ++fails <= 20) printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

int sgn(int v) { return (v > 0) - (v < 0); }
int clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
uint32_t pack(int lo, int hi) { return (uint32_t)(lo & 0xffff) | ((uint32_t)(hi & 0xffff) << 16); }
int lane(uint32_t p, int h) { return (int16_t)(h ? p >> 16 : p & 0xffffu); }

// SaoOffsetVal[edgeIdx] of 8.7.3.2 for the two neighbours' signs
int edge_offset(const int off[4], int c, int a, int b) {
    int e = 2 + sgn(c - a) + sgn(c - b);
    if (e <= 2) e = e == 2 ? 0 : e + 1;
    return e ? off[e - 1] : 0;
}
int band_offset(const int off[4], int c, int bd, int pos) {
    const int k = ((c >> (bd - 5)) - pos) & 31;
    return k < 4 ? off[k] : 0;
}

void words_of(const int off[4], uint32_t &d1, uint32_t &d2, uint32_t &d3) {
    // as the component's offsets lie in SaoParams: junk in the halves that belong to its neighbours
    d1 = 0x5a5au | ((uint32_t)(off[0] & 0xffff) << 16);
    d2 = (uint32_t)(off[1] & 0xffff) | ((uint32_t)(off[2] & 0xffff) << 16);
    d3 = (uint32_t)(off[3] & 0xffff) | 0xa5a50000u;
}

void test_perm() {
    const uint32_t s0 = 0x87f61504u, s1 = 0x03e2c180u;
    const uint8_t in[8] = {0x80, 0xc1, 0xe2, 0x03, 0x04, 0x15, 0xf6, 0x87};
    for (uint32_t s = 0; s < 256; ++s) {
        uint32_t want;
        if (s >= 13) want = 0xff;
        else if (s == 12) want = 0;
        else if (s >= 8) want = (in[2 * (s - 8) + 1] & 0x80) ? 0xff : 0;
        else want = in[s];
        for (int k = 0; k < 4; ++k) {
            const uint32_t sel = (s << (8 * k)) | (0x0c0c0c0cu & ~(0xffu << (8 * k)));
            CHECK(perm(s0, s1, sel) == want << (8 * k));
        }
    }
    CHECK(pk_from_bytes(0xddccbbaau, 0) == 0x00bb00aau && pk_from_bytes(0xddccbbaau, 1) == 0x00dd00ccu);
    CHECK(pk_to_bytes(0x11bb22aau, 0x33dd44ccu) == 0xddccbbaau);
}

void test_lanes() {
    const int vals[] = {0, 1, 2, 127, 128, 255, 256, 1023, 4095, 32767, -1, -2, -124, -32768};
    for (int a : vals)
        for (int b : vals)
            for (int c : vals) {
                const uint32_t x = pack(a, b), y = pack(c, a), z = pack(b, c);
                CHECK(pk_add(x, y) == pack(a + c, b + a) && pk_sub(x, y) == pack(a - c, b - a));
                CHECK(pk_max_i16(x, y) == pack(a > c ? a : c, b > a ? b : a));
                CHECK(pk_min_i16(x, z) == pack(a < b ? a : b, b < c ? b : c));
                for (int n = 0; n < 16; ++n) {
                    CHECK(pk_ashr(x, n) == pack(a >> n, b >> n));
                    CHECK(pk_lshr(x, n) == pack((a & 0xffff) >> n, (b & 0xffff) >> n));
                }
            }
}

// every pair of 8-bit samples in either lane, with a fixed other lane: sign, lookup, add, clip
void test_sao8() {
    const int bd = 8, maxv = 255;
    const uint32_t maxv2 = pack(maxv, maxv);
    for (int o = -7; o <= 7; ++o) {
        const int off[4] = {o, -o, o > 0 ? o - 1 : o + 1, 7 - (o & 7)};
        uint32_t d1, d2, d3, elo, ehi, blo, bhi;
        words_of(off, d1, d2, d3);
        sao_tables(d1, d2, d3, true, elo, ehi);
        sao_tables(d1, d2, d3, false, blo, bhi);
        for (int c = 0; c <= maxv; ++c)
            for (int a = 0; a <= maxv; ++a) {
                const int b = (a * 7 + c + o) & 255, c2 = 255 - c, a2 = (a + 1) & 255, b2 = 255 - b;
                for (int h = 0; h < 2; ++h) {  // the pair under test in lane h, another in the other lane
                    const uint32_t cp = h ? pack(c2, c) : pack(c, c2), ap = h ? pack(a2, a) : pack(a, a2);
                    const uint32_t bp = h ? pack(b2, b) : pack(b, b2);
                    const uint32_t sa = pk_sign_diff(cp, ap), sb = pk_sign_diff(cp, bp);
                    CHECK(lane(sa, h) == sgn(c - a) && lane(sa, !h) == sgn(c2 - a2));
                    const uint32_t idx = pk_add(pk_add(sa, sb), 0x00020002u);
                    const uint32_t r = pk_add_clip(cp, sao_lookup(elo, ehi, idx), maxv2);
                    CHECK(lane(r, h) == clip3(0, maxv, c + edge_offset(off, c, a, b)));
                    CHECK(lane(r, !h) == clip3(0, maxv, c2 + edge_offset(off, c2, a2, b2)));
                }
            }
        for (int pos = 0; pos < 32; ++pos)
            for (int c = 0; c <= maxv; ++c) {
                const int c2 = 255 - c;
                const uint32_t cp = pack(c, c2);
                const uint32_t k = pk_sub(pk_lshr(cp, bd - 5), pack(pos, pos)) & 0x001f001fu;
                const uint32_t r = pk_add_clip(cp, sao_lookup(blo, bhi, pk_min_i16(k, 0x00040004u)), maxv2);
                CHECK(lane(r, 0) == clip3(0, maxv, c + band_offset(off, c, bd, pos)));
                CHECK(lane(r, 1) == clip3(0, maxv, c2 + band_offset(off, c2, bd, pos)));
            }
    }
}

// the ends of the 10- and 12-bit ranges with the largest offsets (31 and 31 << 2)
void test_sao16() {
    for (int bd : {10, 12}) {
        const int maxv = (1 << bd) - 1, m = 31 << (bd - 10);
        const int ends[] = {0, 1, m - 1, m, m + 1, maxv / 2, maxv - m - 1, maxv - m, maxv - m + 1, maxv - 1, maxv};
        const int off[4] = {m, -m, -m, m};
        uint32_t d1, d2, d3, elo, ehi, blo, bhi;
        words_of(off, d1, d2, d3);
        sao_tables(d1, d2, d3, true, elo, ehi);
        sao_tables(d1, d2, d3, false, blo, bhi);
        const uint32_t maxv2 = pack(maxv, maxv);
        for (int c : ends)
            for (int a : ends)
                for (int b : ends)
                    for (int c2 : ends) {
                        const uint32_t cp = pack(c, c2), ap = pack(a, b), bp = pack(b, a);
                        const uint32_t idx = pk_add(pk_add(pk_sign_diff(cp, ap), pk_sign_diff(cp, bp)), 0x00020002u);
                        const uint32_t r = pk_add_clip(cp, sao_lookup(elo, ehi, idx), maxv2);
                        CHECK(lane(r, 0) == clip3(0, maxv, c + edge_offset(off, c, a, b)));
                        CHECK(lane(r, 1) == clip3(0, maxv, c2 + edge_offset(off, c2, b, a)));
                        for (int pos : {0, 1, 28, 29, 30, 31}) {
                            const uint32_t k = pk_sub(pk_lshr(cp, bd - 5), pack(pos, pos)) & 0x001f001fu;
                            const uint32_t q = pk_add_clip(cp, sao_lookup(blo, bhi, pk_min_i16(k, 0x00040004u)), maxv2);
                            CHECK(lane(q, 0) == clip3(0, maxv, c + band_offset(off, c, bd, pos)));
                            CHECK(lane(q, 1) == clip3(0, maxv, c2 + band_offset(off, c2, bd, pos)));
                        }
                    }
    }
}

}  // namespace

int main() {
    test_perm();
    test_lanes();
    test_sao8();
    test_sao16();
    if (fails) {
        printf("LF PACK FAILED: %d checks\n", fails);
        return 1;
    }
    printf("LF PACK OK\n");
    return 0;
}
