// Stand-alone check of the TB records' packed words (kernels/intra_rec.hpp), built with
// -fsanitize=address,undefined (make intra-pack-asan; tests/test_intra_walk.py runs it).
//
// (a) round trip: every reachable combination of CTB size, chroma format, cIdx, TB size and
//     position on the TB grid, with every mode and flag combination, through pack and unpack:
//     each field comes back as it went in, so none bleeds into another;
// (b) damaged records (a mode above 34, a size outside 2..5, coordinates outside the CTB or the
//     picture, a cIdx the format has not) pack to zero words;
// (c) random records: whatever is OK lies inside its CTB's window and inside the residual planes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kernels/intra_rec.hpp"

using namespace hg;

static long g_checks = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        ++g_checks;                                                     \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static const int kAngle[35] = {0, 0, 32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26,
                               -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32};
static const int kInv[35] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -4096, -1638, -910, -630, -482, -390, -315,
                             -256, -315, -390, -482, -630, -910, -1638, -4096, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static TbGeom geom(int log2ctb, int chroma, int ctbs_x, int ctbs_y) {
    TbGeom g;
    g.log2ctb = log2ctb;
    g.chroma = chroma;
    g.W = ctbs_x << log2ctb;
    g.H = ctbs_y << log2ctb;
    g.cw = chroma ? g.W >> chroma_sx(chroma) : 0;
    g.ch = chroma ? g.H >> chroma_sy(chroma) : 0;
    return g;
}

static int ref_zidx(int bx, int by) {
    int z = 0;
    for (int b = 0; b < 4; ++b) z |= ((bx >> b) & 1) << (2 * b) | ((by >> b) & 1) << (2 * b + 1);
    return z;
}

static bool ref_filt(int k, int chroma, int n, int m) {
    if (!(k == 0 || chroma == 3) || m == 1 || n == 4) return false;
    const int d = std::min(std::abs(m - 26), std::abs(m - 10));
    return d > (n == 8 ? 7 : n == 16 ? 1 : 0);
}

static void round_trip() {
    for (int log2ctb = 4; log2ctb <= 6; ++log2ctb)
        for (int chroma = 0; chroma <= 3; ++chroma) {
            const TbGeom g = geom(log2ctb, chroma, 5, 4);
            for (int k = 0; k < (chroma ? 3 : 1); ++k) {
                const int sx = k ? chroma_sx(chroma) : 0, sy = k ? chroma_sy(chroma) : 0;
                const int csx = (1 << log2ctb) >> sx, csy = (1 << log2ctb) >> sy;
                for (int log2 = 2; log2 <= 5 && (1 << log2) <= csx; ++log2) {
                    const int n = 1 << log2;
                    for (int ly = 0; ly + n <= csy; ly += n)
                        for (int lx = 0; lx + n <= csx; lx += n)
                            for (int m = 0; m <= 34; ++m)
                                for (int fl = 0; fl < 4; ++fl)
                                    for (int pos = 0; pos < 2; ++pos) {
                                        const int ctu = pos ? 4 : 0, r = pos ? 3 : 0;
                                        TuRec q{};
                                        q.x = (uint16_t)(ctu * csx + lx);
                                        q.y = (uint16_t)(r * csy + ly);
                                        q.log2 = (uint8_t)log2;
                                        q.mode = (uint8_t)m;
                                        q.flags = (uint8_t)(k | (fl & 1 ? TU_CBF : 0) | (fl & 2 ? TU_PCM | TU_BYPASS : 0) |
                                                            (m & 1 ? TU_TSKIP : 0) | (m & 2 ? TU_DST : 0));
                                        q.ctu = (uint16_t)ctu;
                                        q.qp = 51;
                                        q.coef = 0xffffffffu;
                                        q.ncoef = 0xffff;
                                        uint32_t a = tb_pack_a(q, g, r);
                                        CHECK(a & TBA_OK);
                                        CHECK(tba_lx(a) == lx && tba_ly(a) == ly && tba_log2(a) == log2);
                                        CHECK(tba_mode(a) == m && tba_cidx(a) == k);
                                        CHECK(!!(a & TBA_CBF) == !!(fl & 1) && !!(a & TBA_PCM) == !!(fl & 2));
                                        CHECK(!!(a & TBA_FILT) == ref_filt(k, chroma, n, m));
                                        CHECK(!(a & (TBA_PAIR | TBA_CBF2 | TBA_PCM2)) && !(a >> 29));
                                        const uint32_t b = tb_pack_b(a, g, kAngle[m], kInv[m]);
                                        CHECK(tbb_zc(b) == ref_zidx((lx << sx) >> 2, (ly << sy) >> 2));
                                        CHECK(tbb_ang(b) == kAngle[m] && tbb_inv(b) == kInv[m]);
                                        bool fits = false;
                                        const uint32_t c = tb_pack_c(q, a, g, &fits);
                                        const uint64_t plane = k ? (uint64_t)g.W * g.H + (k == 2 ? (uint64_t)g.cw * g.ch : 0) : 0;
                                        CHECK(fits && c == plane + (uint64_t)q.y * (k ? g.cw : g.W) + q.x);
                                        for (int cf = 0; cf < 4; ++cf) {  // the pair's bits beside the others
                                            const uint32_t p = tb_pack_pair(a, (uint32_t)(2 | (cf & 1 ? TU_CBF : 0) | (cf & 2 ? TU_PCM : 0)));
                                            CHECK((p & TBA_PAIR) && !!(p & TBA_CBF2) == !!(cf & 1) && !!(p & TBA_PCM2) == !!(cf & 2));
                                            CHECK((p & ~(TBA_PAIR | TBA_CBF2 | TBA_PCM2)) == a);
                                        }
                                    }
                }
            }
        }
}

static void expect_rejected(const TuRec &q, const TbGeom &g, int r) {
    const uint32_t a = tb_pack_a(q, g, r);
    CHECK(a == 0);
    CHECK(tb_pack_b(a, g, 32, -256) == 0);
    bool fits = false;
    CHECK(tb_pack_c(q, a, g, &fits) == 0);
}

static void damaged() {
    for (int log2ctb = 4; log2ctb <= 6; ++log2ctb)
        for (int chroma = 0; chroma <= 3; ++chroma) {
            const TbGeom g = geom(log2ctb, chroma, 3, 3);
            for (int k = 0; k < 4; ++k) {
                const bool has = k < (chroma ? 3 : 1);
                const int sx = k && has ? chroma_sx(chroma) : 0, sy = k && has ? chroma_sy(chroma) : 0;
                const int csx = (1 << log2ctb) >> sx, csy = (1 << log2ctb) >> sy;
                TuRec good{};
                good.x = (uint16_t)csx;  // CTB (1, 1), its first TB
                good.y = (uint16_t)csy;
                good.log2 = 2;
                good.mode = 10;
                good.flags = (uint8_t)k;
                good.ctu = 1;
                if (!has) {  // a component the format has not
                    expect_rejected(good, g, 1);
                    continue;
                }
                CHECK(tb_pack_a(good, g, 1) & TBA_OK);
                for (int m = 35; m < 256; ++m) {
                    TuRec q = good;
                    q.mode = (uint8_t)m;
                    expect_rejected(q, g, 1);
                }
                for (int l = 0; l < 256; ++l) {
                    if (l >= 2 && l <= 5 && (1 << l) <= csx) continue;
                    TuRec q = good;
                    q.log2 = (uint8_t)l;
                    expect_rejected(q, g, 1);
                }
                for (int d = 1; d <= 4; ++d) {  // left of / above the CTB, and over its right / lower edge
                    TuRec q = good;
                    q.x = (uint16_t)(csx - d);
                    expect_rejected(q, g, 1);
                    q = good;
                    q.y = (uint16_t)(csy - d);
                    expect_rejected(q, g, 1);
                    q = good;
                    q.x = (uint16_t)(2 * csx - 4 + d);
                    expect_rejected(q, g, 1);
                    q = good;
                    q.y = (uint16_t)(2 * csy - 4 + d);
                    expect_rejected(q, g, 1);
                }
                TuRec q = good;  // another CTB column / row than the record says
                q.ctu = 2;
                expect_rejected(q, g, 1);
                expect_rejected(good, g, 0);
                expect_rejected(good, g, 2);
                q = good;  // outside the picture (the CTB is clipped by it)
                TbGeom small = g;
                small.W = (1 << log2ctb) + 2;
                small.cw = chroma ? small.W >> chroma_sx(chroma) : 0;
                expect_rejected(q, small, 1);
                q.x = 0xffff;
                q.y = 0xffff;
                q.ctu = 0xffff;
                expect_rejected(q, g, 1);
            }
        }
}

static void random_records() {
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto rnd = [&] {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return (uint32_t)(s >> 24);
    };
    long ok = 0;
    for (int it = 0; it < 400000; ++it) {
        const int log2ctb = 4 + (int)(rnd() % 3), chroma = (int)(rnd() % 4);
        TbGeom g = geom(log2ctb, chroma, 1 + (int)(rnd() % 3), 1 + (int)(rnd() % 3));
        if (rnd() & 1) {  // a picture that clips its last CTBs (even, so that the chroma planes are whole)
            g.W -= 2 * (int)(rnd() % 4);
            g.H -= 2 * (int)(rnd() % 4);
            g.cw = chroma ? g.W >> chroma_sx(chroma) : 0;
            g.ch = chroma ? g.H >> chroma_sy(chroma) : 0;
        }
        const int r = (int)(rnd() % 4);
        TuRec q{};
        q.x = (uint16_t)(rnd() % 200);
        q.y = (uint16_t)(rnd() % 200);
        q.log2 = (uint8_t)(rnd() % 8);
        q.mode = (uint8_t)(rnd() % 40);
        q.flags = (uint8_t)rnd();
        q.ctu = (uint16_t)(rnd() % 4);
        if (rnd() % 16 == 0) q.x = (uint16_t)rnd(), q.y = (uint16_t)rnd(), q.ctu = (uint16_t)rnd(), q.log2 = (uint8_t)rnd();
        if (rnd() & 1) {  // a TB of CTB (ctu, r) on its grid (over the picture's edge now and then), one field off at times
            const int k = chroma ? (int)(rnd() % 3) : 0, log2 = 2 + (int)(rnd() % 4), n = 1 << log2;
            const int csx = (1 << log2ctb) >> (k ? chroma_sx(chroma) : 0), csy = (1 << log2ctb) >> (k ? chroma_sy(chroma) : 0);
            q.flags = (uint8_t)((q.flags & ~TU_CIDX_MASK) | k);
            q.log2 = (uint8_t)log2;
            q.mode = (uint8_t)(rnd() % 35);
            q.x = (uint16_t)(q.ctu * csx + (int)(rnd() % (unsigned)csx) / n * n);
            q.y = (uint16_t)(r * csy + (int)(rnd() % (unsigned)csy) / n * n);
            switch (rnd() % 8) {
            case 0: q.x = (uint16_t)(q.x + rnd() % 70 - 35); break;
            case 1: q.y = (uint16_t)(q.y + rnd() % 70 - 35); break;
            case 2: q.mode = (uint8_t)rnd(); break;
            case 3: q.log2 = (uint8_t)rnd(); break;
            default: break;
            }
        }
        const uint32_t a = tb_pack_a(q, g, r);
        bool fits = false;
        const uint32_t c = tb_pack_c(q, a, g, &fits);
        const uint32_t b = tb_pack_b(a, g, 0, 0);
        if (!(a & TBA_OK)) {
            CHECK(a == 0 && b == 0 && c == 0);
            continue;
        }
        ++ok;
        const int k = tba_cidx(a), n = 1 << tba_log2(a);
        CHECK(k < (chroma ? 3 : 1) && tba_mode(a) <= 34);
        const int sx = k ? chroma_sx(chroma) : 0, sy = k ? chroma_sy(chroma) : 0;
        const int csx = (1 << log2ctb) >> sx, csy = (1 << log2ctb) >> sy;
        CHECK(tba_lx(a) + n <= csx && tba_ly(a) + n <= csy);  // inside the CTB's window
        const int PW = k ? g.cw : g.W, PH = k ? g.ch : g.H;
        CHECK(q.ctu * csx + tba_lx(a) + n <= PW && r * csy + tba_ly(a) + n <= PH);  // inside the picture
        const uint64_t total = (uint64_t)g.W * g.H + 2 * (uint64_t)g.cw * g.ch;
        CHECK(fits && (uint64_t)c + (uint64_t)(n - 1) * PW + n <= total);  // the TB's residuals inside the planes
        CHECK(tbb_zc(b) < 256);
    }
    CHECK(ok > 1000);
}

int main() {
    round_trip();
    damaged();
    random_records();
    printf("INTRA PACK OK %ld checks\n", g_checks);
    return 0;
}
