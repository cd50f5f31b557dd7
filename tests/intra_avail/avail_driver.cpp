// Stand-alone check of a TB record's neighbour facts (word D of kernels/intra_rec.hpp), built with
// -fsanitize=address,undefined (make intra-avail-asan; tests/test_intra_avail.py runs it).
//
// The expected side is the per-sample rule of 6.4.1 / 8.4.4.2.2 restated here: a neighbour is
// available where it lies inside the picture, not below or right of the TB's CTB (the row of
// CTBs above is decoded up to the CTB above-right, the CTB to the left is decoded), and, inside
// the CTB, where its 4x4 luma block precedes the TB's first in z-scan order (an index of this
// file's own).  Over 4:2:0, 4:2:2 and 4:4:4, luma and chroma, CTB 16, 32 and 64, every TB size at
// every aligned position, every picture extent from the CTB's origin in multiples of 8 luma
// samples and a picture column / row left of / above the CTB present or not:
// (a) the five facts expand to exactly the per-sample bits;
// (b) tb_subst_src equals the search-order rule (the nearest available sample before s, else the
//     first available one) for every sample;
// (c) the source of every sample, through tb_src_addr / tb_src_at, is the element of the window
//     that holds that neighbour, inside its array (the CTB's samples, the left column, the row
//     above); for the smallest and the largest CTB that is the wave's smallest and largest block;
// (d) word D's window offset is the TB's first sample;
// (e) a record that is not OK packs to zero.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "kernels/intra_rec.hpp"

using namespace hg;

static long g_checks = 0, g_cases = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        ++g_checks;                                                     \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

// z-scan index of the 4x4 luma block (bx, by) of a CTB: the bits of bx and by interleaved, bx lowest
static int zscan(int bx, int by) {
    int z = 0;
    for (int b = 0; b < 4; ++b) z |= ((bx >> b) & 1) << (2 * b) | ((by >> b) & 1) << (2 * b + 1);
    return z;
}

struct Tb {
    int log2ctb, subx, suby;  // of the TB's component
    int x0, y0, n;            // component samples from the CTB's origin
    int vw, vh;               // columns, rows from the CTB's origin to the picture's edge, component samples
    bool hasl, hasa;          // the picture has a column left of / a row above the CTB
};

// the per-sample rule for the neighbour (xn, yn), component samples from the CTB's origin
static bool sample_avail(const Tb &t, int xn, int yn) {
    if (xn < (t.hasl ? -1 : 0) || yn < (t.hasa ? -1 : 0) || xn >= t.vw || yn >= t.vh) return false;  // the picture
    const int csl = 1 << t.log2ctb;
    const int lx = xn * (1 << t.subx), ly = yn * (1 << t.suby);  // luma location (a neighbour's may be -1)
    if (ly < 0) return true;                  // the row of CTBs above, up to the CTB above-right
    if (ly >= csl || lx >= csl) return false;  // the CTBs below and to the right
    if (lx < 0) return true;                  // the CTB to the left
    return zscan(lx >> 2, ly >> 2) < zscan((t.x0 << t.subx) >> 2, (t.y0 << t.suby) >> 2);
}

// search position s of 8.4.4.2.2: the column left of the TB bottom-up, the corner, the row above
static void search_xy(const Tb &t, int s, int *xn, int *yn) {
    const int n = t.n;
    if (s < 2 * n) *xn = t.x0 - 1, *yn = t.y0 + 2 * n - 1 - s;
    else if (s == 2 * n) *xn = t.x0 - 1, *yn = t.y0 - 1;
    else *xn = t.x0 + s - 2 * n - 1, *yn = t.y0 - 1;
}

static std::set<uint32_t> g_facts[4];  // distinct fact words seen, by log2 size - 2
static long g_partial = 0, g_none = 0;

static void one_tb(const Tb &t, int chroma, int k) {
    const int n = t.n, ns = 4 * n + 1;
    const int lsx = t.log2ctb - t.subx, csx = 1 << lsx, csy = 1 << (t.log2ctb - t.suby);
    const int ctu = t.hasl ? 1 : 0, r = t.hasa ? 1 : 0;
    TbGeom g;
    g.log2ctb = t.log2ctb;
    g.chroma = chroma;
    g.W = (ctu << t.log2ctb) + (t.vw << t.subx);
    g.H = (r << t.log2ctb) + (t.vh << t.suby);
    g.cw = chroma ? g.W >> chroma_sx(chroma) : 0;
    g.ch = chroma ? g.H >> chroma_sy(chroma) : 0;
    TuRec q{};
    q.x = (uint16_t)(ctu * csx + t.x0);
    q.y = (uint16_t)(r * csy + t.y0);
    q.log2 = (uint8_t)(31 - __builtin_clz((unsigned)n));
    q.mode = 1;
    q.flags = (uint8_t)k;
    q.ctu = (uint16_t)ctu;
    const uint32_t a = tb_pack_a(q, g, r);
    CHECK(a & TBA_OK);
    const uint32_t d = tb_pack_d(a, g, ctu, r);
    ++g_cases;
    g_facts[q.log2 - 2].insert(d & TBD_FACTS);
    // (d) the TB's first sample in its window
    CHECK(tbd_off(d) == (t.y0 << lsx) + t.x0);
    // (a) the facts, expanded, are the per-sample bits
    std::vector<char> av(ns);
    for (int s = 0; s < ns; ++s) {
        int xn, yn;
        search_xy(t, s, &xn, &yn);
        av[s] = sample_avail(t, xn, yn);
    }
    const int bl = tbd_bl(d), ar = tbd_ar(d);
    CHECK(bl >= 0 && bl <= n && !(bl & 3) && ar >= 0 && ar <= n && !(ar & 3));
    bool any = false;
    for (int s = 0; s < ns; ++s) {
        bool f;
        if (s < n) f = s >= n - bl;  // below-left: nearest the TB first
        else if (s < 2 * n) f = (d & TBD_LEFT) != 0;
        else if (s == 2 * n) f = (d & TBD_CORNER) != 0;
        else if (s <= 3 * n) f = (d & TBD_ABOVE) != 0;
        else f = s < 3 * n + 1 + ar;  // above-right: left to right
        CHECK(f == (bool)av[s]);
        any |= f;
    }
    g_partial += (bl > 0 && bl < n) || (ar > 0 && ar < n);
    g_none += !any;
    // (b) the substitution source, (c) where it is read
    const int cur = 0, left = csx * csy + 40, above = left + csy + 24;  // the three arrays, apart from each other
    const TbSrcAddr sa = tb_src_addr(t.x0, t.y0, n, lsx, left - cur, above - cur);
    int first = -1;
    for (int s = 0; s < ns && first < 0; ++s)
        if (av[s]) first = s;
    CHECK(any ? tbd_first(d) == first : (d & (TBD_FACTS | (0xffu << TBD_FIRST_SHIFT))) == 0u);
    int last = -1;
    for (int s = 0; s < ns; ++s) {
        if (av[s]) last = s;
        const int want = !any ? -1 : (last >= 0 ? last : first);
        const int got = tb_subst_src(s, n, d);
        CHECK(got == want);
        if (got < 0) continue;
        int xn, yn;
        search_xy(t, got, &xn, &yn);
        const int e = cur + tb_src_at(sa, got);
        // the window holds: the CTB's samples row by row; the column left of it from row 0; the row
        // above it from the corner (2 csx + 1 samples)
        int at;
        if (yn < 0) {
            CHECK(xn + 1 >= 0 && xn + 1 <= 2 * csx);
            at = above + xn + 1;
        } else if (xn < 0) {
            CHECK(yn < csy);
            at = left + yn;
        } else {
            CHECK(xn < csx && yn < csy);
            at = cur + (yn << lsx) + xn;
        }
        CHECK(e == at);
    }
}

static void space() {
    for (int chroma = 1; chroma <= 3; ++chroma)
        for (int k = 0; k <= 1; ++k) {
            const int subx = k ? chroma_sx(chroma) : 0, suby = k ? chroma_sy(chroma) : 0;
            for (int log2ctb = 4; log2ctb <= 6; ++log2ctb) {
                const int csl = 1 << log2ctb, csx = csl >> subx, csy = csl >> suby;
                for (int log2n = 2; log2n <= 5; ++log2n) {
                    const int n = 1 << log2n;
                    if (n > csx || n > csy) continue;
                    for (int x0 = 0; x0 < csx; x0 += n)
                        for (int y0 = 0; y0 < csy; y0 += n) {
                            // extents in luma samples: to the end of the next CTB and beyond it; to the
                            // end of this CTB row and beyond it
                            std::vector<int> vws, vhs;
                            for (int v = 8; v <= 2 * csl; v += 8)
                                if ((v >> subx) >= x0 + n) vws.push_back(v >> subx);
                            vws.push_back((4 * csl) >> subx);
                            for (int v = 8; v <= csl; v += 8)
                                if ((v >> suby) >= y0 + n) vhs.push_back(v >> suby);
                            vhs.push_back((3 * csl) >> suby);
                            for (int vw : vws)
                                for (int vh : vhs)
                                    for (int e = 0; e < 4; ++e) {
                                        Tb t{log2ctb, subx, suby, x0, y0, n, vw, vh, (e & 1) != 0, (e & 2) != 0};
                                        one_tb(t, chroma, k ? 1 + (int)((g_cases >> 3) & 1) : 0);
                                    }
                        }
                }
            }
        }
    // partial prefixes exist (the picture's edge cuts a group) and so does "nothing available"
    CHECK(g_partial > 1000 && g_none > 1000);
    for (int i = 0; i < 4; ++i) CHECK(g_facts[i].size() >= 7);
}

// every combination of the five facts, reachable or not: the closed form against the search-order rule
static void all_facts() {
    for (int log2n = 2; log2n <= 5; ++log2n) {
        const int n = 1 << log2n, ns = 4 * n + 1;
        for (int bl4 = 0; bl4 <= n / 4; ++bl4)
            for (int ar4 = 0; ar4 <= n / 4; ++ar4)
                for (int f = 0; f < 8; ++f) {
                    const uint32_t d = tbd_make(n, bl4, ar4, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, 0);
                    CHECK(tbd_bl(d) == 4 * bl4 && tbd_ar(d) == 4 * ar4 && tbd_off(d) == 0);
                    std::vector<char> av(ns, 0);
                    for (int s = n - 4 * bl4; s < n; ++s) av[s] = 1;
                    for (int s = n; s < 2 * n; ++s) av[s] = (f & 1) != 0;
                    av[2 * n] = (f & 4) != 0;
                    for (int s = 2 * n + 1; s <= 3 * n; ++s) av[s] = (f & 2) != 0;
                    for (int s = 3 * n + 1; s < 3 * n + 1 + 4 * ar4; ++s) av[s] = 1;
                    int first = -1, last = -1;
                    for (int s = 0; s < ns && first < 0; ++s)
                        if (av[s]) first = s;
                    for (int s = 0; s < ns; ++s) {
                        if (av[s]) last = s;
                        CHECK(tb_subst_src(s, n, d) == (first < 0 ? -1 : (last >= 0 ? last : first)));
                    }
                }
    }
}

static void not_ok() {
    for (int log2ctb = 4; log2ctb <= 6; ++log2ctb)
        for (int chroma = 0; chroma <= 3; ++chroma) {
            TbGeom g;
            g.log2ctb = log2ctb;
            g.chroma = chroma;
            g.W = 3 << log2ctb;
            g.H = 3 << log2ctb;
            g.cw = chroma ? g.W >> chroma_sx(chroma) : 0;
            g.ch = chroma ? g.H >> chroma_sy(chroma) : 0;
            for (int ctu = 0; ctu < 3; ++ctu)
                for (int r = 0; r < 3; ++r) {
                    CHECK(tb_pack_d(0u, g, ctu, r) == 0u);
                    // the fields of a word A without its OK bit never reach word D
                    CHECK(tb_pack_d(~TBA_OK, g, ctu, r) == 0u);
                    TuRec q{};
                    q.x = (uint16_t)(1 << log2ctb);
                    q.y = (uint16_t)(1 << log2ctb);
                    q.log2 = 2;
                    q.ctu = 1;
                    q.mode = 35;  // no such mode
                    CHECK(tb_pack_d(tb_pack_a(q, g, 1), g, 1, 1) == 0u);
                    q.mode = 1;
                    q.log2 = 6;  // no such TB
                    CHECK(tb_pack_d(tb_pack_a(q, g, 1), g, 1, 1) == 0u);
                    q.log2 = 2;
                    q.ctu = 2;  // another CTB than the record says
                    CHECK(tb_pack_d(tb_pack_a(q, g, 1), g, 2, 1) == 0u);
                    q.ctu = 1;
                    CHECK((tb_pack_a(q, g, 1) & TBA_OK) && tb_pack_d(tb_pack_a(q, g, 1), g, 1, 1) != 0u);
                }
        }
}

int main() {
    space();
    all_facts();
    not_ok();
    printf("INTRA AVAIL OK %ld cases %ld checks\n", g_cases, g_checks);
    return 0;
}
