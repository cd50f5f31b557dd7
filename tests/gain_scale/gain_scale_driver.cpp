// The averaging of Q8 gain codes (kernels/gain_scale.hpp) as a stand-alone program, built under
// ASan + UBSan by `make gain-scale-asan`, against 128-bit arithmetic:
//  - the two-step quotient over the whole stated range: split sums up to 65535^2 * 4095 and
//    65535^2 * 255 (numerators up to 2^54), denominators 2 cw ch up to 2^33, at the ends, around
//    every multiple of the denominator that the ends reach, and at random;
//  - the small quotient at the ends of its regime (numerator 2^46, quotient 2^12);
//  - the weights: those of an output index add up to the window's side, over awkward ratios;
//  - the column and whole sums at their largest values (every weight on the largest code);
//  - gs_average_window over small windows against the contract's formula on 128-bit sums,
//    identity and 1 x 1 included, with exact-capacity buffers;
//  - what the kernel's walk adds to kernels/gain_xform.hpp: the row taps walked in integers
//    (GainTapWalk) against gain_tap at every position, forwards, backwards and after jumps, at
//    sides up to 65535; the sampler in its two steps against gain_sample over every fx, fy.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "kernels/gain_scale.hpp"
#include "kernels/gain_xform.hpp"

using namespace hg;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (++fails <= 20) {                        \
                std::printf("FAIL %s: ", #c);           \
                std::printf(__VA_ARGS__);               \
                std::printf("\n");                      \
            }                                           \
        }                                               \
    } while (0)

static uint64_t compared = 0, above46 = 0;

static void check_average(uint64_t hi, uint64_t lo, uint64_t cwch) {
    const uint64_t den = 2 * cwch;
    const u128 num = 2 * ((u128)256 * hi + lo) + cwch;
    const uint64_t want = (uint64_t)(num / den);
    const GsSum s = {hi, lo};
    const uint32_t got = gs_average(s, den, 1.0 / (double)den);
    ++compared;
    if (num >> 46) ++above46;
    CHECK(got == want, "hi %llu lo %llu cw ch %llu: %u, want %llu", (unsigned long long)hi, (unsigned long long)lo,
          (unsigned long long)cwch, got, (unsigned long long)want);
}

// the contract's average of a window, on 128-bit sums
static uint32_t average_ref(const std::vector<uint32_t> &g, uint32_t W, uint32_t cx, uint32_t cy, uint32_t cw, uint32_t ch,
                            uint32_t ow, uint32_t oh, uint32_t X, uint32_t Y) {
    u128 sum = 0;
    for (uint32_t j = 0; j < ch; ++j) {
        const int64_t a = (int64_t)(j + 1) * oh, b = (int64_t)(Y + 1) * ch, c = (int64_t)j * oh, d = (int64_t)Y * ch;
        const int64_t wy = (a < b ? a : b) - (c > d ? c : d);
        if (wy <= 0) continue;
        for (uint32_t i = 0; i < cw; ++i) {
            const int64_t e = (int64_t)(i + 1) * ow, f = (int64_t)(X + 1) * cw, p = (int64_t)i * ow, q = (int64_t)X * cw;
            const int64_t wx = (e < f ? e : f) - (p > q ? p : q);
            if (wx > 0) sum += (u128)(wy * wx) * g[(size_t)(cy + j) * W + cx + i];
        }
    }
    const uint64_t cwch = (uint64_t)cw * ch;
    return (uint32_t)((2 * sum + cwch) / (2 * cwch));
}

int main() {
    std::mt19937_64 rng(26);
    // ---- the quotient
    const uint64_t sides[] = {1, 2, 3, 255, 256, 4097, 16400, 32768, 46341, 65521, 65534, 65535};
    for (uint64_t cw : sides)
        for (uint64_t ch : sides) {
            const uint64_t area = cw * ch, hmax = area * 4095, lmax = area * 255;
            // the ends
            for (uint64_t hi : {(uint64_t)0, (uint64_t)1, hmax / 2, hmax - 1, hmax})
                for (uint64_t lo : {(uint64_t)0, (uint64_t)1, lmax / 2, lmax - 1, lmax}) check_average(hi, lo, area);
            // around exact halves and multiples: sums whose average lands on a boundary
            for (int k = 0; k < 64; ++k) {
                const uint64_t code = rng() % (kGainScaleMaxCode + 1);  // all pixels `code`: the average is code
                const uint64_t hi = area * (code >> 8), lo = area * (code & 255);
                check_average(hi, lo, area);
                // one unit below and above half the denominator's step
                const uint64_t half = area / 2;
                if (lo + half <= lmax) check_average(hi, lo + half, area);
                if (lo + half + 1 <= lmax) check_average(hi, lo + half + 1, area);
                if (lo >= half + 1) check_average(hi, lo - half - 1, area);
                if (lo >= half) check_average(hi, lo - half, area);
            }
            for (int k = 0; k < 2000; ++k) check_average(rng() % (hmax + 1), rng() % (lmax + 1), area);
        }
    // any split that the sums can hold, not only those of real codes: hi and lo independent
    for (int k = 0; k < 200000; ++k) {
        const uint64_t cw = 1 + rng() % 65535, ch = 1 + rng() % 65535, area = cw * ch;
        check_average(rng() % (area * 4095 + 1), rng() % (area * 255 + 1), area);
    }
    CHECK(above46 > 100000, "numerators above 2^46: %llu", (unsigned long long)above46);
    {
        const uint64_t area = 65535ull * 65535ull;  // the top: numerator 2 * 256 * 4095 * area + area > 2^53
        const GsSum top = {area * 4095, area * 255};  // (more than a real code's: the largest the two sums hold)
        CHECK(gs_average(top, 2 * area, 1.0 / (double)(2 * area)) == 256u * 4095u + 255u, "top");
        CHECK((2 * ((u128)256 * top.hi + top.lo) + area) >> 52, "the top numerator is above 2^52");
        CHECK(2 * area > (1ull << 32) && 2 * area <= (1ull << 33), "the largest denominator");
    }
    // ---- the small quotient at the ends of its regime
    for (int k = 0; k < 200000; ++k) {
        const uint64_t den = 1 + rng() % (1ull << 33);
        uint64_t q = rng() % 4096, r = rng() % den;
        if (k & 1) r = (k & 2) ? 0 : den - 1;
        const uint64_t num = q * den + r;
        if (num >> 46) continue;
        uint64_t rem;
        const uint32_t got = gs_div_small(num, den, 1.0 / (double)den, rem);
        ++compared;
        CHECK(got == q && rem == r, "num %llu den %llu", (unsigned long long)num, (unsigned long long)den);
    }
    // ---- the weights and the sums at their largest values
    const uint32_t ratios[][2] = {{65535, 1}, {65535, 2}, {65535, 65534}, {65534, 65535}, {1, 65535}, {4097, 3}, {16401, 7},
                                  {320, 100}, {48, 20}, {61, 90}, {57, 31}, {1056, 31}, {7, 7}};
    for (const auto &rt : ratios) {
        const uint32_t c = rt[0], o = rt[1];
        for (uint32_t X : {0u, o / 2, o - 1}) {
            uint32_t k0, k1;
            gs_footprint(X, c, o, k0, k1);
            CHECK(k1 <= c && k0 < k1, "footprint %u of %u -> %u", X, c, o);
            uint64_t total = 0;
            GsCol col = {0, 0};
            for (uint32_t k = k0; k < k1; ++k) {
                const uint32_t w = gs_weight(k, o, X * c, X * c + c);
                CHECK(w >= 1 && w <= (c < o ? c : o), "weight %u", w);
                total += w;
                gs_col_add(col, w, kGainScaleMaxCode);
            }
            CHECK(total == c, "weights of %u in %u -> %u add up to %llu", X, c, o, (unsigned long long)total);
            CHECK(col.hi == (uint64_t)c * 4095 && col.lo == 0, "column sum at the top");
            if (k0 > 0) CHECK((uint64_t)k0 * o <= (uint64_t)X * c, "first index");
            GsSum s = {0, 0};
            for (uint32_t k = k0; k < k1; ++k) gs_add(s, gs_weight(k, o, X * c, X * c + c), col.hi, 255u * c);
            CHECK(s.hi == (uint64_t)c * c * 4095 && s.lo == (uint64_t)c * c * 255, "whole sums at the top");
            CHECK(gs_average(s, 2 * (uint64_t)c * c, 1.0 / (double)(2 * (uint64_t)c * c)) == 256u * 4095u + 255u, "their average");
        }
    }
    // ---- windows: exact-capacity buffers
    const uint32_t cases[][8] = {  // W, H, cx, cy, cw, ch, ow, oh
        {64, 48, 3, 5, 57, 31, 20, 11}, {64, 48, 0, 0, 64, 48, 64, 48}, {64, 48, 0, 0, 64, 48, 32, 24},
        {64, 48, 1, 1, 61, 41, 90, 70}, {64, 48, 0, 0, 64, 48, 1, 1},   {33, 7, 32, 6, 1, 1, 5, 3},
        {17, 300, 0, 0, 17, 300, 2, 1}};
    for (const auto &c : cases) {
        const uint32_t W = c[0], H = c[1], cx = c[2], cy = c[3], cw = c[4], ch = c[5], ow = c[6], oh = c[7];
        std::vector<uint32_t> g((size_t)W * H);
        for (uint32_t &v : g) v = (rng() & 3) ? kGainScaleMaxCode - (uint32_t)(rng() % 600) : (uint32_t)(rng() % (kGainScaleMaxCode + 1));
        std::vector<uint32_t> out((size_t)ow * oh);
        std::vector<GsCol> col(cw);
        gs_average_window(g.data(), W, cx, cy, cw, ch, ow, oh, col.data(), out.data());
        for (uint32_t Y = 0; Y < oh; ++Y)
            for (uint32_t X = 0; X < ow; ++X) {
                const uint32_t want = average_ref(g, W, cx, cy, cw, ch, ow, oh, X, Y);
                ++compared;
                CHECK(out[(size_t)Y * ow + X] == want, "window case %u x %u -> %u x %u at %u, %u", cw, ch, ow, oh, X, Y);
                if (ow == cw && oh == ch) CHECK(want == g[(size_t)(cy + Y) * W + cx + X], "identity");
            }
    }
    // ---- the walk of the row taps
    const int sides2[][2] = {{1, 1}, {1, 65535}, {65535, 1}, {65535, 65535}, {65535, 65534}, {4032, 2016}, {3024, 1512},
                             {96, 40}, {64, 24}, {4224, 2112}, {4104, 40}, {48, 24}, {41, 65535}, {65521, 4099}};
    for (const auto &wd : sides2) {
        const int W = wd[0], Wg = wd[1];
        const double inv_w = 1.0 / (double)W;
        auto same = [&](const GainTapWalk &w, int s) {
            const GainTap a = gain_tap(s, W, Wg, inv_w), b = gain_tap_of(w.q, Wg);
            ++compared;
            CHECK(w.s == s && a.i0 == b.i0 && a.i1 == b.i1 && a.f == b.f, "walk W %d Wg %d at %d", W, Wg, s);
            CHECK((uint64_t)w.q * (uint32_t)W + w.rem == (uint64_t)(128u * (2u * (uint32_t)s + 1u)) * (uint32_t)Wg &&
                      w.rem < (uint32_t)W, "walk state W %d Wg %d at %d", W, Wg, s);
        };
        GainTapWalk w;
        gain_walk_start(w, 0, W, Wg, inv_w);
        same(w, 0);
        for (int s = 1; s < W; ++s) gain_walk_seek(w, s, W, Wg, inv_w), same(w, s);  // forwards
        for (int s = W - 1; s >= 0; --s) gain_walk_seek(w, s, W, Wg, inv_w), same(w, s);  // (first: stays), backwards
        for (int k = 0; k < 2000; ++k) {  // jumps, repeats and single steps mixed
            int s = (int)(rng() % (uint64_t)W);
            if (k % 3 == 1) s = w.s + 1 < W ? w.s + 1 : w.s;
            if (k % 3 == 2) s = w.s > 0 ? w.s - 1 : w.s;
            gain_walk_seek(w, s, W, Wg, inv_w);
            same(w, s);
        }
    }
    // ---- the sampler in two steps
    for (uint32_t fx = 0; fx < 256; ++fx)
        for (uint32_t fy = 0; fy < 256; ++fy) {
            uint32_t g[4];
            for (int rep = 0; rep < 3; ++rep) {
                for (uint32_t &v : g) v = rep == 0 ? 4095u : rep == 1 ? (uint32_t)(rng() % 4096) : (uint32_t)(rng() % 65536);
                const uint32_t want = gain_sample(g[0], g[1], g[2], g[3], fx, fy);
                const uint32_t got = gain_sample_rows(gain_sample_row(g[0], g[1], fx), gain_sample_row(g[2], g[3], fx), fy);
                ++compared;
                CHECK(got == want, "sampler fx %u fy %u", fx, fy);
            }
        }
    if (fails) {
        std::printf("GAIN SCALE FAILED: %d\n", fails);
        return 1;
    }
    std::printf("GAIN SCALE OK: %llu compared, %llu numerators above 2^46\n", (unsigned long long)compared,
                (unsigned long long)above46);
    return 0;
}
