// The record-side arithmetic of the transform (kernels/xform_rec.hpp) as a stand-alone
// program, built under ASan + UBSan by `make xform-pack-asan`:
//  - levelScale without the table against the table, over every qp a record can hold;
//  - the scaling against 8.6.3 on a wider product, over every legal qP and bdShift at the
//    ends of the level and of the scaling factor;
//  - the DC-only test over every significance map and sub-block position, with random
//    sign, scan, hidden-sign and escape bits;
//  - the extents over every pair of sub-block coordinates, damaged ones included.
#include <cstdint>
#include <cstdio>
#include <random>

#include "kernels/xform_rec.hpp"

using namespace hg;

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

int main() {
    static const int tab[6] = {40, 45, 51, 57, 64, 72};
    for (int qp = 0; qp < 256; ++qp) {
        const int per = qp / 6 < 16 ? qp / 6 : 16;
        const int64_t want = (int64_t)tab[qp % 6] << per;
        CHECK(xf_level_scale(qp) == want, "qp %d: %d", qp, xf_level_scale(qp));
    }
    CHECK(xf_level_scale(99) == (57 << 16), "the largest legal qP");

    // the scaling at the ends of its operands: 8.6.3 restated on a 128-bit product
    uint64_t compared = 0;
    for (int qp = 0; qp < 100; ++qp) {
        const int ls = xf_level_scale(qp);
        for (int bd_shift = 5; bd_shift <= 16; ++bd_shift)
            for (int m : {1, 16, 255})
                for (int v : {-32768, -32767, -256, -255, -1, 0, 1, 255, 256, 32766, 32767}) {
                    __int128 t = (__int128)v * m * ls + ((__int128)1 << (bd_shift - 1));
                    t = t >= 0 ? t >> bd_shift : -((-t + (((__int128)1 << bd_shift) - 1)) >> bd_shift);  // floor
                    const int want = t < -32768 ? -32768 : (t > 32767 ? 32767 : (int)t);
                    ++compared;
                    CHECK(xf_scale64(v, m, ls, bd_shift) == want, "v %d m %d ls %d bd_shift %d", v, m, ls, bd_shift);
                }
    }
    CHECK(xf_scale64(32767, 255, xf_level_scale(99), 16) == 32767 && xf_scale64(-32768, 255, xf_level_scale(99), 13) == -32768,
          "16 bits qP 99");

    // DC-only: exactly sig == 1 at sub-block (0, 0)
    std::mt19937 rng(24);
    for (uint32_t sig = 0; sig < 65536; ++sig)
        for (uint32_t sb = 0; sb < 64; ++sb) {
            const uint32_t w0 = sig | (rng() & 0xffff0000u), w3 = sb | (rng() & ~63u);
            CHECK(xf_dc_record(w0, w3) == (sig == 1 && sb == 0), "sig %x sb %u", sig, sb);
        }

    // extents
    for (int log2n = 2; log2n <= 5; ++log2n) {
        const int n = 1 << log2n;
        for (int xs = 0; xs < 8; ++xs)
            for (int ys = 0; ys < 8; ++ys) {
                int r4 = -1, c4 = -1;
                xf_extents(xs, ys, n, &r4, &c4);
                const bool in = xs < n / 4 && ys < n / 4;
                CHECK(r4 == (in ? 4 * (ys + 1) : n) && c4 == (in ? 4 * (xs + 1) : n), "n %d xs %d ys %d: %d %d", n, xs, ys, r4, c4);
                CHECK(r4 >= 4 && r4 <= n && c4 >= 4 && c4 <= n && r4 % 4 == 0 && c4 % 4 == 0, "n %d xs %d ys %d", n, xs, ys);
            }
    }
    if (fails) {
        std::printf("XFORM PACK FAILED: %d checks\n", fails);
        return 1;
    }
    std::printf("XFORM PACK OK: %llu scalings compared\n", (unsigned long long)compared);
    return 0;
}
