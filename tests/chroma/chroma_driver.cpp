// chroma_driver.cpp — the chroma upsampling rule (kernels/chroma_up.hpp) and its host hook
// (host/chroma.cpp: what heifgpu_chroma_upsample runs) as a stand-alone program for ASan +
// UBSan (make chroma-asan; tests/test_chroma.py runs it).  Every plane is a heap block of
// exactly w_c * h_c samples and every output one of exactly w * h, so a tap that misses its
// clamp, or a write past the rectangle, is a heap overflow the sanitizer reports.  The values
// are checked against the rule written out per sample with the taps of the header.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host/chroma.hpp"

using namespace hg;

static int failures = 0;

template <typename T>
static void one_case(uint32_t wc, uint32_t hc, uint32_t bits, uint32_t fmt, uint32_t loc, uint32_t x0, uint32_t y0,
                     uint32_t w, uint32_t h, uint32_t pattern) {
    const uint32_t maxv = (1u << bits) - 1;
    T *in = static_cast<T *>(std::malloc(sizeof(T) * wc * hc));
    T *out = static_cast<T *>(std::malloc(sizeof(T) * w * h));
    uint32_t lcg = 12345u + pattern * 977u + wc * 31u + hc;
    for (uint32_t k = 0; k < wc * hc; ++k) {
        lcg = lcg * 1664525u + 1013904223u;
        const uint32_t x = k % wc, y = k / wc;
        in[k] = T(pattern == 0 ? 0 : pattern == 1 ? maxv : pattern == 2 ? (((x + y) & 1) ? maxv : 0) : (lcg >> 8) & maxv);
    }
    const char *err = chroma_upsample_rect(in, wc, hc, int64_t(wc * sizeof(T)), bits, fmt, loc, x0, y0, w, h, out,
                                           int64_t(w * sizeof(T)));
    if (err) {
        std::printf("FAIL %ux%u fmt %u loc %u: %s\n", wc, hc, fmt, loc, err);
        ++failures;
    } else {
        int px, py;
        chroma_phase(int(fmt), int(loc), px, py);
        for (uint32_t j = 0; j < h && !failures; ++j)
            for (uint32_t i = 0; i < w; ++i) {
                const ChromaTap tx = chroma_tap(int(x0 + i), px, int(wc)), ty = chroma_tap(int(y0 + j), py, int(hc));
                if (tx.i0 < 0 || tx.i1 >= int(wc) || ty.i0 < 0 || ty.i1 >= int(hc) || tx.w0 + tx.w1 != 4 || ty.w0 + ty.w1 != 4) {
                    std::printf("FAIL tap outside the plane at (%u, %u)\n", x0 + i, y0 + j);
                    ++failures;
                    break;
                }
                const int want = chroma_value(in[ty.i0 * wc + tx.i0], in[ty.i0 * wc + tx.i1], in[ty.i1 * wc + tx.i0],
                                              in[ty.i1 * wc + tx.i1], tx, ty);
                if (int(out[j * w + i]) != want || want < 0 || want > int(maxv)) {
                    std::printf("FAIL value at (%u, %u): %d, want %d\n", x0 + i, y0 + j, int(out[j * w + i]), want);
                    ++failures;
                    break;
                }
            }
    }
    std::free(in);
    std::free(out);
}

int main() {
    int cases = 0;
    const uint32_t sides[4] = {1, 2, 3, 5};
    for (uint32_t fmt = 1; fmt <= 2; ++fmt)
        for (uint32_t loc = 0; loc < 6; ++loc)
            for (uint32_t wc : sides)
                for (uint32_t hc : sides)
                    for (uint32_t pattern = 0; pattern < 4; ++pattern) {
                        const uint32_t W = 2 * wc, H = (fmt == 1 ? 2 : 1) * hc;
                        // the whole luma grid, then rectangles from odd and even offsets to the far corner
                        one_case<uint8_t>(wc, hc, 8, fmt, loc, 0, 0, W, H, pattern);
                        one_case<uint16_t>(wc, hc, 12, fmt, loc, 0, 0, W, H, pattern);
                        one_case<uint16_t>(wc, hc, 16, fmt, loc, W - 1, H - 1, 1, 1, pattern);
                        if (W > 1) one_case<uint8_t>(wc, hc, 8, fmt, loc, 1, H > 1 ? 1 : 0, W - 1, H > 1 ? H - 1 : 1, pattern);
                        cases += 3 + (W > 1);
                    }
    // refusals: nothing may be written or read
    uint8_t one = 7, dst = 9;
    const bool refused = chroma_upsample_rect(&one, 1, 1, 1, 8, 3, 0, 0, 0, 1, 1, &dst, 1) &&  // 4:4:4
                         chroma_upsample_rect(&one, 1, 1, 1, 8, 1, 6, 0, 0, 1, 1, &dst, 1) &&  // location 6
                         chroma_upsample_rect(&one, 1, 1, 1, 8, 1, 0, 2, 0, 1, 1, &dst, 1) &&  // x0 outside
                         chroma_upsample_rect(&one, 1, 1, 1, 8, 1, 0, 0, 0, 3, 1, &dst, 3) &&  // too wide
                         chroma_upsample_rect(&one, 1, 1, 0, 8, 1, 0, 0, 0, 1, 1, &dst, 1) &&  // pitch
                         chroma_upsample_rect(nullptr, 1, 1, 1, 8, 1, 0, 0, 0, 1, 1, &dst, 1);
    if (!refused || dst != 9) {
        std::printf("FAIL a bad argument was accepted\n");
        ++failures;
    }
    std::printf("cases %d\n", cases);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
