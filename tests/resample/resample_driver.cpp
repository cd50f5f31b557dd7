// resample_driver.cpp — the resampling's host hooks (heif_amd/csrc/host/resample.cpp over
// kernels/resample.hpp) over degenerate sizes, as a stand-alone program built with
// ASan + UBSan (`make resample-asan`; tests/test_resample.py runs it).  Nothing here
// touches a device.
//
// Every buffer is a heap allocation of exactly the size the call may touch, so a read or
// write past an end is an ASan report.  For every case the program also checks what the
// contract promises of a coefficient row: taps inside the side, at most ksize of them, and
// coefficients that sum to 1 << P within one unit per tap.  Prints one line per case and
// "ok"; exit status 1 on a broken promise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host/resample.hpp"

static int g_bad = 0;

static void axis_case(int in_size, int in0, int in1, int out, int filter, int bits) {
    const int ks = hg::resample_coeffs(in_size, in0, in1, out, filter, bits, nullptr, nullptr);
    std::vector<int32_t> bounds(size_t(out) * 2), kk(size_t(out) * size_t(ks));  // exact capacity
    hg::resample_coeffs(in_size, in0, in1, out, filter, bits, bounds.data(), kk.data());
    const int P = hg::rs_precision(bits);
    int worst = 0;
    for (int X = 0; X < out; ++X) {
        const int lo = bounds[2 * size_t(X)], n = bounds[2 * size_t(X) + 1];
        if (lo < 0 || n < 1 || n > ks || lo + n > in_size) {
            std::printf("  bad taps at %d: [%d, %d)\n", X, lo, lo + n);
            ++g_bad;
            break;
        }
        int64_t sum = 0;
        for (int t = 0; t < ks; ++t) sum += kk[size_t(X) * size_t(ks) + size_t(t)];
        const int off = int(std::llabs(sum - (int64_t(1) << P)));
        if (off > n) {
            std::printf("  bad sum at %d: off by %d over %d taps\n", X, off, n);
            ++g_bad;
            break;
        }
        worst = off > worst ? off : worst;
    }
    std::printf("axis %5d [%5d,%5d) -> %5d filter %d bits %2d: ksize %6d, sums within %d\n", in_size, in0, in1, out, filter,
                bits, ks, worst);
}

template <class T>
static void apply_case(int w, int h, int ch, int bits, int wx, int wy, int ww, int wh, int ow, int oh, int filter) {
    const int maxv = (1 << bits) - 1;
    std::vector<T> in(size_t(w) * size_t(h) * size_t(ch)), out(size_t(ow) * size_t(oh) * size_t(ch));
    for (size_t k = 0; k < in.size(); ++k) in[k] = T(((k / size_t(ch)) % 3) ? maxv : 0);  // hard edges: both clips
    hg::resample_apply(in.data(), int(sizeof(T)), w, h, ch, bits, wx, wy, ww, wh, ow, oh, filter, out.data());
    int top = 0;
    for (T v : out) top = v > top ? v : top;
    if (top > maxv) {
        std::printf("  result above maxv\n");
        ++g_bad;
    }
    std::printf("apply %dx%d c%d bits %d window (%d,%d,%d,%d) -> %dx%d filter %d: max %d\n", w, h, ch, bits, wx, wy, ww, wh,
                ow, oh, filter, top);
}

int main() {
    for (int filter = hg::RS_BILINEAR; filter <= hg::RS_BICUBIC; ++filter)
        for (int bits = 8; bits <= 12; bits += 2) {
            axis_case(1, 0, 1, 1, filter, bits);
            axis_case(1, 0, 1, 65535, filter, bits);
            axis_case(65535, 0, 65535, 1, filter, bits);
            axis_case(65535, 0, 65535, 65535, filter, bits);
            axis_case(65535, 0, 1, 7, filter, bits);          // a window at the left edge
            axis_case(65535, 65534, 65535, 7, filter, bits);  // at the right edge
            axis_case(4032, 504, 3528, 224, filter, bits);
            axis_case(100, 0, 50, 33, filter, bits);
            axis_case(100, 50, 100, 33, filter, bits);
            axis_case(100, 37, 38, 1, filter, bits);
        }
    for (int filter = hg::RS_BILINEAR; filter <= hg::RS_BICUBIC; ++filter) {
        apply_case<uint8_t>(1, 1, 3, 8, 0, 0, 1, 1, 1, 1, filter);
        apply_case<uint8_t>(1, 1, 4, 8, 0, 0, 1, 1, 9, 5, filter);
        apply_case<uint8_t>(65535, 1, 1, 8, 0, 0, 65535, 1, 1, 1, filter);
        apply_case<uint8_t>(1, 65535, 1, 8, 0, 0, 1, 65535, 1, 1, filter);
        apply_case<uint8_t>(1, 1, 1, 8, 0, 0, 1, 1, 65535, 1, filter);
        apply_case<uint8_t>(41, 29, 3, 8, 0, 0, 41, 29, 17, 11, filter);
        apply_case<uint8_t>(41, 29, 3, 8, 0, 0, 5, 4, 17, 11, filter);      // the top left corner
        apply_case<uint8_t>(41, 29, 3, 8, 36, 25, 5, 4, 17, 11, filter);    // the bottom right corner
        apply_case<uint16_t>(41, 29, 4, 10, 40, 0, 1, 29, 3, 64, filter);   // the right edge
        apply_case<uint16_t>(41, 29, 3, 12, 0, 28, 41, 1, 64, 3, filter);   // the bottom edge
    }
    std::printf(g_bad ? "FAILED\n" : "ok\n");
    return g_bad ? 1 : 0;
}
