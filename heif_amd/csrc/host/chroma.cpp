// chroma.cpp — see chroma.hpp.
#include "chroma.hpp"

#include <algorithm>

namespace hg {

ChromaUp chroma_up_for(uint32_t mode, int loc, int chroma_format, uint32_t W, uint32_t H) {
    ChromaUp c{};
    if (!mode || (chroma_format != 1 && chroma_format != 2)) return c;  // nothing to interpolate
    c.mode = 1;
    chroma_phase(chroma_format, loc, c.px, c.py);
    c.wc = int32_t((W + 1) >> 1);
    c.hc = chroma_format == 1 ? int32_t((H + 1) >> 1) : int32_t(H);
    return c;
}

void chroma_tap_span(int p0, int p1, int ph, int n, int &c0, int &c1) {
    // (both taps are monotonic in the position)
    const ChromaTap a = chroma_tap(p0, ph, n), b = chroma_tap(p1, ph, n);
    c0 = std::min(a.i0, a.i1);
    c1 = std::max(b.i0, b.i1);
}

template <typename T>
static void upsample(const uint8_t *in, int wc, int hc, int64_t pitch, int px, int py, uint32_t x0, uint32_t y0,
                     uint32_t w, uint32_t h, uint8_t *out, int64_t out_pitch) {
    for (uint32_t j = 0; j < h; ++j) {
        const ChromaTap ty = chroma_tap(int(y0 + j), py, hc);
        const T *r0 = reinterpret_cast<const T *>(in + int64_t(ty.i0) * pitch);
        const T *r1 = reinterpret_cast<const T *>(in + int64_t(ty.i1) * pitch);
        T *o = reinterpret_cast<T *>(out + int64_t(j) * out_pitch);
        for (uint32_t i = 0; i < w; ++i) {
            const ChromaTap tx = chroma_tap(int(x0 + i), px, wc);
            o[i] = T(chroma_value(r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1], tx, ty));
        }
    }
}

const char *chroma_upsample_rect(const void *in, uint32_t w_c, uint32_t h_c, int64_t pitch, uint32_t bits,
                                 uint32_t chroma_format, uint32_t loc, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                 void *out, int64_t out_pitch) {
    if (!in || !out) return "null argument";
    if (chroma_format != 1 && chroma_format != 2) return "chroma_format_idc is neither 1 (4:2:0) nor 2 (4:2:2)";
    if (loc > 5) return "sample location above 5";
    if (bits < 8 || bits > 16) return "bit depth outside 8..16";
    const int64_t bps = bits > 8 ? 2 : 1;
    if (!w_c || !h_c || w_c > 65536 || h_c > 65536) return "chroma plane side outside 1..65536";
    if (pitch < int64_t(w_c) * bps || out_pitch < int64_t(w) * bps) return "pitch smaller than a row";
    if (bps == 2 && ((pitch | out_pitch) & 1)) return "pitch of 2-byte samples is odd";
    // the rectangle lies on the luma grid of the plane: at most 2 * w_c columns, h_c or 2 * h_c rows
    const uint64_t W = 2 * uint64_t(w_c), H = (chroma_format == 1 ? 2 : 1) * uint64_t(h_c);
    if (!w || !h || x0 >= W || y0 >= H || w > W - x0 || h > H - y0) return "rectangle empty or outside the luma grid";
    int px, py;
    chroma_phase(int(chroma_format), int(loc), px, py);
    if (bps == 1)
        upsample<uint8_t>(static_cast<const uint8_t *>(in), int(w_c), int(h_c), pitch, px, py, x0, y0, w, h,
                          static_cast<uint8_t *>(out), out_pitch);
    else
        upsample<uint16_t>(static_cast<const uint8_t *>(in), int(w_c), int(h_c), pitch, px, py, x0, y0, w, h,
                           static_cast<uint8_t *>(out), out_pitch);
    return nullptr;
}

}  // namespace hg
