// chroma.hpp — the host side of bilinear chroma upsampling (kernels/chroma_up.hpp has the
// rule): what an image's setting means for a render, the rule over a rectangle of the luma
// grid (heifgpu_chroma_upsample), and the rectangle of chroma samples a luma box taps
// (window_source_rect).  No GPU, no other unit of the library: the stand-alone
// sanitizer driver (make chroma-asan) links this file alone.
#pragma once
#include <cstdint>

#include "../kernels/chroma_up.hpp"

namespace hg {

// What the render kernels and window_source_rect read of an image: mode 0 (replicate; also
// every 4:4:4 and 4:0:0 image, whatever it is set to) or 1 with the phases of its sample
// location and its chroma planes' size.  (The layout of kernels.hpp's ChromaRef.)
struct ChromaUp {
    int32_t mode, px, py, wc, hc, pad;
};
// mode: the image's setting; loc: the location in force (0..5); W x H: the decoded luma planes
ChromaUp chroma_up_for(uint32_t mode, int loc, int chroma_format, uint32_t W, uint32_t H);

// The chroma samples [c0, c1] (inclusive) of an axis that luma positions [p0, p1] tap, both
// taps of every position whatever their weights (the kernels load both).
void chroma_tap_span(int p0, int p1, int ph, int n, int &c0, int &c1);

// C' (kernels/chroma_up.hpp) of one chroma plane `in` (w_c x h_c samples of `bits` bits,
// uint8 for bits == 8, else uint16; pitch in bytes) over the luma-grid rectangle
// [x0, x0 + w) x [y0, y0 + h) into `out` (same sample type, out_pitch bytes a row).
// Returns 0, or a message for arguments outside the rule's range (nothing is written then).
const char *chroma_upsample_rect(const void *in, uint32_t w_c, uint32_t h_c, int64_t pitch, uint32_t bits,
                                 uint32_t chroma_format, uint32_t loc, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                 void *out, int64_t out_pitch);

}  // namespace hg
