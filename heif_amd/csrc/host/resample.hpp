// resample.hpp (host) — kernels/resample.hpp run on the host: the coefficient rows of one
// axis and the two passes over an interleaved buffer.  heifgpu_resample_coeffs and
// heifgpu_resample_apply are these; tests/resample/resample_driver.cpp links them alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../kernels/resample.hpp"

namespace hg {

// the sizes one axis takes: side 1..65535, window [in0, in1) non-empty inside it, out 1..65535,
// filter RS_BILINEAR or RS_BICUBIC, bits 8..12
bool resample_axis_ok(int64_t in_size, int64_t in0, int64_t in1, int64_t out, int64_t filter, int64_t bits);

// Pillow's precompute_coeffs + normalize_coeffs_8bpc at P = rs_precision(bits).  Returns the row
// length ksize.  bounds (2 * out: first tap, tap count) and kk (out * ksize, rows padded with
// zeros) are filled when not null.
int resample_coeffs(int in_size, int in0, int in1, int out, int filter, int bits, int32_t *bounds, int32_t *kk);

// The two passes over in (in_h x in_w x ch samples of bps bytes, interleaved, tight): window
// (wx, wy, ww, wh) onto out (oh x ow x ch, the same layout).
void resample_apply(const void *in, int bps, int in_w, int in_h, int ch, int bits, int wx, int wy, int ww, int wh,
                    int ow, int oh, int filter, void *out);

}  // namespace hg
