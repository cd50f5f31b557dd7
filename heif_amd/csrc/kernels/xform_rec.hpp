// xform_rec.hpp — what the scaling and the inverse transform read off a TB's
// records without touching the coefficient tile (k_transform, k_intra's
// streaming mode): levelScale without the table load, the scaling, the DC-only
// test on a sub-block record's words and the 4-sample extents of a TB from its
// records' sub-block coordinates.
// Plain inline functions, so the host emulation and a stand-alone sanitizer
// driver (make xform-pack-asan) run the same arithmetic as the kernels.
#pragma once
#include <stdint.h>

#include "../common/desc.hpp"

#if !defined(HG_REC_FN)
#if defined(__HIPCC__) && !defined(HG_HOST_EMU)
#define HG_REC_FN __host__ __device__ __forceinline__
#else
#define HG_REC_FN inline
#endif
#endif

namespace hg {

// levelScale[qp % 6] << (qp / 6) of 8.6.3, the table {40, 45, 51, 57, 64, 72}
// as the bytes of one constant (a constant-memory load and its wait per TB
// before).  The largest legal qP is 51 + 6 * (16 - 8) = 99, a shift of 16; a
// damaged record's qp (up to 255) shifts no further.
HG_REC_FN int xf_level_scale(int qp) {
    const uint64_t tab = 40ull | (45ull << 8) | (51ull << 16) | (57ull << 24) | (64ull << 32) | (72ull << 40);
    const int per = (qp & 255) / 6, rem = (qp & 255) - 6 * per;
    return (int)((tab >> (8 * rem)) & 0xffu) << (per < 16 ? per : 16);
}

HG_REC_FN int xf_clip16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// 8.6.3 as the standard writes it: Clip3(-32768, 32767, (v * m * ls + (1 << (bdShift - 1))) >> bdShift)
HG_REC_FN int xf_scale64(int v, int m, int ls, int bd_shift) {
    const int64_t t = ((int64_t)v * m * ls + ((int64_t)1 << (bd_shift - 1))) >> bd_shift;
    return t < -32768 ? -32768 : (t > 32767 ? 32767 : (int)t);
}

// A TB of one sub-block record is DC-only when that record lies at sub-block
// (0, 0) and codes scan position 0 alone: position 0 is sample (0, 0) in all
// three scans (6.5.3-6.5.5).  w0, w3: the record's words (SbRec, desc.hpp).
HG_REC_FN bool xf_dc_record(uint32_t w0, uint32_t w3) { return (w0 & 0xffffu) == 1u && (w3 & 63u) == 0u; }

// Rows (columns) of a TB of size n that can hold a coefficient, from the largest
// yS (xS) among its records: 4 * (max + 1).  A coordinate outside the TB (a
// damaged record: the scatter wraps its positions) makes both the whole TB.
HG_REC_FN void xf_extents(int xs_max, int ys_max, int n, int *rows4, int *cols4) {
    const bool in = 4 * xs_max < n && 4 * ys_max < n;
    *rows4 = in ? 4 * (ys_max + 1) : n;
    *cols4 = in ? 4 * (xs_max + 1) : n;
}

}  // namespace hg
