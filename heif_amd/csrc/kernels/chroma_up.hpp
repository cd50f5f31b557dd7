// chroma_up.hpp — bilinear chroma upsampling at the signalled sample location: the one
// statement of the rule (include/heifgpu.h "chroma upsampling"), shared by the host
// (host/chroma.cpp: heifgpu_chroma_upsample, the window's source rectangle) and the three
// render kernels (render_px.hpp, render.hip, resample.hip).  Integers only.
//
// t is chroma_sample_loc_type_top_field (0..5).  4:2:0: the chroma grid lies px quarter
// chroma steps right of the even luma columns (px = t & 1: 0 co-sited, 1 midway) and
// py quarter steps below the even luma rows (py = 1 midway, 0 top, 2 bottom); 4:2:2 is
// co-sited horizontally and has a chroma row per luma row.  Luma position p of an axis
// reads chroma samples i0 = floor((2p - ph) / 4) and i0 + 1, each clamped to the plane,
// with weights 4 - f and f, f = (2p - ph) & 3, and
//   C'(x, y) = (sum wy * wx * C + 8) >> 4.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CU_HD __host__ __device__ inline
#else
#define CU_HD inline
#endif

namespace hg {

// the two chroma samples of one axis that a luma position reads (clamped) and their weights (sum 4)
struct ChromaTap {
    int32_t i0, i1, w0, w1;
};

// the phases of (chroma_format_idc 1 or 2, t): py < 0 stands for "no vertical filter"
CU_HD void chroma_phase(int chroma_format, int loc, int &px, int &py) {
    if (chroma_format == 1) {
        px = loc & 1;
        py = (loc >> 1) == 0 ? 1 : (loc >> 1) == 1 ? 0 : 2;
    } else {
        px = 0;
        py = -1;
    }
}

// the taps of luma position p along an axis of n chroma samples at phase ph (ph < 0: the
// chroma sample p itself, weights (4, 0))
CU_HD ChromaTap chroma_tap(int p, int ph, int n) {
    if (ph < 0) return ChromaTap{p, p, 4, 0};
    const int u = 2 * p - ph;                  // may be -1, -2
    const int i0 = (u - (u & 3)) / 4, f = u & 3;  // floor
    const int last = n - 1;
    return ChromaTap{i0 < 0 ? 0 : i0 > last ? last : i0, i0 + 1 < 0 ? 0 : i0 + 1 > last ? last : i0 + 1, 4 - f, f};
}

// C' from the 2 x 2 neighbourhood c[row tap][column tap]
CU_HD int chroma_value(int c00, int c01, int c10, int c11, const ChromaTap &tx, const ChromaTap &ty) {
    return (ty.w0 * (tx.w0 * c00 + tx.w1 * c01) + ty.w1 * (tx.w0 * c10 + tx.w1 * c11) + 8) >> 4;
}

}  // namespace hg
