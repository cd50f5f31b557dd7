// parse_lanes.hip — the general lanes parse kernel (k_parse_lanes: the lanes
// body of parse_lanes_body.hpp with every coding tool at run time), the parse
// launch of every mode (launch_parse) and the tuning builds' counter read-out.
// The lean lanes kernel (parse_lean.hip) and the solo / spread kernels
// (parse_solo.hip) are translation units of their own, so that each gets the
// code-generation flags it is fastest with (Makefile LANES_FLAGS, LEAN_FLAGS,
// PARSE_SCHED / SOLO_SCHED; A/B in DESIGN 5.11, 5.15).
#include "parse_lanes_body.hpp"

namespace hg {

// LDS of one wave: LaneLds per used lane, LanePic per picture, progress words,
// engine tables, and the WPP context staging when rows wrap
// kTabRows + 16 engine-table words, then the 8x8 scan and its inverse (128 bytes)
constexpr size_t kLaneTablesBytes = (kTabRows + 16) * sizeof(uint64_t) + 128;
inline size_t lanes_lds_bytes(int ppw, int lane_rows, bool ring) {
    return lane_blocks_bytes(ppw * lane_rows) + sizeof(LanePic) * (size_t)ppw + 64 * sizeof(uint32_t) +
           kLaneTablesBytes + (ring ? 64 * (size_t)CTX_PAD : 0);
}

__global__ void __launch_bounds__(64) HG_PARSE_ATTR k_parse_lanes(BatchArgs a) { parse_lanes_body<Eng>(a); }

hipError_t launch_parse(const BatchArgs &a0, hipStream_t s) {
    BatchArgs a = a0;
    if (a.lane_rows < 1 || a.lane_rows > 64) return hipErrorInvalidValue;
    if (a.parse_mode == PARSE_SOLO || a.parse_mode == PARSE_SPREAD) return launch_parse_solo(a, s);
    // the dealing of parse_order fixed the pictures per wave (lanes_parse_order)
    const int ppw = a.parse_order && a.parse_group > 0 ? a.parse_group : lanes_pics_per_wave(a.lane_rows, a.n_pics);
    a.parse_group = ppw;
    const int waves = ((a.parse_order ? a.n_slots : a.n_pics) + ppw - 1) / ppw;
    if (a.lanes_lean) {
        // (prepare's choice, lanes_variant_for: never with wrapping rows)
        if (a.wpp_ring) return hipErrorInvalidValue;
        return launch_parse_lean(a, waves, lanes_lds_bytes(ppw, a.lane_rows, false), s);
    } else {
        hipLaunchKernelGGL(k_parse_lanes, dim3(waves), dim3(64), lanes_lds_bytes(ppw, a.lane_rows, a.wpp_ring != 0), s, a);
    }
    return hipGetLastError();
}

}  // namespace hg

#if defined(HG_PARSE_PROF)
// the other two parse units' counters (their device globals are their code objects' own)
extern "C" int hg_debug_counters_solo(uint64_t *out, int n);
extern "C" int hg_debug_counters_lean(uint64_t *out, int n);
#endif
// Tuning hook (include/heifgpu.h): copies out and zeroes the parse kernels'
// per-wave s_memtime counters.  Returns the number of counters written, or 0
// for the product library (counters compiled out; `make prof` has them).
extern "C" int heifgpu_debug_counters(uint64_t *out, int n) {
#if defined(HG_PARSE_PROF)
    const int r = hg::prof_read(out, n);
    if (r > 0) {  // (one of the three units' kernels ran; the others' slots are zero)
        for (int u = 0; u < 2; ++u) {
            std::vector<uint64_t> o2((size_t)r, 0);
            const int r2 = u ? hg_debug_counters_lean(o2.data(), r) : hg_debug_counters_solo(o2.data(), r);
            if (r2 < 0) return -1;
            for (int k = 0; k < r2 && k < r; ++k) out[k] += o2[(size_t)k];
        }
    }
    return r;
#else
    (void)out;
    (void)n;
    return 0;
#endif
}
