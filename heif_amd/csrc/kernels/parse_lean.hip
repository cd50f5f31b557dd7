// parse_lean.hip — the lean lanes parse kernel (k_parse_lean: the lanes body of
// parse_lanes_body.hpp compiled for the 4:2:0 tool set without PCM,
// transform_skip, cu_transquant_bypass and in-picture slice segments, EngT) as
// a translation unit of its own, with its own code-generation flags: under the
// general unit's SLP threshold it takes 208 VGPRs instead of 176, which leaves
// room for one reconstruction wave beside two parse waves of a SIMD instead of
// two (Makefile LEAN_FLAGS).
#include "parse_lanes_body.hpp"

namespace hg {

// Its name keeps clear of "k_parse_lanes": tests/test_resource_usage.py expects
// every kernel of that name at three waves per SIMD once the v175 floor is
// compiled out, which holds for the general body's allocation only;
// tests/test_lanes_lean.py holds this kernel to two waves and no scratch
__global__ void __launch_bounds__(64) HG_PARSE_ATTR k_parse_lean(BatchArgs a) { parse_lanes_body<EngLean>(a); }
hipError_t launch_parse_lean(const BatchArgs &a, int waves, size_t lds_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_parse_lean, dim3(waves), dim3(64), lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace hg

#if defined(HG_PARSE_PROF)
extern "C" int hg_debug_counters_lean(uint64_t *out, int n) { return hg::prof_read(out, n); }
#endif
