// lf_pack.hpp — the packed helpers of the loop filter's wide paths (loopfilter.hip).
//
// A "pack" is a 32-bit word of two 16-bit lanes (sample 2p in the low half,
// 2p + 1 in the high half).  On the GPU each helper is one packed VALU
// instruction (v_pk_*_i16 / u16, v_perm_b32); the host emulation compiles the
// plain C++ twin below it.  Both are the same function of their inputs, lane
// arithmetic modulo 2^16 included (tests/loopfilter/pack_driver.cpp runs the
// host twins over every 8-bit sample pair and offset under ASan + UBSan).
#pragma once
#include "wave.hpp"

namespace hg {
namespace lfp {

#if !defined(HG_HOST_EMU)
typedef short lf_s2 __attribute__((ext_vector_type(2)));
typedef unsigned short lf_u2 __attribute__((ext_vector_type(2)));
template <class V>
__device__ __forceinline__ V lf_as(uint32_t a) {
    V v;
    __builtin_memcpy(&v, &a, 4);
    return v;
}
template <class V>
__device__ __forceinline__ uint32_t lf_word(V v) {
    uint32_t a;
    __builtin_memcpy(&a, &v, 4);
    return a;
}
#endif

__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
#if defined(HG_HOST_EMU)
    return ((a + b) & 0xffffu) | ((((a >> 16) + (b >> 16)) & 0xffffu) << 16);
#else
    return lf_word(lf_as<lf_u2>(a) + lf_as<lf_u2>(b));
#endif
}
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {
#if defined(HG_HOST_EMU)
    return ((a - b) & 0xffffu) | ((((a >> 16) - (b >> 16)) & 0xffffu) << 16);
#else
    return lf_word(lf_as<lf_u2>(a) - lf_as<lf_u2>(b));
#endif
}
// signed maximum / minimum per lane
__device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b) {
#if defined(HG_HOST_EMU)
    const int al = (int16_t)(a & 0xffffu), ah = (int16_t)(a >> 16), bl = (int16_t)(b & 0xffffu), bh = (int16_t)(b >> 16);
    return (uint32_t)((al > bl ? al : bl) & 0xffff) | ((uint32_t)((ah > bh ? ah : bh) & 0xffff) << 16);
#else
    return lf_word(__builtin_elementwise_max(lf_as<lf_s2>(a), lf_as<lf_s2>(b)));
#endif
}
__device__ __forceinline__ uint32_t pk_min_i16(uint32_t a, uint32_t b) {
#if defined(HG_HOST_EMU)
    const int al = (int16_t)(a & 0xffffu), ah = (int16_t)(a >> 16), bl = (int16_t)(b & 0xffffu), bh = (int16_t)(b >> 16);
    return (uint32_t)((al < bl ? al : bl) & 0xffff) | ((uint32_t)((ah < bh ? ah : bh) & 0xffff) << 16);
#else
    return lf_word(__builtin_elementwise_min(lf_as<lf_s2>(a), lf_as<lf_s2>(b)));
#endif
}
// arithmetic / logical shift right of each lane by n (0 <= n < 16)
__device__ __forceinline__ uint32_t pk_ashr(uint32_t a, int n) {
#if defined(HG_HOST_EMU)
    const int al = (int16_t)(a & 0xffffu), ah = (int16_t)(a >> 16);
    return (uint32_t)((al >> n) & 0xffff) | ((uint32_t)((ah >> n) & 0xffff) << 16);
#else
    return lf_word(lf_as<lf_s2>(a) >> (lf_s2){(short)n, (short)n});
#endif
}
__device__ __forceinline__ uint32_t pk_lshr(uint32_t a, int n) {
#if defined(HG_HOST_EMU)
    return ((a & 0xffffu) >> n) | (((a >> 16) >> n) << 16);
#else
    return lf_word(lf_as<lf_u2>(a) >> (lf_u2){(unsigned short)n, (unsigned short)n});
#endif
}

// v_perm_b32: byte k of the result is byte sel[k] of {s0, s1} (0-3: s1, 4-7: s0);
// 8-11: the sign of byte 1 / 3 / 5 / 7 spread over the byte; 12: 0x00; above: 0xff
__device__ __forceinline__ uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
#if defined(HG_HOST_EMU)
    const uint64_t in = ((uint64_t)s0 << 32) | s1;
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = (sel >> (8 * k)) & 0xffu;
        uint32_t b;
        if (s >= 13) b = 0xffu;
        else if (s == 12) b = 0;
        else if (s >= 8) b = ((in >> (16 * (s - 8) + 15)) & 1) ? 0xffu : 0u;
        else b = (uint32_t)(in >> (8 * s)) & 0xffu;
        r |= b << (8 * k);
    }
    return r;
#else
    return __builtin_amdgcn_perm(s0, s1, sel);
#endif
}

// sign(a - b) of each lane as -1 / 0 / 1, for lanes whose difference fits 16 bits signed
__device__ __forceinline__ uint32_t pk_sign_diff(uint32_t a, uint32_t b) {
    return pk_max_i16(pk_min_i16(pk_sub(a, b), 0x00010001u), 0xffffffffu);
}

// bytes 0, 1 (half 0) or 2, 3 (half 1) of w, zero-extended, as a pack
__device__ __forceinline__ uint32_t pk_from_bytes(uint32_t w, int half) {
    return perm(0, w, half ? 0x0c030c02u : 0x0c010c00u);
}
// the low bytes of two packs as four bytes (p0's lanes first)
__device__ __forceinline__ uint32_t pk_to_bytes(uint32_t p0, uint32_t p1) { return perm(p1, p0, 0x06040200u); }

// SAO offset tables: five signed bytes in the low bytes of {hi, lo}, indexed per lane.
//   edge offset: index 2 + sign(c - a) + sign(c - b), entries {off0, off1, 0, off2, off3}
//     (8.7.3.2: edgeIdx 0, 1, 2 -> 1, 2, 0, and SaoOffsetVal[0] = 0)
//   band offset: index min(k, 4) with k = (band - position) & 31, entries {off0 .. off3, 0}
// `d1`, `d2`, `d3` are the three words of SaoParams that hold the component's off[0 .. 3]:
// off0 in d1's high half, off1 | off2 << 16 = d2, off3 in d3's low half.  Each |offset| is at
// most 31 << (bitDepth - 10) <= 124 for bitDepth <= 12 (7.4.9.3.2), so its low byte holds it.
__device__ __forceinline__ void sao_tables(uint32_t d1, uint32_t d2, uint32_t d3, bool edge, uint32_t &lo, uint32_t &hi) {
    if (edge) {
        lo = perm(d1, d2, 0x020c0006u);  // off0, off1, 0, off2
        hi = d3 & 0xffu;                 // off3
    } else {
        lo = perm(d1, d2, 0x0c020006u) | (d3 << 24);  // off0, off1, off2, off3
        hi = 0;
    }
}
// the table entries of a pack of indices (each 0 .. 7), sign-extended to the lanes
__device__ __forceinline__ uint32_t sao_lookup(uint32_t lo, uint32_t hi, uint32_t idx) {
    return pk_ashr(perm(hi, lo, (idx << 8) | 0x000c000cu), 8);
}
// Clip3(0, maxv, c + o) per lane; maxv2 = maxv in both lanes
__device__ __forceinline__ uint32_t pk_add_clip(uint32_t c, uint32_t o, uint32_t maxv2) {
    return pk_min_i16(pk_max_i16(pk_add(c, o), 0), maxv2);
}

}  // namespace lfp
}  // namespace hg
