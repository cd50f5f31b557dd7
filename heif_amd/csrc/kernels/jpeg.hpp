// jpeg.hpp — the arithmetic of the baseline JPEG encoder, stated once for the kernels
// (kernels/jpeg.hip), the host restatement (host/jpeg.cpp) and, in prose, the numpy model
// of the tests (tests/jpeg_ref.py).  Everything here is integer arithmetic.
//
// THE FILE.  Baseline sequential DCT (SOF0), JFIF 1.01, three components Y Cb Cr of 8 bits,
// ids 1 2 3, Y sampled 1x1 ("4:4:4", 8 x 8 MCUs) or 2x2 ("4:2:0", 16 x 16 MCUs), one
// interleaved scan.  Segments in order: SOI, APP0, APP2 x k (an ICC profile in chunks of at
// most 65519 bytes behind "ICC_PROFILE\0", chunk number from 1, chunk count), DQT table 0 (luma),
// DQT table 1 (chroma), SOF0, DHT DC 0, DHT AC 0, DHT DC 1, DHT AC 1 (K.3: Y uses tables 0, Cb
// and Cr tables 1), DRI, SOS, then the scan and EOI.
//
// COLOUR.  JFIF BT.601 full range in 16.16 fixed point (no clipping is needed: the three
// results lie in 0..255 for every R, G, B in 0..255):
//   Y  = ( 19595 R + 38470 G +  7471 B +   32768) >> 16
//   Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16
//   Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
// The picture is extended to a whole number of MCUs by repeating its last column and its last
// row, at full resolution, before anything else.  4:2:0 chroma is (a + b + c + d + 2) >> 2 of the
// four Cb (Cr) values of each 2 x 2 cell of the extended picture.
//
// FORWARD DCT.  T[u][x] = rint(16384 c(u) cos((2x + 1) u pi / 16)), c(0) = sqrt(1/8), c(u) = 1/2
// (kT below: the orthonormal 8-point DCT-II in Q14).  With p the 8 x 8 samples minus 128:
//   rows:     r[y][u] = (sum_x T[u][x] p[y][x] + 128) >> 8        (arithmetic shift; Q6)
//   columns:  c[v][u] =  sum_y T[v][y] r[y][u]                    (Q20)
// c / 2^20 is the coefficient of the orthonormal 8 x 8 DCT.  No 32-bit accumulator overflows:
// the largest sum of |T[u][.]| over a row of T is 46344 (rows 0 and 4), |p| <= 128, so
// |sum_x| <= 46344 * 128 = 5 932 032 and |r| <= 23173; then |c| <= 46344 * 23173 =
// 1 073 929 512 < 2^31 - 1 = 2 147 483 647.
// Measured accuracy (tests/test_jpeg.py, 2000 random blocks, the constant and checkerboard
// blocks and the 64 basis functions at full amplitude, against scipy.fft.dctn in float64):
// max |c / 2^20 - ideal| = 0.1351 (the bound is 1/4, which keeps a coefficient quantised with
// t = 1 within 1 of the ideal one).
//
// QUANTISATION.  Tables: Annex K.1 / K.2 scaled as IJG does: s = 5000 / Q (integer division)
// for Q < 50, else 200 - 2 Q; t = clamp((base s + 50) / 100, 1, 255).  The quantised value is
// c / (t 2^20) rounded half away from zero in one division:
//   q = sign(c) ((|c| + t 2^19) / (t 2^20))         |c| + t 2^19 <= 1 073 929 512 + 255 * 524 288
//                                                    = 1 207 622 952 < 2^31 - 1
// |q| <= 1024 for DC (exactly -1024 for a black block at t = 1) and <= 1023 for AC, so a DC
// difference has at most 11 bits and an AC value at most 10, which is what K.3's tables code.
// Coefficients are stored in zigzag order (kZigzag[k]: the natural index of scan position k).
//
// ENTROPY CODING.  Huffman, the four tables of K.3 (kBits* / kVals*: the DHT contents; the
// codes are derived from them as in C.2).  DC: the difference to the previous block of the
// same component (0 at the start of a restart interval), category n = bit length of |d|, code
// of n then n bits (d, or d - 1 for d < 0, low n bits).  AC: for each non-zero value its
// zero run r; while r > 15, code 0xF0 and r -= 16; then the code of (r << 4 | n) and n bits as for
// DC; 0x00 (EOB) when the block ends in zeros.  Bits fill bytes from the top; a byte 0xFF is
// followed by 0x00.  A restart interval is `ri` MCUs (restart_mcus, or one MCU row for 0); at
// its end the last byte is padded with 1-bits (and stuffed like any other) and RSTm, m =
// interval number mod 8, follows, except after the last interval, where EOI follows.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.hpp"

#if defined(HG_HOST_EMU) || !defined(__HIPCC__)
#define HG_JHD inline
#else
#define HG_JHD __host__ __device__ __forceinline__
#endif

namespace hg {

constexpr int kJpegMaxSide = 65535;
enum : int { JPEG_444 = 0, JPEG_420 = 1 };

// Annex K.1 and K.2, natural order
constexpr uint8_t kJpegBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
     81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T[u][x] (see FORWARD DCT above)
constexpr int32_t kT[8][8] = {{5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793},
                              {8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035},
                              {7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568},
                              {6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811},
                              {5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793},
                              {4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551},
                              {3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135},
                              {1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598}};

// K.3: BITS (codes of each length 1..16) and HUFFVAL of the four tables
constexpr uint8_t kBitsDc[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kValsDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};  // both DC tables
constexpr uint8_t kBitsAc[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kValsAc[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// The encoder's view of a Huffman table (C.2): e[symbol] = length << 16 | code; 0: no code.
struct JpegHuff {
    uint32_t e[256];
};
constexpr JpegHuff jpeg_huff_make(const uint8_t *bits, const uint8_t *vals) {
    JpegHuff h{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) h.e[vals[k++]] = uint32_t(len) << 16 | code++;
        code <<= 1;
    }
    return h;
}
constexpr JpegHuff kHuffDc[2] = {jpeg_huff_make(kBitsDc[0], kValsDc), jpeg_huff_make(kBitsDc[1], kValsDc)};
constexpr JpegHuff kHuffAc[2] = {jpeg_huff_make(kBitsAc[0], kValsAc[0]), jpeg_huff_make(kBitsAc[1], kValsAc[1])};

// t of QUANTISATION for one base value; quality in 1..100
HG_JHD uint8_t jpeg_quant_scale(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int t = (base * s + 50) / 100;
    return uint8_t(t < 1 ? 1 : t > 255 ? 255 : t);
}

HG_JHD int jpeg_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
HG_JHD int jpeg_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16; }
HG_JHD int jpeg_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16; }
// component c (0 Y, 1 Cb, 2 Cr) of the pixel at p
HG_JHD int jpeg_ycc(const uint8_t *p, int c) {
    return c == 0 ? jpeg_y(p[0], p[1], p[2]) : c == 1 ? jpeg_cb(p[0], p[1], p[2]) : jpeg_cr(p[0], p[1], p[2]);
}

// One 8-point pass over v[0], v[stride], ..: out[u] = (sum_x T[u][x] v[x] + round) >> shift, in place.
HG_JHD void jpeg_dct8(int32_t *v, int stride, int32_t round, int shift) {
    int32_t in[8], out[8];
    for (int x = 0; x < 8; ++x) in[x] = v[x * stride];
    for (int u = 0; u < 8; ++u) {
        int32_t s = round;
        for (int x = 0; x < 8; ++x) s += kT[u][x] * in[x];
        out[u] = s >> shift;
    }
    for (int u = 0; u < 8; ++u) v[u * stride] = out[u];
}
HG_JHD void jpeg_dct_row(int32_t *row) { jpeg_dct8(row, 1, 128, 8); }
HG_JHD void jpeg_dct_col(int32_t *col, int stride) { jpeg_dct8(col, stride, 0, 0); }

// q of QUANTISATION
HG_JHD int32_t jpeg_quantise(int32_t c, int32_t t) {
    const int32_t a = c < 0 ? -c : c;
    const int32_t q = (a + (t << 19)) / (t << 20);
    return c < 0 ? -q : q;
}

// ---- entropy coding of one restart interval ----
// The coded bytes go to out[pos++] while pos < cap (kWrite), or are only counted.
template <bool kWrite>
struct JpegSink {
    uint8_t *out;
    uint64_t pos, cap;
    uint32_t acc;  // the low nbits bits are pending
    int nbits;     // < 8 between calls
};
template <bool kWrite>
HG_JHD void jpeg_byte(JpegSink<kWrite> &s, uint32_t b) {
    if (kWrite && s.pos < s.cap) s.out[s.pos] = uint8_t(b);
    ++s.pos;
}
// len <= 16 bits of code (7 + 16 pending bits fit the 32-bit accumulator)
template <bool kWrite>
HG_JHD void jpeg_put(JpegSink<kWrite> &s, uint32_t code, int len) {
    s.acc = (s.acc << len) | code;
    s.nbits += len;
    while (s.nbits >= 8) {
        const uint32_t b = (s.acc >> (s.nbits - 8)) & 0xffu;
        jpeg_byte(s, b);
        if (b == 0xffu) jpeg_byte(s, 0);
        s.nbits -= 8;
    }
    s.acc &= 0xffu;  // (only the pending bits are kept)
}
HG_JHD int jpeg_bitlen(uint32_t a) { return a ? 32 - __builtin_clz(a) : 0; }
// the Huffman code of (run << 4 | category of v), then the category's bits of v
template <bool kWrite>
HG_JHD void jpeg_put_value(JpegSink<kWrite> &s, const JpegHuff &h, int run, int v) {
    const int n = jpeg_bitlen(uint32_t(v < 0 ? -v : v));
    const uint32_t e = h.e[run << 4 | n];
    jpeg_put(s, e & 0xffffu, int(e >> 16));
    if (n) jpeg_put(s, uint32_t(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
}
// one block of 64 zigzag coefficients; tab: 0 luma, 1 chroma tables
template <bool kWrite>
HG_JHD void jpeg_put_block(JpegSink<kWrite> &s, const int16_t *c, int &pred, int tab) {
    const int dc = c[0];
    jpeg_put_value(s, kHuffDc[tab], 0, dc - pred);
    pred = dc;
    const JpegHuff &ac = kHuffAc[tab];
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) jpeg_put(s, ac.e[0xf0] & 0xffffu, int(ac.e[0xf0] >> 16));
        jpeg_put_value(s, ac, run, v);
        run = 0;
    }
    if (run) jpeg_put(s, ac.e[0] & 0xffffu, int(ac.e[0] >> 16));
}
// MCUs [m0, m1) of a picture's coefficients (blocks per MCU: 6 for 4:2:0, Y Y Y Y Cb Cr; 3 for
// 4:4:4), padded to a byte, then the two bytes of `marker` (RSTm or EOI)
template <bool kWrite>
HG_JHD void jpeg_put_interval(JpegSink<kWrite> &s, const int16_t *coef, uint32_t m0, uint32_t m1, int sub,
                              uint32_t marker) {
    const int bpm = sub == JPEG_420 ? 6 : 3, ny = bpm - 2;
    int pred[3] = {0, 0, 0};
    for (uint32_t m = m0; m < m1; ++m) {
        const int16_t *c = coef + size_t(m) * bpm * 64;
        for (int j = 0; j < bpm; ++j) {
            const int comp = j < ny ? 0 : j - ny + 1;
            jpeg_put_block(s, c + j * 64, pred[comp], comp ? 1 : 0);
        }
    }
    if (s.nbits) jpeg_put(s, (1u << (8 - s.nbits)) - 1u, 8 - s.nbits);
    jpeg_byte(s, 0xff);
    jpeg_byte(s, marker);
}

// ---- what the kernels are given ----
// One picture of a batch.  The coefficient kernel takes groups of kJpegGroupPx columns of one MCU
// row (48 blocks: 8 MCUs of 4:2:0, 16 of 4:4:4); the entropy kernels take restart intervals.
constexpr int kJpegGroupPx = 128, kJpegGroupBlocks = 48;
struct JpegPic {
    const uint8_t *rgb;  // R G B interleaved, `pitch` bytes per row, any alignment
    uint8_t *out;        // the scan and EOI, at most `cap` bytes written
    int64_t pitch;
    uint64_t cap;
    uint64_t coef_off;   // int16 units into the batch's coefficients
    uint64_t int_off;    // first of its intervals in the batch's interval arrays
    uint32_t w, h;
    uint32_t mcus_x, mcus_y, groups_x;
    uint32_t ri;         // MCUs per restart interval (> 0)
    uint32_t n_int;
    uint32_t pad;
};
struct JpegArgs {
    const JpegPic *pics;
    int16_t *coef;      // zigzag coefficients, a picture's MCUs in scan order
    uint32_t *ilen;     // bytes of each interval, its marker included
    uint64_t *ioff;     // where each interval starts in its picture's scan
    uint64_t *sizes;    // per picture: scan + EOI bytes; bit 63: larger than cap
    int n;
    int sub;            // JPEG_444 or JPEG_420
    uint8_t qt[2][64];  // luma, chroma; natural order
};

// The batch's plan: fills what JpegPic derives from w, h, sub and restart_mcus (0: one MCU row);
// returns the coefficient count and the interval count of the whole batch.
inline void jpeg_plan(JpegPic *pics, int n, int sub, uint32_t restart_mcus, uint64_t &n_coef, uint64_t &n_int,
                      uint32_t &max_groups, uint32_t &max_int) {
    const uint32_t mcu = sub == JPEG_420 ? 16 : 8, bpm = sub == JPEG_420 ? 6 : 3;
    n_coef = n_int = 0;
    max_groups = max_int = 0;
    for (int i = 0; i < n; ++i) {
        JpegPic &p = pics[i];
        p.mcus_x = (p.w + mcu - 1) / mcu;
        p.mcus_y = (p.h + mcu - 1) / mcu;
        p.groups_x = (p.mcus_x * mcu + kJpegGroupPx - 1) / kJpegGroupPx;
        p.ri = restart_mcus ? restart_mcus : p.mcus_x;
        const uint64_t mcus = uint64_t(p.mcus_x) * p.mcus_y;
        p.n_int = uint32_t((mcus + p.ri - 1) / p.ri);
        p.coef_off = n_coef;
        p.int_off = n_int;
        p.pad = 0;
        n_coef += mcus * bpm * 64;
        n_int += p.n_int;
        max_groups = p.groups_x * p.mcus_y > max_groups ? p.groups_x * p.mcus_y : max_groups;
        max_int = p.n_int > max_int ? p.n_int : max_int;
    }
}

#if defined(HG_HOST_EMU)
void emu_jpeg_encode(const JpegArgs &a, uint32_t max_groups, uint32_t max_int);
#elif defined(__HIPCC__)
// four launches for the whole batch: coefficients, interval sizes, offsets and sizes, bytes
hipError_t launch_jpeg_encode(const JpegArgs &a, uint32_t max_groups, uint32_t max_int, hipStream_t s);
#endif

}  // namespace hg
