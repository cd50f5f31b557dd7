// png.hpp — the PNG encoder, stated once for the kernels (kernels/png.hip), the host
// restatement (api/png.cpp) and, in prose, the Python model of the tests (tests/png_ref.py).
// The bytes of a file are a function of the pixels and the options only.
//
// THE FILE.  The 8-byte signature, then chunks (length, type, data, CRC-32 of type and data;
// all integers big-endian) in this order: IHDR (width, height, bit depth 8 or 16, colour type 2
// (RGB) or 6 (RGBA), compression 0, filter 0, interlace 0); sBIT, for a 16-bit format with
// B < 16 significant bits: one byte B per channel (3 or 4); at most one of sRGB (one byte 0,
// perceptual), cICP (the caller's four bytes: primaries, transfer, matrix, full-range flag) and
// iCCP ("ICC profile", a zero byte, compression method 0, then a zlib stream: the bytes 78 01,
// the profile in stored blocks of at most 65535 bytes, the last with BFINAL, and the profile's
// Adler-32); the IDAT chunks; IEND.
//
// SAMPLES.  The pixels are the surfaces the renders write: rgb8, rgba8 (bytes), rgb16, rgba16
// (16-bit words in the machine's little-endian order, holding samples of B bits, B = 8..16;
// only the low B bits of a word count).  A 16-bit sample s goes to the file as the two bytes,
// high first, of v = (s << (16 - B)) | (s >> (2 B - 16)): the sample's bits repeated below
// themselves, so full scale is 65535 and a reader recovers s = v >> (16 - B).  A raw row is
// width * bpp bytes, bpp = 3, 4, 6, 8.
//
// FILTERING.  Every row becomes one filter-type byte t and the row's bytes filtered by t over
// bytes: with x the byte, a the byte bpp before it (0 in the first bpp bytes), b the byte above
// it (0 in the first row) and c the byte bpp before b (0 where a or b is 0 by those rules):
//   0: x   1: x - a   2: x - b   3: x - ((a + b) >> 1)   4: x - paeth(a, b, c)      (mod 256)
//   paeth: p = a + b - c; pa = |p - a|, pb = |p - b|, pc = |p - c|; a if pa <= pb and pa <= pc,
//   else b if pb <= pc, else c.
// filter 0..4 forces t on every row.  filter 5 (adaptive) takes per row the t whose filtered
// bytes have the least sum of magnitudes, a byte f counting min(f, 256 - f); the lowest t wins a
// tie.  The filtered stream of a picture is its rows' 1 + width * bpp bytes on end.
//
// DEFLATE.  The zlib stream is 78 01, the blocks, and the Adler-32 of the filtered stream (a = 1
// + sum of bytes, b = sum of the running a, both mod 65521; b << 16 | a, big-endian).  The stream
// is cut every 32768 bytes, wherever rows end.  Each piece is one dynamic-Huffman block of
// literals only: bits, least significant first, BFINAL 0, BTYPE 2, HLIT 0 (257 literal/length
// codes), HDIST 0 (one distance code), HCLEN, HCLEN + 4 three-bit lengths of the code-length
// code in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (as few as hold every
// non-zero one, at least 4), the 257 literal/length code lengths and the one distance code
// length, which is 1 (the code is never used), each as its code-length code (symbols 0..15 only:
// no repeat symbols), then every byte's code, then the code of 256.  Codes are canonical (RFC 1951
// 3.2.2) and go in most significant bit first, as Huffman codes do in deflate.  After every such
// block comes an empty stored block: BFINAL (1 after the last piece only), BTYPE 0, zero bits up
// to the byte, 00 00 FF FF.
//
// CODE LENGTHS.  The same construction makes the literal code (257 symbols: the count of every
// byte of the piece and 1 for symbol 256; limit 15) and the code-length code (symbols 0..15: how
// often each length occurs among the 258 lengths sent; limit 7).  At least two symbols have a
// count in either, so every code is complete.
//   1. Huffman by two queues.  The used symbols, as leaves, in ascending order of count; nodes
//      made by merging join the end of a second queue.  Each merge takes twice the front with
//      the smaller weight of the two queues' fronts, the leaf when they weigh the same.  This
//      gives n[l], the number of leaves at depth l.
//   2. The limit L.  Leaves deeper than L count as n[L].  With K = sum n[l] 2^(L - l), while
//      K > 2^L: n[L] -= 1; for the largest l < L with n[l] > 0: n[l] -= 1, n[l + 1] += 2; K -= 1.
//   3. The used symbols in descending order of count, the lower symbol first among equal
//      counts, take the lengths in ascending order: the first n[1] get 1, the next n[2] get 2, ...
//
// IDAT.  One chunk per block: the dynamic block and its stored block.  The first chunk begins
// with 78 01; the last ends with the Adler-32.  IEND follows the last.
//
// LIMITS.  Sides 1..65535; a pitch of at least width * bpp; B = 8 for the 8-bit formats and
// 8..16 for the others; a profile of 1..2147418112 (0x7fff0000) bytes.  A code is at most 15
// bits, so a chunk is never longer than kPngChunkMax bytes: what k_png_emit's LDS holds, and a
// bound on a file's IDAT chunks and IEND by its block count alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wave.hpp"

#if defined(HG_HOST_EMU) || !defined(__HIPCC__)
#define HG_PHD inline
#else
#define HG_PHD __host__ __device__ __forceinline__
#endif

namespace hg {

constexpr int kPngMaxSide = 65535;
constexpr uint32_t kPngBlock = 32768;   // filtered bytes per deflate block
constexpr uint32_t kPngAdlerMod = 65521;
constexpr int kPngLit = 257, kPngCl = 19, kPngLitMax = 15, kPngClMax = 7;
constexpr int kPngAdaptive = 5;
// the block's header: 17 bits, 19 three-bit lengths, 258 lengths of at most 7 bits
constexpr uint32_t kPngHeadBitsMax = 17 + 3 * 19 + 258 * 7;
// a chunk at its longest: length, type, 78 01, the bits (header, 32768 codes and the code of
// 256 of at most 15 bits, the stored block's 3), 00 00 FF FF, Adler-32, CRC, IEND's 12 bytes
constexpr uint32_t kPngChunkMax = 8 + 2 + (kPngHeadBitsMax + 15 * (kPngBlock + 1) + 3 + 7) / 8 + 4 + 4 + 4 + 12;
constexpr uint8_t kPngClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// formats: the renders' (HEIFGPU_PIX_RGB8 .. RGBA16): bit 0 alpha, bit 1 sixteen bits
HG_PHD int png_channels(int fmt) { return fmt & 1 ? 4 : 3; }
HG_PHD int png_wide(int fmt) { return fmt >> 1 & 1; }
HG_PHD int png_bpp(int fmt) { return png_channels(fmt) << png_wide(fmt); }

// byte i of the raw row whose first pixel lies at `row` (SAMPLES)
HG_PHD uint32_t png_raw_byte(const uint8_t *row, uint32_t i, int wide, int bits) {
    if (!wide) return row[i];
    const uint32_t j = i & ~1u;
    const uint32_t s = (uint32_t(row[j]) | uint32_t(row[j + 1]) << 8) & ((1u << bits) - 1u);
    const uint32_t v = (s << (16 - bits)) | (s >> (2 * bits - 16));
    return i & 1 ? v & 0xffu : v >> 8;
}

HG_PHD uint32_t png_paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = int(a) + int(b) - int(c);
    const int pa = p > int(a) ? p - int(a) : int(a) - p;
    const int pb = p > int(b) ? p - int(b) : int(b) - p;
    const int pc = p > int(c) ? p - int(c) : int(c) - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
// the byte x filtered by type t (FILTERING)
HG_PHD uint32_t png_filter_byte(int t, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t pred = t == 0 ? 0u : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
    return (x - pred) & 0xffu;
}
HG_PHD uint32_t png_magnitude(uint32_t f) { return f < 128u ? f : 256u - f; }
// the least of five sums, the lowest type on a tie
HG_PHD int png_pick_filter(const uint32_t *sum) {
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (sum[t] < sum[best]) best = t;
    return best;
}

// x, a, b, c of byte i of a row (up: the row above, nullptr for the first row)
struct PngNeigh {
    uint32_t x, a, b, c;
};
HG_PHD PngNeigh png_neigh(const uint8_t *row, const uint8_t *up, uint32_t i, int bpp, int wide, int bits) {
    PngNeigh q;
    q.x = png_raw_byte(row, i, wide, bits);
    q.a = i >= uint32_t(bpp) ? png_raw_byte(row, i - uint32_t(bpp), wide, bits) : 0u;
    q.b = up ? png_raw_byte(up, i, wide, bits) : 0u;
    q.c = up && i >= uint32_t(bpp) ? png_raw_byte(up, i - uint32_t(bpp), wide, bits) : 0u;
    return q;
}

// ---- code lengths (CODE LENGTHS) ----
// Where symbol s stands when all nsym symbols are put in ascending order of count, the higher
// symbol first among equal counts (the reverse of step 3's order; unused symbols come first).
HG_PHD int png_rank(const uint32_t *cnt, int nsym, int s) {
    int r = 0;
    const uint32_t c = cnt[s];
    for (int t = 0; t < nsym; ++t) r += (cnt[t] < c || (cnt[t] == c && t > s)) ? 1 : 0;
    return r;
}
// the working memory of png_lengths and png_codes (LDS in the kernels)
struct PngHuffWork {
    uint32_t wt[2 * kPngLit];      // node weights, then node depths
    uint16_t parent[2 * kPngLit];
    uint32_t n[16];                // codes of each length
    uint32_t next[16];
};
// len[s] of every symbol from the counts and the symbols in png_rank's order
HG_PHD void png_lengths(const uint32_t *cnt, const uint16_t *order, int nsym, int limit, uint8_t *len,
                        PngHuffWork &k) {
    int nz = 0;
    while (nz < nsym && cnt[order[nz]] == 0) ++nz;
    const int m = nsym - nz;  // leaves: nodes 0..m-1, ascending; merged nodes m..2m-2
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    for (int l = 0; l < 16; ++l) k.n[l] = 0;
    if (m < 2) return;  // (never, by the contract)
    for (int i = 0; i < m; ++i) k.wt[i] = cnt[order[nz + i]];
    int leaf = 0, node = m, made = m;
    for (int j = 0; j + 1 < m; ++j) {
        uint32_t w = 0;
        for (int half = 0; half < 2; ++half) {
            const bool take_leaf = leaf < m && (node >= made || k.wt[leaf] <= k.wt[node]);
            const int pick = take_leaf ? leaf++ : node++;
            w += k.wt[pick];
            k.parent[pick] = uint16_t(made);
        }
        k.wt[made++] = w;
    }
    k.wt[2 * m - 2] = 0;
    for (int i = 2 * m - 3; i >= 0; --i) k.wt[i] = k.wt[k.parent[i]] + 1;
    for (int i = 0; i < m; ++i) k.n[k.wt[i] < uint32_t(limit) ? k.wt[i] : uint32_t(limit)] += 1;
    uint32_t total = 0;
    for (int l = 1; l <= limit; ++l) total += k.n[l] << (limit - l);
    while (total > (1u << limit)) {
        k.n[limit] -= 1;
        for (int l = limit - 1; l >= 1; --l)
            if (k.n[l]) {
                k.n[l] -= 1;
                k.n[l + 1] += 2;
                break;
            }
        total -= 1;
    }
    int at = nsym - 1;
    for (int l = 1; l <= limit; ++l)
        for (uint32_t j = 0; j < k.n[l]; ++j) len[order[at--]] = uint8_t(l);
}
// length << 16 | the code c of l bits with its bits reversed (so that it goes into the stream
// least significant bit first)
HG_PHD uint32_t png_code_entry(int l, uint32_t c) {
    uint32_t r = 0;
    for (int b = 0; b < l; ++b) r |= (c >> b & 1u) << (l - 1 - b);
    return uint32_t(l) << 16 | r;
}
// e[s] = png_code_entry of every symbol's canonical code; 0 for an unused symbol
HG_PHD void png_codes(const uint8_t *len, int nsym, int limit, uint32_t *e, PngHuffWork &k) {
    for (int l = 0; l < 16; ++l) k.n[l] = 0;
    for (int s = 0; s < nsym; ++s) k.n[len[s]] += 1;
    k.n[0] = 0;
    uint32_t code = 0;
    for (int l = 1; l <= limit; ++l) {
        code = (code + k.n[l - 1]) << 1;
        k.next[l] = code;
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        if (!l) {
            e[s] = 0;
            continue;
        }
        e[s] = png_code_entry(l, k.next[l]++);
    }
}
// The same for one symbol, for a thread per symbol: first[l] is the first code of length l (n[l]
// codes have length l, n[0] = 0), and a symbol's code is first[l] plus the number of lower
// symbols of its length.
HG_PHD void png_first_codes(const uint32_t *n, int limit, uint32_t *first) {
    uint32_t code = 0;
    for (int l = 1; l <= limit; ++l) {
        code = (code + n[l - 1]) << 1;
        first[l] = code;
    }
}
HG_PHD uint32_t png_code_of(const uint8_t *len, int s, const uint32_t *first) {
    const int l = len[s];
    if (!l) return 0;
    uint32_t rank = 0;
    for (int t = 0; t < s; ++t) rank += len[t] == l ? 1u : 0u;
    return png_code_entry(l, first[l] + rank);
}

// ---- bits into a zeroed word buffer (byte k of the stream is byte k & 3 of word k >> 2) ----
HG_PHD void png_or(uint32_t *w, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(w, v);  // neighbouring runs share a word
#else
    *w |= v;
#endif
}
struct PngSink {
    uint32_t *w;   // the next word to complete
    uint64_t acc;  // bits n.. are pending (bits below n belong to what came before)
    int n;
};
HG_PHD PngSink png_sink(uint32_t *words, uint32_t bitpos) { return PngSink{words + (bitpos >> 5), 0, int(bitpos & 31u)}; }
// len <= 24 bits of v, least significant first
HG_PHD void png_put(PngSink &s, uint32_t v, int len) {
    s.acc |= uint64_t(v) << s.n;
    s.n += len;
    if (s.n >= 32) {
        png_or(s.w++, uint32_t(s.acc));
        s.acc >>= 32;
        s.n -= 32;
    }
}
HG_PHD void png_flush(PngSink &s) {
    if (s.n && uint32_t(s.acc)) png_or(s.w, uint32_t(s.acc));
}
HG_PHD void png_put_code(PngSink &s, uint32_t e) { png_put(s, e & 0xffffu, int(e >> 16)); }
HG_PHD void png_put_byte(uint32_t *words, uint32_t pos, uint32_t b) { png_or(words + (pos >> 2), b << (8 * (pos & 3u))); }
HG_PHD void png_put_be32(uint32_t *words, uint32_t pos, uint32_t v) {
    for (int i = 0; i < 4; ++i) png_put_byte(words, pos + uint32_t(i), v >> (24 - 8 * i) & 0xffu);
}
HG_PHD uint32_t png_get_byte(const uint32_t *words, uint32_t pos) { return words[pos >> 2] >> (8 * (pos & 3u)) & 0xffu; }

// HCLEN + 4: the lengths of the code-length code that are sent
HG_PHD int png_cl_sent(const uint8_t *cllen) {
    int sent = 4;
    for (int i = 4; i < kPngCl; ++i)
        if (cllen[kPngClOrder[i]]) sent = i + 1;
    return sent;
}
// the bits of a block's header, from BFINAL to the distance code's length
HG_PHD uint32_t png_head_bits(const uint8_t *litlen, const uint8_t *cllen) {
    uint32_t bits = 17 + 3 * uint32_t(png_cl_sent(cllen)) + cllen[1];
    for (int s = 0; s < kPngLit; ++s) bits += cllen[litlen[s]];
    return bits;
}
// writes them; ecl: png_codes of cllen
HG_PHD void png_put_head(PngSink &s, const uint8_t *litlen, const uint8_t *cllen, const uint32_t *ecl) {
    const int sent = png_cl_sent(cllen);
    png_put(s, 4u, 3);  // BFINAL 0, BTYPE 2
    png_put(s, 0u, 5);
    png_put(s, 0u, 5);
    png_put(s, uint32_t(sent - 4), 4);
    for (int i = 0; i < sent; ++i) png_put(s, cllen[kPngClOrder[i]], 3);
    for (int i = 0; i < kPngLit; ++i) png_put_code(s, ecl[litlen[i]]);
    png_put_code(s, ecl[1]);
}
// the bytes of block k's IDAT chunk (and IEND after the last), from the header's bits and
// the bits of the data (every byte's code and the code of 256)
HG_PHD uint32_t png_chunk_bytes(uint32_t head_bits, uint32_t data_bits, bool first, bool last) {
    return 8 + (first ? 2 : 0) + (head_bits + data_bits + 3 + 7) / 8 + 4 + (last ? 4 : 0) + 4 + (last ? 12 : 0);
}

// ---- Adler-32 in pieces: s1 = sum d[i], s2 = sum (len - i) d[i], both mod 65521 ----
HG_PHD void png_adler_join(uint32_t &a, uint32_t &b, uint32_t s1, uint32_t s2, uint32_t len) {
    b = uint32_t((uint64_t(b) + uint64_t(len % kPngAdlerMod) * a + s2) % kPngAdlerMod);
    a = (a + s1) % kPngAdlerMod;
}

// ---- CRC-32 (polynomial 0xEDB88320, reflected), in segments ----
struct PngCrcTable {
    uint32_t t[256];
};
constexpr PngCrcTable png_crc_make() {
    PngCrcTable c{};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t v = i;
        for (int k = 0; k < 8; ++k) v = v & 1u ? 0xedb88320u ^ (v >> 1) : v >> 1;
        c.t[i] = v;
    }
    return c;
}
constexpr PngCrcTable kPngCrc = png_crc_make();
// the register after one more byte; the CRC of a message is ~ of the register run from ~0
HG_PHD uint32_t png_crc_step(uint32_t reg, uint32_t byte) { return kPngCrc.t[(reg ^ byte) & 0xffu] ^ (reg >> 8); }
// a(x) b(x) mod the polynomial, bit 31 being x^0
constexpr uint32_t png_crc_mul_c(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
HG_PHD uint32_t png_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
// The kernel takes the CRC of a chunk in kPngCrcSegs segments of kPngCrcSeg bytes that end where
// the chunk's CRC'd bytes end (zero bytes in front of a message leave a register run from 0 at
// 0; a run from ~0 is a run from 0 over the message with its first four bytes complemented).
// The register of a segment followed by k more segments is the segment's own times
// x^(8 kPngCrcSeg k): kPngCrcShift[j] = x^(8 kPngCrcSeg 2^j).
constexpr uint32_t kPngCrcSeg = 256, kPngCrcSegs = 256;
static_assert(kPngCrcSeg * kPngCrcSegs >= kPngChunkMax, "the segments cover the longest chunk");
struct PngCrcShift {
    uint32_t k[8];
};
constexpr PngCrcShift png_crc_shift_make() {
    PngCrcShift s{};
    uint32_t v = 0x00800000u;  // x^8
    for (uint32_t n = 1; n < kPngCrcSeg; n <<= 1) v = png_crc_mul_c(v, v);
    for (int j = 0; j < 8; ++j) {
        s.k[j] = v;
        v = png_crc_mul_c(v, v);
    }
    return s;
}
constexpr PngCrcShift kPngCrcShift = png_crc_shift_make();

// ---- what the kernels are given ----
struct alignas(16) PngQuad {
    uint32_t v[4];
};
// a block's record: k_png_plan writes it, k_png_offsets and k_png_emit read it
struct PngBlk {
    uint8_t litlen[260];  // 257 used
    uint8_t cllen[20];    // 19 used
    uint32_t head_bits, data_bits;
    uint32_t s1, s2;      // Adler-32 partial sums of the block's bytes
    uint32_t bytes;       // of its chunk (IEND included after the last)
    uint32_t pad;
};
struct PngPic {
    const uint8_t *px;   // the first pixel; `pitch` bytes per row, any alignment
    uint8_t *out;        // the IDAT chunks and IEND, at most `cap` bytes written
    int64_t pitch;
    uint64_t cap;
    uint64_t stream_off; // bytes into the batch's filtered streams (a multiple of 16)
    uint64_t blk_off;    // first of its blocks in the batch's block arrays
    uint64_t len;        // filtered bytes: h * (row + 1)
    uint32_t w, h;
    uint32_t row;        // raw bytes per row
    uint32_t n_blk;
};
struct PngArgs {
    const PngPic *pics;
    uint8_t *stream;   // filtered streams; 16 readable bytes behind each
    PngBlk *blk;
    uint64_t *boff;    // where each block's chunk starts in its picture's output
    uint32_t *adler;   // per picture
    uint64_t *sizes;   // per picture: IDAT chunks + IEND bytes; bit 63: larger than cap
    int n;
    int fmt, bits, filter;
};

// The batch's plan: fills what PngPic derives from w and h; returns the filtered bytes (with the
// slack behind each stream) and the blocks of the whole batch.
inline void png_plan(PngPic *pics, int n, int fmt, uint64_t &n_stream, uint64_t &n_blk, uint32_t &max_h,
                     uint32_t &max_blk) {
    n_stream = n_blk = 0;
    max_h = max_blk = 0;
    for (int i = 0; i < n; ++i) {
        PngPic &p = pics[i];
        p.row = p.w * uint32_t(png_bpp(fmt));
        p.len = uint64_t(p.h) * (uint64_t(p.row) + 1);
        p.n_blk = uint32_t((p.len + kPngBlock - 1) / kPngBlock);
        p.stream_off = n_stream;
        p.blk_off = n_blk;
        n_stream += (p.len + 16 + 15) / 16 * 16;
        n_blk += p.n_blk;
        max_h = p.h > max_h ? p.h : max_h;
        max_blk = p.n_blk > max_blk ? p.n_blk : max_blk;
    }
}
#if defined(HG_HOST_EMU)
void emu_png_encode(const PngArgs &a, uint32_t max_h, uint32_t max_blk);
#elif defined(__HIPCC__)
// four launches for the whole batch: filter, plan, offsets, emit
hipError_t launch_png_encode(const PngArgs &a, uint32_t max_h, uint32_t max_blk, hipStream_t s);
#endif

}  // namespace hg
