// png.hip — PNG encoding of a batch of RGB(A) 8- and 16-bit surfaces (heifgpu_png_encode_batch):
// the IDAT chunks and IEND of every picture, in four launches whatever the batch holds.  The
// file's layout, the filters and the code construction are stated in png.hpp.
//
//   1. k_png_filter   one wave per row: the five filters' sums of magnitudes over the row
//                     (adaptive), a wave reduction, the filter byte and the chosen filter's bytes
//                     to the picture's filtered stream.  16-bit samples are widened and
//                     byte-swapped as they are read.
//   2. k_png_plan     one work-group per 32768-byte block: a histogram in LDS (one per wave:
//                     filtered photographs pile onto a few values near 0 and 255), the Adler-32
//                     partial sums, then the block's two sets of code lengths (the symbols ranked
//                     by all threads, the two-queue merge by one), and from the histogram alone the
//                     exact size of its chunk.
//   3. k_png_offsets  one work-group per picture: the exclusive scan of its chunks' sizes, the
//                     Adler-32 joined in order, and sizes[i] (bit 63 when it exceeds the capacity).
//   4. k_png_emit     one work-group per block: 256 runs of 128 bytes; the runs' bit lengths, a
//                     scan, every run's codes OR-ed into the zeroed chunk in LDS at its final bit,
//                     the CRC-32 of the chunk in 256 segments joined by a tree, and the chunk out
//                     in 16-byte stores at its final offset, nothing at or past the capacity.
// The scratch is the filtered stream and 312 bytes per block.  k_png_emit holds the longest
// chunk the contract allows (15 bits a byte) in LDS, which is what limits its occupancy.
#include "png.hpp"

#if defined(HG_HOST_EMU)
#include <atomic>
#endif

namespace hg {

namespace {

constexpr int kSubHist = 4;                        // histograms per work-group
constexpr uint32_t kRuns = 256, kRunBytes = kPngBlock / kRuns;
constexpr uint32_t kOutQuads = (15 + kPngChunkMax + 15) / 16;

__device__ __forceinline__ void lds_inc(uint32_t *p) {
#if defined(HG_HOST_EMU)
    *p += 1;
#else
    atomicAdd(p, 1u);
#endif
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#if !defined(HG_HOST_EMU)
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
#endif
    return v;
}
__device__ __forceinline__ uint32_t quad_byte(const PngQuad &q, uint32_t k) { return q.v[k >> 2] >> (8 * (k & 3u)) & 0xffu; }

}  // namespace

__global__ void __launch_bounds__(256) k_png_filter(PngArgs a) {
    const PngPic &p = a.pics[blockIdx.y];
    const uint32_t lane = threadIdx.x % kWave, waves = blockDim.x / kWave;
    const uint32_t y = blockIdx.x * waves + threadIdx.x / kWave;
    if (y >= p.h) return;  // (uniform in the wave, and no barrier follows)
    const int bpp = png_bpp(a.fmt), wide = png_wide(a.fmt), bits = a.bits;
    const uint8_t *row = p.px + int64_t(y) * p.pitch;
    const uint8_t *up = y ? row - p.pitch : nullptr;
    int t = a.filter;
    if (t == kPngAdaptive) {
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t i = lane; i < p.row; i += kWave) {
            const PngNeigh q = png_neigh(row, up, i, bpp, wide, bits);
#pragma unroll
            for (int f = 0; f < 5; ++f) sum[f] += png_magnitude(png_filter_byte(f, q.x, q.a, q.b, q.c));
        }
#pragma unroll
        for (int f = 0; f < 5; ++f) sum[f] = wave_sum(sum[f]);
        t = png_pick_filter(sum);
    }
    uint8_t *dst = a.stream + p.stream_off + uint64_t(y) * (uint64_t(p.row) + 1);
    if (lane == 0) dst[0] = uint8_t(t);
    for (uint32_t i = lane; i < p.row; i += kWave) {
        const PngNeigh q = png_neigh(row, up, i, bpp, wide, bits);
        dst[1 + i] = uint8_t(png_filter_byte(t, q.x, q.a, q.b, q.c));
    }
}

__global__ void __launch_bounds__(256) k_png_plan(PngArgs a) {
    HG_BLOCK_SHARED uint32_t hist[kSubHist * 256];
    HG_BLOCK_SHARED uint32_t cnt[kPngLit], clcnt[kPngCl];
    HG_BLOCK_SHARED uint16_t order[kPngLit], clorder[kPngCl];
    HG_BLOCK_SHARED uint8_t litlen[260], cllen[20];
    HG_BLOCK_SHARED PngHuffWork work;
    HG_BLOCK_SHARED uint32_t part1[256];
    HG_BLOCK_SHARED uint64_t part2[256];
    const PngPic &p = a.pics[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= p.n_blk) return;  // (uniform: the whole work-group leaves)
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint64_t at = uint64_t(b) * kPngBlock;
    const uint32_t blen = uint32_t(min(uint64_t(kPngBlock), p.len - at));
    PngBlk &r = a.blk[p.blk_off + b];

    for (uint32_t i = tid; i < kSubHist * 256; i += nthr) hist[i] = 0;
    __syncthreads();
    // the block's bytes in 16-byte loads (the stream has 16 readable bytes behind its last)
    const PngQuad *src = reinterpret_cast<const PngQuad *>(a.stream + p.stream_off + at);
    uint32_t *my = hist + (tid / kWave) % kSubHist * 256;
    uint32_t s1 = 0;
    uint64_t s2 = 0;
    for (uint32_t q = tid; q < (blen + 15) / 16; q += nthr) {
        const PngQuad v = src[q];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t i = 16 * q + k, d = quad_byte(v, k);
            if (i < blen) {
                lds_inc(my + d);
                s1 += d;
                s2 += uint64_t(blen - i) * d;
            }
        }
    }
    part1[tid] = s1;
    part2[tid] = s2;
    __syncthreads();
    for (uint32_t s = tid; s < 256; s += nthr) {
        uint32_t c = 0;
        for (int h = 0; h < kSubHist; ++h) c += hist[h * 256 + s];
        cnt[s] = c;
    }
    if (tid == 0) {
        cnt[256] = 1;
        uint64_t t1 = 0, t2 = 0;
        for (uint32_t t = 0; t < nthr; ++t) t1 += part1[t], t2 += part2[t] % kPngAdlerMod;
        r.s1 = uint32_t(t1 % kPngAdlerMod);
        r.s2 = uint32_t(t2 % kPngAdlerMod);
    }
    __syncthreads();
    for (uint32_t s = tid; s < uint32_t(kPngLit); s += nthr) order[png_rank(cnt, kPngLit, int(s))] = uint16_t(s);
    __syncthreads();
    if (tid == 0) {
        png_lengths(cnt, order, kPngLit, kPngLitMax, litlen, work);
        for (int s = 0; s < kPngCl; ++s) clcnt[s] = 0;
        for (int s = 0; s < kPngLit; ++s) clcnt[litlen[s]] += 1;
        clcnt[1] += 1;  // the distance code
        for (int s = 0; s < kPngCl; ++s) clorder[png_rank(clcnt, kPngCl, s)] = uint16_t(s);
        png_lengths(clcnt, clorder, kPngCl, kPngClMax, cllen, work);
        uint32_t data = 0;
        for (int s = 0; s < kPngLit; ++s) data += cnt[s] * litlen[s];
        r.head_bits = png_head_bits(litlen, cllen);
        r.data_bits = data;
        r.bytes = png_chunk_bytes(r.head_bits, data, b == 0, b + 1 == p.n_blk);
        r.pad = 0;
    }
    __syncthreads();
    for (uint32_t s = tid; s < 260; s += nthr) r.litlen[s] = s < uint32_t(kPngLit) ? litlen[s] : 0;
    for (uint32_t s = tid; s < 20; s += nthr) r.cllen[s] = s < uint32_t(kPngCl) ? cllen[s] : 0;
}

__global__ void __launch_bounds__(256) k_png_offsets(PngArgs a) {
    HG_BLOCK_SHARED uint64_t part[256];
    HG_BLOCK_SHARED uint32_t ps1[256], ps2[256], plen[256];
    const PngPic &p = a.pics[blockIdx.x];
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t seg = (p.n_blk + nthr - 1) / nthr;  // consecutive blocks per thread
    const uint32_t i0 = uint32_t(min(tid * uint64_t(seg), uint64_t(p.n_blk)));
    const uint32_t i1 = uint32_t(min(uint64_t(i0) + seg, uint64_t(p.n_blk)));
    uint64_t sum = 0;
    uint32_t s1 = 0, s2 = 0, len = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const PngBlk &r = a.blk[p.blk_off + i];
        const uint32_t blen = uint32_t(min(uint64_t(kPngBlock), p.len - uint64_t(i) * kPngBlock));
        sum += r.bytes;
        png_adler_join(s1, s2, r.s1, r.s2, blen);
        len = (len + blen) % kPngAdlerMod;
    }
    part[tid] = sum;
    ps1[tid] = s1, ps2[tid] = s2, plen[tid] = len;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        uint32_t ad_a = 1, ad_b = 0;
        for (uint32_t t = 0; t < nthr; ++t) {
            const uint64_t v = part[t];
            part[t] = run;
            run += v;
            png_adler_join(ad_a, ad_b, ps1[t], ps2[t], plen[t]);
        }
        a.adler[blockIdx.x] = ad_b << 16 | ad_a;
        a.sizes[blockIdx.x] = run | (run > p.cap ? uint64_t(1) << 63 : 0);
    }
    __syncthreads();
    uint64_t off = part[tid];
    for (uint32_t i = i0; i < i1; ++i) {
        a.boff[p.blk_off + i] = off;
        off += a.blk[p.blk_off + i].bytes;
    }
}

__global__ void __launch_bounds__(256) k_png_emit(PngArgs a) {
    HG_BLOCK_SHARED PngQuad outq[kOutQuads];
    HG_BLOCK_SHARED uint32_t e[kPngLit], ecl[kPngCl];
    HG_BLOCK_SHARED uint32_t pre[kRuns + 1], crc[kPngCrcSegs];
    HG_BLOCK_SHARED uint8_t litlen[260], cllen[20];
    HG_BLOCK_SHARED PngHuffWork work;
    HG_BLOCK_SHARED uint32_t lit_n[16], lit_first[16];
    HG_BLOCK_SHARED uint32_t crc_end;
    const PngPic &p = a.pics[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= p.n_blk) return;  // (uniform: the whole work-group leaves)
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const PngBlk &r = a.blk[p.blk_off + b];
    const bool first = b == 0, last = b + 1 == p.n_blk;
    const uint64_t at = uint64_t(b) * kPngBlock;
    const uint32_t blen = uint32_t(min(uint64_t(kPngBlock), p.len - at));
    const uint64_t off = a.boff[p.blk_off + b];
    const uintptr_t dst = reinterpret_cast<uintptr_t>(p.out) + off;
    const uint32_t mis = uint32_t(dst & 15u);  // the chunk lies in LDS as it will lie in its 16-byte lines
    const uint32_t total = r.bytes, nq = (mis + total + 15) / 16;
    uint32_t *const w = reinterpret_cast<uint32_t *>(outq);
    const PngQuad *src = reinterpret_cast<const PngQuad *>(a.stream + p.stream_off + at);

    for (uint32_t i = tid; i < 4 * nq; i += nthr) w[i] = 0;
    for (uint32_t s = tid; s < 260; s += nthr) litlen[s] = r.litlen[s];
    for (uint32_t s = tid; s < 20; s += nthr) cllen[s] = r.cllen[s];
    for (uint32_t l = tid; l < 16; l += nthr) lit_n[l] = 0;
    __syncthreads();
    // the literal code's table by a thread per symbol, the code-length code's by one
    for (uint32_t s = tid; s < uint32_t(kPngLit); s += nthr)
        if (litlen[s]) lds_inc(lit_n + litlen[s]);
    __syncthreads();
    if (tid == 0) {
        png_first_codes(lit_n, kPngLitMax, lit_first);
        png_codes(cllen, kPngCl, kPngClMax, ecl, work);
    }
    __syncthreads();
    for (uint32_t s = tid; s < uint32_t(kPngLit); s += nthr) e[s] = png_code_of(litlen, int(s), lit_first);
    __syncthreads();

    // the chunk's first bytes and the block's header by one thread; every run's bits by all
    const uint32_t bit0 = 8 * (mis + 8 + (first ? 2u : 0u));
    if (tid == 0) {
        png_put_be32(w, mis, total - 12 - (last ? 12u : 0u));
        png_put_be32(w, mis + 4, 0x49444154u);  // "IDAT"
        if (first) png_put_byte(w, mis + 8, 0x78), png_put_byte(w, mis + 9, 0x01);
        PngSink s = png_sink(w, bit0);
        png_put_head(s, litlen, cllen, ecl);
        png_flush(s);
    }
    for (uint32_t run = tid; run < kRuns; run += nthr) {
        uint32_t bits = 0;
        for (uint32_t j = 0; j < kRunBytes / 16 && run * kRunBytes + 16 * j < blen; ++j) {
            const PngQuad v = src[run * (kRunBytes / 16) + j];
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k)
                if (run * kRunBytes + 16 * j + k < blen) bits += e[quad_byte(v, k)] >> 16;
        }
        pre[run] = bits;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t pos = bit0 + r.head_bits;
        for (uint32_t run = 0; run < kRuns; ++run) {
            const uint32_t v = pre[run];
            pre[run] = pos;
            pos += v;
        }
        pre[kRuns] = pos;
    }
    __syncthreads();
    for (uint32_t run = tid; run < kRuns; run += nthr) {
        if (run * kRunBytes >= blen) continue;
        PngSink s = png_sink(w, pre[run]);
        for (uint32_t j = 0; j < kRunBytes / 16 && run * kRunBytes + 16 * j < blen; ++j) {
            const PngQuad v = src[run * (kRunBytes / 16) + j];
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k)
                if (run * kRunBytes + 16 * j + k < blen) png_put_code(s, e[quad_byte(v, k)]);
        }
        png_flush(s);
    }
    if (tid == 0) {
        // the code of 256, the stored block (its zero bits and 00 00 are there already), Adler-32
        PngSink s = png_sink(w, pre[kRuns]);
        png_put_code(s, e[256]);
        png_put(s, last ? 1u : 0u, 3);
        png_flush(s);
        uint32_t pos = (pre[kRuns] + (e[256] >> 16) + 3 + 7) / 8;
        png_put_byte(w, pos + 2, 0xff), png_put_byte(w, pos + 3, 0xff);
        pos += 4;
        if (last) png_put_be32(w, pos, a.adler[blockIdx.y]), pos += 4;
        crc_end = pos;
    }
    __syncthreads();

    // CRC-32 of the type and the data: segments that end at crc_end, then the tree
    const int c0 = int(mis) + 4, c1 = int(crc_end);
    for (uint32_t t = tid; t < kPngCrcSegs; t += nthr) {
        const int s1 = c1 - int((kPngCrcSegs - 1 - t) * kPngCrcSeg), s0 = max(s1 - int(kPngCrcSeg), c0);
        uint32_t reg = 0;
        for (int i = s0; i < s1; ++i) reg = png_crc_step(reg, png_get_byte(w, uint32_t(i)) ^ (i - c0 < 4 ? 0xffu : 0u));
        crc[t] = reg;
    }
    __syncthreads();
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t s = 1u << j;
        for (uint32_t i = tid; i < (kPngCrcSegs / 2) >> j; i += nthr) {
            const uint32_t l = i * 2 * s + s - 1;
            crc[l + s] ^= png_crc_mul(kPngCrcShift.k[j], crc[l]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        png_put_be32(w, crc_end, ~crc[kPngCrcSegs - 1]);
        if (last) {
            png_put_be32(w, crc_end + 8, 0x49454e44u);   // an empty "IEND"
            png_put_be32(w, crc_end + 12, 0xae426082u);  // and its CRC
        }
    }
    __syncthreads();

    // whole 16-byte lines inside the chunk and below the capacity as they are, the rest by bytes
    const uint32_t room = off >= p.cap ? 0u : uint32_t(min(uint64_t(total), p.cap - off));
    const uintptr_t base = dst - mis;
    for (uint32_t q = tid; q < nq; q += nthr) {
        const uint32_t lo = 16 * q;
        if (lo >= mis && lo + 16 <= mis + room) {
            *reinterpret_cast<PngQuad *>(base + lo) = outq[q];
        } else {
            for (uint32_t k = 0; k < 16; ++k)
                if (lo + k >= mis && lo + k < mis + room) *reinterpret_cast<uint8_t *>(base + lo + k) = uint8_t(png_get_byte(w, lo + k));
        }
    }
}

#if defined(HG_HOST_EMU)
namespace {
// one block at a time, one host thread of one lane per block (blockDim.x == 1)
template <class K>
void png_emu_launch(K kernel, unsigned gx, unsigned gy, const PngArgs &a) {
    std::atomic<int> cnt{0}, gen{0};
    for (unsigned by = 0; by < gy; ++by)
        for (unsigned bx = 0; bx < gx; ++bx) {
            g_emu.bidx = {bx, by, 0};
            g_emu.tidx = {0, 0, 0};
            g_emu.bdim = {1, 1, 1};
            g_emu.gdim = {gx, gy, 1};
            g_emu.bar_count = &cnt;
            g_emu.bar_gen = &gen;
            g_emu.bar_n = 1;
            g_emu.smem = nullptr;
            kernel(a);
        }
}
}  // namespace

void emu_png_encode(const PngArgs &a, uint32_t max_h, uint32_t max_blk) {
    if (a.n <= 0) return;
    png_emu_launch(k_png_filter, max_h, unsigned(a.n), a);  // (a wave is one lane here: a row per block)
    png_emu_launch(k_png_plan, max_blk, unsigned(a.n), a);
    png_emu_launch(k_png_offsets, unsigned(a.n), 1, a);
    png_emu_launch(k_png_emit, max_blk, unsigned(a.n), a);
}
#else
hipError_t launch_png_encode(const PngArgs &a, uint32_t max_h, uint32_t max_blk, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const unsigned rows = 256 / kWave;  // rows per work-group of k_png_filter
    hipLaunchKernelGGL(k_png_filter, dim3((max_h + rows - 1) / rows, unsigned(a.n)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_png_plan, dim3(max_blk, unsigned(a.n)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_png_offsets, dim3(unsigned(a.n)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_png_emit, dim3(max_blk, unsigned(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}
#endif

}  // namespace hg
