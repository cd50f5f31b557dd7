// jpeg.hip — baseline JPEG encoding of a batch of RGB8 surfaces (heifgpu_jpeg_encode_batch):
// the scan and EOI of every picture, in four launches whatever the batch holds.  The
// arithmetic and the file's layout are stated in jpeg.hpp.
//
//   1. k_jpeg_coef      one work-group per 128 columns of one MCU row (48 blocks): the rows'
//                       RGB through dword loads into LDS, colour conversion and chroma
//                       subsampling with the edge replicated, both DCT passes in LDS,
//                       quantisation, int16 coefficients in zigzag and scan order.
//   2. k_jpeg_entropy<false>  one lane per restart interval: the exact coded size (Huffman
//                       codes, stuffed bytes, padding, marker) with nothing stored.
//   3. k_jpeg_offsets   one work-group per picture: the exclusive scan of its intervals'
//                       sizes, and sizes[i] (bit 63 when it exceeds the capacity).
//   4. k_jpeg_entropy<true>   the same walk again, each interval writing its bytes at its
//                       final offset, none at or past the picture's capacity.
// Coding twice costs the entropy walk's time a second time and no memory: the only scratch is
// the coefficients (2 bytes each, 1.5 x (4:2:0) or 3 x (4:4:4) the padded pixel count) and 12
// bytes per interval.  Coding once into per-interval scratch would need the worst case of a
// block, 416 bytes (63 x 26 + 20 bits, every byte stuffed), for every block.
//
// Lanes of a wave code different intervals, so they diverge at every symbol; what keeps that
// affordable is that intervals are many (a batch of twelve-megapixel pictures has thousands per
// picture at 16 MCUs each) and each lane's coefficient stream is sequential.  LDS: a block's 64
// words lie 72 apart, so the column pass, whose lanes read (block, column), meets each bank
// twice per wave, the least 64 lanes can; the row pass reads 8 consecutive words per lane.
#include "jpeg.hpp"

#if defined(HG_HOST_EMU)
#include <atomic>
#endif

namespace hg {

namespace {

constexpr int kLdsRow = 392;     // bytes of one RGB row: 3 * 128 and up to 3 on either side of it
constexpr int kBlkStride = 72;   // words between blocks in LDS

}  // namespace

__global__ void __launch_bounds__(256) k_jpeg_coef(JpegArgs a) {
    HG_BLOCK_SHARED uint32_t rgb32[16 * kLdsRow / 4];
    HG_BLOCK_SHARED int32_t blk[kJpegGroupBlocks * kBlkStride];
    uint8_t *const rgb = reinterpret_cast<uint8_t *>(rgb32);
    const JpegPic &p = a.pics[blockIdx.y];
    const uint32_t g = blockIdx.x;
    if (g >= p.groups_x * p.mcus_y) return;  // (uniform: the whole work-group leaves)
    const int tid = int(threadIdx.x), nthr = int(blockDim.x);
    const bool s420 = a.sub == JPEG_420;
    const int mcu = s420 ? 16 : 8, bpm = s420 ? 6 : 3;
    const uint32_t mrow = g / p.groups_x, gx = g % p.groups_x;
    const uint32_t x0 = gx * kJpegGroupPx, y0 = mrow * uint32_t(mcu);
    const uint32_t m0 = x0 / uint32_t(mcu);                                                // first MCU of the group
    const int n_mcu = int(min(p.mcus_x - m0, uint32_t(kJpegGroupPx / mcu)));              // MCUs it holds
    const int nblk = n_mcu * bpm;
    const int cols = int(min(p.w - x0, uint32_t(kJpegGroupPx)));                           // picture columns it holds
    const int rows = int(min(p.h - y0, uint32_t(mcu)));                                    // picture rows it holds
    const int nbytes = 3 * cols;

    // the rows' bytes, each row at its address's offset within a dword: whole dwords inside the
    // row are loaded as dwords, the row's ends byte by byte; nothing outside the row is read
    for (int i = tid; i < rows * (kLdsRow / 4); i += nthr) {
        const int r = i / (kLdsRow / 4), d = i % (kLdsRow / 4);
        const uint8_t *src = p.rgb + int64_t(y0 + uint32_t(r)) * p.pitch + size_t(x0) * 3;
        const int mis = int(reinterpret_cast<uintptr_t>(src) & 3u);
        const int lo = 4 * d, hi = lo + 4;  // bytes of this dword, counted from the aligned address
        if (lo >= mis + nbytes || hi <= mis) continue;
        const uint8_t *gp = src - mis + lo;
        if (lo >= mis && hi <= mis + nbytes) {
            rgb32[r * (kLdsRow / 4) + d] = *reinterpret_cast<const uint32_t *>(gp);
        } else {
            for (int j = 0; j < 4; ++j)
                if (lo + j >= mis && lo + j < mis + nbytes) rgb[r * kLdsRow + lo + j] = gp[j];
        }
    }
    __syncthreads();

    // samples minus 128, block by block; column and row clamped to the picture's last
    for (int i = tid; i < nblk * 64; i += nthr) {
        const int b = i >> 6, k = i & 63, bx = k & 7, by = k >> 3;
        const int m = b / bpm, j = b % bpm;
        int comp, px, py, v;
        if (s420 && j < 4) comp = 0, px = m * 16 + (j & 1) * 8 + bx, py = (j >> 1) * 8 + by;
        else if (s420) comp = j - 3, px = m * 16 + 2 * bx, py = 2 * by;
        else comp = j, px = m * 8 + bx, py = by;
        auto at = [&](int x, int y) {
            x = min(x, cols - 1);
            y = min(y, rows - 1);
            const uint8_t *src = p.rgb + int64_t(y0 + uint32_t(y)) * p.pitch + size_t(x0) * 3;
            const int mis = int(reinterpret_cast<uintptr_t>(src) & 3u);
            return jpeg_ycc(rgb + y * kLdsRow + mis + 3 * x, comp);
        };
        if (s420 && j >= 4) v = (at(px, py) + at(px + 1, py) + at(px, py + 1) + at(px + 1, py + 1) + 2) >> 2;
        else v = at(px, py);
        blk[b * kBlkStride + k] = v - 128;
    }
    __syncthreads();
    for (int i = tid; i < nblk * 8; i += nthr) jpeg_dct_row(blk + (i >> 3) * kBlkStride + (i & 7) * 8);
    __syncthreads();
    for (int i = tid; i < nblk * 8; i += nthr) jpeg_dct_col(blk + (i >> 3) * kBlkStride + (i & 7), 8);
    __syncthreads();

    // the group's blocks are consecutive in scan order
    int16_t *out = a.coef + p.coef_off + (size_t(mrow) * p.mcus_x + m0) * size_t(bpm) * 64;
    for (int i = tid; i < nblk * 64; i += nthr) {
        const int b = i >> 6, k = i & 63, j = b % bpm;
        const int nat = kZigzag[k];
        const int tab = s420 ? (j < 4 ? 0 : 1) : (j == 0 ? 0 : 1);
        out[i] = int16_t(jpeg_quantise(blk[b * kBlkStride + nat], a.qt[tab][nat]));
    }
}

template <bool kWrite>
__global__ void __launch_bounds__(256) k_jpeg_entropy(JpegArgs a) {
    const JpegPic &p = a.pics[blockIdx.y];
    const uint64_t mcus = uint64_t(p.mcus_x) * p.mcus_y;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.n_int; i += gridDim.x * blockDim.x) {
        const uint64_t m0 = uint64_t(i) * p.ri, m1 = min(m0 + p.ri, mcus);
        const uint32_t marker = i + 1 < p.n_int ? 0xd0u + (i & 7u) : 0xd9u;
        JpegSink<kWrite> s{p.out, kWrite ? a.ioff[p.int_off + i] : 0, p.cap, 0, 0};
        const uint64_t start = s.pos;
        jpeg_put_interval(s, a.coef + p.coef_off, uint32_t(m0), uint32_t(m1), a.sub, marker);
        if (!kWrite) a.ilen[p.int_off + i] = uint32_t(s.pos - start);
    }
}

__global__ void __launch_bounds__(256) k_jpeg_offsets(JpegArgs a) {
    HG_BLOCK_SHARED uint64_t part[256];
    const JpegPic &p = a.pics[blockIdx.x];
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t seg = (p.n_int + nthr - 1) / nthr;  // consecutive intervals per thread
    const uint32_t i0 = min(tid * uint64_t(seg), uint64_t(p.n_int)), i1 = min(uint64_t(i0) + seg, uint64_t(p.n_int));
    uint64_t sum = 0;
    for (uint32_t i = i0; i < i1; ++i) sum += a.ilen[p.int_off + i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (uint32_t t = 0; t < nthr; ++t) {
            const uint64_t v = part[t];
            part[t] = run;
            run += v;
        }
        a.sizes[blockIdx.x] = run | (run > p.cap ? uint64_t(1) << 63 : 0);
    }
    __syncthreads();
    uint64_t off = part[tid];
    for (uint32_t i = i0; i < i1; ++i) {
        a.ioff[p.int_off + i] = off;
        off += a.ilen[p.int_off + i];
    }
}

#if defined(HG_HOST_EMU)
namespace {
// one block at a time, one host thread of one lane per block (blockDim.x == 1)
template <class K>
void jpeg_emu_launch(K kernel, unsigned gx, unsigned gy, const JpegArgs &a) {
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

void emu_jpeg_encode(const JpegArgs &a, uint32_t max_groups, uint32_t max_int) {
    if (a.n <= 0) return;
    jpeg_emu_launch(k_jpeg_coef, max_groups, unsigned(a.n), a);
    jpeg_emu_launch(k_jpeg_entropy<false>, 1, unsigned(a.n), a);
    jpeg_emu_launch(k_jpeg_offsets, unsigned(a.n), 1, a);
    jpeg_emu_launch(k_jpeg_entropy<true>, 1, unsigned(a.n), a);
}
#else
hipError_t launch_jpeg_encode(const JpegArgs &a, uint32_t max_groups, uint32_t max_int, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const dim3 ent((max_int + 255) / 256, unsigned(a.n));
    hipLaunchKernelGGL(k_jpeg_coef, dim3(max_groups, unsigned(a.n)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_entropy<false>, ent, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_offsets, dim3(unsigned(a.n)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_entropy<true>, ent, dim3(256), 0, s, a);
    return hipGetLastError();
}
#endif

}  // namespace hg
