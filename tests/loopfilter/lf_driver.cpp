// lf_driver.cpp — TEST-ONLY driver of the loop filter alone (tests/test_loopfilter.py):
// k_assemble, k_deblock and k_sao_out, nothing before them.
//
// Reads a case file of hand-built inputs in the product's own structs (SeqParams,
// PicDesc, OutImage, the QpY / flag maps, SaoParams, the sample arena), fills the
// BatchArgs fields these kernels read, runs deblocking, copies the sample arena
// back, runs SAO + output over caller planes pre-filled with a sentinel, and
// writes both buffers.
//   lf_driver --layout            sizeof / offsetof of the mirrored structs
//   lf_driver case.bin result.bin
// Two builds of this one source:
//   hipcc, linked with heif_amd/libheifgpu.so: hg::launch_deblock / hg::launch_sao_out,
//     the product's own object;
//   g++ -DHG_HOST_EMU with kernels/loopfilter.hip: hg::emu_deblock / hg::emu_sao_out
//     (make lf-emu).
//
// Case file (little endian): magic, n_batches, then per batch 16 uint32 of header
//   n_seqs, n_pics, pic0, n_launch, n_outs, map_bytes, n_sao, recon_bytes,
//   out_bytes, bytes_per_sample, chroma_format, has_assembly, sentinel byte, 0, 0, 0
// then the seqs, pics, outs, map bytes, SaoParams and the sample arena, in that
// order.  OutImage::plane holds byte offsets into the batch's one output
// allocation (256-byte aligned, like the sample arena).  A batch is one BatchArgs:
// one sample size.  The result file holds, per batch, the sample arena after
// deblocking and the output allocation after SAO.  Everything the kernels will
// index is checked against the arrays' sizes before anything runs.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels/kernels.hpp"

#if defined(HG_HOST_EMU)
namespace hg {
thread_local EmuCtx g_emu;
}
#endif
using namespace hg;

namespace {

constexpr uint32_t kMagic = 0x3143464cu;  // "LFC1"

struct Batch {
    uint32_t pic0 = 0, n_launch = 0, out_bytes = 0, bps = 0, chroma_format = 0, has_assembly = 0, sentinel = 0;
    std::vector<SeqParams> seqs;
    std::vector<PicDesc> pics;
    std::vector<OutImage> outs;
    std::vector<uint8_t> maps;
    std::vector<SaoParams> sao;
    std::vector<uint8_t> recon;
};

template <class T>
bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool load_case(const char *path, std::vector<Batch> &bs) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint32_t top[2];
    bool ok = fread(top, 4, 2, f) == 2 && top[0] == kMagic && top[1] >= 1 && top[1] <= 64;
    for (uint32_t i = 0; ok && i < top[1]; ++i) {
        uint32_t h[16];
        Batch b;
        ok = fread(h, 4, 16, f) == 16 && h[7] <= (1u << 28) && h[8] <= (1u << 28);
        if (!ok) break;
        b.pic0 = h[2];
        b.n_launch = h[3];
        b.out_bytes = h[8];
        b.bps = h[9];
        b.chroma_format = h[10];
        b.has_assembly = h[11];
        b.sentinel = h[12];
        ok = read_vec(f, b.seqs, h[0]) && read_vec(f, b.pics, h[1]) && read_vec(f, b.outs, h[4]) &&
             read_vec(f, b.maps, h[5]) && read_vec(f, b.sao, h[6]) && read_vec(f, b.recon, h[7]);
        bs.push_back(std::move(b));
    }
    fclose(f);
    return ok;
}

#define REQUIRE(cond)                                                            \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "case rejected (pic %u): %s\n", unsigned(p), #cond); \
            return false;                                                        \
        }                                                                        \
    } while (0)

// the arrays one picture owns lie inside the batch's arenas
bool validate_pic(const Batch &b, size_t p) {
    REQUIRE(p < b.pics.size());
    const PicDesc &pd = b.pics[p];
    REQUIRE(pd.seq < b.seqs.size());
    const SeqParams &sp = b.seqs[pd.seq];
    REQUIRE(sp.width >= 8 && sp.height >= 8 && sp.width <= 8192 && sp.height <= 8192);
    REQUIRE(sp.width % 8 == 0 && sp.height % 8 == 0);  // MinCbSizeY multiples: every p3..q3 line is inside
    REQUIRE(sp.log2_ctb >= 4 && sp.log2_ctb <= 6);
    REQUIRE(sp.chroma_format >= 0 && sp.chroma_format <= 3 && uint32_t(sp.chroma_format) == b.chroma_format);
    REQUIRE(sp.bit_depth_y >= 8 && sp.bit_depth_y <= int(8 * b.bps) && sp.bit_depth_y <= 12);
    REQUIRE(sp.bit_depth_c >= 8 && sp.bit_depth_c <= int(8 * b.bps) && sp.bit_depth_c <= 12);
    const uint64_t W = uint64_t(sp.width), H = uint64_t(sp.height);
    const uint64_t cw = sp.chroma_format ? W >> chroma_sx(sp.chroma_format) : 0;
    const uint64_t ch = sp.chroma_format ? H >> chroma_sy(sp.chroma_format) : 0;
    REQUIRE(pd.recon_off % b.bps == 0);
    REQUIRE(pd.recon_off + (W * H + 2 * cw * ch) * b.bps <= b.recon.size());
    const uint64_t w4 = (W + 3) >> 2, h4 = (H + 3) >> 2;
    REQUIRE(pd.map_off + 2 * w4 * h4 <= b.maps.size());
    const uint64_t wctb = (W + (1u << sp.log2_ctb) - 1) >> sp.log2_ctb;
    const uint64_t hctb = (H + (1u << sp.log2_ctb) - 1) >> sp.log2_ctb;
    REQUIRE(pd.sao_off + wctb * hctb <= b.sao.size());
    const int maxv = (1 << sp.bit_depth_y) - 1, maxc = (1 << sp.bit_depth_c) - 1;
    if (!(pd.flags & PD_ASSEMBLY))  // samples are in range (the band index is a table index); an assembly's are copied in
        for (uint64_t i = 0; i < W * H + 2 * cw * ch; ++i) {
            const uint8_t *s = b.recon.data() + pd.recon_off + i * b.bps;
            const int v = b.bps == 1 ? s[0] : s[0] | s[1] << 8;
            REQUIRE(v <= (i < W * H ? maxv : maxc));
        }
    return true;
}

// every index the three kernels form from the batch's data stays inside the arrays
bool validate(const Batch &b) {
    size_t p = 0;
    REQUIRE(b.bps == 1 || b.bps == 2);
    REQUIRE(b.n_launch >= 1 && uint64_t(b.pic0) + b.n_launch <= b.pics.size());
    for (size_t i = b.pic0; i < size_t(b.pic0) + b.n_launch; ++i) {
        p = i;
        if (!validate_pic(b, p)) return false;
        const PicDesc &pd = b.pics[p];
        const SeqParams &sp = b.seqs[pd.seq];
        if (pd.flags & PD_ASSEMBLY) {
            REQUIRE(b.has_assembly);
            REQUIRE(uint64_t(pd.child0) + pd.nchild <= b.pics.size());
            for (size_t c = pd.child0; c < size_t(pd.child0) + pd.nchild; ++c) {
                if (!validate_pic(b, c)) return false;
                const PicDesc &cd = b.pics[c];
                const SeqParams &cs = b.seqs[cd.seq];
                const int ctb = 1 << sp.log2_ctb;
                REQUIRE(cs.log2_ctb == sp.log2_ctb && cs.chroma_format == sp.chroma_format);
                REQUIRE(cd.org_x >= 0 && cd.org_y >= 0 && cd.org_x % ctb == 0 && cd.org_y % ctb == 0);
                REQUIRE(cd.org_x + cs.width <= sp.width && cd.org_y + cs.height <= sp.height);
            }
        }
        if (pd.flags & PD_CHILD) continue;  // k_sao_out leaves at once
        REQUIRE(pd.image < b.outs.size());
        const OutImage &oi = b.outs[pd.image];
        REQUIRE(sp.conf_l >= 0 && sp.conf_t >= 0 && sp.out_w > 0 && sp.out_h > 0);
        REQUIRE(sp.conf_l + sp.out_w <= sp.width && sp.conf_t + sp.out_h <= sp.height);
        REQUIRE(pd.out_x >= 0 && pd.out_y >= 0 && oi.width > 0 && oi.height > 0);
        const int sx = chroma_sx(sp.chroma_format), sy = chroma_sy(sp.chroma_format);
        REQUIRE(sp.conf_l % (1 << sx) == 0 && sp.conf_t % (1 << sy) == 0);
        const int64_t vw = std::min<int64_t>(sp.out_w, int64_t(oi.width) - pd.out_x);
        const int64_t vh = std::min<int64_t>(sp.out_h, int64_t(oi.height) - pd.out_y);
        if (vw <= 0 || vh <= 0) continue;
        for (int c = 0; c < (sp.chroma_format ? 3 : 1); ++c) {
            const int kx = c ? sx : 0, ky = c ? sy : 0;
            const int64_t cvw = (vw + (1 << kx) - 1) >> kx, cvh = (vh + (1 << ky) - 1) >> ky;
            REQUIRE((sp.conf_l >> kx) + cvw <= (sp.width >> kx) && (sp.conf_t >> ky) + cvh <= (sp.height >> ky));
            REQUIRE(oi.pitch[c] > 0 && oi.pitch[c] % int(b.bps) == 0 && oi.plane[c] % b.bps == 0);
            const uint64_t last = oi.plane[c] + uint64_t((pd.out_y >> ky) + cvh - 1) * oi.pitch[c] +
                                  uint64_t((pd.out_x >> kx) + cvw) * b.bps;
            REQUIRE(last <= b.out_bytes);
        }
    }
    return true;
}

int layout() {
#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
    SZ(SeqParams);
    OFF(SeqParams, width);
    OFF(SeqParams, height);
    OFF(SeqParams, log2_ctb);
    OFF(SeqParams, chroma_format);
    OFF(SeqParams, bit_depth_y);
    OFF(SeqParams, bit_depth_c);
    OFF(SeqParams, cb_qp_offset);
    OFF(SeqParams, cr_qp_offset);
    OFF(SeqParams, conf_l);
    OFF(SeqParams, conf_t);
    OFF(SeqParams, out_w);
    OFF(SeqParams, out_h);
    SZ(PicDesc);
    OFF(PicDesc, seq);
    OFF(PicDesc, sao_luma);
    OFF(PicDesc, sao_chroma);
    OFF(PicDesc, dbk_disabled);
    OFF(PicDesc, beta_off);
    OFF(PicDesc, tc_off);
    OFF(PicDesc, image);
    OFF(PicDesc, out_x);
    OFF(PicDesc, out_y);
    OFF(PicDesc, recon_off);
    OFF(PicDesc, map_off);
    OFF(PicDesc, sao_off);
    OFF(PicDesc, flags);
    OFF(PicDesc, org_x);
    OFF(PicDesc, org_y);
    OFF(PicDesc, child0);
    OFF(PicDesc, nchild);
    SZ(SaoParams);
    OFF(SaoParams, type);
    OFF(SaoParams, band_eo);
    OFF(SaoParams, off);
    OFF(SaoParams, pad);
    SZ(OutImage);
    OFF(OutImage, plane);
    OFF(OutImage, pitch);
    OFF(OutImage, width);
    OFF(OutImage, height);
#undef SZ
#undef OFF
    printf("MF_EDGE_V %u\nMF_EDGE_H %u\nMF_NOFILT %u\n", unsigned(MF_EDGE_V), unsigned(MF_EDGE_H), unsigned(MF_NOFILT));
    printf("PD_CHILD %u\nPD_ASSEMBLY %u\n", unsigned(PD_CHILD), unsigned(PD_ASSEMBLY));
    return 0;
}

#if !defined(HG_HOST_EMU)
#define CK(call)                                                                     \
    do {                                                                             \
        const hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s: %s (%d)\n", #call, hipGetErrorString(e_), int(e_)); \
            exit(1); /* nothing further is launched */                               \
        }                                                                            \
    } while (0)

template <class T>
T *to_device(const std::vector<T> &v) {
    void *d = nullptr;
    CK(hipMalloc(&d, v.empty() ? sizeof(T) : v.size() * sizeof(T)));
    if (!v.empty()) CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return static_cast<T *>(d);
}
#endif

bool write_all(FILE *f, const uint8_t *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

// one batch through deblocking and SAO + output; its two result buffers appended to f
bool run_batch(const Batch &b, FILE *f) {
    BatchArgs a{};
    a.n_pics = int(b.n_launch);
    a.pic0 = int(b.pic0);
    a.bytes_per_sample = int(b.bps);
    a.chroma_format = int(b.chroma_format);
    a.has_assembly = int(b.has_assembly);
    std::vector<OutImage> outs = b.outs;
    std::vector<uint8_t> recon(b.recon.size()), out(b.out_bytes);
#if defined(HG_HOST_EMU)
    const size_t rn = (b.recon.size() + 255) & ~size_t(255), on = (size_t(b.out_bytes) + 255) & ~size_t(255);
    uint8_t *d_recon = static_cast<uint8_t *>(aligned_alloc(256, rn ? rn : 256));
    uint8_t *d_out = static_cast<uint8_t *>(aligned_alloc(256, on ? on : 256));
    if (!d_recon || !d_out) return false;
    memcpy(d_recon, b.recon.data(), b.recon.size());
    memset(d_out, int(b.sentinel), b.out_bytes);
    for (OutImage &oi : outs)
        for (int c = 0; c < 3; ++c) oi.plane[c] += reinterpret_cast<uintptr_t>(d_out);
    std::vector<uint8_t> maps = b.maps;
    std::vector<SaoParams> sao = b.sao;
    a.pics = b.pics.data();
    a.seqs = b.seqs.data();
    a.outs = outs.data();
    a.recon = d_recon;
    a.maps = maps.data();
    a.sao = sao.data();
    emu_deblock(a);
    memcpy(recon.data(), d_recon, recon.size());
    emu_sao_out(a);
    memcpy(out.data(), d_out, out.size());
    free(d_recon);
    free(d_out);
#else
    uint8_t *d_recon = to_device(b.recon);
    void *d_out = nullptr;
    CK(hipMalloc(&d_out, b.out_bytes ? b.out_bytes : 1));
    CK(hipMemset(d_out, int(b.sentinel), b.out_bytes));
    for (OutImage &oi : outs)
        for (int c = 0; c < 3; ++c) oi.plane[c] += reinterpret_cast<uintptr_t>(d_out);
    a.pics = to_device(b.pics);
    a.seqs = to_device(b.seqs);
    a.outs = to_device(outs);
    a.recon = d_recon;
    a.maps = to_device(b.maps);
    a.sao = to_device(b.sao);
    CK(launch_deblock(a, nullptr));
    CK(hipDeviceSynchronize());
    if (!recon.empty()) CK(hipMemcpy(recon.data(), d_recon, recon.size(), hipMemcpyDeviceToHost));
    CK(launch_sao_out(a, nullptr));
    CK(hipDeviceSynchronize());
    if (!out.empty()) CK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
    CK(hipFree(d_out));
    CK(hipFree(d_recon));
    CK(hipFree(const_cast<PicDesc *>(a.pics)));
    CK(hipFree(const_cast<SeqParams *>(a.seqs)));
    CK(hipFree(const_cast<OutImage *>(a.outs)));
    CK(hipFree(a.maps));
    CK(hipFree(a.sao));
#endif
    return write_all(f, recon.data(), recon.size()) && write_all(f, out.data(), out.size());
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--layout")) return layout();
    if (argc != 3) {
        fprintf(stderr, "usage: %s --layout | case.bin result.bin\n", argv[0]);
        return 2;
    }
    std::vector<Batch> bs;
    if (!load_case(argv[1], bs)) {
        fprintf(stderr, "cannot read case file %s\n", argv[1]);
        return 2;
    }
    for (const Batch &b : bs)  // all of them before anything runs
        if (!validate(b)) return 3;
    FILE *f = fopen(argv[2], "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    for (const Batch &b : bs)
        if (!run_batch(b, f)) {
            fprintf(stderr, "batch failed\n");
            return 2;
        }
    if (fclose(f) != 0) return 2;
    printf("loop filter ok: %zu batches\n", bs.size());
    return 0;
}
