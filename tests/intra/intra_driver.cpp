// intra_driver.cpp — TEST-ONLY driver of k_intra alone (tests/test_intra_predict.py).
//
// Reads a case file of hand-built inputs in the product's own structs (SeqParams,
// PicDesc, per-row TU counts, TuRecs, residual planes), fills the BatchArgs fields
// k_intra reads, runs it once per batch over a sample arena pre-filled with a
// sentinel, and writes the arena and the status words back.
//   intra_driver --layout            sizeof / offsetof of the mirrored structs
//   intra_driver case.bin result.bin
// Two builds of this one source:
//   hipcc, linked with heif_amd/libheifgpu.so: hg::launch_intra, the product's own object;
//   g++ -DHG_HOST_EMU with kernels/intra.hip: hg::emu_intra (make intra-emu).
//
// Case file (little endian): magic, n_batches, then per batch 16 uint32 of header
//   n_seqs, n_pics, pic0, n_launch, max_rows, n_row_words, n_tus, resid_elems,
//   recon_bytes, bytes_per_sample, chroma_format, max_log2ctb, sentinel byte, 0, 0, 0
// then the seqs, pics, row-count words, tus and the residual arena, in that order.
// A batch is one BatchArgs: one sample size and one chroma format.  The result
// file holds, per batch, the sample arena and one status word per picture.
// Everything the kernel will index is checked against the arrays' sizes before
// anything runs.
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

constexpr uint32_t kMagic = 0x31435049u;  // "IPC1"

struct Batch {
    uint32_t pic0 = 0, n_launch = 0, max_rows = 0, bps = 0, chroma_format = 0, max_log2ctb = 0, sentinel = 0;
    uint32_t recon_bytes = 0;
    std::vector<SeqParams> seqs;
    std::vector<PicDesc> pics;
    std::vector<uint32_t> rows;
    std::vector<TuRec> tus;
    std::vector<int16_t> resid;
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
        ok = fread(h, 4, 16, f) == 16 && h[7] <= (1u << 27) && h[8] <= (1u << 28) && h[6] <= (1u << 24);
        if (!ok) break;
        b.pic0 = h[2];
        b.n_launch = h[3];
        b.max_rows = h[4];
        b.recon_bytes = h[8];
        b.bps = h[9];
        b.chroma_format = h[10];
        b.max_log2ctb = h[11];
        b.sentinel = h[12];
        ok = read_vec(f, b.seqs, h[0]) && read_vec(f, b.pics, h[1]) && read_vec(f, b.rows, h[5]) &&
             read_vec(f, b.tus, h[6]) && read_vec(f, b.resid, h[7]);
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

uint64_t al16(uint64_t v) { return (v + 15) & ~uint64_t(15); }

// every index k_intra forms from the case's data stays inside the arrays.  The
// record fields themselves are the kernel's to check (a record that does not
// pack is skipped); a record's ctu only ever selects a CTU below wctb.
bool validate(const Batch &c) {
    size_t p = 0;
    REQUIRE(c.n_launch >= 1 && c.max_rows >= 1 && c.max_rows <= 4096);
    REQUIRE(uint64_t(c.pic0) + c.n_launch <= c.pics.size());
    REQUIRE(c.bps == 1 || c.bps == 2);
    REQUIRE(c.chroma_format <= 3);
    REQUIRE(c.max_log2ctb >= 4 && c.max_log2ctb <= 6);
    {  // one wave's LDS block for the largest CTB: scratch, then per component window, left column, row above
        const uint64_t c0 = 1u << c.max_log2ctb, bps = c.bps;
        const uint64_t cx = c.chroma_format ? c0 >> chroma_sx(int(c.chroma_format)) : 0;
        const uint64_t cy = c.chroma_format ? c0 >> chroma_sy(int(c.chroma_format)) : 0;
        const uint64_t blk = al16(4 * 66 * 2) + al16(c0 * c0 * bps) + al16(c0 * bps) + al16((2 * c0 + 1) * bps) +
                             2 * (al16(cx * cy * bps) + al16(cy * bps) + al16((2 * cx + 1) * bps));
        REQUIRE(64 + 2 * blk <= 128 * 1024);  // (two waves: a split launch never runs with fewer)
    }
    for (p = c.pic0; p < size_t(c.pic0) + c.n_launch; ++p) {
        const PicDesc &pd = c.pics[p];
        if (pd.flags & PD_ASSEMBLY) continue;
        REQUIRE(pd.seq < c.seqs.size());
        const SeqParams &sp = c.seqs[pd.seq];
        REQUIRE(sp.width > 0 && sp.height > 0 && sp.width <= 8192 && sp.height <= 8192);
        REQUIRE(sp.log2_ctb >= 4 && sp.log2_ctb <= int(c.max_log2ctb));
        REQUIRE(sp.chroma_format == int(c.chroma_format));
        const int bd_max = c.bps == 1 ? 8 : 15;  // (predictions are held as int16)
        REQUIRE(sp.bit_depth_y >= 8 && sp.bit_depth_y <= bd_max && sp.bit_depth_c >= 8 && sp.bit_depth_c <= bd_max);
        const uint64_t W = uint64_t(sp.width), H = uint64_t(sp.height);
        const uint64_t cw = sp.chroma_format ? W >> chroma_sx(sp.chroma_format) : 0;
        const uint64_t ch = sp.chroma_format ? H >> chroma_sy(sp.chroma_format) : 0;
        const uint64_t samples = W * H + 2 * cw * ch;
        REQUIRE(pd.recon_off % 8 == 0 && pd.recon_off + samples * c.bps <= c.recon_bytes);
        REQUIRE(pd.resid_off + samples <= c.resid.size());
        const uint64_t hctb = (H + (1u << sp.log2_ctb) - 1) >> sp.log2_ctb;
        REQUIRE(hctb <= c.max_rows);
        for (uint64_t r = 0; r < hctb; ++r) {
            REQUIRE(2 * (pd.row_off + r) + 1 < c.rows.size());
            const uint32_t ntu = c.rows[2 * (pd.row_off + r)];
            REQUIRE(ntu <= pd.tu_cap_row);
            REQUIRE(pd.tu_off + r * pd.tu_cap_row + ntu <= c.tus.size());
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
    OFF(SeqParams, log2_min_cb);
    OFF(SeqParams, log2_min_tb);
    OFF(SeqParams, log2_max_tb);
    OFF(SeqParams, max_th_depth_intra);
    OFF(SeqParams, chroma_format);
    OFF(SeqParams, bit_depth_y);
    OFF(SeqParams, bit_depth_c);
    OFF(SeqParams, flags);
    OFF(SeqParams, diff_cu_qp_delta_depth);
    OFF(SeqParams, cb_qp_offset);
    OFF(SeqParams, cr_qp_offset);
    OFF(SeqParams, log2_min_pcm);
    OFF(SeqParams, log2_max_pcm);
    OFF(SeqParams, pcm_bd_y);
    OFF(SeqParams, pcm_bd_c);
    OFF(SeqParams, conf_l);
    OFF(SeqParams, conf_t);
    OFF(SeqParams, out_w);
    OFF(SeqParams, out_h);
    OFF(SeqParams, sf_off);
    OFF(SeqParams, pad);
    SZ(PicDesc);
    OFF(PicDesc, bits_off);
    OFF(PicDesc, bits_len);
    OFF(PicDesc, sub_first);
    OFF(PicDesc, n_sub);
    OFF(PicDesc, seq);
    OFF(PicDesc, slice_qp);
    OFF(PicDesc, cb_qp_off);
    OFF(PicDesc, cr_qp_off);
    OFF(PicDesc, sao_luma);
    OFF(PicDesc, sao_chroma);
    OFF(PicDesc, dbk_disabled);
    OFF(PicDesc, beta_off);
    OFF(PicDesc, tc_off);
    OFF(PicDesc, image);
    OFF(PicDesc, out_x);
    OFF(PicDesc, out_y);
    OFF(PicDesc, recon_off);
    OFF(PicDesc, resid_off);
    OFF(PicDesc, map_off);
    OFF(PicDesc, sao_off);
    OFF(PicDesc, tu_off);
    OFF(PicDesc, coef_off);
    OFF(PicDesc, row_off);
    OFF(PicDesc, tu_cap_row);
    OFF(PicDesc, coef_cap_row);
    OFF(PicDesc, flags);
    OFF(PicDesc, org_x);
    OFF(PicDesc, org_y);
    OFF(PicDesc, child0);
    OFF(PicDesc, nchild);
    SZ(TuRec);
    OFF(TuRec, x);
    OFF(TuRec, y);
    OFF(TuRec, log2);
    OFF(TuRec, flags);
    OFF(TuRec, mode);
    OFF(TuRec, qp);
    OFF(TuRec, coef);
    OFF(TuRec, ncoef);
    OFF(TuRec, ctu);
#undef SZ
#undef OFF
    printf("SP_STRONG_INTRA %u\n", unsigned(SP_STRONG_INTRA));
    printf("PD_ASSEMBLY %u\n", unsigned(PD_ASSEMBLY));
    printf("TU_CIDX_MASK %u\nTU_CBF %u\nTU_BYPASS %u\nTU_PCM %u\n", unsigned(TU_CIDX_MASK), unsigned(TU_CBF),
           unsigned(TU_BYPASS), unsigned(TU_PCM));
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
    for (const Batch &b : bs)
        if (!validate(b)) return 3;
    FILE *f = fopen(argv[2], "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    for (Batch &b : bs) {
        std::vector<uint8_t> recon(b.recon_bytes, uint8_t(b.sentinel));
        std::vector<uint32_t> status(b.pics.size(), 0u);
        std::vector<Coef> coefs(4, 0u);  // (k_intra forms a row's coefficient pointer and never reads it)
        for (PicDesc &pd : b.pics) pd.coef_off = 0, pd.coef_cap_row = 0;
        BatchArgs a{};
        a.n_pics = int(b.n_launch);
        a.pic0 = int(b.pic0);
        a.max_rows = int(b.max_rows);
        a.bytes_per_sample = int(b.bps);
        a.chroma_format = int(b.chroma_format);
        a.max_log2ctb = int(b.max_log2ctb);
        int total_rows = 0;
        for (const PicDesc &pd : b.pics)
            if (!(pd.flags & PD_ASSEMBLY) && pd.seq < b.seqs.size()) {
                const SeqParams &sp = b.seqs[pd.seq];
                total_rows += (sp.height + (1 << sp.log2_ctb) - 1) >> sp.log2_ctb;
            }
        a.total_rows = total_rows;
#if defined(HG_HOST_EMU)
        a.pics = b.pics.data();
        a.seqs = b.seqs.data();
        a.tus = b.tus.data();
        a.coefs = coefs.data();
        a.row_counts = b.rows.data();
        a.resid = b.resid.data();
        a.recon = recon.data();
        a.status = status.data();
        emu_intra(a);
#else
        a.pics = to_device(b.pics);
        a.seqs = to_device(b.seqs);
        a.tus = to_device(b.tus);
        a.coefs = to_device(coefs);
        a.row_counts = to_device(b.rows);
        a.resid = to_device(b.resid);
        a.recon = to_device(recon);
        a.status = to_device(status);
        CK(launch_intra(a, nullptr));
        CK(hipDeviceSynchronize());
        if (!recon.empty()) CK(hipMemcpy(recon.data(), a.recon, recon.size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(status.data(), a.status, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
#endif
        if (fwrite(recon.data(), 1, recon.size(), f) != recon.size() ||
            fwrite(status.data(), sizeof(uint32_t), status.size(), f) != status.size()) {
            fprintf(stderr, "cannot write %s\n", argv[2]);
            return 2;
        }
        printf("intra ok: %u pictures, %zu sample bytes\n", b.n_launch, recon.size());
    }
    if (fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    return 0;
}
