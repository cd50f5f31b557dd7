// rbsp_driver.cpp — TEST-ONLY driver of k_rbsp alone (tests/test_rbsp.py).
//
// Reads a case file of hand-built inputs in the product's own structs (SeqParams,
// PicDesc, the payload arena, the substream table), fills the BatchArgs fields
// k_rbsp reads, runs it once per batch over output arenas pre-filled with a
// sentinel, and writes every one of them back.
//   rbsp_driver --layout            sizeof / offsetof of the mirrored structs
//   rbsp_driver case.bin result.bin
// Two builds of this one source:
//   hipcc, linked with heif_amd/libheifgpu.so: hg::launch_rbsp, the product's own object;
//   g++ -DHG_HOST_EMU with kernels/rbsp.hip: hg::emu_rbsp (make rbsp-emu, under ASan + UBSan).
//
// Case file (little endian): magic, n_batches, then per batch 16 uint32 of header
//   n_seqs, n_pics, pic0, n_launch, bits_bytes, n_subs, total_rows, optional pointers
//   (bit 0 cu_counts, 1 xprog, 2 xntu, 3 xjob; clear: null), intra_stream, sentinel byte, 0 x 6
// then the seqs, pics, the payload arena (its padding included: the case plants what
// lies behind a payload) and the substream table.  The result file holds, per batch,
// rbsp (bits_bytes), rsubs (n_subs words), status (n_pics), row_counts (2 x total_rows),
// cu_counts, xprog (total_rows each), xntu (total_rows + n_pics) and xjob (1); an array
// whose pointer the batch leaves null is written as the sentinel it was filled with.
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

constexpr uint32_t kMagic = 0x31535052u;  // "RPS1"
enum : uint32_t { OPT_CU = 1, OPT_XPROG = 2, OPT_XNTU = 4, OPT_XJOB = 8 };

struct Batch {
    uint32_t pic0 = 0, n_launch = 0, total_rows = 0, opt = 0, intra_stream = 0, sentinel = 0;
    std::vector<SeqParams> seqs;
    std::vector<PicDesc> pics;
    std::vector<uint8_t> bits;
    std::vector<uint32_t> subs;
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
        ok = fread(h, 4, 16, f) == 16 && h[0] <= 4096 && h[1] <= 4096 && h[4] <= (1u << 26) && h[5] <= (1u << 22) &&
             h[6] <= (1u << 20);
        if (!ok) break;
        b.pic0 = h[2];
        b.n_launch = h[3];
        b.total_rows = h[6];
        b.opt = h[7];
        b.intra_stream = h[8];
        b.sentinel = h[9];
        ok = read_vec(f, b.seqs, h[0]) && read_vec(f, b.pics, h[1]) && read_vec(f, b.bits, h[4]) &&
             read_vec(f, b.subs, h[5]);
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

// every index k_rbsp forms from the case's data stays inside the arrays: the 16-byte
// chunks of a payload and the dword behind the last one (loads), the chunks themselves
// (stores), the picture's table entries and its rows' counters.  An entry's VALUE needs
// no check: the kernel compares it with bits_len before it uses it.
bool validate(const Batch &c) {
    size_t p = 0;
    REQUIRE(c.n_launch >= 1 && uint64_t(c.pic0) + c.n_launch <= c.pics.size());
    REQUIRE(c.opt <= 15 && c.intra_stream <= 1);
    for (p = c.pic0; p < size_t(c.pic0) + c.n_launch; ++p) {
        const PicDesc &pd = c.pics[p];
        REQUIRE(pd.bits_off % 64 == 0);
        REQUIRE(pd.bits_off <= c.bits.size() && pd.bits_len <= (1u << 26));
        const uint64_t chunks = (uint64_t(pd.bits_len) + 15) & ~uint64_t(15);
        REQUIRE(pd.bits_off + chunks + 4 <= c.bits.size());
        const uint64_t nent = uint64_t(pd.n_sub) + 1 + (pd.flags >> PD_NMID_SHIFT);
        REQUIRE(uint64_t(pd.sub_first) + nent <= c.subs.size());
        REQUIRE(pd.seq < c.seqs.size());
        const SeqParams &sp = c.seqs[pd.seq];
        REQUIRE(sp.height > 0 && sp.height <= 8192 && sp.log2_ctb >= 4 && sp.log2_ctb <= 6);
        const uint64_t hctb = (uint64_t(sp.height) + (1u << sp.log2_ctb) - 1) >> sp.log2_ctb;
        REQUIRE(uint64_t(pd.row_off) + hctb <= c.total_rows);
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
#undef SZ
#undef OFF
    printf("PD_ASSEMBLY %u\nPD_NMID_SHIFT %u\n", unsigned(PD_ASSEMBLY), unsigned(PD_NMID_SHIFT));
    printf("SUB_OFFSET %u\nSUB_CONTINUE %u\nSUB_SEG_END %u\n", unsigned(SUB_OFFSET), unsigned(SUB_CONTINUE),
           unsigned(SUB_SEG_END));
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

template <class T>
void from_device(std::vector<T> &v, const T *d) {
    if (!v.empty()) CK(hipMemcpy(v.data(), d, v.size() * sizeof(T), hipMemcpyDeviceToHost));
}
#endif

template <class T>
bool put(FILE *f, const std::vector<T> &v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
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
    for (const Batch &b : bs)
        if (!validate(b)) return 3;
    FILE *f = fopen(argv[2], "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    for (Batch &b : bs) {
        const uint32_t sent = b.sentinel * 0x01010101u;
        const size_t rows = b.total_rows, np = b.pics.size();
        std::vector<uint8_t> rbsp(b.bits.size(), uint8_t(b.sentinel));
        std::vector<uint32_t> rsubs(b.subs.size(), sent), status(np, sent), row_counts(2 * rows, sent);
        std::vector<uint32_t> cu_counts(rows, sent), xprog(rows, sent), xntu(rows + np, sent), xjob(1, sent);
        BatchArgs a{};
        a.n_pics = int(b.n_launch);
        a.pic0 = int(b.pic0);
        a.total_rows = int(b.total_rows);
        a.intra_stream = int(b.intra_stream);
#if defined(HG_HOST_EMU)
        a.bits = b.bits.data();
        a.pics = b.pics.data();
        a.seqs = b.seqs.data();
        a.subs = b.subs.data();
        a.rbsp = rbsp.data();
        a.rsubs = rsubs.data();
        a.status = status.data();
        a.row_counts = row_counts.data();
        a.cu_counts = b.opt & OPT_CU ? cu_counts.data() : nullptr;
        a.xprog = b.opt & OPT_XPROG ? xprog.data() : nullptr;
        a.xntu = b.opt & OPT_XNTU ? xntu.data() : nullptr;
        a.xjob = b.opt & OPT_XJOB ? xjob.data() : nullptr;
        emu_rbsp(a);
#else
        a.bits = to_device(b.bits);
        a.pics = to_device(b.pics);
        a.seqs = to_device(b.seqs);
        a.subs = to_device(b.subs);
        a.rbsp = to_device(rbsp);
        a.rsubs = to_device(rsubs);
        a.status = to_device(status);
        a.row_counts = to_device(row_counts);
        a.cu_counts = b.opt & OPT_CU ? to_device(cu_counts) : nullptr;
        a.xprog = b.opt & OPT_XPROG ? to_device(xprog) : nullptr;
        a.xntu = b.opt & OPT_XNTU ? to_device(xntu) : nullptr;
        a.xjob = b.opt & OPT_XJOB ? to_device(xjob) : nullptr;
        CK(launch_rbsp(a, nullptr));
        CK(hipDeviceSynchronize());
        from_device(rbsp, a.rbsp);
        from_device(rsubs, a.rsubs);
        from_device(status, a.status);
        from_device(row_counts, a.row_counts);
        if (a.cu_counts) from_device(cu_counts, a.cu_counts);
        if (a.xprog) from_device(xprog, a.xprog);
        if (a.xntu) from_device(xntu, a.xntu);
        if (a.xjob) from_device(xjob, a.xjob);
        CK(hipFree(const_cast<uint8_t *>(a.bits)));
        CK(hipFree(const_cast<PicDesc *>(a.pics)));
        CK(hipFree(const_cast<SeqParams *>(a.seqs)));
        CK(hipFree(const_cast<uint32_t *>(a.subs)));
        CK(hipFree(a.rbsp));
        CK(hipFree(a.rsubs));
        CK(hipFree(a.status));
        CK(hipFree(a.row_counts));
        if (a.cu_counts) CK(hipFree(a.cu_counts));
        if (a.xprog) CK(hipFree(a.xprog));
        if (a.xntu) CK(hipFree(a.xntu));
        if (a.xjob) CK(hipFree(a.xjob));
#endif
        if (!(put(f, rbsp) && put(f, rsubs) && put(f, status) && put(f, row_counts) && put(f, cu_counts) &&
              put(f, xprog) && put(f, xntu) && put(f, xjob))) {
            fprintf(stderr, "cannot write %s\n", argv[2]);
            return 2;
        }
        printf("rbsp ok: %u pictures, %zu payload bytes\n", b.n_launch, rbsp.size());
    }
    if (fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    return 0;
}
