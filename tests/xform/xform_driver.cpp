// xform_driver.cpp — TEST-ONLY driver of k_transform alone (tests/test_transform.py).
//
// Reads a case file of hand-built inputs in the product's own format (SeqParams,
// PicDesc, per-row TU counts, TuRecs, coefficient words, ScalingFactor blocks),
// fills the BatchArgs fields k_transform reads, runs the transform once over a
// residual arena pre-filled with a sentinel, and writes the arena back.
//   xform_driver --layout            sizeof / offsetof of the mirrored structs
//   xform_driver case.bin resid.bin
// Two builds of this one source:
//   hipcc, linked with heif_amd/libheifgpu.so: hg::launch_transform, the
//     product's own object;
//   g++ -DHG_HOST_EMU with kernels/transform.hip: hg::emu_transform (make xform-emu).
//
// Case file (little endian): 16 uint32 of header
//   magic, n_seqs, n_pics, pic0, n_launch, max_rows, n_row_words, n_tus,
//   n_coefs, sf_bytes, resid_elems, sentinel, 0, 0, 0, 0
// then the seqs, pics, row-count words, tus, coefs and sf bytes, in that order.
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

constexpr uint32_t kMagic = 0x31434658u;  // "XFC1"

struct Case {
    uint32_t pic0 = 0, n_launch = 0, max_rows = 0, resid_elems = 0, sentinel = 0;
    std::vector<SeqParams> seqs;
    std::vector<PicDesc> pics;
    std::vector<uint32_t> rows;
    std::vector<TuRec> tus;
    std::vector<Coef> coefs;
    std::vector<uint8_t> sf;
};

template <class T>
bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool load_case(const char *path, Case &c) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint32_t h[16];
    bool ok = fread(h, 4, 16, f) == 16 && h[0] == kMagic;
    if (ok) {
        c.pic0 = h[3];
        c.n_launch = h[4];
        c.max_rows = h[5];
        c.resid_elems = h[10];
        c.sentinel = h[11];
        ok = read_vec(f, c.seqs, h[1]) && read_vec(f, c.pics, h[2]) && read_vec(f, c.rows, h[6]) &&
             read_vec(f, c.tus, h[7]) && read_vec(f, c.coefs, h[8]) && read_vec(f, c.sf, h[9]);
    }
    fclose(f);
    return ok;
}

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "case rejected (pic %u): %s\n", unsigned(p), #cond); \
            return false;                                                    \
        }                                                                    \
    } while (0)

// every index k_transform forms from the case's data stays inside the arrays
bool validate(const Case &c) {
    size_t p = 0;
    REQUIRE(c.n_launch >= 1 && c.max_rows >= 1 && c.max_rows <= 4096);
    REQUIRE(uint64_t(c.pic0) + c.n_launch <= c.pics.size());
    for (p = c.pic0; p < size_t(c.pic0) + c.n_launch; ++p) {
        const PicDesc &pd = c.pics[p];
        if (pd.flags & PD_ASSEMBLY) continue;
        REQUIRE(pd.seq < c.seqs.size());
        const SeqParams &sp = c.seqs[pd.seq];
        REQUIRE(sp.width > 0 && sp.height > 0 && sp.width <= 8192 && sp.height <= 8192);
        REQUIRE(sp.log2_ctb >= 4 && sp.log2_ctb <= 6);
        REQUIRE(sp.chroma_format >= 0 && sp.chroma_format <= 3);
        REQUIRE(sp.bit_depth_y >= 8 && sp.bit_depth_y <= 16 && sp.bit_depth_c >= 8 && sp.bit_depth_c <= 16);
        REQUIRE(uint64_t(sp.sf_off) + kSfBlockBytes <= c.sf.size());
        const uint64_t W = uint64_t(sp.width), H = uint64_t(sp.height);
        const uint64_t cw = sp.chroma_format ? W >> chroma_sx(sp.chroma_format) : 0;
        const uint64_t ch = sp.chroma_format ? H >> chroma_sy(sp.chroma_format) : 0;
        REQUIRE(pd.resid_off + W * H + 2 * cw * ch <= c.resid_elems);
        const uint64_t hctb = (H + (1u << sp.log2_ctb) - 1) >> sp.log2_ctb;
        const uint64_t rows = hctb < c.max_rows ? hctb : c.max_rows;
        REQUIRE(pd.coef_off % 4 == 0 && pd.coef_cap_row % 4 == 0 && pd.coef_cap_row < (1u << 23));
        for (uint64_t r = 0; r < rows; ++r) {
            REQUIRE(2 * (pd.row_off + r) + 1 < c.rows.size());
            const uint32_t ntu = c.rows[2 * (pd.row_off + r)];
            REQUIRE(ntu <= pd.tu_cap_row);
            REQUIRE(pd.tu_off + r * pd.tu_cap_row + ntu <= c.tus.size());
            REQUIRE(pd.coef_off + (r + 1) * pd.coef_cap_row <= c.coefs.size());
            const Coef *row = c.coefs.data() + pd.coef_off + r * pd.coef_cap_row;
            for (uint32_t t = 0; t < ntu; ++t) {
                const TuRec &tu = c.tus[pd.tu_off + r * pd.tu_cap_row + t];
                if (!(tu.flags & TU_CBF)) continue;
                REQUIRE(uint64_t(tu.coef) + tu.ncoef <= pd.coef_cap_row);
                if (tu.flags & TU_PCM) continue;
                REQUIRE(tu.coef % 4 == 0 && tu.ncoef % 4 == 0);
                for (uint32_t k = 0; k < tu.ncoef; k += 4) {  // the record's escapes: esc0, esc0 - 1, ...
                    const Coef *w = row + tu.coef + k;
                    const uint64_t x = uint64_t(w[1]) | (uint64_t(w[2]) << 32);
                    const int ne = __builtin_popcountll(x & (x >> 1) & (x >> 2) & (x >> 3) & 0x1111111111111111ull);
                    const uint32_t esc0 = w[3] >> 9;
                    REQUIRE(ne == 0 || (esc0 < pd.coef_cap_row && esc0 + 1 >= uint32_t(ne)));
                }
            }
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
    SZ(Coef);
#undef SZ
#undef OFF
    for (int s = 0; s < 4; ++s) printf("sf_size_offset.%d %u\n", s, sf_size_offset(s));
    printf("kSfBlockBytes %u\n", kSfBlockBytes);
    printf("SP_SCALING_LIST %u\n", unsigned(SP_SCALING_LIST));
    printf("PD_ASSEMBLY %u\n", unsigned(PD_ASSEMBLY));
    printf("TU_CIDX_MASK %u\nTU_CBF %u\nTU_TSKIP %u\nTU_BYPASS %u\nTU_DST %u\nTU_PCM %u\n", unsigned(TU_CIDX_MASK),
           unsigned(TU_CBF), unsigned(TU_TSKIP), unsigned(TU_BYPASS), unsigned(TU_DST), unsigned(TU_PCM));
    return 0;
}

#if !defined(HG_HOST_EMU)
#define CK(call)                                                                          \
    do {                                                                                  \
        const hipError_t e_ = (call);                                                     \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s: %s (%d)\n", #call, hipGetErrorString(e_), int(e_));      \
            exit(1); /* nothing further is launched */                                    \
        }                                                                                 \
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
        fprintf(stderr, "usage: %s --layout | case.bin resid.bin\n", argv[0]);
        return 2;
    }
    Case c;
    if (!load_case(argv[1], c)) {
        fprintf(stderr, "cannot read case file %s\n", argv[1]);
        return 2;
    }
    if (!validate(c)) return 3;
    std::vector<int16_t> resid(c.resid_elems, int16_t(uint16_t(c.sentinel)));
    BatchArgs a{};
    a.n_pics = int(c.n_launch);
    a.pic0 = int(c.pic0);
    a.max_rows = int(c.max_rows);
#if defined(HG_HOST_EMU)
    a.pics = c.pics.data();
    a.seqs = c.seqs.data();
    a.sf = c.sf.data();
    a.tus = c.tus.data();
    a.coefs = c.coefs.data();
    a.row_counts = c.rows.data();
    a.resid = resid.data();
    emu_transform(a);
#else
    a.pics = to_device(c.pics);
    a.seqs = to_device(c.seqs);
    a.sf = to_device(c.sf);
    a.tus = to_device(c.tus);
    a.coefs = to_device(c.coefs);
    a.row_counts = to_device(c.rows);
    a.resid = to_device(resid);
    CK(launch_transform(a, nullptr));
    CK(hipDeviceSynchronize());
    if (!resid.empty()) CK(hipMemcpy(resid.data(), a.resid, resid.size() * sizeof(int16_t), hipMemcpyDeviceToHost));
#endif
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(resid.data(), sizeof(int16_t), resid.size(), f) != resid.size() || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    printf("transform ok: %u pictures, %zu residual samples\n", c.n_launch, resid.size());
    return 0;
}
