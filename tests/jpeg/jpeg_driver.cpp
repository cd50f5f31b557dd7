// jpeg_driver.cpp — TEST-ONLY driver of the JPEG kernels alone under the host emulation
// (tests/test_jpeg.py; make jpeg-emu: g++ -DHG_HOST_EMU with kernels/jpeg.hip, under ASan + UBSan).
//
// Reads a case file of batches, plans each batch as heifgpu_jpeg_encode_batch does (jpeg_plan),
// runs the four kernels through hg::emu_jpeg_encode and writes what they left.
//   jpeg_driver case.bin result.bin
// Case file (little endian): magic, n_batches, then per batch 8 uint32
//   n pictures, quality, subsampling, restart_mcus, sentinel byte, 0 x 3
// then per picture 6 uint32 (width, height, pitch, lead, buffer bytes, capacity) and the
// buffer: the first pixel lies `lead` bytes into it (an odd lead: a surface at an odd
// address).  Every heap block has exactly the size the case states, so a read outside a
// picture's buffer or a write at or past a capacity is an ASan report.  The result file
// holds, per picture, the size word (uint64) and the `capacity` output bytes, which were
// filled with the sentinel.  Everything the kernels will index is checked first.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels/jpeg.hpp"

namespace hg {
thread_local EmuCtx g_emu;
}
using namespace hg;

namespace {

constexpr uint32_t kMagic = 0x3147504au;  // "JPG1"

struct Pic {
    uint32_t w, h, pitch, lead, cap;
    std::vector<uint8_t> buf;
};
struct Batch {
    uint32_t quality, sub, restart, sentinel;
    std::vector<Pic> pics;
};

bool load_case(const char *path, std::vector<Batch> &bs) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint32_t top[2];
    bool ok = fread(top, 4, 2, f) == 2 && top[0] == kMagic && top[1] >= 1 && top[1] <= 4096;
    for (uint32_t i = 0; ok && i < top[1]; ++i) {
        uint32_t h[8];
        ok = fread(h, 4, 8, f) == 8 && h[0] >= 1 && h[0] <= 64;
        if (!ok) break;
        Batch b{h[1], h[2], h[3], h[4], {}};
        for (uint32_t k = 0; ok && k < h[0]; ++k) {
            uint32_t q[6];
            ok = fread(q, 4, 6, f) == 6 && q[4] <= (1u << 24) && q[5] <= (1u << 24);
            if (!ok) break;
            Pic p{q[0], q[1], q[2], q[3], q[5], {}};
            p.buf.resize(q[4]);
            ok = q[4] == 0 || fread(p.buf.data(), 1, q[4], f) == q[4];
            b.pics.push_back(std::move(p));
        }
        bs.push_back(std::move(b));
    }
    fclose(f);
    return ok;
}

#define REQUIRE(cond)                                         \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "case rejected: %s\n", #cond);    \
            return false;                                     \
        }                                                     \
    } while (0)

// what heifgpu_jpeg_encode_batch refuses, and the picture inside its buffer
bool validate(const Batch &b) {
    REQUIRE(b.quality >= 1 && b.quality <= 100 && b.sub <= 1 && b.restart <= 65535 && b.sentinel <= 255);
    for (const Pic &p : b.pics) {
        REQUIRE(p.w >= 1 && p.h >= 1 && p.w <= 4096 && p.h <= 4096);
        REQUIRE(p.pitch >= 3 * p.w && p.pitch <= (1u << 20));
        REQUIRE(uint64_t(p.lead) + uint64_t(p.h - 1) * p.pitch + 3 * uint64_t(p.w) <= p.buf.size());
    }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s case.bin result.bin\n", argv[0]);
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
        const size_t n = b.pics.size();
        std::vector<std::vector<uint8_t>> outs(n);
        std::vector<JpegPic> pics(n);
        std::vector<uint64_t> sizes(n, 0x0101010101010101ull * b.sentinel);
        for (size_t i = 0; i < n; ++i) {
            outs[i].assign(b.pics[i].cap, uint8_t(b.sentinel));
            JpegPic &p = pics[i];
            p = JpegPic{};
            p.rgb = b.pics[i].buf.data() + b.pics[i].lead;
            p.out = outs[i].data();
            p.pitch = b.pics[i].pitch;
            p.cap = b.pics[i].cap;
            p.w = b.pics[i].w, p.h = b.pics[i].h;
        }
        uint64_t n_coef, n_int;
        uint32_t max_groups, max_int;
        jpeg_plan(pics.data(), int(n), int(b.sub), b.restart, n_coef, n_int, max_groups, max_int);
        std::vector<int16_t> coef(n_coef);
        std::vector<uint32_t> ilen(n_int);
        std::vector<uint64_t> ioff(n_int);
        JpegArgs a{};
        a.pics = pics.data();
        a.coef = coef.data();
        a.ilen = ilen.data();
        a.ioff = ioff.data();
        a.sizes = sizes.data();
        a.n = int(n);
        a.sub = int(b.sub);
        for (int t = 0; t < 2; ++t)
            for (int k = 0; k < 64; ++k) a.qt[t][k] = jpeg_quant_scale(kJpegBaseQ[t][k], int(b.quality));
        emu_jpeg_encode(a, max_groups, max_int);
        for (size_t i = 0; i < n; ++i) {
            bool ok = fwrite(&sizes[i], 8, 1, f) == 1;
            ok = ok && (outs[i].empty() || fwrite(outs[i].data(), 1, outs[i].size(), f) == outs[i].size());
            if (!ok) {
                fprintf(stderr, "cannot write %s\n", argv[2]);
                return 2;
            }
        }
    }
    if (fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    printf("jpeg ok: %zu batches\n", bs.size());
    return 0;
}
