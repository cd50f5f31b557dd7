// png_driver.cpp — TEST-ONLY driver of the PNG kernels alone under the host emulation
// (tests/test_png.py; make png-emu: g++ -DHG_HOST_EMU with kernels/png.hip, under ASan + UBSan).
//
// Reads a case file of batches, plans each batch as heifgpu_png_encode_batch does (png_plan),
// runs the four kernels through hg::emu_png_encode and writes what they left.
//   png_driver case.bin result.bin
// Case file (little endian): magic, n_batches, then per batch 8 uint32
//   n pictures, format, bits, filter, sentinel byte, 0 x 3
// then per picture 6 uint32 (width, height, pitch, lead, buffer bytes, capacity) and the
// buffer: the first pixel lies `lead` bytes into it (an odd lead: a surface at an odd
// address).  Every heap block has exactly the size the case or the plan states, so a read
// outside a picture's buffer or the scratch, or a write at or past a capacity, is an ASan report.
// The result file holds, per picture, the size word (uint64) and the `capacity` output bytes,
// which were filled with the sentinel.  Everything the kernels will index is checked first.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels/png.hpp"

namespace hg {
thread_local EmuCtx g_emu;
}
using namespace hg;

namespace {

constexpr uint32_t kMagic = 0x31474e50u;  // "PNG1"

struct Pic {
    uint32_t w, h, pitch, lead, cap;
    std::vector<uint8_t> buf;
};
struct Batch {
    uint32_t format, bits, filter, sentinel;
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

// what heifgpu_png_encode_batch refuses, and the picture inside its buffer
bool validate(const Batch &b) {
    REQUIRE(b.format <= 3 && b.filter <= 5 && b.sentinel <= 255);
    REQUIRE(b.format < 2 ? b.bits == 8 : (b.bits >= 8 && b.bits <= 16));
    const uint32_t bpp = uint32_t(png_bpp(int(b.format)));
    for (const Pic &p : b.pics) {
        REQUIRE(p.w >= 1 && p.h >= 1 && p.w <= 4096 && p.h <= 4096);
        REQUIRE(p.pitch >= bpp * p.w && p.pitch <= (1u << 20));
        REQUIRE(uint64_t(p.lead) + uint64_t(p.h - 1) * p.pitch + bpp * uint64_t(p.w) <= p.buf.size());
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
        std::vector<PngPic> pics(n);
        std::vector<uint64_t> sizes(n, 0x0101010101010101ull * b.sentinel);
        for (size_t i = 0; i < n; ++i) {
            outs[i].assign(b.pics[i].cap, uint8_t(b.sentinel));
            PngPic &p = pics[i];
            p = PngPic{};
            p.px = b.pics[i].buf.data() + b.pics[i].lead;
            p.out = outs[i].data();
            p.pitch = b.pics[i].pitch;
            p.cap = b.pics[i].cap;
            p.w = b.pics[i].w, p.h = b.pics[i].h;
        }
        uint64_t n_stream, n_blk;
        uint32_t max_h, max_blk;
        png_plan(pics.data(), int(n), int(b.format), n_stream, n_blk, max_h, max_blk);
        std::vector<PngQuad> stream(n_stream / 16);  // (16-byte aligned, as the device's is)
        std::vector<PngBlk> blk(n_blk);
        std::vector<uint64_t> boff(n_blk);
        std::vector<uint32_t> adler(n);
        PngArgs a{};
        a.pics = pics.data();
        a.stream = reinterpret_cast<uint8_t *>(stream.data());
        a.blk = blk.data();
        a.boff = boff.data();
        a.adler = adler.data();
        a.sizes = sizes.data();
        a.n = int(n);
        a.fmt = int(b.format);
        a.bits = int(b.bits);
        a.filter = int(b.filter);
        emu_png_encode(a, max_h, max_blk);
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
    printf("png ok: %zu batches\n", bs.size());
    return 0;
}
