// display_asan — the display-geometry half of the host parser (clap / irot /
// imir folding, auxC alpha discovery) as a stand-alone program for the
// sanitizers (make -C heif_amd/csrc display-asan: ASan + UBSan, nothing loaded
// into Python).  It first runs display_clap on heap copies of exact length, so
// a read past a truncated box is a sanitizer report, then parses every file
// named on the command line and prints one line per file:
//   <path>: ok <W>x<H> n=<transforms> alpha=<item> prem=<0|1>
//   <path>: parse error: <message>
// Exit status 0 unless a built-in expectation fails (or a sanitizer aborts).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "host/heic_image.hpp"

using namespace hg;

namespace {

int g_failed = 0;

void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int s = 24; s >= 0; s -= 8) v.push_back(uint8_t(x >> s));
}

// display_clap over `len` bytes of the eight fields on a 48 x 32 image; returns true when it throws
bool clap_throws(const int64_t (&f)[8], size_t len, DisplayMap *out = nullptr) {
    std::vector<uint8_t> v;
    for (int64_t x : f) put32(v, uint32_t(x));
    std::unique_ptr<uint8_t[]> heap(new uint8_t[len ? len : 1]);  // exact length: ASan sees any over-read
    std::memcpy(heap.get(), v.data(), len);
    DisplayMap d;
    d.out_width = 48;
    d.out_height = 32;
    try {
        display_clap(d, heap.get(), len);
    } catch (const HeifError &) {
        return true;
    }
    if (out) *out = d;
    return false;
}

void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++g_failed;
    }
}

void builtin_checks() {
    const int64_t good[8] = {40, 1, 20, 1, -3, 1, -5, 1};
    DisplayMap d;
    expect(!clap_throws(good, 32, &d), "a valid clap is accepted");
    expect(d.out_width == 40 && d.out_height == 20 && d.t[0] == 1 && d.t[1] == 1, "clap 40x20 at (1, 1)");
    for (size_t len = 0; len < 32; ++len) expect(clap_throws(good, len), "a truncated clap is rejected");
    const int64_t bad[][8] = {
        {40, 0, 20, 1, 0, 1, 0, 1},                    // zero denominator
        {40, 1, 20, 1, 0, 1, 0, 0},
        {40, 1, 20, -1, 0, 1, 0, 1},                   // negative denominator
        {1, 4, 20, 1, 0, 1, 0, 1},                     // cw < 1
        {49, 1, 20, 1, 0, 1, 0, 1},                    // wider than the image
        {40, 1, 20, 1, 5, 1, 0, 1},                    // off the right edge
        {40, 1, 20, 1, 0, 1, -7, 1},                   // off the top
        {0xffffffffll, 1, 0xffffffffll, 1, 0x7fffffff, 1, -0x80000000ll, 1},  // extremes: no overflow in int64
        {2, 1, 2, 1, -0x80000000ll, 1, 0x7fffffff, 1},
        {2, 0x7fffffff, 2, 1, 0x7fffffff, 0x7fffffff, -0x80000000ll, 0x7fffffff},
    };
    for (const auto &f : bad) expect(clap_throws(f, 32), "an invalid clap is rejected");
    // every rotation and mirror of a map stays a signed permutation
    DisplayMap m;
    m.out_width = 48;
    m.out_height = 32;
    for (uint32_t k = 0; k < 16; ++k) {
        display_irot(m, k);
        display_imir(m, k >> 1);
        expect(m.m[0] * m.m[3] - m.m[1] * m.m[2] == 1 || m.m[0] * m.m[3] - m.m[1] * m.m[2] == -1, "unit determinant");
    }
    expect(m.n_transforms == 32, "one transform per box");
}

}  // namespace

int main(int argc, char **argv) {
    builtin_checks();
    for (int i = 1; i < argc; ++i) {
        std::ifstream in(argv[i], std::ios::binary);
        std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        std::unique_ptr<uint8_t[]> heap(new uint8_t[file.size() ? file.size() : 1]);
        std::memcpy(heap.get(), file.data(), file.size());
        try {
            const ParsedImage img = parse_heic(heap.get(), file.size());
            std::printf("%s: ok %ux%u n=%u alpha=%u prem=%u\n", argv[i], img.display.out_width, img.display.out_height,
                        img.display.n_transforms, img.alpha_item_id, img.alpha_premultiplied);
        } catch (const std::exception &e) {
            std::printf("%s: parse error: %s\n", argv[i], e.what());
        }
    }
    return g_failed ? 1 : 0;
}
