// icc_driver.cpp — the host ICC reader (heif_amd/csrc/host/icc.cpp) over hostile
// profiles, as a stand-alone program built with ASan + UBSan (`make color-asan`;
// tests/test_color.py runs it).  Nothing here touches a device.
//
//   icc_driver PROFILE
//
// reads one matrix/TRC profile and answers, one line per case:
//   whole                      the profile as it is (must be OK)
//   trunc N                    its first N bytes, for every N below its size
//   field OFFSET VALUE         the 32-bit field at OFFSET (the size field, the tag
//                              count and every field of the tag table) set to 0,
//                              0xFFFFFFFF and size - 1
// Each case is a heap copy of exactly its own length, so a read past the end is an
// ASan report.  A profile that reads is also built into transforms to both
// destinations.  The answers are OK, E_PARSE or E_UNSUPPORTED; anything else is a bug.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "host/icc.hpp"

static const char *name_of(int rc) {
    switch (rc) {
    case HEIFGPU_OK: return "OK";
    case HEIFGPU_E_PARSE: return "E_PARSE";
    case HEIFGPU_E_UNSUPPORTED: return "E_UNSUPPORTED";
    default: return "OTHER";
    }
}

static int run(const std::vector<uint8_t> &bytes) {
    const std::vector<uint8_t> exact(bytes.begin(), bytes.end());  // capacity == size
    hg::ColorSource src;
    std::string err;
    int rc = hg::icc_read(exact.data(), exact.size(), src, err);
    if (rc != HEIFGPU_OK) return rc;
    static heifgpu_color_transform t;
    for (uint32_t dst = 0; dst < 2 && rc == HEIFGPU_OK; ++dst)
        for (uint32_t bits = 8; bits <= 12 && rc == HEIFGPU_OK; bits += 4) rc = hg::color_transform_build(src, dst, bits, t, err);
    return rc;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: icc_driver PROFILE\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> prof;
    for (int c; (c = std::fgetc(f)) != EOF;) prof.push_back(uint8_t(c));
    std::fclose(f);
    int bad = 0;
    auto report = [&](const std::string &what, int rc) {
        std::printf("%s %s\n", what.c_str(), name_of(rc));
        if (rc != HEIFGPU_OK && rc != HEIFGPU_E_PARSE && rc != HEIFGPU_E_UNSUPPORTED) ++bad;
    };
    const int whole = run(prof);
    report("whole", whole);
    if (whole != HEIFGPU_OK) ++bad;
    for (size_t n = 0; n < prof.size(); ++n)
        report("trunc " + std::to_string(n), run(std::vector<uint8_t>(prof.begin(), prof.begin() + long(n))));
    if (prof.size() >= 132) {
        const uint32_t count = (uint32_t(prof[128]) << 24) | (uint32_t(prof[129]) << 16) | (uint32_t(prof[130]) << 8) | prof[131];
        std::vector<size_t> fields = {0, 128};
        for (size_t k = 0; k < count && 132 + 12 * k + 12 <= prof.size(); ++k)
            for (size_t j = 0; j < 3; ++j) fields.push_back(132 + 12 * k + 4 * j);
        const uint32_t values[3] = {0u, 0xFFFFFFFFu, uint32_t(prof.size() - 1)};
        for (size_t off : fields)
            for (uint32_t v : values) {
                std::vector<uint8_t> p = prof;
                p[off] = uint8_t(v >> 24), p[off + 1] = uint8_t(v >> 16), p[off + 2] = uint8_t(v >> 8), p[off + 3] = uint8_t(v);
                report("field " + std::to_string(off) + " " + std::to_string(v), run(p));
            }
    }
    return bad ? 1 : 0;
}
