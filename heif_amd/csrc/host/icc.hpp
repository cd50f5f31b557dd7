// icc.hpp — the colour description of an image item and the tables of the
// colour-managed render (include/heifgpu.h, "colour-managed render").  Host only,
// no device code: tests/color/icc_driver.cpp links it alone under ASan + UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/heifgpu.h"

namespace hg {

// what parse_heic keeps of an item's colr boxes
struct ColorDesc {
    std::vector<uint8_t> icc;  // the 'prof' / 'rICC' payload (the first one), empty without
    bool has_icc = false, has_nclx = false;
    uint32_t primaries = 2, transfer = 2;  // of the nclx; 2 = unspecified
};

// a tone reproduction curve, code value in [0, 1] to linear light
struct Trc {
    enum Kind { IDENTITY, GAMMA, TABLE, PARA } kind = IDENTITY;
    int para_type = 0;
    double g = 1.0, a = 1.0, b = 0.0, c = 0.0, d = 0.0, e = 0.0, f = 0.0;
    std::vector<uint16_t> table;  // TABLE: at least two entries
    double eval(double x) const;  // not clamped
};

struct ColorSource {
    double col[9] = {};  // X Y Z of R, of G, of B (D50)
    Trc trc[3];
    bool nclx = false;   // from an nclx (or assumed sRGB), with these primaries:
    uint32_t primaries = 0;
};

// All return HEIFGPU_OK, HEIFGPU_E_PARSE or HEIFGPU_E_UNSUPPORTED and say why in err.
int icc_read(const uint8_t *p, size_t len, ColorSource &out, std::string &err);
int nclx_source(uint32_t primaries, uint32_t transfer, ColorSource &out, std::string &err);
int color_source(const ColorDesc &c, ColorSource &out, std::string &err);
// dst: HEIFGPU_CS_*; bits 8..12
int color_transform_build(const ColorSource &src, uint32_t dst, uint32_t bits, heifgpu_color_transform &out,
                          std::string &err);

}  // namespace hg
