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
    // the payloads of the item's first clli and mdcv boxes, kept unread (hdr_read)
    std::vector<uint8_t> clli, mdcv;
    bool has_clli = false, has_mdcv = false;
};

// what clli and mdcv say (include/heifgpu.h, "HDR render")
struct HdrMeta {
    uint32_t max_cll = 0, max_fall = 0;            // cd/m2
    uint32_t mastering_max = 0, mastering_min = 0;  // 0.0001 cd/m2
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


// ---- the tone stage of PQ / HLG sources (include/heifgpu.h, "HDR render") ----
// 16 or 18 when c is an nclx-defined PQ or HLG source (no profile), else 0
uint32_t hdr_transfer(const ColorDesc &c);
// HEIFGPU_OK, or HEIFGPU_E_PARSE for a box shorter than its fields (out holds what was read)
int hdr_read(const ColorDesc &c, HdrMeta &out, std::string &err);
// the source peak in cd/m2 by the rule of the header
double hdr_source_peak(uint32_t transfer, const HdrMeta &m, double peak_nits);
// BT.2390's EETF from a source peak lsrc to 203 cd/m2, cd/m2 in and out
double hdr_eetf(double x, double lsrc);
// the tone transform of an nclx source (primaries 1, 2, 9, 12; transfer 16, 18) at peak lsrc
int hdr_transform_build(uint32_t primaries, uint32_t transfer, double lsrc, uint32_t dst, uint32_t bits,
                        heifgpu_hdr_transform &out, std::string &err);
// color_transform_build, or for an nclx PQ / HLG source under tone_map hdr_transform_build
// at the peak the boxes and peak_nits give
int hdr_transform_make(const ColorDesc &c, uint32_t dst, uint32_t bits, uint32_t tone_map, double peak_nits,
                       heifgpu_hdr_transform &out, std::string &err);
// whether a transform handed to heifgpu_color_apply or a render keeps the kernels'
// reads inside the tables (in_lut32 below 2^22, w not negative and summing to 16384)
bool hdr_transform_valid(const heifgpu_hdr_transform &t);

}  // namespace hg
