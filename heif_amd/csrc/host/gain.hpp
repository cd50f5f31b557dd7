// gain.hpp — the gain map of an image item and the tables of the gain-map HDR render
// (include/heifgpu.h, "Gain-map HDR render").  Host only, no device code and nothing of the
// container reader: tests/gain/gain_driver.cpp links it with icc.cpp alone under ASan + UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/heifgpu.h"
#include "icc.hpp"

namespace hg {

// what parse_heic keeps of an item's gain map
struct GainDesc {
    uint32_t kind = 0;          // HEIFGPU_GAIN_*
    uint32_t item_id = 0;       // the gain-map image item
    std::vector<uint8_t> tmap;  // ISO: the 'tmap' item's data, kept unread (empty when it could not be fetched)
};

// what a 'tmap' payload says; headrooms, min and max are log2 values, channel 0 of a multichannel map
struct GainMeta {
    uint32_t version = 0, minimum_version = 0, writer_version = 0, multichannel = 0, use_base_colour_space = 0;
    double base_headroom = 0, alternate_headroom = 0, gain_min = 0, gain_max = 0, gamma = 0, base_offset = 0,
           alternate_offset = 0;
};

// HEIFGPU_OK, HEIFGPU_E_PARSE or HEIFGPU_E_UNSUPPORTED, why in err; out holds what was read
int gain_read(const uint8_t *p, size_t len, GainMeta &out, std::string &err);
// the transform of an item (its colour description, its gain map) whose map has depth gain_bits
int gain_transform_build(const GainDesc &g, const ColorDesc &color, uint32_t gain_bits, uint32_t dst, uint32_t bits,
                         uint32_t encoding, uint32_t pq_bits, double headroom, double display_headroom,
                         double sdr_white, heifgpu_gain_transform &out, std::string &err);
// whether a transform handed to heifgpu_gain_apply or a render keeps the reads inside the
// tables and the arithmetic inside its widths; else why not
const char *gain_transform_invalid(const heifgpu_gain_transform &t);

}  // namespace hg
