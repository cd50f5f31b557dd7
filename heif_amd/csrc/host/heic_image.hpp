// heic_image.hpp — host half of HeicDecoder::decode (src/heic/decoder.rs:12-112).
#pragma once
#include <cstdint>
#include <vector>

#include "gain.hpp"
#include "heif_reader.hpp"
#include "hevc_ps.hpp"
#include "icc.hpp"

namespace hg {

struct ParamSet {
    std::vector<uint8_t> key;  // raw SPS ++ PPS NAL bytes (dedupe key)
    VideoParameterSet vps;
    SequenceParameterSet sps;
    PictureParameterSet pps;
    std::vector<int> col_bd, row_bd;  // HEVC tile boundaries in CTBs (one tile without tiles)
};

struct SliceSeg {
    // raw NAL payload after the 2-byte header (EP bytes kept): a view into ParsedImage::coded
    const uint8_t *payload = nullptr;
    size_t payload_len = 0;
    NalUnitHeader nal;
    SliceSegmentHeader sh;
};

struct TileJob {
    std::vector<SliceSeg> segs;  // the coded picture's slice segments in decoding order (one or more)
    int param = 0;
};

// Output pixel (ox, oy) of the displayed image shows decoded sample
// (m[0]*ox + m[1]*oy + t[0], m[2]*ox + m[3]*oy + t[1]); m is a signed permutation matrix.
struct DisplayMap {
    uint32_t out_width = 0, out_height = 0;
    int32_t m[4] = {1, 0, 0, 1}, t[2] = {0, 0};
    uint32_t n_transforms = 0;
};
// The three transformative item properties as steps of a DisplayMap that starts as
// the identity over the decoded W x H image (ISO/IEC 23008-12 6.5.9 / .10 / .12).
// The conventions, in this one place ("parity unpinned": neither the reference nor
// anything else at hand renders them):
//   clap: img[top:top+ch, left:left+cw]; payload = 8 x 32-bit (width N/D, height N/D,
//         horizOff N/D, vertOff N/D; offsets signed), sizes and offsets rounded half up
//   irot: np.rot90(img, k), anticlockwise
//   imir: axis 0 = vertical axis, img[:, ::-1]; axis 1 = horizontal axis, img[::-1, :]
void display_clap(DisplayMap &d, const uint8_t *payload, size_t len);  // throws HeifError
void display_irot(DisplayMap &d, uint32_t quarter_turns);
void display_imir(DisplayMap &d, uint32_t axis);
// the window img[y:y+h, x:x+w] of the displayed picture as one more step, a clap given
// directly (heifgpu_render_batch_scaled; the caller has checked that it lies inside)
void display_window(DisplayMap &d, uint32_t x, uint32_t y, uint32_t w, uint32_t h);

struct ParsedImage {
    // move-only: the tiles' payload views point into `coded`, whose buffer a move keeps
    ParsedImage() = default;
    ParsedImage(const ParsedImage &) = delete;
    ParsedImage &operator=(const ParsedImage &) = delete;
    ParsedImage(ParsedImage &&) = default;
    ParsedImage &operator=(ParsedImage &&) = default;
    std::vector<uint8_t> coded;  // the coded items' bytes, one copy (TileJob payloads point into it)
    std::vector<ParamSet> params;
    std::vector<TileJob> tiles;  // grid order (row-major)
    uint32_t primary_item_id = 0, ispe_width = 0, ispe_height = 0, rotation = 0, num_thumbnails = 0;
    uint32_t item_id = 0;      // the decoded image item (the primary unless asked otherwise)
    uint32_t aux_item_id = 0;  // first auxiliary image of the primary ('auxl'), 0 if none
    bool nclx = false;         // the item has an nclx colr (overrides the VUI colour description)
    uint32_t nclx_matrix = 0, nclx_full_range = 0;
    // every colr of the item: the profile's bytes, the nclx primaries and transfer (icc.hpp);
    // nothing is read out of the profile here, a file with an odd one parses and decodes
    ColorDesc color;
    uint32_t rows = 1, cols = 1, out_width = 0, out_height = 0;
    uint32_t tile_width = 0, tile_height = 0, coded_bytes = 0;
    // the item's transformative properties (clap / irot / imir) in ipma order, folded
    DisplayMap display;
    // first 'auxl' image of the decoded item whose auxC names an alpha plane (0: none);
    // a 'prem' reference from the item to it is reported, nothing is un-premultiplied
    uint32_t alpha_item_id = 0, alpha_premultiplied = 0;
    // how the renders turn subsampled chroma into the luma grid (host/chroma.hpp): replicate
    // (0) or bilinear (1), and the caller's sample location in place of the SPS's (-1: the file's).
    // Set by heifgpu_image_set_chroma_upsampling; read by the render calls and by window_source_rect.
    uint32_t chroma_mode = 0;
    int32_t chroma_loc_override = -1;
    // the item's gain map (gain.hpp): the 'tmap' item that names it as its base, its data kept
    // unread, else the first 'auxl' image whose auxC is Apple's gain-map URN
    GainDesc gain;
};

// Throws HeifError (parse) or UnsupportedError (valid stream, tool outside this path).
// item_id 0 = the primary item (heic/decoder.rs:12-112); otherwise any coded
// image item, e.g. an auxiliary image found through ParsedImage::aux_item_id
ParsedImage parse_heic(const uint8_t *data, size_t len, uint32_t item_id = 0);

}  // namespace hg
