// batch.hpp — flattens parsed images into the device descriptor arrays of
// common/desc.hpp (shared by the HIP path and the host-emulation test build).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../common/desc.hpp"
#include "chroma.hpp"
#include "heic_image.hpp"

namespace hg {

struct HostBatch {
    std::vector<uint8_t> bits;  // every picture's payload, 64-byte aligned (+128 B tail), unless deferred
    // deferred bits (build_batch(..., defer_bits = true)): where each payload
    // goes in the bits arena, copied by the caller straight into its staging
    struct Piece {
        const uint8_t *src;
        size_t len, dst;
    };
    std::vector<Piece> pieces;
    size_t bits_size = 0;  // bytes of the bits arena
    std::vector<PicDesc> pics;
    std::vector<uint32_t> subs;
    std::vector<SeqParams> seqs;
    std::vector<uint8_t> sf;
    std::vector<uint32_t> pic_image;  // picture → image index
    uint64_t recon_bytes = 0, resid_elems = 0, map_bytes = 0, sao_n = 0, tu_n = 0, coef_n = 0;
    uint32_t rows = 0;
    int max_w = 0, max_wctb = 0, max_rows = 0, max_log2ctb = 4, bps = 0, chroma = -1;
    int lane_rows = 1, wpp_ring = 0;  // k_parse_lanes geometry (BatchArgs::lane_rows / wpp_ring)
    int max_wpp_rows = 0;             // CTB rows of the tallest WPP picture (k_parse_solo's context staging)
    bool has_assembly = false;        // some picture is a PD_ASSEMBLY (BatchArgs::has_assembly)
};

// A rectangle of samples; w == 0 && h == 0 stands for "everything".
struct Rect {
    uint32_t x = 0, y = 0, w = 0, h = 0;
    bool everything() const { return w == 0 && h == 0; }
};

// Window decode, exact integers, host only.
// rect_inside: r is "everything", or a non-empty rectangle inside W x H.
bool rect_inside(const Rect &r, uint32_t W, uint32_t H);
// The decoded samples of `im` that a render of `window` (displayed coordinates;
// "everything": the whole displayed picture) reads: the bounding box of the display
// map over the window's opposite corners, grown to the chroma sample grid and clipped
// to the image.  An image set to replicate chroma (the default) reads, for a luma
// sample, its own chroma sample: the box grows to whole chroma cells.  An image set to
// bilinear upsampling reads the two chroma columns floor((2x - px) / 4) and the next
// (clamped to the plane) and the two such rows: the box also covers the cells of the
// taps of its first and last luma column and row.  False if the window is not inside
// the displayed picture.
bool window_source_rect(const ParsedImage &im, const Rect &window, Rect &src);
// the chroma upsampling in force for an image: its setting, the caller's sample location
// or else its first SPS's (what the render calls and window_source_rect both read)
ChromaUp image_chroma_up(const ParsedImage &im);
// The grid tiles whose visible part meets src (rect_inside the image): columns
// [col0, col0 + cols), rows [row0, row0 + rows).
void tiles_for_rect(const ParsedImage &im, const Rect &src, uint32_t &col0, uint32_t &row0, uint32_t &cols,
                    uint32_t &rows);

// Throws HeifError / UnsupportedError.  Only grid tiles k (row-major) with
// k % tile_stride == tile_offset become pictures (the single-image tile split
// across GPUs); the default takes every tile.  rects (nullptr:
// everything) holds one rectangle per image in decoded-plane coordinates, each
// rect_inside its image: a picture (a grid tile; inside a coded picture each
// independent sub-picture; an assembly with all its children) is taken only if
// its visible rectangle in the output planes meets the image's rectangle.
HostBatch build_batch(const ParsedImage *const *imgs, size_t n, uint32_t tile_stride = 1, uint32_t tile_offset = 0,
                      bool defer_bits = false, const Rect *rects = nullptr);

}  // namespace hg
