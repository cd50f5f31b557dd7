// image.cpp — the host-only calls of the C ABI: the error message, the HEIC parse, what a
// parsed image tells (info, display map, colour, ICC, window geometry, tile parameters),
// the colour transform on the host, and the test hooks of the host bit readers.
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

#include "../common/desc.hpp"
#include "../host/icc.hpp"
#include "../kernels/cabac.hpp"
#include "../kernels/color_xform.hpp"
#include "api.hpp"

using namespace hg;

// the C structs' layouts are part of the ABI (INTEGRATION.md's Rust binding mirrors them)
static_assert(sizeof(heifgpu_image_info) == 80, "heifgpu_image_info: 20 x uint32");
static_assert(sizeof(heifgpu_planes) == 40, "heifgpu_planes: 3 pointers + 3 int32 (+ padding)");
static_assert(sizeof(heifgpu_batch_opts) == 20, "heifgpu_batch_opts: 5 x uint32");
static_assert(sizeof(heifgpu_display_info) == 44, "heifgpu_display_info: 11 x 32 bits");
static_assert(sizeof(heifgpu_surface) == 16, "heifgpu_surface: pointer + int32 (+ padding)");
static_assert(sizeof(heifgpu_rect) == 16, "heifgpu_rect: 4 x uint32");
static_assert(HEIFGPU_PIX_RGB8 == RENDER_RGB8 && HEIFGPU_PIX_RGBA8 == RENDER_RGBA8 && HEIFGPU_PIX_RGB16 == RENDER_RGB16 &&
                  HEIFGPU_PIX_RGBA16 == RENDER_RGBA16,
              "pixel formats");
static_assert(sizeof(heifgpu_ipc_handle) == 72, "heifgpu_ipc_handle: 64-byte HIP handle + uint64 offset");
static_assert(HEIFGPU_PARSE_AUTO == PARSE_AUTO && HEIFGPU_PARSE_LANES == PARSE_LANES && HEIFGPU_PARSE_SOLO == PARSE_SOLO &&
                  HEIFGPU_PARSE_SPREAD == PARSE_SPREAD,
              "parse modes");
static_assert(sizeof(heifgpu_tile_params) == 55 * 4 + 64 * 4, "heifgpu_tile_params: 55 int32 + 64 uint32");

thread_local std::string hg::g_err;

extern "C" {

const char *heifgpu_last_error(void) { return g_err.c_str(); }

int heifgpu_image_parse(const uint8_t *data, size_t len, heifgpu_image **out) {
    return heifgpu_image_parse_item(data, len, 0, out);
}

int heifgpu_image_parse_item(const uint8_t *data, size_t len, uint32_t item_id, heifgpu_image **out) {
    if (!data || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    *out = nullptr;
    try {
        auto im = std::make_unique<heifgpu_image>();
        im->img = parse_heic(data, len, item_id);
        *out = im.release();
        return HEIFGPU_OK;
    } catch (const UnsupportedError &e) {
        return fail(HEIFGPU_E_UNSUPPORTED, e.what());
    } catch (const std::exception &e) {
        return fail(HEIFGPU_E_PARSE, e.what());
    }
}

int heifgpu_image_parse_many(const uint8_t *const *data, const size_t *len, size_t n, int threads,
                             heifgpu_image **out, int *rc) {
    if (!data || !len || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    for (size_t i = 0; i < n; ++i) out[i] = nullptr;
    std::vector<int> codes(n, HEIFGPU_OK);
    std::vector<std::string> msgs(n);
    std::atomic<size_t> next{0};
    auto worker = [&] {
        for (size_t i; (i = next.fetch_add(1)) < n;) {
            if (!data[i]) {
                codes[i] = HEIFGPU_E_INVALID;
                msgs[i] = "null data";
                continue;
            }
            try {
                auto im = std::make_unique<heifgpu_image>();
                im->img = parse_heic(data[i], len[i], 0);
                out[i] = im.release();
            } catch (const UnsupportedError &e) {
                codes[i] = HEIFGPU_E_UNSUPPORTED;
                msgs[i] = e.what();
            } catch (const std::exception &e) {
                codes[i] = HEIFGPU_E_PARSE;
                msgs[i] = e.what();
            }
        }
    };
    size_t nt = threads > 0 ? size_t(threads) : size_t(std::max(1u, std::thread::hardware_concurrency()));
    nt = std::min(nt, n);
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; ++t) pool.emplace_back(worker);
    worker();
    for (auto &th : pool) th.join();
    int first = HEIFGPU_OK;
    for (size_t i = 0; i < n; ++i) {
        if (rc) rc[i] = codes[i];
        if (codes[i] != HEIFGPU_OK && first == HEIFGPU_OK) {
            first = codes[i];
            g_err = "image " + std::to_string(i) + ": " + msgs[i];
        }
    }
    return first;
}

int heifgpu_image_get_info(const heifgpu_image *img, heifgpu_image_info *info) {
    if (!img || !info) return fail(HEIFGPU_E_INVALID, "null argument");
    const ParsedImage &p = img->img;
    const SequenceParameterSet &s = p.params[0].sps;
    std::memset(info, 0, sizeof(*info));
    info->width = p.out_width;
    info->height = p.out_height;
    info->chroma_format_idc = uint32_t(s.chroma_array_type());
    info->bit_depth = uint32_t(8 + s.bit_depth_luma_minus8);
    info->bytes_per_sample = info->bit_depth > 8 ? 2 : 1;
    info->grid_rows = p.rows;
    info->grid_cols = p.cols;
    info->tile_width = p.tile_width;
    info->tile_height = p.tile_height;
    info->num_tiles = uint32_t(p.tiles.size());
    info->rotation = p.rotation;
    info->ispe_width = p.ispe_width;
    info->ispe_height = p.ispe_height;
    info->coded_bytes = p.coded_bytes;
    info->primary_item_id = p.primary_item_id;
    info->num_thumbnails = p.num_thumbnails;
    info->matrix_coeffs = p.nclx ? p.nclx_matrix : uint32_t(s.matrix_coeffs);
    info->full_range = p.nclx ? p.nclx_full_range : (s.video_full_range_flag ? 1u : 0u);
    info->item_id = p.item_id;
    info->aux_item_id = p.aux_item_id;
    return HEIFGPU_OK;
}

int heifgpu_image_get_display(const heifgpu_image *img, heifgpu_display_info *out) {
    if (!img || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    const ParsedImage &p = img->img;
    std::memset(out, 0, sizeof(*out));
    out->out_width = p.display.out_width;
    out->out_height = p.display.out_height;
    for (int k = 0; k < 4; ++k) out->m[k] = p.display.m[k];
    out->t[0] = p.display.t[0];
    out->t[1] = p.display.t[1];
    out->n_transforms = p.display.n_transforms;
    out->alpha_item_id = p.alpha_item_id;
    out->alpha_premultiplied = p.alpha_premultiplied;
    return HEIFGPU_OK;
}

// ---- colour-managed render (include/heifgpu.h): description, transform, tables --
int heifgpu_image_get_color(const heifgpu_image *img, heifgpu_color_info *out) {
    if (!img || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    const ColorDesc &c = img->img.color;
    std::memset(out, 0, sizeof(*out));
    out->kind = c.has_icc ? HEIFGPU_COLOR_ICC : c.has_nclx ? HEIFGPU_COLOR_NCLX : HEIFGPU_COLOR_NONE;
    out->has_nclx = c.has_nclx;
    out->primaries = c.primaries;
    out->transfer = c.transfer;
    out->icc_size = uint32_t(c.icc.size());
    ColorSource src;
    std::string err;
    out->status = color_source(c, src, err);
    if (out->status == HEIFGPU_OK)
        for (int k = 0; k < 9; ++k) out->colorants[k] = src.col[k];
    return HEIFGPU_OK;
}

int heifgpu_image_get_icc(const heifgpu_image *img, uint8_t *buf, size_t cap, size_t *len) {
    if (!img || !len) return fail(HEIFGPU_E_INVALID, "null argument");
    const std::vector<uint8_t> &icc = img->img.color.icc;
    *len = icc.size();
    if (buf && cap >= icc.size() && !icc.empty()) std::memcpy(buf, icc.data(), icc.size());
    return HEIFGPU_OK;
}

int heifgpu_color_transform_make(const heifgpu_image *img, uint32_t dst, uint32_t bits, heifgpu_color_transform *out) {
    if (!img || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    ColorSource src;
    std::string err;
    if (int rc = color_source(img->img.color, src, err)) return fail(rc, err);
    if (int rc = color_transform_build(src, dst, bits, *out, err)) return fail(rc, err);
    return HEIFGPU_OK;
}

int heifgpu_image_get_hdr(const heifgpu_image *img, heifgpu_hdr_info *out) {
    if (!img || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    const ColorDesc &c = img->img.color;
    std::memset(out, 0, sizeof(*out));
    out->transfer = hdr_transfer(c);
    out->present = (c.has_clli ? HEIFGPU_HDR_HAS_CLLI : 0u) | (c.has_mdcv ? HEIFGPU_HDR_HAS_MDCV : 0u);
    HdrMeta m;
    std::string err;
    out->status = hdr_read(c, m, err);
    out->max_cll = m.max_cll, out->max_fall = m.max_fall;
    out->mastering_max = m.mastering_max, out->mastering_min = m.mastering_min;
    return HEIFGPU_OK;
}

int heifgpu_color_transform_make_hdr(const heifgpu_image *img, uint32_t dst, uint32_t bits, uint32_t tone_map,
                                     double peak_nits, heifgpu_hdr_transform *out) {
    if (!img || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    std::string err;
    if (int rc = hdr_transform_make(img->img.color, dst, bits, tone_map, peak_nits, *out, err)) return fail(rc, err);
    return HEIFGPU_OK;
}

// heifgpu_color_apply for a tone transform (t->base.tone != 0)
static int tone_apply(const heifgpu_hdr_transform *t, const uint16_t *rgb_in, size_t n_pixels, uint16_t *rgb_out) {
    if (t->base.tone != HEIFGPU_TONE_BT2390 || !hdr_transform_valid(*t))
        return fail(HEIFGPU_E_INVALID, "tone transform: tag, depth, weights or a level above 2^22 - 1");
    const int n = 1 << t->base.bits;
    std::vector<uint32_t> in_lut(size_t(3) * n);
    for (int c = 0; c < 3; ++c) std::memcpy(in_lut.data() + size_t(c) * n, t->in_lut32[c], size_t(n) * 4);
    for (size_t i = 0; i < 3 * n_pixels; ++i)
        if (rgb_in[i] >= n) return fail(HEIFGPU_E_INVALID, "code above maxv");
    const uint32_t *in = in_lut.data();
    const XfToneLut<const uint32_t *> tone{t->T};
    const XfOutLut<const uint16_t *> out{t->base.out_lut};
    for (size_t i = 0; i < n_pixels; ++i) {
        uint32_t r = rgb_in[3 * i], g = rgb_in[3 * i + 1], b = rgb_in[3 * i + 2];
        color_tone_px(in, n, t->w, tone, out, t->base.m, r, g, b);
        rgb_out[3 * i] = uint16_t(r), rgb_out[3 * i + 1] = uint16_t(g), rgb_out[3 * i + 2] = uint16_t(b);
    }
    return HEIFGPU_OK;
}

int heifgpu_color_apply(const heifgpu_color_transform *t, const uint16_t *rgb_in, size_t n_pixels, uint16_t *rgb_out) {
    if (!t || !rgb_in || !rgb_out) return fail(HEIFGPU_E_INVALID, "null argument");
    if (t->tone) return tone_apply(reinterpret_cast<const heifgpu_hdr_transform *>(t), rgb_in, n_pixels, rgb_out);
    if (t->bits < 8 || t->bits > 12) return fail(HEIFGPU_E_INVALID, "transform depth outside 8..12");
    const int n = 1 << t->bits;
    // the tables as the device holds them: three of n entries, one after the other
    std::vector<uint16_t> in_lut(size_t(3) * n);
    for (int c = 0; c < 3; ++c) std::memcpy(in_lut.data() + size_t(c) * n, t->in_lut[c], size_t(n) * 2);
    for (size_t i = 0; i < 3 * n_pixels; ++i)
        if (rgb_in[i] >= n) return fail(HEIFGPU_E_INVALID, "code above maxv");
    const uint16_t *in = in_lut.data();
    const XfOutLut<const uint16_t *> out{t->out_lut};
    for (size_t i = 0; i < n_pixels; ++i) {
        uint32_t r = rgb_in[3 * i], g = rgb_in[3 * i + 1], b = rgb_in[3 * i + 2];
        color_xform_px(in, n, out, t->m, r, g, b);
        rgb_out[3 * i] = uint16_t(r), rgb_out[3 * i + 1] = uint16_t(g), rgb_out[3 * i + 2] = uint16_t(b);
    }
    return HEIFGPU_OK;
}

// The linear-light scaled render's contract on the host (include/heifgpu.h "Linear-light scaled
// render"), through the functions the kernel calls: color_linear_level per sample, the separable
// sum in the kernel's order (a line's column sums, then the row of outputs), color_linear_mean,
// color_linear_encode.  A fourth channel is averaged as codes.
int heifgpu_linear_average_apply(const heifgpu_color_transform *t, const uint16_t *rgb_in, uint32_t in_width,
                                 uint32_t in_height, uint32_t channels, const heifgpu_rect *window, uint32_t out_width,
                                 uint32_t out_height, uint16_t *rgb_out) {
    if (!t || !rgb_in || !rgb_out) return fail(HEIFGPU_E_INVALID, "null argument");
    if (t->tone) return fail(HEIFGPU_E_UNSUPPORTED, "linear-light average of a tone transform");
    if (t->bits < 8 || t->bits > 12) return fail(HEIFGPU_E_INVALID, "transform depth outside 8..12");
    if (channels != 3 && channels != 4) return fail(HEIFGPU_E_INVALID, "channels other than 3 or 4");
    heifgpu_rect w{0, 0, in_width, in_height};
    if (window && (window->width || window->height)) w = *window;
    if (!w.width || !w.height || w.x >= in_width || w.y >= in_height || w.width > in_width - w.x ||
        w.height > in_height - w.y)
        return fail(HEIFGPU_E_INVALID, "window empty or outside the picture");
    if (w.width > 65535 || w.height > 65535) return fail(HEIFGPU_E_UNSUPPORTED, "window side above 65535");
    if (!out_width || !out_height || out_width > 65535 || out_height > 65535)
        return fail(HEIFGPU_E_INVALID, "rendered size outside 1..65535");
    const int n = 1 << t->bits;
    const size_t count = size_t(in_width) * in_height * channels;
    for (size_t k = 0; k < count; ++k)
        if (rgb_in[k] >= n) return fail(HEIFGPU_E_INVALID, "code above maxv");
    std::vector<uint16_t> in_lut(size_t(3) * n);
    for (int c = 0; c < 3; ++c) std::memcpy(in_lut.data() + size_t(c) * n, t->in_lut[c], size_t(n) * 2);
    const uint16_t *in = in_lut.data();
    const XfOutLut<const uint16_t *> out{t->out_lut};
    const uint64_t cw = w.width, ch = w.height, ow = out_width, oh = out_height;
    std::vector<uint64_t> col(size_t(cw) * channels);  // a line's column sums: at most 65535 * 65535 each
    for (uint64_t Y = 0; Y < oh; ++Y) {
        const uint64_t alo = Y * ch, ahi = alo + ch;
        std::fill(col.begin(), col.end(), 0);
        for (uint64_t j = alo / oh; j < (ahi + oh - 1) / oh; ++j) {
            const uint64_t wy = std::min((j + 1) * oh, ahi) - std::max(j * oh, alo);
            const uint16_t *row = rgb_in + (size_t(w.y + j) * in_width + w.x) * channels;
            for (uint64_t i = 0; i < cw; ++i)
                for (uint32_t c = 0; c < channels; ++c) {
                    const uint32_t code = row[i * channels + c];
                    col[i * channels + c] += wy * (c < 3 ? color_linear_level(in, n, int(c), code) : code);
                }
        }
        for (uint64_t X = 0; X < ow; ++X) {
            const uint64_t blo = X * cw, bhi = blo + cw;
            uint64_t S[4] = {0, 0, 0, 0};  // below 2^48
            for (uint64_t i = blo / ow; i < (bhi + ow - 1) / ow; ++i) {
                const uint64_t wx = std::min((i + 1) * ow, bhi) - std::max(i * ow, blo);
                for (uint32_t c = 0; c < channels; ++c) S[c] += wx * col[i * channels + c];
            }
            uint16_t *o = rgb_out + (size_t(Y) * out_width + X) * channels;
            uint32_t r, g, b;
            color_linear_encode(out, t->m, color_linear_mean(S[0], cw * ch), color_linear_mean(S[1], cw * ch),
                                color_linear_mean(S[2], cw * ch), r, g, b);
            o[0] = uint16_t(r), o[1] = uint16_t(g), o[2] = uint16_t(b);
            if (channels == 4) o[3] = uint16_t(color_linear_mean(S[3], cw * ch));
        }
    }
    return HEIFGPU_OK;
}

// ---- chroma upsampling (include/heifgpu.h): the signalled location, the setting, the rule ----
int heifgpu_image_get_chroma(const heifgpu_image *img, heifgpu_chroma_info *out) {
    if (!img || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    const ParsedImage &p = img->img;
    const SequenceParameterSet &s = p.params[0].sps;
    std::memset(out, 0, sizeof(*out));
    out->loc = uint32_t(s.chroma_loc_top);
    out->signalled = s.chroma_loc_present ? 1 : 0;
    out->loc_override = p.chroma_loc_override;
    out->mode = p.chroma_mode;
    out->sub_width_c = 1u << chroma_sx(s.chroma_array_type());
    out->sub_height_c = 1u << chroma_sy(s.chroma_array_type());
    return HEIFGPU_OK;
}

int heifgpu_image_set_chroma_upsampling(heifgpu_image *img, uint32_t mode, int32_t loc) {
    if (!img) return fail(HEIFGPU_E_INVALID, "null argument");
    if (mode > HEIFGPU_CHROMA_BILINEAR) return fail(HEIFGPU_E_INVALID, "chroma upsampling mode");
    if (loc < -1 || loc > 5) return fail(HEIFGPU_E_INVALID, "chroma sample location outside -1..5");
    img->img.chroma_mode = mode;
    img->img.chroma_loc_override = loc;
    return HEIFGPU_OK;
}

int heifgpu_chroma_upsample(const void *in, uint32_t w_c, uint32_t h_c, int32_t pitch, uint32_t bits,
                            uint32_t chroma_format_idc, uint32_t loc, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                            void *out, int32_t out_pitch) {
    if (const char *err = chroma_upsample_rect(in, w_c, h_c, pitch, bits, chroma_format_idc, loc, x0, y0, w, h, out, out_pitch))
        return fail(HEIFGPU_E_INVALID, err);
    return HEIFGPU_OK;
}

void heifgpu_image_free(heifgpu_image *img) { delete img; }

// ---- window decode: geometry (host only) ----
int heifgpu_window_source_rect(const heifgpu_image *img, const heifgpu_rect *window, heifgpu_rect *src) {
    if (!img || !src) return fail(HEIFGPU_E_INVALID, "null argument");
    Rect out;
    if (!window_source_rect(img->img, window ? rect_of(*window) : Rect{}, out))
        return fail(HEIFGPU_E_INVALID, "window empty or outside the displayed picture");
    *src = heifgpu_rect{out.x, out.y, out.w, out.h};
    return HEIFGPU_OK;
}

int heifgpu_image_tiles_for_rect(const heifgpu_image *img, const heifgpu_rect *src, uint32_t *col0, uint32_t *row0,
                                 uint32_t *cols, uint32_t *rows) {
    if (!img) return fail(HEIFGPU_E_INVALID, "null argument");
    const Rect r = src ? rect_of(*src) : Rect{};
    if (!rect_inside(r, img->img.out_width, img->img.out_height))
        return fail(HEIFGPU_E_INVALID, "source rectangle empty or outside the image");
    uint32_t v[4];
    tiles_for_rect(img->img, r, v[0], v[1], v[2], v[3]);
    if (col0) *col0 = v[0];
    if (row0) *row0 = v[1];
    if (cols) *cols = v[2];
    if (rows) *rows = v[3];
    return HEIFGPU_OK;
}

int heifgpu_abi_version(void) { return HEIFGPU_ABI_VERSION; }

// ---------------------------------------------------------------- test hooks
size_t heifgpu_remove_emulation_prevention(const uint8_t *in, size_t n, uint8_t *out) {
    std::vector<uint8_t> v = RbspReader::remove_emulation_prevention(in, n);
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    return v.size();
}

int heifgpu_read_ue(const uint8_t *buf, size_t n, uint32_t *val) {
    try {
        RbspReader r(buf, n);
        *val = r.read_ue();
        return HEIFGPU_OK;
    } catch (const std::exception &e) {
        return fail(HEIFGPU_E_PARSE, e.what());
    }
}

int heifgpu_read_se(const uint8_t *buf, size_t n, int32_t *val) {
    try {
        RbspReader r(buf, n);
        *val = r.read_se();
        return HEIFGPU_OK;
    } catch (const std::exception &e) {
        return fail(HEIFGPU_E_PARSE, e.what());
    }
}

namespace {
struct VecBins {
    const uint8_t *b;
    int n, i = 0;
    bool under = false;
    int operator()() {
        if (i >= n) {
            under = true;
            return 0;
        }
        return b[i++] ? 1 : 0;
    }
};
}  // namespace

int heifgpu_bins_truncated_rice(const uint8_t *bins, int n, int c_max, int c_rice, int *used) {
    VecBins v{bins, n};
    uint32_t r = bin_truncated_rice(v, uint32_t(c_max), c_rice);
    if (used) *used = v.i;
    return v.under ? -1 : int(r);
}

int heifgpu_bins_chroma_pred_mode(const uint8_t *bins, int n, int *used) {
    VecBins v{bins, n};
    uint32_t r = bin_intra_chroma_pred_mode(v, v);
    if (used) *used = v.i;
    return v.under ? -1 : int(r);
}

int heifgpu_bins_coeff_abs_level_remaining(const uint8_t *bins, int n, int c_rice, int *used) {
    VecBins v{bins, n};
    uint32_t r = bin_coeff_abs_level_remaining(v, c_rice);
    if (used) *used = v.i;
    return (v.under || r == 0xffffffffu) ? -1 : int(r);
}

int heifgpu_bins_exp_golomb(const uint8_t *bins, int n, int k, int *used) {
    VecBins v{bins, n};
    uint32_t r = bin_exp_golomb(v, k);
    if (used) *used = v.i;
    return (v.under || r == 0xffffffffu) ? -1 : int(r);
}

int heifgpu_image_tile_params(const heifgpu_image *img, uint32_t tile, heifgpu_tile_params *o) {
    if (!img || !o) return fail(HEIFGPU_E_INVALID, "invalid argument");
    const ParsedImage &pi = img->img;
    if (tile >= pi.tiles.size()) return fail(HEIFGPU_E_INVALID, "tile index out of range");
    const TileJob &t = pi.tiles[tile];
    const SequenceParameterSet &sps = pi.params[t.param].sps;
    const PictureParameterSet &pps = pi.params[t.param].pps;
    const SliceSegmentHeader &sh = t.segs[0].sh;  // the picture's first slice segment
    std::memset(o, 0, sizeof(*o));
    o->nal_unit_type = t.segs[0].nal.nal_unit_type();
    o->slice_type = sh.slice_type;
    o->first_slice_segment_in_pic = sh.first_slice_segment_in_pic_flag;
    o->general_profile_idc = sps.general_profile_idc;
    o->general_level_idc = sps.general_level_idc;
    o->pic_width = sps.pic_width_in_luma_samples;
    o->pic_height = sps.pic_height_in_luma_samples;
    o->chroma_format_idc = sps.chroma_format_idc;
    o->bit_depth_luma = 8 + sps.bit_depth_luma_minus8;
    o->bit_depth_chroma = 8 + sps.bit_depth_chroma_minus8;
    o->log2_max_poc_lsb = sps.log2_max_pic_order_cnt_lsb;
    o->log2_min_cb = sps.log2_min_luma_coding_block_size;
    o->log2_ctb = sps.log2_ctb_size;
    o->log2_min_tb = sps.log2_min_tb_size;
    o->log2_max_tb = sps.log2_max_tb_size;
    o->max_th_depth_inter = sps.max_transform_hierarchy_depth_inter;
    o->max_th_depth_intra = sps.max_transform_hierarchy_depth_intra;
    o->scaling_list_enabled = sps.scaling_list_enabled_flag;
    o->amp = sps.amp_enabled_flag;
    o->sao = sps.sample_adaptive_offset_enabled_flag;
    o->pcm = sps.pcm_enabled_flag;
    o->num_short_term_ref_pic_sets = sps.num_short_term_ref_pic_sets;
    o->long_term_refs = sps.long_term_ref_pics_present_flag;
    o->temporal_mvp = sps.sps_temporal_mvp_enabled_flag;
    o->strong_intra_smoothing = sps.strong_intra_smoothing_enabled_flag;
    o->video_full_range = sps.video_full_range_flag;
    o->colour_primaries = sps.colour_primaries;
    o->transfer_characteristics = sps.transfer_characteristics;
    o->matrix_coeffs = sps.matrix_coeffs;
    o->init_qp = 26 + pps.init_qp_minus26;
    o->sign_data_hiding = pps.sign_data_hiding_enabled_flag;
    o->cabac_init_present = pps.cabac_init_present_flag;
    o->constrained_intra_pred = pps.constrained_intra_pred_flag;
    o->transform_skip = pps.transform_skip_enabled_flag;
    o->cu_qp_delta_enabled = pps.cu_qp_delta_enabled_flag;
    o->diff_cu_qp_delta_depth = pps.diff_cu_qp_delta_depth;
    o->cb_qp_offset = pps.pps_cb_qp_offset;
    o->cr_qp_offset = pps.pps_cr_qp_offset;
    o->slice_chroma_qp_offsets_present = pps.pps_slice_chroma_qp_offsets_present_flag;
    o->transquant_bypass = pps.transquant_bypass_enabled_flag;
    o->tiles_enabled = pps.tiles_enabled_flag;
    o->entropy_coding_sync = pps.entropy_coding_sync_enabled_flag;
    o->loop_filter_across_slices = pps.pps_loop_filter_across_slices_enabled_flag;
    o->deblocking_control_present = pps.deblocking_filter_control_present_flag;
    o->deblocking_override_enabled = pps.deblocking_filter_override_enabled_flag;
    o->deblocking_disabled = sh.slice_deblocking_filter_disabled_flag;
    o->beta_offset_div2 = sh.slice_beta_offset_div2;
    o->tc_offset_div2 = sh.slice_tc_offset_div2;
    o->log2_parallel_merge_level = pps.log2_parallel_merge_level;
    o->slice_sao_luma = sh.slice_sao_luma_flag;
    o->slice_sao_chroma = sh.slice_sao_chroma_flag;
    o->slice_qp_y = 26 + pps.init_qp_minus26 + sh.slice_qp_delta;
    o->num_entry_point_offsets = sh.num_entry_point_offsets;
    o->slice_data_raw_offset = int32_t(sh.slice_data_raw_offset);
    o->payload_bytes = int32_t(t.segs[0].payload_len);
    for (size_t i = 0; i < sh.entry_point_offset.size() && i < 64; ++i) o->entry_point_offset[i] = sh.entry_point_offset[i];
    return HEIFGPU_OK;
}

}  // extern "C"
