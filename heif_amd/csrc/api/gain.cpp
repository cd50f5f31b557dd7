// gain.cpp — the host-only calls of the gain-map HDR render (include/heifgpu.h, "Gain-map HDR
// render"): what a parsed image says of its gain map, the transform, and the per-pixel formula
// and the sampler on the host (kernels/gain_xform.hpp: the functions k_render_gain runs), and the
// scaled render's averaging of gain codes (kernels/gain_scale.hpp: what k_render_gain_scaled runs).
// heifgpu_render_batch_gain and heifgpu_render_batch_gain_scaled are with the other renders in render.cpp.
#include <vector>

#include "../host/gain.hpp"
#include "../kernels/gain_scale.hpp"
#include "../kernels/gain_xform.hpp"
#include "api.hpp"

using namespace hg;

extern "C" {

int heifgpu_image_get_gain(const heifgpu_image *img, heifgpu_gain_info *out) {
    if (!img || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    const GainDesc &g = img->img.gain;
    std::memset(out, 0, sizeof(*out));
    out->kind = g.kind;
    out->gain_item_id = g.item_id;
    out->status = HEIFGPU_OK;
    if (g.kind == HEIFGPU_GAIN_ISO) {
        GainMeta m;
        std::string err;
        out->status = gain_read(g.tmap.data(), g.tmap.size(), m, err);
        out->version = m.version, out->minimum_version = m.minimum_version, out->writer_version = m.writer_version;
        out->multichannel = m.multichannel, out->use_base_colour_space = m.use_base_colour_space;
        out->base_headroom = m.base_headroom, out->alternate_headroom = m.alternate_headroom;
        out->gain_min = m.gain_min, out->gain_max = m.gain_max, out->gamma = m.gamma;
        out->base_offset = m.base_offset, out->alternate_offset = m.alternate_offset;
    }
    return HEIFGPU_OK;
}

int heifgpu_gain_transform_make(const heifgpu_image *base, const heifgpu_image *gain, uint32_t dst, uint32_t bits,
                                uint32_t encoding, uint32_t pq_bits, double headroom, double display_headroom,
                                double sdr_white, heifgpu_gain_transform *out) {
    if (!base || !gain || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    heifgpu_image_info gi;
    heifgpu_image_get_info(gain, &gi);
    std::string err;
    if (int rc = gain_transform_build(base->img.gain, base->img.color, gi.bit_depth, dst, bits, encoding, pq_bits, headroom,
                                      display_headroom, sdr_white, *out, err))
        return fail(rc, err);
    return HEIFGPU_OK;
}

int heifgpu_gain_apply(const heifgpu_gain_transform *t, const uint16_t *rgb_in, const uint32_t *g_q8, size_t n,
                       uint16_t *out) {
    if (!t || !rgb_in || !g_q8 || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    if (const char *why = gain_transform_invalid(*t)) return fail(HEIFGPU_E_INVALID, why);
    const int nn = 1 << t->bits;
    const uint32_t gmax = 256u * ((1u << t->gain_bits) - 1);
    // the tables as the device holds them: three of n entries, one after the other
    std::vector<uint16_t> in_lut(size_t(3) * nn);
    for (int c = 0; c < 3; ++c) std::memcpy(in_lut.data() + size_t(c) * nn, t->in_lut[c], size_t(nn) * 2);
    for (size_t i = 0; i < n; ++i) {
        if (rgb_in[3 * i] >= nn || rgb_in[3 * i + 1] >= nn || rgb_in[3 * i + 2] >= nn)
            return fail(HEIFGPU_E_INVALID, "code above maxv");
        if (g_q8[i] > gmax) return fail(HEIFGPU_E_INVALID, "gain code above 256 * maxg");
    }
    GainParams gp;
    for (int k = 0; k < 9; ++k) gp.m[k] = t->m[k];
    gp.k_b = t->k_b, gp.k_a = t->k_a;
    gp.encoding = t->encoding == HEIFGPU_GAIN_PQ ? GAIN_ENC_PQ : GAIN_ENC_LINEAR;
    const uint16_t *in = in_lut.data();
    const XfToneLut<const uint32_t *> T{t->T}, E{t->E};
    for (size_t i = 0; i < n; ++i) {
        uint32_t r = rgb_in[3 * i], g = rgb_in[3 * i + 1], b = rgb_in[3 * i + 2];
        gain_px(in, nn, T, E, gp, g_q8[i], r, g, b);
        out[3 * i] = uint16_t(r), out[3 * i + 1] = uint16_t(g), out[3 * i + 2] = uint16_t(b);
    }
    return HEIFGPU_OK;
}

int heifgpu_gain_sample(const void *gain, uint32_t wg, uint32_t hg_, int32_t pitch, uint32_t gain_bits, uint32_t w,
                        uint32_t h, uint32_t *g_q8) {
    if (!gain || !g_q8) return fail(HEIFGPU_E_INVALID, "null argument");
    if (gain_bits < 8 || gain_bits > 12) return fail(HEIFGPU_E_INVALID, "gain map depth outside 8..12");
    const uint32_t lim = uint32_t(kGainMaxSide);
    if (!w || !h || !wg || !hg_ || w > lim || h > lim || wg > lim || hg_ > lim)
        return fail(HEIFGPU_E_INVALID, "a side outside 1..65535");
    const int bps = gain_bits > 8 ? 2 : 1;
    if (int64_t(pitch) < int64_t(wg) * bps) return fail(HEIFGPU_E_INVALID, "pitch smaller than the row");
    const uint32_t maxg = (1u << gain_bits) - 1;
    auto at = [&](int x, int y) -> uint32_t {
        const uint8_t *row = static_cast<const uint8_t *>(gain) + size_t(y) * size_t(pitch);
        if (bps == 1) return row[x];
        uint16_t v;
        std::memcpy(&v, row + 2 * size_t(x), 2);
        return v;
    };
    for (uint32_t y = 0; y < hg_; ++y)
        for (uint32_t x = 0; x < wg; ++x)
            if (at(int(x), int(y)) > maxg) return fail(HEIFGPU_E_INVALID, "gain sample above maxg");
    const double inv_w = 1.0 / double(w), inv_h = 1.0 / double(h);
    for (uint32_t y = 0; y < h; ++y) {
        const GainTap ty = gain_tap(int(y), int(h), int(hg_), inv_h);
        for (uint32_t x = 0; x < w; ++x) {
            const GainTap tx = gain_tap(int(x), int(w), int(wg), inv_w);
            g_q8[size_t(y) * w + x] = gain_sample(at(tx.i0, ty.i0), at(tx.i1, ty.i0), at(tx.i0, ty.i1), at(tx.i1, ty.i1),
                                                  uint32_t(tx.f), uint32_t(ty.f));
        }
    }
    return HEIFGPU_OK;
}

int heifgpu_gain_average(const uint32_t *g_q8, uint32_t w, uint32_t h, const heifgpu_scale *scale, uint32_t *out) {
    if (!g_q8 || !scale || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    if (!w || !h || w > kGainScaleMaxSide || h > kGainScaleMaxSide) return fail(HEIFGPU_E_INVALID, "a side outside 1..65535");
    const heifgpu_scale &sc = *scale;
    if (!sc.out_width || !sc.out_height || sc.out_width > kGainScaleMaxSide || sc.out_height > kGainScaleMaxSide)
        return fail(HEIFGPU_E_INVALID, "rendered size outside 1..65535");
    uint32_t cx = 0, cy = 0, cw = w, ch = h;
    if (sc.width || sc.height) {
        if (!sc.width || !sc.height || sc.x >= w || sc.y >= h || sc.width > w - sc.x || sc.height > h - sc.y)
            return fail(HEIFGPU_E_INVALID, "window empty or outside the picture");
        cx = sc.x, cy = sc.y, cw = sc.width, ch = sc.height;
    }
    for (size_t i = 0; i < size_t(w) * h; ++i)
        if (g_q8[i] > kGainScaleMaxCode) return fail(HEIFGPU_E_INVALID, "gain code above 256 * 4095");
    std::vector<GsCol> col(cw);
    gs_average_window(g_q8, w, cx, cy, cw, ch, sc.out_width, sc.out_height, col.data(), out);
    return HEIFGPU_OK;
}

}  // extern "C"
