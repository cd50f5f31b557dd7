// render.cpp — the render family of the C ABI: heifgpu_render_batch, _scaled and _tensor
// with their _color forms, heifgpu_scale_fit, and the filtered (bilinear / bicubic) forms
// of the scaled and tensor renders with their host hooks, and the gain-map HDR render at
// full size and scaled.  Each call begins with call_check, checks its arguments and fills its
// descriptors, all without the context; submit then sends any of the descriptor types with the
// blocks that follow them (render_submit: the ColorRefs and ChromaUps; gain_submit: the GainRefs),
// their tables out of the one ColorCache.
// (The calls take their C linkage from the declarations of include/heifgpu.h.)
#include <cmath>
#include <initializer_list>
#include <memory>
#include <type_traits>
#include <vector>

#include "../common/desc.hpp"
#include "../host/icc.hpp"
#include "../host/resample.hpp"
#include "../kernels/color_xform.hpp"
#include "../kernels/gain_xform.hpp"
#include "api.hpp"

using namespace hg;

// The descriptors of a render call travel through a ring of slots,
// each a pinned host image, a device array and an event recorded behind the kernel
// that reads them: a call never rewrites descriptors that an earlier call's
// copy or kernel may still read (the host waits only when the ring wraps).
constexpr int kRenderSlots = 4;
struct RenderRing {
    struct Slot {
        PinnedBuf host;
        DevBuf<uint8_t> dev;  // n descriptors of the call's type, then its trailing blocks (submit)
        hipEvent_t done = nullptr;
        bool pending = false;
    } slot[kRenderSlots];
    int next = 0;
    ~RenderRing() {
        for (Slot &s : slot)
            if (s.done) (void)hipEventDestroy(s.done);
    }
};

// The tables of the transforms on the device, keyed by content: in_lut[3][1 << B] then
// out_lut as 4096 pairs (xf_out_pair), as ColorRef::lut addresses them; for a tone transform
// in_lut32[3][1 << B], the same pairs and a ToneBlock (another size), for a gain transform
// gain_table_image's, which ends in a tag: keys of two kinds never compare equal.  An entry is
// written once, by a blocking copy before the call that first uses it launches anything, and
// never again, so no launch in flight can see a table change; a steady-state call finds its
// tables here.
constexpr size_t kColorCacheMax = 256;
struct ColorCache {
    struct Entry {
        std::vector<uint16_t> key;
        uint16_t *dev = nullptr;
    };
    std::vector<Entry> entries;
    // lut: where the table with this content lies on the device, uploaded now if it is new
    // (what: "colour" or "gain", for the message of an upload that fails)
    int table(const std::vector<uint16_t> &key, const char *what, uint64_t &lut) {
        for (const Entry &e : entries)
            if (e.key == key) {
                lut = reinterpret_cast<uint64_t>(e.dev);
                return HEIFGPU_OK;
            }
        Entry e;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e.dev), key.size() * 2));
        const hipError_t up = hipMemcpy(e.dev, key.data(), key.size() * 2, hipMemcpyHostToDevice);  // blocking
        if (up != hipSuccess) {
            (void)hipFree(e.dev);
            return fail(HEIFGPU_E_DEVICE, std::string(what) + " table upload: " + hipGetErrorString(up));
        }
        lut = reinterpret_cast<uint64_t>(e.dev);
        e.key = key;
        entries.push_back(std::move(e));
        return HEIFGPU_OK;
    }
    void clear() {
        for (Entry &e : entries)
            if (e.dev) (void)hipFree(e.dev);
        entries.clear();
    }
    ~ColorCache() { clear(); }
};

// The context's cache for the tables of one call, made by the first call that needs it.  When it
// holds kColorCacheMax tables it is emptied, here and so once per call (a call may go past the
// limit by its own tables, and none of them is freed under it), after a device synchronise:
// nothing in flight reads a table that is freed.
static int color_cache_open(heifgpu_ctx *ctx, ColorCache *&cache) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->color) ctx->color = new ColorCache;
    cache = ctx->color;
    if (cache->entries.size() >= kColorCacheMax) {
        HIP_TRY(hipDeviceSynchronize());
        cache->clear();
    }
    return HEIFGPU_OK;
}

void hg::render_state_free(heifgpu_ctx *ctx) {
    delete ctx->render;
    delete ctx->color;
}

// the 4096 words out_lut[k] | out_lut[k + 1] << 16 of a colour table's image (xf_out_pair), at dst
static void out_pairs_write(const uint16_t *out_lut, void *dst) {
    for (int k = 0; k < kXfPairEntries; ++k) {
        const uint32_t w = xf_out_pair(out_lut, k);
        std::memcpy(static_cast<uint8_t *>(dst) + 4 * k, &w, 4);
    }
}

// The device image of a tone transform (t->tone != 0: the first member of a
// heifgpu_hdr_transform) as 16-bit units, and where its ToneBlock lies in it.
static void tone_table_image(const heifgpu_color_transform *t, std::vector<uint16_t> &key, int32_t &tone_off) {
    const heifgpu_hdr_transform &h = *reinterpret_cast<const heifgpu_hdr_transform *>(t);
    const size_t tn = size_t(1) << t->bits;
    const size_t off = 4 * (3 * tn + kXfPairEntries);  // bytes: a multiple of 8
    std::vector<uint8_t> img(off + sizeof(ToneBlock));
    for (int c = 0; c < 3; ++c) std::memcpy(img.data() + 4 * c * tn, h.in_lut32[c], 4 * tn);
    out_pairs_write(t->out_lut, img.data() + 4 * 3 * tn);
    ToneBlock tb{};
    for (int c = 0; c < 3; ++c) tb.w[c] = h.w[c];
    for (int k = 0; k < kXfTonePairs; ++k) tb.pairs[2 * k] = h.T[k], tb.pairs[2 * k + 1] = h.T[k + 1];
    std::memcpy(img.data() + off, &tb, sizeof(tb));
    key.resize(img.size() / 2);
    std::memcpy(key.data(), img.data(), img.size());
    tone_off = int32_t(off);
}

// refs[i] for the images of a render call (empty when no image is to be transformed:
// the call is then the unmanaged call); tone: some image has a tone transform.  Every
// check runs before anything is launched.  linear (the linear-light calls, behind linear_check):
// every image has a transform and every transform its tables, an identity too.
static int color_refs_fill(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, uint32_t format,
                           const heifgpu_color_transform *const *xf, bool linear, std::vector<ColorRef> &refs,
                           bool &tone) {
    static_assert(sizeof(ToneBlock) == 16 + 8 * kXfTonePairs && sizeof(ToneBlock) % 8 == 0, "ToneBlock: weights, then pairs");
    refs.clear();
    tone = false;
    if (!xf) return HEIFGPU_OK;
    bool any = false;
    for (size_t i = 0; i < n; ++i) {
        const heifgpu_color_transform *t = xf[i];
        if (!t) continue;
        heifgpu_image_info info;
        heifgpu_image_get_info(imgs[i], &info);
        const uint32_t depth = format >= HEIFGPU_PIX_RGB16 ? info.bit_depth : 8;
        if (t->bits != depth || t->bits < 8 || t->bits > 12)
            return fail(HEIFGPU_E_INVALID, "transform made for another depth than the image is rendered at");
        if (t->tone && (t->tone != HEIFGPU_TONE_BT2390 || t->identity ||
                        !hdr_transform_valid(*reinterpret_cast<const heifgpu_hdr_transform *>(t))))
            return fail(HEIFGPU_E_INVALID, "tone transform: tag, weights or a level above 2^22 - 1");
        any = any || linear || !t->identity;
    }
    if (!any) return HEIFGPU_OK;
    ColorCache *cache = nullptr;
    if (int rc = color_cache_open(ctx, cache)) return rc;
    refs.assign(n, ColorRef{});
    std::vector<uint16_t> key;
    for (size_t i = 0; i < n; ++i) {
        const heifgpu_color_transform *t = xf[i];
        if (!t || (t->identity && !linear)) continue;  // lut == 0: untouched
        const size_t tn = size_t(1) << t->bits;
        int32_t tone_off = 0;
        if (t->tone) {
            tone_table_image(t, key, tone_off);
            tone = true;
        } else {
            key.resize(3 * tn + 2 * kXfPairEntries);
            for (int c = 0; c < 3; ++c) std::memcpy(key.data() + c * tn, t->in_lut[c], tn * 2);
            out_pairs_write(t->out_lut, key.data() + 3 * tn);
        }
        if (int rc = cache->table(key, "colour", refs[i].lut)) return rc;
        refs[i].n = int32_t(tn);
        for (int k = 0; k < 9; ++k) refs[i].m[k] = t->m[k];
        refs[i].tone = int32_t(t->tone);
        refs[i].tone_off = tone_off;
    }
    return HEIFGPU_OK;
}

// What every render call checks first: its pointers (all: none of them is null) and n, its
// format (format_invalid: what is wrong with it, or nullptr), and n again.  The context is not
// among them: every check of the arguments answers without one, and the submit looks at it.
static int call_check(bool all, size_t n, const char *format_invalid) {
    if (!all || n == 0) return fail(HEIFGPU_E_INVALID, "invalid argument");
    if (format_invalid) return fail(HEIFGPU_E_INVALID, format_invalid);
    if (n > 65535) return fail(HEIFGPU_E_INVALID, "more than 65535 images in one render call");
    return HEIFGPU_OK;
}
// call_check's format_invalid for a pixel format of first..last
static const char *format_outside(uint32_t format, uint32_t first, uint32_t last) {
    return format < first || format > last ? "format" : nullptr;
}

// What heifgpu_render_batch and heifgpu_render_batch_scaled check and fill alike for
// image i: dm is the map the kernel reads through (for the scaled call the window is
// folded in; dm.out_width x out_height is then the window), ow x oh the size written.
// out == nullptr (heifgpu_render_batch_tensor): the caller checks and fills its own output.
static int render_desc_fill(size_t i, const heifgpu_image *const *imgs, const heifgpu_planes *in,
                            const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                            const heifgpu_surface *out, const DisplayMap &dm, uint32_t ow, uint32_t oh, int &bps,
                            RenderDesc &d) {
    const bool wide = format >= HEIFGPU_PIX_RGB16, with_alpha = (format & 1) != 0;
    const int bpp = (with_alpha ? 4 : 3) * (wide ? 2 : 1);
    heifgpu_image_info info;
    heifgpu_image_get_info(imgs[i], &info);
    if (!in[i].plane[0] || (out && !out[i].pixels)) return fail(HEIFGPU_E_INVALID, "missing plane or surface");
    if (info.chroma_format_idc && (!in[i].plane[1] || !in[i].plane[2]))
        return fail(HEIFGPU_E_INVALID, "missing chroma plane");
    if (info.bit_depth < 8 || info.bit_depth > (wide ? 12u : 16u)) return fail(HEIFGPU_E_INVALID, "bit depth");
    if (bps && bps != int(info.bytes_per_sample))
        return fail(HEIFGPU_E_UNSUPPORTED, "images of 1-byte and 2-byte samples in one render call");
    bps = int(info.bytes_per_sample);
    if (out && int64_t(out[i].pitch) < int64_t(bpp) * ow)
        return fail(HEIFGPU_E_INVALID, "surface pitch smaller than the output row");
    if (out && wide && ((reinterpret_cast<uintptr_t>(out[i].pixels) | uint32_t(out[i].pitch)) & 1))
        return fail(HEIFGPU_E_INVALID, "16-bit surface not 2-byte aligned");
    // the map's corners inside the decoded planes (parse_heic built it so; the kernel reads unchecked)
    for (int c = 0; c < 4; ++c) {
        const int64_t ox = (c & 1) ? int64_t(dm.out_width) - 1 : 0, oy = (c & 2) ? int64_t(dm.out_height) - 1 : 0;
        const int64_t x = dm.m[0] * ox + dm.m[1] * oy + dm.t[0], y = dm.m[2] * ox + dm.m[3] * oy + dm.t[1];
        if (x < 0 || y < 0 || x >= int64_t(info.width) || y >= int64_t(info.height))
            return fail(HEIFGPU_E_INVALID, "display map outside the decoded image");
    }
    d = RenderDesc{};
    for (int k = 0; k < 3; ++k) {
        d.plane[k] = reinterpret_cast<uint64_t>(in[i].plane[k]);
        d.pitch[k] = in[i].pitch[k];
    }
    if (out) {
        d.out = reinterpret_cast<uint64_t>(out[i].pixels);
        d.out_pitch = out[i].pitch;
    }
    d.out_w = int32_t(ow);
    d.out_h = int32_t(oh);
    for (int k = 0; k < 4; ++k) d.m[k] = dm.m[k];
    d.t[0] = dm.t[0];
    d.t[1] = dm.t[1];
    d.swap = dm.m[0] == 0;
    d.chroma = int32_t(info.chroma_format_idc);
    const int depth = wide ? int(info.bit_depth) : 8;  // the depth the arithmetic runs at
    d.shift = int32_t(info.bit_depth) - depth;
    render_coefs(info.matrix_coeffs, info.full_range != 0, depth, d);
    if (with_alpha && alpha_imgs && alpha_imgs[i]) {
        if (!alpha_in || !alpha_in[i].plane[0]) return fail(HEIFGPU_E_INVALID, "missing alpha plane");
        heifgpu_image_info ai;
        heifgpu_image_get_info(alpha_imgs[i], &ai);
        if (ai.width != info.width || ai.height != info.height)
            return fail(HEIFGPU_E_UNSUPPORTED, "alpha image of another size than its colour image");
        if (int(ai.bytes_per_sample) != bps)
            return fail(HEIFGPU_E_UNSUPPORTED, "images of 1-byte and 2-byte samples in one render call");
        d.alpha = reinterpret_cast<uint64_t>(alpha_in[i].plane[0]);
        d.alpha_pitch = alpha_in[i].pitch[0];
        d.alpha_bps = int32_t(ai.bytes_per_sample);
        d.alpha_shift = int32_t(ai.bit_depth) - depth;  // right when positive, left when negative
    }
    return HEIFGPU_OK;
}

// What every render call ends in, for any descriptor type: the next slot of the context's ring,
// drained of the call that used it last, the descriptors then the call's trailing blocks in one
// staging image, in the order given, one copy, the one launch (launch(descriptors on the device,
// stream)) and the slot's event.
struct Block {
    const void *p;
    size_t bytes;  // a multiple of 8, or 0: the call has no such block
};
template <class Desc, class Launch>
static int submit(heifgpu_ctx *ctx, const std::vector<Desc> &descs, std::initializer_list<Block> blocks, Launch launch,
                  void *stream) {
    static_assert(sizeof(Desc) % 8 == 0, "the blocks behind the descriptors are 8-byte aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->render) {
        auto ring = std::make_unique<RenderRing>();
        for (RenderRing::Slot &sl : ring->slot) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        ctx->render = ring.release();
    }
    RenderRing::Slot &sl = ctx->render->slot[ctx->render->next];
    ctx->render->next = (ctx->render->next + 1) % kRenderSlots;
    if (sl.pending) HIP_TRY(hipEventSynchronize(sl.done));  // the call that used this slot last
    sl.pending = false;
    const size_t dbytes = descs.size() * sizeof(Desc);
    size_t bytes = dbytes;
    for (const Block &b : blocks) bytes += b.bytes;
    HIP_TRY(sl.host.reserve(bytes));
    HIP_TRY(sl.dev.alloc(bytes));
    std::memcpy(sl.host.p, descs.data(), dbytes);
    size_t at = dbytes;
    for (const Block &b : blocks) {  // behind the descriptors: one copy
        if (b.bytes) std::memcpy(sl.host.p + at, b.p, b.bytes);
        at += b.bytes;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(sl.dev.p, sl.host.p, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(launch(reinterpret_cast<const Desc *>(sl.dev.p), s));  // the one launch
    HIP_TRY(hipEventRecord(sl.done, s));
    sl.pending = true;
    return HEIFGPU_OK;
}

// The tail of every render but the gain-map renders, for Desc = RenderDesc, ScaleDesc, TensorDesc
// or the filtered calls': the context, the colour refs, and the submit.  When an image of the
// call is set to bilinear chroma upsampling (image_chroma_up: the setting window_source_rect
// reads too) the call goes to the kernels that know it: a ChromaRef per image follows the
// ColorRefs, which are then always there (lut == 0 for an image without a transform).
// linear (Desc = ScaleDesc or TensorDesc, behind linear_check): the call goes to the kernels that
// average in linear light, which always read a ColorRef with tables and a ChromaRef per image.
template <class Desc>
static int render_submit(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, const std::vector<Desc> &descs,
                         int max_tiles, uint32_t format, int bps, const heifgpu_color_transform *const *xf,
                         void *stream, bool linear = false) {
    static_assert(sizeof(ColorRef) % 8 == 0, "the ChromaUps behind the ColorRefs are 8-byte aligned");
    static_assert(sizeof(ChromaUp) == sizeof(ChromaRef), "ChromaUp is ChromaRef's image");
    if (!ctx) return fail(HEIFGPU_E_INVALID, "null context");
    const size_t n = descs.size();
    std::vector<ColorRef> refs;
    bool tone = false;
    if (int rc = color_refs_fill(ctx, imgs, n, format, xf, linear, refs, tone)) return rc;
    std::vector<ChromaUp> ups;
    bool any_up = false;
    for (size_t i = 0; i < n; ++i) any_up = any_up || image_chroma_up(imgs[i]->img).mode != 0;
    if (any_up || linear) {
        if (refs.empty()) refs.assign(n, ColorRef{});
        ups.resize(n);
        for (size_t i = 0; i < n; ++i) ups[i] = image_chroma_up(imgs[i]->img);
    }
    const int nn = int(n), fmt = int(format);
    const int color = any_up ? RENDER_CHROMA : refs.empty() ? RENDER_PLAIN : tone ? RENDER_TONE : RENDER_MANAGED;
    if constexpr (std::is_same<Desc, ScaleDesc>::value || std::is_same<Desc, TensorDesc>::value) {
        if (linear)
            return submit(ctx, descs, {{refs.data(), refs.size() * sizeof(ColorRef)}, {ups.data(), ups.size() * sizeof(ChromaUp)}},
                          [=](const Desc *dev, hipStream_t s) { return launch_render_linear(dev, nn, max_tiles, fmt, bps, s); },
                          stream);
    }
    return submit(ctx, descs, {{refs.data(), refs.size() * sizeof(ColorRef)}, {ups.data(), ups.size() * sizeof(ChromaUp)}},
                  [=](const Desc *dev, hipStream_t s) { return launch_render(dev, nn, max_tiles, fmt, bps, color, s); },
                  stream);
}

// the tile geometry of a full-size render (k_render, k_render_gain) in its descriptor; returns d.tiles
static int full_size_tiles(RenderDesc &d) {
    const int tw = d.swap ? kRenderTile : kRenderRowW, th = d.swap ? kRenderTile : kRenderRowH;
    d.tiles_x = (d.out_w + tw - 1) / tw;
    d.tiles = d.tiles_x * ((d.out_h + th - 1) / th);
    return d.tiles;
}

static int render_batch_impl(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                             const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                             const heifgpu_color_transform *const *xf, const heifgpu_surface *out, void *stream) {
    if (int rc = call_check(imgs && in && out, n, format_outside(format, 0, HEIFGPU_PIX_RGBA16))) return rc;
    std::vector<RenderDesc> descs(n);
    int bps = 0, max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!imgs[i]) return fail(HEIFGPU_E_INVALID, "null image");
        const DisplayMap &dm = imgs[i]->img.display;
        if (int rc = render_desc_fill(i, imgs, in, alpha_imgs, alpha_in, format, out, dm, dm.out_width, dm.out_height,
                                      bps, descs[i]))
            return rc;
        max_tiles = std::max(max_tiles, full_size_tiles(descs[i]));
    }
    return render_submit(ctx, imgs, descs, max_tiles, format, bps, xf, stream);
}

int heifgpu_render_batch(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                         const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                         const heifgpu_surface *out, void *stream) {
    return render_batch_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, format, nullptr, out, stream);
}

int heifgpu_render_batch_color(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                               const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                               const heifgpu_color_transform *const *xf, const heifgpu_surface *out, void *stream) {
    return render_batch_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, format, xf, out, stream);
}

// round_half_up(n / d) = floor((2n + d) / 2d); n, d < 2^32
static uint64_t round_div(uint64_t n, uint64_t d) { return (2 * n + d) / (2 * d); }

int heifgpu_scale_fit(const heifgpu_display_info *d, uint32_t box_w, uint32_t box_h, uint32_t mode, heifgpu_scale *out) {
    if (!d || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    if (!box_w || !box_h) return fail(HEIFGPU_E_INVALID, "empty box");
    if (mode > HEIFGPU_FIT_COVER) return fail(HEIFGPU_E_INVALID, "fit mode");
    if (!d->out_width || !d->out_height) return fail(HEIFGPU_E_INVALID, "empty picture");
    const uint64_t dw = d->out_width, dh = d->out_height, bw = box_w, bh = box_h;
    heifgpu_scale s{};
    s.out_width = box_w;
    s.out_height = box_h;  // STRETCH; x = y = width = height = 0: the whole picture
    const bool wider = dw * bh >= dh * bw;  // the picture is at least as wide as the box, relatively
    if (mode == HEIFGPU_FIT_CONTAIN) {
        if (wider) s.out_height = uint32_t(std::max<uint64_t>(1, round_div(dh * bw, dw)));
        else s.out_width = uint32_t(std::max<uint64_t>(1, round_div(dw * bh, dh)));
    } else if (mode == HEIFGPU_FIT_COVER) {
        s.width = d->out_width;
        s.height = d->out_height;
        if (wider) {
            s.width = uint32_t(std::max<uint64_t>(1, round_div(dh * bw, bh)));
            s.x = (d->out_width - s.width) / 2;
        } else {
            s.height = uint32_t(std::max<uint64_t>(1, round_div(dw * bh, bw)));
            s.y = (d->out_height - s.height) / 2;
        }
    }
    *out = s;
    return HEIFGPU_OK;
}

// The one reading of a heifgpu_scale: its rendered size, and its window of image img as
// (x, y, w, h) of the displayed picture (the whole picture when it names none).
static int scale_window(const heifgpu_image *img, const heifgpu_scale &sc, uint32_t (&w)[4]) {
    if (!img) return fail(HEIFGPU_E_INVALID, "null image");
    const DisplayMap &dm = img->img.display;
    if (!sc.out_width || !sc.out_height || sc.out_width > 65535 || sc.out_height > 65535)
        return fail(HEIFGPU_E_INVALID, "rendered size outside 1..65535");
    w[0] = w[1] = 0, w[2] = dm.out_width, w[3] = dm.out_height;
    if (sc.width || sc.height) {
        if (!sc.width || !sc.height || sc.x >= dm.out_width || sc.y >= dm.out_height ||
            sc.width > dm.out_width - sc.x || sc.height > dm.out_height - sc.y)
            return fail(HEIFGPU_E_INVALID, "window empty or outside the displayed picture");
        w[0] = sc.x, w[1] = sc.y, w[2] = sc.width, w[3] = sc.height;
    }
    return HEIFGPU_OK;
}

// What heifgpu_render_batch_scaled and heifgpu_render_batch_tensor check and fill alike
// for image i: the window (scale_window), then `flip` (bit 0: columns, bit 1: rows of the rendered
// picture, which is the mirrored window rendered: the weights are symmetric) as further
// steps of the display map, render_desc_fill through that map, and the tile geometry.
static int scale_desc_fill(size_t i, const heifgpu_image *const *imgs, const heifgpu_planes *in,
                           const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                           const heifgpu_scale &sc, uint32_t flip, const heifgpu_surface *out, int &bps, ScaleDesc &sd) {
    uint32_t w[4];
    if (int rc = scale_window(imgs[i], sc, w)) return rc;
    DisplayMap dm = imgs[i]->img.display;
    if (sc.width || sc.height) display_window(dm, w[0], w[1], w[2], w[3]);
    if (flip & 1) display_imir(dm, 0);
    if (flip & 2) display_imir(dm, 1);
    if (dm.out_width > 65535 || dm.out_height > 65535)
        return fail(HEIFGPU_E_UNSUPPORTED, "window side above 65535");  // (the 32-bit line sums of the kernel)
    sd = ScaleDesc{};
    RenderDesc &d = sd.r;
    if (int rc = render_desc_fill(i, imgs, in, alpha_imgs, alpha_in, format, out, dm, sc.out_width, sc.out_height, bps,
                                  d))
        return rc;
    // the source's axes: a runs along its y, b along its x (kernels.hpp)
    const int32_t cw = int32_t(dm.out_width), ch = int32_t(dm.out_height);
    if (d.swap) {
        sd.ca = cw, sd.oa = d.out_w, sd.ma = d.m[2], sd.ta = d.t[1];
        sd.cb = ch, sd.ob = d.out_h, sd.mb = d.m[1], sd.tb = d.t[0];
        // 64 pixels along the output's x (store_row); along its y as many as keep the footprint
        // within a chunk of kScaleCols source columns, 16 at the least
        sd.na = kScaleTile, sd.nb = kScaleTile;
        while (sd.nb > 16 && int64_t(sd.nb) * sd.cb > int64_t(kScaleCols) * sd.ob) sd.nb /= 2;
    } else {
        sd.ca = ch, sd.oa = d.out_h, sd.ma = d.m[3], sd.ta = d.t[1];
        sd.cb = cw, sd.ob = d.out_w, sd.mb = d.m[0], sd.tb = d.t[0];
        // as many columns as fill a chunk of kScaleCols source columns, 64 at ratios from 4 up
        sd.na = kScaleRowsA;
        sd.nb = 64;
        while (sd.nb < 256 && int64_t(2 * sd.nb) * sd.cb <= int64_t(kScaleCols) * sd.ob) sd.nb *= 2;
    }
    for (sd.nb_log2 = 4; (1 << sd.nb_log2) < sd.nb;) ++sd.nb_log2;
    sd.den = 2 * uint64_t(cw) * uint64_t(ch);
    sd.inv_den = 1.0 / double(sd.den);
    d.tiles_x = (sd.ob + sd.nb - 1) / sd.nb;
    d.tiles = d.tiles_x * ((sd.oa + sd.na - 1) / sd.na);
    return HEIFGPU_OK;
}

// What the two linear-light calls refuse beside their siblings' checks (include/heifgpu.h
// "Linear-light scaled render"), before the context is looked at: an image without a transform
// (an identity transform is applied here, not skipped), one made for another depth, a tone stage.
static int linear_check(const heifgpu_image *const *imgs, size_t n, uint32_t format,
                        const heifgpu_color_transform *const *xf) {
    if (!xf) return fail(HEIFGPU_E_INVALID, "linear-light render without transforms");
    for (size_t i = 0; i < n; ++i) {
        if (!imgs[i]) return fail(HEIFGPU_E_INVALID, "null image");
        const heifgpu_color_transform *t = xf[i];
        if (!t) return fail(HEIFGPU_E_INVALID, "linear-light render of an image without a transform");
        heifgpu_image_info info;
        heifgpu_image_get_info(imgs[i], &info);
        const uint32_t depth = format >= HEIFGPU_PIX_RGB16 ? info.bit_depth : 8;
        if (t->bits != depth || t->bits < 8 || t->bits > 12)
            return fail(HEIFGPU_E_INVALID, "transform made for another depth than the image is rendered at");
        if (t->tone) return fail(HEIFGPU_E_UNSUPPORTED, "linear-light render of a tone transform");
    }
    return HEIFGPU_OK;
}

static int render_scaled_impl(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                              const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                              const heifgpu_scale *scale, const heifgpu_color_transform *const *xf,
                              const heifgpu_surface *out, void *stream, bool linear = false) {
    if (int rc = call_check(imgs && in && scale && out, n, format_outside(format, 0, HEIFGPU_PIX_RGBA16))) return rc;
    if (linear)
        if (int rc = linear_check(imgs, n, format, xf)) return rc;
    std::vector<ScaleDesc> descs(n);
    int bps = 0, max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        if (int rc = scale_desc_fill(i, imgs, in, alpha_imgs, alpha_in, format, scale[i], 0, out, bps, descs[i]))
            return rc;
        max_tiles = std::max(max_tiles, descs[i].r.tiles);
    }
    return render_submit(ctx, imgs, descs, max_tiles, format, bps, xf, stream, linear);
}

int heifgpu_render_batch_scaled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                                const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                                const heifgpu_scale *scale, const heifgpu_surface *out, void *stream) {
    return render_scaled_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, format, scale, nullptr, out, stream);
}

int heifgpu_render_batch_scaled_color(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                      const heifgpu_planes *in, const heifgpu_image *const *alpha_imgs,
                                      const heifgpu_planes *alpha_in, uint32_t format, const heifgpu_scale *scale,
                                      const heifgpu_color_transform *const *xf, const heifgpu_surface *out,
                                      void *stream) {
    return render_scaled_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, format, scale, xf, out, stream);
}

// what is wrong with the heifgpu_tensor_format of a tensor call, or nullptr (call_check's format_invalid)
static const char *tensor_format_invalid(const heifgpu_tensor_format *fmt) {
    if (!fmt) return "invalid argument";
    if (fmt->src > HEIFGPU_PIX_RGBA16) return "source format";
    if (fmt->elem > HEIFGPU_ELEM_BF16) return "element type";
    if (fmt->layout > HEIFGPU_LAYOUT_HWC) return "layout";
    for (int c = 0; c < ((fmt->src & 1) ? 4 : 3); ++c)
        if (!std::isfinite(fmt->a[c]) || !std::isfinite(fmt->b[c])) return "scale or bias not finite";
    return nullptr;
}

// The output half of image i's TensorDesc, behind the fill of td.s.r (its out_w is the row): the
// image's flip and tensor surface checked, the surface and the format's constants filled in.
static int tensor_out_fill(const heifgpu_tensor_format &fmt, const heifgpu_tensor_surface &o, uint32_t flip, TensorDesc &td) {
    if (flip > 3) return fail(HEIFGPU_E_INVALID, "flip above 3");
    const int nch = (fmt.src & 1) ? 4 : 3;
    const int64_t esz = fmt.elem == HEIFGPU_ELEM_F32 ? 4 : 2;
    if (!o.data || (reinterpret_cast<uintptr_t>(o.data) & uintptr_t(esz - 1)))
        return fail(HEIFGPU_E_INVALID, "tensor data null or not aligned to its element");
    const int64_t row = int64_t(td.s.r.out_w) * esz * (fmt.layout == HEIFGPU_LAYOUT_HWC ? nch : 1);
    if (o.stride_y < row || (o.stride_y & (esz - 1)))
        return fail(HEIFGPU_E_INVALID, "stride_y below the row or not a multiple of the element size");
    if (fmt.layout == HEIFGPU_LAYOUT_CHW && (o.stride_c & (esz - 1)))
        return fail(HEIFGPU_E_INVALID, "stride_c not a multiple of the element size");
    td.s.r.out = reinterpret_cast<uint64_t>(o.data);
    td.stride_c = fmt.layout == HEIFGPU_LAYOUT_CHW ? o.stride_c : 0;
    td.stride_y = o.stride_y;
    td.elem = int32_t(fmt.elem);
    td.layout = int32_t(fmt.layout);
    for (int c = 0; c < 4; ++c) {
        td.a[c] = c < nch ? fmt.a[c] : 0.f;
        td.b[c] = c < nch ? fmt.b[c] : 0.f;
    }
    return HEIFGPU_OK;
}

static int render_tensor_impl(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                              const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in,
                              const heifgpu_tensor_format *fmt, const heifgpu_scale *scale, const uint32_t *flip,
                              const heifgpu_color_transform *const *xf, const heifgpu_tensor_surface *out,
                              void *stream, bool linear = false) {
    if (int rc = call_check(imgs && in && fmt && scale && out, n, tensor_format_invalid(fmt))) return rc;
    if (linear)
        if (int rc = linear_check(imgs, n, fmt->src, xf)) return rc;
    std::vector<TensorDesc> descs(n);
    int bps = 0, max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t fl = flip ? flip[i] : 0;
        TensorDesc &td = descs[i];
        if (int rc = scale_desc_fill(i, imgs, in, alpha_imgs, alpha_in, fmt->src, scale[i], fl, nullptr, bps, td.s))
            return rc;
        if (int rc = tensor_out_fill(*fmt, out[i], fl, td)) return rc;
        max_tiles = std::max(max_tiles, td.s.r.tiles);
    }
    return render_submit(ctx, imgs, descs, max_tiles, fmt->src, bps, xf, stream, linear);
}

int heifgpu_render_batch_tensor(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                                const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in,
                                const heifgpu_tensor_format *fmt, const heifgpu_scale *scale, const uint32_t *flip,
                                const heifgpu_tensor_surface *out, void *stream) {
    return render_tensor_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, fmt, scale, flip, nullptr, out, stream);
}

int heifgpu_render_batch_scaled_linear(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                       const heifgpu_planes *in, const heifgpu_image *const *alpha_imgs,
                                       const heifgpu_planes *alpha_in, uint32_t format, const heifgpu_scale *scale,
                                       const heifgpu_color_transform *const *xf, const heifgpu_surface *out,
                                       void *stream) {
    return render_scaled_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, format, scale, xf, out, stream, true);
}

int heifgpu_render_batch_tensor_linear(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                       const heifgpu_planes *in, const heifgpu_image *const *alpha_imgs,
                                       const heifgpu_planes *alpha_in, const heifgpu_tensor_format *fmt,
                                       const heifgpu_scale *scale, const uint32_t *flip,
                                       const heifgpu_color_transform *const *xf, const heifgpu_tensor_surface *out,
                                       void *stream) {
    return render_tensor_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, fmt, scale, flip, xf, out, stream, true);
}

// ---- the filtered renders (k_render_resampled) ----
// scale_window for the filtered calls, whose taps reach over the whole displayed picture
static int filtered_window(const heifgpu_image *img, const heifgpu_scale &sc, uint32_t (&w)[4]) {
    if (int rc = scale_window(img, sc, w)) return rc;
    if (img->img.display.out_width > 65535 || img->img.display.out_height > 65535)
        return fail(HEIFGPU_E_UNSUPPORTED, "displayed side above 65535");
    return HEIFGPU_OK;
}

// What the two filtered calls check and fill alike for image i: the window, render_desc_fill
// through the map of the whole displayed picture, the two axes and the tile geometry.
static int resample_desc_fill(size_t i, const heifgpu_image *const *imgs, const heifgpu_planes *in,
                              const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                              const heifgpu_scale &sc, uint32_t filter, uint32_t flip, const heifgpu_surface *out,
                              int &bps, RenderDesc &d, RsParams &p) {
    uint32_t w[4];
    if (int rc = filtered_window(imgs[i], sc, w)) return rc;
    const DisplayMap &dm = imgs[i]->img.display;
    if (int rc = render_desc_fill(i, imgs, in, alpha_imgs, alpha_in, format, out, dm, sc.out_width, sc.out_height, bps, d))
        return rc;
    int depth = 8;
    while ((1 << depth) - 1 < d.maxv) ++depth;
    p = RsParams{};
    p.ax = rs_axis(int(dm.out_width), int(w[0]), int(w[0] + w[2]), int(sc.out_width), int(filter));
    p.ay = rs_axis(int(dm.out_height), int(w[1]), int(w[1] + w[3]), int(sc.out_height), int(filter));
    p.P = rs_precision(depth);
    p.flip = int32_t(flip);
    p.sw = rs_subtile(p.ax);
    d.tiles_x = (d.out_w + kRsTileW - 1) / kRsTileW;
    d.tiles = d.tiles_x * ((d.out_h + kRsTileH - 1) / kRsTileH);
    return HEIFGPU_OK;
}

int heifgpu_render_batch_resampled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                   const heifgpu_planes *in, const heifgpu_image *const *alpha_imgs,
                                   const heifgpu_planes *alpha_in, uint32_t format, const heifgpu_scale *scale,
                                   uint32_t filter, const heifgpu_color_transform *const *xf,
                                   const heifgpu_surface *out, void *stream) {
    if (filter > HEIFGPU_FILTER_BICUBIC) return fail(HEIFGPU_E_INVALID, "filter");
    if (filter == HEIFGPU_FILTER_AREA)
        return render_scaled_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, format, scale, xf, out, stream);
    if (int rc = call_check(imgs && in && scale && out, n, format_outside(format, 0, HEIFGPU_PIX_RGBA16))) return rc;
    std::vector<ResampleDesc> descs(n);
    int bps = 0, max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        if (int rc = resample_desc_fill(i, imgs, in, alpha_imgs, alpha_in, format, scale[i], filter, 0, out, bps,
                                        descs[i].r, descs[i].p))
            return rc;
        max_tiles = std::max(max_tiles, descs[i].r.tiles);
    }
    return render_submit(ctx, imgs, descs, max_tiles, format, bps, xf, stream);
}

int heifgpu_render_batch_tensor_resampled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                          const heifgpu_planes *in, const heifgpu_image *const *alpha_imgs,
                                          const heifgpu_planes *alpha_in, const heifgpu_tensor_format *fmt,
                                          const heifgpu_scale *scale, uint32_t filter, const uint32_t *flip,
                                          const heifgpu_color_transform *const *xf, const heifgpu_tensor_surface *out,
                                          void *stream) {
    if (filter > HEIFGPU_FILTER_BICUBIC) return fail(HEIFGPU_E_INVALID, "filter");
    if (filter == HEIFGPU_FILTER_AREA)
        return render_tensor_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, fmt, scale, flip, xf, out, stream);
    if (int rc = call_check(imgs && in && fmt && scale && out, n, tensor_format_invalid(fmt))) return rc;
    std::vector<ResampleTensorDesc> descs(n);
    int bps = 0, max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t fl = flip ? flip[i] : 0;
        TensorDesc &td = descs[i].t;
        if (int rc = resample_desc_fill(i, imgs, in, alpha_imgs, alpha_in, fmt->src, scale[i], filter, fl, nullptr, bps,
                                        td.s.r, descs[i].p))
            return rc;
        if (int rc = tensor_out_fill(*fmt, out[i], fl, td)) return rc;
        max_tiles = std::max(max_tiles, td.s.r.tiles);
    }
    return render_submit(ctx, imgs, descs, max_tiles, fmt->src, bps, xf, stream);
}

// ---- host only: the resampling's coefficients, its two passes, its source rectangle ----
int heifgpu_resample_coeffs(uint32_t in_size, uint32_t in0, uint32_t in1, uint32_t out_size, uint32_t filter,
                            uint32_t bits, int32_t *bounds, int32_t *kk, size_t cap, uint32_t *ksize) {
    if (!ksize) return fail(HEIFGPU_E_INVALID, "null argument");
    if (!resample_axis_ok(in_size, in0, in1, out_size, filter, bits))
        return fail(HEIFGPU_E_INVALID, "side, window, size, filter or depth outside the resampling's range");
    const uint32_t ks = uint32_t(resample_coeffs(int(in_size), int(in0), int(in1), int(out_size), int(filter), int(bits),
                                                 nullptr, nullptr));
    *ksize = ks;
    if (kk && cap < size_t(ks) * out_size) return fail(HEIFGPU_E_INVALID, "kk holds fewer than out_size * ksize entries");
    if (bounds || kk)
        resample_coeffs(int(in_size), int(in0), int(in1), int(out_size), int(filter), int(bits), bounds, kk);
    return HEIFGPU_OK;
}

int heifgpu_resample_apply(const void *in, uint32_t in_width, uint32_t in_height, uint32_t channels, uint32_t bits,
                           const heifgpu_rect *window, uint32_t out_width, uint32_t out_height, uint32_t filter,
                           void *out) {
    if (!in || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    if (channels < 1 || channels > 4) return fail(HEIFGPU_E_INVALID, "channels outside 1..4");
    heifgpu_rect w{0, 0, in_width, in_height};
    if (window && (window->width || window->height)) w = *window;
    if (!resample_axis_ok(in_width, w.x, uint64_t(w.x) + w.width, out_width, filter, bits) ||
        !resample_axis_ok(in_height, w.y, uint64_t(w.y) + w.height, out_height, filter, bits))
        return fail(HEIFGPU_E_INVALID, "side, window, size, filter or depth outside the resampling's range");
    const size_t count = size_t(in_width) * in_height * channels;
    const uint32_t maxv = (1u << bits) - 1;
    for (size_t k = 0; bits > 8 && k < count; ++k)
        if (static_cast<const uint16_t *>(in)[k] > maxv) return fail(HEIFGPU_E_INVALID, "code above maxv");
    resample_apply(in, bits > 8 ? 2 : 1, int(in_width), int(in_height), int(channels), int(bits), int(w.x), int(w.y),
                   int(w.width), int(w.height), int(out_width), int(out_height), int(filter), out);
    return HEIFGPU_OK;
}

int heifgpu_window_source_rect_resampled(const heifgpu_image *img, const heifgpu_scale *scale, uint32_t filter,
                                         heifgpu_rect *src) {
    if (!img || !scale || !src) return fail(HEIFGPU_E_INVALID, "null argument");
    if (filter > HEIFGPU_FILTER_BICUBIC) return fail(HEIFGPU_E_INVALID, "filter");
    uint32_t w[4];
    if (int rc = filtered_window(img, *scale, w)) return rc;
    if (filter != HEIFGPU_FILTER_AREA) {
        // per axis the taps of the first output to those of the last, in the displayed picture
        const DisplayMap &dm = img->img.display;
        const uint32_t side[2] = {dm.out_width, dm.out_height}, outs[2] = {scale->out_width, scale->out_height};
        for (int k = 0; k < 2; ++k) {
            const RsAxis a = rs_axis(int(side[k]), int(w[k]), int(w[k] + w[2 + k]), int(outs[k]), int(filter));
            int lo, hi, skip;
            rs_bounds(a, 0, lo, skip);
            rs_bounds(a, int(outs[k]) - 1, skip, hi);
            w[k] = uint32_t(lo);
            w[2 + k] = uint32_t(hi - lo);
        }
    }
    Rect r;
    if (!window_source_rect(img->img, Rect{w[0], w[1], w[2], w[3]}, r))
        return fail(HEIFGPU_E_INVALID, "window empty or outside the displayed picture");
    *src = heifgpu_rect{r.x, r.y, r.w, r.h};
    return HEIFGPU_OK;
}

int heifgpu_render_batch_tensor_color(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                      const heifgpu_planes *in, const heifgpu_image *const *alpha_imgs,
                                      const heifgpu_planes *alpha_in, const heifgpu_tensor_format *fmt,
                                      const heifgpu_scale *scale, const uint32_t *flip,
                                      const heifgpu_color_transform *const *xf, const heifgpu_tensor_surface *out,
                                      void *stream) {
    return render_tensor_impl(ctx, imgs, n, in, alpha_imgs, alpha_in, fmt, scale, flip, xf, out, stream);
}

// ---- the gain-map HDR render (k_render_gain; include/heifgpu.h "Gain-map HDR render") ----
// The device image of a gain transform as 16-bit units (the cache's key): in_lut[3][n], the
// pairs T[i], T[i + 1] for i = 0 .. maxg, for PQ the pairs E[i], E[i + 1] for i = 0 .. 639, and a
// tag that no colour table ends in.
static void gain_table_image(const heifgpu_gain_transform &t, std::vector<uint16_t> &key, int32_t &t_off, int32_t &e_off) {
    const size_t tn = size_t(1) << t.bits, ng = size_t(1) << t.gain_bits;  // ng = maxg + 1 pairs
    const size_t ne = t.encoding == HEIFGPU_GAIN_PQ ? size_t(kGainEPairs) : 0;
    const size_t toff = 6 * tn, eoff = toff + 8 * ng, end = eoff + 8 * ne;  // bytes: multiples of 8
    std::vector<uint8_t> img(end + 8);
    for (int c = 0; c < 3; ++c) std::memcpy(img.data() + 2 * c * tn, t.in_lut[c], 2 * tn);
    for (size_t i = 0; i < ng; ++i) std::memcpy(img.data() + toff + 8 * i, &t.T[i], 8);  // T[i], T[i + 1]
    for (size_t i = 0; i < ne; ++i) std::memcpy(img.data() + eoff + 8 * i, &t.E[i], 8);
    std::memcpy(img.data() + end, "gain map", 8);
    key.resize(img.size() / 2);
    std::memcpy(key.data(), img.data(), img.size());
    t_off = int32_t(toff);
    e_off = ne ? int32_t(eoff) : 0;
}

// The fields GainRef and GainScaleDesc have alike, in either (G): the gain plane, the decoded
// base and gain-map sizes, the top gain code.
template <class G>
static void gain_map_fill(const heifgpu_planes &gain_in, const heifgpu_image_info &info, const heifgpu_image_info &ginfo,
                          uint32_t gain_bits, G &g) {
    g.gain = reinterpret_cast<uint64_t>(gain_in.plane[0]);
    g.gain_pitch = gain_in.pitch[0];
    g.gain_bps = int32_t(ginfo.bytes_per_sample);
    g.w = int32_t(info.width), g.h = int32_t(info.height), g.wg = int32_t(ginfo.width), g.hg = int32_t(ginfo.height);
    g.inv_w = 1.0 / double(info.width), g.inv_h = 1.0 / double(info.height);
    g.gmax = 256u * ((1u << gain_bits) - 1);
}

// What the two gain-map renders check and fill alike for image i, in front of its descriptor:
// the transform, the images' depths and sides, the gain image's display map, the planes'
// pitches.  g: everything of the GainRef but its tables; gd: the scaled render's descriptor, which
// gets its gain_map_fill too (nullptr at full size); abits: the alpha image's depth, 0 without one.
static int gain_image_fill(size_t i, const heifgpu_image *const *imgs, const heifgpu_image *const *gain_imgs,
                           const heifgpu_planes *gain_in, const heifgpu_image *const *alpha_imgs,
                           const heifgpu_planes *alpha_in, bool pq, bool with_alpha,
                           const heifgpu_gain_transform *const *xf, GainRef &g, GainScaleDesc *gd, uint32_t &abits) {
    if (!imgs[i] || !gain_imgs[i]) return fail(HEIFGPU_E_INVALID, "null image");
    if (!xf[i]) return fail(HEIFGPU_E_INVALID, "null gain transform");
    const heifgpu_gain_transform &t = *xf[i];
    if (const char *why = gain_transform_invalid(t)) return fail(HEIFGPU_E_INVALID, why);
    if (t.encoding != (pq ? HEIFGPU_GAIN_PQ : HEIFGPU_GAIN_LINEAR))
        return fail(HEIFGPU_E_INVALID, "gain transform made for the other encoding than the format's");
    const ParsedImage &bi = imgs[i]->img, &gi = gain_imgs[i]->img;
    if (image_chroma_up(bi).mode != 0 || image_chroma_up(gi).mode != 0 ||
        (with_alpha && alpha_imgs && alpha_imgs[i] && image_chroma_up(alpha_imgs[i]->img).mode != 0))
        return fail(HEIFGPU_E_UNSUPPORTED, "gain-map render of an image set to bilinear chroma upsampling");
    heifgpu_image_info info, ginfo;
    heifgpu_image_get_info(imgs[i], &info);
    heifgpu_image_get_info(gain_imgs[i], &ginfo);
    if (t.bits != info.bit_depth) return fail(HEIFGPU_E_INVALID, "gain transform made for another depth than the base image's");
    if (t.gain_bits != ginfo.bit_depth) return fail(HEIFGPU_E_INVALID, "gain transform made for another depth than the gain map's");
    const uint32_t lim = uint32_t(kGainMaxSide);
    if (info.width > lim || info.height > lim || ginfo.width > lim || ginfo.height > lim)
        return fail(HEIFGPU_E_UNSUPPORTED, "gain-map render of a side above 65535");
    // the map is sampled at decoded base positions: its own display map must say nothing, or the same
    const DisplayMap &dm = bi.display, &gm = gi.display;
    const bool ident = gm.m[0] == 1 && gm.m[1] == 0 && gm.m[2] == 0 && gm.m[3] == 1 && gm.t[0] == 0 && gm.t[1] == 0 &&
                       gm.out_width == gi.out_width && gm.out_height == gi.out_height;
    const bool same = std::memcmp(gm.m, dm.m, sizeof(dm.m)) == 0 && gm.t[0] == dm.t[0] && gm.t[1] == dm.t[1] &&
                      gm.out_width == dm.out_width && gm.out_height == dm.out_height;
    // (the base's irot / imir over the map's own whole picture, as Apple's files carry them, is the base's map at the map's size)
    const bool turned = std::memcmp(gm.m, dm.m, sizeof(dm.m)) == 0 &&
                        uint64_t(gm.out_width) * gm.out_height == uint64_t(gi.out_width) * gi.out_height;
    if (!ident && !same && !turned)
        return fail(HEIFGPU_E_UNSUPPORTED, "gain image with a display map that is neither the identity nor the base's");
    if (!gain_in[i].plane[0]) return fail(HEIFGPU_E_INVALID, "missing gain plane");
    if (int64_t(gain_in[i].pitch[0]) < int64_t(ginfo.width) * ginfo.bytes_per_sample)
        return fail(HEIFGPU_E_INVALID, "gain plane pitch smaller than its row");
    // (the alpha image may be of another sample width here: convert() reads it by alpha_bps)
    abits = 0;
    if (with_alpha && alpha_imgs && alpha_imgs[i]) {
        heifgpu_image_info ai;
        heifgpu_image_get_info(alpha_imgs[i], &ai);
        abits = ai.bit_depth;
        if (!alpha_in || !alpha_in[i].plane[0]) return fail(HEIFGPU_E_INVALID, "missing alpha plane");
        if (ai.width != info.width || ai.height != info.height)
            return fail(HEIFGPU_E_UNSUPPORTED, "alpha image of another size than its colour image");
        if (abits > 12) return fail(HEIFGPU_E_UNSUPPORTED, "alpha image deeper than 12 bits");
        if (int64_t(alpha_in[i].pitch[0]) < int64_t(ai.width) * ai.bytes_per_sample)
            return fail(HEIFGPU_E_INVALID, "alpha plane pitch smaller than its row");
    }
    g = GainRef{};
    gain_map_fill(gain_in[i], info, ginfo, t.gain_bits, g);
    if (gd) gain_map_fill(gain_in[i], info, ginfo, t.gain_bits, *gd);
    g.n = 1 << t.bits;
    for (int k = 0; k < 9; ++k) g.m[k] = t.m[k];
    g.k_b = t.k_b, g.k_a = t.k_a;
    g.maxp = pq ? int32_t((1u << t.pq_bits) - 1) : 0;
    g.alpha_shift = pq && abits ? int32_t(abits) - int32_t(t.pq_bits) : 0;
    g.alpha_scale = abits ? 1.0f / float((1u << abits) - 1) : 1.0f;
    return HEIFGPU_OK;
}

// the alpha image of a gain-map render in its descriptor (gain_image_fill has checked it)
static void gain_alpha_fill(const heifgpu_image *alpha_img, const heifgpu_planes &alpha_in, RenderDesc &d) {
    heifgpu_image_info ai;
    heifgpu_image_get_info(alpha_img, &ai);
    d.alpha = reinterpret_cast<uint64_t>(alpha_in.plane[0]);
    d.alpha_pitch = alpha_in.pitch[0];
    d.alpha_bps = int32_t(ai.bytes_per_sample);
    d.alpha_shift = 0;  // the sample as decoded: the GainRef says where it goes
}

// What the two gain-map renders end in, for Desc = RenderDesc or GainScaleDesc: the context, the
// tables of the transforms out of the context's cache into the GainRefs, and the submit with the
// GainRefs behind the descriptors.
template <class Desc, class Launch>
static int gain_submit(heifgpu_ctx *ctx, const std::vector<Desc> &descs, std::vector<GainRef> &refs,
                       const heifgpu_gain_transform *const *xf, Launch launch, void *stream) {
    if (!ctx) return fail(HEIFGPU_E_INVALID, "null context");
    ColorCache *cache = nullptr;
    if (int rc = color_cache_open(ctx, cache)) return rc;
    std::vector<uint16_t> key;
    for (size_t i = 0; i < refs.size(); ++i) {
        gain_table_image(*xf[i], key, refs[i].t_off, refs[i].e_off);
        if (int rc = cache->table(key, "gain", refs[i].lut)) return rc;
    }
    return submit(ctx, descs, {{refs.data(), refs.size() * sizeof(GainRef)}}, launch, stream);
}

int heifgpu_render_batch_gain(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *in,
                              const heifgpu_image *const *gain_imgs, const heifgpu_planes *gain_in,
                              const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in, uint32_t format,
                              const heifgpu_gain_transform *const *xf, const heifgpu_surface *out, void *stream) {
    static_assert(HEIFGPU_PIX_HDR_RGB16F - 4 == GAIN_RGB16F && HEIFGPU_PIX_HDR_RGBA16PQ - 4 == GAIN_RGBA16PQ, "HDR formats");
    if (int rc = call_check(imgs && in && gain_imgs && gain_in && xf && out, n,
                            format_outside(format, HEIFGPU_PIX_HDR_RGB16F, HEIFGPU_PIX_HDR_RGBA16PQ)))
        return rc;
    const int hf = int(format) - 4;  // k_render_gain's: GAIN_*
    const bool pq = (hf & 2) != 0, with_alpha = (hf & 1) != 0;
    const uint32_t wide = with_alpha ? HEIFGPU_PIX_RGBA16 : HEIFGPU_PIX_RGB16;  // what the descriptors are filled for
    std::vector<RenderDesc> descs(n);
    std::vector<GainRef> refs(n);
    int bps = 0, max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t abits = 0;
        if (int rc = gain_image_fill(i, imgs, gain_imgs, gain_in, alpha_imgs, alpha_in, pq, with_alpha, xf, refs[i], nullptr,
                                     abits))
            return rc;
        const DisplayMap &dm = imgs[i]->img.display;
        RenderDesc &d = descs[i];
        if (int rc = render_desc_fill(i, imgs, in, nullptr, nullptr, wide, out, dm, dm.out_width, dm.out_height, bps, d))
            return rc;
        if (abits) gain_alpha_fill(alpha_imgs[i], alpha_in[i], d);
        max_tiles = std::max(max_tiles, full_size_tiles(d));
    }
    const int nn = int(n);
    return gain_submit(ctx, descs, refs, xf,
                       [=](const RenderDesc *dev, hipStream_t s) { return launch_render_gain(dev, nn, max_tiles, hf, bps, s); },
                       stream);
}

// heifgpu_render_batch_gain onto another grid (k_render_gain_scaled): its checks, then those of
// heifgpu_render_batch_scaled for the heifgpu_scale, all before anything is launched.
int heifgpu_render_batch_gain_scaled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                     const heifgpu_planes *in, const heifgpu_image *const *gain_imgs,
                                     const heifgpu_planes *gain_in, const heifgpu_image *const *alpha_imgs,
                                     const heifgpu_planes *alpha_in, uint32_t format, const heifgpu_scale *scales,
                                     const heifgpu_gain_transform *const *xf, const heifgpu_surface *out, void *stream) {
    if (int rc = call_check(imgs && in && gain_imgs && gain_in && scales && xf && out, n,
                            format_outside(format, HEIFGPU_PIX_HDR_RGB16F, HEIFGPU_PIX_HDR_RGBA16PQ)))
        return rc;
    const int hf = int(format) - 4;  // k_render_gain's: GAIN_*
    const bool pq = (hf & 2) != 0, with_alpha = (hf & 1) != 0;
    const uint32_t wide = with_alpha ? HEIFGPU_PIX_RGBA16 : HEIFGPU_PIX_RGB16;  // what the descriptors are filled for
    std::vector<GainScaleDesc> descs(n);
    std::vector<GainRef> refs(n);
    int bps = 0, max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t abits = 0;
        GainScaleDesc &gd = descs[i];
        if (int rc = gain_image_fill(i, imgs, gain_imgs, gain_in, alpha_imgs, alpha_in, pq, with_alpha, xf, refs[i], &gd,
                                     abits))
            return rc;
        if (int rc = scale_desc_fill(i, imgs, in, nullptr, nullptr, wide, scales[i], 0, out, bps, gd.s)) return rc;
        if (abits) gain_alpha_fill(alpha_imgs[i], alpha_in[i], gd.s.r);
        max_tiles = std::max(max_tiles, gd.s.r.tiles);
    }
    const int nn = int(n);
    return gain_submit(ctx, descs, refs, xf,
                       [=](const GainScaleDesc *dev, hipStream_t s) {
                           return launch_render_gain_scaled(dev, nn, max_tiles, hf, bps, s);
                       },
                       stream);
}
