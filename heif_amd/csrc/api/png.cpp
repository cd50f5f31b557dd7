// png.cpp — the PNG output of the C ABI: the bytes before the first IDAT and the host
// restatement of the whole encoder (host only), and heifgpu_png_encode_batch, which checks its
// arguments, plans the batch and sends it through kernels/png.hip's four launches.  The file's
// layout, the filters and the code construction are kernels/png.hpp's.
// (The calls take their C linkage from the declarations of include/heifgpu.h.)
#include <memory>
#include <vector>

#include "../kernels/png.hpp"
#include "api.hpp"

using namespace hg;

// The encoder's scratch (filtered streams, block records, offsets, Adler-32 words) and its
// descriptors' staging, reused from call to call: a call waits for the previous one's kernels
// before it touches them.
struct PngState {
    DevBuf<uint8_t> stream;
    DevBuf<PngBlk> blk;
    DevBuf<uint64_t> boff;
    DevBuf<uint32_t> adler;
    DevBuf<PngPic> pics;
    PinnedBuf host;
    hipEvent_t done = nullptr;
    bool pending = false;
    ~PngState() {
        if (done) (void)hipEventDestroy(done);
    }
};

void hg::png_state_free(heifgpu_ctx *ctx) { delete ctx->png; }

namespace {

constexpr size_t kIccMax = 0x7fff0000u;

const char *opts_error(const heifgpu_png_opts *o) {
    if (!o) return "null options";
    if (o->format > HEIFGPU_PIX_RGBA16) return "format: one of the four render formats";
    if (o->format < HEIFGPU_PIX_RGB16 ? o->bits != 8 : (o->bits < 8 || o->bits > 16))
        return "bits: 8 for the 8-bit formats, 8..16 for the 16-bit ones";
    if (o->filter > 5) return "filter above 5";
    if (o->reserved) return "reserved must be 0";
    return nullptr;
}
const char *size_error(uint32_t w, uint32_t h) {
    if (w == 0 || h == 0) return "a side of zero";
    if (w > uint32_t(kPngMaxSide) || h > uint32_t(kPngMaxSide)) return "a side above 65535";
    return nullptr;
}
const char *colour_error(const heifgpu_png_colour *c) {
    if (!c) return nullptr;
    if (c->kind > HEIFGPU_PNG_COLOUR_ICC) return "colour kind";
    if (c->kind == HEIFGPU_PNG_COLOUR_ICC && (!c->icc || c->icc_len == 0 || c->icc_len > kIccMax))
        return "profile: 1..0x7fff0000 bytes";
    return nullptr;
}

uint32_t crc_of(const uint8_t *p, size_t n) {
    uint32_t reg = ~0u;
    for (size_t i = 0; i < n; ++i) reg = png_crc_step(reg, p[i]);
    return ~reg;
}

struct Bytes {
    std::vector<uint8_t> v;
    void u8(uint32_t b) { v.push_back(uint8_t(b)); }
    void u16le(uint32_t x) { u8(x & 0xff), u8(x >> 8 & 0xff); }
    void u32(uint32_t x) { u8(x >> 24), u8(x >> 16 & 0xff), u8(x >> 8 & 0xff), u8(x & 0xff); }
    void put(const void *p, size_t n) { v.insert(v.end(), static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + n); }
    // a chunk: begin() before its data, end() after
    size_t begin(const char *type) {
        u32(0);
        put(type, 4);
        return v.size();
    }
    void end(size_t data) {
        const uint32_t n = uint32_t(v.size() - data);
        for (int i = 0; i < 4; ++i) v[data - 8 + size_t(i)] = uint8_t(n >> (24 - 8 * i));
        u32(crc_of(v.data() + data - 4, n + 4));
    }
};

void header_bytes(uint32_t w, uint32_t h, const heifgpu_png_opts &o, const heifgpu_png_colour *c, Bytes &b) {
    const int fmt = int(o.format);
    b.put("\x89PNG\r\n\x1a\n", 8);
    size_t d = b.begin("IHDR");
    b.u32(w), b.u32(h), b.u8(png_wide(fmt) ? 16 : 8), b.u8(png_channels(fmt) == 4 ? 6 : 2), b.u8(0), b.u8(0), b.u8(0);
    b.end(d);
    if (png_wide(fmt) && o.bits < 16) {
        d = b.begin("sBIT");
        for (int i = 0; i < png_channels(fmt); ++i) b.u8(o.bits);
        b.end(d);
    }
    if (c && c->kind == HEIFGPU_PNG_COLOUR_SRGB) {
        d = b.begin("sRGB");
        b.u8(0);
        b.end(d);
    } else if (c && c->kind == HEIFGPU_PNG_COLOUR_CICP) {
        d = b.begin("cICP");
        b.put(c->cicp, 4);
        b.end(d);
    } else if (c && c->kind == HEIFGPU_PNG_COLOUR_ICC) {
        d = b.begin("iCCP");
        b.put("ICC profile\0", 13);  // the name, its terminator and compression method 0
        b.u8(0x78), b.u8(0x01);
        uint32_t ad_a = 1, ad_b = 0;
        for (size_t at = 0; at < c->icc_len; at += 65535) {
            const size_t n = std::min<size_t>(65535, c->icc_len - at);
            b.u8(at + n == c->icc_len ? 1 : 0);
            b.u16le(uint32_t(n)), b.u16le(uint32_t(n) ^ 0xffffu);
            b.put(c->icc + at, n);
            uint32_t s1 = 0;
            uint64_t s2 = 0;
            for (size_t i = 0; i < n; ++i) s1 += c->icc[at + i], s2 += uint64_t(n - i) * c->icc[at + i];
            png_adler_join(ad_a, ad_b, s1 % kPngAdlerMod, uint32_t(s2 % kPngAdlerMod), uint32_t(n));
        }
        b.u32(ad_b << 16 | ad_a);
        b.end(d);
    }
}

int give(const std::vector<uint8_t> &v, uint8_t *buf, size_t cap, size_t *len) {
    *len = v.size();
    if (buf && cap >= v.size()) std::memcpy(buf, v.data(), v.size());
    return HEIFGPU_OK;
}

uint32_t bpp_of(const heifgpu_png_opts &o) { return uint32_t(png_bpp(int(o.format))); }

}  // namespace

int heifgpu_png_header(uint32_t w, uint32_t h, const heifgpu_png_opts *opts, const heifgpu_png_colour *colour,
                       uint8_t *buf, size_t cap, size_t *len) {
    if (!len) return fail(HEIFGPU_E_INVALID, "null argument");
    if (const char *e = opts_error(opts)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = size_error(w, h)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = colour_error(colour)) return fail(HEIFGPU_E_INVALID, e);
    Bytes b;
    header_bytes(w, h, *opts, colour, b);
    return give(b.v, buf, cap, len);
}

int heifgpu_png_encode_host(const void *pixels, int32_t pitch, uint32_t w, uint32_t h, const heifgpu_png_opts *opts,
                            const heifgpu_png_colour *colour, uint8_t *buf, size_t cap, size_t *len) {
    if (!pixels || !len) return fail(HEIFGPU_E_INVALID, "null argument");
    if (const char *e = opts_error(opts)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = size_error(w, h)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = colour_error(colour)) return fail(HEIFGPU_E_INVALID, e);
    if (pitch < 0 || uint32_t(pitch) < bpp_of(*opts) * w) return fail(HEIFGPU_E_INVALID, "pitch below width * bytes per pixel");
    Bytes b;
    header_bytes(w, h, *opts, colour, b);
    const int fmt = int(opts->format), bpp = png_bpp(fmt), wide = png_wide(fmt), bits = int(opts->bits);
    PngPic p{};
    p.w = w, p.h = h;
    uint64_t n_stream, n_blk;
    uint32_t mh, mb;
    png_plan(&p, 1, fmt, n_stream, n_blk, mh, mb);
    // the filtered stream
    std::vector<uint8_t> stream(p.len);
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t *row = static_cast<const uint8_t *>(pixels) + size_t(y) * size_t(pitch);
        const uint8_t *up = y ? row - pitch : nullptr;
        int t = int(opts->filter);
        if (t == kPngAdaptive) {
            uint32_t sum[5] = {0, 0, 0, 0, 0};
            for (uint32_t i = 0; i < p.row; ++i) {
                const PngNeigh q = png_neigh(row, up, i, bpp, wide, bits);
                for (int f = 0; f < 5; ++f) sum[f] += png_magnitude(png_filter_byte(f, q.x, q.a, q.b, q.c));
            }
            t = png_pick_filter(sum);
        }
        uint8_t *dst = stream.data() + size_t(y) * (size_t(p.row) + 1);
        dst[0] = uint8_t(t);
        for (uint32_t i = 0; i < p.row; ++i) {
            const PngNeigh q = png_neigh(row, up, i, bpp, wide, bits);
            dst[1 + i] = uint8_t(png_filter_byte(t, q.x, q.a, q.b, q.c));
        }
    }
    // block by block: counts, lengths, codes, the chunk in a zeroed word buffer
    auto work = std::make_unique<PngHuffWork>();
    std::vector<uint32_t> words;
    uint32_t ad_a = 1, ad_b = 0;
    for (uint32_t k = 0; k < p.n_blk; ++k) {
        const uint8_t *d = stream.data() + size_t(k) * kPngBlock;
        const uint32_t blen = uint32_t(std::min<uint64_t>(kPngBlock, p.len - uint64_t(k) * kPngBlock));
        const bool first = k == 0, last = k + 1 == p.n_blk;
        uint32_t cnt[kPngLit] = {}, clcnt[kPngCl] = {}, e[kPngLit], ecl[kPngCl];
        uint16_t order[kPngLit], clorder[kPngCl];
        uint8_t litlen[kPngLit], cllen[kPngCl];
        uint32_t s1 = 0;
        uint64_t s2 = 0;
        for (uint32_t i = 0; i < blen; ++i) cnt[d[i]] += 1, s1 += d[i], s2 += uint64_t(blen - i) * d[i];
        cnt[256] = 1;
        png_adler_join(ad_a, ad_b, s1 % kPngAdlerMod, uint32_t(s2 % kPngAdlerMod), blen);
        for (int s = 0; s < kPngLit; ++s) order[png_rank(cnt, kPngLit, s)] = uint16_t(s);
        png_lengths(cnt, order, kPngLit, kPngLitMax, litlen, *work);
        for (int s = 0; s < kPngLit; ++s) clcnt[litlen[s]] += 1;
        clcnt[1] += 1;
        for (int s = 0; s < kPngCl; ++s) clorder[png_rank(clcnt, kPngCl, s)] = uint16_t(s);
        png_lengths(clcnt, clorder, kPngCl, kPngClMax, cllen, *work);
        png_codes(litlen, kPngLit, kPngLitMax, e, *work);
        png_codes(cllen, kPngCl, kPngClMax, ecl, *work);
        uint32_t data = 0;
        for (int s = 0; s < kPngLit; ++s) data += cnt[s] * litlen[s];
        const uint32_t total = png_chunk_bytes(png_head_bits(litlen, cllen), data, first, last);
        words.assign((total + 3) / 4 + 1, 0);
        uint32_t *wp = words.data();
        png_put_be32(wp, 0, total - 12 - (last ? 12u : 0u));
        png_put_be32(wp, 4, 0x49444154u);
        if (first) png_put_byte(wp, 8, 0x78), png_put_byte(wp, 9, 0x01);
        PngSink s = png_sink(wp, 8 * (8 + (first ? 2u : 0u)));
        png_put_head(s, litlen, cllen, ecl);
        for (uint32_t i = 0; i < blen; ++i) png_put_code(s, e[d[i]]);
        png_put_code(s, e[256]);
        png_put(s, last ? 1u : 0u, 3);
        png_flush(s);
        uint32_t pos = total - 4 - (last ? 16u : 0u) - 4;  // of 00 00 FF FF
        png_put_byte(wp, pos + 2, 0xff), png_put_byte(wp, pos + 3, 0xff);
        pos += 4;
        if (last) png_put_be32(wp, pos, ad_b << 16 | ad_a), pos += 4;
        uint32_t reg = ~0u;
        for (uint32_t i = 4; i < pos; ++i) reg = png_crc_step(reg, png_get_byte(wp, i));
        png_put_be32(wp, pos, ~reg);
        if (last) png_put_be32(wp, pos + 8, 0x49454e44u), png_put_be32(wp, pos + 12, 0xae426082u);
        for (uint32_t i = 0; i < total; ++i) b.u8(png_get_byte(wp, i));
    }
    return give(b.v, buf, cap, len);
}

int heifgpu_png_encode_batch(heifgpu_ctx *ctx, size_t n, const heifgpu_surface *surfaces, const uint32_t *w,
                             const uint32_t *h, const heifgpu_png_opts *opts, const heifgpu_surface *out,
                             uint64_t *sizes, void *stream) {
    if (!ctx || !surfaces || !w || !h || !out || !sizes || n == 0) return fail(HEIFGPU_E_INVALID, "invalid argument");
    if (n > 65535) return fail(HEIFGPU_E_INVALID, "more than 65535 pictures in one encode call");
    if (const char *e = opts_error(opts)) return fail(HEIFGPU_E_INVALID, e);
    std::vector<PngPic> pics(n);
    for (size_t i = 0; i < n; ++i) {
        if (const char *e = size_error(w[i], h[i])) return fail(HEIFGPU_E_INVALID, e);
        if (!surfaces[i].pixels) return fail(HEIFGPU_E_INVALID, "null surface");
        if (surfaces[i].pitch < 0 || uint32_t(surfaces[i].pitch) < bpp_of(*opts) * w[i])
            return fail(HEIFGPU_E_INVALID, "pitch below width * bytes per pixel");
        if (out[i].pitch < 0 || (out[i].pitch > 0 && !out[i].pixels)) return fail(HEIFGPU_E_INVALID, "output buffer");
        PngPic &p = pics[i];
        p = PngPic{};
        p.px = static_cast<const uint8_t *>(surfaces[i].pixels);
        p.out = static_cast<uint8_t *>(out[i].pixels);
        p.pitch = surfaces[i].pitch;
        p.cap = uint64_t(out[i].pitch);
        p.w = w[i], p.h = h[i];
    }
    uint64_t n_stream, n_blk;
    uint32_t max_h, max_blk;
    png_plan(pics.data(), int(n), int(opts->format), n_stream, n_blk, max_h, max_blk);

    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->png) {
        auto st = std::make_unique<PngState>();
        HIP_TRY(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
        ctx->png = st.release();
    }
    PngState &st = *ctx->png;
    if (st.pending) HIP_TRY(hipEventSynchronize(st.done));  // the previous call's kernels: the scratch is theirs
    st.pending = false;
    HIP_TRY(st.stream.alloc(n_stream));
    HIP_TRY(st.blk.alloc(n_blk));
    HIP_TRY(st.boff.alloc(n_blk));
    HIP_TRY(st.adler.alloc(n));
    HIP_TRY(st.pics.alloc(n));
    HIP_TRY(st.host.reserve(n * sizeof(PngPic)));
    std::memcpy(st.host.p, pics.data(), n * sizeof(PngPic));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(st.pics.p, st.host.p, n * sizeof(PngPic), hipMemcpyHostToDevice, s));
    PngArgs a{};
    a.pics = st.pics.p;
    a.stream = st.stream.p;
    a.blk = st.blk.p;
    a.boff = st.boff.p;
    a.adler = st.adler.p;
    a.sizes = sizes;
    a.n = int(n);
    a.fmt = int(opts->format);
    a.bits = int(opts->bits);
    a.filter = int(opts->filter);
    HIP_TRY(launch_png_encode(a, max_h, max_blk, s));
    HIP_TRY(hipEventRecord(st.done, s));
    st.pending = true;
    return HEIFGPU_OK;
}
