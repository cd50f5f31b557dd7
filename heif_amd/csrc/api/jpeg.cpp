// jpeg.cpp — the JPEG output of the C ABI: the quantisation tables, the header bytes and
// the host restatement of the whole encoder (host only), and heifgpu_jpeg_encode_batch, which
// checks its arguments, plans the batch and sends it through kernels/jpeg.hip's four launches.
// The arithmetic and the file's layout are kernels/jpeg.hpp's.
// (The calls take their C linkage from the declarations of include/heifgpu.h.)
#include <memory>
#include <vector>

#include "../kernels/jpeg.hpp"
#include "api.hpp"

using namespace hg;

// The encoder's scratch (coefficients, interval sizes and offsets) and its descriptors' staging,
// reused from call to call: a call waits for the previous one's kernels before it touches them.
struct JpegState {
    DevBuf<int16_t> coef;
    DevBuf<uint32_t> ilen;
    DevBuf<uint64_t> ioff;
    DevBuf<JpegPic> pics;
    PinnedBuf host;
    hipEvent_t done = nullptr;
    bool pending = false;
    ~JpegState() {
        if (done) (void)hipEventDestroy(done);
    }
};

void hg::jpeg_state_free(heifgpu_ctx *ctx) { delete ctx->jpeg; }

namespace {

constexpr size_t kIccChunk = 65519;

const char *opts_error(const heifgpu_jpeg_opts *o) {
    if (!o) return "null options";
    if (o->quality < 1 || o->quality > 100) return "quality outside 1..100";
    if (o->subsampling > HEIFGPU_JPEG_420) return "subsampling";
    if (o->restart_mcus > 65535) return "restart_mcus above 65535";
    return nullptr;
}
const char *size_error(uint32_t w, uint32_t h) {
    if (w == 0 || h == 0) return "a side of zero";
    if (w > uint32_t(kJpegMaxSide) || h > uint32_t(kJpegMaxSide)) return "a side above 65535";
    return nullptr;
}

void quant_tables(uint32_t quality, uint8_t qt[2][64]) {
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) qt[t][i] = jpeg_quant_scale(kJpegBaseQ[t][i], int(quality));
}

struct Bytes {
    std::vector<uint8_t> v;
    void u8(uint32_t b) { v.push_back(uint8_t(b)); }
    void u16(uint32_t w) { u8(w >> 8), u8(w & 0xff); }
    void seg(uint32_t marker, size_t payload) { u8(0xff), u8(marker), u16(uint32_t(payload + 2)); }
    void put(const void *p, size_t n) { v.insert(v.end(), static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + n); }
};

void header_bytes(uint32_t w, uint32_t h, const heifgpu_jpeg_opts &o, const uint8_t *icc, size_t icc_len, Bytes &b) {
    const int sub = int(o.subsampling);
    b.u8(0xff), b.u8(0xd8);
    b.seg(0xe0, 14);
    b.put("JFIF\0\1\1\0\0\1\0\1\0\0", 14);
    const size_t chunks = (icc_len + kIccChunk - 1) / kIccChunk;
    for (size_t c = 0; c < chunks; ++c) {
        const size_t n = std::min(kIccChunk, icc_len - c * kIccChunk);
        b.seg(0xe2, 14 + n);
        b.put("ICC_PROFILE\0", 12);
        b.u8(uint32_t(c + 1)), b.u8(uint32_t(chunks));
        b.put(icc + c * kIccChunk, n);
    }
    uint8_t qt[2][64];
    quant_tables(o.quality, qt);
    for (int t = 0; t < 2; ++t) {
        b.seg(0xdb, 65);
        b.u8(uint32_t(t));
        for (int k = 0; k < 64; ++k) b.u8(qt[t][kZigzag[k]]);
    }
    b.seg(0xc0, 15);
    b.u8(8), b.u16(h), b.u16(w), b.u8(3);
    b.u8(1), b.u8(sub == JPEG_420 ? 0x22 : 0x11), b.u8(0);
    b.u8(2), b.u8(0x11), b.u8(1);
    b.u8(3), b.u8(0x11), b.u8(1);
    for (int t = 0; t < 2; ++t) {
        b.seg(0xc4, 17 + 12);
        b.u8(uint32_t(t)), b.put(kBitsDc[t], 16), b.put(kValsDc, 12);
        b.seg(0xc4, 17 + 162);
        b.u8(0x10u | uint32_t(t)), b.put(kBitsAc[t], 16), b.put(kValsAc[t], 162);
    }
    const uint32_t mcu = sub == JPEG_420 ? 16 : 8;
    b.seg(0xdd, 2);
    b.u16(o.restart_mcus ? o.restart_mcus : (w + mcu - 1) / mcu);
    b.seg(0xda, 10);
    b.put("\3\1\0\2\x11\3\x11\0\x3f\0", 10);
}

int give(const std::vector<uint8_t> &v, uint8_t *buf, size_t cap, size_t *len) {
    *len = v.size();
    if (buf && cap >= v.size()) std::memcpy(buf, v.data(), v.size());
    return HEIFGPU_OK;
}

const char *icc_error(const uint8_t *icc, size_t icc_len) {
    if (icc_len && !icc) return "null profile";
    if (icc_len > 255 * kIccChunk) return "profile above 255 chunks";
    return nullptr;
}

}  // namespace

int heifgpu_jpeg_quant_tables(uint32_t quality, uint8_t luma[64], uint8_t chroma[64]) {
    if (!luma || !chroma) return fail(HEIFGPU_E_INVALID, "null argument");
    if (quality < 1 || quality > 100) return fail(HEIFGPU_E_INVALID, "quality outside 1..100");
    uint8_t qt[2][64];
    quant_tables(quality, qt);
    std::memcpy(luma, qt[0], 64);
    std::memcpy(chroma, qt[1], 64);
    return HEIFGPU_OK;
}

int heifgpu_jpeg_header(uint32_t w, uint32_t h, const heifgpu_jpeg_opts *opts, const uint8_t *icc, size_t icc_len,
                        uint8_t *buf, size_t cap, size_t *len) {
    if (!len) return fail(HEIFGPU_E_INVALID, "null argument");
    if (const char *e = opts_error(opts)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = size_error(w, h)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = icc_error(icc, icc_len)) return fail(HEIFGPU_E_INVALID, e);
    Bytes b;
    header_bytes(w, h, *opts, icc, icc_len, b);
    return give(b.v, buf, cap, len);
}

int heifgpu_jpeg_encode_host(const uint8_t *rgb, int32_t pitch, uint32_t w, uint32_t h, const heifgpu_jpeg_opts *opts,
                             const uint8_t *icc, size_t icc_len, uint8_t *buf, size_t cap, size_t *len) {
    if (!rgb || !len) return fail(HEIFGPU_E_INVALID, "null argument");
    if (const char *e = opts_error(opts)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = size_error(w, h)) return fail(HEIFGPU_E_INVALID, e);
    if (const char *e = icc_error(icc, icc_len)) return fail(HEIFGPU_E_INVALID, e);
    if (pitch < 0 || uint32_t(pitch) < 3 * w) return fail(HEIFGPU_E_INVALID, "pitch below 3 * width");
    Bytes b;
    header_bytes(w, h, *opts, icc, icc_len, b);
    const int sub = int(opts->subsampling);
    JpegPic p{};
    p.w = w, p.h = h;
    uint64_t n_coef, n_int;
    uint32_t mg, mi;
    jpeg_plan(&p, 1, sub, opts->restart_mcus, n_coef, n_int, mg, mi);
    uint8_t qt[2][64];
    quant_tables(opts->quality, qt);
    const int mcu = sub == JPEG_420 ? 16 : 8, bpm = sub == JPEG_420 ? 6 : 3;
    std::vector<int16_t> coef(n_coef);
    // component c of the extended picture at (x, y)
    auto at = [&](uint32_t x, uint32_t y, int c) {
        return jpeg_ycc(rgb + size_t(std::min(y, h - 1)) * size_t(pitch) + size_t(std::min(x, w - 1)) * 3, c);
    };
    size_t blk = 0;
    for (uint32_t my = 0; my < p.mcus_y; ++my)
        for (uint32_t mx = 0; mx < p.mcus_x; ++mx)
            for (int j = 0; j < bpm; ++j, ++blk) {
                const int comp = sub == JPEG_420 ? (j < 4 ? 0 : j - 3) : j;
                int32_t s[64];
                for (int k = 0; k < 64; ++k) {
                    const uint32_t bx = uint32_t(k & 7), by = uint32_t(k >> 3);
                    int v;
                    if (sub == JPEG_420 && comp) {
                        const uint32_t x = mx * 16 + 2 * bx, y = my * 16 + 2 * by;
                        v = (at(x, y, comp) + at(x + 1, y, comp) + at(x, y + 1, comp) + at(x + 1, y + 1, comp) + 2) >> 2;
                    } else if (sub == JPEG_420) {
                        v = at(mx * 16 + uint32_t(j & 1) * 8 + bx, my * 16 + uint32_t(j >> 1) * 8 + by, 0);
                    } else {
                        v = at(mx * uint32_t(mcu) + bx, my * uint32_t(mcu) + by, comp);
                    }
                    s[k] = v - 128;
                }
                for (int r = 0; r < 8; ++r) jpeg_dct_row(s + 8 * r);
                for (int c = 0; c < 8; ++c) jpeg_dct_col(s + c, 8);
                for (int k = 0; k < 64; ++k)
                    coef[blk * 64 + size_t(k)] = int16_t(jpeg_quantise(s[kZigzag[k]], qt[comp ? 1 : 0][kZigzag[k]]));
            }
    const uint64_t mcus = uint64_t(p.mcus_x) * p.mcus_y;
    for (uint32_t i = 0; i < p.n_int; ++i) {
        const uint64_t m0 = uint64_t(i) * p.ri, m1 = std::min(m0 + p.ri, mcus);
        const uint32_t marker = i + 1 < p.n_int ? 0xd0u + (i & 7u) : 0xd9u;
        JpegSink<false> count{nullptr, 0, 0, 0, 0};
        jpeg_put_interval(count, coef.data(), uint32_t(m0), uint32_t(m1), sub, marker);
        const size_t at0 = b.v.size();
        b.v.resize(at0 + count.pos);
        JpegSink<true> sink{b.v.data() + at0, 0, count.pos, 0, 0};
        jpeg_put_interval(sink, coef.data(), uint32_t(m0), uint32_t(m1), sub, marker);
    }
    return give(b.v, buf, cap, len);
}

int heifgpu_jpeg_encode_batch(heifgpu_ctx *ctx, size_t n, const heifgpu_surface *rgb, const uint32_t *w,
                              const uint32_t *h, const heifgpu_jpeg_opts *opts, const heifgpu_surface *out,
                              uint64_t *sizes, void *stream) {
    if (!ctx || !rgb || !w || !h || !out || !sizes || n == 0) return fail(HEIFGPU_E_INVALID, "invalid argument");
    if (n > 65535) return fail(HEIFGPU_E_INVALID, "more than 65535 pictures in one encode call");
    if (const char *e = opts_error(opts)) return fail(HEIFGPU_E_INVALID, e);
    std::vector<JpegPic> pics(n);
    for (size_t i = 0; i < n; ++i) {
        if (const char *e = size_error(w[i], h[i])) return fail(HEIFGPU_E_INVALID, e);
        if (!rgb[i].pixels) return fail(HEIFGPU_E_INVALID, "null surface");
        if (rgb[i].pitch < 0 || uint32_t(rgb[i].pitch) < 3 * w[i]) return fail(HEIFGPU_E_INVALID, "pitch below 3 * width");
        if (out[i].pitch < 0 || (out[i].pitch > 0 && !out[i].pixels)) return fail(HEIFGPU_E_INVALID, "output buffer");
        JpegPic &p = pics[i];
        p = JpegPic{};
        p.rgb = static_cast<const uint8_t *>(rgb[i].pixels);
        p.out = static_cast<uint8_t *>(out[i].pixels);
        p.pitch = rgb[i].pitch;
        p.cap = uint64_t(out[i].pitch);
        p.w = w[i], p.h = h[i];
    }
    uint64_t n_coef, n_int;
    uint32_t max_groups, max_int;
    jpeg_plan(pics.data(), int(n), int(opts->subsampling), opts->restart_mcus, n_coef, n_int, max_groups, max_int);

    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->jpeg) {
        auto st = std::make_unique<JpegState>();
        HIP_TRY(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
        ctx->jpeg = st.release();
    }
    JpegState &st = *ctx->jpeg;
    if (st.pending) HIP_TRY(hipEventSynchronize(st.done));  // the previous call's kernels: the scratch is theirs
    st.pending = false;
    HIP_TRY(st.coef.alloc(n_coef));
    HIP_TRY(st.ilen.alloc(n_int));
    HIP_TRY(st.ioff.alloc(n_int));
    HIP_TRY(st.pics.alloc(n));
    HIP_TRY(st.host.reserve(n * sizeof(JpegPic)));
    std::memcpy(st.host.p, pics.data(), n * sizeof(JpegPic));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(st.pics.p, st.host.p, n * sizeof(JpegPic), hipMemcpyHostToDevice, s));
    JpegArgs a{};
    a.pics = st.pics.p;
    a.coef = st.coef.p;
    a.ilen = st.ilen.p;
    a.ioff = st.ioff.p;
    a.sizes = sizes;
    a.n = int(n);
    a.sub = int(opts->subsampling);
    quant_tables(opts->quality, a.qt);
    HIP_TRY(launch_jpeg_encode(a, max_groups, max_int, s));
    HIP_TRY(hipEventRecord(st.done, s));
    st.pending = true;
    return HEIFGPU_OK;
}
