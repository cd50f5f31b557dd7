// context.cpp — the context of the C ABI (its streams, events and stage timing) and the
// calls that need no batch: heifgpu_ycbcr_to_rgb, heifgpu_gather_tiles and IPC.
#include <memory>
#include <mutex>
#include <vector>

#include "api.hpp"

using namespace hg;

namespace {
// k_rbsp on its own stream (HEIFGPU_PREP_STREAM=0/1, read at context creation)
bool prep_stream_default() {
    const char *e = std::getenv("HEIFGPU_PREP_STREAM");
    return e && std::atoi(e) != 0;
}
}  // namespace

hipError_t hg::fold_timing(heifgpu_ctx *ctx, int slot) {
    hipEvent_t *e = ctx->tev[slot];
    hipError_t r = hipEventSynchronize(e[8]);
    if (r != hipSuccess) return r;
    float t = 0.f;
    if ((r = hipEventElapsedTime(&t, e[0], e[1])) != hipSuccess) return r;
    ctx->acc[5] += t;  // k_rbsp
    if ((r = hipEventElapsedTime(&t, e[9], e[2])) != hipSuccess) return r;
    ctx->acc[0] += t;  // k_parse
    if ((r = hipEventElapsedTime(&t, e[3], e[4])) != hipSuccess) return r;
    ctx->acc[1] += t;  // k_transform
    for (int i = 2; i < 5; ++i) {  // k_intra, k_deblock, k_sao_out
        if ((r = hipEventElapsedTime(&t, e[i + 3], e[i + 4])) != hipSuccess) return r;
        ctx->acc[i] += t;
    }
    return hipSuccess;
}

extern "C" {

int heifgpu_create(int device, heifgpu_ctx **out) {
    if (!out) return fail(HEIFGPU_E_INVALID, "null argument");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(HEIFGPU_E_DEVICE, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    auto c = std::make_unique<heifgpu_ctx>();
    c->device = device;
    c->stream = stream_knobs_from_env();
    // parse and reconstruction streams at the same priority: with the parse
    // stream at the highest priority (HEIFGPU_PARSE_PRIORITY=1) k_transform
    // starves beside it and the bench measured 1 % lower (two A/B pairs,
    // 14909 / 14881 vs 15039 / 15058 Mpix/s)
    static const bool prio = [] {
        const char *e = std::getenv("HEIFGPU_PARSE_PRIORITY");
        return e && std::atoi(e) != 0;
    }();
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamCreateWithPriority(&c->parse, hipStreamNonBlocking, prio ? greatest : least));
    // HEIFGPU_RECON_PRIORITY=1: the transform and reconstruction streams at the
    // highest priority instead (tuning knob; the recon stream sets the step)
    static const bool rprio = [] {
        const char *e = std::getenv("HEIFGPU_RECON_PRIORITY");
        return e && std::atoi(e) != 0;
    }();
    HIP_TRY(hipStreamCreateWithPriority(&c->xform, hipStreamNonBlocking, rprio ? greatest : least));
    HIP_TRY(hipStreamCreateWithPriority(&c->recon, hipStreamNonBlocking, rprio ? greatest : least));
    HIP_TRY(hipStreamCreateWithFlags(&c->upload, hipStreamNonBlocking));
    if (prep_stream_default()) HIP_TRY(hipStreamCreateWithFlags(&c->prep, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->join, hipEventDisableTiming));
    for (auto &row : c->tev)
        for (auto &e : row) HIP_TRY(hipEventCreate(&e));
    *out = c.release();
    return HEIFGPU_OK;
}

void heifgpu_destroy(heifgpu_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto &row : ctx->tev)
        for (auto &e : row)
            if (e) (void)hipEventDestroy(e);
    if (ctx->fork) (void)hipEventDestroy(ctx->fork);
    if (ctx->join) (void)hipEventDestroy(ctx->join);
    if (ctx->parse) (void)hipStreamDestroy(ctx->parse);
    if (ctx->xform) (void)hipStreamDestroy(ctx->xform);
    if (ctx->recon) (void)hipStreamDestroy(ctx->recon);
    if (ctx->upload) (void)hipStreamDestroy(ctx->upload);
    if (ctx->prep) (void)hipStreamDestroy(ctx->prep);
    render_state_free(ctx);
    jpeg_state_free(ctx);
    png_state_free(ctx);
    delete ctx;
}

int heifgpu_set_timing(heifgpu_ctx *ctx, int enable) {
    if (!ctx) return fail(HEIFGPU_E_INVALID, "null ctx");
    if (enable && !ctx->timing) {  // a fresh accumulation
        for (double &v : ctx->acc) v = 0.0;
        ctx->timed_calls = ctx->folded = 0;
    }
    ctx->timing = enable != 0;
    return HEIFGPU_OK;
}

int heifgpu_stage_times(heifgpu_ctx *ctx, float ms[6]) {
    if (!ctx || !ms) return fail(HEIFGPU_E_INVALID, "null argument");
    if (!ctx->timing) return fail(HEIFGPU_E_INVALID, "timing disabled");
    // mean per decode call over the timed calls since the previous query
    for (int i = 0; i < 6; ++i) ms[i] = 0.f;
    for (int c = ctx->folded; c < ctx->timed_calls; ++c) HIP_TRY(fold_timing(ctx, c % kTimingSlots));
    if (ctx->timed_calls)
        for (int i = 0; i < 6; ++i) ms[i] = float(ctx->acc[i] / ctx->timed_calls);
    for (double &v : ctx->acc) v = 0.0;
    ctx->timed_calls = ctx->folded = 0;
    return HEIFGPU_OK;
}

int heifgpu_ycbcr_to_rgb(heifgpu_ctx *ctx, const heifgpu_image_info *info, const heifgpu_planes *in, void *rgb,
                         int32_t rgb_pitch, void *stream) {
    if (!ctx || !info || !in || !rgb || !in->plane[0]) return fail(HEIFGPU_E_INVALID, "invalid argument");
    if (info->chroma_format_idc > 3) return fail(HEIFGPU_E_INVALID, "chroma_format_idc");
    if (info->chroma_format_idc && (!in->plane[1] || !in->plane[2])) return fail(HEIFGPU_E_INVALID, "missing chroma plane");
    if (info->bit_depth < 8 || info->bit_depth > 16) return fail(HEIFGPU_E_INVALID, "bit depth");
    HIP_TRY(hipSetDevice(ctx->device));
    ColorArgs c{};
    for (int k = 0; k < 3; ++k) {
        c.plane[k] = reinterpret_cast<uint64_t>(in->plane[k]);
        c.pitch[k] = in->pitch[k];
    }
    c.rgb = reinterpret_cast<uint64_t>(rgb);
    c.rgb_pitch = rgb_pitch;
    c.w = int32_t(info->width);
    c.h = int32_t(info->height);
    c.rotation = int32_t(info->rotation & 3);
    c.out_w = (c.rotation & 1) ? c.h : c.w;
    c.out_h = (c.rotation & 1) ? c.w : c.h;
    if (rgb_pitch < 3 * c.out_w) return fail(HEIFGPU_E_INVALID, "rgb_pitch smaller than 3 * output width");
    c.chroma = int32_t(info->chroma_format_idc);
    c.shift = int32_t(info->bit_depth) - 8;
    color_coefs(info->matrix_coeffs, info->full_range != 0, c);
    HIP_TRY(launch_ycbcr_rgb(c, int(info->bytes_per_sample), static_cast<hipStream_t>(stream)));
    return HEIFGPU_OK;
}

int heifgpu_gather_tiles(const heifgpu_image_info *info, const heifgpu_planes *dst, const heifgpu_planes *src,
                         uint32_t tile_stride, uint32_t tile_offset, void *stream) {
    if (!info || !dst || !src) return fail(HEIFGPU_E_INVALID, "null argument");
    if (tile_stride == 0) tile_stride = 1;
    if (tile_offset >= tile_stride) return fail(HEIFGPU_E_INVALID, "tile_offset must be below tile_stride");
    if (info->chroma_format_idc > 3) return fail(HEIFGPU_E_INVALID, "chroma_format_idc");
    const int planes = info->chroma_format_idc ? 3 : 1;
    for (int c = 0; c < planes; ++c)
        if (!dst->plane[c] || !src->plane[c]) return fail(HEIFGPU_E_INVALID, "missing plane");
    hipPointerAttribute_t ad{}, as{};
    HIP_TRY(hipPointerGetAttributes(&ad, dst->plane[0]));
    HIP_TRY(hipPointerGetAttributes(&as, src->plane[0]));
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    HIP_TRY(hipSetDevice(ad.device));
    if (ad.device != as.device) {  // a pointer of another device in this process: read it over xGMI
        const hipError_t e = hipDeviceEnablePeerAccess(as.device, 0);
        (void)hipGetLastError();
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
            (void)hipSetDevice(cur);
            HIP_TRY(e);
        }
    }
    GatherArgs g{};
    for (int c = 0; c < 3; ++c) {
        g.dst[c] = reinterpret_cast<uint64_t>(dst->plane[c]);
        g.src[c] = reinterpret_cast<uint64_t>(src->plane[c]);
        g.dpitch[c] = dst->pitch[c];
        g.spitch[c] = src->pitch[c];
    }
    g.planes = planes;
    g.sx = chroma_sx(int(info->chroma_format_idc));
    g.sy = chroma_sy(int(info->chroma_format_idc));
    g.bps = int32_t(info->bytes_per_sample);
    g.W = int32_t(info->width);
    g.H = int32_t(info->height);
    g.cols = int32_t(std::max(1u, info->grid_cols));
    g.tw = int32_t(info->tile_width ? info->tile_width : info->width);
    g.th = int32_t(info->tile_height ? info->tile_height : info->height);
    g.n_tiles = int32_t(std::max(1u, info->num_tiles));
    g.stride = int32_t(tile_stride);
    g.offset = int32_t(tile_offset);
    const hipError_t e = launch_gather_tiles(g, static_cast<hipStream_t>(stream));
    (void)hipSetDevice(cur);
    HIP_TRY(e);
    return HEIFGPU_OK;
}

namespace {
std::mutex g_ipc_mu;
std::vector<std::pair<void *, void *>> g_ipc_open;  // (pointer returned, mapping base)
}  // namespace

int heifgpu_ipc_export(const void *dev_ptr, heifgpu_ipc_handle *out) {
    static_assert(sizeof(hipIpcMemHandle_t) == sizeof(out->handle), "hipIpcMemHandle_t is 64 bytes");
    if (!dev_ptr || !out) return fail(HEIFGPU_E_INVALID, "null argument");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    HIP_TRY(hipMemGetAddressRange(&base, &size, const_cast<void *>(dev_ptr)));
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, base));
    std::memcpy(out->handle, &h, sizeof(h));
    out->offset = uint64_t(static_cast<const uint8_t *>(dev_ptr) - static_cast<const uint8_t *>(base));
    return HEIFGPU_OK;
}

int heifgpu_ipc_open(int device, const heifgpu_ipc_handle *h, void **dev_ptr) {
    if (!h || !dev_ptr) return fail(HEIFGPU_E_INVALID, "null argument");
    *dev_ptr = nullptr;
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    HIP_TRY(hipSetDevice(device));
    hipIpcMemHandle_t mh;
    std::memcpy(&mh, h->handle, sizeof(mh));
    void *base = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&base, mh, hipIpcMemLazyEnablePeerAccess);
    (void)hipSetDevice(cur);
    HIP_TRY(e);
    *dev_ptr = static_cast<uint8_t *>(base) + h->offset;
    std::lock_guard<std::mutex> lk(g_ipc_mu);
    g_ipc_open.emplace_back(*dev_ptr, base);
    return HEIFGPU_OK;
}

int heifgpu_ipc_close(void *dev_ptr) {
    void *base = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ipc_mu);
        for (size_t i = 0; i < g_ipc_open.size(); ++i)
            if (g_ipc_open[i].first == dev_ptr) {
                base = g_ipc_open[i].second;
                g_ipc_open.erase(g_ipc_open.begin() + long(i));
                break;
            }
    }
    if (!base) return fail(HEIFGPU_E_INVALID, "not a pointer returned by heifgpu_ipc_open");
    HIP_TRY(hipIpcCloseMemHandle(base));
    return HEIFGPU_OK;
}

}  // extern "C"
