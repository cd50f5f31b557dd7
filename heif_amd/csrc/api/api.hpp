// api.hpp — what the units of the C ABI layer (include/heifgpu.h) share: the two
// opaque handles every unit looks into, the error message, and the device and
// pinned buffers.  image.cpp, gain.cpp, context.cpp, render.cpp, jpeg.cpp, png.cpp and batch.cpp hold the calls.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../../include/heifgpu.h"
#include "../host/batch.hpp"
#include "../host/heic_image.hpp"
#include "../kernels/kernels.hpp"

struct heifgpu_image {
    hg::ParsedImage img;
};

constexpr int kTimingSlots = 32;
struct RenderRing;  // the render calls' descriptor staging
struct ColorCache;  // the tables of the colour, tone and gain transforms on the device
struct JpegState;   // the JPEG encoder's scratch and descriptor staging
struct PngState;    // the PNG encoder's scratch and descriptor staging
struct heifgpu_ctx {
    int device = 0;
    bool timing = false;
    hipStream_t parse = nullptr, xform = nullptr, recon = nullptr, upload = nullptr;
    // k_rbsp of the next decode (its parse set's RBSP and zeroed words) beside the
    // running parse instead of in front of the next one on the parse stream
    hipStream_t prep = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    hg::StreamKnobs stream;  // the streaming knobs, read once at heifgpu_create
    // timing ring, one slot per timed decode call: rbsp start, rbsp end, parse
    // end, transform start, transform end, recon start, 3 stage ends, parse
    // start.  heifgpu_stage_times folds every call since the previous query (a
    // slot about to be reused is folded first).
    hipEvent_t tev[kTimingSlots][10] = {};
    int timed_calls = 0, folded = 0;
    double acc[6] = {};
    // render.cpp's, opaque here; heifgpu_destroy frees them with render_state_free
    RenderRing *render = nullptr;  // created by the first render call
    ColorCache *color = nullptr;   // created by the first render that has a table to upload
    // jpeg.cpp's, opaque here; heifgpu_destroy frees it with jpeg_state_free
    JpegState *jpeg = nullptr;     // created by the first heifgpu_jpeg_encode_batch
    // png.cpp's, likewise (png_state_free)
    PngState *png = nullptr;       // created by the first heifgpu_png_encode_batch
};

namespace hg {

extern thread_local std::string g_err;  // heifgpu_last_error's message (image.cpp)

inline int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// Test hook: HEIFGPU_FAULT_INJECT names a failure to inject ("prepare": a
// reload fails after it has begun to overwrite its descriptor generation).
// Read at every call, so one test process can switch it on and off.
inline bool fault_injected(const char *what) {
    const char *e = std::getenv("HEIFGPU_FAULT_INJECT");
    return e && std::strcmp(e, what) == 0;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(HEIFGPU_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    size_t cap = 0;
    // count elements, reusing the allocation when it is large enough (a
    // reloaded batch, heifgpu_batch_prepare_ex); the caller has drained every
    // use of the old contents before a reallocation
    hipError_t alloc(size_t count) {
        n = count;
        if (p && count <= cap) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return e;
        }
        cap = std::max<size_t>(count, 1);
        return hipMalloc(reinterpret_cast<void **>(&p), cap * sizeof(T));
    }
};

// page-locked host staging of a batch's uploads (one hipMemcpyAsync source)
struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t reserve(size_t bytes) {
        if (p && bytes <= cap) return hipSuccess;
        if (p) {
            hipError_t e = hipHostFree(p);
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return e;
        }
        cap = std::max<size_t>(bytes, 4096);
        return hipHostMalloc(reinterpret_cast<void **>(&p), cap, hipHostMallocDefault);
    }
};

inline Rect rect_of(const heifgpu_rect &r) { return Rect{r.x, r.y, r.width, r.height}; }

// adds the stage times of the decode call recorded in `slot` to ctx->acc (context.cpp)
hipError_t fold_timing(heifgpu_ctx *ctx, int slot);
// deletes ctx->render and ctx->color (render.cpp, which alone knows their layouts)
void render_state_free(heifgpu_ctx *ctx);
// deletes ctx->jpeg (jpeg.cpp)
void jpeg_state_free(heifgpu_ctx *ctx);
// deletes ctx->png (png.cpp)
void png_state_free(heifgpu_ctx *ctx);

}  // namespace hg
