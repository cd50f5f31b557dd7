// batch.cpp — the batch of the C ABI: its device arenas (one plan, arena_plan), the load
// (heifgpu_batch_prepare_rects), the five-stage launch sequence (heifgpu_batch_decode)
// and the status read-out.
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

#include "../common/desc.hpp"
#include "../kernels/cabac.hpp"
#include "api.hpp"

using namespace hg;

// Pipelined decode.  k_rbsp + k_parse run on an internal parse stream, the
// four reconstruction kernels on an internal recon stream.  A batch holds up to
// three sets of parse outputs (TU records, coefficients, maps, SAO, per-row counts,
// status, residual planes) used by successive decode calls in turn, so the parse of
// call n + 1 runs while call n reconstructs: neither depends on anything the
// caller can touch (the bitstreams are the batch's own) except k_sao_out,
// which writes the caller's planes and so waits for everything the caller
// enqueued on its stream before the call; the caller's stream waits for
// k_sao_out.  A set is reused only after the reconstruction that read it.
// HEIFGPU_PIPELINE=0 or 1 keeps one set (no overlap), 2 two sets on two
// streams (before r04 every value but 0 and 3 meant two); the default, 3 (or
// more), uses three sets and a third stream for k_transform, so
// parse n + 2, transform n + 1 and reconstruction n overlap.  While the parse
// was the critical path (r02) three sets lost (15.32 / 15.33 vs 15.67 / 15.64
// Gpix/s); since the r03 parse got faster the reconstruction stream sets the
// step and three sets win (same-box pairs at 20 steps: 18.56 / 18.49 vs
// 17.86 / 17.77 Gpix/s, profiles/r03d/ab_pipeline_sets.txt).

namespace {
// per-set words of the spread and rows parses: one progress word per CTB row, then the job counter
size_t xprog_words(const HostBatch &hb) { return size_t(hb.rows) + 1; }
// k_intra_stream: one TU count per CTB row, then one done word per picture (+ 1 spare)
size_t xntu_words(const HostBatch &hb) { return size_t(hb.rows) + hb.pics.size() + 1; }
}  // namespace

// outputs of one k_parse run (see above)
struct ParseSet {
    DevBuf<TuRec> tus;
    DevBuf<Coef> coefs;
    DevBuf<uint32_t> row_counts, status;
    // lanes parse: a word per CU and the words of every CTB row (BatchArgs::cus); k_paint_flags
    // paints the QpY map from them.  As large as the QpY maps padded to whole CTBs.
    DevBuf<uint32_t> cus, cu_counts;
    DevBuf<uint8_t> maps;
    DevBuf<SaoParams> sao;
    DevBuf<int16_t> resid;  // k_transform -> k_intra
    // spread mode: per-row WPP progress words and (streaming) TU counts, per set
    // because k_intra_stream of this set's decode polls them while the next
    // decode's parse already runs
    DevBuf<uint32_t> xprog, xntu;
    // k_rbsp's output, per set so that the next decode's k_rbsp can run while
    // this set's parse still reads it
    DevBuf<uint8_t> rbsp;
    DevBuf<uint32_t> rsubs;
    hipEvent_t parsed = nullptr, transformed = nullptr, recon_done = nullptr, progreset = nullptr, prepped = nullptr;
    bool pending = false;  // recon_done recorded and not yet waited for by a parse
    ~ParseSet() {
        if (parsed) (void)hipEventDestroy(parsed);
        if (transformed) (void)hipEventDestroy(transformed);
        if (recon_done) (void)hipEventDestroy(recon_done);
        if (progreset) (void)hipEventDestroy(progreset);
        if (prepped) (void)hipEventDestroy(prepped);
    }
};

// The descriptors every stage reads (pictures, sequences, scaling factors,
// output planes) and the sticky status, in two generations: a reload writes
// the generation the previous load did not use, so it waits only for the
// decodes of the load before that (`done`), not for the ones in flight.
struct DescGen {
    DevBuf<PicDesc> pics;
    DevBuf<SeqParams> seqs;
    DevBuf<uint8_t> sf;
    DevBuf<OutImage> outs;
    DevBuf<uint32_t> sticky;  // per picture: OR of every decode's status since the last heifgpu_batch_status
    std::vector<OutImage> out_host;
    hipEvent_t done = nullptr;  // the last decode that read this generation (recon stream)
    bool pending = false;
    // the load this generation holds: picture -> image, image count (heifgpu_batch_status_previous
    // maps the sticky words of the load before the current one with these)
    std::vector<uint32_t> pic_image;
    size_t n_images = 0;
    bool loaded = false;
    ~DescGen() {
        if (done) (void)hipEventDestroy(done);
    }
};

struct heifgpu_batch {
    int device = 0;
    size_t n_images = 0;
    int n_pics = 0;
    uint32_t tile_stride = 1, tile_offset = 0;
    PinnedBuf stage;
    hipEvent_t uploaded = nullptr;  // the last load's H2D copies (upload stream)
    bool loaded = false;
    BatchArgs args{};
    // read by k_rbsp / the parse only: a reload waits for the parses in flight
    DevBuf<uint8_t> bits;
    DevBuf<uint32_t> subs, porder;
    DevBuf<uint8_t> xctx;
    // the sample arena: written by k_intra, which runs after every earlier
    // decode's k_sao_out on the one recon stream
    DevBuf<uint8_t> recon;
    DescGen gen[2];
    int cur = 0;
    ParseSet set[3];
    int n_sets = 1, next_set = 0, last_set = 0;
    std::vector<uint32_t> pic_image;  // picture → image
    std::vector<heifgpu_image_info> infos;
    ~heifgpu_batch() {
        if (uploaded) (void)hipEventDestroy(uploaded);
    }
};

// Every device arena of a load with the elements the load needs, in allocation order:
// f(arena, count, the allocation as text) for each, stopping at the first answer but
// HEIFGPU_OK.  G is the generation the load writes, n its images, order its parse order.
// heifgpu_batch_prepare_rects walks it twice: does any arena grow (then every decode in
// flight is drained before the old allocation is freed), and the allocations themselves,
// so an arena added here is in both.
template <class F>
static int arena_plan(heifgpu_batch *b, DescGen &G, const HostBatch &hb, int mode, size_t n,
                      const std::vector<uint32_t> &order, F f) {
#define ARENA(buf, count) \
    if (int rc_ = f(buf, size_t(count), #buf ".alloc(" #count ")")) return rc_
    ARENA(b->bits, hb.bits_size);
    ARENA(G.pics, hb.pics.size());
    ARENA(b->subs, hb.subs.size());
    ARENA(G.seqs, hb.seqs.size());
    ARENA(G.sf, hb.sf.size());
    ARENA(G.outs, n);
    ARENA(G.sticky, hb.pics.size());
    for (int k = 0; k < b->n_sets; ++k) {
        ParseSet &ps = b->set[k];
        ARENA(ps.tus, hb.tu_n);
        ARENA(ps.coefs, hb.coef_n);
        ARENA(ps.row_counts, size_t(2) * hb.rows);
        if (mode == PARSE_LANES) {
            ARENA(ps.cus, cu_list_off(hb.sao_n, hb.max_log2ctb));
            ARENA(ps.cu_counts, hb.rows);
        }
        ARENA(ps.maps, hb.map_bytes);
        ARENA(ps.sao, hb.sao_n);
        ARENA(ps.status, hb.pics.size());
        ARENA(ps.resid, hb.resid_elems);  // (each decode zeroes its set's status before the parse)
        ARENA(ps.rbsp, hb.bits_size);
        ARENA(ps.rsubs, hb.subs.size());
    }
    ARENA(b->recon, hb.recon_bytes);
    ARENA(b->porder, order.size());
    if (mode == PARSE_SPREAD) {  // per-row WPP progress words (+ the job counter), TU counts, context hand-off blocks
        for (int k = 0; k < b->n_sets; ++k) {
            ARENA(b->set[k].xprog, xprog_words(hb));
            ARENA(b->set[k].xntu, xntu_words(hb));
        }
        ARENA(b->xctx, std::max<size_t>(hb.rows, 1) * CTX_PAD);
    }
#undef ARENA
    return HEIFGPU_OK;
}

// The sticky status words of a load (generation G), read and cleared on s, folded per image.
// pic_image: picture -> image of that load.
static int read_sticky(DescGen &G, const std::vector<uint32_t> &pic_image, size_t n_images, uint32_t *status,
                       hipStream_t s, bool &bad) {
    std::vector<uint32_t> st(pic_image.size());
    if (!st.empty()) {
        HIP_TRY(hipMemcpyAsync(st.data(), G.sticky.p, st.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemsetAsync(G.sticky.p, 0, st.size() * sizeof(uint32_t), s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint32_t> per(n_images, 0);
    for (size_t p = 0; p < st.size(); ++p) per[pic_image[p]] |= st[p];
    bad = false;
    for (size_t i = 0; i < n_images; ++i) {
        if (status) status[i] = per[i];
        bad |= per[i] != 0;
    }
    return HEIFGPU_OK;
}

extern "C" {

// the checks of the arguments that heifgpu_batch_prepare_rects and heifgpu_batch_count_pictures
// share: the tile split of the options, then the images and their rectangles
static int tile_split_args(const heifgpu_batch_opts *opts, uint32_t &stride, uint32_t &offset) {
    stride = opts && opts->tile_stride ? opts->tile_stride : 1u;
    offset = opts ? opts->tile_offset : 0u;
    if (offset >= stride) return fail(HEIFGPU_E_INVALID, "tile_offset must be below tile_stride");
    return HEIFGPU_OK;
}

static int image_args(const heifgpu_image *const *imgs, size_t n, const heifgpu_rect *src,
                      std::vector<const ParsedImage *> &parsed, std::vector<Rect> &rects) {
    for (size_t i = 0; i < n; ++i) {
        if (!imgs[i]) return fail(HEIFGPU_E_INVALID, "null image");
        parsed.push_back(&imgs[i]->img);
        if (!src) continue;
        rects.push_back(rect_of(src[i]));
        if (!rect_inside(rects.back(), imgs[i]->img.out_width, imgs[i]->img.out_height))
            return fail(HEIFGPU_E_INVALID, "source rectangle of image " + std::to_string(i) + " empty or outside the image");
    }
    return HEIFGPU_OK;
}

int heifgpu_batch_count_pictures(const heifgpu_image *const *imgs, size_t n, const heifgpu_batch_opts *opts,
                                 const heifgpu_rect *src, uint32_t *pictures) {
    if (!imgs || !pictures || n == 0) return fail(HEIFGPU_E_INVALID, "invalid argument");
    uint32_t stride, offset;
    std::vector<const ParsedImage *> parsed;
    std::vector<Rect> rects;
    if (int rc = tile_split_args(opts, stride, offset)) return rc;
    if (int rc = image_args(imgs, n, src, parsed, rects)) return rc;
    try {
        *pictures = uint32_t(build_batch(parsed.data(), n, stride, offset, /*defer_bits=*/true,
                                         src ? rects.data() : nullptr).pics.size());
    } catch (const UnsupportedError &e) {
        return fail(HEIFGPU_E_UNSUPPORTED, e.what());
    } catch (const std::exception &e) {
        return fail(HEIFGPU_E_PARSE, e.what());
    }
    return HEIFGPU_OK;
}

int heifgpu_batch_picture_count(const heifgpu_batch *b, uint32_t *pictures) {
    if (!b || !pictures) return fail(HEIFGPU_E_INVALID, "null argument");
    if (!b->loaded) return fail(HEIFGPU_E_INVALID, "batch not loaded (its last prepare failed)");
    *pictures = uint32_t(b->n_pics);
    return HEIFGPU_OK;
}

int heifgpu_batch_prepare_ex(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                             const heifgpu_batch_opts *opts, heifgpu_batch **inout) {
    return heifgpu_batch_prepare_rects(ctx, imgs, n, opts, nullptr, inout);
}

int heifgpu_batch_prepare_rects(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                const heifgpu_batch_opts *opts, const heifgpu_rect *src, heifgpu_batch **inout) {
    if (!ctx || !imgs || !inout || n == 0) return fail(HEIFGPU_E_INVALID, "invalid argument");
    uint32_t stride, offset;
    if (int rc = tile_split_args(opts, stride, offset)) return rc;
    const uint32_t mode_req = opts ? opts->parse_mode : 0u;
    if (mode_req > HEIFGPU_PARSE_ROWS) return fail(HEIFGPU_E_INVALID, "parse_mode");
    if (mode_req == HEIFGPU_PARSE_ROWS)
        return fail(HEIFGPU_E_UNSUPPORTED, "HEIFGPU_PARSE_ROWS was removed in ABI 6 (DESIGN.md 5.9)");
    const int ppw_req = opts ? int(std::min<uint32_t>(opts->pics_per_wave, 64u)) : 0;
    if (*inout && (*inout)->device != ctx->device) return fail(HEIFGPU_E_INVALID, "batch belongs to another device");
    // the rectangles are checked here: nothing has been uploaded or launched, a reloaded batch is untouched
    std::vector<const ParsedImage *> parsed;
    std::vector<Rect> rects;
    if (int rc = image_args(imgs, n, src, parsed, rects)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<heifgpu_image_info> infos;
    for (size_t i = 0; i < n; ++i) {
        heifgpu_image_info info;
        heifgpu_image_get_info(imgs[i], &info);
        infos.push_back(info);
    }
    HostBatch hb;
    try {
        hb = build_batch(parsed.data(), n, stride, offset, /*defer_bits=*/true, src ? rects.data() : nullptr);
    } catch (const UnsupportedError &e) {
        return fail(HEIFGPU_E_UNSUPPORTED, e.what());
    } catch (const std::exception &e) {
        return fail(HEIFGPU_E_PARSE, e.what());
    }
    std::unique_ptr<heifgpu_batch> fresh;
    heifgpu_batch *b = *inout;
    if (!b) {
        fresh = std::make_unique<heifgpu_batch>();
        b = fresh.get();
        b->device = ctx->device;
        HIP_TRY(hipEventCreateWithFlags(&b->uploaded, hipEventDisableTiming));
        static const int pipeline = [] {
            const char *e = std::getenv("HEIFGPU_PIPELINE");
            return e ? std::atoi(e) : 3;
        }();
        // sets of parse outputs: the batch's own choice, else HEIFGPU_PIPELINE (default 3)
        const int sets = opts && opts->pipeline_sets ? int(opts->pipeline_sets) : pipeline;
        b->n_sets = sets <= 1 ? 1 : (sets >= 3 ? 3 : 2);
        for (int k = 0; k < b->n_sets; ++k) {
            HIP_TRY(hipEventCreateWithFlags(&b->set[k].parsed, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b->set[k].transformed, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b->set[k].recon_done, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b->set[k].progreset, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b->set[k].prepped, hipEventDisableTiming));
        }
        for (DescGen &g : b->gen) HIP_TRY(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
    }
    // A reloaded batch.  The staging buffer is rewritten only after the
    // previous load's copies (long finished in a double-buffered loop).  The
    // upload stream then waits for
    // - the parses in flight (they read bits / rbsp / subs / the parse order);
    // - the decodes of the load before the previous one, which read the
    //   descriptor generation this load overwrites;
    // not for the in-flight decodes' transform and reconstruction, which read
    // only their parse set, the other generation and the sample arena (that
    // one is ordered by the recon stream).
    // (unconditionally: a reload that failed may have issued copies from staging)
    HIP_TRY(hipEventSynchronize(b->uploaded));
    // The generation the last successful load did not use (not the
    // one of b->loaded, which a failed reload clears while gen[cur] still holds
    // the last good load, its in-flight decodes and their sticky status)
    const int gi = b->gen[b->cur].loaded ? b->cur ^ 1 : b->cur;
    DescGen &G = b->gen[gi];
    for (int k = 0; k < b->n_sets; ++k)
        if (b->set[k].pending) HIP_TRY(hipStreamWaitEvent(ctx->upload, b->set[k].parsed, 0));
    if (G.pending) HIP_TRY(hipStreamWaitEvent(ctx->upload, G.done, 0));
    std::vector<uint32_t> order;
    const int mode = parse_mode_for(int(mode_req), int(hb.pics.size()), hb.pics.data());
    const int solo_waves = solo_waves_for(hb.lane_rows);
    int parse_group = 1;
    if (mode == PARSE_SPREAD) {
        if (spread_parse_order(hb.pics.data(), int(hb.pics.size()), order) < 0)
            return fail(HEIFGPU_E_UNSUPPORTED, "spread parse: over 2^20 pictures or 4096 substreams per picture");
    } else {  // pictures dealt by payload size (r03: dealing by WPP critical path lost, 16.9 vs 17.0 Gpix/s)
        parse_group = lanes_parse_order(hb.pics.data(), int(hb.pics.size()), hb.lane_rows,
                                        mode == PARSE_SOLO ? 1 : ppw_req, order);
    }
    // spread parse: WPP neighbours in other waves (progress words,
    // context hand-off blocks, the job counter after the progress words)
    const bool cross_rows = mode == PARSE_SPREAD;
    bool grows = false;  // some arena of the plan is too small for this load
    (void)arena_plan(b, G, hb, mode, n, order, [&](auto &buf, size_t count, const char *) {
        grows = grows || count > buf.cap;
        return HEIFGPU_OK;
    });
    if (grows) {  // reallocation: every decode of the old contents fully drained
        for (int k = 0; k < b->n_sets; ++k)
            if (b->set[k].pending) HIP_TRY(hipEventSynchronize(b->set[k].recon_done));
        HIP_TRY(hipStreamSynchronize(ctx->upload));
    }
    // A failure from here on leaves the batch unusable until a reload succeeds
    // (its arguments may point at freed arenas): `loaded` is set again last.
    b->loaded = false;
    G.loaded = false;  // its previous contents (two loads back) are overwritten from here on
    G.pic_image.clear();
    G.n_images = 0;
    if (fault_injected("prepare"))  // test hook: a reload that fails after touching the generation
        return fail(HEIFGPU_E_INVALID, "injected prepare failure (HEIFGPU_FAULT_INJECT=prepare)");
    // ---- device arenas (reused when large enough)
    if (int rc = arena_plan(b, G, hb, mode, n, order, [](auto &buf, size_t count, const char *what) {
            const hipError_t e = buf.alloc(count);
            return e == hipSuccess ? HEIFGPU_OK : fail(HEIFGPU_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        }))
        return rc;
    HIP_TRY(hipMemsetAsync(G.sticky.p, 0, hb.pics.size() * sizeof(uint32_t), ctx->upload));
    // ---- one pinned staging image of every upload, copied asynchronously
    struct Seg {
        const void *src;
        size_t bytes;
        void *dst;
    };
    const Seg segs[] = {
        {nullptr, hb.bits_size, b->bits.p},  // the payload pieces, copied below
        {hb.pics.data(), hb.pics.size() * sizeof(PicDesc), G.pics.p},
        {hb.subs.data(), hb.subs.size() * sizeof(uint32_t), b->subs.p},
        {hb.seqs.data(), hb.seqs.size() * sizeof(SeqParams), G.seqs.p},
        {hb.sf.data(), hb.sf.size(), G.sf.p},
        {order.data(), order.size() * sizeof(uint32_t), b->porder.p},
    };
    size_t total = 0;
    for (const Seg &g : segs) total += (g.bytes + 255) & ~size_t(255);
    HIP_TRY(b->stage.reserve(total));
    {  // the bitstreams (most of the bytes) straight from the parsed images into staging, on a few threads
        uint8_t *dst = b->stage.p;
        const size_t np = hb.pieces.size();
        const size_t nt = std::min<size_t>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())),
                                           (hb.bits_size >> 22) + 1);  // ~4 MB per thread at least
        std::atomic<size_t> next{0};
        auto copy = [&] {
            for (size_t i; (i = next.fetch_add(64)) < np;)
                for (size_t j = i; j < std::min(np, i + 64); ++j) {
                    const HostBatch::Piece &pc = hb.pieces[j];
                    std::memcpy(dst + pc.dst, pc.src, pc.len);
                    const size_t end = j + 1 < np ? hb.pieces[j + 1].dst : hb.bits_size;
                    std::memset(dst + pc.dst + pc.len, 0, end - pc.dst - pc.len);  // alignment padding
                }
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nt; ++t) pool.emplace_back(copy);
        copy();
        for (auto &th : pool) th.join();
        if (np == 0) std::memset(dst, 0, hb.bits_size);
    }
    size_t off = 0;
    for (const Seg &g : segs) {
        if (g.bytes) {
            if (g.src) std::memcpy(b->stage.p + off, g.src, g.bytes);
            HIP_TRY(hipMemcpyAsync(g.dst, b->stage.p + off, g.bytes, hipMemcpyHostToDevice, ctx->upload));
        }
        off += (g.bytes + 255) & ~size_t(255);
    }
    for (int k = 0; k < b->n_sets; ++k) HIP_TRY(hipMemsetAsync(b->set[k].rbsp.p, 0, hb.bits_size, ctx->upload));
    HIP_TRY(hipEventRecord(b->uploaded, ctx->upload));
    b->n_images = n;
    b->tile_stride = stride;
    b->tile_offset = offset;
    b->infos = std::move(infos);
    b->pic_image = hb.pic_image;
    G.pic_image = hb.pic_image;
    G.n_images = n;
    G.loaded = true;
    b->n_pics = int(hb.pics.size());
    b->cur = gi;
    b->loaded = true;
    BatchArgs &a = b->args;
    a = BatchArgs{};
    a.bits = b->bits.p;
    a.pics = G.pics.p;
    a.subs = b->subs.p;
    a.rbsp = nullptr;  // (per parse set: heifgpu_batch_decode)
    a.rsubs = nullptr;
    a.parse_order = b->porder.p;
    a.n_slots = int(order.size());
    a.parse_group = parse_group;
    a.seqs = G.seqs.p;
    a.sf = G.sf.p;
    a.outs = G.outs.p;
    a.recon = b->recon.p;
    a.n_pics = b->n_pics;
    a.max_width = hb.max_w;
    a.max_wctb = hb.max_wctb;
    a.max_rows = hb.max_rows;
    a.max_log2ctb = hb.max_log2ctb;
    a.lane_rows = hb.lane_rows;
    a.parse_mode = mode;
    a.solo_waves = solo_waves;
    a.xprog = nullptr;  // (per parse set: heifgpu_batch_decode)
    a.xctx = cross_rows ? b->xctx.p : nullptr;
    a.intra_stream = intra_stream_for(mode, int(hb.pics.size()), hb.has_assembly, ctx->stream) ? 1 : 0;
    a.xntu = nullptr;
    a.stream_patience_us = ctx->stream.patience_us;
    // rows wrap round the lanes (waves) of a picture: the WPP context staging
    a.wpp_ring = mode == PARSE_SOLO ? (hb.max_wpp_rows > solo_waves ? 1 : 0) : hb.wpp_ring;
    a.lanes_lean = mode == PARSE_LANES
                       ? lanes_variant_for(hb.seqs.data(), hb.pics.data(), int(hb.pics.size()), a.wpp_ring)
                       : LANES_GENERAL;
    a.flags_from_recs = mode == PARSE_LANES ? 1 : 0;  // (never streaming: launch_transform paints)
    a.has_assembly = hb.has_assembly ? 1 : 0;
    a.total_rows = int(hb.rows);
    a.bytes_per_sample = hb.bps;
    a.chroma_format = hb.chroma;
    G.out_host.assign(n, OutImage{});
    if (fresh) *inout = fresh.release();
    return HEIFGPU_OK;
}

int heifgpu_batch_prepare(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, heifgpu_batch **out) {
    if (!out) return fail(HEIFGPU_E_INVALID, "invalid argument");
    *out = nullptr;
    const int rc = heifgpu_batch_prepare_ex(ctx, imgs, n, nullptr, out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->upload));  // v1 semantics: uploaded on return
    return HEIFGPU_OK;
}

int heifgpu_batch_decode(heifgpu_ctx *ctx, heifgpu_batch *b, const heifgpu_planes *out, void *stream) {
    if (!ctx || !b || !out) return fail(HEIFGPU_E_INVALID, "invalid argument");
    if (b->device != ctx->device) return fail(HEIFGPU_E_INVALID, "batch belongs to another device");
    if (!b->loaded) return fail(HEIFGPU_E_INVALID, "batch not loaded (its last prepare failed)");
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream, as in HIP
    HIP_TRY(hipSetDevice(ctx->device));
    DescGen &G = b->gen[b->cur];
    bool changed = false;
    for (size_t i = 0; i < b->n_images; ++i) {
        OutImage o{};
        for (int c = 0; c < 3; ++c) {
            o.plane[c] = reinterpret_cast<uint64_t>(out[i].plane[c]);
            o.pitch[c] = out[i].pitch[c];
        }
        if (!out[i].plane[0] || (b->infos[i].chroma_format_idc && (!out[i].plane[1] || !out[i].plane[2])))
            return fail(HEIFGPU_E_INVALID, "missing output plane");
        o.width = int32_t(b->infos[i].width);
        o.height = int32_t(b->infos[i].height);
        if (std::memcmp(&o, &G.out_host[i], sizeof(o)) != 0) {
            G.out_host[i] = o;
            changed = true;
        }
    }
    if (changed)
        HIP_TRY(hipMemcpyAsync(G.outs.p, G.out_host.data(), b->n_images * sizeof(OutImage), hipMemcpyHostToDevice, s));
    // parse set of this call
    const int k = b->next_set;
    b->next_set = (k + 1) % b->n_sets;
    b->last_set = k;
    ParseSet &ps = b->set[k];
    BatchArgs a = b->args;
    a.tus = ps.tus.p;
    a.coefs = ps.coefs.p;
    a.row_counts = ps.row_counts.p;
    a.cus = a.parse_mode == PARSE_LANES ? ps.cus.p : nullptr;
    a.cu_counts = a.parse_mode == PARSE_LANES ? ps.cu_counts.p : nullptr;
    a.maps = ps.maps.p;
    a.sao = ps.sao.p;
    a.status = ps.status.p;
    a.resid = ps.resid.p;
    a.rbsp = ps.rbsp.p;
    a.rsubs = ps.rsubs.p;
    if (a.parse_mode == PARSE_SPREAD) {
        a.xprog = ps.xprog.p;
        a.xjob = ps.xprog.p + a.total_rows;
        a.xntu = a.intra_stream ? ps.xntu.p : nullptr;
    }
    // bring-up knob: HEIFGPU_STAGES=k launches only the first k stages (in order, on the caller's stream)
    static const int max_stages = [] {
        const char *e = std::getenv("HEIFGPU_STAGES");
        return e ? std::atoi(e) : 5;
    }();
    if (max_stages < 5) {
        a.intra_stream = 0;  // (stages one after another: k_transform, then the plain k_intra)
        a.xntu = nullptr;
        HIP_TRY(hipStreamSynchronize(ctx->upload));
        HIP_TRY(hipStreamSynchronize(ctx->parse));
        HIP_TRY(hipStreamSynchronize(ctx->xform));
        HIP_TRY(hipStreamSynchronize(ctx->recon));
        HIP_TRY(hipMemsetAsync(ps.status.p, 0, size_t(b->n_pics) * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(ps.row_counts.p, 0, size_t(2) * uint32_t(b->args.total_rows) * sizeof(uint32_t), s));
        if (a.cu_counts) HIP_TRY(hipMemsetAsync(a.cu_counts, 0, uint32_t(b->args.total_rows) * sizeof(uint32_t), s));
        HIP_TRY(launch_rbsp(a, s));
        hipError_t (*fns[5])(const BatchArgs &, hipStream_t) = {launch_parse, launch_transform, launch_intra,
                                                                launch_deblock, launch_sao_out};
        for (int i = 0; i < max_stages; ++i) HIP_TRY(fns[i](a, s));
        HIP_TRY(launch_status_fold(ps.status.p, G.sticky.p, b->n_pics, s));
        return HEIFGPU_OK;
    }
#if defined(HG_ABLATE)
    // measurement builds only (make variant VDEFS=-DHG_ABLATE): HEIFGPU_ABLATE bit i
    // drops reconstruction stage i (1 transform, 2 intra, 4 deblock, 8 sao): wrong
    // pixels, the co-run cost of each stage on the parse
    static const int ablate = [] {
        const char *e = std::getenv("HEIFGPU_ABLATE");
        return e ? std::atoi(e) : 0;
    }();
#else
    constexpr int ablate = 0;
#endif
    hipStream_t p = ctx->parse, r = ctx->recon;
    if (b->n_pics == 0) {  // a tile subset without pictures: nothing to decode
        return HEIFGPU_OK;
    }
    const bool t = ctx->timing;
    hipEvent_t *ev = nullptr;
    if (t) {  // this call's timing slot; the call that used it last is folded first
        const int slot = ctx->timed_calls % kTimingSlots;
        if (ctx->timed_calls - ctx->folded >= kTimingSlots) {
            HIP_TRY(fold_timing(ctx, slot));
            ++ctx->folded;
        }
        ev = ctx->tev[slot];
        ++ctx->timed_calls;
    }
    // k_rbsp (prep stream, or the parse stream itself): the batch's uploads, and
    // this set's previous reconstruction must be done with it.  It also zeroes
    // this set's status words and row counts (rows a stopped substream never
    // reaches keep zero TBs) and, streaming, the progress words, TU counts and
    // done words k_intra_stream polls from its start (launch_parse leaves them
    // alone in that mode).  On the prep stream it runs beside the previous
    // decode's parse, so the parse stream goes from one k_parse to the next.
    hipStream_t q = ctx->prep ? ctx->prep : p;
    HIP_TRY(hipStreamWaitEvent(q, b->uploaded, 0));
    if (ps.pending) HIP_TRY(hipStreamWaitEvent(q, ps.recon_done, 0));
    if (t) HIP_TRY(hipEventRecord(ev[0], q));
    HIP_TRY(launch_rbsp(a, q));
    if (a.intra_stream) HIP_TRY(hipEventRecord(ps.progreset, q));
    if (t) HIP_TRY(hipEventRecord(ev[1], q));
    if (q != p) {
        HIP_TRY(hipEventRecord(ps.prepped, q));
        HIP_TRY(hipStreamWaitEvent(p, ps.prepped, 0));
    }
    if (t) HIP_TRY(hipEventRecord(ev[9], p));
    HIP_TRY(launch_parse(a, p));
    if (t) HIP_TRY(hipEventRecord(ev[2], p));
    HIP_TRY(hipEventRecord(ps.parsed, p));
    HIP_TRY(hipEventRecord(ctx->fork, s));
    if (a.intra_stream) {
        // streaming (small batches): no k_transform; the
        // reconstruction starts beside this decode's parse and trails it
        HIP_TRY(hipStreamWaitEvent(r, ps.progreset, 0));
        if (t) {
            HIP_TRY(hipEventRecord(ev[3], r));
            HIP_TRY(hipEventRecord(ev[4], r));
        }
    } else {
        // transform stream (the recon stream with two sets): this set's parse
        hipStream_t x = b->n_sets >= 3 ? ctx->xform : r;
        HIP_TRY(hipStreamWaitEvent(x, ps.parsed, 0));
        if (t) HIP_TRY(hipEventRecord(ev[3], x));
        if (!(ablate & 1)) HIP_TRY(launch_transform(a, x));
        if (t) HIP_TRY(hipEventRecord(ev[4], x));
        HIP_TRY(hipEventRecord(ps.transformed, x));
        // recon stream: this set's transform, and the caller's prior work before the planes are written
        HIP_TRY(hipStreamWaitEvent(r, ps.transformed, 0));
    }
    if (t) HIP_TRY(hipEventRecord(ev[5], r));
    if (!(ablate & 2)) HIP_TRY(launch_intra(a, r));
    if (a.intra_stream) {
        // the second launch, after the parse: the pictures the first one gave up
        // on (none, unless the parse did not run beside it); the rest exit at once
        HIP_TRY(hipStreamWaitEvent(r, ps.parsed, 0));
        BatchArgs a2 = a;
        a2.stream_redo = 1;
        HIP_TRY(launch_intra(a2, r));
    }
    if (t) HIP_TRY(hipEventRecord(ev[6], r));
    if (!(ablate & 4)) HIP_TRY(launch_deblock(a, r));
    if (t) HIP_TRY(hipEventRecord(ev[7], r));
    HIP_TRY(hipStreamWaitEvent(r, ctx->fork, 0));
    if (!(ablate & 8)) HIP_TRY(launch_sao_out(a, r));
    if (t) HIP_TRY(hipEventRecord(ev[8], r));
    HIP_TRY(launch_status_fold(ps.status.p, G.sticky.p, b->n_pics, r));
    HIP_TRY(hipEventRecord(ps.recon_done, r));
    ps.pending = true;
    HIP_TRY(hipEventRecord(G.done, r));
    G.pending = true;
    HIP_TRY(hipEventRecord(ctx->join, r));
    HIP_TRY(hipStreamWaitEvent(s, ctx->join, 0));
    return HEIFGPU_OK;
}

int heifgpu_batch_parse_geometry(const heifgpu_batch *b, uint32_t *mode, uint32_t *workgroups,
                                 uint32_t *pics_per_wave, uint32_t *waves_per_workgroup) {
    if (!b || !b->loaded) return fail(HEIFGPU_E_INVALID, "invalid batch");
    const BatchArgs &a = b->args;
    const bool solo = a.parse_mode == PARSE_SOLO, lanes = a.parse_mode == PARSE_LANES;
    const uint32_t ppw = lanes ? uint32_t(std::max(1, a.parse_group)) : 1u;
    if (mode) *mode = uint32_t(a.parse_mode);
    if (workgroups) *workgroups = (uint32_t(a.n_slots) + ppw - 1) / ppw;
    if (pics_per_wave) *pics_per_wave = ppw;
    if (waves_per_workgroup) *waves_per_workgroup = solo ? uint32_t(a.solo_waves) : 1u;
    return HEIFGPU_OK;
}

int heifgpu_batch_lanes_variant(const heifgpu_batch *b, uint32_t *variant) {
    if (!b || !b->loaded || !variant) return fail(HEIFGPU_E_INVALID, "invalid argument");
    *variant = b->args.parse_mode == PARSE_LANES ? uint32_t(b->args.lanes_lean) : uint32_t(LANES_GENERAL);
    return HEIFGPU_OK;
}

int heifgpu_batch_status(heifgpu_ctx *ctx, heifgpu_batch *b, uint32_t *status, void *stream) {
    if (!ctx || !b) return fail(HEIFGPU_E_INVALID, "invalid argument");
    if (b->device != ctx->device) return fail(HEIFGPU_E_INVALID, "batch belongs to another device");
    if (!b->loaded) return fail(HEIFGPU_E_INVALID, "batch not loaded (its last prepare failed)");
    hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null stream, as in HIP
    HIP_TRY(hipSetDevice(ctx->device));
    // every decode since the last query (or the load) ORed its status words
    // into the sticky array (k_status_fold after k_sao_out); read and clear it
    bool bad = false;
    if (int rc = read_sticky(b->gen[b->cur], b->pic_image, b->n_images, status, s, bad)) return rc;
    return bad ? fail(HEIFGPU_E_DECODE, "one or more pictures failed the kernel bitstream checks") : HEIFGPU_OK;
}

// The load before the current one: decodes of it still in flight when the
// batch was reloaded fold their status into that load's generation, which
// heifgpu_batch_status (current load only) does not read.  This reads and
// clears it, per image of that load (errors must reach the
// caller, as the reference's src/heic/decoder.rs:109-112 does).
int heifgpu_batch_status_previous(heifgpu_ctx *ctx, heifgpu_batch *b, uint32_t *status, size_t cap, size_t *n_prev,
                                  void *stream) {
    if (!ctx || !b || !n_prev) return fail(HEIFGPU_E_INVALID, "invalid argument");
    if (b->device != ctx->device) return fail(HEIFGPU_E_INVALID, "batch belongs to another device");
    *n_prev = 0;
    if (!b->loaded) return fail(HEIFGPU_E_INVALID, "batch not loaded (its last prepare failed)");
    DescGen &P = b->gen[b->cur ^ 1];
    if (!P.loaded || P.pic_image.empty()) return HEIFGPU_OK;  // no previous load
    *n_prev = P.n_images;
    if (!status) return HEIFGPU_OK;  // the size query: nothing read or cleared
    if (cap < P.n_images) return fail(HEIFGPU_E_INVALID, "status array smaller than the previous load");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(ctx->device));
    if (P.pending) HIP_TRY(hipStreamWaitEvent(s, P.done, 0));  // its last decode
    bool bad = false;
    if (int rc = read_sticky(P, P.pic_image, P.n_images, status, s, bad)) return rc;
    return bad ? fail(HEIFGPU_E_DECODE, "one or more pictures of the previous load failed the kernel bitstream checks")
               : HEIFGPU_OK;
}

void heifgpu_batch_free(heifgpu_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();  // in-flight parses / reconstructions of this batch
    delete b;
}

int heifgpu_decode_batch(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *out,
                         void *stream, uint32_t *status) {
    heifgpu_batch *b = nullptr;
    int rc = heifgpu_batch_prepare(ctx, imgs, n, &b);
    if (rc) return rc;
    rc = heifgpu_batch_decode(ctx, b, out, stream);
    if (!rc) rc = heifgpu_batch_status(ctx, b, status, stream);
    heifgpu_batch_free(b);
    return rc;
}

}  // extern "C"
