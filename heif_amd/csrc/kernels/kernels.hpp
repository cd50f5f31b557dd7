// kernels.hpp — launch interface of the gfx950 decode pipeline.
//
// Pipeline per batch (6 launches):
//   0. k_rbsp       emulation-prevention removal + entry-point remap (7.3.1.1)
//   1. k_parse_lanes CABAC substreams (one per lane) → TU records +
//                   coefficients + QP/edge maps + SAO parameters
//                   (slice.rs:206-256 + todo!()s)
//   2. k_transform  dequant (8.6.2-3) + inverse DST/DCT (8.6.4) → residuals
//   3. k_intra      intra prediction (8.4.4.2) + reconstruction (8.6.7)
//   4. k_deblock    vertical then horizontal edges (8.7.2), in place (after
//                   k_assemble puts sub-picture assemblies together, if any)
//   5. k_sao_out    SAO (8.7.3) + crop + grid placement into the caller's planes
#pragma once
#include "../common/desc.hpp"
#include "resample.hpp"
#include "wave.hpp"
#include <cstdlib>
#include <vector>

#if defined(HG_HOST_EMU)
#include <atomic>
#include <thread>
#endif

namespace hg {

struct BatchArgs {
    const uint8_t *bits;       // raw NAL payloads
    const PicDesc *pics;
    const uint32_t *subs;      // substream raw start offsets (n_sub + 1 per picture, last = len)
    uint8_t *rbsp;             // k_rbsp: NAL payloads with emulation prevention removed (same offsets as bits)
    uint32_t *rsubs;           // k_rbsp: substream start offsets into rbsp (last = RBSP length)
    const uint32_t *parse_order;  // k_parse_lanes: picture (minus pic0) of wave slot i (~0u: empty); null = identity
    int n_slots;               // entries of parse_order (wave slots; a multiple of the pictures per wave)
    const SeqParams *seqs;
    const uint8_t *sf;         // ScalingFactor blocks
    const OutImage *outs;
    TuRec *tus;
    Coef *coefs;
    uint32_t *row_counts;      // [row] = {ntu, ncoef}
    uint8_t *recon;            // sample arena (uint8 or uint16 samples)
    int16_t *resid;
    uint8_t *maps;
    SaoParams *sao;
    uint32_t *status;          // per picture
    int n_pics;                // pictures of this launch: [pic0, pic0 + n_pics)
    int pic0;
    int max_width;             // luma samples, batch max
    int max_wctb;
    int max_rows;              // CTB rows, batch max
    int total_rows;            // sum of CTB rows over pictures
    int bytes_per_sample;      // 1 or 2
    int chroma_format;         // chroma_format_idc, shared by the batch's pictures
    int parse_group;           // k_parse_lanes pictures per wave (lanes_parse_order's choice; launch_parse otherwise)
    int max_log2ctb;           // largest CTB size in the batch (sizes k_intra's LDS)
    int lane_rows;             // k_parse_lanes lanes per picture: max over pictures of (WPP ? min(rows, 64) : 1)
    int wpp_ring;              // some WPP picture has more CTB rows than lanes (its rows wrap round its lanes)
    int parse_mode;            // PARSE_LANES (k_parse_lanes) or PARSE_SOLO (k_parse_solo)
    int solo_waves;            // k_parse_solo waves per workgroup (solo_waves_for(lane_rows))
    uint32_t *xprog;           // spread mode: per-row WPP progress words (total_rows)
    uint8_t *xctx;             // spread mode: per-row context hand-off blocks (total_rows * CTX_PAD)
    uint32_t *xntu;            // streaming mode: per-row TU records written so far (null otherwise)
    uint32_t *xjob;            // spread parse: the job counter each workgroup dequeues its substream job from
    int intra_stream;          // k_intra transforms and reconstructs each row behind the spread parse (same launch window)
    int stream_redo;           // k_intra_stream's second launch (after the parse): the pictures the first gave up on
    uint32_t stream_patience_us;  // first launch: give a picture up after this long without parse progress (0: at once)
    int has_assembly;          // some picture is PD_ASSEMBLY (launch_deblock runs k_assemble first)
    int intra_split;           // k_intra: luma and chroma on separate waves (set by launch_intra)
    // (added last: every other kernel's argument offsets, and so its code, stay as they were)
    int lanes_lean;            // lanes parse: the lean tool set's body (lanes_variant_for; LANES_*)
    // the lanes parse's CU lists: a word per CU (cu_word), CTB row r of a picture at word
    // cu_list_off(sao_off, max_log2ctb) + r * cu_cap_row(wctb, log2_ctb), and the words of every row
    // (indexed like row_counts / 2; k_rbsp and the decode's memset clear them with the row counts)
    uint32_t *cus;
    uint32_t *cu_counts;
    int flags_from_recs;       // the edge / no-filter map is painted from the luma TuRecs and the QpY map from the
                               // CU lists after the parse (k_paint_flags: the lanes parse leaves both out); 0: the
                               // parse wrote them (solo / spread)
};

// CU list geometry.  CUs are at least 8x8 and disjoint, so a CTB row holds at most
// wctb * (ctb / 8)^2 of them; a picture's lists start at its first CTB's index (PicDesc::sao_off,
// every picture's CTBs counted) times the batch's largest (ctb / 8)^2, which leaves each picture
// at least its own rows' room.  The arena is as large as the QpY maps padded to whole CTBs.
constexpr uint32_t cu_cap_row(int wctb, int log2ctb) { return (uint32_t)wctb << (2 * (log2ctb - 3)); }
constexpr uint64_t cu_list_off(uint64_t sao_off, int max_log2ctb) { return sao_off << (2 * (max_log2ctb - 3)); }
// a CU's word: x >> 3 (bits 0-15), its 8x8 row inside the CTB row (16-19), log2 size (20-23), QpY (24-31)
constexpr uint32_t cu_word(int x, int y_in_row, int log2, int qpy) {
    return (uint32_t)(x >> 3) | ((uint32_t)(y_in_row >> 3) << 16) | ((uint32_t)log2 << 20) | ((uint32_t)qpy << 24);
}

// k_ycbcr_rgb (color.hip): one decoded image → interleaved RGB8, rotated
struct ColorArgs {
    uint64_t plane[3];  // Y, Cb, Cr (device)
    int32_t pitch[3];   // bytes
    uint64_t rgb;       // device
    int32_t rgb_pitch;
    int32_t w, h;            // decoded (coded-orientation) size
    int32_t out_w, out_h;    // rotated size
    int32_t rotation;        // irot, anticlockwise 90-degree units
    int32_t chroma, shift;   // chroma_format_idc (0: no chroma planes); bit depth - 8
    int32_t yoff, ys;        // luma offset (16 limited range / 0 full) and scale (16.16)
    int32_t cr_r, cb_g, cr_g, cb_b;  // H.273 chroma weights (16.16, limited range rescaled)
};
// k_gather_tiles (gather.hip): tile windows k % stride == offset of src → dst
struct GatherArgs {
    uint64_t dst[3], src[3];  // planes (device pointers; src may be a peer / IPC mapping)
    int32_t dpitch[3], spitch[3];
    int32_t planes, bps;      // 1 or 3 planes, bytes per sample
    int32_t sx, sy;           // log2 chroma subsampling (chroma_sx / chroma_sy)
    int32_t W, H;             // luma output size
    int32_t tw, th, cols, n_tiles, stride, offset;
};
// H.273 coefficients for matrix_coefficients / video_full_range_flag, rounded to 16.16
inline void color_coefs(uint32_t matrix, bool full, ColorArgs &c) {
    double kr = 0.299, kb = 0.114;  // BT.601 (5, 6, and the unspecified default)
    if (matrix == 1) kr = 0.2126, kb = 0.0722;
    else if (matrix == 9) kr = 0.2627, kb = 0.0593;
    const double kg = 1.0 - kr - kb;
    const double ys = full ? 1.0 : 255.0 / 219.0, cs = full ? 1.0 : 255.0 / 224.0;
    auto fx = [](double v) { return (int32_t)(v * 65536.0 + 0.5); };
    c.yoff = full ? 0 : 16;
    c.ys = fx(ys);
    c.cr_r = fx(2.0 * (1.0 - kr) * cs);
    c.cb_b = fx(2.0 * (1.0 - kb) * cs);
    c.cb_g = fx(2.0 * kb * (1.0 - kb) / kg * cs);
    c.cr_g = fx(2.0 * kr * (1.0 - kr) / kg * cs);
}

// k_render (render.hip): one descriptor per image of a heifgpu_render_batch call.
// Output pixel (ox, oy) shows decoded sample (m[0]*ox + m[1]*oy + t[0],
// m[2]*ox + m[3]*oy + t[1]); the host has checked that the whole output maps
// inside the w x h planes.
enum : int { RENDER_RGB8 = 0, RENDER_RGBA8 = 1, RENDER_RGB16 = 2, RENDER_RGBA16 = 3 };
constexpr int kRenderXf = 4;  // added to a kernel's format parameter: the colour-managed instantiation
constexpr int kRenderTone = 8;  // added beside kRenderXf: the instantiation that also knows the tone stage of HDR sources
// added beside both: the instantiations that also know bilinear chroma upsampling (ChromaRef)
constexpr int kRenderChromaUp = 16;
// read by k_render_scaled only: the instantiations that average in linear light (render_linear.hip;
// include/heifgpu.h "Linear-light scaled render"), always with kRenderXf and kRenderChromaUp
constexpr int kRenderLinear = 32;
constexpr int kRenderTile = 64;                   // axis-swapping images: 64 x 64 output pixels per workgroup
constexpr int kRenderRowW = 256, kRenderRowH = 16;  // the others: 256 x 16
struct RenderDesc {
    uint64_t plane[3];  // Y, Cb, Cr (device)
    uint64_t alpha;     // the alpha image's luma plane, 0 = opaque
    uint64_t out;       // interleaved pixels (device)
    int32_t pitch[3], alpha_pitch, out_pitch;  // bytes
    int32_t out_w, out_h;
    int32_t m[4], t[2];
    int32_t tiles_x, tiles;  // the image's tiles (of its path's shape) along x and in all
    int32_t swap;            // m[0] == 0: output x runs along source y (staged through LDS)
    int32_t chroma, shift;   // chroma_format_idc; samples >> shift before the arithmetic (8-bit formats: depth - 8)
    int32_t alpha_bps, alpha_shift;  // alpha sample bytes; a >> alpha_shift, or a << -alpha_shift
    int32_t yoff, cmid, maxv;        // luma offset, chroma centre, clip (255, or (1 << depth) - 1)
    int32_t ys, cr_r, cb_g, cr_g, cb_b;  // 16.16, as ColorArgs
};
// ColorArgs coefficients at bit depth `depth`: color_coefs itself at 8; above it the
// offsets and the limited-range scales of that depth, ((1 << B) - 1) / (219 << (B - 8)) and
// ((1 << B) - 1) / (224 << (B - 8)), rounded to 16.16 the same way
inline void render_coefs(uint32_t matrix, bool full, int depth, RenderDesc &d) {
    ColorArgs c{};
    color_coefs(matrix, full, c);
    if (depth > 8) {
        double kr = 0.299, kb = 0.114;
        if (matrix == 1) kr = 0.2126, kb = 0.0722;
        else if (matrix == 9) kr = 0.2627, kb = 0.0593;
        const double kg = 1.0 - kr - kb, top = double((1 << depth) - 1);
        const double ys = full ? 1.0 : top / double(219 << (depth - 8)), cs = full ? 1.0 : top / double(224 << (depth - 8));
        auto fx = [](double v) { return (int32_t)(v * 65536.0 + 0.5); };
        c.yoff = full ? 0 : 16 << (depth - 8);
        c.ys = fx(ys);
        c.cr_r = fx(2.0 * (1.0 - kr) * cs);
        c.cb_b = fx(2.0 * (1.0 - kb) * cs);
        c.cb_g = fx(2.0 * kb * (1.0 - kb) / kg * cs);
        c.cr_g = fx(2.0 * kr * (1.0 - kr) / kg * cs);
    }
    d.yoff = c.yoff;
    d.ys = c.ys;
    d.cr_r = c.cr_r;
    d.cb_g = c.cb_g;
    d.cr_g = c.cr_g;
    d.cb_b = c.cb_b;
    d.cmid = 1 << (depth - 1);
    d.maxv = (1 << depth) - 1;
}

// k_render_scaled (render.hip): one descriptor per image of a heifgpu_render_batch_scaled
// call.  r is the image's RenderDesc with the window folded into m / t (window
// pixel (i, j) shows decoded sample (m[0]*i + m[1]*j + t[0], m[2]*i + m[3]*j + t[1]))
// and out_w x out_h the rendered size.  The kernel works in the source's axes:
// axis "a" is the output axis the source's y runs along (the output's y unless
// r.swap), axis "b" the one the source's x runs along.  Window index k of axis a
// is source row ma * k + ta, of axis b source column mb * k + tb.
constexpr int kScaleCols = 512;                   // source columns of one chunk: 2 per thread
constexpr int kScaleRowsA = 8, kScaleTile = 64;   // a-lines per workgroup: 8 (axes kept), 64 (axes swapped)
struct ScaleDesc {
    RenderDesc r;
    int32_t ca, cb;      // window size along a, b (1..65535)
    int32_t oa, ob;      // rendered size along a, b (1..65535)
    int32_t ma, ta, mb, tb;
    int32_t na, nb, nb_log2;  // the workgroup's tile: na a-lines x nb b-lines (nb a power of two, 16..256)
    int32_t pad;
    uint64_t den;        // 2 * ca * cb
    double inv_den;      // 1 / den (the quotient's estimate; corrected exactly)
};

// k_render_scaled's tensor epilogue (heifgpu_render_batch_tensor): the same descriptor
// (s.r.out is the tensor's base, s.r.out_pitch is unused) and where every element goes:
// out = round_to_elem(fadd(fmul(float(R), a[c]), b[c])), element (c, Y, X) at
// out + c * stride_c + Y * stride_y + X * size (CHW) or out + Y * stride_y + (X * C + c) * size (HWC).
enum : int { TENSOR_F32 = 0, TENSOR_F16 = 1, TENSOR_BF16 = 2 };
enum : int { TENSOR_CHW = 0, TENSOR_HWC = 1 };
struct TensorDesc {
    ScaleDesc s;
    int64_t stride_c, stride_y;  // bytes, multiples of the element size
    int32_t elem, layout;
    float a[4], b[4];
};

// k_render_resampled (resample.hip): one descriptor per image of a heifgpu_render_batch_resampled
// call.  r is the image's RenderDesc with the map of the WHOLE displayed picture D (no window
// folded in: taps reach beyond the window) and out_w x out_h the rendered size; ax and ay are
// the resampling along D's x and y (resample.hpp), in D's coordinates.  Stored pixel (sx, sy)
// shows output (flip & 1 ? out_w - 1 - sx : sx, flip & 2 ? out_h - 1 - sy : sy).
constexpr int kRsTileW = 64, kRsTileH = 16;  // stored pixels of a workgroup
constexpr int kRsRows = 16, kRsCols = 256;   // rows x columns of D in one chunk
constexpr int kRsCoefCap = 2048;             // the coefficient table in LDS: sw * min(ax.ksize, kRsCols) entries
struct RsParams {
    RsAxis ax, ay;
    int32_t P;       // rs_precision(depth)
    int32_t flip;
    int32_t sw;      // columns of the tile taken together, 1..64
    int32_t pad;
};
struct ResampleDesc {
    RenderDesc r;
    RsParams p;
};
// with the tensor epilogue: t.s.r as ResampleDesc::r, t's own fields as in TensorDesc
// (the ScaleDesc fields between them are unused)
struct ResampleTensorDesc {
    TensorDesc t;
    RsParams p;
};
// the sub-tile width for an axis: the widest whose footprint fits a chunk and whose
// coefficients fit the table (a wider footprint is walked in several chunks, one column at a time)
inline int rs_subtile(const RsAxis &ax) {
    const int kw = ax.ksize < kRsCols ? ax.ksize : kRsCols;
    int sw = kRsTileW;
    while (sw > 1 && (double(sw - 1) * ax.scale + double(ax.ksize) + 1.0 > double(kRsCols) || sw * kw > kRsCoefCap)) --sw;
    return sw;
}

// The colour-managed renders (heifgpu_render_batch_color and its kin): one ColorRef per
// image, in the same device array behind the call's descriptors.  lut addresses the
// transform's tables in the context's cache, in_lut[3][n] (uint16) then 4096 words out_lut[i] | out_lut[i + 1] << 16;
// 0 leaves the image as the unmanaged render writes it.  color_xform.hpp has the arithmetic.
// A tone transform (tone != 0; read by the kRenderTone instantiations only, which a call
// launches when one of its images has one) has other tables at lut: in_lut32[3][n]
// (uint32), the same 4096 out_lut words, and tone_off bytes from lut a ToneBlock.
struct ColorRef {
    uint64_t lut;
    int32_t n;     // 1 << B
    int32_t m[9];  // Q14
    int32_t tone;      // HEIFGPU_TONE_*; 0 from every call without a tone transform
    int32_t tone_off;  // bytes from lut to the ToneBlock (a multiple of 8)
};
struct ToneBlock {
    int32_t w[3];  // Q14 luminance weights
    int32_t pad;
    uint32_t pairs[2 * 576];  // T[idx], T[idx + 1] for idx = 0 .. 575 (kXfTonePairs): one 8-byte gather
};
static_assert(sizeof(ColorRef) == 56, "ColorRef: a multiple of 8 bytes behind the descriptors");

// Bilinear chroma upsampling (chroma_up.hpp; include/heifgpu.h "chroma upsampling"): one
// ChromaRef per image behind the call's ColorRefs, read by the kRenderChromaUp
// instantiations only, which a call launches when one of its images is set to bilinear
// (such a call always carries ColorRefs, with lut == 0 for its unmanaged images).  The
// fields live here and not in RenderDesc so that the descriptors, and with them the
// machine code of every other instantiation, stay what they were.
struct ChromaRef {
    int32_t mode;    // 0: replicate (also every 4:4:4 / 4:0:0 image), 1: bilinear
    int32_t px, py;  // chroma_phase(); py < 0: no vertical filter (4:2:2)
    int32_t wc, hc;  // the chroma planes' size in samples: where the taps clamp
    int32_t pad;
};
static_assert(sizeof(ChromaRef) == 24, "ChromaRef: a multiple of 8 bytes behind the ColorRefs");

// The gain-map HDR render (k_render_gain, render_gain.hip; gain_xform.hpp has the arithmetic;
// include/heifgpu.h "Gain-map HDR render"): one GainRef per image behind the call's RenderDescs,
// which are heifgpu_render_batch's at the 16-bit formats with alpha_shift 0 (convert() then
// hands the alpha sample on as decoded).  lut addresses the transform's tables in the
// context's cache: in_lut[3][n] (uint16), at t_off the (maxg + 1) pairs T[i], T[i + 1] and at
// e_off the 640 pairs E[i], E[i + 1] (uint32 each: one 8-byte gather per pair).
struct GainRef {
    uint64_t lut;
    uint64_t gain;         // the gain map's luma plane
    int32_t gain_pitch, gain_bps;
    int32_t w, h, wg, hg;  // the decoded base and gain-map sizes
    double inv_w, inv_h;   // 1.0 / w, 1.0 / h (gain_tap's estimate)
    int32_t n;             // 1 << B
    int32_t t_off, e_off;  // bytes from lut, multiples of 8
    int32_t m[9];          // Q14
    int32_t k_b, k_a;
    int32_t alpha_shift;   // PQ: a >> alpha_shift, or a << -alpha_shift, to depth P
    int32_t maxp;          // PQ: (1 << P) - 1, the alpha of an opaque pixel
    float alpha_scale;     // linear: the binary32 nearest to 1 / maxa
    uint32_t gmax;         // 256 * maxg: a plane that holds more than its depth allows still reads inside T
};
static_assert(sizeof(GainRef) % 8 == 0, "GainRef: a multiple of 8 bytes behind the descriptors");
// k_render_gain's formats: bit 0 alpha, bit 1 PQ (HEIFGPU_PIX_HDR_* - 4)
enum : int { GAIN_RGB16F = 0, GAIN_RGBA16F = 1, GAIN_RGB16PQ = 2, GAIN_RGBA16PQ = 3 };

// The scaled gain-map HDR render (k_render_gain_scaled, render_gain_scaled.hip; gain_scale.hpp has
// the averaging of the gain codes): one descriptor per image, k_render_scaled's (at the 16-bit
// formats with alpha_shift 0, as above) followed by what the first stage reads of the gain map;
// the image's GainRef lies behind the call's descriptors as k_render_gain's does and is read in
// the epilogue only.
struct GainScaleDesc {
    ScaleDesc s;
    uint64_t gain;         // the gain map's luma plane
    int32_t gain_pitch, gain_bps;
    int32_t w, h, wg, hg;  // the decoded base and gain-map sizes
    double inv_w, inv_h;   // 1.0 / w, 1.0 / h (gain_tap's estimate)
    uint32_t gmax;         // 256 * maxg (GainRef::gmax)
    int32_t pad;
};
static_assert(sizeof(GainScaleDesc) % 8 == 0, "GainScaleDesc: the GainRefs behind the descriptors are 8-byte aligned");

// parse modes (BatchArgs::parse_mode; heifgpu_batch_opts::parse_mode)
// (4 was r05's row waves, HEIFGPU_PARSE_ROWS: removed in ABI 6, prepare answers HEIFGPU_E_UNSUPPORTED)
enum : int { PARSE_AUTO = 0, PARSE_LANES = 1, PARSE_SOLO = 2, PARSE_SPREAD = 3 };
constexpr int kSoloMaxWaves = 16;
// host: BatchArgs::parse_order for a batch (size-balanced k_parse_lanes waves,
// or for solo mode with ppw_force = 1 one picture per workgroup, heaviest
// first); returns the pictures per wave it dealt for (BatchArgs::parse_group).
// ppw_force = 0: the adaptive choice.
int lanes_parse_order(const PicDesc *pics, int n, int lane_rows, int ppw_force, std::vector<uint32_t> &order);
// the adaptive choice itself: pictures per k_parse_lanes wave for a batch (launch_parse without a parse_order)
int lanes_pics_per_wave(int lane_rows, int n_pics);
// k_intra_stream (reconstruction behind the spread parse, k_transform folded in) for this batch
// (same box, spread, one-decode latency: 4 images 28.3 vs 33.7 ms streamed; 8
// images 44.4 vs 40.5, the reconstruction no longer keeps up with the parse)
constexpr int kStreamMaxPics = 192;
struct StreamKnobs {
    bool enabled = true;
    int max_pics = kStreamMaxPics;
    uint32_t patience_us = 200000;  // first launch: give a picture up after this long without parse progress
};
StreamKnobs stream_knobs_from_env();
bool intra_stream_for(int parse_mode, int n_pics, bool has_assembly, const StreamKnobs &k);
// the parse mode a batch of n_pics pictures runs in (requested: PARSE_*)
// (pics: the batch's pictures; one with dependent slice segments starting inside a
// CTB row (PicDesc.flags, PD_NMID_SHIFT) makes it a lanes parse: only that engine takes them)
int parse_mode_for(int requested, int n_pics, const PicDesc *pics = nullptr);
// the lanes parse's body for a batch (parse_engine.hpp, EngT): lean when every
// picture is 4:2:0 without PCM, transform_skip, cu_transquant_bypass, slice
// segments inside it or wrapping rows; HEIFGPU_LANES_VARIANT=general|auto
enum : int { LANES_GENERAL = 0, LANES_LEAN = 1 };
bool lanes_lean_eligible(const SeqParams *seqs, const PicDesc *pics, int n_pics, int wpp_ring);
int lanes_variant_for(const SeqParams *seqs, const PicDesc *pics, int n_pics, int wpp_ring);
// spread mode's wave slots (row << 20 | picture); -1 if the batch exceeds the encoding
int spread_parse_order(const PicDesc *pics, int n, std::vector<uint32_t> &order);
int solo_waves_for(int lane_rows);

#if defined(HG_HOST_EMU)
// Runs kernel(a) over a gx * gy grid, one block at a time, with `waves` host
// threads per block (threadIdx.x = 64 * wave).  grid_stride kernels (which
// loop t = blockIdx.x*blockDim.x+threadIdx.x .. total) get a 1x1 geometry in x.
template <class K>
void emu_launch(K kernel, int gx, int gy, int waves, const BatchArgs &a, bool grid_stride = false,
                size_t dyn_lds = 0) {
    for (int by = 0; by < gy; ++by)
        for (int bx = 0; bx < (grid_stride ? 1 : gx); ++bx) {
            std::atomic<int> cnt{0}, gen{0};
            std::vector<std::thread> th;
            unsigned char *lds = dyn_lds ? static_cast<unsigned char *>(std::malloc(dyn_lds)) : nullptr;
            for (int w = 0; w < waves; ++w)
                th.emplace_back([&, w] {
                    g_emu.bidx = {unsigned(bx), unsigned(by), 0};
                    g_emu.tidx = {unsigned(grid_stride ? 0 : 64 * w), 0, 0};
                    g_emu.bdim = {unsigned(grid_stride ? 1 : 64 * waves), 1, 1};
                    g_emu.gdim = {unsigned(grid_stride ? 1 : gx), unsigned(gy), 1};
                    g_emu.bar_count = &cnt;
                    g_emu.bar_gen = &gen;
                    g_emu.bar_n = waves;
                    g_emu.smem = lds;
                    kernel(a);
                });
            for (auto &t : th) t.join();
            std::free(lds);
        }
}
void emu_rbsp(const BatchArgs &a);
void emu_parse(const BatchArgs &a);
void emu_transform(const BatchArgs &a);
void emu_intra(const BatchArgs &a);
void emu_deblock(const BatchArgs &a);
void emu_sao_out(const BatchArgs &a);
#else
hipError_t launch_rbsp(const BatchArgs &a, hipStream_t s);
hipError_t launch_ycbcr_rgb(const ColorArgs &c, int bytes_per_sample, hipStream_t s);
hipError_t launch_gather_tiles(const GatherArgs &g, hipStream_t s);
// one launch over (max_tiles, n_images); descs on the device.  color: RENDER_MANAGED, the
// colour-managed kernels, with a ColorRef per image behind the n_images descriptors (lut == 0:
// image i untouched), or RENDER_TONE, the kernels that also take ColorRefs with a tone stage
// RENDER_CHROMA: the kernels that take everything, with a ChromaRef per image behind the ColorRefs
enum : int { RENDER_PLAIN = 0, RENDER_MANAGED = 1, RENDER_TONE = 2, RENDER_CHROMA = 3 };
// Desc: RenderDesc, ScaleDesc or TensorDesc (instantiated in render.hip)
template <typename Desc>
hipError_t launch_render(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample, int color,
                         hipStream_t s);
// (the two descriptors of k_render_resampled: specialised in resample.hip)
template <>
hipError_t launch_render<ResampleDesc>(const ResampleDesc *descs, int n_images, int max_tiles, int format,
                                       int bytes_per_sample, int color, hipStream_t s);
template <>
hipError_t launch_render<ResampleTensorDesc>(const ResampleTensorDesc *descs, int n_images, int max_tiles, int format,
                                             int bytes_per_sample, int color, hipStream_t s);
// launch_render's for RENDER_TONE: the kRenderTone instantiations, code objects of their own
// (render_tone.hip, resample_tone.hip)
template <typename Desc>
hipError_t launch_render_tone(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                              hipStream_t s);
template <>
hipError_t launch_render_tone<ResampleDesc>(const ResampleDesc *descs, int n_images, int max_tiles, int format,
                                            int bytes_per_sample, hipStream_t s);
template <>
hipError_t launch_render_tone<ResampleTensorDesc>(const ResampleTensorDesc *descs, int n_images, int max_tiles,
                                                  int format, int bytes_per_sample, hipStream_t s);
// launch_render's for RENDER_CHROMA: the kRenderChromaUp instantiations, code objects of their own
// (render_chroma.hip, resample_chroma.hip)
template <typename Desc>
hipError_t launch_render_chroma(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                                hipStream_t s);
template <>
hipError_t launch_render_chroma<ResampleDesc>(const ResampleDesc *descs, int n_images, int max_tiles, int format,
                                              int bytes_per_sample, hipStream_t s);
template <>
hipError_t launch_render_chroma<ResampleTensorDesc>(const ResampleTensorDesc *descs, int n_images, int max_tiles,
                                                    int format, int bytes_per_sample, hipStream_t s);
// the linear-light scaled renders: the kRenderLinear instantiations of k_render_scaled, a code object
// of their own (render_linear.hip).  Desc: ScaleDesc or TensorDesc; behind the n_images descriptors a
// ColorRef per image, every one with its tables (lut != 0, no tone), then a ChromaRef per image.
template <typename Desc>
hipError_t launch_render_linear(const Desc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                                hipStream_t s);
// k_render_gain (render_gain.hip): one launch over (max_tiles, n_images); n_images RenderDescs with
// as many GainRefs behind them on the device; format GAIN_*
hipError_t launch_render_gain(const RenderDesc *descs, int n_images, int max_tiles, int format, int bytes_per_sample,
                              hipStream_t s);
// k_render_gain_scaled (render_gain_scaled.hip): the same, over GainScaleDescs
hipError_t launch_render_gain_scaled(const GainScaleDesc *descs, int n_images, int max_tiles, int format,
                                     int bytes_per_sample, hipStream_t s);
hipError_t launch_parse(const BatchArgs &a, hipStream_t s);
// (launch_parse's: the kernels of parse_solo.hip and parse_lean.hip)
hipError_t launch_parse_solo(const BatchArgs &a, hipStream_t s);
hipError_t launch_parse_lean(const BatchArgs &a, int waves, size_t lds_bytes, hipStream_t s);
hipError_t launch_transform(const BatchArgs &a, hipStream_t s);
hipError_t launch_intra(const BatchArgs &a, hipStream_t s);
hipError_t launch_deblock(const BatchArgs &a, hipStream_t s);
hipError_t launch_sao_out(const BatchArgs &a, hipStream_t s);
hipError_t launch_status_fold(const uint32_t *status, uint32_t *sticky, int n, hipStream_t s);
#endif

}  // namespace hg
