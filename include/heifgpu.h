/*
 * heifgpu.h — C ABI of the MI355X-native HEIC (HEVC intra still) decode path.
 *
 * Drop-in boundary for friendlymatthew/heif:
 *   - heifgpu_image_parse / heifgpu_image_info replace the host half of
 *     HeicDecoder::decode (src/heic/decoder.rs:12-112: HeifReader::read,
 *     hvcC → VPS/SPS/PPS, primary item → grid tiles → slice headers);
 *   - heifgpu_decode_batch replaces the serial per-tile loop
 *     (src/heic/decoder.rs:114-119: SliceSegmentReader::try_new +
 *     read_data, src/hevc/slice.rs:19-42, :206-256) and, unlike the
 *     reference (which returns Result<()> and panics at slice.rs:250), writes
 *     the reconstructed Y/Cb/Cr planes.
 * The test hooks at the end expose the host pieces the reference unit-tests
 * (src/hevc/rbsp_reader.rs:139-303, src/cabac/decoder.rs:286-373,
 * tests/libheif_comparison.rs:9-112).
 *
 * Conventions: functions return 0 on success and a negative HEIFGPU_E_*
 * code on failure (the reference's anyhow::Result / ensure! / bail!);
 * heifgpu_last_error() returns the message of the last failure on the
 * calling thread.  All pointers are plain host or device pointers; no
 * framework types cross the boundary.  A context is bound to one device and
 * must not be used from two threads at once; distinct contexts may run
 * concurrently (one per GPU).
 */
#ifndef HEIFGPU_H
#define HEIFGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEIFGPU_ABI_VERSION 6

enum {
    HEIFGPU_OK = 0,
    HEIFGPU_E_INVALID = -1,     /* bad argument */
    HEIFGPU_E_PARSE = -2,       /* container / parameter-set / slice-header error */
    HEIFGPU_E_UNSUPPORTED = -3, /* valid stream using a tool outside this path */
    HEIFGPU_E_DEVICE = -4,      /* HIP runtime error */
    HEIFGPU_E_DECODE = -5       /* a picture's bitstream failed the kernel checks */
};

/* per-image status bits reported by heifgpu_batch_status */
enum {
    HEIFGPU_ST_CABAC_INIT = 1 << 0,
    HEIFGPU_ST_SUBSTREAM_END = 1 << 1,
    HEIFGPU_ST_OVERRUN = 1 << 2,
    HEIFGPU_ST_SYNTAX = 1 << 3,
    HEIFGPU_ST_UNSUPPORTED = 1 << 4,
    HEIFGPU_ST_CAPACITY = 1 << 5
};

typedef struct heifgpu_image heifgpu_image; /* host-parsed HEIC image */
typedef struct heifgpu_ctx heifgpu_ctx;     /* per-device decoder context */
typedef struct heifgpu_batch heifgpu_batch; /* device-resident batch */

typedef struct {
    uint32_t width, height;       /* output (grid-cropped) size, coded orientation */
    uint32_t chroma_format_idc;   /* 0 = 4:0:0, 1 = 4:2:0, 2 = 4:2:2, 3 = 4:4:4 (Cb/Cr planes
                                     ceil(w / SubWidthC) x ceil(h / SubHeightC)) */
    uint32_t bit_depth;           /* luma bit depth (chroma equal) */
    uint32_t bytes_per_sample;    /* 1 for 8-bit, 2 otherwise */
    uint32_t grid_rows, grid_cols;/* 1x1 for a single coded item */
    uint32_t tile_width, tile_height;
    uint32_t num_tiles;
    uint32_t rotation;            /* irot angle, anticlockwise in 90-degree units */
    uint32_t ispe_width, ispe_height;
    uint32_t coded_bytes;         /* sum of tile item bytes */
    uint32_t primary_item_id;
    uint32_t num_thumbnails;
    uint32_t matrix_coeffs, full_range;
    uint32_t item_id;             /* the decoded item (primary_item_id unless parsed by item) */
    uint32_t aux_item_id;         /* first auxiliary image of the primary ('auxl'), 0 if none */
} heifgpu_image_info;

typedef struct {
    void *plane[3];               /* device pointers, caller-owned (Y, Cb, Cr) */
    int32_t pitch[3];             /* bytes per row */
} heifgpu_planes;

/* decode options of heifgpu_batch_prepare_ex */
typedef struct {
    /* Single-image tile split across GPUs: only grid tiles k
     * (row-major) with k % tile_stride == tile_offset are decoded, each into
     * its window of the full-size output planes; the other windows are not
     * written.  0 or 1 = every tile.  Tiles are independent IDR pictures
     * (src/heic/decoder.rs:98-119 decodes them one by one). */
    uint32_t tile_stride, tile_offset;
    /* CABAC parse mode: HEIFGPU_PARSE_AUTO picks by batch
     * size (spread up to 1536 pictures, lanes above; lanes whatever is asked
     * for a batch with dependent slice segments starting inside a CTB row);
     * HEIFGPU_PARSE_LANES packs one substream per lane (throughput);
     * HEIFGPU_PARSE_SOLO runs one substream per wavefront, a picture's rows in
     * one workgroup; HEIFGPU_PARSE_SPREAD one substream per wavefront, every
     * row its own workgroup (latency of small batches).  HEIFGPU_PARSE_ROWS
     * (ABI 5 only: one picture per lane, one CTB row of up to 64 pictures per
     * wavefront) was removed in ABI 6, as it won only on batches that repeat
     * bitstreams; prepare answers HEIFGPU_E_UNSUPPORTED. */
    uint32_t parse_mode;
    /* lanes mode: pictures per wavefront (0 = adaptive; larger values are
     * capped at 64 / CTB rows) */
    uint32_t pics_per_wave;
    /* sets of parse outputs (ABI 4): 0 = the default (3, or HEIFGPU_PIPELINE);
     * 1 = no overlap; 2 = parse n+1 beside the reconstruction of n; 3 = parse
     * n+2, transform n+1 and reconstruction n overlap.  Every set holds its own
     * TU / coefficient / residual / map arenas (~3.2 MB per 512x512 picture),
     * so a memory-tight caller can ask for fewer.  Taken when the batch is
     * created (the first prepare); reloads keep it. */
    uint32_t pipeline_sets;
} heifgpu_batch_opts;

enum {
    HEIFGPU_PARSE_AUTO = 0,
    HEIFGPU_PARSE_LANES = 1,
    HEIFGPU_PARSE_SOLO = 2,
    HEIFGPU_PARSE_SPREAD = 3,
    HEIFGPU_PARSE_ROWS = 4 /* removed in ABI 6: HEIFGPU_E_UNSUPPORTED */
};

/* ---- host: demux + parameter sets + slice headers ------------------- */
/* data is copied; the returned image owns its bytes. */
int heifgpu_image_parse(const uint8_t *data, size_t len, heifgpu_image **out);
/* n independent files parsed on `threads` host threads (<= 0: all hardware
 * threads).  out[i] is NULL when file i failed; rc[i] (optional) receives its
 * code.  Returns 0 when every file parsed, else the first failure's code. */
int heifgpu_image_parse_many(const uint8_t *const *data, const size_t *len, size_t n, int threads,
                             heifgpu_image **out, int *rc);
/* Any coded image item by ID (0 = primary), e.g. the HDR gain map the primary
 * references through 'auxl' (info.aux_item_id; src/heif/grammar.rs:202-207
 * parses the reference but nothing decodes it).  Grid or single hvc1 item. */
int heifgpu_image_parse_item(const uint8_t *data, size_t len, uint32_t item_id, heifgpu_image **out);
int heifgpu_image_get_info(const heifgpu_image *img, heifgpu_image_info *info);
void heifgpu_image_free(heifgpu_image *img);

/* ---- device context --------------------------------------------------- */
int heifgpu_create(int device, heifgpu_ctx **out);
void heifgpu_destroy(heifgpu_ctx *ctx);
const char *heifgpu_last_error(void);

/* ---- batched decode ----------------------------------------------------
 * heifgpu_batch_prepare flattens n images (all must share bit depth and
 * chroma format) into device descriptors, uploads their bitstreams
 * (complete on return) and allocates the work arenas.
 * heifgpu_batch_prepare_ex does the same with options (NULL = defaults) and
 * without waiting for the upload: the host work (flattening into a pinned
 * staging buffer) is done on return, the host-to-device copies run on an
 * internal upload stream that the next heifgpu_batch_decode of the batch
 * waits for.  With *inout == NULL it creates a batch; otherwise it reloads
 * *inout with the new images, reusing its device arenas when they are large
 * enough (the copies wait for every decode still reading the old contents).
 * Two batches reloaded alternately overlap host parsing and upload of batch
 * n + 1 with the decode of batch n.  heifgpu_batch_decode
 * then enqueues the five decode stages on `stream` (a hipStream_t; NULL =
 * the device's null stream, as everywhere in HIP) and returns immediately; out[i] receives
 * image i.  It may be called repeatedly on the same batch (the bench times
 * exactly this call).  heifgpu_batch_status synchronises the stream and
 * returns the per-image status words (0 = ok): the OR over every decode of
 * the batch since the previous heifgpu_batch_status call or the last
 * (re)load, so damage seen by any of several pipelined decodes is reported;
 * the call clears them. */
int heifgpu_batch_prepare(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, heifgpu_batch **out);
int heifgpu_batch_prepare_ex(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                             const heifgpu_batch_opts *opts, heifgpu_batch **inout);
int heifgpu_batch_decode(heifgpu_ctx *ctx, heifgpu_batch *batch, const heifgpu_planes *out, void *stream);
int heifgpu_batch_status(heifgpu_ctx *ctx, heifgpu_batch *batch, uint32_t *status, void *stream);
/* ABI 5.  A reload does not wait for the previous load's decodes in flight;
 * their status words stay with that load (heifgpu_batch_status reports the
 * current load only).  This reads and clears them: per image of the load
 * before the current one (*n_prev images, 0 if there is none; status must
 * hold cap >= *n_prev words; status = NULL only sets *n_prev and reads
 * nothing), after its last decode.  The words survive until the batch is
 * reloaded again.  Returns HEIFGPU_E_DECODE if any is nonzero. */
int heifgpu_batch_status_previous(heifgpu_ctx *ctx, heifgpu_batch *batch, uint32_t *status, size_t cap,
                                  size_t *n_prev, void *stream);
/* HEIFGPU_ABI_VERSION of the library.  Call this first: a caller built
 * against another version (e.g. ABI 3's 16-byte heifgpu_batch_opts) must not
 * call the other entry points.  ABI 6: HEIFGPU_PARSE_ROWS removed; a reload
 * that fails no longer costs heifgpu_batch_status_previous the last good
 * load's status. */
int heifgpu_abi_version(void);
void heifgpu_batch_free(heifgpu_batch *batch);
/* stage timing (ms per decode call, from HIP events on the streams the
 * kernels run on, enabled with heifgpu_set_timing(ctx, 1)): the mean over the
 * decode calls since the previous query (or since timing was enabled) of
 * parse, transform, intra, deblock, sao/output, and (last) the
 * emulation-prevention pass k_rbsp; the query resets the mean.  k_rbsp and
 * k_parse run on an internal parse stream, k_transform on an internal
 * transform stream and the rest on an internal recon stream, over three sets
 * of parse outputs, so decode n+2's parse, decode n+1's transform and decode
 * n's reconstruction overlap (HEIFGPU_PIPELINE=2: two sets, the transform on
 * the recon stream). */
int heifgpu_set_timing(heifgpu_ctx *ctx, int enable);
int heifgpu_stage_times(heifgpu_ctx *ctx, float ms[6]);
/* convenience: prepare + decode + status + free */
int heifgpu_decode_batch(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n, const heifgpu_planes *out,
                         void *stream, uint32_t *status);

/* Gather of a tile split: copies the visible windows of the grid tiles k with
 * k % tile_stride == tile_offset from `src` (planes decoded by a batch with
 * those options) into `dst` (full-size planes) with one kernel launch on
 * `stream`, a stream of dst's device.  src may live on another device: a
 * pointer of this process (peer access is enabled here) or a peer process's
 * planes mapped with heifgpu_ipc_open; the kernel reads them over xGMI.
 * Ordering: the copy reads src when it runs on `stream`, so the caller must
 * order `stream` after the decode that wrote src (synchronise that decode, or
 * make `stream` wait for an event recorded after it; across processes, the
 * owner synchronises before it signals the gathering process).  `info`
 * describes the image (heifgpu_image_get_info). */
int heifgpu_gather_tiles(const heifgpu_image_info *info, const heifgpu_planes *dst, const heifgpu_planes *src,
                         uint32_t tile_stride, uint32_t tile_offset, void *stream);

/* Cross-process device memory (the tile split with one process per GPU):
 * heifgpu_ipc_export describes the device allocation holding `dev_ptr` (a HIP
 * IPC handle plus the pointer's offset in it); another process passes the
 * 72 bytes (e.g. over torch.distributed) to heifgpu_ipc_open, which maps the
 * allocation on `device` and returns the same byte's address there.
 * heifgpu_ipc_close unmaps a pointer heifgpu_ipc_open returned.  The owner
 * must keep the allocation alive until every importer has closed it. */
typedef struct {
    uint8_t handle[64];  /* hipIpcMemHandle_t */
    uint64_t offset;     /* dev_ptr - allocation base */
} heifgpu_ipc_handle;
int heifgpu_ipc_export(const void *dev_ptr, heifgpu_ipc_handle *out);
int heifgpu_ipc_open(int device, const heifgpu_ipc_handle *h, void **dev_ptr);
int heifgpu_ipc_close(void *dev_ptr);

/* ---- YCbCr -> RGB with the irot rotation (libheif's default output) -------
 * Converts one decoded image (planes as written by heifgpu_batch_decode,
 * `info` from heifgpu_image_get_info) into interleaved 8-bit R,G,B at `rgb`
 * (device, caller-owned, rgb_pitch bytes per row), rotated anticlockwise by
 * info->rotation * 90 degrees: the output is height x width for rotation 1
 * and 3.  Matrix from info->matrix_coeffs (H.273: 1 BT.709, 9 BT.2020 NCL,
 * anything else BT.601), range from info->full_range, 4:2:0 / 4:2:2 chroma by
 * sample replication, samples above 8 bits rounded down to 8.  Fixed point: 16
 * fractional bits, round half up, clip to 0..255.  Asynchronous on `stream`.
 * The call takes no image handle, so heifgpu_image_set_chroma_upsampling does not
 * reach it: chroma here is always replicated. */
int heifgpu_ycbcr_to_rgb(heifgpu_ctx *ctx, const heifgpu_image_info *info, const heifgpu_planes *in, void *rgb,
                         int32_t rgb_pitch, void *stream);

/* ---- display-ready output: clap / irot / imir, alpha, 8 or 16 bits, batched --
 * (added within ABI 6: new entry points only.)
 * heifgpu_image_get_display (host only, no device) reports how the decoded
 * image is shown.  The item's transformative properties are applied in the
 * order its 'ipma' entry lists them (ISO/IEC 23008-12 6.5; several of a kind
 * are legal) and folded into one map: output pixel (ox, oy) shows decoded sample
 *     src_x = m[0]*ox + m[1]*oy + t[0],   src_y = m[2]*ox + m[3]*oy + t[1],
 * m one of the eight signed permutation matrices.  'clap' is the crop
 * img[top:top+ch, left:left+cw] with cw = round_half_up(widthN/widthD),
 * left = round_half_up(horizOffN/horizOffD + (W - cw)/2) (same for ch, top; W x H
 * the image at that point of the chain; exact integer arithmetic); a zero or
 * negative denominator, an empty rectangle or one not inside W x H fails the
 * parse (HEIFGPU_E_PARSE).  'irot' turns anticlockwise by 90 degrees per unit.
 * 'imir' axis 0 mirrors about a vertical axis (left and right swap), axis 1
 * about a horizontal one.  alpha_item_id is the first 'auxl' image of the item
 * whose 'auxC' type is urn:mpeg:hevc:2015:auxid:1 or
 * urn:mpeg:mpegB:cicp:systems:auxiliary:alpha (a gain map or depth map is not
 * alpha; heifgpu_image_info.aux_item_id still is the first 'auxl' of any
 * type); alpha_premultiplied reports a 'prem' reference, nothing is
 * un-premultiplied. */
typedef struct {
    uint32_t out_width, out_height;   /* displayed size */
    int32_t  m[4], t[2];              /* output -> source map, above */
    uint32_t n_transforms;            /* clap / irot / imir boxes folded in */
    uint32_t alpha_item_id;           /* 0: none */
    uint32_t alpha_premultiplied;
} heifgpu_display_info;
int heifgpu_image_get_display(const heifgpu_image *img, heifgpu_display_info *out);

enum { HEIFGPU_PIX_RGB8 = 0, HEIFGPU_PIX_RGBA8 = 1, HEIFGPU_PIX_RGB16 = 2, HEIFGPU_PIX_RGBA16 = 3 };
typedef struct { void *pixels; int32_t pitch; } heifgpu_surface;   /* device, caller-owned, bytes per row */
/* Renders n decoded images (in[i]: planes as written by heifgpu_batch_decode
 * for imgs[i]) into out[i] as interleaved R,G,B(,A) through each image's display
 * map, with ONE kernel launch whatever n and the sizes are.  The images may
 * differ in size, orientation, chroma format and matrix; their samples (and
 * those of the alpha images) must all be 1 byte or all 2 bytes wide, and n is
 * at most 65535.  Asynchronous on `stream`; calls issued back to back each keep
 * their own descriptors (a ring of staging slots; a call waits on the host
 * only for the call four before it).
 * 8-bit formats: exactly heifgpu_ycbcr_to_rgb's arithmetic (samples shifted
 * down to 8 bits), so HEIFGPU_PIX_RGB8 of an image whose only transform is
 * 'irot' is byte-identical to it.  16-bit formats: native-endian uint16 at the
 * image's own bit depth B (8..12), computed at that depth: luma offset
 * 16 << (B-8) (limited range) or 0, chroma centre 1 << (B-1), limited-range
 * scales ((1<<B)-1) / (219<<(B-8)) and ((1<<B)-1) / (224<<(B-8)) rounded to
 * 16.16 the same way, clip to (1<<B)-1; pixels and pitch must be even.
 * Alpha (RGBA formats): alpha_imgs NULL or alpha_imgs[i] NULL stores the
 * maximum (255, or (1<<B)-1).  Otherwise alpha_in[i].plane[0] is the decoded
 * luma of alpha_imgs[i] (bit depth Ba, full range), addressed through the
 * colour image's map: 8-bit formats store a >> (Ba-8); 16-bit formats store a
 * shifted to depth B (a << (B-Ba) or a >> (Ba-B): exact only when Ba == B).
 * An alpha image whose decoded size differs from its colour image's is
 * HEIFGPU_E_UNSUPPORTED, reported before anything is launched.  The RGB
 * formats ignore the alpha arguments.  4:0:0 gives R = G = B.  A pitch below
 * the row size is HEIFGPU_E_INVALID. */
int heifgpu_render_batch(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                         const heifgpu_planes *in,
                         const heifgpu_image *const *alpha_imgs,
                         const heifgpu_planes *alpha_in,
                         uint32_t format, const heifgpu_surface *out, void *stream);

/* ---- scaled render: a window of the displayed picture, area-averaged --------
 * (added within ABI 6: new entry points only.)
 * Let D be the displayed picture of an image in the chosen format, exactly what
 * heifgpu_render_batch writes (dw x dh = heifgpu_display_info.out_width x
 * out_height).  A heifgpu_scale names a window (cx, cy, cw, ch) of D and a
 * rendered size ow x oh; the result R is the exact area average of the window
 * on that grid, per channel (alpha is averaged like a colour, nothing is
 * premultiplied), in integers:
 *     wx(X, i) = max(0, min((i+1)*ow, (X+1)*cw) - max(i*ow, X*cw))     i in [0, cw)
 *     wy(Y, j) = max(0, min((j+1)*oh, (Y+1)*ch) - max(j*oh, Y*ch))     j in [0, ch)
 *     acc      = sum_j sum_i wy(Y,j) * wx(X,i) * D[cy + j][cx + i][c]
 *     R[Y][X][c] = floor((2*acc + cw*ch) / (2*cw*ch))                  (round half up)
 * with no intermediate rounding (acc is a 64-bit sum).  ow == cw and oh == ch
 * gives the window of D byte for byte; integer ratios give the rounded mean of
 * each block; enlargement follows the same formula.  The average is taken over
 * converted pixels, not over the YCbCr planes.  (The area average is a box
 * filter; heifgpu_render_batch_resampled, further down, offers Pillow's
 * bilinear and bicubic filters on the same window.) */
typedef struct {
    uint32_t out_width, out_height;   /* rendered size, each 1..65535 */
    uint32_t x, y, width, height;     /* window of the displayed picture, in its coordinates;
                                         width == 0 && height == 0: the whole picture */
} heifgpu_scale;
enum { HEIFGPU_FIT_STRETCH = 0, HEIFGPU_FIT_CONTAIN = 1, HEIFGPU_FIT_COVER = 2 };
/* The spec that shows a dw x dh picture (d->out_width x out_height) in a
 * box_w x box_h box (host only, no device; exact 64-bit integers, round =
 * round half up):
 * STRETCH: the whole picture to box_w x box_h.
 * CONTAIN: the whole picture; if dw*box_h >= dh*box_w: ow = box_w,
 *   oh = max(1, round(dh*box_w / dw)); otherwise oh = box_h,
 *   ow = max(1, round(dw*box_h / dh)).
 * COVER: box_w x box_h out of a centred window of the box's aspect; if
 *   dw*box_h >= dh*box_w: height = dh, width = max(1, round(dh*box_w / box_h)),
 *   x = (dw - width) / 2 rounded down, y = 0; otherwise width = dw,
 *   height = max(1, round(dw*box_h / box_w)), x = 0, y = (dh - height) / 2.
 * A zero box side or an unknown mode is HEIFGPU_E_INVALID. */
int heifgpu_scale_fit(const heifgpu_display_info *d, uint32_t box_w, uint32_t box_h, uint32_t mode,
                      heifgpu_scale *out);
/* heifgpu_render_batch with a heifgpu_scale per image: out[i] receives
 * scale[i].out_width x out_height pixels.  Everything not named here is as in
 * heifgpu_render_batch (formats, alpha rules, mixed batches, n <= 65535, the
 * descriptor ring shared with it, ONE kernel launch whatever the sizes and
 * ratios).  All checks run before anything is launched: a window that is empty
 * (other than the 0, 0 "whole" form) or not inside dw x dh, a rendered side of
 * 0 or above 65535 and a pitch below the rendered row are HEIFGPU_E_INVALID; a
 * window side above 65535 is HEIFGPU_E_UNSUPPORTED.  Tuned for reduction;
 * identity and enlargement are exact but slower than heifgpu_render_batch. */
int heifgpu_render_batch_scaled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                const heifgpu_planes *in,
                                const heifgpu_image *const *alpha_imgs,
                                const heifgpu_planes *alpha_in,
                                uint32_t format, const heifgpu_scale *scale,
                                const heifgpu_surface *out, void *stream);

/* ---- tensor render: crop, flip, normalise to f32 / f16 / bf16 ---------------
 * (added within ABI 6: new entry points only.)
 * Let R be exactly what heifgpu_render_batch_scaled writes for an image, a
 * heifgpu_scale and the pixel format `src` (one of HEIFGPU_PIX_*): integers,
 * C = 3 or 4 channels, oh x ow.  The tensor render writes, for every channel c,
 *     Rf         = R, columns reversed if flip & 1, rows reversed if flip & 2
 *                  (the flip acts on the rendered picture)
 *     F[Y][X][c] = fadd_rn(fmul_rn((float)Rf[Y][X][c], a[c]), b[c])
 *                  (binary32, two roundings, never a fused multiply-add)
 *     out        = F rounded to the element type: binary32 as is; binary16 and
 *                  bfloat16 by round-to-nearest-even, gradual underflow for
 *                  binary16, overflow to infinity
 * so float32 arithmetic on the host (numpy) reproduces it bit for bit.  a[c] and
 * b[c] are the caller's; the C used must be finite.  A value whose binary32
 * intermediate (the product or the sum) is subnormal is outside the contract.
 * A normaliser passes a = 1 / (maxv * std), b = -mean / std, maxv = 255 or
 * (1 << B) - 1; with a 16-bit src the images of one call share a and b whatever
 * their bit depths are, which is the caller's concern.
 * HEIFGPU_LAYOUT_CHW puts element (c, Y, X) at data + c*stride_c + Y*stride_y +
 * X*size, HEIFGPU_LAYOUT_HWC at data + Y*stride_y + (X*C + c)*size (size = 4 or
 * 2 bytes; strides in bytes, so n images can be the slices of one (N, C, h, w)
 * or (N, h, w, C) tensor).  Overlapping planes are the caller's business.
 * flip[i] is 0..3 (flip NULL: none); it is folded into the image's display map
 * behind the window, as one more 'imir'.
 * Everything not named here is as in heifgpu_render_batch_scaled: alpha rules,
 * mixed sizes, orientations and chroma formats, n <= 65535, the descriptor ring
 * shared with it, one descriptor copy and ONE kernel launch whatever n, the
 * sizes and the flips are (the same kernel, ending in another store).  All its
 * checks apply and, like them, run before anything is launched and before ctx
 * is looked at; HEIFGPU_E_INVALID besides for an unknown src, elem or layout, a
 * flip above 3, a non-finite a or b among the C used, data NULL or not aligned
 * to the element size, a stride_y below the row or not a multiple of the element
 * size and, for CHW, a stride_c not a multiple of the element size.
 * There is no full-size fast path: a full-size tensor is the identity window
 * through this kernel, exact but slower than heifgpu_render_batch (which has
 * no tensor store). */
enum { HEIFGPU_ELEM_F32 = 0, HEIFGPU_ELEM_F16 = 1, HEIFGPU_ELEM_BF16 = 2 };
enum { HEIFGPU_LAYOUT_CHW = 0, HEIFGPU_LAYOUT_HWC = 1 };
typedef struct {
    uint32_t src, elem, layout;       /* HEIFGPU_PIX_*, HEIFGPU_ELEM_*, HEIFGPU_LAYOUT_* */
    float a[4], b[4];                 /* per channel; the first C are used */
} heifgpu_tensor_format;
typedef struct {
    void *data;                       /* device, caller-owned */
    int64_t stride_c, stride_y;       /* bytes; stride_c is unused for HWC */
} heifgpu_tensor_surface;
int heifgpu_render_batch_tensor(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                const heifgpu_planes *in,
                                const heifgpu_image *const *alpha_imgs,
                                const heifgpu_planes *alpha_in,
                                const heifgpu_tensor_format *fmt, const heifgpu_scale *scale,
                                const uint32_t *flip, const heifgpu_tensor_surface *out, void *stream);

/* ---- colour-managed render: ICC / nclx source to sRGB or Display P3 ----------
 * (added within ABI 6: new entry points only.)
 * The renders above apply the colr matrix and range and nothing else: their RGB
 * is in the image's own colour space.  The calls below describe that space and
 * convert every RGB triple of a render to a destination space in the same launch.
 *
 * THE SOURCE (ISO/IEC 23008-12 6.5.5).  Every colr of the decoded item is kept.
 * An ICC profile ('prof' / 'rICC') defines the colour space; an nclx in the same
 * item still supplies the YCbCr matrix and range.  Without a profile an nclx
 * defines it; with no colr, or for colour_primaries or transfer_characteristics
 * 2 (unspecified), sRGB is assumed.
 *   ICC: three-component matrix/TRC profiles, v2 and v4, data space 'RGB ', PCS
 *   'XYZ ': rXYZ / gXYZ / bXYZ (XYZType, D50-adapted as they are; chad and wtpt
 *   are read past) and rTRC / gTRC / bTRC, which may share an offset: 'curv' with
 *   count 0 (identity), 1 (u8.8 gamma) or n (a table, interpolated linearly) and
 *   'para' function types 0..4 (ICC.1:2010 table 68).  LUT-only profiles, a Lab
 *   PCS, another data space or a 'para' type above 4 are HEIFGPU_E_UNSUPPORTED; a
 *   size field beyond the box, a tag offset or length outside the profile, a
 *   'curv' count beyond its tag are HEIFGPU_E_PARSE.  Both are answered when a
 *   transform is asked for, never at parse or decode: such files decode as before.
 *   nclx: primaries 1 (BT.709 / sRGB), 9 (BT.2020), 12 (P3 D65) from their
 *   chromaticities to XYZ, Bradford-adapted to the ICC D50 white (s15.16 F6D6
 *   10000 D32D), in double.  Transfer 1, 6, 13, 14, 15: the sRGB curve (709-coded
 *   stills are shown as sRGB, as browsers and libheif show them); 8: linear; 4:
 *   gamma 2.2; 16 (PQ) and 18 (HLG) need tone mapping, which
 *   heifgpu_color_transform_make_hdr (below, "HDR render") gives on request: here
 *   they, and every other code, are HEIFGPU_E_UNSUPPORTED.
 * THE DESTINATIONS both encode with the sRGB curve g; colourants (X Y Z, s15.16):
 *   HEIFGPU_CS_SRGB        R 6FA2 38F5 0390      G 6299 B785 18DA   B 24A0 0F84 B6CF
 *   HEIFGPU_CS_DISPLAY_P3  R 83DF 3DBF FFFFFFBB  G 4ABF B137 0AB9   B 2838 110B C8B9
 * THE TRANSFORM is made for the depth B the render computes at (8 for the 8-bit
 * formats, the image's depth, at most 12, for the 16-bit ones), maxv = (1<<B)-1:
 *   in_lut[c][v] = round_half_up(65535 * clamp(f_c(v / maxv), 0, 1)),  v in [0, 1<<B),
 *                  f_c channel c's TRC
 *   m            = inv(Dst) * Src in double, each row divided by its sum (the s15.16
 *                  colourants of two spaces sum to whites that differ in the last
 *                  digits, sRGB's to F6DB FFFE D339 and Display P3's to F6D6 10001
 *                  D32D: row sums of 1 +- 3e-4 otherwise), then in Q14, each entry
 *                  rounded to nearest (m_rounded), then the largest entry of each row
 *                  adjusted so that the row sums to 16384 exactly (neutral in,
 *                  neutral out when the TRCs are equal); an nclx source of the
 *                  destination's own primaries code gets exactly 16384 * I
 *   out_lut[i]   = round_half_up(16 * maxv * g(min(16 * i, 65535) / 65535)),  i in [0, 4096]
 *                  (1/16 code; 16 bits hold it up to B = 12)
 *   identity     = m == 16384 * I and every code 0..maxv of every channel maps to
 *                  itself; a render given an identity transform takes the unmanaged path
 * Per pixel, with (c_0, c_1, c_2) the R, G, B integers the unmanaged render gives:
 *   L_c  = in_lut[c][c_c]
 *   L'_k = clamp((m[3k]*L_0 + m[3k+1]*L_1 + m[3k+2]*L_2 + 8192) >> 14, 0, 65535)
 *          (64-bit sum, arithmetic shift)
 *   i = L'_k >> 4, f = L'_k & 15
 *   out_k = (out_lut[i]*(16-f) + out_lut[i+1]*f + 128) >> 8
 * Alpha is not touched.  numpy reproduces this bit for bit (tests/color_ref.py);
 * kernels/color_xform.hpp is its one statement in code, shared by the kernels and
 * heifgpu_color_apply.  The scaled and tensor renders transform the rounded
 * average R (what heifgpu_render_batch_scaled writes), not each source pixel:
 * averaging in linear light is another feature, "Linear-light scaled render"
 * further down, and is not done here. */
enum { HEIFGPU_CS_SRGB = 0, HEIFGPU_CS_DISPLAY_P3 = 1 };
enum { HEIFGPU_COLOR_NONE = 0, HEIFGPU_COLOR_ICC = 1, HEIFGPU_COLOR_NCLX = 2 };
typedef struct {
    uint32_t kind;                    /* HEIFGPU_COLOR_*: what defines the colour space */
    uint32_t has_nclx;                /* the item has an nclx colr (beside a profile or alone) */
    uint32_t primaries, transfer;     /* of that nclx; 2 (unspecified) without one */
    uint32_t icc_size;                /* bytes of the profile, 0 without one */
    int32_t status;                   /* HEIFGPU_OK, or what a transform of this source answers */
    double colorants[9];              /* X Y Z of R, then of G, then of B (D50); zeros unless status is OK */
} heifgpu_color_info;
typedef struct {
    uint32_t bits;                    /* B */
    uint32_t identity;
    uint32_t dst;                     /* HEIFGPU_CS_* */
    uint32_t tone;                    /* 0 from every call but heifgpu_color_transform_make_hdr: HEIFGPU_TONE_* */
    int32_t m[9];
    int32_t m_rounded[9];             /* m before the row fix-up (informative) */
    uint16_t in_lut[3][4096];         /* the first 1 << B entries of each are used */
    uint16_t out_lut[4098];           /* 4097 used */
} heifgpu_color_transform;
/* host only, always HEIFGPU_OK for a parsed image */
int heifgpu_image_get_color(const heifgpu_image *img, heifgpu_color_info *out);
/* host only: the profile's bytes into buf (cap bytes; buf NULL or cap too small:
 * only *len is set, to the profile's size; 0 without a profile) */
int heifgpu_image_get_icc(const heifgpu_image *img, uint8_t *buf, size_t cap, size_t *len);
/* host only: the transform of img's colour space to dst at depth bits (8..12). */
int heifgpu_color_transform_make(const heifgpu_image *img, uint32_t dst, uint32_t bits,
                                 heifgpu_color_transform *out);
/* host only: the per-pixel formula over n_pixels R G B triples of codes
 * 0..maxv (a larger code is HEIFGPU_E_INVALID); an identity transform is applied
 * like any other.  rgb_out may be rgb_in. */
int heifgpu_color_apply(const heifgpu_color_transform *t, const uint16_t *rgb_in, size_t n_pixels,
                        uint16_t *rgb_out);
/* The three renders with one transform pointer per image: xf[i] NULL or an
 * identity transform leaves image i exactly as the unmanaged call writes it (xf
 * NULL: all of them, and the call is the unmanaged call).  xf[i]->bits must be
 * the depth image i is rendered at, else HEIFGPU_E_INVALID.  Still ONE launch and
 * one descriptor copy whatever the mix of sources and depths is.  The tables live
 * in device memory owned by the context, cached by content: a steady-state call
 * uploads nothing, and a cached table is never rewritten (the cache is emptied,
 * after a device synchronise, when it holds 256 tables).  The transforms are read
 * during the call only. */
int heifgpu_render_batch_color(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                               const heifgpu_planes *in,
                               const heifgpu_image *const *alpha_imgs,
                               const heifgpu_planes *alpha_in,
                               uint32_t format, const heifgpu_color_transform *const *xf,
                               const heifgpu_surface *out, void *stream);
int heifgpu_render_batch_scaled_color(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                      const heifgpu_planes *in,
                                      const heifgpu_image *const *alpha_imgs,
                                      const heifgpu_planes *alpha_in,
                                      uint32_t format, const heifgpu_scale *scale,
                                      const heifgpu_color_transform *const *xf,
                                      const heifgpu_surface *out, void *stream);
int heifgpu_render_batch_tensor_color(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                      const heifgpu_planes *in,
                                      const heifgpu_image *const *alpha_imgs,
                                      const heifgpu_planes *alpha_in,
                                      const heifgpu_tensor_format *fmt, const heifgpu_scale *scale,
                                      const uint32_t *flip,
                                      const heifgpu_color_transform *const *xf,
                                      const heifgpu_tensor_surface *out, void *stream);

/* ---- HDR render: opt-in BT.2390 tone mapping of PQ and HLG sources -----------
 * (added within ABI 6: new entry points only; no struct above changes its layout.)
 * Without the calls below nothing changes: a PQ / HLG source is refused as above.
 *
 * WHAT THE FILE CARRIES.  Two more item properties of the decoded item are kept, the
 * first of each kind (plain boxes, not FullBoxes):
 *   clli  u16 max_content_light_level (MaxCLL), u16 max_pic_average_light_level (MaxFALL), cd/m2
 *   mdcv  3 x (u16 x, u16 y) primaries, u16 x 2 white point, u32 max and u32 min
 *         display mastering luminance in 0.0001 cd/m2
 * A box shorter than its fields (4 and 24 bytes) is HEIFGPU_E_PARSE when a tone
 * transform is asked for, never at parse or decode (the rule of the ICC profiles).
 * WHEN IT APPLIES.  The item's colour space is defined by an nclx (no ICC profile: a
 * profile still wins and gets no tone stage) of primaries 1, 2 (taken as 1), 9 or 12
 * and transfer 16 (PQ, SMPTE ST 2084) or 18 (HLG, ARIB STD-B67 / BT.2100).  For every
 * other image heifgpu_color_transform_make_hdr gives exactly what
 * heifgpu_color_transform_make gives (tone == 0), errors included.
 * THE PEAKS.  Source peak Lsrc in cd/m2: peak_nits if > 0, else MaxCLL if non-zero,
 * else the mdcv maximum if non-zero, else 1000; clamped to [203, 10000].  HLG always
 * uses the BT.2100 nominal display, Lw = 1000 cd/m2 and system gamma 1.2: its Lsrc is
 * 1000 whatever the file or the caller says.  The destination peak is the SDR
 * reference white of BT.2408, 203 cd/m2; black is 0 on both sides.
 * THE TONE STAGE sits between in_lut and the matrix; everything from the matrix on
 * is the transform above, unchanged (m = inv(Dst) * Src of the nclx primaries, rows
 * normalised, Q14; out_lut).  U = 65535 stands for 203 cd/m2.
 *   in_lut32[c][v] = round_half_up(U * F(v / maxv) / 203)                      (u32, < 2^22)
 *       PQ:  F = the ST 2084 EOTF in cd/m2 (at most 10000)
 *       HLG: F = 1000 * E, E the BT.2100 HLG inverse OETF (scene light, before the OOTF)
 *   w[3]: the Y row of the source primaries' RGB -> XYZ matrix (D65, from the
 *       chromaticities) divided by its sum, in Q14 rounded to nearest, the largest
 *       entry then adjusted so that the three sum to 16384 exactly
 *   Y = (w0*L0 + w1*L1 + w2*L2 + 8192) >> 14                                   (64-bit sum)
 *   the gain g(Y), a table on a floating index (32 nodes per octave from 64 on):
 *       Y < 64:  g = T[Y]
 *       else     e = bitlength(Y) - 6, idx = 32 + 32 e + ((Y >> e) - 32), frac = Y & ((1 << e) - 1)
 *                g = (T[idx] * ((1 << e) - frac) + T[idx + 1] * frac + (1 << (e - 1))) >> e   (64 bits)
 *       T: 577 u32 entries, node k at Y_k = k for k < 64, else (32 + ((k - 32) & 31)) << ((k - 32) >> 5)
 *       T[k] = round_half_up(2^24 * min(G(Y_k), 1)), with Yn = 203 * Y_k / U (cd/m2)
 *       (24 fractional bits: G falls to 203 / 12992 = 0.016, where 16 bits left a relative
 *       step of 5e-4 and more than one 8-bit code of error on a saturated dark channel):
 *       PQ:  G = EETF(Yn) / Yn, G(0) = 1
 *       HLG: Ys = Yn / 1000, Yd = 1000 * Ys^1.2, G = Ys^0.2 * EETF(Yd) / Yd, G(0) = 0
 *            (the BT.2100 OOTF on luminance, then the same tone curve at Lsrc = 1000)
 *       EETF is BT.2390's (5.4.1), in double.  With N the ST 2084 inverse EOTF of x / 10000:
 *            E1 = (N(min(x, Lsrc)) - N(0)) / (N(Lsrc) - N(0)),   maxLum = (N(203) - N(0)) / (N(Lsrc) - N(0))
 *            KS = 1.5 maxLum - 0.5;  E1 <= KS: EETF(x) = min(x, Lsrc) itself;  else with t = (E1 - KS) / (1 - KS)
 *            E2 = (2t^3 - 3t^2 + 1) KS + (t^3 - 2t^2 + t)(1 - KS) + (3t^2 - 2t^3) maxLum
 *            EETF(x) = EOTF(E2 (N(Lsrc) - N(0)) + N(0));  no black lift (minLum = 0); inputs above Lsrc clip to it
 *   L''_c = min((L_c * g + 2^23) >> 24, 65535)                                  (64-bit product)
 *   then L'_k, i, f and out_k of the transform above, with L'' in the place of L.
 * Out-of-gamut results clip at the existing clamp (no gamut mapping).  A tone
 * transform is never an identity.  numpy reproduces this bit for bit
 * (tests/tone_ref.py); kernels/color_xform.hpp is its one statement in code. */
enum { HEIFGPU_TONE_NONE = 0, HEIFGPU_TONE_BT2390 = 1 };
enum { HEIFGPU_HDR_HAS_CLLI = 1, HEIFGPU_HDR_HAS_MDCV = 2 };
#define HEIFGPU_TONE_ENTRIES 577
typedef struct {
    uint32_t transfer;                /* 16 (PQ), 18 (HLG); 0: not an nclx-defined PQ / HLG item */
    uint32_t present;                 /* HEIFGPU_HDR_HAS_* of the boxes the item carries */
    uint32_t max_cll, max_fall;       /* clli, cd/m2; 0 without the box (or for a short one) */
    uint32_t mastering_max, mastering_min;  /* mdcv, 0.0001 cd/m2; 0 without the box (or for a short one) */
    int32_t status;                   /* HEIFGPU_OK, or what a tone transform of this item answers */
    uint32_t reserved;
} heifgpu_hdr_info;
typedef struct {
    heifgpu_color_transform base;     /* base.tone != 0; base.in_lut is not used (zeros) */
    uint32_t in_lut32[3][4096];       /* the first 1 << B entries of each are used */
    int32_t w[3];
    uint32_t transfer;                /* 16 or 18 */
    uint32_t T[HEIFGPU_TONE_ENTRIES + 1];  /* 577 used */
    double Lsrc;                      /* cd/m2, as used */
} heifgpu_hdr_transform;
/* host only, always HEIFGPU_OK for a parsed image */
int heifgpu_image_get_hdr(const heifgpu_image *img, heifgpu_hdr_info *out);
/* host only: heifgpu_color_transform_make with a tone stage on request.  tone_map
 * HEIFGPU_TONE_NONE: out->base is what heifgpu_color_transform_make gives, the rest
 * zeros.  HEIFGPU_TONE_BT2390: the same for every image but an nclx-defined PQ / HLG
 * one, whose tone transform is made (peak_nits <= 0: from the file).  A transform
 * whose base.tone is non-zero is passed on as &out->base: heifgpu_color_apply and
 * every render that takes heifgpu_color_transform pointers read the whole
 * heifgpu_hdr_transform behind such a pointer.  Still one descriptor copy and one
 * launch per render call, whatever the mix of tone, managed and unmanaged images. */
int heifgpu_color_transform_make_hdr(const heifgpu_image *img, uint32_t dst, uint32_t bits, uint32_t tone_map,
                                     double peak_nits, heifgpu_hdr_transform *out);

/* ---- chroma upsampling: replicate (default) or bilinear at the signalled location ----
 * (added within ABI 6: new entry points only; no existing struct changes layout.)
 * By default every render turns 4:2:0 / 4:2:2 chroma into RGB by replication: a luma
 * sample reads the one chroma sample of its cell.  An image set to
 * HEIFGPU_CHROMA_BILINEAR renders as if Cb and Cr had first been upsampled to the luma
 * grid by the filter below and the unchanged pipeline (>> shift, the matrix, the clip,
 * then area average / filter / colour transform / tone map / tensor epilogue) ran on that
 * 4:4:4 picture.  Integers only:
 *   t  = the SPS VUI's chroma_sample_loc_type_top_field (0 without a VUI or with
 *        chroma_loc_info_present_flag 0; above 5 fails the parse), or the caller's override;
 *   4:2:0: px = t & 1 (0: co-sited with even luma columns, 1: midway);
 *          py = 1 (midway) for t >> 1 == 0, 0 (top) for 1, 2 (bottom) for 2;
 *   4:2:2: px = 0, no vertical filter; 4:4:4 and 4:0:0: the setting has no effect;
 *   luma column x: u = 2x - px, i0 = floor(u / 4), f = u & 3: chroma columns i0 and i0 + 1,
 *        each clamped to [0, Wc - 1], weights 4 - f and f; rows likewise with v = 2y - py
 *        (4:2:2: row y, weights 4 and 0);
 *   C'(x, y) = (sum wy * wx * C + 8) >> 4 on the decoded samples at the image's depth.
 * x, y, Wc, Hc are those of the decoded planes: a clap crop interpolates across its own
 * edge from real samples, only the edge of the coded picture clamps.
 * The setting lives on the image handle, where every render call and
 * heifgpu_window_source_rect* read it, so the two cannot disagree about the samples read.
 * heifgpu_image_set_chroma_upsampling is host only; loc is -1 (the file's location) or
 * 0..5, anything else HEIFGPU_E_INVALID.  It must not be called while a render of that
 * image is being submitted from another thread (a submitted render is not affected).
 * A call with one bilinear image runs kernels of its own (one launch, as ever); a
 * call without one runs what it ran before, bit for bit.
 * heifgpu_chroma_upsample is the rule on the host for one plane: `in` holds w_c x h_c
 * samples (uint8 for bits == 8, else uint16; pitch bytes a row), the luma-grid rectangle
 * [x0, x0 + w) x [y0, y0 + h) of C' goes to `out` (same type, out_pitch bytes a row).
 * chroma_format_idc 1 or 2, loc 0..5, the rectangle inside 2 * w_c columns and 2 * h_c
 * (4:2:2: h_c) rows, else HEIFGPU_E_INVALID. */
enum { HEIFGPU_CHROMA_REPLICATE = 0, HEIFGPU_CHROMA_BILINEAR = 1 };
typedef struct {
    uint32_t loc;           /* chroma_sample_loc_type_top_field of the first coded picture's SPS, 0..5 */
    uint32_t signalled;     /* 1 if the SPS carries chroma_loc_info */
    int32_t  loc_override;  /* the caller's location, -1: none */
    uint32_t mode;          /* HEIFGPU_CHROMA_* */
    uint32_t sub_width_c, sub_height_c;
} heifgpu_chroma_info;
int heifgpu_image_get_chroma(const heifgpu_image *img, heifgpu_chroma_info *out);
int heifgpu_image_set_chroma_upsampling(heifgpu_image *img, uint32_t mode, int32_t loc);
int heifgpu_chroma_upsample(const void *in, uint32_t w_c, uint32_t h_c, int32_t pitch, uint32_t bits,
                            uint32_t chroma_format_idc, uint32_t loc, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                            void *out, int32_t out_pitch);

/* ---- Gain-map HDR render: base picture x gain map -> linear half-float or PQ --------
 * (added within ABI 6: new entry points only; no existing struct, call or kernel changes.)
 * An SDR base picture with a gain map is shown as HDR: every pixel of the base, in linear
 * light, is multiplied by a factor read from a second, usually smaller, picture.
 *
 * WHERE THE MAP COMES FROM.  Two sources; the first wins if a file has both:
 *   ISO 21496-1: an item of type 'tmap' whose 'dimg' reference lists [base item, gain-map
 *     item] with the parsed image as the base.  Its data (through iloc: mdat, idat, several
 *     extents) is kept unread at parse and read when a transform or heifgpu_image_get_gain
 *     asks (the rule of the ICC profiles: such a file always parses and decodes).  Layout,
 *     big-endian ("parity unpinned": written from memory of the standard and of what libavif
 *     writes; this layout is the contract here):
 *       u8 version (0), u16 minimum_version (0), u16 writer_version,
 *       u8 flags (bit 7 is_multichannel, bit 6 use_base_colour_space),
 *       u32/u32 base HDR headroom N/D, u32/u32 alternate HDR headroom N/D,
 *       then per channel (1, or 3 when multichannel): s32/u32 gain_map_min, s32/u32
 *       gain_map_max, u32/u32 gamma, s32/u32 base_offset, s32/u32 alternate_offset.
 *     Headrooms, min and max are log2 values.  HEIFGPU_E_PARSE: a payload shorter than its
 *     fields (an item whose data cannot be fetched, or of more than 64 KiB, counts as empty),
 *     a zero denominator.  HEIFGPU_E_UNSUPPORTED: a version or minimum_version other
 *     than 0, multichannel, use_base_colour_space == 0, alternate headroom <= base headroom
 *     (an HDR base), gamma <= 0, |min|, |max| or a headroom above 8, an offset above 16 in
 *     magnitude.
 *   Apple: the first 'auxl' image of the item whose 'auxC' type is
 *     urn:com:apple:photo:2020:aux:hdrgainmap.  Its headroom lies in the Exif maker note,
 *     which this library does not read: the caller passes it.
 *
 * THE CONTRACT.  U = 65535 is the base picture's SDR white.  The base is W x H decoded
 * samples; the gain map is Wg x Hg decoded samples of depth Bg (8..12, luma plane only),
 * maxg = (1 << Bg) - 1; all four sides at most 65535.
 *   Base: (c0, c1, c2) are the integers the unmanaged render gives at the image's depth B;
 *     L_c = in_lut[c][c_c], the table heifgpu_color_transform_make builds for this item (same
 *     ICC / nclx rules and errors; a PQ / HLG base is HEIFGPU_E_UNSUPPORTED).
 *   Gain sample at decoded base position (sx, sy), aligned centres, exact integers:
 *     nx = (2 sx + 1) Wg - W, dx = 2 W, ix = floor(nx / dx), fx = floor(256 (nx - ix dx) / dx),
 *     x0 = clamp(ix, 0, Wg - 1), x1 = clamp(ix + 1, 0, Wg - 1); the same in y;
 *     g = ((256 - fy) ((256 - fx) G[y0][x0] + fx G[y0][x1])
 *          + fy ((256 - fx) G[y1][x0] + fx G[y1][x1]) + 128) >> 8       (Q8, 0 .. 256 maxg)
 *     (Wg == W gives the sample itself).
 *   Multiplier: i = g >> 8, f = g & 255, M = (T[i] (256 - f) + T[i + 1] f + 128) >> 8.  T holds
 *     maxg + 2 u32 entries with 16 fractional bits, each at most 2^24; the last repeats.  Built
 *     in double, rhu = round half up, w = clamp((log2(display_headroom) - Hbase) / (Halt - Hbase),
 *     0, 1), display_headroom <= 0 meaning full (w = 1):
 *     ISO:   T[v] = rhu(2^16 2^(w (min + (max - min) (v / maxg)^(1 / gamma)))),
 *            k_b = rhu(U base_offset), k_a = rhu(U alternate_offset)
 *     Apple: hr = headroom, or min(headroom, max(display_headroom, 1)) with a display_headroom;
 *            T[v] = rhu(2^16 (1 + (hr - 1) f709(v / maxg))), f709 the BT.709 inverse OETF
 *            (V < 0.081: V / 4.5, else ((V + 0.099) / 1.099)^(1 / 0.45)); k_b = k_a = 0; headroom
 *            is required and lies in [1, 256], else HEIFGPU_E_INVALID.  ("parity unpinned": as
 *            Apple's published description is remembered.  T is a public field: a caller who
 *            knows better fills it.)  An image without a map of either kind takes this rule.
 *   Apply:  H_c = clamp((((L_c + k_b) M + 2^15) >> 16) - k_a, 0, 2^24 - 1)     (64-bit product)
 *   Matrix: H'_k = clamp((m[3k] H_0 + m[3k+1] H_1 + m[3k+2] H_2 + 8192) >> 14, 0, 2^24 - 1),
 *     m the Q14 inv(Dst) Src of the colour-managed render with its row fix-up; destinations
 *     sRGB, Display P3 and, for these calls only, BT.2020 (HEIFGPU_CS_BT2020: the nclx
 *     primaries 9, Bradford-adapted to D50 in double).  Out of gamut clips.
 *   Encodings, 16 bits per sample, native-endian:
 *     linear (HEIFGPU_PIX_HDR_RGB16F / RGBA16F): F = fmul_rn((float)H'_k, c), c the binary32
 *       nearest to 1 / 65535, then binary16 by round-to-nearest-even: 1.0 is SDR white.  Alpha:
 *       fmul_rn((float)a, ca), a the alpha sample at its own depth Ba and ca the binary32
 *       nearest to 1 / ((1 << Ba) - 1), the same way; 1.0 without an alpha image.
 *     PQ (HEIFGPU_PIX_HDR_RGB16PQ / RGBA16PQ): codes at depth P in {10, 12, 16}, maxp =
 *       (1 << P) - 1, through a table E of 641 u32 entries on the tone transform's floating
 *       index extended to 2^24 (node k at Y_k = k for k < 64, else (32 + ((k - 32) & 31)) <<
 *       ((k - 32) >> 5)): E[k] = rhu(256 maxp N(min(sdr_white Y_k / U, 10000) / 10000)), N the
 *       ST 2084 inverse EOTF, sdr_white in cd/m2 (<= 0: 203).  v = E[H'] for H' < 64, else
 *       with e = bitlength(H') - 6, idx = 32 e + (H' >> e), frac = H' & ((1 << e) - 1):
 *       v = (E[idx] ((1 << e) - frac) + E[idx + 1] frac + (1 << (e - 1))) >> e; code = (v + 128) >> 8.
 *       Alpha: the 16-bit rule of heifgpu_render_batch at depth P (a << (P - Ba) or
 *       a >> (Ba - P); maxp without an alpha image).
 * numpy reproduces this bit for bit (tests/gain_ref.py); kernels/gain_xform.hpp is its one
 * statement in code, shared by the kernel and heifgpu_gain_apply. */
enum { HEIFGPU_GAIN_NONE = 0, HEIFGPU_GAIN_APPLE = 1, HEIFGPU_GAIN_ISO = 2 };
enum { HEIFGPU_CS_BT2020 = 2 };  /* a destination of heifgpu_gain_transform_make only */
enum { HEIFGPU_GAIN_LINEAR = 0, HEIFGPU_GAIN_PQ = 1 };
enum { HEIFGPU_PIX_HDR_RGB16F = 4, HEIFGPU_PIX_HDR_RGBA16F = 5, HEIFGPU_PIX_HDR_RGB16PQ = 6, HEIFGPU_PIX_HDR_RGBA16PQ = 7 };
#define HEIFGPU_GAIN_T_ENTRIES 4097   /* maxg + 2 at 12 bits */
#define HEIFGPU_GAIN_E_ENTRIES 641
typedef struct {
    uint32_t kind;                    /* HEIFGPU_GAIN_* */
    uint32_t gain_item_id;            /* the gain-map image item, 0 without one */
    int32_t status;                   /* HEIFGPU_OK, or what a transform answers (Apple: given a headroom) */
    uint32_t version, minimum_version, writer_version;   /* ISO; zeros otherwise */
    uint32_t multichannel, use_base_colour_space;
    double base_headroom, alternate_headroom;            /* log2 */
    double gain_min, gain_max, gamma, base_offset, alternate_offset;  /* of channel 0 */
} heifgpu_gain_info;
typedef struct {
    uint32_t bits;                    /* B, the base image's depth */
    uint32_t gain_bits;               /* Bg */
    uint32_t dst;                     /* HEIFGPU_CS_*, BT.2020 included */
    uint32_t encoding;                /* HEIFGPU_GAIN_LINEAR / _PQ: the formats it serves */
    uint32_t pq_bits;                 /* P; 0 for the linear encoding */
    uint32_t kind;                    /* HEIFGPU_GAIN_*: the rule T was filled by (informative) */
    int32_t m[9];
    int32_t k_b, k_a;
    double weight, headroom, sdr_white;   /* w, hr (Apple) and sdr_white as used (informative) */
    uint16_t in_lut[3][4096];         /* the first 1 << B entries of each are used */
    uint32_t T[HEIFGPU_GAIN_T_ENTRIES + 1];  /* maxg + 2 used */
    uint32_t E[HEIFGPU_GAIN_E_ENTRIES + 1];  /* 641 used (PQ) */
} heifgpu_gain_transform;
/* host only, always HEIFGPU_OK for a parsed image */
int heifgpu_image_get_gain(const heifgpu_image *img, heifgpu_gain_info *out);
/* host only: the transform of `base` with its gain map `gain` (the parsed gain-map image:
 * it gives Bg) to dst at depth bits (the base's, 8..12).  headroom: the Apple rule's, ignored
 * by the ISO rule; display_headroom: a linear ratio, <= 0 for full; sdr_white in cd/m2, <= 0
 * for 203 (PQ only); pq_bits 10, 12 or 16 (PQ only). */
int heifgpu_gain_transform_make(const heifgpu_image *base, const heifgpu_image *gain, uint32_t dst, uint32_t bits,
                                uint32_t encoding, uint32_t pq_bits, double headroom, double display_headroom,
                                double sdr_white, heifgpu_gain_transform *out);
/* host only: the per-pixel formula over n R G B triples of codes 0..maxv with their Q8 gain
 * codes g_q8 (0 .. 256 maxg), binary16 bits or PQ codes out; a larger code, or a transform a
 * render would refuse, is HEIFGPU_E_INVALID.  out may be rgb_in. */
int heifgpu_gain_apply(const heifgpu_gain_transform *t, const uint16_t *rgb_in, const uint32_t *g_q8, size_t n,
                       uint16_t *out);
/* host only: the Q8 gain code of every decoded base position of a W x H base from a Wg x Hg
 * map of depth gain_bits (uint8 for 8, else uint16; pitch bytes a row), W * H uint32 out. */
int heifgpu_gain_sample(const void *gain, uint32_t wg, uint32_t hg, int32_t pitch, uint32_t gain_bits, uint32_t w,
                        uint32_t h, uint32_t *g_q8);
/* heifgpu_render_batch for HDR: base pictures in[i] of imgs[i] and the decoded luma planes
 * gain_in[i] of their gain-map images gain_imgs[i], through the base's display map, as
 * format HEIFGPU_PIX_HDR_* with ONE launch.  xf[i] is never NULL.  Alpha as in
 * heifgpu_render_batch (the RGBA formats; its samples may be of another width than the
 * base's).  The base images' samples must all be 1 byte or all 2 bytes wide; a gain plane may
 * be of either width beside any base.  All checks run before anything is launched.
 * The map is sampled at decoded base positions, so its own display map must say the same as
 * the base's or nothing.  HEIFGPU_E_UNSUPPORTED: a gain image whose own display map is neither
 * the identity nor the base's (the base's exactly, or the base's m over the whole of the map's
 * own picture: the same irot / imir at the map's size, as Apple's files carry them), an image
 * set to bilinear chroma upsampling, a side above 65535.  HEIFGPU_E_INVALID:
 * xf[i] NULL, bits or gain_bits that disagree with the images, an encoding or pq_bits that
 * disagree with the format, a T or E entry above 2^24, an offset above 16 * 65535, a pitch
 * too small.  A window-decoded image is not known to this layer: the caller must have decoded
 * both images whole (DecodeContext.render_hdr refuses otherwise).  The tables live in the
 * context's content cache, as those of the colour-managed render do. */
int heifgpu_render_batch_gain(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                              const heifgpu_planes *in,
                              const heifgpu_image *const *gain_imgs, const heifgpu_planes *gain_in,
                              const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in,
                              uint32_t format, const heifgpu_gain_transform *const *xf,
                              const heifgpu_surface *out, void *stream);
/* THE SCALED CALL (added within ABI 6: new entry points only; no table or transform struct
 * changes, a heifgpu_gain_transform made for heifgpu_render_batch_gain serves it).
 * heifgpu_render_batch_gain onto another grid, with ONE launch and without the full-size HDR
 * surface: scales[i] names a window (x, y, width, height) of base i's displayed picture and the
 * rendered size out_width x out_height by heifgpu_render_batch_scaled's rules (0 sizes: the
 * whole picture; the window non-empty and inside the picture; every side at most 65535), and
 * out[i] is out_width x out_height pixels.  With wx, wy the weights of the scaled render and
 *   avg(v) = floor((2 sum_j sum_i wy(Y, j) wx(X, i) v[y + j][x + i] + cw ch) / (2 cw ch))
 * over the displayed positions of the window, output pixel (X, Y) is made of three rounded
 * area averages, "alpha like a colour":
 *   C_c = avg(c_c), c_c the base's integers at depth B as above: what
 *         heifgpu_render_batch_scaled writes without a transform at the 16-bit formats;
 *   Gq  = avg(g), g the Q8 gain code of the position's decoded base position (sx, sy),
 *         exactly as above (aligned centres, the + 128 >> 8 rounding per source pixel);
 *   A   = avg(a), a the alpha sample at its own depth Ba (the RGBA formats with an alpha image).
 * Then, per output pixel only, the formula above on (L_c = in_lut[c][C_c], Gq): i = Gq >> 8,
 * f = Gq & 255 and M from T, the apply with k_b and k_a, the matrix, the encoding; alpha is
 * encoded from A by the alpha rules of the two encodings.  Nothing of this is computed in
 * floating point beyond what the formula above already is.  (The rounded averages are
 * transformed, not the source pixels: the rule of every scaled render here, and what a viewer
 * does that scales base and map as images and applies the map afterwards.  It is not an
 * average of the HDR levels in linear light.)  With out_width x out_height the window's own
 * size every avg is the value itself: the result is bit for bit that window of what
 * heifgpu_render_batch_gain writes.  RANGES: the weights of an output line add up to the
 * window's side, so a line's column sum of g reaches 65535 * 256 * 4095 > 2^35, the whole sum
 * 2^52 and the numerator 2^53: g is summed as its parts g >> 8 and g & 255, each within the
 * sums of a 12-bit sample, and the quotient taken in two exact steps (kernels/gain_scale.hpp,
 * the one statement of it in code; tests/gain_scale_ref.py restates the call in numpy).
 * Refusals: those of heifgpu_render_batch_gain with their codes, then those of
 * heifgpu_render_batch_scaled for scales[i] (HEIFGPU_E_INVALID: a rendered size outside
 * 1..65535, a window empty or outside the picture; HEIFGPU_E_UNSUPPORTED: a window side above
 * 65535), all before anything is launched.  A window-decoded image is not known to this layer
 * either (DecodeContext.render_hdr_scaled refuses it). */
int heifgpu_render_batch_gain_scaled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                     const heifgpu_planes *in,
                                     const heifgpu_image *const *gain_imgs, const heifgpu_planes *gain_in,
                                     const heifgpu_image *const *alpha_imgs, const heifgpu_planes *alpha_in,
                                     uint32_t format, const heifgpu_scale *scales,
                                     const heifgpu_gain_transform *const *xf,
                                     const heifgpu_surface *out, void *stream);
/* host only: avg(g) of the scaled call over a w x h array of Q8 gain codes in displayed
 * orientation (each at most 256 * 4095, rows of w entries), for the window and rendered size of
 * `scale` (by the rules above, the picture being w x h); out_width * out_height uint32 out.
 * Runs the kernel's own accumulation and quotient. */
int heifgpu_gain_average(const uint32_t *g_q8, uint32_t w, uint32_t h, const heifgpu_scale *scale, uint32_t *out);

/* ---- JPEG output: RGB8 surfaces to baseline JPEG files on the device --------
 * (added within ABI 6: new entry points only.)
 * The input is what the renders write for HEIFGPU_PIX_RGB8 (R, G, B interleaved, a pitch in
 * bytes, any alignment), so every render option composes with it.  The file is baseline
 * sequential JPEG (SOF0), JFIF, Y Cb Cr (BT.601 full range) at 4:4:4 or 4:2:0, the Annex K
 * tables scaled by `quality` as IJG and Pillow scale them, the Huffman tables of K.3, and a
 * restart marker every `restart_mcus` MCUs (0: every MCU row; at most 65535).  Its bytes are
 * fully determined by the pixels and the options: heif_amd/csrc/kernels/jpeg.hpp states the
 * arithmetic, heifgpu_jpeg_encode_host restates the whole encoder on the host.
 * A file is heifgpu_jpeg_header's bytes followed by what heifgpu_jpeg_encode_batch writes (the
 * scan and EOI).  quality outside 1..100, a zero side, a side above 65535, a pitch below
 * 3 * width, a profile above 255 * 65519 bytes or n above 65535 is HEIFGPU_E_INVALID, reported
 * before anything is launched or written. */
#define HEIFGPU_JPEG_444 0u
#define HEIFGPU_JPEG_420 1u
typedef struct {
    uint32_t quality;      /* 1..100 */
    uint32_t subsampling;  /* HEIFGPU_JPEG_444 or HEIFGPU_JPEG_420 */
    uint32_t restart_mcus; /* MCUs per restart interval; 0: one MCU row */
    uint32_t reserved;     /* 0 */
} heifgpu_jpeg_opts;
/* host only: the two quantisation tables of `quality` in natural (row-major) order */
int heifgpu_jpeg_quant_tables(uint32_t quality, uint8_t luma[64], uint8_t chroma[64]);
/* host only: the bytes before the scan (SOI, APP0, APP2 with the ICC profile in chunks when
 * icc_len > 0, DQT, SOF0, DHT, DRI, SOS) of a width x height picture.  *len receives their
 * length; they are written when buf is not NULL and cap >= *len. */
int heifgpu_jpeg_header(uint32_t width, uint32_t height, const heifgpu_jpeg_opts *opts, const uint8_t *icc,
                        size_t icc_len, uint8_t *buf, size_t cap, size_t *len);
/* host only: the whole file of one picture in host memory, by the kernels' own arithmetic;
 * *len and buf as above. */
int heifgpu_jpeg_encode_host(const uint8_t *rgb, int32_t pitch, uint32_t width, uint32_t height,
                             const heifgpu_jpeg_opts *opts, const uint8_t *icc, size_t icc_len, uint8_t *buf,
                             size_t cap, size_t *len);
/* Asynchronous on `stream`: the scan and EOI of n pictures (sizes may differ; one set of options)
 * in a fixed number of launches.  out[i].pixels receives picture i's bytes, out[i].pitch is its
 * capacity in bytes.  sizes (n entries, device memory or pinned host memory the device can
 * write) receives the exact length of every picture's scan and EOI; when that exceeds the
 * capacity, bit 63 of sizes[i] is set as well, nothing at or past the capacity is written and
 * what was written is to be discarded: the caller encodes that picture again with room for
 * the stated length.  The call's scratch belongs to the context: a call waits on the host for
 * the context's previous encode call to finish. */
int heifgpu_jpeg_encode_batch(heifgpu_ctx *ctx, size_t n, const heifgpu_surface *rgb, const uint32_t *width,
                              const uint32_t *height, const heifgpu_jpeg_opts *opts, const heifgpu_surface *out,
                              uint64_t *sizes, void *stream);

/* ---- PNG output: RGB(A) 8- and 16-bit surfaces to PNG files on the device ----
 * (added within ABI 6: new entry points only.)
 * The input is what the renders write for HEIFGPU_PIX_RGB8, RGBA8, RGB16 and RGBA16 (a pitch in
 * bytes, any alignment), so every render option composes with it, alpha and more than 8 bits
 * included, and the file holds exactly the pixels it was given.  The file is a non-interlaced
 * PNG of colour type 2 or 6 and bit depth 8 or 16.  A 16-bit surface holds samples of `bits`
 * significant bits (the image's depth); sample s is stored as (s << (16 - bits)) | (s >> (2 bits
 * - 16)) with an sBIT chunk of `bits`, so a reader recovers s = v >> (16 - bits).  Rows are
 * filtered by one of the five PNG filter types (`filter` 0..4) or, with HEIFGPU_PNG_FILTER_ADAPTIVE,
 * by the type with the least sum of magnitudes per row.  The filtered bytes are deflated in
 * independent blocks of 32768 bytes, each a dynamic-Huffman block of literals only (no matches:
 * long flat regions cost a bit per byte) in an IDAT chunk of its own.  The bytes of a file are
 * fully determined by the pixels and the options: heif_amd/csrc/kernels/png.hpp states every
 * rule, heifgpu_png_encode_host restates the whole encoder on the host.
 * A file is heifgpu_png_header's bytes followed by what heifgpu_png_encode_batch writes (the
 * IDAT chunks and IEND).  A format that is not one of the four, bits outside 8..16 (or not 8 for
 * an 8-bit format), a filter above 5, a nonzero reserved, a zero side, a side above 65535, a
 * pitch below width * bytes per pixel, a profile of 0 or more than 0x7fff0000 bytes or n above
 * 65535 is HEIFGPU_E_INVALID, reported before anything is launched or written. */
#define HEIFGPU_PNG_FILTER_ADAPTIVE 5u
typedef struct {
    uint32_t format;   /* HEIFGPU_PIX_RGB8, RGBA8, RGB16 or RGBA16 */
    uint32_t bits;     /* significant bits of a 16-bit format's samples, 8..16; 8 for an 8-bit format */
    uint32_t filter;   /* 0 none, 1 sub, 2 up, 3 average, 4 Paeth, 5 adaptive */
    uint32_t reserved; /* 0 */
} heifgpu_png_opts;
#define HEIFGPU_PNG_COLOUR_NONE 0u
#define HEIFGPU_PNG_COLOUR_SRGB 1u /* an sRGB chunk, perceptual intent */
#define HEIFGPU_PNG_COLOUR_CICP 2u /* a cICP chunk of the four bytes of `cicp` */
#define HEIFGPU_PNG_COLOUR_ICC 3u  /* an iCCP chunk of the profile at `icc` */
typedef struct {
    uint32_t kind;
    uint8_t cicp[4]; /* colour primaries, transfer function, matrix coefficients (0 for RGB), full-range flag */
    const uint8_t *icc;
    size_t icc_len;
} heifgpu_png_colour;
/* host only: the bytes before the first IDAT (signature, IHDR, sBIT for a 16-bit format of fewer
 * than 16 bits, and the chunk `colour` selects; NULL selects none) of a width x height picture.
 * The profile is deflated in stored blocks.  *len receives their length; they are written when
 * buf is not NULL and cap >= *len. */
int heifgpu_png_header(uint32_t width, uint32_t height, const heifgpu_png_opts *opts, const heifgpu_png_colour *colour,
                       uint8_t *buf, size_t cap, size_t *len);
/* host only: the whole file of one picture in host memory, by the kernels' own rules;
 * *len and buf as above. */
int heifgpu_png_encode_host(const void *pixels, int32_t pitch, uint32_t width, uint32_t height,
                            const heifgpu_png_opts *opts, const heifgpu_png_colour *colour, uint8_t *buf, size_t cap,
                            size_t *len);
/* Asynchronous on `stream`: the IDAT chunks and IEND of n pictures (sizes may differ; one set of
 * options, so one format) in a fixed number of launches.  out[i].pixels receives picture i's
 * bytes, out[i].pitch is its capacity in bytes.  sizes (n entries, device memory or pinned host
 * memory the device can write) receives the exact length of every picture's IDAT chunks and
 * IEND; when that exceeds the capacity, bit 63 of sizes[i] is set as well, nothing at or past the
 * capacity is written and what was written is to be discarded: the caller encodes that picture
 * again with room for the stated length.  The call's scratch belongs to the context: a call
 * waits on the host for the context's previous encode call to finish. */
int heifgpu_png_encode_batch(heifgpu_ctx *ctx, size_t n, const heifgpu_surface *surfaces, const uint32_t *width,
                             const uint32_t *height, const heifgpu_png_opts *opts, const heifgpu_surface *out,
                             uint64_t *sizes, void *stream);

/* ---- window decode: decode only the pictures a window reads ----------------
 * (added within ABI 6: new entry points only; heifgpu_batch_opts keeps its layout.)
 * A render of a window of the displayed picture (heifgpu_scale's x, y, width,
 * height) reads a rectangle of the decoded planes, the SOURCE RECTANGLE:
 *   - the window is taken by heifgpu_scale's rules (0, 0 sizes: the whole
 *     displayed picture; otherwise non-empty and inside out_width x out_height,
 *     else HEIFGPU_E_INVALID);
 *   - its two opposite corners go through the display map (m, t of
 *     heifgpu_display_info); their bounding box is the box of the whole window,
 *     m being a signed permutation;
 *   - the box is grown to the chroma sample grid (x0 down and x1 up to multiples
 *     of SubWidthC, y likewise with SubHeightC; 4:0:0 and 4:4:4 grow nothing).
 *     For an image that replicates chroma (the default) that is all: a luma sample
 *     reads the chroma sample of its cell.  For an image set to bilinear chroma
 *     upsampling ("chroma upsampling" below) a luma column x reads the chroma
 *     columns floor((2x - px) / 4) and the next one, so the box then also covers the
 *     cells of chroma columns floor((2*x0 - px) / 4) to floor((2*(x1 - 1) - px) / 4) + 1
 *     ([x0, x1) the luma box), clamped to the plane and scaled back by SubWidthC; rows
 *     likewise with py and SubHeightC (4:2:2 has no vertical filter and grows no rows);
 *   - and clipped to width x height (heifgpu_image_info).
 * That is exactly the set of decoded samples heifgpu_render_batch (whole
 * picture), heifgpu_render_batch_scaled and heifgpu_render_batch_tensor read for
 * that window (a flip reads the same samples).
 * SELECTION, one rule at every level: a picture of the batch is decoded iff its
 * visible rectangle in the output planes (its placement clipped to the image)
 * intersects the source rectangle.  "Picture" is a grid tile and, inside a coded
 * picture, each independent sub-picture the decode splits it into: an HEVC tile
 * or a row band of a slice with no loop filter across the boundaries.  Pictures
 * filtered across their boundaries (the children of an assembly) are taken all
 * or none: if any sample of the coded picture is needed it is decoded whole.  A
 * skipped picture costs no upload, no parse and no reconstruction.
 * heifgpu_batch_prepare_rects is heifgpu_batch_prepare_ex with one rectangle per
 * image, src[i], in DECODED-PLANE coordinates (not displayed ones): what
 * heifgpu_window_source_rect returns.  An alpha or other auxiliary image is
 * given its colour image's source rectangle (the render addresses it through
 * the colour image's map) and selects by its own tile grid.  src == NULL, or
 * src[i] with width == 0 && height == 0, decodes everything as
 * heifgpu_batch_prepare_ex does (which is this call with src == NULL).  A
 * rectangle that is empty otherwise or not inside width x height is
 * HEIFGPU_E_INVALID, reported before anything is uploaded or launched; a batch
 * being reloaded then keeps its contents and stays decodable.  The selection
 * combines with tile_stride / tile_offset: a grid tile must pass both.  After a
 * decode every sample of src[i] has been written; samples outside it may or may
 * not have been (whole pictures are written), nothing outside the caller's
 * planes is touched.  Status words, heifgpu_batch_status_previous, the parse
 * mode chosen by picture count, heifgpu_batch_parse_geometry and
 * heifgpu_batch_lanes_variant all speak of the pictures selected. */
typedef struct { uint32_t x, y, width, height; } heifgpu_rect;  /* width == 0 && height == 0: everything */
/* host only: the source rectangle of `window` (NULL: the whole displayed picture),
 * for the image's chroma upsampling as it is set at the time of the call */
int heifgpu_window_source_rect(const heifgpu_image *img, const heifgpu_rect *window, heifgpu_rect *src);
/* host only: the grid tiles a source rectangle selects (src NULL: everything):
 * columns [col0, col0 + cols), rows [row0, row0 + rows); cols * rows tiles.  Any
 * of the four pointers may be NULL.  1 x 1 for a single coded item. */
int heifgpu_image_tiles_for_rect(const heifgpu_image *img, const heifgpu_rect *src,
                                 uint32_t *col0, uint32_t *row0, uint32_t *cols, uint32_t *rows);
int heifgpu_batch_prepare_rects(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                const heifgpu_batch_opts *opts, const heifgpu_rect *src,
                                heifgpu_batch **inout);
/* host only, no device: the number of pictures heifgpu_batch_prepare_rects would
 * make of these arguments (sub-pictures and assemblies counted as the decode
 * counts them), so a loader can size a batch of crops before it prepares it. */
int heifgpu_batch_count_pictures(const heifgpu_image *const *imgs, size_t n, const heifgpu_batch_opts *opts,
                                 const heifgpu_rect *src, uint32_t *pictures);
/* the pictures of a prepared batch */
int heifgpu_batch_picture_count(const heifgpu_batch *batch, uint32_t *pictures);

/* ---- filtered render: Pillow-exact bilinear and bicubic ---------------------
 * (added within ABI 6: new entry points only.)
 * The scaled and tensor renders above resample by the area average, a box
 * filter.  The calls below resample the same window of the same D (what
 * heifgpu_render_batch writes) by Pillow's antialiased BILINEAR or BICUBIC
 * instead: for the 8-bit formats every channel c of the result equals
 *     PIL.Image.fromarray(D[..., c]).resize((ow, oh), BILINEAR | BICUBIC,
 *                                           box=(cx, cy, cx + cw, cy + ch))
 * bit for bit.  Per axis, Pillow's precompute_coeffs in IEEE binary64, in exactly
 * this order of operations, with in_size D's side, [in0, in1 = in0 + c) the
 * window, out the rendered side and S the filter's support (1 bilinear, 2 bicubic):
 *     scale = (in1 - in0) / out;  fs = max(scale, 1.0);  support = S * fs;  ss = 1.0 / fs
 *     for X in [0, out):
 *       center = in0 + (X + 0.5) * scale
 *       xmin = (int)(center - support + 0.5);  if xmin < 0: xmin = 0         (C truncation)
 *       xmax = (int)(center + support + 0.5);  if xmax > in_size: xmax = in_size
 *       w[t] = f((t + xmin - center + 0.5) * ss),  t in [0, xmax - xmin)
 *       ww = w[0] + w[1] + ...                                              (left to right)
 *       if ww != 0: w[t] = w[t] / ww                       (a division, not a reciprocal)
 *       k[t] = (int)(w[t] * (1 << P) + (w[t] < 0 ? -0.5 : 0.5))
 *     bilinear f(x): x = |x|;  x < 1 ? 1 - x : 0
 *     bicubic  f(x): x = |x|, a = -0.5;  x < 1 ? ((a+2)*x - (a+3))*x*x + 1
 *                                      : x < 2 ? (((x-5)*x + 8)*x - 4)*a : 0
 * No product and sum of these is fused.  Taps reach beyond the window into D,
 * as Pillow's box does, and stop at D's edges.  Two passes, horizontal first,
 * which means along D's x whatever the irot:
 *     T[y][X] = clip((2^(P-1) + sum_t k[t] * D[y][xmin + t]) >> P, 0, maxv)
 * then the same rule along y over T (>> is an arithmetic shift, sums are int32).
 * The rounding and the clip between the passes are part of the result.
 * P = 32 - 2 - max(8, B), B the depth the format computes at: 22 at 8 bits
 * (Pillow's PRECISION_BITS), 20 at 10, 18 at 12.  The 16-bit formats follow the
 * same rule at their P; Pillow has no such mode, so they are pinned to
 * tests/resample_ref.py only.  Alpha is a channel like the others, nothing is
 * premultiplied (Image.resize on an RGBA image premultiplies; the per-channel
 * statement above does not).  A colour transform acts on the rounded result, as
 * for the area average; the tensor epilogue is unchanged.  A tensor's flip acts
 * on the result R at the store: the coefficients are those of D's coordinates,
 * never of mirrored ones.  Identity (ow == cw, oh == ch) gives the window of D
 * byte for byte.  kernels/resample.hpp is the one statement of this in code,
 * shared by the kernel and the two host hooks below.
 * `filter` is one value per call.  HEIFGPU_FILTER_AREA forwards to the calls
 * above (xf NULL or not) and gives their bytes; an unknown filter is
 * HEIFGPU_E_INVALID, reported like every check before ctx is looked at.  xf may
 * be NULL.  Everything else (checks, mixed batches, ONE launch, the descriptor
 * ring) is as in heifgpu_render_batch_scaled / _tensor; a displayed side above
 * 65535 is HEIFGPU_E_UNSUPPORTED.  Ratios of any size work: the kernel walks
 * footprints in chunks and is tuned for the reductions a loader asks for. */
enum { HEIFGPU_FILTER_AREA = 0, HEIFGPU_FILTER_BILINEAR = 1, HEIFGPU_FILTER_BICUBIC = 2 };
int heifgpu_render_batch_resampled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                   const heifgpu_planes *in,
                                   const heifgpu_image *const *alpha_imgs,
                                   const heifgpu_planes *alpha_in,
                                   uint32_t format, const heifgpu_scale *scale, uint32_t filter,
                                   const heifgpu_color_transform *const *xf /* may be NULL */,
                                   const heifgpu_surface *out, void *stream);
int heifgpu_render_batch_tensor_resampled(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                          const heifgpu_planes *in,
                                          const heifgpu_image *const *alpha_imgs,
                                          const heifgpu_planes *alpha_in,
                                          const heifgpu_tensor_format *fmt, const heifgpu_scale *scale,
                                          uint32_t filter, const uint32_t *flip,
                                          const heifgpu_color_transform *const *xf /* may be NULL */,
                                          const heifgpu_tensor_surface *out, void *stream);
/* host only: one axis's coefficients at P = 32 - 2 - max(8, bits).  *ksize is
 * Pillow's row length, (int)ceil(support) * 2 + 1, always set when the sizes are
 * valid; bounds (2 * out_size: xmin, xmax - xmin per output) and kk (out_size
 * rows of ksize, padded with zeros; cap = the entries kk holds) are filled when
 * not NULL.  in_size and out_size 1..65535, 0 <= in0 < in1 <= in_size, filter
 * BILINEAR or BICUBIC, bits 8..12, cap >= out_size * ksize: else HEIFGPU_E_INVALID. */
int heifgpu_resample_coeffs(uint32_t in_size, uint32_t in0, uint32_t in1, uint32_t out_size, uint32_t filter,
                            uint32_t bits, int32_t *bounds, int32_t *kk, size_t cap, uint32_t *ksize);
/* host only: the two passes over in, in_height x in_width x channels (1..4)
 * interleaved samples without padding, uint8 for bits == 8 and uint16 for bits
 * 9..12 (a code above maxv is HEIFGPU_E_INVALID), window NULL or 0, 0 sized: the
 * whole of it; out receives out_height x out_width x channels in the same layout. */
int heifgpu_resample_apply(const void *in, uint32_t in_width, uint32_t in_height, uint32_t channels, uint32_t bits,
                           const heifgpu_rect *window, uint32_t out_width, uint32_t out_height, uint32_t filter,
                           void *out);
/* host only: heifgpu_window_source_rect for a filtered render, the taps' halo
 * included: per axis the window becomes [xmin(0), xmax(out - 1)) of the formula
 * above, in D; that rectangle then goes through the display map, is grown to the
 * chroma grid and clipped as heifgpu_window_source_rect does.  HEIFGPU_FILTER_AREA
 * gives heifgpu_window_source_rect of the scale's window. */
int heifgpu_window_source_rect_resampled(const heifgpu_image *img, const heifgpu_scale *scale, uint32_t filter,
                                         heifgpu_rect *src);

/* ---- Linear-light scaled render: the area average taken in linear light ------
 * (added within ABI 6: new entry points only; no struct changes.)
 * The scaled and tensor renders above average the encoded (gamma-coded) R'G'B'
 * integers, and their _color forms transform the rounded average.  Fine bright
 * detail on dark ground then comes out too dark: a pixel-pitch black / white
 * pattern averages to code 128 where a display shows the light of code 188.  The
 * calls below take the same area average over LINEAR levels instead: decode to
 * linear before the sum, encode after the quotient.  Opt-in; every other call is
 * what it was, byte for byte.
 * Per image, with
 *   t          a heifgpu_color_transform made for the depth B the render computes at,
 *   (c_0, c_1, c_2, A)  the integers the unmanaged render gives for a source pixel
 *              of the window (clap / irot / imir folded in, bilinear chroma when the
 *              image is set to it),
 *   wy, wx, cw, ch      the weights and window sides of "scaled render" above:
 *     L_c(j,i) = t.in_lut[c][c_c(j,i)]                               c = 0,1,2   (u16)
 *     S_c(Y,X) = sum_j sum_i wy(Y,j) * wx(X,i) * L_c(j,i)
 *     Lm_c     = floor((2*S_c + cw*ch) / (2*cw*ch))                  (round half up; 0..65535)
 *     L'_k     = clamp((m[3k]*Lm_0 + m[3k+1]*Lm_1 + m[3k+2]*Lm_2 + 8192) >> 14, 0, 65535)
 *     out_k    = the out_lut interpolation of L'_k, exactly as in "colour-managed render"
 *     alpha    = the scaled render's average of A, unchanged (straight alpha, codes;
 *                nothing is premultiplied)
 * Ranges: a level and a window side are at most 65535, so the weighted sum down one
 * output line's rows of a column is at most 65535 * 65535 < 2^32, S_c < 2^48 and
 * 2*S_c + cw*ch < 2^50: 64-bit integers hold everything, and a double-precision
 * estimate of the quotient corrected in integers is exact.
 * Consequences: with out = the window's own size S_c = cw*ch*L_c, so Lm_c = L_c and
 * the result is bit for bit the window of heifgpu_render_batch_color with the same
 * transform, which for an identity transform is the window of heifgpu_render_batch
 * (identity includes "every code maps to itself"); a uniform window gives the
 * per-pixel managed result at any size.
 * An identity transform is APPLIED here, not skipped: its tables are what makes the
 * average linear.  Refusals, all before anything is launched and before ctx is
 * looked at: xf NULL, an xf[i] NULL, or xf[i]->bits not the depth image i is
 * rendered at: HEIFGPU_E_INVALID; a transform with tone != 0 (PQ / HLG sources):
 * HEIFGPU_E_UNSUPPORTED; then everything the _color siblings refuse.  Everything
 * else is theirs too: the arguments, ONE launch and one descriptor copy whatever
 * the mix of sources, orientations and chroma modes, the descriptor ring, the table
 * cache.  Not done: the filtered (bilinear / bicubic) renders, premultiplied alpha,
 * tone transforms and the gain-map renders in linear light.
 * numpy restates this (tests/linear_ref.py); kernels/color_xform.hpp holds the
 * per-sample and the level-to-code step, shared by the kernel and
 * heifgpu_linear_average_apply. */
int heifgpu_render_batch_scaled_linear(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                       const heifgpu_planes *in,
                                       const heifgpu_image *const *alpha_imgs,
                                       const heifgpu_planes *alpha_in,
                                       uint32_t format, const heifgpu_scale *scale,
                                       const heifgpu_color_transform *const *xf,
                                       const heifgpu_surface *out, void *stream);
int heifgpu_render_batch_tensor_linear(heifgpu_ctx *ctx, const heifgpu_image *const *imgs, size_t n,
                                       const heifgpu_planes *in,
                                       const heifgpu_image *const *alpha_imgs,
                                       const heifgpu_planes *alpha_in,
                                       const heifgpu_tensor_format *fmt, const heifgpu_scale *scale,
                                       const uint32_t *flip,
                                       const heifgpu_color_transform *const *xf,
                                       const heifgpu_tensor_surface *out, void *stream);
/* host only: the contract above over rgb_in, in_height x in_width x channels (3 or
 * 4; the fourth is averaged as codes) interleaved uint16 codes 0..maxv without
 * padding (a larger code is HEIFGPU_E_INVALID), window NULL or 0, 0 sized: the whole
 * of it; rgb_out (not rgb_in) receives out_height x out_width x channels.  Sides as
 * in heifgpu_render_batch_scaled; a tone transform is HEIFGPU_E_UNSUPPORTED. */
int heifgpu_linear_average_apply(const heifgpu_color_transform *t, const uint16_t *rgb_in, uint32_t in_width,
                                 uint32_t in_height, uint32_t channels, const heifgpu_rect *window,
                                 uint32_t out_width, uint32_t out_height, uint16_t *rgb_out);

/* ---- host test hooks (reference unit-test surface) -------------------- */
size_t heifgpu_remove_emulation_prevention(const uint8_t *in, size_t n, uint8_t *out); /* rbsp_reader.rs:11-39 */
int heifgpu_read_ue(const uint8_t *buf, size_t n, uint32_t *val);                      /* rbsp_reader.rs:87-99 */
int heifgpu_read_se(const uint8_t *buf, size_t n, int32_t *val);                       /* rbsp_reader.rs:101-113 */
/* the kernels' binarizations (cabac/decoder.rs:152-261) over explicit bins;
 * return the value (or -1 on underrun), *used = bins consumed */
int heifgpu_bins_truncated_rice(const uint8_t *bins, int n, int c_max, int c_rice, int *used);
int heifgpu_bins_chroma_pred_mode(const uint8_t *bins, int n, int *used);
int heifgpu_bins_coeff_abs_level_remaining(const uint8_t *bins, int n, int c_rice, int *used);
int heifgpu_bins_exp_golomb(const uint8_t *bins, int n, int k, int *used);

/* parsed parameter sets + slice header of one tile (grammar.rs:224-572;
 * the values SURVEY Appendix A lists for halfmoonbay) */
typedef struct {
    int32_t nal_unit_type, slice_type, first_slice_segment_in_pic;
    int32_t general_profile_idc, general_level_idc;
    int32_t pic_width, pic_height, chroma_format_idc, bit_depth_luma, bit_depth_chroma;
    int32_t log2_max_poc_lsb, log2_min_cb, log2_ctb, log2_min_tb, log2_max_tb;
    int32_t max_th_depth_inter, max_th_depth_intra;
    int32_t scaling_list_enabled, amp, sao, pcm, num_short_term_ref_pic_sets, long_term_refs;
    int32_t temporal_mvp, strong_intra_smoothing;
    int32_t video_full_range, colour_primaries, transfer_characteristics, matrix_coeffs;
    int32_t init_qp, sign_data_hiding, cabac_init_present, constrained_intra_pred, transform_skip;
    int32_t cu_qp_delta_enabled, diff_cu_qp_delta_depth, cb_qp_offset, cr_qp_offset;
    int32_t slice_chroma_qp_offsets_present, transquant_bypass, tiles_enabled, entropy_coding_sync;
    int32_t loop_filter_across_slices, deblocking_control_present, deblocking_override_enabled;
    int32_t deblocking_disabled, beta_offset_div2, tc_offset_div2, log2_parallel_merge_level;
    int32_t slice_sao_luma, slice_sao_chroma, slice_qp_y, num_entry_point_offsets;
    int32_t slice_data_raw_offset, payload_bytes;
    uint32_t entry_point_offset[64]; /* offset_minus1 + 1 (raw bytes), first 64 */
} heifgpu_tile_params;
int heifgpu_image_tile_params(const heifgpu_image *img, uint32_t tile, heifgpu_tile_params *out);

/* ---- tuning hook ------------------------------------------------------ */
/* k_parse_lanes counters (s_memtime cycles: whole wave, passes, per unit
 * kind CTU / tree / TB / sub-block / CTU end; lanes that ran a unit),
 * summed over waves since the last call, then reset.  Returns the number of
 * counters written, or 0 for the product build (counters compiled out; the
 * `make prof` library has them). */
int heifgpu_debug_counters(uint64_t *out, int n);
/* The CABAC parse geometry a prepared batch launches: mode
 * (HEIFGPU_PARSE_LANES / _SOLO / _SPREAD), workgroups (waves in lanes mode,
 * pictures in solo mode, substreams in spread mode), pictures per wave (lanes)
 * and waves per workgroup (solo). */
int heifgpu_batch_parse_geometry(const heifgpu_batch *batch, uint32_t *mode, uint32_t *workgroups,
                                 uint32_t *pics_per_wave, uint32_t *waves_per_workgroup);
/* The body a prepared batch's lanes parse runs: 1 the lean one, compiled for
 * 4:2:0 pictures without PCM, transform_skip, cu_transquant_bypass, slice
 * segments inside a picture or WPP rows beyond its lanes (chosen when every
 * picture of the batch is such a picture), 0 the general one (also what the
 * other parse modes report).  HEIFGPU_LANES_VARIANT=general, read at every
 * prepare, keeps the general body; auto or unset leaves the choice. */
int heifgpu_batch_lanes_variant(const heifgpu_batch *batch, uint32_t *variant);

#ifdef __cplusplus
}
#endif
#endif
