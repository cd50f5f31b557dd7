"""heif_amd — MI355X-native HEIC (HEVC intra still) decode path.

Host-side mirror of the reference API (friendlymatthew/heif):

* ``HeicDecoder.decode(data)``  ↔ ``heif::HeicDecoder::decode(&[u8])``
  (src/heic/decoder.rs:12) — but returns the decoded planes instead of ``()``.
* ``HeifImage.parse(data)`` / ``.info`` ↔ the host half of that function
  (HeifReader::read, hvcC → VPS/SPS/PPS, grid tiles, slice headers).
* ``RbspReader.remove_emulation_prevention`` / ``read_ue`` / ``read_se``
  ↔ src/hevc/rbsp_reader.rs.

Everything runs through the C ABI in ``include/heifgpu.h`` (libheifgpu.so);
decoding runs in gfx950 HIP kernels.  PyTorch only supplies device memory,
streams and ``torch.distributed``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

from . import _lib
from ._lib import HeifGpuError, UnsupportedError, lib

__all__ = [
    "HeicDecoder", "HeifImage", "DecodeContext", "DeviceBatch", "DecodedImage", "RbspReader",
    "HeifGpuError", "UnsupportedError", "ipc_export", "ipc_open", "ipc_close", "chroma_dims", "ColorDescription", "GainMapDescription",
    "HdrDescription", "ChromaDescription",
]


class RbspReader:
    """rbsp_reader.rs surface used by the reference's unit tests."""

    @staticmethod
    def remove_emulation_prevention(data: bytes) -> bytes:
        src = _lib.u8buf(data)
        dst = (ctypes.c_uint8 * max(len(data), 1))()
        n = lib.heifgpu_remove_emulation_prevention(src, len(data), dst)
        return bytes(dst[:n])

    @staticmethod
    def read_ue(data: bytes) -> int:
        v = ctypes.c_uint32()
        _lib.check(lib.heifgpu_read_ue(_lib.u8buf(data), len(data), ctypes.byref(v)))
        return v.value

    @staticmethod
    def read_se(data: bytes) -> int:
        v = ctypes.c_int32()
        _lib.check(lib.heifgpu_read_se(_lib.u8buf(data), len(data), ctypes.byref(v)))
        return v.value


class HeifImage:
    """A host-parsed HEIC image (container + parameter sets + slice headers)."""

    def __init__(self, handle: int):
        self._h = ctypes.c_void_p(handle)

    @classmethod
    def parse(cls, data: bytes, item_id: int = 0, chroma: Optional[str] = None) -> "HeifImage":
        """The primary image (item_id 0), or any coded image item, e.g. the
        auxiliary HDR gain map at `HeifImage.parse(d).info.aux_item_id`.
        chroma "bilinear" sets chroma_upsampling on the image returned."""
        h = ctypes.c_void_p()
        _lib.check(lib.heifgpu_image_parse_item(_lib.u8buf(data), len(data), item_id, ctypes.byref(h)))
        img = cls(h.value)
        if chroma is not None:
            img.chroma_upsampling = chroma
        return img

    @classmethod
    def parse_many(cls, files: Sequence[bytes], threads: int = 0, chroma: Optional[str] = None) -> List["HeifImage"]:
        """Primary images of many files, parsed on `threads` native host threads
        (heifgpu_image_parse_many; 0 = every hardware thread).  chroma as in parse()."""
        if chroma is not None and chroma not in _lib.CHROMA_MODES:
            raise ValueError(f"chroma {chroma!r}: one of {sorted(_lib.CHROMA_MODES)}")
        n = len(files)
        files = [bytes(f) for f in files]  # no copy for bytes; the library copies what it keeps
        # pointers straight into the bytes objects (no Python-side copy of the files)
        data = (ctypes.POINTER(ctypes.c_uint8) * max(n, 1))(
            *[ctypes.cast(ctypes.c_char_p(f), ctypes.POINTER(ctypes.c_uint8)) for f in files])
        lens = (ctypes.c_size_t * max(n, 1))(*[len(f) for f in files])
        hs = (ctypes.c_void_p * max(n, 1))()
        rc = lib.heifgpu_image_parse_many(data, lens, n, threads, hs, None)
        imgs = [cls(h) if h else None for h in hs[:n]]
        _lib.check(rc)
        if chroma is not None:
            for im in imgs:
                im.chroma_upsampling = chroma
        return imgs

    @property
    def info(self) -> _lib.ImageInfo:
        info = _lib.ImageInfo()
        _lib.check(lib.heifgpu_image_get_info(self._h, ctypes.byref(info)))
        return info

    @property
    def display(self) -> _lib.DisplayInfo:
        """How the image is shown (heifgpu_image_get_display): displayed size,
        the folded clap / irot / imir map, the alpha auxiliary item."""
        d = _lib.DisplayInfo()
        _lib.check(lib.heifgpu_image_get_display(self._h, ctypes.byref(d)))
        return d

    @property
    def color(self) -> "ColorDescription":
        """The image's colour space (heifgpu_image_get_color): what defines it
        ("icc", "nclx" or "none", which is taken as sRGB), the nclx primaries and
        transfer codes, and the source colourants (3 x 3: row c is X Y Z of
        primary c, D50), None when a transform of this source is refused."""
        ci = _lib.ColorInfo()
        _lib.check(lib.heifgpu_image_get_color(self._h, ctypes.byref(ci)))
        col = None
        if ci.status == _lib.HEIFGPU_OK:
            col = tuple(tuple(ci.colorants[3 * c + k] for k in range(3)) for c in range(3))
        return ColorDescription(_lib.COLOR_KINDS[ci.kind], ci.primaries, ci.transfer, col, ci.icc_size, bool(ci.has_nclx),
                                ci.status)

    @property
    def icc_profile(self) -> Optional[bytes]:
        """The bytes of the item's ICC profile (heifgpu_image_get_icc), None without one."""
        n = ctypes.c_size_t()
        _lib.check(lib.heifgpu_image_get_icc(self._h, None, 0, ctypes.byref(n)))
        if not n.value:
            return None
        buf = (ctypes.c_uint8 * n.value)()
        _lib.check(lib.heifgpu_image_get_icc(self._h, buf, n.value, ctypes.byref(n)))
        return bytes(buf)

    @property
    def hdr(self) -> Optional["HdrDescription"]:
        """What an HDR item carries (heifgpu_image_get_hdr): the transfer (16 PQ,
        18 HLG), MaxCLL / MaxFALL of its clli box and the mastering luminances of
        its mdcv box (None without the box), and what a tone transform of it
        answers.  None for an item whose colour is not defined by a PQ / HLG nclx."""
        hi = _lib.HdrInfo()
        _lib.check(lib.heifgpu_image_get_hdr(self._h, ctypes.byref(hi)))
        if not hi.transfer:
            return None
        clli, mdcv = bool(hi.present & _lib.HDR_HAS_CLLI), bool(hi.present & _lib.HDR_HAS_MDCV)
        return HdrDescription(hi.transfer, hi.max_cll if clli else None, hi.max_fall if clli else None,
                              hi.mastering_max * 1e-4 if mdcv else None, hi.mastering_min * 1e-4 if mdcv else None,
                              hi.status)

    @property
    def gain_map(self) -> Optional["GainMapDescription"]:
        """The image's HDR gain map (heifgpu_image_get_gain), None without one: kind
        "iso" (an ISO 21496-1 'tmap' item names this image as its base; the payload's
        fields are reported, log2 values for the headrooms, min and max) or "apple"
        (an auxiliary image with Apple's URN; its headroom is the caller's to give),
        item_id of the gain-map image, and what a transform of it answers (status)."""
        gi = _lib.GainInfo()
        _lib.check(lib.heifgpu_image_get_gain(self._h, ctypes.byref(gi)))
        if gi.kind == _lib.GAIN_NONE:
            return None
        return GainMapDescription(_lib.GAIN_KINDS[gi.kind], gi.gain_item_id, gi.status, gi.version, gi.minimum_version,
                                  gi.writer_version, bool(gi.multichannel), bool(gi.use_base_colour_space),
                                  gi.base_headroom, gi.alternate_headroom, gi.gain_min, gi.gain_max, gi.gamma,
                                  gi.base_offset, gi.alternate_offset)

    def gain_transform(self, gain: "HeifImage", colorspace: str = "display-p3", encoding: str = "linear",
                       pq_bits: int = 10, headroom: Optional[float] = None, display_headroom: Optional[float] = None,
                       sdr_white: float = 203.0):
        """The gain-map HDR transform of this base image with its parsed gain-map image
        `gain` (heifgpu_gain_transform_make) to "srgb", "display-p3" or "bt2020", for the
        "linear" or the "pq" encoding: a _lib.GainTransform.  headroom is the Apple
        rule's (required there); display_headroom None means the full HDR rendition."""
        if colorspace not in _lib.HDR_COLORSPACES:
            raise ValueError(f"colorspace {colorspace!r}: one of {sorted(_lib.HDR_COLORSPACES)}")
        if encoding not in ("linear", "pq"):
            raise ValueError(f"encoding {encoding!r}: 'linear' or 'pq'")
        t = _lib.GainTransform()
        _lib.check(lib.heifgpu_gain_transform_make(
            self._h, gain._h, _lib.HDR_COLORSPACES[colorspace], int(self.info.bit_depth),
            _lib.GAIN_PQ if encoding == "pq" else _lib.GAIN_LINEAR, int(pq_bits),
            0.0 if headroom is None else float(headroom), 0.0 if display_headroom is None else float(display_headroom),
            float(sdr_white), ctypes.byref(t)))
        return t

    def _chroma_info(self) -> _lib.ChromaInfo:
        ci = _lib.ChromaInfo()
        _lib.check(lib.heifgpu_image_get_chroma(self._h, ctypes.byref(ci)))
        return ci

    @property
    def chroma(self) -> "ChromaDescription":
        """Where the stream puts its chroma samples (heifgpu_image_get_chroma): loc,
        the SPS's chroma_sample_loc_type_top_field (0 when not signalled),
        signalled, and subsampling = (SubWidthC, SubHeightC)."""
        ci = self._chroma_info()
        return ChromaDescription(ci.loc, bool(ci.signalled), (ci.sub_width_c, ci.sub_height_c))

    @property
    def chroma_upsampling(self) -> str:
        """How every render of this image turns 4:2:0 / 4:2:2 chroma into the luma
        grid: "replicate" (the default: a luma sample reads the chroma sample of its
        cell) or "bilinear" (interpolated at the sample location in force,
        include/heifgpu.h "chroma upsampling").  4:4:4 and 4:0:0 images accept the
        setting, which changes nothing for them.  source_rect() follows it.  Not to
        be set while another thread submits a render of this image."""
        return "bilinear" if self._chroma_info().mode == _lib.CHROMA_BILINEAR else "replicate"

    @chroma_upsampling.setter
    def chroma_upsampling(self, mode: str) -> None:
        if mode not in _lib.CHROMA_MODES:
            raise ValueError(f"chroma_upsampling {mode!r}: one of {sorted(_lib.CHROMA_MODES)}")
        _lib.check(lib.heifgpu_image_set_chroma_upsampling(self._h, _lib.CHROMA_MODES[mode], self._chroma_info().loc_override))

    @property
    def chroma_loc(self) -> int:
        """The chroma sample location in force for "bilinear" (0..5): the caller's
        override, else the file's.  Set None to return to the file's."""
        ci = self._chroma_info()
        return ci.loc_override if ci.loc_override >= 0 else ci.loc

    @chroma_loc.setter
    def chroma_loc(self, loc: Optional[int]) -> None:
        if loc is not None and (isinstance(loc, bool) or int(loc) != loc or not 0 <= int(loc) <= 5):
            raise ValueError(f"chroma_loc {loc!r}: None or 0..5")
        _lib.check(lib.heifgpu_image_set_chroma_upsampling(self._h, self._chroma_info().mode, -1 if loc is None else int(loc)))

    # a caller's source peak in cd/m2 for the tone transforms of this image (None: the file's);
    # color_transform(peak_nits=) overrides it for one call
    peak_nits: Optional[float] = None

    def color_transform(self, colorspace: str, bits: int = 8, tone_map: Optional[str] = None,
                        peak_nits: Optional[float] = None):
        """The transform of this image's colour space to "srgb" or "display-p3" at
        the depth a render computes at (heifgpu_color_transform_make): 8 for the
        8-bit formats, the image's bit depth for the 16-bit ones.  UnsupportedError
        for a source outside the supported set (LUT profiles, PQ / HLG, ...),
        HeifGpuError for a malformed profile.  tone_map "bt2390" gives an nclx PQ /
        HLG source a transform with a BT.2390 tone stage instead of the refusal (a
        _lib.HdrTransform, heifgpu_color_transform_make_hdr; peak_nits replaces the
        source peak the file states) and every other image the transform it gets
        without.  Cached per (colorspace, bits, tone_map, peak_nits)."""
        if colorspace not in _lib.COLORSPACES:
            raise ValueError(f"colorspace {colorspace!r}: one of {sorted(_lib.COLORSPACES)}")
        if tone_map is not None and tone_map not in _lib.TONE_MAPS:
            raise ValueError(f"tone_map {tone_map!r}: None or one of {sorted(_lib.TONE_MAPS)}")
        if peak_nits is None:
            peak_nits = self.peak_nits
        peak = float(peak_nits) if peak_nits is not None and tone_map is not None else 0.0
        cache = self.__dict__.setdefault("_xf", {})
        key = (colorspace, int(bits)) if tone_map is None else (colorspace, int(bits), tone_map, peak)
        if key not in cache:
            if tone_map is None:
                t = _lib.ColorTransform()
                _lib.check(lib.heifgpu_color_transform_make(self._h, _lib.COLORSPACES[colorspace], int(bits), ctypes.byref(t)))
            else:
                h = _lib.HdrTransform()
                _lib.check(lib.heifgpu_color_transform_make_hdr(self._h, _lib.COLORSPACES[colorspace], int(bits),
                                                                _lib.TONE_MAPS[tone_map], peak, ctypes.byref(h)))
                t = h
                if not h.base.tone:  # not an HDR source: the transform it gets without tone_map, as that type
                    t = _lib.ColorTransform()
                    ctypes.memmove(ctypes.byref(t), ctypes.byref(h.base), ctypes.sizeof(t))
            cache[key] = t
        return cache[key]

    def source_rect(self, window=None, size=None, filter: str = "area"):
        """(x, y, w, h) of the decoded planes that a render of `window` reads
        (heifgpu_window_source_rect): window = (x, y, w, h) in displayed
        coordinates, the tuples render_scaled(windows=) takes; None or
        (0, 0, 0, 0) is the whole displayed picture.  filter "bilinear" or
        "bicubic" with size = (h, w), the rendered size, widens the rectangle by
        the halo the filter's taps reach beyond the window
        (heifgpu_window_source_rect_resampled).  ValueError for a window that is
        empty or not inside the displayed picture."""
        w = _lib.Rect(*(int(v) for v in window)) if window is not None else _lib.Rect()
        src = _lib.Rect()
        f = _filter_code(filter)
        try:
            if f == _lib.FILTER_AREA:
                _lib.check(lib.heifgpu_window_source_rect(self._h, ctypes.byref(w), ctypes.byref(src)))
            else:
                if size is None:
                    raise ValueError(f"source_rect(filter={filter!r}) needs the rendered size")
                sc = _lib.Scale(int(size[1]), int(size[0]), w.x, w.y, w.width, w.height)
                _lib.check(lib.heifgpu_window_source_rect_resampled(self._h, ctypes.byref(sc), f, ctypes.byref(src)))
        except HeifGpuError as e:
            raise ValueError(str(e)) from None
        return src.as_tuple()

    def tiles_for(self, rect=None):
        """(col0, row0, cols, rows): the grid tiles a source rectangle of the
        decoded planes selects (heifgpu_image_tiles_for_rect); None = all of
        them.  ValueError for a rectangle that is empty or outside the image."""
        r = _lib.Rect(*(int(v) for v in rect)) if rect is not None else _lib.Rect()
        v = [ctypes.c_uint32() for _ in range(4)]
        try:
            _lib.check(lib.heifgpu_image_tiles_for_rect(self._h, ctypes.byref(r), *[ctypes.byref(x) for x in v]))
        except HeifGpuError as e:
            raise ValueError(str(e)) from None
        return tuple(x.value for x in v)

    def tile_params(self, tile: int) -> dict:
        """Parsed SPS/PPS/slice-header fields of grid tile `tile` (row-major)."""
        tp = _lib.TileParams()
        _lib.check(lib.heifgpu_image_tile_params(self._h, tile, ctypes.byref(tp)))
        d = {n: getattr(tp, n) for n, _ in tp._fields_ if n != "entry_point_offset"}
        d["entry_point_offset"] = list(tp.entry_point_offset[: min(tp.num_entry_point_offsets, 64)])
        return d

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:  # lib is None during interpreter teardown
            lib.heifgpu_image_free(h)
            self._h = None


@dataclass
class ColorDescription:
    kind: str                   # "icc", "nclx" or "none"
    primaries: int              # of the nclx colr; 2 (unspecified) without one
    transfer: int
    colorants: Optional[tuple]  # ((Xr, Yr, Zr), (Xg, Yg, Zg), (Xb, Yb, Zb)), D50
    icc_size: int = 0
    has_nclx: bool = False
    status: int = 0             # HEIFGPU_OK, or the code a transform of this source answers


@dataclass
class ChromaDescription:
    loc: int               # chroma_sample_loc_type_top_field of the SPS, 0..5 (0 when not signalled)
    signalled: bool        # the SPS's VUI carries chroma_loc_info
    subsampling: tuple     # (SubWidthC, SubHeightC)


@dataclass
class GainMapDescription:
    kind: str                 # "apple" or "iso"
    item_id: int              # the gain-map image item
    status: int               # HEIFGPU_OK, or what a transform answers
    version: int = 0          # the rest: the ISO 21496-1 payload ("iso"; zeros otherwise)
    minimum_version: int = 0
    writer_version: int = 0
    multichannel: bool = False
    use_base_colour_space: bool = False
    base_headroom: float = 0.0
    alternate_headroom: float = 0.0
    gain_min: float = 0.0
    gain_max: float = 0.0
    gamma: float = 0.0
    base_offset: float = 0.0
    alternate_offset: float = 0.0


@dataclass
class HdrDescription:
    transfer: int                      # 16 (PQ) or 18 (HLG)
    max_cll: Optional[int]             # clli, cd/m2; None without the box
    max_fall: Optional[int]
    mastering_max: Optional[float]     # mdcv, cd/m2; None without the box
    mastering_min: Optional[float]
    status: int = 0                    # HEIFGPU_OK, or the code a tone transform of this item answers


def chroma_dims(info):
    """(height, width) of an image's Cb / Cr planes: chroma_format_idc 1 (4:2:0)
    halves both axes, 2 (4:2:2) the width, 3 (4:4:4) neither (Table 6-1), odd
    sizes rounded up."""
    sx = 1 if info.chroma_format_idc in (1, 2) else 0
    sy = 1 if info.chroma_format_idc == 1 else 0
    return (info.height + sy) >> sy, (info.width + sx) >> sx


@dataclass
class DecodedImage:
    y: "object"            # torch tensor on the device, (H, W)
    cb: Optional["object"]  # (ceil(H/2), ceil(W/2)) for 4:2:0
    cr: Optional["object"]
    info: _lib.ImageInfo
    image: Optional["HeifImage"] = None  # the parsed image (its display map; DecodeContext.render)
    # window decode: the (x, y, w, h) of the planes the last decode_async wrote for certain
    # (DeviceBatch.rects); None after a full decode.  The renders refuse to read outside it.
    valid: Optional[tuple] = None


def _inside(need, valid) -> bool:
    return (need[0] >= valid[0] and need[1] >= valid[1] and need[0] + need[2] <= valid[0] + valid[2]
            and need[1] + need[3] <= valid[1] + valid[3])


def _filter_code(filter: str) -> int:
    if filter not in _lib.FILTERS:
        raise ValueError(f"filter {filter!r}: one of {sorted(_lib.FILTERS)}")
    return _lib.FILTERS[filter]


def _check_valid(what: str, i: int, out: "DecodedImage", alpha, window, size=None, filter: str = "area") -> None:
    """ValueError if rendering `window` of out (None: the whole displayed picture)
    would read samples a window decode did not write, of out or of its alpha image
    (for a filtered render to `size`: the window and its taps' halo)."""
    parts = [(n, o) for n, o in (("image", out), ("alpha image", alpha)) if o is not None and o.valid is not None]
    if not parts:
        return
    need = out.image.source_rect(window, size, filter)
    for name, o in parts:
        if not _inside(need, o.valid):
            raise ValueError(f"{what}: {name} {i} was decoded for the rectangle {o.valid} of its planes, "
                             f"this call reads {need}")


class DecodeContext:
    """One heifgpu context per device (not shared across threads)."""

    def __init__(self, device: int = 0):
        import torch

        self.device = device
        self._torch = torch
        h = ctypes.c_void_p()
        _lib.check(lib.heifgpu_create(device, ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h is not None and self._h.value:
            lib.heifgpu_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc_outputs_contiguous(self, images: Sequence[HeifImage]):
        """Output planes of `images` carved from ONE device buffer (256-byte
        aligned planes), so a single heifgpu_ipc_export handle covers all of
        them; returns (outputs, buffer)."""
        torch = self._torch
        dev = torch.device("cuda", self.device)
        shapes = []
        total = 0
        for im in images:
            inf = im.info
            dims = [(inf.height, inf.width)]
            if inf.chroma_format_idc:
                dims += [chroma_dims(inf)] * 2
            offs = []
            for h, w in dims:
                offs.append((total, h, w))
                total += (h * w * inf.bytes_per_sample + 255) // 256 * 256
            shapes.append((inf, offs))
        buf = torch.empty(max(total, 256), dtype=torch.uint8, device=dev)
        outs = []
        for inf, offs in shapes:
            dt = torch.uint8 if inf.bytes_per_sample == 1 else torch.int16
            pl = [buf[o:o + h * w * inf.bytes_per_sample].view(dt).view(h, w) for o, h, w in offs]
            outs.append(DecodedImage(pl[0], pl[1] if len(pl) > 1 else None, pl[2] if len(pl) > 1 else None, inf))
        for o, im in zip(outs, images):
            o.image = im
        return outs, buf

    def alloc_outputs(self, images: Sequence[HeifImage]) -> List[DecodedImage]:
        torch = self._torch
        outs = []
        for im in images:
            inf = im.info
            dt = torch.uint8 if inf.bytes_per_sample == 1 else torch.int16
            dev = torch.device("cuda", self.device)
            y = torch.empty((inf.height, inf.width), dtype=dt, device=dev)
            cb = cr = None
            if inf.chroma_format_idc:
                ch, cw = chroma_dims(inf)
                cb = torch.empty((ch, cw), dtype=dt, device=dev)
                cr = torch.empty((ch, cw), dtype=dt, device=dev)
            outs.append(DecodedImage(y, cb, cr, inf, im))
        return outs

    @staticmethod
    def planes_of(outs: Sequence[DecodedImage]):
        arr = (_lib.Planes * len(outs))()
        for i, o in enumerate(outs):
            for c, t in enumerate((o.y, o.cb, o.cr)):
                if t is not None:
                    arr[i].plane[c] = t.data_ptr()
                    arr[i].pitch[c] = t.stride(0) * t.element_size()
        return arr

    def prepare(self, images: Sequence[HeifImage], tile_stride: int = 1, tile_offset: int = 0,
                reuse: Optional["DeviceBatch"] = None, wait: bool = True, parse: str = "auto",
                pics_per_wave: int = 0, pipeline_sets: int = 0, windows=None, rects=None, size=None,
                filter: str = "area") -> "DeviceBatch":
        """Device batch of `images` (heifgpu_batch_prepare_ex).  tile_stride /
        tile_offset select the grid tiles k % tile_stride == tile_offset (the
        single-image tile split across GPUs); `reuse` reloads an existing batch
        in place; wait=False returns before the upload has finished (the next
        decode of the batch waits for it).  parse: "auto" (by batch size),
        "lanes" (one substream per lane, `pics_per_wave` pictures per wave, 0 =
        adaptive), "solo" (one substream per wave, a picture's rows in one
        workgroup) or "spread" (one substream per wave, one workgroup per row:
        small-batch latency).  pipeline_sets: parse-output sets of a new batch
        (0 = default 3; 1-3, include/heifgpu.h).
        Window decode (heifgpu_batch_prepare_rects): windows[i] = (x, y, w, h)
        in displayed coordinates, the tuples render_scaled(windows=) takes, or
        None for the whole image; only the grid tiles (and independent
        sub-pictures) that a render of that window reads are uploaded and
        decoded.  rects[i] = (x, y, w, h) gives the rectangle in decoded-plane
        coordinates instead and wins over windows[i]: an alpha image is
        prepared with its colour image's HeifImage.source_rect(window).  For a
        filtered render (render_scaled / render_tensor with filter "bilinear"
        or "bicubic") pass that filter and size = (h, w), the rendered size:
        the windows' rectangles then include the halo the taps read.  The
        rectangles end up in DeviceBatch.rects and, at decode_async, in
        DecodedImage.valid."""
        n = len(images)
        _filter_code(filter)
        for name, v in (("windows", windows), ("rects", rects)):
            if v is not None and len(v) != n:
                raise ValueError(f"{name} must have one entry per image")
        chosen = [None] * n
        for i, im in enumerate(images):
            if rects is not None and rects[i] is not None:
                chosen[i] = tuple(int(v) for v in rects[i])
            elif windows is not None and windows[i] is not None:
                chosen[i] = im.source_rect(windows[i], size, filter)
            if chosen[i] is not None and chosen[i][2] == 0 and chosen[i][3] == 0:
                chosen[i] = None  # the "everything" form
        src = None
        if any(r is not None for r in chosen):
            src = (_lib.Rect * n)(*[_lib.Rect(*r) if r is not None else _lib.Rect() for r in chosen])
        arr = (ctypes.c_void_p * n)(*[im._h.value for im in images])
        opts = _lib.BatchOpts(tile_stride, tile_offset, _lib.PARSE_MODES[parse], pics_per_wave, pipeline_sets)
        if src is None and not hasattr(lib, "heifgpu_batch_prepare_rects"):  # an earlier build of this ABI
            def load(handle):
                return lib.heifgpu_batch_prepare_ex(self._h, arr, n, ctypes.byref(opts), handle)
        else:
            def load(handle):
                return lib.heifgpu_batch_prepare_rects(self._h, arr, n, ctypes.byref(opts), src, handle)
        if reuse is not None:
            _lib.check(load(ctypes.byref(reuse._h)))
            reuse.images = list(images)
            batch = reuse
        else:
            b = ctypes.c_void_p()
            _lib.check(load(ctypes.byref(b)))
            batch = DeviceBatch(self, b, list(images))
        batch.rects = chosen
        if wait:
            self._torch.cuda.synchronize(self.device)
        return batch

    def gather_tiles(self, dst: DecodedImage, src: DecodedImage, tile_stride: int, tile_offset: int,
                     stream: Optional[int] = None):
        """Copy the tiles k % tile_stride == tile_offset of `src` (decoded with
        those options, on any device) into `dst` on this context's device."""
        if stream is None:
            stream = self._torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(lib.heifgpu_gather_tiles(ctypes.byref(dst.info), DecodeContext.planes_of([dst]),
                                            DecodeContext.planes_of([src]), tile_stride, tile_offset,
                                            ctypes.c_void_p(stream)))

    def gather_tiles_from(self, dst: DecodedImage, src_ptrs: Sequence[int], src_pitches: Sequence[int],
                          tile_stride: int, tile_offset: int, stream: Optional[int] = None):
        """gather_tiles from raw device pointers, e.g. another process's planes
        mapped with ipc_open."""
        if stream is None:
            stream = self._torch.cuda.current_stream(self.device).cuda_stream
        src = (_lib.Planes * 1)()
        for c in range(3):
            src[0].plane[c] = src_ptrs[c] if c < len(src_ptrs) else None
            src[0].pitch[c] = src_pitches[c] if c < len(src_pitches) else 0
        _lib.check(lib.heifgpu_gather_tiles(ctypes.byref(dst.info), DecodeContext.planes_of([dst]), src, tile_stride,
                                            tile_offset, ctypes.c_void_p(stream)))

    def set_timing(self, enable: bool):
        _lib.check(lib.heifgpu_set_timing(self._h, 1 if enable else 0))

    def stage_times(self) -> List[float]:
        """ms of the last timed decode: parse, transform, intra, deblock, sao_out, rbsp."""
        ms = (ctypes.c_float * 6)()
        _lib.check(lib.heifgpu_stage_times(self._h, ms))
        return list(ms)

    def to_rgb(self, img: DecodedImage, stream: Optional[int] = None):
        """Interleaved 8-bit RGB (H', W', 3) with the irot rotation applied
        (heifgpu_ycbcr_to_rgb), as a torch tensor on the device."""
        torch = self._torch
        inf = img.info
        if img.valid is not None and not _inside((0, 0, inf.width, inf.height), img.valid):
            raise ValueError(f"to_rgb reads the whole image, which was decoded for the rectangle {img.valid} only")
        rot = inf.rotation & 3
        ow, oh = (inf.height, inf.width) if rot & 1 else (inf.width, inf.height)
        rgb = torch.empty((oh, ow, 3), dtype=torch.uint8, device=torch.device("cuda", self.device))
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        planes = DecodeContext.planes_of([img])
        _lib.check(lib.heifgpu_ycbcr_to_rgb(self._h, ctypes.byref(inf), planes, ctypes.c_void_p(rgb.data_ptr()),
                                            rgb.stride(0), ctypes.c_void_p(stream)))
        return rgb


    def render(self, outs: Sequence[DecodedImage], fmt: str = "rgb8",
               alphas: Optional[Sequence[Optional[DecodedImage]]] = None, stream: Optional[int] = None,
               colorspace: Optional[str] = None, tone_map: Optional[str] = None):
        """Display-ready pixels of a batch of decoded images with ONE
        heifgpu_render_batch call (one kernel launch): a list of (H', W', C)
        device tensors, C = 3 or 4, uint8 for "rgb8" / "rgba8" and int16 (like
        the 16-bit planes) for "rgb16" / "rgba16", with every image's clap /
        irot / imir applied.  alphas[i] is the decoded alpha image of outs[i]
        (None = opaque).  The images come from alloc_outputs (they carry their
        parsed HeifImage).  colorspace None leaves every picture in its own colour
        space (the colr matrix and range applied, nothing else); "srgb" or
        "display-p3" converts every RGB triple from the image's ICC profile or
        nclx description to that space in the same launch (heifgpu_render_batch_color;
        alpha untouched); a source the library cannot transform raises
        UnsupportedError before anything is launched.  tone_map "bt2390", with a
        colorspace, tone-maps the nclx PQ / HLG pictures of the batch to SDR in the
        same launch (BT.2390 on luminance, include/heifgpu.h "HDR render") instead
        of refusing them; every other picture gets the transform it gets without."""
        self._check_tone(colorspace, tone_map)
        torch = self._torch
        f = _lib.PIX_FORMATS[fmt]
        ch, wide = (4 if f & 1 else 3), f >= _lib.PIX_RGB16
        self._check_images("render", outs, alphas)
        for i, o in enumerate(outs):
            _check_valid("render", i, o, alphas[i] if alphas is not None else None, None)
        dev = torch.device("cuda", self.device)
        res = [torch.empty((o.image.display.out_height, o.image.display.out_width, ch),
                           dtype=torch.int16 if wide else torch.uint8, device=dev) for o in outs]
        self._submit("heifgpu_render_batch", outs, alphas, colorspace, wide, stream, (f,), self._surfaces(res), tone_map)
        return res

    def render_hdr(self, outs: Sequence[DecodedImage], gains: Sequence[DecodedImage], fmt: str = "rgba16f",
                   colorspace: str = "display-p3", headroom: Optional[float] = None,
                   display_headroom: Optional[float] = None, sdr_white: float = 203.0, pq_bits: int = 10,
                   alphas: Optional[Sequence[Optional[DecodedImage]]] = None, stream: Optional[int] = None,
                   transforms=None, out=None):
        """The HDR rendition of a batch of SDR base pictures with their decoded gain
        maps, with ONE heifgpu_render_batch_gain call (one kernel launch): a list of
        (H', W', C) device tensors with clap / irot / imir applied, float16 in linear
        light with 1.0 at SDR white for "rgb16f" / "rgba16f", uint16 PQ codes of depth
        pq_bits (10, 12, 16; sdr_white cd/m2 at SDR white) for "rgb16pq" / "rgba16pq",
        in "srgb", "display-p3" or "bt2020" primaries (out of gamut clips).  gains[i] is
        the decoded gain-map image of outs[i] (HeifImage.gain_map.item_id), of any size.
        headroom is required for Apple maps (theirs lies in the Exif maker note, which
        is not read); display_headroom limits the rendition to a display's headroom
        (None: full).  alphas as in render().  transforms: one _lib.GainTransform per
        image in place of those made here; out: the tensors to write into.  Images
        decoded for a window, or set to bilinear chroma, are refused (UnsupportedError)
        before anything is launched."""
        torch = self._torch
        f, ch, pq, transforms = self._hdr_args("render_hdr", outs, gains, fmt, alphas, transforms,
                                               (colorspace, pq_bits, headroom, display_headroom, sdr_white), out=out)
        dev = torch.device("cuda", self.device)
        dtype = torch.uint16 if pq else torch.float16
        res = out if out is not None else [
            torch.empty((o.image.display.out_height, o.image.display.out_width, ch), dtype=dtype, device=dev) for o in outs]
        imgs, aimgs, aplanes = self._render_args(outs, alphas)
        gimgs, _, _ = self._render_args(gains, None)
        xf = (ctypes.c_void_p * max(len(outs), 1))(*[ctypes.addressof(t) for t in transforms])
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(lib.heifgpu_render_batch_gain(self._h, imgs, len(outs), DecodeContext.planes_of(outs), gimgs,
                                                 DecodeContext.planes_of(gains), aimgs, aplanes, f, xf,
                                                 self._surfaces(res), ctypes.c_void_p(stream)))
        return res

    def render_hdr_scaled(self, outs: Sequence[DecodedImage], gains: Sequence[DecodedImage], size, mode: str = "cover",
                          fmt: str = "rgba16f", colorspace: str = "display-p3", headroom: Optional[float] = None,
                          display_headroom: Optional[float] = None, sdr_white: float = 203.0, pq_bits: int = 10,
                          alphas: Optional[Sequence[Optional[DecodedImage]]] = None, windows=None,
                          stream: Optional[int] = None, transforms=None, out=None):
        """render_hdr() onto a smaller (or any) grid with ONE heifgpu_render_batch_gain_scaled
        call (one kernel launch); the full-size HDR surface is never written.  size, mode
        and windows as in render_scaled(): ONE (N, h, w, C) device tensor for cover,
        stretch and windows, a list of (h_i, w_i, C) tensors for "contain"; float16 or
        uint16 as in render_hdr().  Every output pixel is the HDR formula applied to the
        exact area averages of the base's integers, of the Q8 gain codes and of the alpha
        samples over its footprint (include/heifgpu.h "Gain-map HDR render", the scaled
        call): what a viewer gives that scales base and map as images and applies the map
        afterwards, not an average in linear light.  At the window's own size the result
        is render_hdr()'s window bit for bit.  fmt, colorspace, headroom, display_headroom,
        sdr_white, pq_bits, alphas and transforms as in render_hdr(); so are the
        refusals, images decoded for a window included.  out: the (h_i, w_i, C) tensors to
        write into, which are then returned as a list."""
        torch = self._torch
        n = len(outs)
        if fmt in _lib.HDR_FORMATS and mode not in _lib.FIT_MODES:  # (a bad fmt answers first, in _hdr_args)
            raise ValueError(f"mode {mode!r}: one of {sorted(_lib.FIT_MODES)}")
        f, ch, pq, transforms = self._hdr_args("render_hdr_scaled", outs, gains, fmt, alphas, transforms,
                                               (colorspace, pq_bits, headroom, display_headroom, sdr_white),
                                               windows=windows, out=out)
        bh, bw, scales = self._scales("render_hdr_scaled", outs, alphas, size, mode, windows)
        whole, res = self._scaled_outputs(n, scales, (bh, bw) if windows is not None or mode != "contain" else None,
                                          lambda h, w: (h, w, ch), torch.uint16 if pq else torch.float16) \
            if out is None else (None, list(out))
        if n:
            imgs, aimgs, aplanes = self._render_args(outs, alphas)
            gimgs, _, _ = self._render_args(gains, None)
            xf = (ctypes.c_void_p * n)(*[ctypes.addressof(t) for t in transforms])
            if stream is None:
                stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(lib.heifgpu_render_batch_gain_scaled(self._h, imgs, n, DecodeContext.planes_of(outs), gimgs,
                                                            DecodeContext.planes_of(gains), aimgs, aplanes, f, scales, xf,
                                                            self._surfaces(res), ctypes.c_void_p(stream)))
        return whole if whole is not None else res

    def _hdr_args(self, what, outs, gains, fmt, alphas, transforms, make, **more):
        """What render_hdr and render_hdr_scaled (`what`) do alike before anything else: fmt
        as (f, channels, pq), the checks of the images, and the transforms, made here from
        make = (colorspace, pq_bits, headroom, display_headroom, sdr_white) when none are given."""
        if fmt not in _lib.HDR_FORMATS:
            raise ValueError(f"fmt {fmt!r}: one of {sorted(_lib.HDR_FORMATS)}")
        f = _lib.HDR_FORMATS[fmt]
        ch, pq = (4 if f & 1 else 3), f >= _lib.PIX_HDR_RGB16PQ
        self._check_images(what, outs, alphas, gains=gains, transforms=transforms, **more)
        if any(g is None or g.image is None for g in gains):
            raise ValueError(f"{what} needs gain images that carry their HeifImage (alloc_outputs)")
        for i, o in enumerate(outs):
            for name, im in (("image", o), ("gain image", gains[i]), ("alpha image", alphas[i] if alphas is not None else None)):
                if im is not None and im.valid is not None:
                    raise UnsupportedError(_lib.HEIFGPU_E_UNSUPPORTED,
                                           f"{what}: {name} {i} was decoded for a window ({im.valid}) only")
        if transforms is None:
            colorspace, pq_bits, headroom, display_headroom, sdr_white = make
            transforms = [o.image.gain_transform(g.image, colorspace, "pq" if pq else "linear", pq_bits, headroom,
                                                 display_headroom, sdr_white) for o, g in zip(outs, gains)]
        return f, ch, pq, transforms

    @staticmethod
    def _check_tone(colorspace, tone_map):
        """ValueError for an unknown tone_map, or one without a colorspace to map to."""
        if tone_map is None:
            return
        if tone_map not in _lib.TONE_MAPS:
            raise ValueError(f"tone_map {tone_map!r}: None or one of {sorted(_lib.TONE_MAPS)}")
        if colorspace is None:
            raise ValueError("tone_map needs a colorspace to map to")

    @staticmethod
    def _check_linear(what, linear, colorspace, filter="area", tone_map=None, size=True):
        """ValueError for linear=True where the area average in linear light is not
        defined: without a colorspace (whose tables make it linear), with another
        filter than "area", with a tone_map, or (render_jpeg) without a size."""
        if not linear:
            return
        if colorspace is None:
            raise ValueError(f"{what}: linear=True needs a colorspace")
        if filter != "area":
            raise ValueError(f"{what}: linear=True averages areas; filter {filter!r} is not done in linear light")
        if tone_map is not None:
            raise ValueError(f"{what}: linear=True with a tone_map is not done")
        if size is None:
            raise ValueError(f"{what}: linear=True needs a size (a full-size render averages nothing)")

    @staticmethod
    def _check_images(what, outs, alphas, **more):
        """ValueError unless every image and alpha image carries its HeifImage and
        alphas and the sequences of `more` have one entry per image."""
        if any(o.image is None for o in outs) or (alphas is not None and any(a is not None and a.image is None for a in alphas)):
            raise ValueError(f"{what} needs images that carry their HeifImage (alloc_outputs)")
        for name, v in dict(alphas=alphas, **more).items():
            if v is not None and len(v) != len(outs):
                raise ValueError(f"{name} must have one entry per image")

    @staticmethod
    def _surfaces(tensors):
        """The heifgpu_surface array of (h, w, C) device tensors."""
        surf = (_lib.Surface * max(len(tensors), 1))()
        for i, t in enumerate(tensors):
            surf[i].pixels = t.data_ptr()
            surf[i].pitch = t.stride(0) * t.element_size()
        return surf

    def _submit(self, name, outs, alphas, colorspace, wide, stream, mid, surf, tone_map=None, linear=False):
        """The one call of a render: lib.<name>, or lib.<name>_color with the images'
        transforms in front of the surfaces when a colorspace is asked for
        (lib.<name>_linear with linear, which _check_linear has let through).  mid: the
        arguments between the alpha planes and the surfaces."""
        imgs, aimgs, aplanes = self._render_args(outs, alphas)
        if stream is None:
            stream = self._torch.cuda.current_stream(self.device).cuda_stream
        xf, keep = self._transforms(outs, colorspace, wide, tone_map)
        if callable(mid):  # a filtered render: one entry point, its transforms (or NULL) where mid puts them
            fn, mid = getattr(lib, name), mid(xf)
        elif linear:
            fn, mid = getattr(lib, name + "_linear"), mid + (xf,)
        else:
            fn, mid = (getattr(lib, name), mid) if xf is None else (getattr(lib, name + "_color"), mid + (xf,))
        _lib.check(fn(self._h, imgs, len(outs), DecodeContext.planes_of(outs), aimgs, aplanes, *mid, surf,
                      ctypes.c_void_p(stream)))

    def _scales(self, what, outs, alphas, size, mode, windows, filter="area"):
        """(box height, box width, the heifgpu_scale of every image) of a scaled render:
        windows[i], else the fit of `mode`; ValueError if one reads samples that a
        window decode did not write (through `filter`'s taps)."""
        bh, bw = int(size[0]), int(size[1])
        scales = (_lib.Scale * max(len(outs), 1))()
        for i, o in enumerate(outs):
            if windows is not None:
                x, y, w, h = (int(v) for v in windows[i])
                scales[i] = _lib.Scale(bw, bh, x, y, w, h)
            else:
                d = o.image.display
                _lib.check(lib.heifgpu_scale_fit(ctypes.byref(d), bw, bh, _lib.FIT_MODES[mode], ctypes.byref(scales[i])))
        for i, o in enumerate(outs):
            sc = scales[i]
            _check_valid(what, i, o, alphas[i] if alphas is not None else None, (sc.x, sc.y, sc.width, sc.height),
                         (sc.out_height, sc.out_width), filter)
        return bh, bw, scales

    def _scaled_outputs(self, n, scales, box, shape, dtype):
        """(one batch tensor, its n slices) when every output has the size of `box`
        (h, w), else (None, a tensor per image of its scale's size); shape(h, w) is
        the shape of one output."""
        torch = self._torch
        dev = torch.device("cuda", self.device)
        if box is not None:
            whole = torch.empty((n,) + shape(*box), dtype=dtype, device=dev)
            return whole, [whole[i] for i in range(n)]
        return None, [torch.empty(shape(scales[i].out_height, scales[i].out_width), dtype=dtype, device=dev)
                      for i in range(n)]

    @staticmethod
    def _transforms(outs, colorspace, wide, tone_map=None):
        """(one transform pointer per image, the transforms they point to) for a
        colour-managed render call; (None, None) for colorspace None.  Raises
        before anything is launched (UnsupportedError, HeifGpuError)."""
        if colorspace is None:
            return None, None
        if colorspace not in _lib.COLORSPACES:
            raise ValueError(f"colorspace {colorspace!r}: None or one of {sorted(_lib.COLORSPACES)}")
        keep = [o.image.color_transform(colorspace, int(o.info.bit_depth) if wide else 8, tone_map) for o in outs]
        arr = (ctypes.c_void_p * max(len(outs), 1))(*[ctypes.addressof(t) for t in keep])
        return arr, keep

    @staticmethod
    def _render_args(outs, alphas):
        """The image handles and the alpha arguments of a render call."""
        n = len(outs)
        imgs = (ctypes.c_void_p * max(n, 1))(*[o.image._h.value for o in outs])
        aimgs = aplanes = None
        if alphas is not None:
            aimgs = (ctypes.c_void_p * max(n, 1))(*[a.image._h.value if a is not None else None for a in alphas])
            aplanes = (_lib.Planes * max(n, 1))()
            for i, a in enumerate(alphas):
                if a is not None:
                    aplanes[i].plane[0] = a.y.data_ptr()
                    aplanes[i].pitch[0] = a.y.stride(0) * a.y.element_size()
        return imgs, aimgs, aplanes

    def render_scaled(self, outs: Sequence[DecodedImage], size, mode: str = "cover", fmt: str = "rgb8",
                      alphas: Optional[Sequence[Optional[DecodedImage]]] = None, windows=None,
                      stream: Optional[int] = None, colorspace: Optional[str] = None, filter: str = "area",
                      tone_map: Optional[str] = None, linear: bool = False):
        """render() onto a smaller grid: the exact area average of a window of
        every displayed picture, with ONE heifgpu_render_batch_scaled call (one
        kernel launch).  size = (h, w) is the box; mode "cover" (a centred
        window of the box's aspect fills it), "stretch" (the whole picture
        fills it) or "contain" (the whole picture, its aspect kept, fits in
        it), through heifgpu_scale_fit.  windows[i] = (x, y, w, h) in displayed
        coordinates replaces the mode's window; the output is then `size`
        exactly.  Returns ONE (N, h, w, C) device tensor when every output has
        the same size (cover, stretch, windows), whose slices are the surfaces,
        and a list of (h_i, w_i, C) tensors for "contain".  Dtypes, fmt,
        alphas, colorspace and tone_map as in render(): with a colorspace the result is
        the transform of what render_scaled() writes without one (the rounded
        averages are transformed, not the source pixels).  filter "bilinear" or
        "bicubic" resamples with Pillow's antialiased filter of that name
        instead of the area average (heifgpu_render_batch_resampled): per
        channel, for the 8-bit formats, exactly what PIL's
        Image.resize(size, filter, box=window) makes of render()'s picture.
        linear=True (with a colorspace and the area filter) takes the average in
        linear light instead (heifgpu_render_batch_scaled_linear): every source
        pixel is decoded to linear before the sum and the mean is encoded after it,
        so fine bright detail keeps its light; alpha is averaged as before."""
        self._check_tone(colorspace, tone_map)
        self._check_linear("render_scaled", linear, colorspace, filter, tone_map)
        torch = self._torch
        n = len(outs)
        f = _lib.PIX_FORMATS[fmt]
        ch, wide = (4 if f & 1 else 3), f >= _lib.PIX_RGB16
        filt = _filter_code(filter)
        if mode not in _lib.FIT_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(_lib.FIT_MODES)}")
        self._check_images("render_scaled", outs, alphas, windows=windows)
        bh, bw, scales = self._scales("render_scaled", outs, alphas, size, mode, windows, filter)
        whole, res = self._scaled_outputs(n, scales, (bh, bw) if windows is not None or mode != "contain" else None,
                                          lambda h, w: (h, w, ch), torch.int16 if wide else torch.uint8)
        if n and filt == _lib.FILTER_AREA:
            self._submit("heifgpu_render_batch_scaled", outs, alphas, colorspace, wide, stream, (f, scales),
                         self._surfaces(res), tone_map, linear)
        elif n:
            self._submit("heifgpu_render_batch_resampled", outs, alphas, colorspace, wide, stream,
                         lambda xf: (f, scales, filt, xf), self._surfaces(res), tone_map)
        return whole if whole is not None else res

    def encode_jpeg(self, pictures, quality: int = 90, subsampling: str = "4:2:0", icc_profiles=None,
                    restart_mcus: int = 0) -> List[bytes]:
        """Baseline JPEG files (JFIF, Y Cb Cr) of a batch of RGB pictures, encoded on
        the device with heifgpu_jpeg_encode_batch: a fixed number of kernel launches
        for the whole batch, and only the files cross to the host.  pictures is an
        (N, h, w, 3) uint8 device tensor or a list of (h, w, 3) uint8 device tensors
        (sizes may differ; rows may be strided, pixels are packed): what render()
        and render_scaled() return for "rgb8".  quality 1..100 scales the Annex K
        tables as IJG and Pillow do; subsampling "4:2:0" or "4:4:4"; icc_profiles[i]
        (bytes or None) goes into picture i's APP2 segments; restart_mcus is the
        number of MCUs between restart markers (0: one MCU row), the unit the device
        codes in parallel.  The output buffers are a first guess; a picture that
        does not fit is encoded once more with the room its size word states.  The
        call runs on the current stream and waits for it."""
        torch = self._torch
        if subsampling not in _lib.JPEG_SUBSAMPLINGS:
            raise ValueError(f"subsampling {subsampling!r}: one of {sorted(_lib.JPEG_SUBSAMPLINGS)}")
        pics = list(pictures) if isinstance(pictures, (list, tuple)) else [pictures[i] for i in range(len(pictures))]
        n = len(pics)
        if icc_profiles is not None and len(icc_profiles) != n:
            raise ValueError("icc_profiles must have one entry per picture")
        for t in pics:
            if (t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_cuda or t.device.index != self.device
                    or t.stride(2) != 1 or t.stride(1) != 3 or 0 in t.shape):
                raise ValueError("encode_jpeg takes (h, w, 3) uint8 tensors of this context's device with packed pixels")
        if n == 0:
            return []
        opts = _lib.JpegOpts(int(quality), _lib.JPEG_SUBSAMPLINGS[subsampling], int(restart_mcus), 0)
        heads = []
        for i, t in enumerate(pics):
            icc = (icc_profiles[i] if icc_profiles is not None else None) or b""
            ln = ctypes.c_size_t()
            args = (t.shape[1], t.shape[0], ctypes.byref(opts), _lib.u8buf(icc), len(icc))
            _lib.check(lib.heifgpu_jpeg_header(*args, None, 0, ctypes.byref(ln)))
            buf = (ctypes.c_uint8 * ln.value)()
            _lib.check(lib.heifgpu_jpeg_header(*args, buf, ln.value, ctypes.byref(ln)))
            heads.append(bytes(buf))
        dev = torch.device("cuda", self.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        per_px = 0.75 if subsampling == "4:2:0" else 1.25  # bytes: room for quality 90 and some above
        caps = [min(int(t.shape[0] * t.shape[1] * per_px) + 4096, 2 ** 31 - 16) for t in pics]
        scans = [None] * n
        todo = list(range(n))
        for _ in range(2):  # the guess, then the stated sizes
            offs, total = [], 0
            for i in todo:
                offs.append(total)
                total += (caps[i] + 15) // 16 * 16
            out = torch.empty(total, dtype=torch.uint8, device=dev)
            sizes = torch.empty(len(todo), dtype=torch.int64, device=dev)
            src = self._surfaces([pics[i] for i in todo])
            dst = (_lib.Surface * len(todo))()
            for k, i in enumerate(todo):
                dst[k].pixels = out.data_ptr() + offs[k]
                dst[k].pitch = caps[i]
            ws = (ctypes.c_uint32 * len(todo))(*[pics[i].shape[1] for i in todo])
            hs = (ctypes.c_uint32 * len(todo))(*[pics[i].shape[0] for i in todo])
            _lib.check(lib.heifgpu_jpeg_encode_batch(self._h, len(todo), src, ws, hs, ctypes.byref(opts), dst,
                                                     ctypes.cast(sizes.data_ptr(), ctypes.POINTER(ctypes.c_uint64)), stream))
            got = [int(v) & (2 ** 64 - 1) for v in sizes.cpu().tolist()]  # (the copy waits for the kernels)
            again = []
            for k, i in enumerate(todo):
                size = got[k] & ~_lib.JPEG_TOO_SMALL
                if got[k] & _lib.JPEG_TOO_SMALL:
                    caps[i] = size
                    again.append(i)
                else:
                    scans[i] = bytes(out[offs[k]:offs[k] + size].cpu().numpy())
            todo = again
            if not todo:
                break
        if todo:
            raise HeifGpuError(_lib.HEIFGPU_E_DEVICE, "encode_jpeg: a picture did not fit the size the device stated")
        return [h + s for h, s in zip(heads, scans)]

    def render_jpeg(self, outs: Sequence[DecodedImage], size=None, mode: str = "cover", windows=None,
                    filter: str = "area", colorspace: Optional[str] = None, tone_map: Optional[str] = None,
                    quality: int = 90, subsampling: str = "4:2:0", embed_icc: bool = True, icc_profiles=None,
                    restart_mcus: int = 0, linear: bool = False) -> List[bytes]:
        """The JPEG files of a batch of decoded images: render() (render_scaled() when
        size or windows is given; windows need a size) as "rgb8", then encode_jpeg(),
        all on the device.  JPEG has no alpha: the pictures are rendered opaque.
        With colorspace None and embed_icc, each item's own ICC profile
        (HeifImage.icc_profile, when it has one) is embedded, which is what makes a
        Display P3 picture look right in a viewer; an nclx-only item gets none.  With
        colorspace "srgb" nothing is embedded (an untagged JPEG is taken as sRGB).
        With "display-p3" nothing is embedded either, so most viewers will show the
        picture as sRGB, unless the caller passes icc_profiles (one profile or None
        per image, embedded as given whatever the colorspace): this library reads
        ICC profiles and does not write them.  linear (with a size) as in
        render_scaled()."""
        if windows is not None and size is None:
            raise ValueError("render_jpeg: windows need a size")
        self._check_linear("render_jpeg", linear, colorspace, filter, tone_map, size)
        if size is not None:
            rgb = self.render_scaled(outs, size, mode, "rgb8", None, windows, colorspace=colorspace, filter=filter,
                                     tone_map=tone_map, linear=linear)
        else:
            rgb = self.render(outs, "rgb8", None, colorspace=colorspace, tone_map=tone_map)
        if icc_profiles is None and colorspace is None and embed_icc:
            icc_profiles = [o.image.icc_profile for o in outs]
        return self.encode_jpeg(rgb, quality, subsampling, icc_profiles, restart_mcus)

    @staticmethod
    def _png_first_guess(filtered: int) -> int:
        """encode_png's first capacity for a picture of `filtered` filtered bytes: eight bits a
        byte, and per block the code lengths (at most 235 bytes) and the chunk around them (21).
        Filtered pictures stay far below it; a picture that does not is encoded once more."""
        return filtered + (filtered // _lib.PNG_BLOCK + 1) * 256 + 64

    def encode_png(self, pictures, bits: Optional[int] = None, filter: str = "adaptive", icc_profiles=None,
                   srgb: bool = False, cicp=None) -> List[bytes]:
        """PNG files of a batch of RGB or RGBA pictures of 8 or 16 bits, encoded on the
        device with heifgpu_png_encode_batch: a fixed number of kernel launches for
        the whole batch, and only the files cross to the host.  The files are lossless:
        a reader gets back exactly the samples given, alpha included.  pictures is an
        (N, h, w, C) device tensor or a list of (h, w, C) device tensors, C 3 or 4,
        uint8, or int16 / uint16 for the 16-bit formats (sizes may differ; rows may be
        strided, pixels are packed; one dtype and C per call): what render(),
        render_scaled() and render_hdr(fmt="rgb16pq") return.  bits is the number of
        significant bits of 16-bit samples (the image's bit depth; None: 16): sample s
        is stored as (s << (16 - bits)) | (s >> (2 bits - 16)) with an sBIT chunk, so
        s = v >> (16 - bits) comes back.  filter "adaptive" picks per row the PNG
        filter type with the least sum of magnitudes; "none", "sub", "up", "average"
        or "paeth" forces one.  At most one of: icc_profiles[i] (bytes or None) goes
        into picture i's iCCP chunk; srgb=True writes an sRGB chunk; cicp=(primaries,
        transfer, matrix, full_range) writes a cICP chunk.  An HDR PNG is
        encode_png(render_hdr(outs, gains, fmt="rgb16pq", pq_bits=P), bits=P,
        cicp=(primaries, 16, 0, 1)), primaries 1 (BT.709), 12 (Display P3) or 9
        (BT.2020).  The deflate stream is Huffman-coded literals in independent blocks
        (no matches: long flat regions, such as a fully transparent area, cost one bit
        per byte).  The output buffers are a first guess; a picture that does not fit
        is encoded once more with the room its size word states.  The call runs on the
        current stream and waits for it."""
        torch = self._torch
        if filter not in _lib.PNG_FILTERS:
            raise ValueError(f"filter {filter!r}: one of {sorted(_lib.PNG_FILTERS)}")
        pics = list(pictures) if isinstance(pictures, (list, tuple)) else [pictures[i] for i in range(len(pictures))]
        n = len(pics)
        if icc_profiles is not None and len(icc_profiles) != n:
            raise ValueError("icc_profiles must have one entry per picture")
        if (icc_profiles is not None and any(icc_profiles)) + bool(srgb) + (cicp is not None) > 1:
            raise ValueError("encode_png: at most one of icc_profiles, srgb and cicp")
        if cicp is not None and (len(cicp) != 4 or any(not 0 <= int(v) <= 255 for v in cicp)):
            raise ValueError("cicp: four values in 0..255")
        if n == 0:
            return []
        wide_types = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ())
        wide, ch = pics[0].dtype in wide_types, pics[0].shape[-1] if pics[0].dim() == 3 else 0
        for t in pics:
            if (t.dtype != pics[0].dtype or (t.dtype != torch.uint8 and not wide) or t.dim() != 3 or t.shape[2] != ch
                    or ch not in (3, 4) or not t.is_cuda or t.device.index != self.device or t.stride(2) != 1
                    or t.stride(1) != ch or 0 in t.shape):
                raise ValueError("encode_png takes (h, w, 3 or 4) uint8 or int16 / uint16 tensors of this context's device, "
                                 "one dtype and channel count per call, with packed pixels")
        if bits is None:
            bits = 16 if wide else 8
        fmt = (_lib.PIX_RGB16 if wide else 0) | (1 if ch == 4 else 0)
        opts = _lib.PngOpts(fmt, int(bits), _lib.PNG_FILTERS[filter], 0)
        bpp = ch * (2 if wide else 1)
        heads, keep = [], []
        for i, t in enumerate(pics):
            col = _lib.PngColour()
            icc = (icc_profiles[i] if icc_profiles is not None else None) or b""
            if icc:
                keep = _lib.u8buf(icc)
                col.kind, col.icc, col.icc_len = _lib.PNG_COLOUR_ICC, ctypes.cast(keep, ctypes.POINTER(ctypes.c_uint8)), len(icc)
            elif srgb:
                col.kind = _lib.PNG_COLOUR_SRGB
            elif cicp is not None:
                col.kind = _lib.PNG_COLOUR_CICP
                col.cicp[:] = [int(v) for v in cicp]
            ln = ctypes.c_size_t()
            args = (t.shape[1], t.shape[0], ctypes.byref(opts), ctypes.byref(col))
            _lib.check(lib.heifgpu_png_header(*args, None, 0, ctypes.byref(ln)))
            buf = (ctypes.c_uint8 * ln.value)()
            _lib.check(lib.heifgpu_png_header(*args, buf, ln.value, ctypes.byref(ln)))
            heads.append(bytes(buf))
        dev = torch.device("cuda", self.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        caps = [min(self._png_first_guess(t.shape[0] * (t.shape[1] * bpp + 1)), 2 ** 31 - 16) for t in pics]
        bodies = [None] * n
        todo = list(range(n))
        for _ in range(2):  # the guess, then the stated sizes
            offs, total = [], 0
            for i in todo:
                offs.append(total)
                total += (caps[i] + 15) // 16 * 16
            out = torch.empty(total, dtype=torch.uint8, device=dev)
            sizes = torch.empty(len(todo), dtype=torch.int64, device=dev)
            src = self._surfaces([pics[i] for i in todo])
            dst = (_lib.Surface * len(todo))()
            for k, i in enumerate(todo):
                dst[k].pixels = out.data_ptr() + offs[k]
                dst[k].pitch = caps[i]
            ws = (ctypes.c_uint32 * len(todo))(*[pics[i].shape[1] for i in todo])
            hs = (ctypes.c_uint32 * len(todo))(*[pics[i].shape[0] for i in todo])
            _lib.check(lib.heifgpu_png_encode_batch(self._h, len(todo), src, ws, hs, ctypes.byref(opts), dst,
                                                    ctypes.cast(sizes.data_ptr(), ctypes.POINTER(ctypes.c_uint64)), stream))
            got = [int(v) & (2 ** 64 - 1) for v in sizes.cpu().tolist()]  # (the copy waits for the kernels)
            again = []
            for k, i in enumerate(todo):
                size = got[k] & ~_lib.PNG_TOO_SMALL
                if got[k] & _lib.PNG_TOO_SMALL:
                    caps[i] = size
                    again.append(i)
                else:
                    bodies[i] = bytes(out[offs[k]:offs[k] + size].cpu().numpy())
            todo = again
            if not todo:
                break
        if todo:
            raise HeifGpuError(_lib.HEIFGPU_E_DEVICE, "encode_png: a picture did not fit the size the device stated")
        return [h + s for h, s in zip(heads, bodies)]

    def render_png(self, outs: Sequence[DecodedImage], size=None, mode: str = "cover", windows=None, fmt: str = "rgb8",
                   alphas: Optional[Sequence[Optional[DecodedImage]]] = None, filter: str = "area",
                   colorspace: Optional[str] = None, tone_map: Optional[str] = None, linear: bool = False,
                   embed_icc: bool = True, icc_profiles=None) -> List[bytes]:
        """The PNG files of a batch of decoded images: render() (render_scaled() when
        size or windows is given; windows need a size) in `fmt` ("rgb8", "rgba8",
        "rgb16", "rgba16", with alphas as there), then encode_png(), all on the
        device: the file holds exactly the render's pixels.  The 16-bit formats need
        one bit depth in the batch, which becomes encode_png's bits.  `filter` is the
        resize filter of render_scaled(); the PNG row filter is adaptive.  With
        colorspace "srgb" the files carry an sRGB chunk, with "display-p3" a cICP chunk
        of (12, 13, 0, 1).  With colorspace None and embed_icc, each item's own ICC
        profile (HeifImage.icc_profile, when it has one) goes into an iCCP chunk; an
        nclx-only item gets no colour chunk.  icc_profiles (one profile or None per
        image) are embedded as given instead, whatever the colorspace.  linear (with a
        size) as in render_scaled()."""
        if windows is not None and size is None:
            raise ValueError("render_png: windows need a size")
        if fmt not in ("rgb8", "rgba8", "rgb16", "rgba16"):
            raise ValueError(f"render_png: fmt {fmt!r}: one of rgb8, rgba8, rgb16, rgba16")
        self._check_linear("render_png", linear, colorspace, filter, tone_map, size)
        bits = 8
        if fmt.endswith("16"):
            depths = {o.info.bit_depth for o in outs}
            if len(depths) > 1:
                raise ValueError(f"render_png: {fmt} needs one bit depth in the batch, got {sorted(depths)}")
            bits = depths.pop() if depths else 16
        if size is not None:
            px = self.render_scaled(outs, size, mode, fmt, alphas, windows, colorspace=colorspace, filter=filter,
                                    tone_map=tone_map, linear=linear)
        else:
            px = self.render(outs, fmt, alphas, colorspace=colorspace, tone_map=tone_map)
        srgb, cicp = False, None
        if icc_profiles is None:
            if colorspace == "srgb":
                srgb = True
            elif colorspace == "display-p3":
                cicp = (12, 13, 0, 1)
            elif colorspace is None and embed_icc:
                icc_profiles = [o.image.icc_profile for o in outs]
        return self.encode_png(px, bits, "adaptive", icc_profiles, srgb, cicp)

    def render_tensor(self, outs: Sequence[DecodedImage], size, mode: str = "cover", dtype=None, layout: str = "chw",
                      mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), src: str = "rgb8", windows=None,
                      flips=None, alphas: Optional[Sequence[Optional[DecodedImage]]] = None, scale_bias=None,
                      stream: Optional[int] = None, colorspace: Optional[str] = None, filter: str = "area",
                      tone_map: Optional[str] = None, linear: bool = False):
        """render_scaled() as a loader wants it: crop, flip and normalise into
        float elements with ONE heifgpu_render_batch_tensor call (one kernel
        launch).  With R the integers render_scaled(fmt=src) gives, flipped
        (flips[i] & 1 reverses the columns, & 2 the rows), every element is
        float32(R) * a[c] + b[c] in float32 (two roundings), rounded to `dtype`
        (torch.float16 by default, float32 or bfloat16).  a and b come from
        scale_bias=(a, b), or from mean / std (one per channel; four for an
        RGBA src): a = float32(1 / (maxv * std)), b = float32(-mean / std),
        maxv = 255 for the 8-bit sources and (1 << B) - 1 for the 16-bit ones
        (pictures of different bit depths B then have no common a, b: ValueError).
        layout "chw" returns ONE (N, C, h, w) tensor, "hwc" ONE (N, h, w, C)
        tensor, for cover, stretch and windows; "contain" returns a list of
        (C, h_i, w_i) or (h_i, w_i, C) tensors.  size, mode, windows, alphas,
        colorspace, tone_map and filter as in render_scaled(): R is then what
        render_scaled(colorspace=, filter=, tone_map=) gives (with "bilinear" or "bicubic"
        the pixels Pillow's resize gives, which is what most vision models were
        trained on; a flip then acts on R, not on the taps).  linear as in
        render_scaled(): R is then what render_scaled(linear=True) gives
        (heifgpu_render_batch_tensor_linear)."""
        filt = _filter_code(filter)
        self._check_tone(colorspace, tone_map)
        self._check_linear("render_tensor", linear, colorspace, filter, tone_map)
        torch = self._torch
        n = len(outs)
        f = _lib.PIX_FORMATS[src]
        ch, wide = (4 if f & 1 else 3), f >= _lib.PIX_RGB16
        dtype = torch.float16 if dtype is None else dtype
        elems = {torch.float32: _lib.ELEM_F32, torch.float16: _lib.ELEM_F16, torch.bfloat16: _lib.ELEM_BF16}
        if dtype not in elems:
            raise ValueError(f"dtype {dtype!r}: torch.float32, torch.float16 or torch.bfloat16")
        if layout not in _lib.LAYOUTS:
            raise ValueError(f"layout {layout!r}: one of {sorted(_lib.LAYOUTS)}")
        if mode not in _lib.FIT_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(_lib.FIT_MODES)}")
        self._check_images("render_tensor", outs, alphas, windows=windows, flips=flips)
        if flips is not None and any(int(v) not in (0, 1, 2, 3) for v in flips):
            raise ValueError("flips[i] is 0, 1 (columns), 2 (rows) or 3 (both)")
        tf = _lib.TensorFormat(src=f, elem=elems[dtype], layout=_lib.LAYOUTS[layout])
        if scale_bias is not None:
            a, b = ([float(v) for v in part] for part in scale_bias)
            if len(a) != ch or len(b) != ch:
                raise ValueError(f"scale_bias needs {ch} scales and {ch} biases for {src}")
        else:
            mean, std = [float(v) for v in mean], [float(v) for v in std]
            if len(mean) != ch or len(std) != ch:
                raise ValueError(f"mean and std need {ch} entries for {src}")
            depths = {int(o.info.bit_depth) for o in outs} if wide else {8}
            if len(depths) > 1:
                raise ValueError(f"pictures of bit depths {sorted(depths)} share no scale for {src}: pass scale_bias")
            maxv = float((1 << depths.pop()) - 1) if depths else 255.0
            a, b = [1.0 / (maxv * s) for s in std], [-m / s for m, s in zip(mean, std)]  # in double, rounded once below
        for c in range(ch):
            tf.a[c], tf.b[c] = a[c], b[c]
        bh, bw, scales = self._scales("render_tensor", outs, alphas, size, mode, windows, filter)
        chw = layout == "chw"
        whole, res = self._scaled_outputs(n, scales, (bh, bw) if windows is not None or mode != "contain" else None,
                                          lambda h, w: (ch, h, w) if chw else (h, w, ch), dtype)
        if n == 0:
            return whole if whole is not None else res
        surf = (_lib.TensorSurface * n)()
        for i, t in enumerate(res):
            surf[i].data = t.data_ptr()
            surf[i].stride_c = t.stride(0) * t.element_size() if chw else 0
            surf[i].stride_y = t.stride(1 if chw else 0) * t.element_size()
        fl = None if flips is None else (ctypes.c_uint32 * n)(*[int(v) for v in flips])
        if filt == _lib.FILTER_AREA:
            self._submit("heifgpu_render_batch_tensor", outs, alphas, colorspace, wide, stream,
                         (ctypes.byref(tf), scales, fl), surf, tone_map, linear)
        else:
            self._submit("heifgpu_render_batch_tensor_resampled", outs, alphas, colorspace, wide, stream,
                         lambda xf: (ctypes.byref(tf), scales, filt, fl, xf), surf, tone_map)
        return whole if whole is not None else res


def ipc_export(tensor) -> bytes:
    """heifgpu_ipc_export of a device tensor's storage: 72 bytes another
    process passes to ipc_open (e.g. through torch.distributed)."""
    h = _lib.IpcHandle()
    _lib.check(lib.heifgpu_ipc_export(ctypes.c_void_p(tensor.data_ptr()), ctypes.byref(h)))
    return bytes(h)


def ipc_open(device: int, blob: bytes) -> int:
    """Maps another process's exported allocation on `device`; returns the
    device address of the exported byte (close with ipc_close)."""
    h = _lib.IpcHandle.from_buffer_copy(blob)
    p = ctypes.c_void_p()
    _lib.check(lib.heifgpu_ipc_open(device, ctypes.byref(h), ctypes.byref(p)))
    return p.value


def ipc_close(ptr: int) -> None:
    _lib.check(lib.heifgpu_ipc_close(ctypes.c_void_p(ptr)))


class DeviceBatch:
    """Device-resident batch: bitstreams uploaded once, decoded many times."""

    def __init__(self, ctx: DecodeContext, handle: ctypes.c_void_p, images: List[HeifImage]):
        self.ctx, self._h, self.images = ctx, handle, images
        # window decode: per image the (x, y, w, h) of its planes this load decodes for
        # certain, None where it decodes everything (DecodeContext.prepare sets it)
        self.rects: List[Optional[tuple]] = [None] * len(images)

    def decode_async(self, outs: Sequence[DecodedImage], stream: Optional[int] = None):
        torch = self.ctx._torch
        if stream is None:
            stream = torch.cuda.current_stream(self.ctx.device).cuda_stream
        planes = DecodeContext.planes_of(outs)
        _lib.check(lib.heifgpu_batch_decode(self.ctx._h, self._h, planes, ctypes.c_void_p(stream)))
        for o, r in zip(outs, self.rects):
            o.valid = r

    @property
    def pictures(self) -> int:
        """The pictures this load decodes (heifgpu_batch_picture_count)."""
        v = ctypes.c_uint32()
        _lib.check(lib.heifgpu_batch_picture_count(self._h, ctypes.byref(v)))
        return v.value

    def status(self, stream: Optional[int] = None) -> List[int]:
        torch = self.ctx._torch
        if stream is None:
            stream = torch.cuda.current_stream(self.ctx.device).cuda_stream
        st = (ctypes.c_uint32 * len(self.images))()
        rc = lib.heifgpu_batch_status(self.ctx._h, self._h, st, ctypes.c_void_p(stream))
        if rc not in (_lib.HEIFGPU_OK, _lib.HEIFGPU_E_DECODE):
            _lib.check(rc)
        return list(st)

    def status_previous(self, stream: Optional[int] = None) -> List[int]:
        """Per-image status of the load before the current one (its decodes
        that were in flight at the reload), read and cleared
        (heifgpu_batch_status_previous); [] if there was no previous load."""
        torch = self.ctx._torch
        if stream is None:
            stream = torch.cuda.current_stream(self.ctx.device).cuda_stream
        n = ctypes.c_size_t()
        rc = lib.heifgpu_batch_status_previous(self.ctx._h, self._h, None, 0, ctypes.byref(n),
                                               ctypes.c_void_p(stream))
        if n.value == 0:
            _lib.check(rc)
            return []
        st = (ctypes.c_uint32 * n.value)()
        rc = lib.heifgpu_batch_status_previous(self.ctx._h, self._h, st, n.value, ctypes.byref(n),
                                               ctypes.c_void_p(stream))
        if rc not in (_lib.HEIFGPU_OK, _lib.HEIFGPU_E_DECODE):
            _lib.check(rc)
        return list(st)

    def parse_geometry(self) -> dict:
        """The CABAC parse launch of this batch (heifgpu_batch_parse_geometry)."""
        v = [ctypes.c_uint32() for _ in range(4)]
        _lib.check(lib.heifgpu_batch_parse_geometry(self._h, *[ctypes.byref(x) for x in v]))
        mode = {_lib.PARSE_LANES: "lanes", _lib.PARSE_SOLO: "solo", _lib.PARSE_SPREAD: "spread"}[v[0].value]
        return {"mode": mode, "workgroups": v[1].value, "pics_per_wave": v[2].value,
                "waves_per_workgroup": v[3].value}

    def lanes_variant(self) -> str:
        """The body this batch's lanes parse runs (heifgpu_batch_lanes_variant):
        "lean" or "general" ("general" too in the other parse modes).
        HEIFGPU_LANES_VARIANT=general at prepare keeps the general body."""
        if not hasattr(lib, "heifgpu_batch_lanes_variant"):  # an earlier build of this ABI
            return "general"
        v = ctypes.c_uint32()
        _lib.check(lib.heifgpu_batch_lanes_variant(self._h, ctypes.byref(v)))
        return "lean" if v.value else "general"

    def free(self):
        if self._h is not None and self._h.value:
            lib.heifgpu_batch_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HeicDecoder:
    """Mirror of heif::HeicDecoder (src/heic/decoder.rs:8-132)."""

    _ctx: dict = {}

    @classmethod
    def context(cls, device: int = 0) -> DecodeContext:
        ctx = cls._ctx.get(device)
        if ctx is None:
            ctx = cls._ctx[device] = DecodeContext(device)
        return ctx

    @classmethod
    def decode_rgb(cls, data: bytes, device: int = 0, item_id: int = 0):
        """decode() then YCbCr -> RGB8 with the irot rotation (libheif's default output)."""
        return cls.context(device).to_rgb(cls.decode(data, device, item_id))

    @staticmethod
    def _fit_window(img: HeifImage, size, mode: str):
        """The window of the displayed picture that render_scaled / render_tensor
        read for (size, mode); None: the whole picture."""
        if size is None:
            return None
        if mode not in _lib.FIT_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(_lib.FIT_MODES)}")
        sc = _lib.Scale()
        d = img.display
        _lib.check(lib.heifgpu_scale_fit(ctypes.byref(d), int(size[1]), int(size[0]), _lib.FIT_MODES[mode],
                                         ctypes.byref(sc)))
        return (sc.x, sc.y, sc.width, sc.height) if sc.width or sc.height else None

    @classmethod
    def _decode_pair(cls, data: bytes, device: int, size, mode: str, tiles: str, with_alpha: bool,
                     filter: str = "area", chroma: str = "replicate", chroma_loc: Optional[int] = None):
        """The primary image and (with_alpha, when the file has one) its alpha
        image, decoded whole (tiles="all") or for the window that (size, mode)
        reads through `filter` (tiles="window")."""
        if tiles not in ("all", "window"):
            raise ValueError(f"tiles {tiles!r}: 'all' or 'window'")
        _filter_code(filter)
        ctx = cls.context(device)
        img = HeifImage.parse(data, chroma=chroma)
        img.chroma_loc = chroma_loc
        rect = None
        if tiles == "window":
            rsize = None
            if size is not None and filter != "area":  # the rendered size: the fit's, not the box ("contain")
                sc = _lib.Scale()
                d = img.display
                _lib.check(lib.heifgpu_scale_fit(ctypes.byref(d), int(size[1]), int(size[0]), _lib.FIT_MODES[mode],
                                                 ctypes.byref(sc)))
                rsize = (sc.out_height, sc.out_width)
            rect = img.source_rect(cls._fit_window(img, size, mode), rsize, filter if rsize is not None else "area")
        out = cls._decode_image(ctx, img, rect)
        aid = img.display.alpha_item_id
        alpha = cls._decode_image(ctx, HeifImage.parse(data, aid), rect) if aid and with_alpha else None
        return out, alpha

    @classmethod
    def decode_display(cls, data: bytes, fmt: Optional[str] = None, device: int = 0, size=None,
                       mode: str = "contain", tiles: str = "all", colorspace: Optional[str] = None,
                       filter: str = "area", tone_map: Optional[str] = None, peak_nits: Optional[float] = None,
                       chroma: str = "replicate", chroma_loc: Optional[int] = None, linear: bool = False):
        """The picture a viewer shows: decodes the primary image and, when it
        has one (display.alpha_item_id), its alpha plane, then renders
        (DecodeContext.render) with clap / irot / imir applied.  fmt None picks
        RGBA when there is alpha and 16 bits when the bit depth is above 8.
        size = (h, w) renders it into that box instead (DecodeContext.render_scaled
        with `mode`); None is the full size.  tiles="window" decodes only the
        grid tiles the rendered window reads (of the alpha image too): the same
        pixels, bit for bit, for less work when `mode` or a clap crops.
        colorspace "srgb" / "display-p3" converts the picture from its ICC profile
        or nclx description to that space (DecodeContext.render); None leaves it
        in its own, unlabelled.  filter, with a size: "area" (the area average,
        right for reduction), "bilinear" or "bicubic" (Pillow's antialiased
        filters, which also interpolate an enlargement as a viewer expects).
        tone_map "bt2390", with a colorspace, shows a PQ / HLG picture tone-mapped
        to SDR (DecodeContext.render); peak_nits replaces the source peak the file
        states (clli, mdcv).  chroma "bilinear" interpolates 4:2:0 / 4:2:2 chroma at
        the sample location the stream signals (chroma_loc 0..5 replaces it) instead
        of replicating it (HeifImage.chroma_upsampling); with tiles="window" the
        decoded rectangle then includes the samples the taps read.  linear=True, with a
        size and a colorspace, averages in linear light (DecodeContext.render_scaled)."""
        DecodeContext._check_tone(colorspace, tone_map)
        DecodeContext._check_linear("decode_display", linear, colorspace, filter, tone_map, size)
        ctx = cls.context(device)
        out, alpha = cls._decode_pair(data, device, size, mode, tiles, True, filter, chroma, chroma_loc)
        out.image.peak_nits = peak_nits
        if fmt is None:
            fmt = ("rgba" if alpha is not None else "rgb") + ("16" if out.info.bit_depth > 8 else "8")
        alphas = [alpha] if alpha is not None else None
        if size is not None:
            return ctx.render_scaled([out], size, mode, fmt, alphas, colorspace=colorspace, filter=filter,
                                     tone_map=tone_map, linear=linear)[0]
        return ctx.render([out], fmt, alphas, colorspace=colorspace, tone_map=tone_map)[0]

    @classmethod
    def decode_jpeg(cls, data: bytes, device: int = 0, size=None, mode: str = "cover", filter: str = "area",
                    colorspace: Optional[str] = None, tone_map: Optional[str] = None, quality: int = 90,
                    subsampling: str = "4:2:0", embed_icc: bool = True, icc_profile: Optional[bytes] = None,
                    restart_mcus: int = 0, linear: bool = False) -> bytes:
        """One HEIC file as one baseline JPEG file: decodes the primary image, then
        DecodeContext.render_jpeg of that one picture (its arguments; icc_profile is
        render_jpeg's icc_profiles for the one picture)."""
        DecodeContext._check_tone(colorspace, tone_map)
        DecodeContext._check_linear("decode_jpeg", linear, colorspace, filter, tone_map, size)
        out, _ = cls._decode_pair(data, device, size, mode, "all", False, filter)
        return cls.context(device).render_jpeg([out], size, mode, None, filter, colorspace, tone_map, quality, subsampling,
                                               embed_icc, None if icc_profile is None else [icc_profile], restart_mcus,
                                               linear)[0]

    @classmethod
    def decode_png(cls, data: bytes, fmt: Optional[str] = None, device: int = 0, size=None, mode: str = "cover",
                   tiles: str = "all", filter: str = "area", colorspace: Optional[str] = None,
                   tone_map: Optional[str] = None, linear: bool = False, embed_icc: bool = True,
                   icc_profile: Optional[bytes] = None) -> bytes:
        """One HEIC file as one PNG file: decodes the primary image and, when it has
        one, its alpha plane, then DecodeContext.render_png of that one picture (its
        arguments; icc_profile is render_png's icc_profiles for the one picture).
        fmt None picks the format as decode_display does: RGBA when the file has
        alpha, 16 bits (with an sBIT chunk of the bit depth) above 8.  tiles="window"
        decodes only the grid tiles the rendered window reads, as there."""
        DecodeContext._check_tone(colorspace, tone_map)
        DecodeContext._check_linear("decode_png", linear, colorspace, filter, tone_map, size)
        with_alpha = fmt is None or fmt.startswith("rgba")
        out, alpha = cls._decode_pair(data, device, size, mode, tiles, with_alpha, filter)
        if fmt is None:
            fmt = ("rgba" if alpha is not None else "rgb") + ("16" if out.info.bit_depth > 8 else "8")
        alphas = [alpha] if alpha is not None and fmt.startswith("rgba") else None
        return cls.context(device).render_png([out], size, mode, None, fmt, alphas, filter, colorspace, tone_map, linear,
                                              embed_icc, None if icc_profile is None else [icc_profile])[0]

    @classmethod
    def decode_hdr(cls, data: bytes, fmt: Optional[str] = None, device: int = 0, colorspace: str = "display-p3",
                   headroom: Optional[float] = None, display_headroom: Optional[float] = None,
                   sdr_white: float = 203.0, pq_bits: int = 10, size=None, mode: str = "contain"):
        """The HDR rendition of a file whose primary image has a gain map
        (HeifImage.gain_map): decodes the primary image, its gain-map image and, when
        it has one, its alpha plane, then DecodeContext.render_hdr of that one picture.
        fmt None picks "rgba16f" when there is alpha, else "rgb16f".  ValueError for a
        file without a gain map; an Apple map needs the caller's headroom.  size = (h, w)
        renders onto that box instead (DecodeContext.render_hdr_scaled with `mode`, in the
        same one launch: the full-size HDR picture is never written)."""
        ctx = cls.context(device)
        out, alpha = cls._decode_pair(data, device, None, "contain", "all", True)
        gm = out.image.gain_map
        if gm is None:
            raise ValueError("decode_hdr: the file's primary image has no gain map")
        gain = cls._decode_image(ctx, HeifImage.parse(data, gm.item_id), None)
        if fmt is None:
            fmt = "rgba16f" if alpha is not None else "rgb16f"
        alphas = [alpha] if alpha is not None and fmt.startswith("rgba") else None
        if size is not None:
            return ctx.render_hdr_scaled([out], [gain], size, mode, fmt, colorspace, headroom, display_headroom, sdr_white,
                                         pq_bits, alphas)[0]
        return ctx.render_hdr([out], [gain], fmt, colorspace, headroom, display_headroom, sdr_white, pq_bits, alphas)[0]

    @classmethod
    def decode_tensor(cls, data: bytes, size, mode: str = "cover", device: int = 0, flip: int = 0,
                      tiles: str = "all", peak_nits: Optional[float] = None, chroma: str = "replicate",
                      chroma_loc: Optional[int] = None, **kw):
        """decode_display(size=) as a normalised float tensor: decodes the
        primary image (and its alpha plane when `src` is an RGBA format and the
        file has one), then DecodeContext.render_tensor of that one picture:
        (C, h, w), or (h, w, C) for layout="hwc".  dtype, layout, mean, std, src
        scale_bias, colorspace, tone_map, filter and linear go through to render_tensor; tiles and
        peak_nits, chroma and chroma_loc as in decode_display."""
        DecodeContext._check_tone(kw.get("colorspace"), kw.get("tone_map"))
        DecodeContext._check_linear("decode_tensor", kw.get("linear", False), kw.get("colorspace"), kw.get("filter", "area"),
                                    kw.get("tone_map"))
        ctx = cls.context(device)
        rgba = kw.get("src", "rgb8").startswith("rgba")
        out, alpha = cls._decode_pair(data, device, size, mode, tiles, rgba, kw.get("filter", "area"), chroma, chroma_loc)
        alphas = [alpha] if alpha is not None else None
        out.image.peak_nits = peak_nits
        return ctx.render_tensor([out], size, mode, flips=[flip], alphas=alphas, **kw)[0]

    @classmethod
    def decode(cls, data: bytes, device: int = 0, item_id: int = 0, window=None, rect=None) -> DecodedImage:
        """Decodes one image item.  window = (x, y, w, h) in displayed
        coordinates decodes only the grid tiles a render of that window reads
        (DecodedImage.valid then names the rectangle of the planes that was
        written); rect gives it in decoded-plane coordinates instead (an alpha
        image takes its colour image's HeifImage.source_rect(window))."""
        ctx = cls.context(device)
        img = HeifImage.parse(data, item_id)
        if rect is None and window is not None:
            rect = img.source_rect(window)
        return cls._decode_image(ctx, img, rect)

    @staticmethod
    def _decode_image(ctx: DecodeContext, img: HeifImage, rect) -> DecodedImage:
        outs = ctx.alloc_outputs([img])
        batch = ctx.prepare([img], rects=[rect])
        try:
            batch.decode_async(outs)
            st = batch.status()
        finally:
            batch.free()
        if st[0]:
            bits = [n for b, n in _lib.STATUS_BITS.items() if st[0] & b]
            raise HeifGpuError(_lib.HEIFGPU_E_DECODE, f"bitstream check failed: {bits}")
        return outs[0]
