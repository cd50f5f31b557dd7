// heic_image.cpp — see heic_image.hpp.
#include "heic_image.hpp"

#include <algorithm>
#include <cstring>
#include <map>

namespace hg {

namespace {

// read_hvcc_nal_unit (decoder.rs:135-143): 2-byte header + EP-stripped RBSP
std::vector<uint8_t> nal_rbsp(const std::vector<uint8_t> &nal) {
    if (nal.size() < 3) throw HeifError("nal unit is too short");
    return RbspReader::remove_emulation_prevention(nal.data() + 2, nal.size() - 2);
}

void check_supported(const SequenceParameterSet &s, const PictureParameterSet &p) {
    if (s.separate_colour_plane_flag) throw UnsupportedError("separate_colour_plane_flag");
    if (s.bit_depth_luma_minus8 != s.bit_depth_chroma_minus8) throw UnsupportedError("luma/chroma bit depth differ");
    if (s.range_extension_tools || p.range_extension_tools) throw UnsupportedError("range-extension coding tools");
    // HEVC tiles decode as sub-pictures (batch.cpp), with WPP each tile's CTB rows
    // its substreams (9.3.1: a row of a tile syncs with the tile's row above)
    if (s.pic_width_in_luma_samples > 8192 || s.pic_height_in_luma_samples > 8192)
        throw UnsupportedError("picture larger than 8192");
    if (s.pic_width_in_luma_samples % (1 << s.log2_min_luma_coding_block_size) ||
        s.pic_height_in_luma_samples % (1 << s.log2_min_luma_coding_block_size))
        throw HeifError("picture size not a multiple of MinCbSizeY");
}

// The slice segments of a picture: in order and covering it (7.4.7.1), and
// each with one entry point per tile / WPP row.  A dependent segment takes its
// slice's header values (7.4.7.1), copied in here.  The GPU path decodes
// several slices as one sub-picture per slice (batch.cpp), so every segment
// must start at a CTB row (a slice's dependent segments are concatenated);
// with HEVC tiles every segment must start at a tile (slices of whole tiles,
// each tile a sub-picture with its slice's values) and nothing is filtered
// across the tiles.  Loop filtering across the
// slices' boundaries is either off for all (independent sub-pictures) or on
// for all, with one set of deblocking values (sub-pictures of an assembly
// filtered whole).
void check_segments(TileJob &job, const ParamSet &ps) {
    for (size_t k = 1; k < job.segs.size(); ++k) {
        SliceSegmentHeader &sh = job.segs[k].sh;
        if (!sh.dependent_slice_segment_flag) continue;
        const SliceSegmentHeader &s = job.segs[k - 1].sh;  // (already inherited when dependent itself)
        sh.slice_type = s.slice_type;
        sh.slice_sao_luma_flag = s.slice_sao_luma_flag;
        sh.slice_sao_chroma_flag = s.slice_sao_chroma_flag;
        sh.slice_qp_delta = s.slice_qp_delta;
        sh.slice_cb_qp_offset = s.slice_cb_qp_offset;
        sh.slice_cr_qp_offset = s.slice_cr_qp_offset;
        sh.slice_deblocking_filter_disabled_flag = s.slice_deblocking_filter_disabled_flag;
        sh.slice_beta_offset_div2 = s.slice_beta_offset_div2;
        sh.slice_tc_offset_div2 = s.slice_tc_offset_div2;
        sh.slice_loop_filter_across_slices_enabled_flag = s.slice_loop_filter_across_slices_enabled_flag;
    }
    const SequenceParameterSet &sps = ps.sps;
    const PictureParameterSet &pps = ps.pps;
    const uint32_t pw = uint32_t(sps.pic_width_in_ctbs_y());
    for (size_t k = 0; k < job.segs.size(); ++k) {
        const SliceSegmentHeader &sh = job.segs[k].sh;
        if (sh.first_slice_segment_in_pic_flag != (k == 0)) throw HeifError("first_slice_segment_in_pic_flag out of order");
        if (k > 0 && sh.slice_segment_address <= job.segs[k - 1].sh.slice_segment_address)
            throw HeifError("slice segments out of order");
        if (k == 0) continue;
        if (pps.tiles_enabled_flag) {
            // slices of whole tiles (7.4.7.1 allows that or tiles of whole slices): each
            // tile decodes with its slice's header values; nothing may be filtered across
            const uint32_t x = sh.slice_segment_address % pw, y = sh.slice_segment_address / pw;
            const bool at_tile = std::find(ps.col_bd.begin(), ps.col_bd.end(), int(x)) != ps.col_bd.end() &&
                                 std::find(ps.row_bd.begin(), ps.row_bd.end(), int(y)) != ps.row_bd.end();
            if (!at_tile)
                throw UnsupportedError("several slice segments together with HEVC tiles (a segment starting inside a tile)");
            if (pps.loop_filter_across_tiles_enabled_flag)
                throw UnsupportedError("several slice segments together with HEVC tiles filtered across tiles");
            continue;
        }
        // a dependent segment inside a row continues its slice's substream there
        // (the row's, with WPP): the parse switches to its data (batch.cpp)
        if (sh.slice_segment_address % pw && !sh.dependent_slice_segment_flag)
            throw UnsupportedError("a slice segment starting inside a CTB row");
        if (sh.dependent_slice_segment_flag) continue;  // the loop-filter rules below are per slice
        size_t second = 1;  // the second slice
        while (job.segs[second].sh.dependent_slice_segment_flag) ++second;
        const SliceSegmentHeader &s1 = job.segs[second].sh;
        if (sh.slice_loop_filter_across_slices_enabled_flag != s1.slice_loop_filter_across_slices_enabled_flag)
            throw UnsupportedError("slices filtered across some slice boundaries only");
        const SliceSegmentHeader &s0 = job.segs[0].sh;
        if (s1.slice_loop_filter_across_slices_enabled_flag &&
            (sh.slice_deblocking_filter_disabled_flag != s0.slice_deblocking_filter_disabled_flag ||
             sh.slice_beta_offset_div2 != s0.slice_beta_offset_div2 ||
             sh.slice_tc_offset_div2 != s0.slice_tc_offset_div2))
            throw UnsupportedError("slices filtered across their boundaries with different deblocking values");
    }
    const size_t ntiles = (ps.col_bd.size() - 1) * (ps.row_bd.size() - 1);
    // tiles: one substream per tile, or with WPP one per CTB row of each tile
    const size_t nsub_tiles = pps.entropy_coding_sync_enabled_flag
                                  ? (ps.col_bd.size() - 1) * size_t(sps.pic_height_in_ctbs_y())
                                  : ntiles;
    size_t nsub_segs = 0;
    for (const SliceSeg &g : job.segs) nsub_segs += size_t(g.sh.num_entry_point_offsets) + 1;
    if (pps.tiles_enabled_flag && nsub_segs != nsub_tiles)
        throw HeifError("tiled picture without one entry point per tile (per tile row with WPP)");
    if (pps.entropy_coding_sync_enabled_flag && !pps.tiles_enabled_flag)
        for (size_t k = 0; k < job.segs.size(); ++k) {
            // the rows the segment's CTUs touch (it may start and end inside rows)
            const uint32_t r0 = job.segs[k].sh.slice_segment_address / pw;
            const uint32_t r1 = k + 1 < job.segs.size() ? (job.segs[k + 1].sh.slice_segment_address - 1) / pw + 1
                                                        : uint32_t(sps.pic_height_in_ctbs_y());
            if (uint32_t(job.segs[k].sh.num_entry_point_offsets) + 1 != r1 - r0)
                throw HeifError("WPP slice without one entry point per CTB row");
        }
}

}  // namespace

namespace {
// new[oy][ox] = cur[a * (ox, oy) + b]: composes the step behind the map so far
void display_step(DisplayMap &d, const int32_t a[4], const int32_t b[2], uint32_t w, uint32_t h) {
    const int32_t m[4] = {d.m[0] * a[0] + d.m[1] * a[2], d.m[0] * a[1] + d.m[1] * a[3],
                          d.m[2] * a[0] + d.m[3] * a[2], d.m[2] * a[1] + d.m[3] * a[3]};
    const int32_t t[2] = {d.m[0] * b[0] + d.m[1] * b[1] + d.t[0], d.m[2] * b[0] + d.m[3] * b[1] + d.t[1]};
    for (int k = 0; k < 4; ++k) d.m[k] = m[k];
    d.t[0] = t[0];
    d.t[1] = t[1];
    d.out_width = w;
    d.out_height = h;
    ++d.n_transforms;
}
int64_t floor_div(int64_t a, int64_t b) {  // b > 0
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}
}  // namespace

void display_clap(DisplayMap &d, const uint8_t *q, size_t len) {
    if (len < 32) throw HeifError("clap too short");
    int64_t f[8];
    for (int k = 0; k < 8; ++k) {
        const uint32_t v = (uint32_t(q[4 * k]) << 24) | (uint32_t(q[4 * k + 1]) << 16) | (uint32_t(q[4 * k + 2]) << 8) | q[4 * k + 3];
        // the offsets' numerators are signed; a denominator with the top bit set counts as negative
        f[k] = (k == 0 || k == 2) ? int64_t(v) : int64_t(int32_t(v));
    }
    for (int k = 1; k < 8; k += 2)
        if (f[k] <= 0) throw HeifError("clap: zero or negative denominator");
    const int64_t W = d.out_width, H = d.out_height;
    // round_half_up(n / d) = floor((2n + d) / 2d), exact in int64 (|n|, d < 2^32, W, H < 2^32)
    const int64_t cw = floor_div(2 * f[0] + f[1], 2 * f[1]), ch = floor_div(2 * f[2] + f[3], 2 * f[3]);
    if (cw < 1 || ch < 1) throw HeifError("clap: empty clean aperture");
    if (cw > W || ch > H) throw HeifError("clap: clean aperture outside the image");
    const int64_t left = floor_div(2 * f[4] + (W - cw) * f[5] + f[5], 2 * f[5]);
    const int64_t top = floor_div(2 * f[6] + (H - ch) * f[7] + f[7], 2 * f[7]);
    if (left < 0 || top < 0 || left + cw > W || top + ch > H) throw HeifError("clap: clean aperture outside the image");
    const int32_t a[4] = {1, 0, 0, 1}, b[2] = {int32_t(left), int32_t(top)};
    display_step(d, a, b, uint32_t(cw), uint32_t(ch));
}

void display_irot(DisplayMap &d, uint32_t quarter_turns) {
    const uint32_t n = d.n_transforms;
    for (uint32_t k = 0; k < (quarter_turns & 3); ++k) {
        // np.rot90(img)[oy][ox] = img[ox][W - 1 - oy]
        const int32_t a[4] = {0, -1, 1, 0}, b[2] = {int32_t(d.out_width) - 1, 0};
        display_step(d, a, b, d.out_height, d.out_width);
    }
    d.n_transforms = n + 1;  // one box, whatever its angle
}

void display_imir(DisplayMap &d, uint32_t axis) {
    if (axis & 1) {
        const int32_t a[4] = {1, 0, 0, -1}, b[2] = {0, int32_t(d.out_height) - 1};
        display_step(d, a, b, d.out_width, d.out_height);
    } else {
        const int32_t a[4] = {-1, 0, 0, 1}, b[2] = {int32_t(d.out_width) - 1, 0};
        display_step(d, a, b, d.out_width, d.out_height);
    }
}

void display_window(DisplayMap &d, uint32_t x, uint32_t y, uint32_t w, uint32_t h) {
    const int32_t a[4] = {1, 0, 0, 1}, b[2] = {int32_t(x), int32_t(y)};
    display_step(d, a, b, w, h);
}

ParsedImage parse_heic(const uint8_t *data, size_t len, uint32_t item_id) {
    HeifReader reader(data, len);
    Heif heif = reader.read();
    ParsedImage img;
    img.primary_item_id = heif.primary_item_id;
    img.item_id = item_id ? item_id : heif.primary_item_id;
    for (const auto &r : heif.references)  // 'auxl' from an auxiliary image to the primary
        if (r.type == fourcc('a', 'u', 'x', 'l') && !img.aux_item_id)
            for (uint32_t t : r.to)
                if (t == heif.primary_item_id) img.aux_item_id = r.from;
    const ItemInfo *pi = heif.item_info_by_item_id(img.item_id);
    if (!pi) throw HeifError("item " + std::to_string(img.item_id) + " not found in item_info");
    if (const Property *ispe = heif.item_property(*pi, fourcc('i', 's', 'p', 'e'))) {
        if (ispe->length < 12) throw HeifError("ispe too short");
        const uint8_t *q = data + ispe->offset + 4;
        img.ispe_width = (uint32_t(q[0]) << 24) | (uint32_t(q[1]) << 16) | (uint32_t(q[2]) << 8) | q[3];
        img.ispe_height = (uint32_t(q[4]) << 24) | (uint32_t(q[5]) << 16) | (uint32_t(q[6]) << 8) | q[7];
    }
    if (const Property *irot = heif.item_property(*pi, fourcc('i', 'r', 'o', 't')))
        if (irot->length >= 1) img.rotation = data[irot->offset] & 3;
    // colr of type nclx (ISO/IEC 23008-12 6.5.5; reader.rs:525 leaves it todo!()):
    // its matrix / range override the SPS VUI for RGB conversion.  An item may
    // carry both an ICC ('prof') and an nclx colr, so scan all of them.
    for (uint32_t idx : pi->properties) {
        if (idx == 0 || idx > heif.properties.size()) continue;
        const Property &p = heif.properties[idx - 1];
        // the light-level boxes of an HDR item (the first of each): their payloads, unread
        if (p.type == fourcc('c', 'l', 'l', 'i') && !img.color.has_clli) {
            img.color.has_clli = true;
            img.color.clli.assign(data + p.offset, data + p.offset + p.length);
        } else if (p.type == fourcc('m', 'd', 'c', 'v') && !img.color.has_mdcv) {
            img.color.has_mdcv = true;
            img.color.mdcv.assign(data + p.offset, data + p.offset + p.length);
        }
        if (p.type != fourcc('c', 'o', 'l', 'r') || p.length < 4) continue;
        const uint8_t *q = data + p.offset;
        const uint32_t kind = (uint32_t(q[0]) << 24) | (uint32_t(q[1]) << 16) | (uint32_t(q[2]) << 8) | q[3];
        if ((kind == fourcc('p', 'r', 'o', 'f') || kind == fourcc('r', 'I', 'C', 'C')) && !img.color.has_icc) {
            img.color.has_icc = true;  // the profile defines the colour space; its bytes are kept unread
            img.color.icc.assign(q + 4, q + p.length);
        }
        if (kind != fourcc('n', 'c', 'l', 'x') || p.length < 11) continue;
        img.nclx = true;
        img.nclx_matrix = (uint32_t(q[8]) << 8) | q[9];
        img.nclx_full_range = q[10] >> 7;
        img.color.has_nclx = true;
        img.color.primaries = (uint32_t(q[4]) << 8) | q[5];
        img.color.transfer = (uint32_t(q[6]) << 8) | q[7];
    }
    img.num_thumbnails = heif.num_thumbnails();

    std::vector<uint32_t> tile_ids;
    if (pi->type == fourcc('g', 'r', 'i', 'd')) {
        ImageGrid g = heif.grid(*pi);
        img.rows = g.rows;
        img.cols = g.cols;
        img.out_width = g.output_width;
        img.out_height = g.output_height;
        tile_ids = heif.references_from(fourcc('d', 'i', 'm', 'g'), pi->id);
        if (tile_ids.empty()) throw HeifError("grid " + std::to_string(pi->id) + " has no tile references");
        if (tile_ids.size() != size_t(g.rows) * g.cols) throw HeifError("grid tile count mismatch");
    } else if (pi->type == fourcc('h', 'v', 'c', '1')) {
        tile_ids.push_back(pi->id);
    } else {
        throw UnsupportedError("unsupported primary item type");
    }

    // one owned copy of every tile item's bytes; the tiles' payloads are views into it
    std::vector<const ItemInfo *> items;
    size_t coded_total = 0;
    for (uint32_t id : tile_ids) {
        const ItemInfo *it = heif.item_info_by_item_id(id);
        if (!it) throw HeifError("tile item " + std::to_string(id) + " not found");
        if (it->type != fourcc('h', 'v', 'c', '1')) throw UnsupportedError("grid tile is not hvc1");
        items.push_back(it);
        coded_total += heif.item_data(*it, nullptr);
    }
    img.coded.reserve(coded_total);
    std::vector<size_t> item_off;
    for (const ItemInfo *it : items) {
        item_off.push_back(img.coded.size());
        heif.item_data(*it, &img.coded);
    }
    item_off.push_back(img.coded.size());

    std::map<size_t, int> param_of_prop;  // hvcC property offset → params index
    for (size_t ti = 0; ti < items.size(); ++ti) {
        const ItemInfo *it = items[ti];
        const Property *hv = heif.item_property(*it, fourcc('h', 'v', 'c', 'C'));
        if (!hv) throw HeifError("missing HEVC decoder configuration");
        int param;
        auto found = param_of_prop.find(hv->offset);
        HevcConfig cfg = parse_hvcc(data + hv->offset, hv->length);
        if (found == param_of_prop.end()) {
            if (cfg.vps.empty()) throw HeifError("no VPS in hvcC");
            if (cfg.sps.empty()) throw HeifError("no SPS in hvcC");
            if (cfg.pps.empty()) throw HeifError("no PPS in hvcC");
            ParamSet ps;
            ps.key = cfg.sps[0];
            ps.key.insert(ps.key.end(), cfg.pps[0].begin(), cfg.pps[0].end());
            ps.vps = video_parameter_set_rbsp(nal_rbsp(cfg.vps[0]));
            ps.sps = sequence_parameter_set_rbsp(nal_rbsp(cfg.sps[0]));
            ps.pps = picture_parameter_set_rbsp(nal_rbsp(cfg.pps[0]), ps.sps);
            check_supported(ps.sps, ps.pps);
            tile_boundaries(ps.sps, ps.pps, ps.col_bd, ps.row_bd);
            param = int(img.params.size());
            img.params.push_back(std::move(ps));
            param_of_prop[hv->offset] = param;
        } else {
            param = found->second;
        }
        const ParamSet &ps = img.params[size_t(param)];
        // read_item_nal_unit (decoder.rs:146-164), generalised: length-prefixed NAL units,
        // the VCL ones are the picture's slice segments in order, non-VCL units skipped
        const uint8_t *item = img.coded.data() + item_off[ti];
        const size_t item_len = item_off[ti + 1] - item_off[ti];
        img.coded_bytes += uint32_t(item_len);
        int lsz = cfg.length_size_minus_one + 1;
        size_t pos = 0;
        TileJob job;
        job.param = param;
        while (pos < item_len) {
            if (pos + size_t(lsz) > item_len) throw HeifError("truncated NAL length prefix");
            size_t nl = 0;
            for (int k = 0; k < lsz; ++k) nl = (nl << 8) | item[pos + size_t(k)];
            pos += size_t(lsz);
            if (nl < 3 || nl > item_len - pos) throw HeifError("NAL unit length out of range");
            NalUnitHeader h{uint16_t((item[pos] << 8) | item[pos + 1])};
            if (h.nal_unit_type() < 32) {
                SliceSeg sg;
                sg.nal = h;
                sg.payload = item + pos + 2;
                sg.payload_len = nl - 2;
                sg.sh = slice_segment_header(sg.payload, sg.payload_len, sg.nal, ps.sps, ps.pps);
                job.segs.push_back(sg);
            }
            pos += nl;
        }
        if (job.segs.empty()) throw HeifError("tile item holds no VCL NAL unit");
        check_segments(job, ps);
        img.tiles.push_back(std::move(job));
    }
    const SequenceParameterSet &s0 = img.params[0].sps;
    img.tile_width = uint32_t(s0.out_width());
    img.tile_height = uint32_t(s0.out_height());
    for (auto &ps : img.params) {
        if (ps.sps.out_width() != s0.out_width() || ps.sps.out_height() != s0.out_height())
            throw UnsupportedError("grid tiles of different sizes");
        if (ps.sps.bit_depth_luma_minus8 != s0.bit_depth_luma_minus8 || ps.sps.chroma_format_idc != s0.chroma_format_idc)
            throw UnsupportedError("grid tiles with different formats");
        if (ps.sps.chroma_loc_present != s0.chroma_loc_present || ps.sps.chroma_loc_top != s0.chroma_loc_top)
            throw UnsupportedError("grid tiles with different formats");
    }
    if (pi->type != fourcc('g', 'r', 'i', 'd')) {
        img.out_width = img.tile_width;
        img.out_height = img.tile_height;
    }
    if (img.out_width > img.cols * img.tile_width || img.out_height > img.rows * img.tile_height)
        throw HeifError("grid output larger than its tiles");

    // display geometry: the transformative properties in the order ipma lists them
    // (ISO/IEC 23008-12 6.5: a reader applies them in that order), several of a kind allowed
    img.display.out_width = img.out_width;
    img.display.out_height = img.out_height;
    for (uint32_t idx : pi->properties) {
        if (idx == 0 || idx > heif.properties.size()) continue;
        const Property &p = heif.properties[idx - 1];
        if (p.type == fourcc('c', 'l', 'a', 'p')) display_clap(img.display, data + p.offset, p.length);
        else if (p.type == fourcc('i', 'r', 'o', 't') && p.length >= 1) display_irot(img.display, data[p.offset] & 3u);
        else if (p.type == fourcc('i', 'm', 'i', 'r') && p.length >= 1) display_imir(img.display, data[p.offset] & 1u);
    }
    // alpha: the first auxiliary image of this item whose auxC (FullBox, then the
    // zero-terminated aux_type URN) names an alpha plane; other auxiliaries are not alpha
    // (depth is passed over; a gain map is found further down)
    static const char *const kAlphaUrn[2] = {"urn:mpeg:hevc:2015:auxid:1", "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha"};
    for (const auto &r : heif.references) {
        if (r.type != fourcc('a', 'u', 'x', 'l') || img.alpha_item_id) continue;
        if (std::find(r.to.begin(), r.to.end(), img.item_id) == r.to.end()) continue;
        const ItemInfo *ai = heif.item_info_by_item_id(r.from);
        const Property *ac = ai ? heif.item_property(*ai, fourcc('a', 'u', 'x', 'C')) : nullptr;
        if (!ac || ac->length < 4) continue;
        const char *urn = reinterpret_cast<const char *>(data + ac->offset + 4);
        const size_t ulen = strnlen(urn, ac->length - 4);
        for (const char *want : kAlphaUrn)
            if (ulen == std::strlen(want) && std::memcmp(urn, want, ulen) == 0) img.alpha_item_id = r.from;
    }
    if (img.alpha_item_id)
        for (const auto &r : heif.references)
            if (r.type == fourcc('p', 'r', 'e', 'm') && r.from == img.item_id &&
                std::find(r.to.begin(), r.to.end(), img.alpha_item_id) != r.to.end())
                img.alpha_premultiplied = 1;
    // gain map: a 'tmap' item whose dimg lists [this item, the map] (its data kept unread; data
    // that cannot be fetched stays empty and is a parse error when a transform is asked for) ...
    for (const ItemInfo &it : heif.items) {
        if (it.type != fourcc('t', 'm', 'a', 'p') || img.gain.kind) continue;
        const std::vector<uint32_t> to = heif.references_from(fourcc('d', 'i', 'm', 'g'), it.id);
        if (to.size() < 2 || to[0] != img.item_id) continue;
        img.gain.kind = HEIFGPU_GAIN_ISO;
        img.gain.item_id = to[1];
        try {
            // (its fields are 62 or 142 bytes: an item above 64 KiB is not copied and reads as damaged)
            if (heif.item_data(it, nullptr) <= 65536) heif.item_data(it, &img.gain.tmap);
        } catch (const std::exception &) {
            img.gain.tmap.clear();
        }
    }
    // ... else the first auxiliary image of this item that Apple's URN names
    static const char kGainUrn[] = "urn:com:apple:photo:2020:aux:hdrgainmap";
    for (const auto &r : heif.references) {
        if (r.type != fourcc('a', 'u', 'x', 'l') || img.gain.kind) continue;
        if (std::find(r.to.begin(), r.to.end(), img.item_id) == r.to.end()) continue;
        const ItemInfo *ai = heif.item_info_by_item_id(r.from);
        const Property *ac = ai ? heif.item_property(*ai, fourcc('a', 'u', 'x', 'C')) : nullptr;
        if (!ac || ac->length < 4) continue;
        const char *urn = reinterpret_cast<const char *>(data + ac->offset + 4);
        const size_t ulen = strnlen(urn, ac->length - 4);
        if (ulen == sizeof(kGainUrn) - 1 && std::memcmp(urn, kGainUrn, ulen) == 0) {
            img.gain.kind = HEIFGPU_GAIN_APPLE;
            img.gain.item_id = r.from;
        }
    }
    return img;
}

}  // namespace hg
