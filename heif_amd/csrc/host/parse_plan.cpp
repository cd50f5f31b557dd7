// parse_plan.cpp — the host's choices for the CABAC parse of a batch: the
// parse mode, the lanes parse's tool set and pictures per wave, and the
// dealing of pictures (lanes, solo) or substreams (spread) to wave slots.
// Declared in kernels/kernels.hpp; the kernels are kernels/parse_*.hip.
#include "../kernels/kernels.hpp"

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace hg {

// pictures per wave: a picture's lanes (BatchArgs::lane_rows) are consecutive.
// A wave's time is its pictures' WPP chains times the cost of a pass, and a
// pass costs more with more pictures' lanes in it (more unit kinds and longer
// divergent loops), so a batch that cannot fill every SIMD takes the fewest
// pictures per wave that still fit one wave per SIMD (single 4032x3024
// image on MI355X: parse 85 -> 66 ms at 1 picture per wave instead of 4);
// a full batch packs 64 lanes (config 4: 1536 waves).  HEIFGPU_LANES_PPW
// forces a value (tuning); HEIFGPU_PARSE_ADAPT=0 always packs.
static int lanes_simds() {
    static const int simds = [] {
        const char *e = std::getenv("HEIFGPU_PARSE_SIMDS");
        if (e) return std::atoi(e);
#if !defined(HG_HOST_EMU)
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            return 4 * cus;
#endif
        return 1024;
    }();
    return simds;
}
int lanes_pics_per_wave(int lane_rows, int n_pics) {
    static const int forced = [] {
        const char *e = std::getenv("HEIFGPU_LANES_PPW");
        return e ? std::atoi(e) : 0;
    }();
    static const bool adapt = [] {
        const char *e = std::getenv("HEIFGPU_PARSE_ADAPT");
        return !e || std::atoi(e) != 0;
    }();
    const int full = 64 / (lane_rows < 1 ? 1 : (lane_rows > 64 ? 64 : lane_rows));
    if (forced > 0) return forced < full ? forced : full;
    if (adapt && n_pics > 0) {
        const long S = lanes_simds();
        for (int p = 1; p < full; ++p)
            if ((n_pics + p - 1) / p <= S) return p;
        // No packing fits one wave per SIMD: the fewest pictures per wave that
        // fit two per SIMD (k_parse_lanes' VGPRs allow two), so no SIMD holds
        // two waves while others hold one.  Config 4 (6144 pictures): 3 per
        // wave, 2048 waves; r04 A/B: parse alone 70.3 -> 64.6 ms, beside the
        // reconstruction 78.4 -> 73.4, step 85.9 -> 85.4 ms.
        for (int p = 1; p < full; ++p)
            if ((n_pics + p - 1) / p <= 2 * S) return p;
    }
    return full;
}

// Wave slot -> picture.  A wave runs until its heaviest picture is parsed,
// and every extra busy picture in it adds divergent units to each pass, so
// the critical path is the wave holding the most work.  Pictures are sorted
// by payload size and dealt snake-wise (wave w of W gets ranks w, 2W-1-w,
// 2W+w, 4W-1-w, ...): heavy beside light.  Empty slots are ~0u.
// HEIFGPU_PARSE_ORDER=0: batch order (kept for the emulation test of an
// unsorted dealing).  (r06 A/B, DESIGN 5.13: dealing by WPP critical path, or
// the lightest pictures beside each wave's heaviest, won only where a wave's
// companions repeat one bitstream, on the permuted halfmoonbay shard; on
// distinct tiles both were neutral or worse, so snake dealing stays.  The
// dispatcher puts waves w and w + W/2 on one SIMD; pairing the heaviest wave
// with the lightest moved nothing, and the heaviest pictures two per wave (the
// rest four) lost 7.7 %: a wave's time is its heaviest picture's chain.)
int lanes_parse_order(const PicDesc *pics, int n, int lane_rows, int ppw_force, std::vector<uint32_t> &order) {
    static const int on = [] {
        const char *e = std::getenv("HEIFGPU_PARSE_ORDER");
        return e ? std::atoi(e) : 1;
    }();
    const int full = 64 / (lane_rows < 1 ? 1 : (lane_rows > 64 ? 64 : lane_rows));
    const int ppw = ppw_force > 0 ? std::min(ppw_force, full) : lanes_pics_per_wave(lane_rows, n);
    if (!on || n <= 0) {
        order.resize((size_t)n);
        for (int i = 0; i < n; ++i) order[(size_t)i] = (uint32_t)i;
        order.resize((size_t)((n + ppw - 1) / ppw) * ppw, ~0u);
        return ppw;
    }
    std::vector<uint32_t> by_size;  // assembly pictures have nothing to parse: no slot
    for (int i = 0; i < n; ++i)
        if (!(pics[i].flags & PD_ASSEMBLY)) by_size.push_back((uint32_t)i);
    n = (int)by_size.size();
    std::stable_sort(by_size.begin(), by_size.end(),
                     [&](uint32_t x, uint32_t y) { return pics[x].bits_len > pics[y].bits_len; });
    const int W = (n + ppw - 1) / ppw;
    order.assign((size_t)W * ppw, ~0u);
    for (int r = 0; r < n; ++r) {
        const int band = r / W, pos = r % W;
        const int w = (band & 1) ? W - 1 - pos : pos;
        order[(size_t)w * ppw + band] = by_size[(size_t)r];
    }
    return ppw;
}

// Parse mode of a batch.  Spread mode parses each substream on a wave of its
// own (every lane alike, so one syntax unit at a time with nothing else in
// the pass), one workgroup per substream so a picture's rows spread over CUs:
// far faster per substream than a lane of a packed wave, but 64 lanes do one
// substream's work, so it is the latency path of small and middle batches,
// where packed waves cannot fill the SIMDs anyway.  MI355X, halfmoonbay
// permutations, row-major spread against lanes (profiles/r06/ab/ab_mid.txt,
// Mpix/s): 4 images 1,677 / 910, 16 4,711 / 2,864, 32 6,787 / 6,174, 64 7,819
// / 11,135; distinct tiles at 32 images 7,683 / 7,768.  So batches up to 1536
// pictures (32 such images) take spread mode.  HEIFGPU_PARSE=lanes|solo|spread
// forces a mode for every batch, HEIFGPU_SOLO_MAX_PICS moves the switch-over.
int parse_mode_for(int requested, int n_pics, const PicDesc *pics) {
    if (pics)
        for (int i = 0; i < n_pics; ++i)
            if (pics[i].flags >> PD_NMID_SHIFT) return PARSE_LANES;
    static const int env = [] {
        const char *e = std::getenv("HEIFGPU_PARSE");
        if (!e) return PARSE_AUTO;
        const std::string v(e);
        return v == "solo"     ? PARSE_SOLO
               : v == "spread" ? PARSE_SPREAD
               : v == "lanes"  ? PARSE_LANES
                               : PARSE_AUTO;
    }();
    static const int max_pics = [] {
        const char *e = std::getenv("HEIFGPU_SOLO_MAX_PICS");
        return e ? std::atoi(e) : 1536;
    }();
    if (env != PARSE_AUTO) return env;
    if (requested == PARSE_LANES || requested == PARSE_SOLO || requested == PARSE_SPREAD)
        return requested;
    return n_pics <= max_pics ? PARSE_SPREAD : PARSE_LANES;
}

// The lanes parse's body for a batch (BatchArgs::lanes_lean): the lean tool
// set (EngT) when every picture with coded data is inside it, else the general
// one; one launch either way.  HEIFGPU_LANES_VARIANT=general (read at every
// prepare) keeps the general body for every batch (A/B, tests); auto or unset: this choice.
bool lanes_lean_eligible(const SeqParams *seqs, const PicDesc *pics, int n_pics, int wpp_ring) {
    if (wpp_ring) return false;
    for (int i = 0; i < n_pics; ++i) {
        if (pics[i].flags & PD_ASSEMBLY) continue;  // no coded data of its own
        const SeqParams &sp = seqs[pics[i].seq];
        if (sp.chroma_format != 1) return false;
        if (sp.flags & (SP_PCM | SP_TRANSFORM_SKIP | SP_TQ_BYPASS | SP_ROW_SEGMENTS)) return false;
        if (pics[i].flags >> PD_NMID_SHIFT) return false;  // dependent segments starting inside rows
    }
    return true;
}
int lanes_variant_for(const SeqParams *seqs, const PicDesc *pics, int n_pics, int wpp_ring) {
    const char *e = std::getenv("HEIFGPU_LANES_VARIANT");
    if (e && std::string(e) == "general") return LANES_GENERAL;
    return lanes_lean_eligible(seqs, pics, n_pics, wpp_ring) ? LANES_LEAN : LANES_GENERAL;
}

// waves per solo workgroup: one per WPP row of the tallest picture, at most 16
// (1024 threads); taller pictures wrap their rows round the waves
int solo_waves_for(int lane_rows) { return lane_rows < 1 ? 1 : (lane_rows > kSoloMaxWaves ? kSoloMaxWaves : lane_rows); }

// spread mode: one wave slot per substream, entry row << 20 | picture, in
// row-major order: row r of every picture (heaviest picture first) before row
// r + 1 of any.  A row's wave holds its slot (and its SIMD residency) from the
// dequeue until the row is parsed; picture-major order (a picture's rows in
// consecutive slots) filled the resident waves with rows waiting on the WPP
// ramp of their own picture, row-major order finds the row above long started.
// r06 A/B: 16 images 3,474 -> 4,711 Mpix/s, 32 images 3,847 ->
// 6,787 (distinct tiles: 3,709 -> 6,651 and 3,994 -> 7,683), one image equal.
// A row's predecessor keeps a lower slot, held by a running wave
// (k_parse_solo<true> takes its slot from the job counter).
int spread_parse_order(const PicDesc *pics, int n, std::vector<uint32_t> &order) {
    std::vector<uint32_t> by_size((size_t)n);
    for (int i = 0; i < n; ++i) by_size[(size_t)i] = (uint32_t)i;
    std::stable_sort(by_size.begin(), by_size.end(),
                     [&](uint32_t x, uint32_t y) { return pics[x].bits_len > pics[y].bits_len; });
    order.clear();
    uint32_t max_sub = 0;
    for (uint32_t p : by_size) {
        if (p >= (1u << 20) || pics[p].n_sub >= (1u << 12)) return -1;
        max_sub = std::max(max_sub, pics[p].n_sub);
    }
    for (uint32_t r = 0; r < max_sub; ++r)
        for (uint32_t p : by_size)
            if (r < pics[p].n_sub) order.push_back(p | (r << 20));
    return 1;
}

}  // namespace hg
