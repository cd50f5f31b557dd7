// resample.cpp — kernels/resample.hpp run on the host (no device, no HIP).
#include "resample.hpp"

#include <vector>

namespace hg {

bool resample_axis_ok(int64_t in_size, int64_t in0, int64_t in1, int64_t out, int64_t filter, int64_t bits) {
    return in_size >= 1 && in_size <= 65535 && in0 >= 0 && in0 < in1 && in1 <= in_size && out >= 1 && out <= 65535 &&
           (filter == RS_BILINEAR || filter == RS_BICUBIC) && bits >= 8 && bits <= 12;
}

namespace {

// the taps of one output: first sample and the integer coefficients
struct Row {
    int lo = 0;
    std::vector<int32_t> k;
};

void row_of(const RsAxis &a, int X, int P, Row &r) {
    int lo, hi;
    rs_bounds(a, X, lo, hi);
    const double center = rs_center(a, X);
    const double ww = rs_weight_sum(a, center, lo, hi);
    r.lo = lo;
    r.k.resize(size_t(hi > lo ? hi - lo : 0));
    for (int at = lo; at < hi; ++at) r.k[size_t(at - lo)] = rs_coeff(rs_weight(a, center, at), ww, P);
}

template <class T>
void apply(const T *in, int in_w, int ch, int maxv, int P, const RsAxis &ax, const RsAxis &ay, T *out) {
    const int ow = ax.out, oh = ay.out;
    int y0, y1, lo, hi;
    rs_bounds(ay, 0, y0, hi);
    rs_bounds(ay, oh - 1, lo, y1);
    // horizontal: rows [y0, y1) of the side, every output column
    std::vector<T> mid(size_t(y1 - y0) * size_t(ow) * size_t(ch));
    Row r;
    for (int X = 0; X < ow; ++X) {
        row_of(ax, X, P, r);
        for (int y = y0; y < y1; ++y)
            for (int c = 0; c < ch; ++c) {
                int32_t acc = rs_half(P);
                const T *src = in + (size_t(y) * size_t(in_w) + size_t(r.lo)) * size_t(ch) + size_t(c);
                for (size_t t = 0; t < r.k.size(); ++t) acc += r.k[t] * int32_t(src[t * size_t(ch)]);
                mid[(size_t(y - y0) * size_t(ow) + size_t(X)) * size_t(ch) + size_t(c)] = T(rs_round(acc, P, maxv));
            }
    }
    // vertical, over the rounded and clipped intermediate
    for (int Y = 0; Y < oh; ++Y) {
        row_of(ay, Y, P, r);
        for (int X = 0; X < ow; ++X)
            for (int c = 0; c < ch; ++c) {
                int32_t acc = rs_half(P);
                for (size_t t = 0; t < r.k.size(); ++t)
                    acc += r.k[t] * int32_t(mid[(size_t(r.lo - y0 + int(t)) * size_t(ow) + size_t(X)) * size_t(ch) + size_t(c)]);
                out[(size_t(Y) * size_t(ow) + size_t(X)) * size_t(ch) + size_t(c)] = T(rs_round(acc, P, maxv));
            }
    }
}

}  // namespace

int resample_coeffs(int in_size, int in0, int in1, int out, int filter, int bits, int32_t *bounds, int32_t *kk) {
    const RsAxis a = rs_axis(in_size, in0, in1, out, filter);
    const int P = rs_precision(bits);
    if (!bounds && !kk) return a.ksize;
    Row r;
    for (int X = 0; X < out; ++X) {
        row_of(a, X, P, r);
        if (bounds) {
            bounds[2 * size_t(X)] = r.lo;
            bounds[2 * size_t(X) + 1] = int32_t(r.k.size());
        }
        if (kk)
            for (int t = 0; t < a.ksize; ++t) kk[size_t(X) * size_t(a.ksize) + size_t(t)] = size_t(t) < r.k.size() ? r.k[size_t(t)] : 0;
    }
    return a.ksize;
}

void resample_apply(const void *in, int bps, int in_w, int in_h, int ch, int bits, int wx, int wy, int ww, int wh,
                    int ow, int oh, int filter, void *out) {
    const RsAxis ax = rs_axis(in_w, wx, wx + ww, ow, filter), ay = rs_axis(in_h, wy, wy + wh, oh, filter);
    const int P = rs_precision(bits), maxv = (1 << bits) - 1;
    if (bps == 1) apply(static_cast<const uint8_t *>(in), in_w, ch, maxv, P, ax, ay, static_cast<uint8_t *>(out));
    else apply(static_cast<const uint16_t *>(in), in_w, ch, maxv, P, ax, ay, static_cast<uint16_t *>(out));
}

}  // namespace hg
