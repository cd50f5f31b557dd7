"""A numpy model of the baseline JPEG encoder, written from the prose at the head of
heif_amd/csrc/kernels/jpeg.hpp (not from the kernels): colour conversion, padding,
subsampling, the integer DCT, quantisation, zigzag, DC prediction, Huffman coding,
stuffing, restart intervals and the headers.  encode() returns the file's bytes."""
import numpy as np

# Annex K.1 / K.2 in natural order, and K.3's BITS / HUFFVAL (tests/test_jpeg.py pins all of
# them to what Pillow writes)
BASE_Q = (
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32,
)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    list(bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435"
        "363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798"
        "999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4"
        "f5f6f7f8f9fa")),
    list(bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a2627"
        "28292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a8283848586878889"
        "8a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6"
        "e7e8e9eaf2f3f4f5f6f7f8f9fa")),
)
ICC_CHUNK = 65519


def zigzag():
    """Natural index of scan position k: the anti-diagonals of the block, alternating direction."""
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]  # y ascending: down-left
        if s % 2 == 0:
            cells.reverse()                                       # even diagonals run up-right
        order += [y * 8 + x for y, x in cells]
    return np.array(order)


ZIGZAG = zigzag()


def dct_matrix():
    u, x = np.mgrid[0:8, 0:8]
    c = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    return np.rint(16384 * c * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


T = dct_matrix()


def quant_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((np.array(b) * s + 50) // 100, 1, 255) for b in BASE_Q]


def huff_codes(bits, vals):
    """symbol -> (code, length), as C.2 derives them."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [huff_codes(b, v) for b, v in zip(DC_BITS, DC_VALS)]
AC_CODES = [huff_codes(b, v) for b, v in zip(AC_BITS, AC_VALS)]


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    return y, cb, cr


def fdct(p):
    """(..., 8, 8) samples minus 128 -> Q20 coefficients [v][u]."""
    # (float64 products and sums of these integers are exact: every partial sum is below 2^53)
    tf = T.astype(np.float64)
    rows = ((np.asarray(p, np.float64) @ tf.T).astype(np.int64) + 128) >> 8   # [y][u] = sum_x T[u][x] p[y][x]
    out = (tf @ rows.astype(np.float64)).astype(np.int64)                      # [v][u] = sum_y T[v][y] r[y][u]
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out


def quantise(c, t):
    t = t.reshape(8, 8).astype(np.int64)
    return np.sign(c) * ((np.abs(c) + (t << 19)) // (t << 20))


def blocks_of(plane):
    """(H, W) -> (H/8, W/8, 8, 8)."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def coefficients(rgb, quality, subsampling):
    """The quantised blocks of every MCU in scan order: (mcus, blocks per MCU, 64) in zigzag
    order, the component of each of an MCU's blocks, and the MCUs per row."""
    h, w, _ = rgb.shape
    mcu = 16 if subsampling == "4:2:0" else 8
    ph, pw = -(-h // mcu) * mcu, -(-w // mcu) * mcu
    ext = np.pad(rgb, ((0, ph - h), (0, pw - w), (0, 0)), mode="edge")
    y, cb, cr = ycc(ext)
    if subsampling == "4:2:0":
        cb, cr = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in (cb, cr))
    qt = quant_tables(quality)
    q = [quantise(fdct(blocks_of(pl - 128)), qt[1 if i else 0]).reshape(pl.shape[0] // 8, pl.shape[1] // 8, 64)[..., ZIGZAG]
         for i, pl in enumerate((y, cb, cr))]
    my, mx = ph // mcu, pw // mcu
    if subsampling == "4:2:0":
        yb = q[0].reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        per = np.concatenate([yb, q[1][:, :, None], q[2][:, :, None]], axis=2)
        comps = [0, 0, 0, 0, 1, 2]
    else:
        per = np.stack(q, axis=2)
        comps = [0, 1, 2]
    return per.reshape(my * mx, len(comps), 64), comps, mx


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.stuffed = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def value(self, table, run, v):
        n = int(abs(v)).bit_length()
        self.put(*table[run << 4 | n])
        if n:
            self.put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)


def scan(rgb, quality, subsampling, restart_mcus, stats=None):
    """The scan and EOI.  stats (a dict) receives what the case list's coverage asserts."""
    per, comps, mx = coefficients(rgb, quality, subsampling)
    ri = restart_mcus or mx
    out = bytearray()
    st = dict(zrl=0, no_eob=0, ac_zero=0, dc_cat=0, ac_cat=0, stuffed=0, aligned=0, intervals=0)
    n_int = -(-len(per) // ri)
    for i in range(n_int):
        bw = BitWriter()
        pred = [0, 0, 0]
        for m in range(i * ri, min((i + 1) * ri, len(per))):
            for j, comp in enumerate(comps):
                c = [int(v) for v in per[m, j]]
                tab = 1 if comp else 0
                d = c[0] - pred[comp]
                pred[comp] = c[0]
                st["dc_cat"] = max(st["dc_cat"], abs(d).bit_length())
                bw.value(DC_CODES[tab], 0, d)
                run = 0
                for v in c[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bw.put(*AC_CODES[tab][0xF0])
                        run -= 16
                        st["zrl"] += 1
                    st["ac_cat"] = max(st["ac_cat"], abs(v).bit_length())
                    bw.value(AC_CODES[tab], run, v)
                    run = 0
                if run:
                    bw.put(*AC_CODES[tab][0x00])
                else:
                    st["no_eob"] += 1
                st["ac_zero"] += not any(c[1:])
        if bw.n:
            bw.put((1 << (8 - bw.n)) - 1, 8 - bw.n)
        else:
            st["aligned"] += 1
        st["stuffed"] += bw.stuffed
        out += bw.out
        out += bytes([0xFF, 0xD0 + (i & 7) if i + 1 < n_int else 0xD9])
    st["intervals"] = n_int
    if stats is not None:
        stats.update(st)
    return bytes(out)


def scan_fast(rgb, quality, subsampling, restart_mcus):
    """scan() without its statistics, vectorised for large pictures: every code word of the scan
    as a (bits, length) token, sorted into scan order, expanded to bits and packed
    (tests/test_jpeg.py holds it equal to scan() on every case)."""
    per, comps, mx = coefficients(rgb, quality, subsampling)
    nm, bpm, _ = per.shape
    ri = restart_mcus or mx
    c = per.reshape(nm * bpm, 64).astype(np.int64)
    nb = len(c)
    comp = np.tile(np.array(comps), nm)
    interval = np.repeat(np.arange(nm), bpm) // ri
    tab = (comp > 0).astype(np.int64)
    n_int = -(-nm // ri)
    bitlen = np.array([v.bit_length() for v in range(2048)])
    lut = lambda codes: np.array([[codes[t].get(s, (0, 0)) for s in range(256)] for t in range(2)], dtype=np.int64)
    dc_lut, ac_lut = lut(DC_CODES), lut(AC_CODES)

    def token(table, t, run, v):
        n = bitlen[np.abs(v)]
        code, length = table[t, run << 4 | n, 0], table[t, run << 4 | n, 1]
        return code << n | (np.where(v < 0, v - 1, v) & ((1 << n) - 1)), length + n

    diff = np.empty(nb, np.int64)
    for k in range(3):
        idx = np.flatnonzero(comp == k)
        prev = np.concatenate([[0], c[idx[:-1], 0]])
        prev[np.concatenate([[True], interval[idx[1:]] != interval[idx[:-1]]])] = 0
        diff[idx] = c[idx, 0] - prev
    blocks = np.arange(nb)
    keys, vals, lens = [blocks * 260 + 3], *([x] for x in token(dc_lut, tab, 0, diff))
    b, k = np.nonzero(c[:, 1:])
    k = k + 1
    v = c[b, k]
    prev = np.concatenate([[0], k[:-1]])
    prev[np.concatenate([[True], b[1:] != b[:-1]])] = 0
    run = k - prev - 1
    tv, tl = token(ac_lut, tab[b], run & 15, v)
    keys.append(b * 260 + k * 4 + 3), vals.append(tv), lens.append(tl)
    zb, zk = np.repeat(b, run >> 4), np.repeat(k, run >> 4)
    keys.append(zb * 260 + zk * 4), vals.append(ac_lut[tab[zb], 0xF0, 0]), lens.append(ac_lut[tab[zb], 0xF0, 1])
    eb = np.flatnonzero(c[:, 63] == 0)
    keys.append(eb * 260 + 256), vals.append(ac_lut[tab[eb], 0, 0]), lens.append(ac_lut[tab[eb], 0, 1])
    keys, vals, lens = (np.concatenate(x) for x in (keys, vals, lens))
    order = np.argsort(keys, kind="stable")
    vals, lens, tok_int = vals[order], lens[order], interval[keys[order] // 260]
    int_bits = np.bincount(tok_int, weights=lens, minlength=n_int).astype(np.int64)
    pad = -int_bits % 8
    # the padding as one more token behind each interval's last
    last = np.cumsum(np.bincount(tok_int, minlength=n_int))
    vals, lens = np.insert(vals, last, (1 << pad) - 1), np.insert(lens, last, pad)
    starts = np.cumsum(lens) - lens
    rep = np.repeat(np.arange(len(lens), dtype=np.int32), lens)
    pos = np.arange(int(lens.sum()), dtype=np.int64) - starts[rep]
    packed = np.packbits(((vals[rep] >> (lens[rep] - 1 - pos)) & 1).astype(np.uint8)).tobytes()
    ends = np.cumsum(int_bits + pad) // 8
    out = bytearray()
    for i in range(n_int):
        out += packed[(ends[i - 1] if i else 0):ends[i]].replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + (i & 7) if i + 1 < n_int else 0xD9])
    return bytes(out)


def segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(w, h, quality, subsampling, restart_mcus=0, icc=None):
    out = b"\xff\xd8" + segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    icc = icc or b""
    chunks = [icc[i:i + ICC_CHUNK] for i in range(0, len(icc), ICC_CHUNK)]
    for k, ch in enumerate(chunks):
        out += segment(0xE2, b"ICC_PROFILE\0" + bytes([k + 1, len(chunks)]) + ch)
    for t, q in enumerate(quant_tables(quality)):
        out += segment(0xDB, bytes([t]) + bytes(int(v) for v in q[ZIGZAG]))
    out += segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes(
        [3, 1, 0x22 if subsampling == "4:2:0" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in range(2):
        out += segment(0xC4, bytes([t] + DC_BITS[t] + DC_VALS[t]))
        out += segment(0xC4, bytes([0x10 | t] + AC_BITS[t] + AC_VALS[t]))
    mcu = 16 if subsampling == "4:2:0" else 8
    out += segment(0xDD, (restart_mcus or -(-w // mcu)).to_bytes(2, "big"))
    out += segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(rgb, quality=90, subsampling="4:2:0", restart_mcus=0, icc=None, stats=None, fast=False):
    rgb = np.asarray(rgb)
    h, w, _ = rgb.shape
    body = scan_fast(rgb, quality, subsampling, restart_mcus) if fast else scan(rgb, quality, subsampling, restart_mcus, stats)
    return header(w, h, quality, subsampling, restart_mcus, icc) + body
