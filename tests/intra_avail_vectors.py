"""Pictures of a few CTBs for k_intra's neighbour gather (tests/test_intra_avail_gpu.py).

The gather reads, per search position, the sample that stands there after the substitution of
8.4.4.2.2, from the record's five availability facts.  A wrong fact or a wrong source address
must show as a wrong sample, so every probe TB here has pairwise distinct values planted on all
its neighbours: the probes are chosen, in decoding order, so that no probe covers a neighbour of
another and no two probes share a neighbour, every other TB is PCM (its reconstruction is what
was planted), and intra_vectors.plant_distinct() writes the values.

Pictures: 72 x 40 with CTB 32, 40 x 24 with CTB 16 and 136 x 72 with CTB 64, each with a
remainder of 8 luma samples on both edges, under quadtrees of one TB size and a random one.
A remainder of 8 is one minimum coding block: it removes a group of neighbours whole, never
part-way, and none of the three has a whole 64 CTB below the first CTB row.  168 x 168 with CTB 64
is added for both: its CTU (1, 1) has every neighbour (a 32x32 TB with full below-left and
above-right groups), and its last CTB is 40 x 40, so a 32x32 TB there and the 16x16 TBs beside it
have 8 of their below-left and above-right samples inside the picture (4 of a 16x16 or 8x8 chroma
TB's).
"""
import functools

import numpy as np

import intra_ref as ref
from intra_vectors import Batch, Case, Pic, plant_distinct, random_tree, tile, uniform
from xform_vectors import hash_str

GEOMS = ((72, 40, 5), (40, 24, 4), (136, 72, 6), (168, 168, 6))  # W, H, log2 CTB
KINDS = ("u2", "u3", "u4", "u5", "rnd", "rnd2")


def _neighbours(g, t):
    n = 1 << t.log2
    w, h = g.plane(t.cidx)
    return [(t.x + dx, t.y + dy) for dx, dy in ref.search_positions(n) if 0 <= t.x + dx < w and 0 <= t.y + dy < h]


def choose_probes(g, split, first=None, turn=0):
    """Keys (class, x, y, log2) of the probe TBs: every TB that can be one, taken in decoding order
    (Cr follows its Cb TB, so that pairs stay pairs).  first = (row, column): the TBs of that CTU
    get their pick before the others, beginning with its TB number `turn` of each component class,
    which moves the choice inside the CTU."""
    tbs = [t for row in tile(g, split) for t in row if t.cidx < 2]
    if first is not None:
        ctb = 1 << g.log2_ctb
        mine = [t for t in tbs if (t.tu[1] // ctb, t.tu[0] // ctb) == first]
        head = []
        for k in (0, 1):
            of_k = [t for t in mine if t.cidx == k]
            head += of_k[turn % max(len(of_k), 1):] + of_k[:turn % max(len(of_k), 1)]
        tbs = head + [t for t in tbs if not any(t is m for m in mine)]
    taken = [np.zeros(g.plane(k)[::-1], dtype=bool) for k in range(min(g.ncomp, 2))]   # the probes' samples
    needed = [np.zeros(g.plane(k)[::-1], dtype=bool) for k in range(min(g.ncomp, 2))]  # the probes' neighbours
    keys = set()
    for t in tbs:
        n, k = 1 << t.log2, t.cidx
        nb = _neighbours(g, t)
        if needed[k][t.y:t.y + n, t.x:t.x + n].any() or any(taken[k][y, x] or needed[k][y, x] for x, y in nb):
            continue
        keys.add((k, t.x, t.y, t.log2))
        taken[k][t.y:t.y + n, t.x:t.x + n] = True
        for x, y in nb:
            needed[k][y, x] = True
    return keys


def probe_pic(name, g, split, first=None, turn=0):
    keys = choose_probes(g, split, first, turn)
    probes = []

    def style(t):
        n = 1 << t.log2
        t.pcm = (min(t.cidx, 1), t.x, t.y, t.log2) not in keys
        if not t.pcm:
            t.tag = f"c{t.cidx}n{n}@{t.x},{t.y}"
            probes.append(t)

    def plant(pic):
        plant_distinct(pic, probes, np.random.default_rng(hash_str(name + "/plant")))

    return Pic(name, g, split, style, plant)


def _pics(cf, bd, tag, geoms=GEOMS, kinds=KINDS):
    pics = []
    for W, H, log2ctb in geoms:
        ctb = 1 << log2ctb
        for kind in kinds:
            if kind[0] == "u" and int(kind[1]) > log2ctb:
                continue
            name = f"{tag}/{W}x{H}/ctb{ctb}/{kind}"
            split = random_tree(name) if kind[0] == "r" else uniform(int(kind[1]))
            min_tb = 2 if kind in ("u2", "rnd", "rnd2") else 3
            g = ref.Geom(W, H, cf, bd, bd, log2ctb, min_tb)
            pics.append(probe_pic(name, g, split))
            if (W, H) == GEOMS[-1][:2] and kind in ("u3", "u4", "u5"):
                # the added picture: its CTU (1, 1) has every neighbour, its last CTU is cut by both edges
                for first in ((1, 1), ((H - 1) // ctb, (W - 1) // ctb)):
                    for turn in range(4):
                        pics.append(probe_pic(f"{name}/r{first[0]}c{first[1]}t{turn}", g, split, first, turn))
    return pics


def case_420():
    return Case("avail420", [Batch(_pics(1, 8, "avail/420"))])


def case_422():
    return Case("avail422", [Batch(_pics(2, 10, "avail/422", geoms=GEOMS[:3], kinds=("rnd",)))])


def case_444():
    return Case("avail444", [Batch(_pics(3, 10, "avail/444", geoms=GEOMS[:3], kinds=("rnd",)))])


CASES = {"avail420": case_420, "avail422": case_422, "avail444": case_444}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once (its expectation stays as computed)."""
    return CASES[name]()


def arms(avail, n):
    """What a TB's availability asks of the gather."""
    a = np.asarray(avail, dtype=bool)
    bl, left, above, ar = a[0:n], a[n:2 * n], a[2 * n + 1:3 * n + 1], a[3 * n + 1:4 * n + 1]
    out = set()
    if not a.any():
        out.add("nothing")
    if a.any() and not a[0]:
        out.add("forward_fill")  # the first search position takes a later one's sample
    if not left.any() and above.all():
        out.add("left_missing")
    if bl.all() and ar.all():
        out.add("full_bl_ar")
    if 0 < bl.sum() < n:
        out.add("part_bl")
    if 0 < ar.sum() < n:
        out.add("part_ar")
    return out
