"""Inputs of the trainer's feature-response tests (tests/test_training_features.py): frames and proposals that put the
depth probes of csrc/tree_train_hip.hip on the edges of its staged tiles and of the image, its numerators on both sides of
the ranges its divide paths are verified for, and its thresholds on the values the response takes.  Seeded numpy
builders that the CPU tests (do the cases bite?) and the GPU tests (every entry point against oracle/train_numpy.py) both
call, so that both see the same arrays.

The kernels' geometry, restated: a workgroup takes a 32 x 8 tile of pixels (TILE_W, TILE_H); k_train_histogram stages it
with 16 cells around it (HALO_HIST), k_train_bits with 32 (HALO_BITS).  A probe inside the staged cells is answered by
LDS, any other one by global memory after a bounds check.

`response` below is a COPY of tn.compute_feature, vectorised over the proposals, that also returns where the probes land
and that takes a `mutant`: one wrong reading of the operation a kernel could make.  The CPU tests check that without a
mutant it is tn.compute_feature bit for bit, and that every mutant changes the decisions of the case built against it.
The GPU tests never use it for an expected value: those come from train_numpy alone."""
import functools
from typing import NamedTuple

import numpy as np

from oracle import train_numpy as tn

F32 = np.float32
TILE_W, TILE_H = 32, 8
HALO_HIST, HALO_BITS = 16, 32
N_IMG, H, W = 2, 77, 150             # no multiple of the tile; far probes of an interior tile stay in the image on all sides
C, LEVEL = 3, 2                      # four nodes
WINDOWS = ((0, 8, 8), (2, 6, 4))     # (start, end, NB) over the 8 children: all of them, and those of nodes 1 and 2
DEPTHS = (1, 2, 3, 4, 6, 12)         # of the live pixels: a numerator 12 k is a whole offset at every one of them
LCM = 12
DENORM_MIN = np.array([1], np.uint32).view(np.float32)[0]

MUTANTS = ("shift_x", "shift_y", "halo15", "halo31", "no_y_check16", "no_y_check32", "truncate", "le", "nan_int_max",
           "depth0_as_1", "flush_thr", "inf_as_nan")


class Frames(NamedTuple):
    depth: np.ndarray        # uint16 [n, h, w]
    labels: np.ndarray       # uint16 [n, h, w]
    nodes: np.ndarray        # int32 [n, h, w]
    C: int
    level: int
    parents: np.ndarray      # uint64 [2^level, C]: live pixels by (node, label)

    @property
    def live(self):
        return (self.nodes >= 0) & (self.labels < self.C)

    def live_pixels(self):
        """(img, y, x) of the live pixels in memory order: the order of every per-pixel array of this module."""
        return np.nonzero(self.live)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _parents(nodes, labels, n_nodes, n_classes):
    live = (nodes >= 0) & (labels < n_classes)
    out = np.zeros((n_nodes, n_classes), np.uint64)
    np.add.at(out, (nodes[live], labels[live].astype(np.int64)), 1)
    return out


@functools.lru_cache(maxsize=None)
def frames():
    """Two frames of 77 x 150.  Live pixels (about 30 %, and every second pixel of the frame's border) carry depths from
    DEPTHS, a few 0 and 65535; every other pixel a random depth in 1 .. 65534, so a probe one cell off reads another value.
    Of the pixels that are not live, a few sit on a node with a label >= C: train_numpy counts no such pixel (the reference
    would index its histogram out of bounds there: undefined), and it routes them in update_pixels like any other."""
    rng = np.random.default_rng(H * W)
    shape = (N_IMG, H, W)
    depth = rng.integers(1, 65535, size=shape).astype(np.uint16)
    live = rng.random(shape) < 0.3
    live[:, 0, 0::2] = live[:, H - 1, 1::2] = live[:, 0::2, 0] = live[:, 1::2, W - 1] = True
    nodes = rng.integers(0, 1 << LEVEL, size=shape).astype(np.int32)
    labels = rng.integers(0, C, size=shape).astype(np.uint16)
    r = rng.random(shape)
    nodes[~live & (r >= 0.03)] = -1
    labels[~live & (r < 0.03)] = rng.choice([C, C + 1, 65535], size=int((~live & (r < 0.03)).sum()))
    labels[~live & (r >= 0.03) & (r < 0.5)] = C + 1
    small = rng.choice(DEPTHS, size=shape).astype(np.uint16)
    q = rng.random(shape)
    small[q < 0.006] = 0
    small[(q >= 0.006) & (q < 0.012)] = 65535
    depth[live] = small[live]
    f = Frames(depth, labels, nodes, C, LEVEL, _parents(nodes, labels, 1 << LEVEL, C))
    assert np.array_equal(f.live, live)
    _freeze(f.depth, f.labels, f.nodes, f.parents)
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the restatement's response, copied: all proposals at once, with the probe positions and the mutants
# ---------------------------------------------------------------------------------------------------------------------
def _floor_i32(q, mutant):
    with np.errstate(invalid="ignore"):
        q = q.astype(np.float32)
        f = (np.trunc(q) if mutant == "truncate" else np.floor(q)).astype(np.float64)
    f = np.where(np.isnan(f), 2147483647.0 if mutant == "nan_int_max" else 0.0, f)
    if mutant == "inf_as_nan":
        f = np.where(np.isinf(f), 0.0, f)
    return np.clip(f, -2147483648.0, 2147483647.0).astype(np.int64)


def _in_staged(px, py, x, y, halo):
    rx, ry = px - (x // TILE_W) * TILE_W, py - (y // TILE_H) * TILE_H
    return (rx >= -halo) & (rx < TILE_W + halo) & (ry >= -halo) & (ry < TILE_H + halo)


def response(depth, img, y, x, props, mutant=None):
    """f [P, n] of the pixels (img, y, x) under the proposals `props` [P, 5], and the four probe coordinates
    (ux, uy, vx, vy), each int64 [P, n], in image coordinates after the wrapping add."""
    n_img, h, w = depth.shape
    d = depth[img, y, x]
    df = d.astype(np.float32)
    if mutant == "depth0_as_1":
        df = np.where(d == 0, F32(1), df)
    num = np.asarray(props, np.float32)[:, :4]
    with np.errstate(all="ignore"):
        off = [_floor_i32(num[:, k, None] / df[None, :], mutant) for k in range(4)]
    ux, uy, vx, vy = tn._wrap(x + off[0]), tn._wrap(y + off[1]), tn._wrap(x + off[2]), tn._wrap(y + off[3])

    def get(py, px):
        if mutant == "shift_x":
            px = px + 1
        if mutant == "shift_y":
            py = py + 1
        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        flat = (img * h + py) * w + px
        out = np.where(ok, depth.ravel()[np.where(ok, flat, 0)], 65535)
        if mutant in ("halo15", "halo31"):
            out = np.where(_in_staged(px, py, x, y, int(mutant[4:])), out, 65535)
        if mutant in ("no_y_check16", "no_y_check32"):
            far = ~_in_staged(px, py, x, y, int(mutant[10:]))
            loose = far & (px >= 0) & (px < w) & (flat >= 0) & (flat < depth.size)
            out = np.where(loose, depth.ravel()[np.where(loose, flat, 0)], out)
        return out.astype(np.float32)

    f = get(uy, ux) - get(vy, vx)
    if mutant != "depth0_as_1":
        f = np.where(d == 0, F32(0), f)
    return f.astype(np.float32), (ux, uy, vx, vy)


def decisions(fr, props, mutant=None):
    """bool [n_live, P]: live pixel i goes left under proposal j."""
    img, y, x = fr.live_pixels()
    f, _ = response(fr.depth, img, y, x, props, mutant)
    thr = np.asarray(props, np.float32)[:, 4]
    if mutant == "flush_thr":
        thr = np.where(np.abs(thr) < np.finfo(np.float32).tiny, F32(0), thr)
    with np.errstate(invalid="ignore"):
        left = (f <= thr[:, None]) if mutant == "le" else (f < thr[:, None])
    return np.ascontiguousarray(left.T)


def split_threshold(f):
    """The threshold between two values f takes (their mean: a whole number or a half) that sends the share of pixels
    closest to one half left."""
    vals, cnt = np.unique(f, return_counts=True)
    assert len(vals) > 1, "the response takes one value only"
    share = np.cumsum(cnt)[:-1] / f.size
    i = int(np.argmin(np.abs(share - 0.5)))
    thr = F32((np.float64(vals[i]) + np.float64(vals[i + 1])) / 2)
    assert vals[i] < thr <= vals[i + 1]
    return thr


def with_split_thresholds(fr, props, which=None):
    img, y, x = fr.live_pixels()
    f, _ = response(fr.depth, img, y, x, props)
    for j in (range(len(props)) if which is None else which):
        props[j, 4] = split_threshold(f[j])
    return props


# ---------------------------------------------------------------------------------------------------------------------
# case 1: halo and image edges
# ---------------------------------------------------------------------------------------------------------------------
# offsets in pixels at depth 12 (times 12 / d at depth d): from a pixel's place in its tile to the last staged cell and
# the first one beyond it, -16/-17 and 47/48 in x, -16/-17 and 23/24 in y for the 16-cell halo, -32/-33, 63/64 and 39/40
# for the 32-cell one; small ones for the image's border
OFFS_X = (0, 1, -1, 2, -3, 5, 16, -16, 17, -17, 20, -21, 24, -25, 31, -31, 32, -32, 33, -33, 40, -41, 47, -47, 48, -48,
          56, -57, 63, -63, 64, -64)
OFFS_Y = (0, 1, -1, 2, -2, 3, -3, 16, -16, 17, -17, 20, -20, 23, -23, 24, -24, 32, -32, 33, -33, 36, -36, 39, -39, 40,
          -40, 8, -8)
P_HALO = 70


@functools.lru_cache(maxsize=None)
def halo_props():
    rng = np.random.default_rng(70)
    props = np.zeros((P_HALO, 5), np.float32)
    for j in range(P_HALO):
        ox = [OFFS_X[(2 * j + k) % len(OFFS_X)] for k in (0, 1)]
        oy = [OFFS_Y[(2 * j + k) % len(OFFS_Y)] for k in (0, 1)]
        kind = j % 5
        if kind in (0, 1):          # one axis at an edge, the other one near the pixel: that axis alone decides LDS or global
            if j % 2 == 0:
                oy = [int(rng.integers(-1, 2)), int(rng.integers(-1, 2))]
            else:
                ox = [int(rng.integers(-1, 2)), int(rng.integers(-1, 2))]
        num = np.array([ox[0], oy[0], ox[1], oy[1]], np.float32) * F32(LCM)
        for k in range(4):          # the whole multiple, or the float next to it on either side
            nudge = (j + k) % 3 if num[k] != 0 else 0      # (next to zero lie denormals: not this case's business)
            if nudge == 1:
                num[k] = np.nextafter(num[k], F32(np.inf))
            elif nudge == 2:
                num[k] = np.nextafter(num[k], F32(-np.inf))
        if kind == 4:               # f depends on one probe only
            num[2:4] = 0.0
        props[j, :4] = num
    fr = frames()
    with_split_thresholds(fr, props)
    lopsided = [j for j, s in enumerate(decisions(fr, props).mean(axis=0)) if not 0.3 <= s <= 0.7]
    props[lopsided, 2:4] = 0.0      # both probes left the image at most pixels (f = 0): keep one, f = 65535 - d there
    with_split_thresholds(fr, props, which=lopsided)
    _freeze(props)
    return props


# ---------------------------------------------------------------------------------------------------------------------
# case 2: numerators and thresholds
# ---------------------------------------------------------------------------------------------------------------------
BIG_IN = F32(2.0 ** 21 - 0.25)       # the largest numerators k_train_bits takes on its one-fma path
TINY_IN = F32(2.0 ** -87)            # and the smallest
MENU_A = (0.0, -0.0, -0.5, 0.5, -0.999, 0.75, -1e-3, 1e-3, BIG_IN, -BIG_IN, TINY_IN, -TINY_IN, 60.0, -84.0, 11.5, -11.5,
          -1.0, 1.0, -2.0, 3.0, 24.0, -36.0, np.nextafter(F32(-12), F32(0)), np.nextafter(F32(12), F32(0)))
P_NUM = 37


@functools.lru_cache(maxsize=None)
def numerator_props_a():
    """Block (a): every numerator in range for both kernels' fast paths."""
    L = len(MENU_A)
    props = np.zeros((P_NUM, 5), np.float32)
    for j in range(P_NUM):
        props[j, :4] = [MENU_A[j % L], MENU_A[(5 * j + 1) % L], MENU_A[(7 * j + 2) % L], MENU_A[(11 * j + 3) % L]]
        if j % 3 == 2:
            props[j, 2:4] = (0.0, -0.0) if j % 2 else (0.0, 0.0)
        if j % 3 == 1:               # (the proposals block (b) replaces a numerator of: both probes move, so f still varies)
            props[j, :4] = np.roll(np.array([60.0, -84.0, -36.0, 24.0], np.float32) * (-1) ** (j // 3), j // 3)
    with_split_thresholds(frames(), props)
    _freeze(props)
    return props


# name -> (value, numerator slot).  2^21 leaves k_train_bits' range and stays in k_train_histogram's; every other one leaves
# both.  3e38 / 65535 > 2^31: the quotient saturates at every depth.  2147483520 = 2^31 - 128 in x: at depth 1 the add
# wraps from x = 128 on.
REPLACEMENTS = {
    "2p21": (F32(2.0 ** 21), 0), "2p104": (F32(2.0 ** 104), 1), "2m100": (F32(2.0 ** -100), 2), "denormal": (F32(1e-40), 3),
    "pos_inf": (F32(np.inf), 0), "neg_inf": (F32(-np.inf), 1), "nan": (F32(np.nan), 2), "saturating": (F32(3e38), 3),
    "neg_saturating": (F32(-3e38), 1), "int_max_less_127": (F32(2147483520.0), 0),
}


def replaced_proposal(name):
    return 1 + 3 * list(REPLACEMENTS).index(name)       # 1, 4, 7, ...: every place of a batch of four


@functools.lru_cache(maxsize=None)
def numerator_props_b(name):
    """Block (a) with one numerator of one proposal replaced (and that proposal's threshold put back at its median)."""
    value, slot = REPLACEMENTS[name]
    props = numerator_props_a().copy()
    j = replaced_proposal(name)
    props[j, slot] = value
    with_split_thresholds(frames(), props, which=[j])
    _freeze(props)
    return props


THR_BASES = ((0.0, 0.0, 0.0, 0.0),            # f = 0 at every pixel
             (2400.0, 0.0, 0.0, 0.0),         # u leaves the image at every listed depth: f = 65535 - d
             (0.0, 0.0, 0.0, -2400.0),        # f = d - 65535
             (-12.0, 24.0, 36.0, -12.0))      # two probes near the pixel


@functools.lru_cache(maxsize=None)
def threshold_props():
    """Block (c): for each of four responses, the value it takes most often, the floats on either side, and the edges."""
    fr = frames()
    img, y, x = fr.live_pixels()
    rows = []
    for base in THR_BASES:
        f, _ = response(fr.depth, img, y, x, np.array([base + (0.0,)], np.float32))
        vals, cnt = np.unique(f[0], return_counts=True)
        mode = F32(vals[np.argmax(cnt)])
        for thr in (mode, np.nextafter(mode, F32(np.inf)), np.nextafter(mode, F32(-np.inf)), 0.0, -0.0, np.inf, -np.inf,
                    np.nan, DENORM_MIN, -DENORM_MIN, 65535.0, -65535.0, 65536.0, -65536.0):
            rows.append(base + (thr,))
    rows.append(THR_BASES[1] + (65532.5,))          # (a ragged last batch)
    props = np.array(rows, np.float32)
    assert len(props) % 4 == 1 and np.signbit(props[4, 4]) and props[8, 4] > 0 and props[8, 4] < np.finfo(np.float32).tiny
    _freeze(props)
    return props


CASES = ("halo", "num_a") + tuple("num_b_" + k for k in REPLACEMENTS) + ("thr",)


def case_props(name):
    if name == "halo":
        return halo_props()
    if name == "num_a":
        return numerator_props_a()
    if name == "thr":
        return threshold_props()
    return numerator_props_b(name[len("num_b_"):])


# which mutants each case is built to notice
KILLS = {
    "halo": ("shift_x", "shift_y", "halo15", "halo31", "no_y_check16", "no_y_check32", "truncate", "depth0_as_1"),
    "num_a": ("shift_x", "shift_y", "truncate", "depth0_as_1"),
    "num_b_nan": ("nan_int_max",),
    "num_b_pos_inf": ("inf_as_nan",),
    "num_b_neg_inf": ("inf_as_nan",),
    "thr": ("le", "flush_thr"),
}


# ---------------------------------------------------------------------------------------------------------------------
# expected values: train_numpy alone
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_bits(name):
    """bool [n_live, P] from tn.compute_feature, one proposal at a time."""
    fr, props = frames(), case_props(name)
    img, y, x = fr.live_pixels()
    out = np.zeros((len(img), len(props)), bool)
    for j, p in enumerate(props):
        with np.errstate(invalid="ignore"):
            out[:, j] = tn.compute_feature(fr.depth, img, y, x, p[0:2], p[2:4]) < p[4]
    _freeze(out)
    return out


@functools.lru_cache(maxsize=None)
def expected_counts(name, window):
    fr, props = frames(), case_props(name)
    start, end, NB = window
    out = tn.count_children(fr.depth, fr.labels, fr.nodes, props, start, end, NB, fr.C)
    _freeze(out)
    return out


def routing_nodes(fr, P, turn):
    """Nodes for rdf_train_update_pixels at a level of at least P nodes: pixel i sits on node (i + turn) mod P, every pixel
    that is live for the counting kernels and the ones with a label >= C as well; over P turns every pixel meets every
    proposal."""
    idx = np.arange(fr.depth.size, dtype=np.int64).reshape(fr.depth.shape)
    return np.where(fr.nodes >= 0, (idx + turn) % P, -1).astype(np.int32)


def routing_tree(props, n_classes):
    """(tree, level, D): one record per proposal at the first level that holds them all, both child flags -1."""
    P = len(props)
    level = max(1, int(np.ceil(np.log2(P))))
    D = level + 2
    tree = np.zeros(((1 << D) - 1, 7 + 2 * n_classes), np.float32)
    base = (1 << level) - 1
    tree[base:base + P, 0:5] = props
    tree[base:base + P, 5:7] = -1.0
    return tree, level, D


# ---------------------------------------------------------------------------------------------------------------------
# coverage: where the probes of a case land
# ---------------------------------------------------------------------------------------------------------------------
def coverage(fr, props):
    """Counts of live (pixel, proposal, probe) triples by where the probe lands, all inside the image.  For the staged
    tile's edges the other axis lies inside the staged cells, so that the named axis alone decides between LDS and global
    memory: "h16 x- last" is tile-relative x = -16, "h16 x- beyond" is x = -17, and so on.  For the image's border the
    other axis lies inside the image: "image x- beyond" is x = -1, "image x+ beyond" is x = W."""
    n_img, h, w = fr.depth.shape
    img, y, x = fr.live_pixels()
    f, (ux, uy, vx, vy) = response(fr.depth, img, y, x, props)
    px, py = np.concatenate([ux, vx]), np.concatenate([uy, vy])
    rx, ry = px - (x // TILE_W) * TILE_W, py - (y // TILE_H) * TILE_H
    in_x, in_y = (px >= 0) & (px < w), (py >= 0) & (py < h)
    out = {}
    for halo in (HALO_HIST, HALO_BITS):
        st_x = (rx >= -halo) & (rx < TILE_W + halo)
        st_y = (ry >= -halo) & (ry < TILE_H + halo)
        for axis, r, other, size in (("x", rx, st_y, TILE_W), ("y", ry, st_x, TILE_H)):
            ok = other & in_x & in_y
            out[f"h{halo} {axis}- last"] = int((ok & (r == -halo)).sum())
            out[f"h{halo} {axis}- beyond"] = int((ok & (r == -halo - 1)).sum())
            out[f"h{halo} {axis}+ last"] = int((ok & (r == size + halo - 1)).sum())
            out[f"h{halo} {axis}+ beyond"] = int((ok & (r == size + halo)).sum())
    out["image x- last"], out["image x- beyond"] = int((in_y & (px == 0)).sum()), int((in_y & (px == -1)).sum())
    out["image x+ last"], out["image x+ beyond"] = int((in_y & (px == w - 1)).sum()), int((in_y & (px == w)).sum())
    out["image y- last"], out["image y- beyond"] = int((in_x & (py == 0)).sum()), int((in_x & (py == -1)).sum())
    out["image y+ last"], out["image y+ beyond"] = int((in_x & (py == h - 1)).sum()), int((in_x & (py == h)).sum())
    far = ~_in_staged(px, py, x, y, HALO_BITS)
    out["image 0 far y >= H"] = int((far & in_x & (py >= h) & (img == 0)).sum())
    out["image 1 far y < 0"] = int((far & in_x & (py < 0) & (img == n_img - 1)).sum())
    out["f == thr"] = int((f == np.asarray(props, np.float32)[:, 4, None]).sum())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# case 5: the 16-bit counter limit
# ---------------------------------------------------------------------------------------------------------------------
LIMIT_SHAPE = (4, 150, 220)          # 132000 pixels
LIMIT_GROUPS = (((0, 1), 65535), ((1, 1), 65536), ((0, 2), 929))      # ((node, class), pixels): every pixel is live
LIMIT_C, LIMIT_LEVEL = 3, 1


@functools.lru_cache(maxsize=None)
def limit_case():
    """Three (node, class) groups scattered over four frames; proposals 0, 1 send every pixel left (+Inf), 2, 3 none
    (-Inf), 4, 5 are mixed."""
    rng = np.random.default_rng(65535)
    n_px = int(np.prod(LIMIT_SHAPE))
    assert sum(n for _, n in LIMIT_GROUPS) == n_px
    group = rng.permutation(np.repeat(np.arange(len(LIMIT_GROUPS)), [n for _, n in LIMIT_GROUPS])).reshape(LIMIT_SHAPE)
    nodes = np.array([g[0][0] for g in LIMIT_GROUPS], np.int32)[group]
    labels = np.array([g[0][1] for g in LIMIT_GROUPS], np.uint16)[group]
    depth = rng.integers(1, 9, size=LIMIT_SHAPE).astype(np.uint16)
    props = np.array([[24.0, -12.0, 0.0, 0.0, np.inf], [-36.0, 5.0, 12.0, 12.0, np.inf],
                      [24.0, -12.0, 0.0, 0.0, -np.inf], [-36.0, 5.0, 12.0, 12.0, -np.inf],
                      [24.0, -12.0, 0.0, 0.0, 0.5], [-36.0, 5.0, 12.0, 12.0, -0.5]], np.float32)
    fr = Frames(depth, labels, nodes, LIMIT_C, LIMIT_LEVEL, _parents(nodes, labels, 1 << LIMIT_LEVEL, LIMIT_C))
    _freeze(fr.depth, fr.labels, fr.nodes, fr.parents, props)
    return fr, props


@functools.lru_cache(maxsize=None)
def limit_counts():
    fr, props = limit_case()
    out = tn.count_children(fr.depth, fr.labels, fr.nodes, props, 0, 4, 4, fr.C)
    _freeze(out)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# case 6: the counting sort's key counts
# ---------------------------------------------------------------------------------------------------------------------
SORT_SHAPE = (1, 53, 49)             # 2597 pixels = 40 waves and 37 pixels
SORT_KEYS = ((1, 1), (4096, 4), (4097, 4))        # (n_nodes, C): 1, 16384 and 16388 keys
SORT_COUNTERS = 16384                # kSortCounters: a key has 2^shift counters while keys << shift fits
SORT_P = 5


def sort_slot_shift(n_keys):
    sh = 0
    while sh < 8 and (n_keys << (sh + 1)) <= SORT_COUNTERS:
        sh += 1
    return sh


@functools.lru_cache(maxsize=None)
def sort_case(n_nodes, n_classes):
    """One frame whose pixels, 64 at a time in memory order (a wave of k_train_sort), hold: waves 0 .. 7 exactly four keys
    (the wave aggregates them, kSortIters = 4), waves 8 .. 15 one key, waves 16 .. 23 exactly five, the others random keys
    (with 16384 keys: 40 or more distinct ones) -- among them the first and the last key.  About a fifth is not live."""
    rng = np.random.default_rng(n_nodes * 64 + n_classes)
    n_keys = n_nodes * n_classes
    n_px = int(np.prod(SORT_SHAPE))
    key = rng.integers(0, n_keys, size=n_px)
    for wv in range(24):
        k = {0: 4, 1: 1, 2: 5}[wv // 8]
        pick = rng.choice(n_keys, size=min(k, n_keys), replace=False)
        seg = pick[rng.integers(0, len(pick), size=64)]
        seg[:len(pick)] = pick
        key[wv * 64:(wv + 1) * 64] = seg
    key[1600], key[1601], key[-1] = 0, n_keys - 1, n_keys - 1
    nodes = (key // n_classes).astype(np.int32)
    labels = (key % n_classes).astype(np.uint16)
    dead = rng.random(n_px) < 0.2
    dead[:24 * 64] = False
    dead[[1600, 1601, n_px - 1]] = False
    kind = rng.integers(0, 2, size=n_px)
    nodes[dead & (kind == 0)] = -1
    labels[dead & (kind == 1)] = n_classes + 2
    depth = rng.integers(1, 40, size=n_px).astype(np.uint16)
    state = np.random.get_state()
    np.random.seed(n_keys)
    props = tn.make_random_features(SORT_P)
    np.random.set_state(state)
    fr = Frames(depth.reshape(SORT_SHAPE), labels.reshape(SORT_SHAPE), nodes.reshape(SORT_SHAPE), n_classes,
                int(np.ceil(np.log2(n_nodes))), _parents(nodes, labels, n_nodes, n_classes))
    _freeze(fr.depth, fr.labels, fr.nodes, fr.parents, props)
    return fr, props


def sort_window(n_nodes):
    """(start, end, NB): the children of the upper half of the nodes."""
    start = (n_nodes // 2) * 2
    return start, 2 * n_nodes, 2 * n_nodes - start


def distinct_keys_per_wave(fr):
    key = np.where(fr.live, fr.nodes.astype(np.int64) * fr.C + fr.labels, -1).ravel()
    return [len(set(key[i:i + 64].tolist()) - {-1}) for i in range(0, key.size, 64)]
