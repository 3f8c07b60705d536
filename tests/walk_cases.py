"""The cases of tests/test_label_walks.py: inputs that break a tree walk, for the two walks of librdf_labels.so (k_refit_count,
k_posterior), and inputs that reach the counting paths of k_refit_count that no other case reaches.  Seeded numpy builders, each
cached and frozen, that the CPU tests (does the case contain what it is meant to?) and the GPU tests (every entry point against
refit_numpy / posterior_numpy / prune_numpy) both call, so that both see the same arrays.

  adversarial_case()   T6/D6/C5 on 2 x 13 x 70: every offset of ADVERSARIAL_OFFSETS and every threshold of SPECIAL_THRESHOLDS on
                       a node of levels 0 to 2 that live walks pass, planted flags, trained-like levels below.
  divide_case()        one D = 1 tree per (numerator, depth): numerators on and next to whole multiples of the pixel's depth,
                       neighbours that alternate between two depths, so a quotient one off changes the side.
  counting_case(name)  the shapes on both sides of `lds_levels == 0`, labels up to C - 1 = 2048.
  bucket_case()        one workgroup a row, 256 slots a row: cells of one workgroup that want the same bucket of its table.

`trace` below is refit_numpy.walk taken apart (the same helpers, the same order) so that a test can see what each feature step
met; the CPU tests check that it ends where refit_numpy.walk ends.  No expected value of a GPU test comes from it."""
import functools
from fractions import Fraction

import numpy as np

import posterior_cases as pc
import refit_cases as rc
import refit_numpy as rn

F32 = np.float32
NO_PIXEL = 65535
SCALES = (1.0, 0.5, 3.0)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ------------------------------------------------------------ the walk, taken apart ------------------------------------------
def step(frame, rec, x, y, scale):
    """One feature step of rule R2 at pixel (x, y) under record `rec`, as refit_numpy.walk makes it.  Returns a dict: `num` the
    four rounded products s * o, `quot` the four rounded quotients, `off` their floors, `at` the two probes' (x, y) after the
    wrapping add, `val` what the probes read, `f`, `side`."""
    d = F32(frame[y, x])
    scale = F32(scale)
    with np.errstate(all="ignore"):
        num = [F32(scale * rec[k]) for k in range(4)]
        quot = [F32(n / d) for n in num]
        off = [rn.floor_i32(q) for q in quot]
        at = [(rn.wrap_i32(x + off[0]), rn.wrap_i32(y + off[1])), (rn.wrap_i32(x + off[2]), rn.wrap_i32(y + off[3]))]
        val = [rn.probe(frame, *p) for p in at]
        f = val[0] - val[1]
        side = 0 if f < rec[4] else 1
    return dict(num=num, quot=quot, off=off, sums=[x + off[0], y + off[1], x + off[2], y + off[3]], at=at, val=val, f=f, side=side)


def trace(frame, tree, D, x, y, scale):
    """([(node, step dict)], end): the nodes the walk passes and where it ends, (node, side) or None for a walk that falls off."""
    g, seen = 0, []
    for j in range(D):
        n = (1 << j) - 1 + g
        st = step(frame, tree[n], x, y, scale)
        seen.append((n, st))
        if rn.is_leaf_slot(tree[n], st["side"]):
            return seen, (n, st["side"])
        g = 2 * g + st["side"]
    return seen, None


def live_pixels(depth, labels, C):
    """(image, y, x) of the pixels rule R1 walks, in memory order."""
    return [tuple(int(v) for v in p) for p in np.argwhere((labels > 0) & (labels < C) & (depth > 0) & (depth < NO_PIXEL))]


# ------------------------------------------------------------ 1. the adversarial walk ----------------------------------------
# tests/test_gpu_parity.py's ADVERSARIAL, copied (that module builds its known-answer cases on import): offsets at the edges of
# what the evaluator's 16-byte record can hold, values a hair below whole numbers, denormals, inf, NaN
PARITY_ADVERSARIAL = [8388607.5, 8388607.0, 8388608.0, -8388608.0, -8388608.5, -8388607.5, 16777216.0, 3e9, -3e9, 1e-30,
                      -1e-30, 1e-45, -1e-45, 2.0 ** -87, -(2.0 ** -87), 2.0 ** -88, 11.999999, -11.999999, 23.999998,
                      0.99999994, -0.99999994, -1.0000001, 65534.0, 65533.996, 131067.99, 4000.0, 3999.9998, -4000.0,
                      0.0, -0.0, 0.5, -0.5, 1e38, -1e38, float("inf"), float("-inf"), float("nan"), 2.5e6, -2.5e6,
                      7999.9995, 12345.678, -12345.678, 1.17549435e-38, 8388606.5,
                      4194303.5, 4194303.75, 4194304.0, -4194304.0, -4194303.5, -4194304.5, 4194302.0, -4194303.0, 2097151.9]
OVERFLOWS_AT_3 = (3e38, -3e38)             # finite at scales 1.0 and 0.5; s * o is +-inf at 3.0
INT_MAX_LESS_127 = 2147483520.0            # 2^31 - 128: at depth 1 the quotient is the largest int32 an fp32 holds
DENORMALS = (1e-40, -1e-40)                # denormal at every scale: a flushed product would still floor to 0 and to -1 ...
ADVERSARIAL_OFFSETS = tuple(PARITY_ADVERSARIAL) + OVERFLOWS_AT_3 + (INT_MAX_LESS_127,) + DENORMALS
# thresholds that send every response one way (NaN: right; +inf: left; -inf, -65535.0: right; 65535.5: left), that split by the
# response's sign (+-0.0) and that only a probe on depth 0 against a probe outside the frame goes left of (-65534.5)
SPECIAL_THRESHOLDS = (np.nan, np.inf, -np.inf, 0.0, -0.0, 65535.5, -65535.0, -65534.5)
# flags on sides that walks take: floor(-0.5) = -1 goes on; 0.5, NaN (-> 0), +inf and -inf (saturate) are leaf slots
PLANTED_FLAGS = (-0.5, 0.5, np.nan, np.inf, -np.inf)
PLANT_LEVELS = 3                           # levels 0, 1, 2 carry the plants; every one of their sides says "go on"
SPECIAL_DEPTHS = (1, 2, 3, 7, 11, 12, 4000, 65534)          # under labelled pixels, at both ends of the batch
ADV = dict(n=2, H=13, W=70, T=6, D=6, C=5, first=140, seed=4242, filter_class=2)


def adversarial_frames():
    """2 images of 70 x 13 (the width no multiple of 8 or 64: a wave spans both images): depths in 300..3000, 0 and 65535
    sprinkled in, labels 0 .. C + 1, SPECIAL_DEPTHS under labelled pixels at the first pixels of image 0 and the last of image 1."""
    m = ADV
    rng = np.random.default_rng(m["seed"])
    shape = (m["n"], m["H"], m["W"])
    depth = rng.integers(300, 3001, shape).astype(np.uint16)
    r = rng.random(shape)
    depth[r < 0.04] = 0
    depth[(r >= 0.04) & (r < 0.08)] = NO_PIXEL
    labels = rng.integers(0, m["C"] + 2, shape).astype(np.uint16)               # ids C and C + 1 are unknown
    labels[rng.random(shape) < 0.2] = 0
    k = len(SPECIAL_DEPTHS)
    depth[0, 0, :k] = SPECIAL_DEPTHS
    depth[-1, -1, -k:] = SPECIAL_DEPTHS
    labels[0, 0, :k] = labels[-1, -1, -k:] = 1 + np.arange(k) % (m["C"] - 1)
    return depth, labels


def _reaching(depth, tree, node, pixels, scale):
    """The pixels of `pixels` whose walk through `tree` passes `node`, with their step there."""
    level = int(node + 1).bit_length() - 1
    out = []
    for i, y, x in pixels:
        seen, _ = trace(depth[i], tree, level + 1, x, y, scale)
        if seen[-1][0] == node:
            out.append(((i, y, x), seen[-1][1]))
    return out


@functools.lru_cache(maxsize=None)
def adversarial_case():
    """(depth, labels, forest, plants).  Node m of the 42 nodes of levels 0 to 2 (level by level, trees in order) gives one probe
    two offsets of ADVERSARIAL_OFFSETS -- dealt in order, so every one is planted, the first 26 twice -- and draws the other
    probe one to six pixels long at these depths, so that the response varies; u and v take turns.  Levels 0 and 1 and every fourth
    node of level 2 get the median response of the live pixels that reach them at scale 1.0 as threshold (`f == thresh` occurs,
    both children are visited); the other nodes of level 2 get SPECIAL_THRESHOLDS in turn.  PLANTED_FLAGS go on sides of
    median-threshold nodes of level 2; one "go on" goes on a slot of level D - 1 that walks reach at every scale.  `plants` says
    where: {"flags": [(tree, node, side, flag)], "fall_off": (tree, node, side), "special": [(tree, node)]}."""
    m = ADV
    T, D, C = m["T"], m["D"], m["C"]
    depth, labels = adversarial_frames()
    forest = rc.trained_like(T, D, C, first=m["first"], leaf_prob=0.3, min_leaf_level=PLANT_LEVELS)
    forest[:, :, 0:4] /= F32(100.)                        # a few pixels at depths 300..3000
    forest[:, :, 4] /= F32(20.)                           # thresholds inside the range of depth differences
    rng = np.random.default_rng(m["seed"] + 1)
    adv = np.array(ADVERSARIAL_OFFSETS, np.float32)
    pixels = live_pixels(depth, labels, C)
    plants = dict(flags=[], special=[], fall_off=None)
    todo_flags = list(PLANTED_FLAGS)
    m_idx = -1
    for level in range(PLANT_LEVELS):                     # level by level: a node's threshold needs the levels above it
        for t in range(T):
            for n in range((1 << level) - 1, (2 << level) - 1):
                m_idx += 1
                pair = adv[[(2 * m_idx) % adv.size, (2 * m_idx + 1) % adv.size]]
                at = 0 if m_idx % 2 == 0 else 2
                forest[t, n, at:at + 2] = pair
                forest[t, n, 2 - at:4 - at] = rng.choice([-1., 1.], 2) * rng.uniform([1500., 600.], [9000., 4000.])     # one to six pixels
                special = level == PLANT_LEVELS - 1 and n % 4 != 0
                if special:
                    k = len(plants["special"])
                    forest[t, n, 4] = SPECIAL_THRESHOLDS[k % len(SPECIAL_THRESHOLDS)]
                    plants["special"].append((t, n))
                    continue
                f = sorted(float(st["f"]) for _, st in _reaching(depth, forest[t], n, pixels, 1.0))
                assert len(f) >= 8 and f[0] < f[-1], (t, n, len(f))
                forest[t, n, 4] = f[len(f) // 2] if f[len(f) // 2] > f[0] else f[-1]
                if level == PLANT_LEVELS - 1:
                    for s in (0, 1):
                        if todo_flags:
                            flag = todo_flags.pop(0)
                            forest[t, n, 5 + s] = flag
                            plants["flags"].append((t, n, s, flag))
                            if rn.is_leaf_slot(forest[t, n], s):              # a leaf slot now: it needs a PDF
                                pdf = rng.integers(1, 1000, C).astype(np.float32)
                                forest[t, n, 7 + s * C:7 + (s + 1) * C] = pdf / pdf.sum(dtype=np.float32)
    assert not todo_flags
    # the fall-off: the slot of level D - 1 that the most walks reach at the scale at which the fewest reach it
    reached = []
    for scale in SCALES:
        ends = [trace(depth[i], forest[t], D, x, y, scale)[1] for i, y, x in pixels for t in range(T)]
        tn = [(k % T,) + e for k, e in enumerate(ends)]
        reached.append({s: tn.count(s) for s in set(tn) if s[1] >= (1 << (D - 1)) - 1})
    common = set(reached[0]) & set(reached[1]) & set(reached[2])
    assert common, "no slot of the last level is reached at every scale"
    t, n, s = max(sorted(common), key=lambda slot: min(r[slot] for r in reached))
    forest[t, n, 5 + s] = -1.
    plants["fall_off"] = (t, n, s)
    _freeze(depth, labels, forest)
    return depth, labels, forest, plants


def adversarial_filter():
    """The filter image of the r = 2 posterior run: three label pixels in five carry ADV["filter_class"]."""
    m = ADV
    f = pc.filter_image(m["seed"], (m["n"], m["H"] // 2, m["W"] // 2), m["filter_class"])
    _freeze(f)
    return f


# ------------------------------------------------------------ 2. the divide, one ulp at a time -------------------------------
DIV_DEPTHS = (1, 2, 3, 7, 11, 12, 4000, 65534)             # row r holds the pixel of depth DIV_DEPTHS[r]
DIV_K = (1, -1, 2, -2, 3, -3, 5, -5)
DIV_XC, DIV_W = 32, 65                                     # the pixel's column; whole offsets up to 6 k stay inside the row
DIV_NEAR, DIV_FAR = 20000, 50000                           # the neighbours' two depths
DIV_C = 3


def _next(v, towards):
    return np.nextafter(F32(v), F32(towards))


def div_numerators(d, scale):
    """The numerators of depth d meant for `scale`: for every k the one that `scale` takes to k * d, and its two fp32 neighbours.
    At scale 3.0 the one is fp32(k * d / 3) and of the three only those are kept whose product 3 * u is no fp32: it rounds."""
    out = []
    for k in DIV_K:
        if scale == 3.0:
            u = F32(np.float64(k * d) / 3.)
            trio = [v for v in (u, _next(u, np.inf), _next(u, -np.inf)) if Fraction(float(F32(3. * np.float64(v)))) != 3 * Fraction(float(v))]
        else:
            u = F32(k * d / scale)
            assert Fraction(float(u)) * Fraction(scale) == k * d
            trio = [u, _next(u, np.inf), _next(u, -np.inf)]
        out += trio
    return out


def div_even_odd(d):
    """The depths of the neighbours an even and an odd number of columns away, and the threshold between their responses.  The
    pixel itself is zero columns away and answers f = 0: the even depth is the one on whose side of the threshold 0 lies."""
    thr = (DIV_NEAR + DIV_FAR) // 2 - d
    return ((DIV_NEAR, DIV_FAR) if 0 < thr else (DIV_FAR, DIV_NEAR)) + (thr,)


@functools.lru_cache(maxsize=None)
def divide_case():
    """(depth [1, 8, 65], labels, filter, forest [T, 1, 7 + 2 C], combos).  Tree t probes u = (numerator, 0) against the pixel
    itself, with the threshold of its depth's row; left is class 1's leaf, right class 2's.  Only the pixels of column DIV_XC
    carry a label (and the filter's class 1): eight live pixels, each walked through every tree.  combos = [(tree, row, scale)]:
    the (numerator, d, scale) each tree was made for."""
    rows = len(DIV_DEPTHS)
    depth = np.zeros((1, rows, DIV_W), np.uint16)
    labels = np.zeros(depth.shape, np.uint16)
    filt = np.zeros(depth.shape, np.uint16)
    cols = np.arange(DIV_W)
    for r, d in enumerate(DIV_DEPTHS):
        even, odd, _ = div_even_odd(d)
        depth[0, r] = np.where((cols - DIV_XC) % 2 == 0, even, odd)
        depth[0, r, DIV_XC] = d
        labels[0, r, DIV_XC] = 1 + r % 2
        filt[0, r, DIV_XC] = 1
    recs, combos, index = [], [], {}
    for r, d in enumerate(DIV_DEPTHS):
        thr = div_even_odd(d)[2]
        for scale in SCALES:
            for u in div_numerators(d, scale):
                key = (np.array([u], np.float32).view(np.uint32)[0], r)
                if key not in index:
                    index[key] = len(recs)
                    rec = np.zeros(7 + 2 * DIV_C, np.float32)
                    rec[0], rec[4] = u, thr
                    rec[7 + 1], rec[7 + DIV_C + 2] = 1., 1.                     # one-hot: left says 1, right says 2
                    recs.append(rec)
                combos.append((index[key], r, scale))
    forest = np.stack(recs)[:, None, :].copy()
    _freeze(depth, labels, filt, forest)
    return depth, labels, filt, forest, tuple(combos)


def exact_floor_of_rounded_quotient(p, d):
    """floor(RN(p / d)) for an fp32 p and an integer d >= 1, RN the correctly rounded fp32 quotient, by exact arithmetic alone:
    the floor of the exact quotient, unless the exact quotient lies at or above the midpoint between the next whole number and
    the fp32 below it (a tie goes to the even mantissa), where the rounded quotient IS that whole number."""
    exact = Fraction(float(p)) / d
    e = exact.numerator // exact.denominator
    if exact == e:
        return e
    up = F32(e + 1)
    below = np.nextafter(up, F32(-np.inf))
    mid = (Fraction(float(below)) + (e + 1)) / 2
    even_up = (np.array([up], np.float32).view(np.uint32)[0] & 1) == 0
    return e + 1 if exact > mid or (exact == mid and even_up) else e


def div_side_of_offset(row, off):
    """The side (0 left, 1 right) of the pixel of row `row` when its u probe lands `off` columns away, in integers."""
    d = DIV_DEPTHS[row]
    even, odd, thr = div_even_odd(d)
    col = DIV_XC + off
    v = NO_PIXEL if col < 0 or col >= DIV_W else d if off == 0 else even if off % 2 == 0 else odd
    return 0 if v - d < thr else 1


# ------------------------------------------------------------ 3. the counting paths ------------------------------------------
# name: T, D, C and the frame; COUNTING_FIRST holds the first tree's seed, chosen by find_counting_first
COUNTING = {
    "t1_c2048": dict(T=1, D=3, C=2048, H=9, W=130),      # L = 1 and the histogram exactly full: 1 * 1 * 2 * 2048 cells
    "t1_c2049": dict(T=1, D=3, C=2049, H=9, W=130),      # one cell too many: L = 0
    "t3_c700":  dict(T=3, D=3, C=700, H=9, W=130),       # L = 0 with trees whose first cell is not cell 0
}
COUNTING_FIRST = {"t1_c2048": 600, "t1_c2049": 600, "t3_c700": 684}


def _one_root_leaf(forest):
    return all(rn.is_leaf_slot(tree[0], 0) != rn.is_leaf_slot(tree[0], 1) for tree in forest)


def root_keys_per_wave(depth, labels, forest):
    """Per tree (distinct, shared): over the waves of k_refit_count -- 64 consecutive pixels in memory -- the most distinct
    (side, class) keys of walks that end at the root in one wave, and the most lanes of one wave that hold the same such key."""
    T, D, C = rn.dims(forest)
    out = []
    for t in range(T):
        flat = np.full(depth.size, -1, np.int64)
        for i, y, x in live_pixels(depth, labels, C):
            at = rn.walk(depth[i], forest[t], D, x, y, 1.)
            if at is not None and at[0] == 0:
                flat[(i * depth.shape[1] + y) * depth.shape[2] + x] = at[1] * C + int(labels[i, y, x])
        waves = [w[w >= 0] for w in (flat[k:k + 64] for k in range(0, flat.size, 64))]
        out.append((max(len(set(w.tolist())) for w in waves), max((int(np.bincount(w).max()) for w in waves if w.size), default=0)))
    return out


def _counting_build(name, first):
    m = COUNTING[name]
    T, D, C = m["T"], m["D"], m["C"]
    rng = np.random.default_rng(C)
    shape = (1, m["H"], m["W"])
    depth = rng.integers(400, 1201, shape).astype(np.uint16)
    depth[rng.random(shape) < 0.03] = 0
    labels = rng.choice(np.array([1, 2, C // 2, C - 2, C - 1, C], np.uint16), size=shape).astype(np.uint16)
    labels[rng.random(shape) < 0.2] = 0
    forest = rc.trained_like(T, D, C, first=first, leaf_prob=0.4, min_leaf_level=0)
    forest[:, :, 0:4] /= F32(100.)
    forest[:, :, 4] /= F32(20.)
    return depth, labels, forest


def find_counting_first(name, start=600):
    """The search that chose COUNTING_FIRST: the first seed from `start` on whose trees all have one leaf side at the root, each
    with a wave that holds five and more distinct root-level keys and three lanes on one key."""
    first = start
    while True:
        depth, labels, forest = _counting_build(name, first)
        if _one_root_leaf(forest) and all(d >= 5 and s >= 3 for d, s in root_keys_per_wave(depth, labels, forest)):
            return first
        first += 1


@functools.lru_cache(maxsize=None)
def counting_case(name):
    """(depth [1, 9, 130], labels, forest): trained-like trees with leaf slots from level 0 on (one side of every root is one),
    depths in 400..1200 with a few holes, four pixels in five labelled from {1, 2, C // 2, C - 2, C - 1} and the unknown id C."""
    depth, labels, forest = _counting_build(name, COUNTING_FIRST[name])
    _freeze(depth, labels, forest)
    return depth, labels, forest


kTableBits = 11
kHashMul = 0x9E3779B1


def table_bucket(cell):
    """add_deep's bucket of a cell of counts: tag = (uint32_t)cell, h = (tag * 0x9E3779B1u) >> (32 - kTableBits)."""
    tag = int(cell) & 0xffffffff
    return ((tag * kHashMul) & 0xffffffff) >> (32 - kTableBits)


BUCKET = dict(D=10, C=4, tree_width=1024, H=4, W=256)
BUCKET_ROW_LABELS = (1, 2, 3, 1)           # constant along a row, neighbouring rows differ
# The hash is Fibonacci hashing, and the cells of ONE column tree under a constant label are an arithmetic progression (stride
# C): such keys never share a bucket, whatever the label or the columns (find_bucket_trees shows it: T = 1 gives no pair).  Cells
# of different trees lie T N 2C apart and do meet, so the forest is the column tree several times over: 6 is the smallest
# number of copies at which three cells of one row want one bucket.
BUCKET_TREES = 6


def bucket_cells(T, row_labels=BUCKET_ROW_LABELS):
    """Per row (one workgroup of 256 lanes) the cells of counts its pixels add to: column x ends, in every tree t, in slot (node
    511 + (x >> 1), side x & 1) of level 9 with the row's label; tree t's first cell is t N 2C."""
    m = BUCKET
    first, N = (1 << (m["D"] - 1)) - 1, (1 << m["D"]) - 1
    return [[t * N * 2 * m["C"] + ((first + (x >> 1)) * 2 + (x & 1)) * m["C"] + l for t in range(T) for x in range(m["W"])]
            for l in row_labels]


def bucket_sharing(T, row_labels=BUCKET_ROW_LABELS):
    """(pairs, most): per row the pairs of distinct cells that want one bucket, and the most cells that want one bucket."""
    pairs, most = [], []
    for cells in bucket_cells(T, row_labels):
        wanted = {}
        for c in cells:
            wanted.setdefault(table_bucket(c), set()).add(c)
        sizes = [len(v) for v in wanted.values()]
        pairs.append(sum(k * (k - 1) // 2 for k in sizes))
        most.append(max(sizes))
    return pairs, most


def find_bucket_trees():
    """The search that chose BUCKET_TREES: the smallest T at which some row has three pairs and some bucket three cells."""
    for T in range(1, 17):
        pairs, most = bucket_sharing(T)
        if max(pairs) >= 3 and max(most) >= 3:
            return T
    raise AssertionError("no number of trees puts three cells into one bucket")


@functools.lru_cache(maxsize=None)
def bucket_case():
    """(depth [1, 4, 256] of 1000 everywhere, labels, forest): BUCKET_TREES copies of refit_cases.column_tree(10, 4, 1024), so
    the 256 pixels of a row -- one workgroup -- end in 256 different slots of level 9 of every tree, below the six levels the
    LDS histogram holds for T6/C4."""
    m = BUCKET
    depth = np.full((1, m["H"], m["W"]), 1000, np.uint16)
    labels = np.repeat(np.array(BUCKET_ROW_LABELS, np.uint16), m["W"]).reshape(depth.shape)
    forest = np.stack([rc.column_tree(m["D"], m["C"], m["tree_width"])] * BUCKET_TREES)
    _freeze(depth, labels, forest)
    return depth, labels, forest
