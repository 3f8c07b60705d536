"""The cases of tests/test_shape.py: seeded numpy builders, cached and frozen, that the CPU tests and the GPU tests both call, so
that both see the same arrays.  The pool cases are the smallest shapes at which k_shape_pool can go wrong: 335 label pixels an
image (waves straddle images), widths that labels_reduce does not divide, every class capacity with padding lanes, an image
without a live pixel between two with, PDFs no trainer writes (dead pixels, shares that clamp), the adversarial walk of
walk_cases.py, a filter.  The decide cases are literal pool rows.

EDITS names wrong readings of rules G, `mutant(name)` loads tests/shape_numpy.py with that reading (tests/mutants.py),
`outputs(mod, name)` computes what the device test of case `name` compares, and KILLS says which case notices which reading."""
import functools

import numpy as np

import mutants
import posterior_cases as pc
import walk_cases as wc

NO_PIXEL = 65535


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ------------------------------------------------------------ the case worked by hand -----------------------------------------
def hand_case():
    """T = 1, D = 1, C = 2 on one 7 x 1 frame.  The root probes (x + 1, y) against the pixel itself at depth 1000 (offset 1000),
    thresh 50: left is the leaf [.75, .25], right the leaf [.5, .5], a tie."""
    depth = np.array([[[1000, 1000, 1100, 1000, 1000, 65535, 0]]], np.uint16)
    forest = np.zeros((1, 1, 7 + 2 * 2), np.float32)
    forest[0, 0, :7] = [1000., 0., 0., 0., 50., 0., 0.]
    forest[0, 0, 7:] = [.75, .25, .5, .5]
    return depth, forest


# ------------------------------------------------------------ the pool cases ---------------------------------------------------
# id: n, H, W, r, scale, T, D, C, filter class or None, forest kind, the image that is blanked or None
POOL = {
    "w67_n3":      (3, 5, 67, 1, 1.0, 2, 4, 3, None, "trained", None),
    "w131_r2_c5":  (2, 7, 131, 2, 0.5, 2, 6, 5, 2, "sharp", None),
    "w131_r3_c16": (1, 7, 131, 3, 1.0, 2, 5, 16, None, "trained", None),
    "w67_c2":      (3, 5, 67, 1, 1.0, 3, 3, 2, None, "sharp", 1),
    "awkward":     (3, 3, 65, 1, 1.0, 2, 2, 3, None, "awkward", None),
    "c9":          (1, 4, 130, 1, 1.0, 2, 3, 9, None, "trained", None),
    "order":       (1, 2, 65, 1, 1.0, 1, 1, 3, None, "order", None),
}


@functools.lru_cache(maxsize=None)
def pool_case(name):
    """(depth, forest, kwargs of shape_numpy.pool)."""
    n, h, w, r, scale, T, D, C, fclass, fkind, blank = POOL[name]
    seed = sorted(POOL).index(name)
    depth = pc.live_rows(700 + 10 * seed, n, h, w)
    if blank is not None:
        depth[blank] = NO_PIXEL
        depth[blank, 0, :3] = 0                               # (holes are no pixels either)
    forest = {"awkward": pc.awkward_forest, "order": order_forest, "sharp": lambda: pc.sharp_forest(T, D, C, 200 + 5 * seed),
              "trained": lambda: pc.trained_like(T, D, C, 200 + 5 * seed)}[fkind]()
    assert forest.shape == (T, (1 << D) - 1, 7 + 2 * C)
    filt = None if fclass is None else pc.filter_image(50 + seed, (n, h // r, w // r), fclass)
    _freeze(depth, forest, filt)
    return depth, forest, dict(labels_reduce=r, scale=scale, filter_images=filt, filter_class=fclass)


def order_forest():
    """T = 1, D = 1, C = 3, both leaves [2^-24, 2^-24, 1]: in class order S = (2^-24 + 2^-24) + 1 = 1 + 2^-23, a float; from the
    other end 1 + 2^-24 rounds back to 1 (a tie, to even) twice and S = 1.  The last class's share is floor(65535 / (1 + 2^-23)) =
    65534 under the rule and 65535 under the other order."""
    forest = np.zeros((1, 1, 7 + 2 * 3), np.float32)
    forest[0, 0, 7:] = [2. ** -24, 2. ** -24, 1.] * 2
    return forest


def adversarial_runs():
    """The planted-flag forest and the off-range offsets of walk_cases.adversarial_case(): (depth, forest, kwargs) at scale 3.0
    (some products overflow) and at r = 2, scale 0.5 under walk_cases.adversarial_filter()."""
    depth, _, forest, _ = wc.adversarial_case()
    return [(depth, forest, dict(labels_reduce=1, scale=3.0, filter_images=None, filter_class=None)),
            (depth, forest, dict(labels_reduce=2, scale=0.5, filter_images=wc.adversarial_filter(), filter_class=wc.ADV["filter_class"]))]


BIG = dict(H=300, W=300)       # one single-class frame: 90 000 shares of 65 535 pass 2^32


def big_case():
    """(depth [1, 300, 300] of 900 everywhere, a T1/D1/C1 forest whose two leaves are [1.0], the pool row as a literal)."""
    depth = np.full((1, BIG["H"], BIG["W"]), 900, np.uint16)
    forest = np.zeros((1, 1, 9), np.float32)
    forest[0, 0, 7:] = 1.
    n = BIG["H"] * BIG["W"]
    return depth, forest, np.array([[n * 65535, n, n, 0]], np.uint64)


def chunk_case():
    """Five frames for max_frames = 2: (depth, forest, kwargs)."""
    depth = pc.live_rows(820, 5, 4, 67)
    forest = pc.sharp_forest(2, 4, 4, 260)
    _freeze(depth, forest)
    return depth, forest, dict(labels_reduce=1, scale=1.0, filter_images=None, filter_class=None)


# ------------------------------------------------------------ the decide cases -------------------------------------------------
def rows(C, *frames):
    """Pool rows from (soft sums, voting pixels) pairs; the hard votes and the dead count play no part in rules G6 and G7."""
    out = np.zeros((len(frames), 2 * C + 2), np.uint64)
    for f, (soft, live) in enumerate(frames):
        out[f, :C] = soft
        out[f, 2 * C] = live
    return out


A, B, THIRD, NONE, WEAK = ([900, 100, 0], 10), ([100, 900, 0], 10), ([0, 100, 900], 10), ([0, 0, 0], 0), ([340, 330, 330], 10)
# name: (C, frames, settings of shape_numpy.decide, want (raw, conf, held, changed) per frame)
CONF_A, CONF_WEAK = 58981, 22281       # floordiv(900 * 65535, 1000) = 58981 (.5); floordiv(340 * 65535, 1000) = 22281 (.9)
DECIDE = {
    # a switch after exactly `hold` frames: B is held from its third frame on, and a fourth changes nothing
    "switch": (3, [A, A, A, B, B, B, B], dict(min_pixels=1, hold=3),
               [(0, CONF_A, -1, 0), (0, CONF_A, -1, 0), (0, CONF_A, 0, 1), (1, CONF_A, 0, 0), (1, CONF_A, 0, 0), (1, CONF_A, 1, 1),
                (1, CONF_A, 1, 0)]),
    # an interrupted candidate starts again: B, THIRD, B, B under hold 2 switches at the last frame only; an invalid frame
    # interrupts too
    "interrupted": (3, [A, A, B, THIRD, B, B, A, NONE, A, A], dict(min_pixels=1, hold=2),
                    [(0, CONF_A, -1, 0), (0, CONF_A, 0, 1), (1, CONF_A, 0, 0), (2, CONF_A, 0, 0), (1, CONF_A, 0, 0), (1, CONF_A, 1, 1),
                     (0, CONF_A, 1, 0), (-1, 0, 1, 0), (0, CONF_A, 1, 0), (0, CONF_A, 0, 1)]),
    # release 2: two frames without a valid shape let go; one does not, and a valid frame between them resets the count
    "release": (3, [A, NONE, A, NONE, NONE, NONE, A], dict(min_pixels=1, hold=1, release=2),
                [(0, CONF_A, 0, 1), (-1, 0, 0, 0), (0, CONF_A, 0, 0), (-1, 0, 0, 0), (-1, 0, -1, 1), (-1, 0, -1, 0), (0, CONF_A, 0, 1)]),
    # release 0 never lets go
    "no_release": (3, [A, NONE, NONE, NONE], dict(min_pixels=1, hold=1, release=0),
                   [(0, CONF_A, 0, 1), (-1, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 0, 0)]),
    # min_conf: a raw shape below it is reported and not valid; at it, valid
    "min_conf": (3, [WEAK, WEAK], dict(min_pixels=1, hold=1, min_conf=CONF_WEAK + 1),
                 [(0, CONF_WEAK, -1, 0), (0, CONF_WEAK, -1, 0)]),
    "min_conf_met": (3, [WEAK], dict(min_pixels=1, hold=1, min_conf=CONF_WEAK), [(0, CONF_WEAK, 0, 1)]),
    # min_pixels is <: 10 voting pixels pass min_pixels 10 and fail 11; total == 0 with pixels enough is -1 too
    "min_pixels": (3, [A, ([0, 0, 0], 50)], dict(min_pixels=10, hold=1), [(0, CONF_A, 0, 1), (-1, 0, 0, 0)]),
    "min_pixels_missed": (3, [A], dict(min_pixels=11, hold=1), [(-1, 0, -1, 0)]),
    # the first greatest: equal sums give the lower class, also when the greatest comes last
    "ties": (4, [([5, 7, 7, 1], 3), ([7, 7, 7, 7], 3), ([0, 0, 3, 3], 3), ([1, 2, 3, 9], 3)], dict(min_pixels=1, hold=1),
             [(1, 22937, 1, 1), (0, 16383, 0, 1), (2, 32767, 2, 1), (3, 39321, 3, 1)]),
    # sums beyond 2^32 and a product beyond 2^62: (2^31 - 1) * 65535 pixels' worth of shares in one class
    "wide": (2, [([(2 ** 31 - 1) * 65535, 1], 2 ** 31 - 1), ([2 ** 40, 2 ** 41], 5)], dict(min_pixels=1, hold=1),
             [(0, 65534, 0, 1), (1, 43690, 1, 1)]),
}


def decide_case(name):
    C, frames, settings, want = DECIDE[name]
    return C, rows(C, *frames), settings, np.array(want, np.int32)


SPLITS = {"switch": 2, "interrupted": 5, "release": 4}        # a split call equals one call: where these traces are cut


# ------------------------------------------------------------ wrong readings of rules G ----------------------------------------
EDITS = {
    "S == 0 votes": [("if not (S > f32(0.)):", "if not (S >= f32(0.)):")],
    "label ties go up": [("if acc[c] > best:", "if acc[c] >= best:")],
    "S in reverse class order": [("for c in range(acc.shape[0]):\n            S = f32(S + acc[c])",
                                  "for c in reversed(range(acc.shape[0])):\n            S = f32(S + acc[c])")],
    "shares not clamped above": [("q.append(min(max(v, 0), 65535))", "q.append(max(v, 0))")],
    "shares round to nearest": [("v = rn.floor_i32(f32(f32(acc[c] / S) * f32(65535.)))",
                                 "v = rn.floor_i32(f32(f32(f32(acc[c] / S) * f32(65535.)) + f32(.5)))")],
    "the pool overwrites": [("if pool is None else pool\n", "if pool is None else np.zeros_like(pool)\n")],
    "a dead pixel is a voting pixel": [("        row[2 * C + 1] += one\n        return", "        row[2 * C] += one\n        return")],
    "hard votes are not counted": [("    row[C + label_of(acc)] += one\n", "")],
    "the filter is ignored": [("if filter_images is not None and int(filter_images[i, y, x]) != int(filter_class):",
                               "if False:")],
    "raw ties go up": [("if soft[c] > soft[best]:", "if soft[c] >= soft[best]:")],
    "conf rounds to nearest": [("(soft[best] * 65535) // total", "(soft[best] * 65535 + total // 2) // total")],
    "min_pixels is <=": [("int(row[2 * C]) < min_pixels", "int(row[2 * C]) <= min_pixels")],
    "min_conf is >": [("raw != -1 and conf >= min_conf", "raw != -1 and conf > min_conf")],
    "hold is >": [("if run >= hold:", "if run > hold:")],
    "an interrupted candidate keeps its run": [("candidate, run = raw, 1", "candidate, run = raw, run + 1")],
    "an invalid frame keeps the candidate": [("        candidate, run = -1, 0\n        miss = min(miss + 1, MISS_MAX)",
                                              "        miss = min(miss + 1, MISS_MAX)")],
    "miss is never reset": [("        miss = 0\n", "        pass\n")],
    "release is >": [("miss >= release and held != -1", "miss > release and held != -1")],
    "release 0 lets go": [("if release > 0 and miss", "if miss")],
    "held is reported before the frame": [("out[f] = (raw, conf, state[0], changed)", "out[f] = (raw, conf, before, changed)"),
                                          ("        state, changed = hold_step(", "        before = state[0]\n        state, changed = hold_step(")],
}
MUTANTS = tuple(EDITS)


@functools.lru_cache(maxsize=None)
def mutant(name):
    return mutants.load("shape_numpy", EDITS[name] if name else ())


def outputs(mod, name):
    """What the device test of case `name` compares, from the restatement (or a mutant of it) `mod`: a tuple of arrays."""
    if name == "hand":
        depth, forest = hand_case()
        pool = mod.pool(depth, forest)
        return (pool,) + tuple(mod.decide(pool, 2, min_pixels=5, hold=1))
    if name in POOL:
        depth, forest, kw = pool_case(name)
        pool = mod.pool(depth, forest, **kw)
        C = (forest.shape[2] - 7) // 2
        return (pool,) + tuple(mod.decide(pool, C, min_pixels=1, hold=1))
    if name == "adds":
        depth, forest, kw = pool_case("w67_n3")
        pool = mod.pool(depth, forest, **kw)
        first = pool.copy()
        again = mod.pool(depth, forest, pool=pool, **kw)
        return first, np.ascontiguousarray(again)
    if name.startswith("decide:"):
        C, pool, settings, _ = decide_case(name[7:])
        return tuple(mod.decide(pool, C, **settings))
    raise KeyError(name)


# which case must notice which reading (exact: tests/test_shape.py compares the sets).  Every case's outputs end in the state after
# its last frame, so readings of rule G7 that leave the rows alone still show; "hold is >" changes every case decided at hold 1.
_ROWS = ["hold is >", "held is reported before the frame"]
_POOLED = ["shares round to nearest", "hard votes are not counted"]
KILLS = {
    "hand": _POOLED + _ROWS + ["label ties go up", "min_pixels is <="],
    "w67_n3": _POOLED + _ROWS + ["conf rounds to nearest"],
    "w131_r2_c5": _POOLED + _ROWS + ["the filter is ignored", "conf rounds to nearest"],
    "w131_r3_c16": _POOLED + _ROWS + ["conf rounds to nearest"],
    # (the image without a live pixel is an invalid frame between two valid ones)
    "w67_c2": _POOLED + _ROWS + ["conf rounds to nearest", "miss is never reset", "release 0 lets go"],
    "awkward": _ROWS + ["S == 0 votes", "shares not clamped above", "a dead pixel is a voting pixel", "hard votes are not counted"],
    "c9": _POOLED + _ROWS + ["conf rounds to nearest"],
    "order": _POOLED + _ROWS + ["S in reverse class order"],
    "adds": _POOLED + ["the pool overwrites"],
    "decide:switch": _ROWS + ["conf rounds to nearest"],
    "decide:interrupted": _ROWS + ["conf rounds to nearest", "an interrupted candidate keeps its run", "an invalid frame keeps the candidate",
                                   "miss is never reset", "release 0 lets go"],
    "decide:release": _ROWS + ["conf rounds to nearest", "miss is never reset", "release is >"],
    "decide:no_release": _ROWS + ["conf rounds to nearest", "release 0 lets go"],
    "decide:min_conf": ["conf rounds to nearest"],
    "decide:min_conf_met": _ROWS + ["conf rounds to nearest", "min_conf is >"],
    "decide:min_pixels": _ROWS + ["conf rounds to nearest", "min_pixels is <=", "release 0 lets go"],
    "decide:min_pixels_missed": [],
    "decide:ties": _ROWS + ["raw ties go up", "conf rounds to nearest"],
    "decide:wide": _ROWS + ["conf rounds to nearest"],
}
EQUIVALENT = {}
