"""Inputs of the front end's small device tests (tests/test_frontend.py): frames, planes and candidate sets that put
rdf_frame_front, rdf_gaussian_depth_filter, rdf_plane_inliers and rdf_plane_select on the edges of their rules
(include/rdf_frontend.h).  The CPU tests (do the cases bite?) and the GPU tests (the device against
tests/frontend_numpy.py) both call these builders, so that both see the same arrays.

CHAIN      the per-pixel chain on three planes whose last rows are (0, 0, 0, 1), (0, 0, 0, 2) and (0, 0, 0, 0), with depths that
           put z' on -T exactly and one unit above it; every expected image is worked by hand and a literal.
TIES       small frames against the Gaussian's tie w0 == wn, its corners (taps beyond the frame are skipped) and a window
           without weight.
SHAPES     three frames (odd frame offsets) smaller than the 32 x 8 tile, smaller than the half-width of k = 41, one more
           than a tile each way, and one pixel; with k = 0, 5 and 41.
SELECT     candidate counts whose best value stands at two indices beyond 256 (another lane of k_plane_select each), all
           -1, and all 0.
INLIERS    points on +-T, beside it, with w != 1 and NaN; candidates that count none.

MUTANTS names wrong readings of the rules, `mutant(name)` loads tests/frontend_numpy.py with that reading (tests/mutants.py),
KILLS says which device case must notice which."""
import functools
import importlib

import numpy as np

import frontend_numpy as fnp
import mutants

F = np.float32
T = 40.
EYE = np.identity(4, np.float32)


def gaussian_kernel(k, sigma):
    return importlib.import_module("3d-beats_amd.cuda.points_ops").gaussian_kernel(k, sigma)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


# ------------------------------------------------------------------ the per-pixel chain ---------------------------------------
# camera (ppx, ppy, f) = (0, 0, 1): x' = d * x, y' = d * y, exact.  Three frames of 5 x 3 (a frame's offset is odd).
CHAIN_CAM = (0., 0., 1.)
CHAIN_DEPTH = _freeze(np.array([[[0, 50, 60, 61, 200], [59, 60, 61, 62, 0], [1, 60, 0, 61, 65535]],
                                [[61, 61, 61, 61, 61], [61, 60, 60, 60, 61], [61, 61, 61, 61, 61]],
                                [[0, 0, 0, 0, 0], [0, 0, 60, 0, 0], [0, 0, 0, 0, 61]]], np.uint16))


def _chain_planes():
    lift = EYE.copy()
    lift[2, 3] = -100.              # z' = d - 100: -T exactly at d = 60 (kept: z' > -T is false), -39 at d = 61 (cut)
    w2 = EYE.copy()
    w2[3, 3] = 2.                   # w' = 2: never cut, depth kept, although z' = d > -T everywhere
    w0 = EYE.copy()
    w0[3, 3] = 0.                   # w' = 0: the depth is removed, the point is written as transformed
    return {"last row (0, 0, 0, 1), z' on -T": lift, "last row (0, 0, 0, 2)": w2, "last row (0, 0, 0, 0)": w0}


CHAIN_PLANES = _chain_planes()
# worked by hand, without the Gaussian: the cleaned depth ...
CHAIN_WANT_DEPTH = {
    "last row (0, 0, 0, 1), z' on -T": np.where(CHAIN_DEPTH <= 60, CHAIN_DEPTH, 0).astype(np.uint16),
    "last row (0, 0, 0, 2)": CHAIN_DEPTH,
    "last row (0, 0, 0, 0)": np.zeros_like(CHAIN_DEPTH),
}
UNIFORM3 = _freeze(np.full((3, 3), 1 / 9, np.float32))


def chain_want_points(name):
    """... and the points, by hand: (d x, d y, z', w') where the depth is not 0 and the point was not cut, else zeros."""
    d = CHAIN_DEPTH.astype(np.float32)
    y, x = np.mgrid[:3, :5].astype(np.float32)
    if name == "last row (0, 0, 0, 1), z' on -T":
        p = np.stack([d * x, d * y, d - F(100.), np.ones_like(d)], -1)
        keep = (CHAIN_DEPTH > 0) & (CHAIN_DEPTH <= 60)
    else:
        p = np.stack([d * x, d * y, d, np.full_like(d, 2. if name == "last row (0, 0, 0, 2)" else 0.)], -1)
        keep = CHAIN_DEPTH > 0
    return np.where(keep[..., None], p, F(0)).astype(np.float32)


# ------------------------------------------------------------------ the Gaussian's ties and corners ---------------------------
# (name, frame, weights).  In the first frame corner (0, 0) sees four taps, two of them 0: w0 == wn, the average stands; the
# five taps beyond the frame are skipped, not counted as holes.  Corner (2, 2): four taps, all 0.  Centre: 7 zeros against 2.
TIES = (
    ("a corner whose four taps tie", _freeze(np.array([[0, 10, 0], [30, 0, 0], [0, 0, 0]], np.uint16)), UNIFORM3),
    ("a window without weight", _freeze(np.array([[5]], np.uint16)), _freeze(np.zeros((1, 1), np.float32))),
    ("65535 under a weight above 1", _freeze(np.array([[65535]], np.uint16)), _freeze(np.array([[1.0000001]], np.float32))),
    ("an edge whose six taps tie", _freeze(np.array([[7, 0, 9, 0], [0, 8, 0, 0]], np.uint16)), UNIFORM3),
    # four large values in random places (found by a seeded search): the nine products' sum is within a rounding of a whole
    # multiple of wn at several pixels, so another order of addition, or a contracted product, gives the number below
    ("sums beside a whole number", _freeze(np.array([[31010, 31010, 62288, 62288, 31010, 33542, 62288],
                                                      [33542, 33542, 62288, 33542, 33542, 49490, 49490],
                                                      [31010, 31010, 62288, 62288, 62288, 49490, 62288],
                                                      [33542, 33542, 62288, 31010, 33542, 31010, 33542],
                                                      [62288, 31010, 33542, 33542, 62288, 31010, 49490],
                                                      [33542, 31010, 62288, 31010, 33542, 33542, 33542]], np.uint16)), UNIFORM3),
)
TIES_WANT = {"a corner whose four taps tie": [[20, 0, 0], [0, 0, 0], [0, 0, 0]],          # worked by hand
             "a window without weight": [[0]], "65535 under a weight above 1": [[65535]]}
FAR_BELOW = EYE.copy()
FAR_BELOW[2, 3] = -1e6               # z' = d - 10^6: nothing is cut, the cleaned frame is the frame


# ------------------------------------------------------------------ shapes ----------------------------------------------------
SHAPES = ((19, 5), (13, 11), (33, 9), (1, 1))           # (W, H): every W * H is odd
SHAPE_N, SHAPE_K = 3, (0, 5, 41)
SHAPE_CAM = (4.25, 2.5, 30.)


@functools.lru_cache(maxsize=None)
def shape_case(W, H):
    """(depth uint16 [3, H, W], plane [4, 4]): depths around 600 with holes, a slightly tilted plane 600 away, so that
    about half of the pixels are cut."""
    rng = np.random.default_rng(W * 100 + H)
    depth = rng.integers(500, 700, (SHAPE_N, H, W)).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.15] = 0
    if W * H == 1:
        depth[:, 0, 0] = (520, 0, 680)
    plane = EYE.copy()
    plane[2] = (0.02, -0.03, 1., -640.)
    return _freeze(depth, plane)


@functools.lru_cache(maxsize=None)
def shape_weights(k):
    return None if k == 0 else _freeze(np.ascontiguousarray(gaussian_kernel(k, 2.0), np.float32))


# ------------------------------------------------------------------ plane_select ----------------------------------------------
SELECT_G = 600


def _select_candidates():
    cand = np.tile(EYE.reshape(16), (SELECT_G, 1))
    cand[:, 4] = np.arange(SELECT_G)                    # M[1][0] tells which candidate a plane was
    cand[:, 3], cand[:, 7] = 3., 0.5                    # (recentring takes c[0] = 3 and c[1] = 0.5 off these two)
    cand[:, 10], cand[:, 11] = 2., -8.                  # t = 4, c[2] = 0 exactly
    return _freeze(cand.astype(np.float32))


def _select_counts():
    rng = np.random.default_rng(600)
    tie = rng.integers(0, 900, SELECT_G).astype(np.int32)
    tie[[300, 520, 599]] = 1000                         # lanes 44, 8 and 87 of 256: the lowest index is in none of the first
    one = np.full(SELECT_G, -1, np.int32)
    zero = np.zeros(SELECT_G, np.int32)
    late = tie.copy()
    late[[300, 520]] = 5                                # the best is the last candidate
    return {"equal best counts at 300, 520 and 599": _freeze(tie), "every count -1": _freeze(one), "every count 0": _freeze(zero),
            "the best is the last": _freeze(late)}


SELECT_CANDIDATES = _select_candidates()
SELECT_COUNTS = _select_counts()
SELECT_WANT_BEST = {"equal best counts at 300, 520 and 599": (300, 1000, 0), "every count -1": (0, -1, 1), "every count 0": (0, 0, 1),
                    "the best is the last": (599, 1000, 0)}            # (best_index, best_count, status), by hand
PLANE_IN = _freeze(np.full(16, 5., np.float32))


# ------------------------------------------------------------------ inliers ---------------------------------------------------
def inlier_case():
    """(pts [8, 4], candidates [4, 16], counts before): +-T exactly is out, just inside is in, w != 1, NaN and inf never
    count; a candidate without inliers keeps its count."""
    M = EYE.reshape(16).copy()
    pts = np.array([[0, 0, T, 1], [0, 0, -T, 1], [0, 0, np.nextafter(np.float32(T), 0), 1], [0, 0, -39.5, 1],
                    [0, 0, 0, 2], [0, 0, 0, 0], [np.nan, 0, 0, 1], [0, np.inf, 0, 1]], np.float32)
    far = M.copy()
    far[11] = 1e6
    nan = np.full(16, np.nan, np.float32)
    return pts, np.stack([M, far, nan, M]), np.array([0, 5, -1, 3], np.int32)


INLIER_WANT = [2, 5, -1, 5]


# ------------------------------------------------------------------ mutants ---------------------------------------------------
EDITS = {
    "cut read as z' >= -T": [("gone = (depth == 0) | ((q[..., 3] == 1) & (q[..., 2] > -F(T)))", "gone = (depth == 0) | ((q[..., 3] == 1) & (q[..., 2] >= -F(T)))")],
    "cut whatever w' is": [("gone = (depth == 0) | ((q[..., 3] == 1) & (q[..., 2] > -F(T)))", "gone = (depth == 0) | (q[..., 2] > -F(T))")],
    "w' == 0 keeps the depth": [("clean = np.where(gone | (q[..., 3] == 0), 0, depth)", "clean = np.where(gone, 0, depth)")],
    "a point with w' == 0 is zeroed": [("pts = np.where(gone[..., None], F(0), q)", "pts = np.where((gone | (q[..., 3] == 0))[..., None], F(0), q)")],
    "a cut point keeps its coordinates": [("pts = np.where(gone[..., None], F(0), q)", "pts = np.where((depth == 0)[..., None], F(0), q)")],
    "matrix rows summed left to right": [("return (r[0] * x + r[1] * y) + (r[2] * z + r[3] * w)", "return ((r[0] * x + r[1] * y) + r[2] * z) + r[3] * w")],
    "Gaussian tie read as w0 >= wn": [("return np.where(w0 > wn, 0,", "return np.where(w0 >= wn, 0,")],
    "taps outside the frame are holes": [("zero = ok & (d == 0)", "zero = (d == 0)")],
    "Gaussian rounded, not floored": [("q = np.floor(np.asarray(v, np.float32)).astype(np.float64)", "q = np.floor(np.asarray(v, np.float32) + F(0.5)).astype(np.float64)")],
    "Gaussian summed column first": [("    for dy in range(k):\n        for dx in range(k):", "    for dx in range(k):\n        for dy in range(k):")],
    "Gaussian product contracted": [("s = np.where(non, s + d.astype(np.float32) * wt, s)", "s = np.where(non, _fma(d.astype(np.float32), wt, s), s)")],
    "Gaussian NaN read as 65535": [("q = np.where(np.isnan(q) | (q < 0), 0, np.minimum(q, 4294967295.0))", "q = np.where(np.isnan(q), 65535, np.where(q < 0, 0, np.minimum(q, 4294967295.0)))")],
    "inlier test read as |z'| <= T": [("(zz.abs_() < float(T))", "(zz.abs_() <= float(T))"), ("((zz < T) & (zz > -T))", "((zz <= T) & (zz >= -T))")],
    "points with any w != 0 count": [("P = P[P[:, 3] == 1]", "P = P[P[:, 3] != 0]")],
    "a candidate without inliers is reset": [("return np.where(out > 0, base + out, base).astype(np.int32)", "return np.where(out > 0, base + out, 0).astype(np.int32)")],
    "best count ties to the highest index": [("best = int(np.argmax(counts))", "best = len(counts) - 1 - int(np.argmax(counts[::-1]))")],
    "a best count of 0 is a plane": [("ok = counts[best] > 0 and", "ok = counts[best] >= 0 and")],
    "a best count of -1 is a plane": [("ok = counts[best] > 0 and", "ok = counts[best] != 0 and")],
}
MUTANTS = tuple(EDITS)
EQUIVALENT = {}


@functools.lru_cache(maxsize=None)
def mutant(name=None):
    """tests/frontend_numpy.py under one wrong reading; the unchanged copy without a name."""
    return mutants.load("frontend_numpy", EDITS[name] if name else ())


def _select_record(mod, counts):
    plane, best, count, c, status = mod.plane_select(SELECT_CANDIDATES, counts, PLANE_IN)
    return [plane, np.array([best, count, status], np.int64), np.asarray(c, np.float64)]


def outputs(mod, name):
    """What the device tests of case `name` compare, under the restatement module `mod`: a list of arrays."""
    out = []
    with np.errstate(all="ignore"):
        if name in CHAIN_PLANES:
            for w in (None, UNIFORM3):
                out += list(mod.frame_front(CHAIN_DEPTH, *CHAIN_CAM, CHAIN_PLANES[name], T, w))
        elif name in [t[0] for t in TIES]:
            frame, w = [t[1:] for t in TIES if t[0] == name][0]
            out += [mod.gaussian(frame, w), mod.frame_front(frame[None], *CHAIN_CAM, FAR_BELOW, T, w)[0]]
        elif name.startswith("shape "):
            W, H = (int(v) for v in name[6:].split(" x "))
            depth, plane = shape_case(W, H)
            for k in SHAPE_K:
                got = mod.frame_front(depth, *SHAPE_CAM, plane, T, shape_weights(k))
                out += list(got)
                if k:
                    out.append(mod.gaussian(mod.frame_front(depth, *SHAPE_CAM, plane, T)[0][1], shape_weights(k)))
        elif name in SELECT_COUNTS:
            out += _select_record(mod, SELECT_COUNTS[name])
        elif name == "inlier edge points":
            pts, cand, init = inlier_case()
            out.append(mod.plane_inliers(pts, cand, T, init))
        else:
            raise KeyError(name)
    return out


# device case -> the mutants it must kill
KILLS = {
    "last row (0, 0, 0, 1), z' on -T": ("cut read as z' >= -T", "a cut point keeps its coordinates"),
    "last row (0, 0, 0, 2)": ("cut whatever w' is",),
    "last row (0, 0, 0, 0)": ("w' == 0 keeps the depth", "a point with w' == 0 is zeroed"),
    "a corner whose four taps tie": ("Gaussian tie read as w0 >= wn", "taps outside the frame are holes"),
    "a window without weight": ("Gaussian NaN read as 65535",),
    "65535 under a weight above 1": (),
    "an edge whose six taps tie": ("Gaussian tie read as w0 >= wn", "taps outside the frame are holes", "Gaussian rounded, not floored"),
    "sums beside a whole number": ("Gaussian summed column first", "Gaussian product contracted"),
    "shape 19 x 5": ("matrix rows summed left to right", "a cut point keeps its coordinates", "taps outside the frame are holes",
                     "Gaussian rounded, not floored"),
    "shape 13 x 11": ("matrix rows summed left to right", "a cut point keeps its coordinates", "taps outside the frame are holes",
                      "Gaussian rounded, not floored"),
    "shape 33 x 9": ("matrix rows summed left to right", "a cut point keeps its coordinates", "taps outside the frame are holes",
                     "Gaussian rounded, not floored"),
    "shape 1 x 1": ("matrix rows summed left to right", "taps outside the frame are holes"),
    "equal best counts at 300, 520 and 599": ("best count ties to the highest index",),
    "every count -1": ("a best count of -1 is a plane", "best count ties to the highest index"),
    "every count 0": ("a best count of 0 is a plane", "best count ties to the highest index"),
    "the best is the last": (),
    "inlier edge points": ("inlier test read as |z'| <= T", "points with any w != 0 count", "a candidate without inliers is reset"),
}
