"""Inputs of tests/test_soft_modes.py: small pure functions that the CPU tests (hand-worked answers, preconditions, the
restatement's own error) and the GPU tests (the kernels against the restatement) both call, so that both see the same arrays.
Every reference is computed once, shared and left unchanged (read-only arrays).

TAB_CAP is the kernel's kTabCap (csrc/rdf_modes.hpp); the list cap is read from the library
(rdf_labels_weighted_modes_list_cap) and handed in by the GPU tests, CAP_FOR_CPU is what the CPU tests build the same cases from."""
import functools

import numpy as np

import soft_modes_numpy as sn

NO_LABEL = 65535
PREFILL = 0xABCD
TAB_CAP = 3072
BOUND_PX = 1e-9             # the project's bound for the mean-shift row against its restatement
OFFSETS = (1, 2, 3, 4, 5, 6, 7)     # elements past a 16-byte boundary: every one takes the scalar lister

# ------------------------------------------------------------ composite weights -------------------------------------------------
# layer 0 answers 1..4: 1 and 3 are final, 2 goes on at offset 4, 4 at offset 7.  Layer 1 from offset 4 answers 1..3 (entries 4..6:
# final, on to offset 9, final), from offset 7 answers 1..2 (entries 7, 8: final, on to offset 9).  Layer 2 from offset 9 answers
# 1..2 (entries 9, 10).  Labels 5 and 9 in layer 0 reach entries of the later groups (the walk does not care), 200 leaves the table,
# and from offset 4 or more a 9 leaves it too.
COND = ((0, 1), (1, 4), (0, 2), (1, 7), (0, 3), (1, 9), (0, 4), (0, 5), (1, 9), (0, 6), (0, 7))
WEIGHT_SHAPES = ((1, 1, 1), (1, 5, 7), (3, 33, 65), (2, 61, 130))
SPECIAL_CONF = (0, 1, 255, 32767, 32768, 65534, 65535)


@functools.lru_cache(maxsize=None)
def weights_case(shape, n_layers=3):
    """(labels, conf): n_layers read-only uint16 maps of `shape` each.  Labels from {0, 65535, 1, 2, 3, 4, 5, 9, 200}; half of the
    confidences from SPECIAL_CONF, half random.  The one-pixel shape starts a two-layer path."""
    rng = np.random.default_rng(shape[0] * 100000 + shape[1] * 1000 + shape[2])
    pool = np.array([0, NO_LABEL, 1, 1, 2, 2, 2, 3, 4, 4, 5, 9, 200], np.uint16)
    labels, conf = [], []
    for j in range(n_layers):
        lab = pool[rng.integers(0, pool.size, size=shape)]
        k = rng.integers(0, 65536, size=shape).astype(np.uint16)
        special = rng.random(shape) < 0.5
        k[special] = np.array(SPECIAL_CONF, np.uint16)[rng.integers(0, len(SPECIAL_CONF), size=int(special.sum()))]
        if shape == (1, 1, 1):
            lab[...] = (2, 1, 1)[j]
            k[...] = (32768, 32768, 7)[j]
        lab.setflags(write=False)
        k.setflags(write=False)
        labels.append(lab)
        conf.append(k)
    return tuple(labels), tuple(conf)


@functools.lru_cache(maxsize=None)
def weights_answer(shape, n_layers, flip_x):
    labels, conf = weights_case(shape)
    out, written = sn.composite_weights(labels[:n_layers], conf[:n_layers], COND, flip_x, PREFILL)
    out.setflags(write=False)
    written.setflags(write=False)
    return out, written


# ------------------------------------------------------------ weighted modes ----------------------------------------------------
def blob_labels(seed, h, w, n_classes, absent=()):
    """Ellipses of one class each with three outliers nearby, a label 0 and a label beyond the classes; 65535 elsewhere."""
    rng = np.random.default_rng(seed)
    lab = np.full((h, w), NO_LABEL, np.uint16)
    yy, xx = np.mgrid[0:h, 0:w]
    for c in range(1, n_classes + 1):
        if c in absent:
            continue
        cx, cy = rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.2 * h, 0.8 * h)
        a, b = rng.uniform(0.04, 0.12) * w, rng.uniform(0.06, 0.2) * h
        lab[((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1] = c
        for _ in range(3):      # (within a quarter of the map of the centre: far outliers would sit in the band the CPU test excludes)
            oy, ox = cy + rng.uniform(-0.25, 0.25) * h, cx + rng.uniform(-0.25, 0.25) * w
            lab[int(np.clip(oy, 0, h - 1)), int(np.clip(ox, 0, w - 1))] = c
    lab[0, 0] = 0
    lab[min(1, h - 1), min(1, w - 1)] = 60000
    return lab


def random_weights(seed, shape):
    """A tenth 0, a tenth each of 1 and 65535, the rest uniform."""
    rng = np.random.default_rng(seed)
    wts = rng.integers(1, 65536, size=shape).astype(np.uint16)
    u = rng.random(shape)
    wts[u < 0.1] = 0
    wts[(u >= 0.1) & (u < 0.2)] = 1
    wts[(u >= 0.2) & (u < 0.3)] = 65535
    return wts


WRAP_CASES = ((9, 8, 27, 8), (7, 9, 3, 13), (5, 15, 35, 0))      # h, w, the seeds of the labels and of the weights


def wrap_case(h, w, label_seed, weight_seed):
    """Two classes on a map whose rows are just wide enough for the lister's unrolled write-out (dim_x >= 8): at width 8 a
    lane's eight pixels are exactly a row, at 9 and 15 they wrap once, at a different pixel in every lane.  Some pixels of the
    classes have weight 0 (they take no slot: the slots after them move up) and every class keeps a counted pixel."""
    lab, wts = blob_labels(label_seed, h, w, 2), random_weights(weight_seed, (h, w))
    on = (lab == 1) | (lab == 2)
    assert w >= 8 and (wts[on] == 0).any() and all(((lab == k) & (wts != 0)).any() for k in (1, 2))
    return lab, wts


def _raster_class(lab, label, start, count, holes):
    flat = lab.reshape(-1)
    idx = np.setdiff1d(np.arange(start, start + count + len(holes)), np.asarray(holes, np.int64))[:count]
    assert idx.size == count
    flat[idx] = label
    return idx


CAP_SHAPE = (129, 257)


def cap_image(cap, n_class, n_zero):
    """Class 1 = n_class pixels in raster order from pixel 0 on but for six holes (the cap then falls inside a lane's eight
    pixels), n_zero of them with weight 0 (one early, one just before the cap); class 2 a small blob after it; class 3 absent."""
    h, w = CAP_SHAPE
    lab = np.full((h, w), NO_LABEL, np.uint16)
    idx = _raster_class(lab, 1, 0, n_class, (3, 100, 5000, 15001, cap - 8, cap - 3))
    assert idx[-1] < 127 * w
    lab[127, 200:230] = 2
    lab[128, 200:230] = 2
    lab[128, 0] = 0
    lab[128, 256] = 4
    wts = random_weights(cap, (h, w))        # (the same map for every n_class: class 2's pixels weigh the same)
    wts[wts == 0] = 9
    zeros = [int(idx[17]), int(idx[cap - 5])][:n_zero]
    wts.reshape(-1)[zeros] = 0
    assert int(((lab == 1) & (wts != 0)).sum()) == n_class - n_zero
    return lab, wts


def both_over_cap_image(cap):
    h, w = 200, 400
    lab = np.full((h, w), NO_LABEL, np.uint16)
    a = _raster_class(lab, 1, 0, cap + 1521, (9, 4000, 13333))
    b = _raster_class(lab, 2, int(a[-1]) + 998, cap + 523, (int(a[-1]) + 1000, int(a[-1]) + 2001))
    assert b[-1] < 190 * w
    lab[190:195, 300:320] = 3
    wts = random_weights(cap, (h, w))
    wts[wts == 0] = 3
    return lab, wts


def table_boundary(w):
    """The same blobs, weights and variances at (3, 3069) -- dim_x + dim_y = 3072: tables -- and (3, 3070): one exp per pixel."""
    lab = np.full((3, w), NO_LABEL, np.uint16)
    lab[0:3, 100:141] = 1
    lab[1, 90] = 1
    lab[0:2, 1000:1011] = 2
    lab[1:3, 1030:1041] = 2
    lab[0:3, 3060:3069] = 3
    lab[2, 0] = 4
    wts = np.full((3, w), 5, np.uint16)
    wts[:, :3069] = random_weights(3069, (3, 3069))
    return lab, wts


BATCH = 16 * 13 * 512       # pixels the sixteen waves list per batch (kModesWaves * kSteps * 512): larger maps take the lister's outer loop
BATCH_SHAPES = ((5, 21301), (4, 53253))
assert 5 * 21301 == BATCH + 9 and 2 * BATCH < 4 * 53253 < 3 * BATCH


def scattered(seed, h, w, L=8):
    """Labels drawn from 1 .. L, 0, L + 1 and 65535 (twice): every class all over the map, in every batch of the lister."""
    rng = np.random.default_rng(seed)
    pool = np.array(list(range(1, L + 1)) + [0, L + 1, NO_LABEL, NO_LABEL], np.uint16)
    return pool[rng.integers(0, pool.size, size=(h, w))]


def wide_variances(w, L):
    """Wide enough for pixels scattered over a row of w to keep every exponent above -600 (no tables on these maps: the CPU test
    asserts it)."""
    return (w / 24.0 + 0.125 * np.arange(L)).astype(np.float32)


def batches_image(cap):
    """(4, 53253): two batches and a third of 20 pixels.  Class 1 crosses the cap inside batch 0 (a raster run from pixel 0 on) and has pixels in the later
    batches too; class 2 has no pixel in batch 0 and is listed from the later ones; class 3 is listed from both full batches; class 4
    is under the cap after batch 0 and crosses it in batch 1 (a raster run there); classes 5 .. 8 are listed like class 3."""
    h, w = BATCH_SHAPES[1]
    lab = scattered(77, h, w)
    flat = lab.reshape(-1)
    head = flat[:BATCH]
    head[head == 2] = NO_LABEL
    _raster_class(lab, 1, 0, cap + 301, (5, 1000, cap - 2))
    _raster_class(lab, 4, BATCH + 1000, 12000, (BATCH + 1003, BATCH + 9000))
    wts = random_weights(78, (h, w))
    counted = lambda c, sl: int(((flat[sl] == c) & (wts.reshape(-1)[sl] != 0)).sum())
    b0, rest = slice(0, BATCH), slice(BATCH, None)
    assert counted(1, b0) > cap and counted(1, rest) > 100
    assert counted(2, b0) == 0 and 100 < counted(2, rest) <= cap
    assert counted(4, b0) <= cap < counted(4, b0) + counted(4, slice(BATCH, 2 * BATCH))
    assert all(100 < counted(c, b0) and counted(c, b0) + counted(c, rest) <= cap and counted(c, slice(BATCH, 2 * BATCH)) > 100
               for c in (3, 5, 6, 7, 8))
    return lab, wts


def zero_variance():
    """v * v == 0 in float (0, and a subnormal): no tables; a weight of exp(-d / 0) is 0 off the mean and NaN on it, so these
    classes are NaN from the second round on whatever their weights; an ordinary class next to them."""
    lab = np.full((4, 9), NO_LABEL, np.uint16)
    lab[1, 2] = 1
    lab[0, 1] = lab[3, 8] = 2
    lab[2, 5] = 3
    lab[0, 7] = lab[0, 8] = 4
    lab[3, 0:3] = 5
    wts = np.array([[7, 3, 9, 1, 1, 1, 1, 65535, 1]] * 4, np.uint16)
    wts[3, 1] = 0
    var = np.array([0.0, 0.0, 1e-40, 1e-40, 2.0], np.float32)
    assert var[2] > 0 and np.float32(var[2] * var[2]) == 0
    return lab, wts, 5, var, (1, 2, 3)


class Case:
    def __init__(self, name, labels, weights, L, variances, rounds):
        self.name, self.labels, self.weights, self.L, self.rounds = name, labels, weights, L, tuple(rounds)
        self.variances = np.asarray(variances, np.float32)
        for a in (self.labels, self.weights, self.variances):
            if a is not None:
                a.setflags(write=False)


def _builders(cap):
    b = {}
    b["blobs_33x65"] = lambda: (blob_labels(5, 33, 65, 2), random_weights(50, (33, 65)), 2, [5.0, 7.0], (1, 2, 6, 7))
    b["blobs_120x212"] = lambda: (blob_labels(3, 120, 212, 6, (5,)), random_weights(51, (120, 212)), 6,
                                  np.linspace(6.0, 14.0, 6), (1, 2, 6, 7))
    b["blobs_240x424"] = lambda: (blob_labels(4, 240, 424, 7), random_weights(52, (240, 424)), 7,
                                  [50., 8., 8., 8., 8., 8., 8.], (1, 2, 6, 7))
    b["narrow_45x7"] = lambda: (blob_labels(8, 45, 7, 2), random_weights(53, (45, 7)), 2, [4.0, 6.0], (1, 2, 6, 7))
    for wrap in WRAP_CASES:
        b["wrap_%dx%d" % wrap[:2]] = lambda wrap=wrap: wrap_case(*wrap) + (2, [2.0, 3.0], (1, 2, 6, 7))
    for n_class, n_zero in ((cap - 1, 0), (cap, 0), (cap + 1, 0), (cap + 1, 2), (cap + 2, 2)):
        b[f"cap_{n_class - cap:+d}_zeros_{n_zero}"] = lambda n=n_class, z=n_zero: cap_image(cap, n, z) + (3, [30.0, 5.0, 4.0], (1, 4))
    b["both_over_cap"] = lambda: both_over_cap_image(cap) + (3, [40.0, 45.0, 4.0], (1, 4))
    b["tables_3069"] = lambda: table_boundary(3069) + (5, [6.0, 8.0, 2.5, 1.0, 3.0], (1, 2, 4))
    b["no_tables_3070"] = lambda: table_boundary(3070) + (5, [6.0, 8.0, 2.5, 1.0, 3.0], (1, 2, 4))
    for h, w in BATCH_SHAPES:      # one batch and a 9-pixel tail; two batches and a tail
        b[f"scattered_{h}x{w}"] = lambda h=h, w=w: (scattered(h, h, w), random_weights(w, (h, w)), 8, wide_variances(w, 8), (1, 3))
    b["batches_cross_cap"] = lambda: batches_image(cap) + (8, wide_variances(BATCH_SHAPES[1][1], 8), (1, 3))
    b["zero_variance"] = zero_variance
    return b


CAP_FOR_CPU = 20480          # the cap the library reports (the GPU tests assert it): lets the CPU tests build the same cases


@functools.lru_cache(maxsize=None)
def case(name, cap=CAP_FOR_CPU):
    lab, wts, L, var, rounds = _builders(cap)[name]()
    return Case(name, np.ascontiguousarray(lab), np.ascontiguousarray(wts), L, var, rounds)


def case_names(cap=CAP_FOR_CPU):
    return tuple(_builders(cap))


@functools.lru_cache(maxsize=None)
def trace(name, cap=CAP_FOR_CPU):
    """The restatement's means after every round of max(case.rounds): computed once, shared, read-only."""
    c = case(name, cap)
    out = []
    sn.weighted_modes(c.labels, c.weights, c.L, c.variances, max(c.rounds), trace=out)
    for t in out:
        t.setflags(write=False)
    return tuple(out)


def uses_tables(c):
    h, w = c.labels.shape
    v2 = (c.variances * c.variances).astype(np.float32)
    return [bool(h + w <= TAB_CAP and v > 0) for v in v2]


# ------------------------------------------------------------ heights -----------------------------------------------------------
def session_stack(rdf, dims, cfg4):
    """The two-layer stack of the session tests over session_cases.forest_config's forests, labels_reduce 2."""
    f0, f1, conditions, colors = cfg4
    cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                      {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
           "conditions": conditions, "label_colors": colors}
    return rdf.LayeredDecisionForest(cfg, dims, 2)


def height_inputs(h, w, r, seed):
    """A depth frame [h * r, w * r] with a 0 and a 65535, a plane and intrinsics."""
    rng = np.random.default_rng(seed)
    depth = rng.integers(1, 65535, size=(h * r, w * r)).astype(np.uint16)
    depth[0, 0], depth[r, r] = 0, 65535
    plane = (np.eye(4) + 0.1 * rng.standard_normal((4, 4))).astype(np.float32)
    return depth, plane, (0.9 * w * r, 0.91 * w * r, 0.5 * w * r + 0.3, 0.5 * h * r - 0.4)
