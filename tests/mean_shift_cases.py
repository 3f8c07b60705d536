"""Inputs of the mean-shift tests: small pure functions that the CPU tests (preconditions, the restatement's own error) and
the GPU tests (the kernel against the restatement) both call, so that both see the same arrays.

Every builder names the branch of the kernel body (csrc/rdf_modes.hpp, the Unweighted policy) it is there for.  The three
limits below are the kernel's (Unweighted::kListCap, kTabCap, kModesMaxClasses); a test that passes with other values there
checks another branch than it says."""
import functools
import math
from typing import NamedTuple

import numpy as np

from oracle import mean_shift_numpy as ms_np

LIST_CAP = 32768        # pixels of one class a workgroup lists in LDS; one more and its rounds rescan the image
TAB_CAP = 3072          # dim_x + dim_y up to which a round's weights come from two tables (exp(-a) * exp(-b))
MAX_CLASSES = 64
BATCH = 16 * 13 * 512   # pixels the sixteen waves list per batch

NO_LABEL = 65535
OFFSETS = (0, 1, 3, 4, 7)   # label-pointer offsets in elements: 0 is the 16-byte (vector) lister, the others the scalar one

# (h, w) of the random images: tiny images and rows narrower than a lane's eight pixels (the lister that wraps more than
# once); a lane's eight straddling two rows; one batch plus a 9-pixel tail; two batches plus a tail; the largest dim_x;
# the largest dim_y, eight rows per lane
RANDOM_SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (9, 8), (33, 65), (5, 21301), (4, 53253), (1, 65535), (65535, 1))
assert 5 * 21301 == BATCH + 9 and 2 * BATCH < 4 * 53253 < 3 * BATCH


class Case(NamedTuple):
    name: str
    labels: np.ndarray      # uint16 [h, w]
    L: int
    variances: np.ndarray   # float32 [L]
    rounds: tuple           # the numbers of rounds the GPU test runs; the CPU test walks max(rounds)


def uses_tables(case):
    """Whether the kernel takes a round's weights from its two tables for class c (else: one exp per pixel)."""
    h, w = case.labels.shape
    v2 = (case.variances * case.variances).astype(np.float32)
    return [bool(h + w <= TAB_CAP and v > 0) for v in v2]


# ---------------------------------------------------------------------------------------------------------------------
# part 1: images whose first round has an exact answer
# ---------------------------------------------------------------------------------------------------------------------
def exact_centroids(labels, L):
    """Round 0 from integer sums: float64(sum x) / float64(n) per class, NaN for a class without pixels.  Every partial sum
    of the kernel is a sum of small integers, exact in fp64 in any order, and the division is IEEE: bit for bit."""
    want = np.full((L, 2), np.nan, np.float64)
    for c in range(1, L + 1):
        ys, xs = np.nonzero(labels == c)
        if xs.size:
            n = np.float64(xs.size)
            want[c - 1] = (np.float64(int(xs.sum(dtype=np.int64))) / n, np.float64(int(ys.sum(dtype=np.int64))) / n)
    return want


RANDOM_ABSENT = (5, 64)


@functools.lru_cache(maxsize=None)
def random_at_class_limit(h, w):
    """L = 64, labels drawn from {0 .. 66, 65535}: 0, 65, 66 and 65535 must be ignored; classes 5 and 64 are absent."""
    rng = np.random.default_rng(1000 * h + w)
    pool = np.array([v for v in range(67) if v not in RANDOM_ABSENT] + [NO_LABEL], np.uint16)
    lab = pool[rng.integers(0, pool.size, size=(h, w))]
    lab.setflags(write=False)
    return lab


def random_variances(h, w):
    """Wide enough for the scattered pixels of a random image to keep every weight sum far from 0 (the CPU test asserts it)."""
    return (max(3.0, max(h, w) / 32.0) + 0.125 * np.arange(MAX_CLASSES)).astype(np.float32)


ONE_PIXEL_SHAPE = (5, 21301)


@functools.lru_cache(maxsize=None)
def one_pixel_per_class():
    """(labels, pixel index of class c + 1): the first and last pixel of a lane's eight, of a step's 512, of a wave's round of
    8192, of the batch and of its tail, and both ends of every row."""
    h, w = ONE_PIXEL_SHAPE
    n_px = h * w
    picks = [0, 7, 8, 511, 512, 8191, 8192, BATCH - 1, BATCH, n_px - 1]
    for r in range(1, h):
        picks += [r * w - 1, r * w]
    picks += [w - 2, 1, 63, 64, 4095, 4096, 65535, 65536, BATCH - 8, BATCH - 9, BATCH + 1, BATCH + 2, n_px - 2]
    assert len(picks) == len(set(picks))
    rng = np.random.default_rng(64)
    while len(picks) < MAX_CLASSES:
        p = int(rng.integers(0, n_px))
        if p not in picks:
            picks.append(p)
    assert len(picks) == MAX_CLASSES == len(set(picks))
    lab = np.full(n_px, NO_LABEL, np.uint16)
    lab[picks] = np.arange(1, MAX_CLASSES + 1)
    lab = lab.reshape(h, w)
    lab.setflags(write=False)
    return lab, tuple(picks)


def _raster_class(lab, label, start, count, holes):
    """The first `count` pixels from raster index `start` on, skipping `holes`, become `label`; returns the index after."""
    flat = lab.reshape(-1)
    idx = np.setdiff1d(np.arange(start, start + count + len(holes)), np.asarray(holes, np.int64))[:count]
    assert idx.size == count
    flat[idx] = label
    return int(idx[-1]) + 1


CAP_SHAPE = (129, 257)
CAP_HOLES = (3, 100, 5000, 20001, 32760, 32765)     # six: every later lane's first slot is off a multiple of eight


@functools.lru_cache(maxsize=None)
def list_cap_image(n1):
    """Class 1 = the first n1 pixels in raster order but for a few holes, so that slot LIST_CAP falls inside a lane's
    eight pixels; class 2 a small blob after it; class 3 absent."""
    h, w = CAP_SHAPE
    lab = np.full((h, w), NO_LABEL, np.uint16)
    end = _raster_class(lab, 1, 0, n1, CAP_HOLES)
    assert end <= 127 * w + 200          # class 1 ends before class 2 starts
    lab[127, 200:230] = 2
    lab[128, 200:230] = 2
    lab[128, 0] = 0
    lab[128, 256] = 4       # beyond L = 3
    assert (lab == 1).sum() == n1 and (lab == 2).sum() == 60
    lab.setflags(write=False)
    return lab


BOTH_OVER_SHAPE = (200, 400)


@functools.lru_cache(maxsize=None)
def both_over_cap_image():
    """Classes 1 and 2 both over the list cap: both rescan the label image in every round; class 3 is a small listed blob."""
    h, w = BOTH_OVER_SHAPE
    lab = np.full((h, w), NO_LABEL, np.uint16)
    end = _raster_class(lab, 1, 0, 35001, (9, 4000, 33333))
    end = _raster_class(lab, 2, end + 997, 33003, (end + 1000, end + 2001, end + 30000, end + 30001))
    lab[190:195, 300:320] = 3
    assert (lab == 1).sum() == 35001 and (lab == 2).sum() == 33003 and end < 190 * w
    lab.setflags(write=False)
    return lab


TRIP_COUNTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
TRIP_SHAPE = (40, 130)


@functools.lru_cache(maxsize=None)
def exact_count_image(n):
    """Class 1 has exactly n pixels scattered over the image (n_list = n: one entry per thread is 1024, the later rounds'
    four entries per trip 4096), class 2 three pixels, and there are labels to ignore."""
    h, w = TRIP_SHAPE
    rng = np.random.default_rng(n)
    order = rng.permutation(h * w)
    lab = np.full(h * w, NO_LABEL, np.uint16)
    lab[order[:n]] = 1
    lab[order[n:n + 3]] = 2
    lab[order[n + 3:n + 40]] = 0
    lab[order[n + 40:n + 60]] = 3       # beyond L = 2
    lab = lab.reshape(h, w)
    lab.setflags(write=False)
    return lab


# ---------------------------------------------------------------------------------------------------------------------
# part 2: later rounds, against the restatement within 1e-9 px
# ---------------------------------------------------------------------------------------------------------------------
def _table_boundary(w):
    """The same blobs and variances at (3, 3069) -- dim_x + dim_y = 3072, tables -- and (3, 3070), one exp per pixel; class 3
    sits on the last columns the tables cover."""
    lab = np.full((3, w), NO_LABEL, np.uint16)
    lab[0:3, 100:141] = 1
    lab[1, 90] = 1
    lab[0:2, 1000:1011] = 2
    lab[1:3, 1030:1041] = 2
    lab[0:3, 3060:3069] = 3
    lab[2, 0] = 4
    lab[0, 0] = 0
    lab[0, 1] = 6           # beyond L = 5; class 5 absent
    return lab, 5, np.array([6.0, 8.0, 2.5, 1.0, 3.0], np.float32)


def _zero_variance():
    """v * v == 0 in float (0, and a subnormal): no tables, and a weight of exp(-0/0) = NaN for a pixel on the mean, of
    exp(-inf) = 0 off it: a one-pixel and a two-pixel class are both NaN from the second round on."""
    lab = np.full((4, 9), NO_LABEL, np.uint16)
    lab[1, 2] = 1
    lab[0, 1] = lab[3, 8] = 2
    lab[2, 5] = 3
    lab[0, 7] = lab[0, 8] = 4
    lab[3, 0:3] = 5                      # an ordinary class next to them
    var = np.array([0.0, 0.0, 1e-40, 1e-40, 2.0], np.float32)
    assert var[2] > 0 and np.float32(var[2] * var[2]) == 0
    return lab, 5, var


def _clean_underflow():
    """Two 3 x 4 blobs 550 columns apart and a fingertip-sized variance: from the centroid (286.5, 3) every weight is exactly
    0 (its exponent is below -4000), so the second round divides 0 by 0 and the mode stays NaN."""
    lab = np.full((8, 600), NO_LABEL, np.uint16)
    lab[2:5, 10:14] = 1
    lab[2:5, 560:564] = 1
    lab[6, 300:310] = 2
    return lab, 2, np.array([3.0, 3.0], np.float32)


def _partial_underflow():
    """A 3 x 20 blob plus one pixel 470 columns away: that pixel's weight is exactly 0 in both forms, the blob's are ordinary."""
    lab = np.full((8, 600), NO_LABEL, np.uint16)
    lab[2:5, 100:120] = 1
    lab[3, 590] = 1
    return lab, 1, np.array([4.0], np.float32)


def _one_class_everywhere(h, w):
    return np.ones((h, w), np.uint16), 1, np.array([100.0], np.float32)


def _restatement_builders():
    b = {}
    for n1 in (LIST_CAP - 1, LIST_CAP, LIST_CAP + 1):
        b[f"cap_{n1}"] = lambda n1=n1: (list_cap_image(n1), 3, np.array([30.0, 5.0, 4.0], np.float32), (4,))
    b["both_over_cap"] = lambda: (both_over_cap_image(), 3, np.array([40.0, 45.0, 4.0], np.float32), (4,))
    b["tables_3069"] = lambda: _table_boundary(3069) + ((1, 2, 4),)
    b["no_tables_3070"] = lambda: _table_boundary(3070) + ((1, 2, 4),)
    for h, w in RANDOM_SHAPES:
        b[f"random_{h}x{w}"] = lambda h=h, w=w: (random_at_class_limit(h, w), MAX_CLASSES, random_variances(h, w), (3,))
    b["row_65535"] = lambda: _one_class_everywhere(1, 65535) + ((3,),)
    b["column_65535"] = lambda: _one_class_everywhere(65535, 1) + ((3,),)
    b["zero_variance"] = lambda: _zero_variance() + ((1, 2, 3),)
    b["clean_underflow"] = lambda: _clean_underflow() + ((1, 2, 3),)
    b["partial_underflow"] = lambda: _partial_underflow() + ((1, 2, 4),)
    for n in TRIP_COUNTS:
        b[f"count_{n}"] = lambda n=n: (exact_count_image(n), 2, np.array([25.0, 30.0], np.float32), (3,))
    return b


_BUILDERS = _restatement_builders()
RESTATEMENT_CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def restatement_case(name):
    lab, L, var, rounds = _BUILDERS[name]()
    lab = np.ascontiguousarray(lab, np.uint16)
    lab.setflags(write=False)
    var.setflags(write=False)
    return Case(name, lab, L, var, tuple(rounds))


@functools.lru_cache(maxsize=None)
def restatement_trace(name):
    """The restatement's means after every round of max(case.rounds), computed once and shared: [rounds][L, 2], read-only."""
    case = restatement_case(name)
    trace = []
    ms_np.mean_shift(case.labels, case.L, case.variances, max(case.rounds), trace=trace)
    for t in trace:
        t.setflags(write=False)
    return tuple(trace)


def mean_shift_long(labels, L, variances, num_rounds):
    """The same rounds with np.longdouble coordinates and weights and math.fsum for every sum (exact sum of the rounded
    terms): the yardstick for the restatement's own rounding.  Where np.longdouble is no wider than fp64 the exact sums are
    what is left of it, and they remove the only error that grows with the number of pixels."""
    LD = np.longdouble
    var = np.asarray(variances, np.float32)
    pix = [np.nonzero(labels == c + 1) for c in range(L)]
    means = np.zeros((L, 2), LD)
    out = []
    for rnd in range(num_rounds):
        for c, (ys, xs) in enumerate(pix):
            if xs.size == 0:
                means[c] = np.nan           # 0 / 0
                continue
            if rnd == 0:
                s = (LD(int(xs.sum(dtype=np.int64))), LD(int(ys.sum(dtype=np.int64))), LD(xs.size))
            else:
                dx, dy = xs.astype(LD) - means[c, 0], ys.astype(LD) - means[c, 1]
                v2 = LD(np.float32(var[c] * var[c]))
                with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
                    p = np.exp(-((dx * dx) + (dy * dy)) / (2 * v2))
                    tx, ty = dx * p, dy * p
                if np.isnan(p).any():
                    s = (LD(np.nan),) * 3
                else:
                    s = (LD(math.fsum(tx)), LD(math.fsum(ty)), LD(math.fsum(p)))
            with np.errstate(invalid="ignore", divide="ignore"):
                means[c] = (means[c, 0] + s[0] / s[2], means[c, 1] + s[1] / s[2])
        out.append(means.copy())
    return out
