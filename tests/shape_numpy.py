"""Plain numpy / fp32 restatement of the hand's shape, rules G1 to G7 of include/rdf_labels.h: `pool` (every evaluated
pixel's 16-bit shares of its vote, added into one row of integers per frame) and `decide` (the pooled vote's class, its share,
and the held decision).  Written from the rules for reading, one pixel and one frame at a time; the kernels of
forest_shape_hip.hip must match it byte for byte.  The walk is rule R2's, refit_numpy.walk, as in the other restatements;
tests/test_shape.py pins this file to a case worked by hand."""
import numpy as np

import refit_numpy as rn

NO_PIXEL = 65535
f32 = np.float32
FRESH = (-1, -1, 0, 0)
MISS_MAX = 2 ** 31 - 1


def sums_of_pixel(frame, forest, x, y, scale, walk=rn.walk):
    """Rule G2 (Q2): acc float32 [C] of depth pixel (x, y), the trees in index order, one rounded fp32 add per class and leaf."""
    T, D, C = rn.dims(forest)
    acc = np.zeros(C, f32)
    for t in range(T):
        at = walk(frame, forest[t], D, x, y, scale)
        if at is None:                                       # told to go on at level D - 1: nothing is added
            continue
        n, s = at
        with np.errstate(all="ignore"):
            for c in range(C):
                acc[c] = f32(acc[c] + forest[t, n, 7 + s * C + c])
    return acc


def label_of(acc):
    """Rule Q3."""
    best, label = f32(0.), 0
    for c in range(acc.shape[0]):
        if acc[c] > best:                                    # False for NaN
            best, label = acc[c], c
    return label


def shares_of(acc):
    """Rule G3: the C shares of a pixel's vote, or None for a dead pixel."""
    with np.errstate(all="ignore"):
        S = f32(0.)
        for c in range(acc.shape[0]):
            S = f32(S + acc[c])
        if not (S > f32(0.)):
            return None
        q = []
        for c in range(acc.shape[0]):
            v = rn.floor_i32(f32(f32(acc[c] / S) * f32(65535.)))
            q.append(min(max(v, 0), 65535))
    return q


def add_pixel(row, acc):
    """Rule G4 for one evaluated pixel: row uint64 [2 C + 2] is added to in place."""
    C = acc.shape[0]
    one = np.uint64(1)
    q = shares_of(acc)
    if q is None:
        row[2 * C + 1] += one
        return
    for c in range(C):
        row[c] += np.uint64(q[c])
    row[C + label_of(acc)] += one
    row[2 * C] += one


def pool(depth, forest, labels_reduce=1, scale=1., filter_images=None, filter_class=None, pool=None, walk=rn.walk):
    """Rules G1 to G4 on depth uint16 [n, H, W].  Adds onto pool uint64 [n, 2 C + 2] (made zero when not given) and returns it."""
    T, D, C = rn.dims(forest)
    n_img, h, w = depth.shape
    r = int(labels_reduce)
    out = np.zeros((n_img, 2 * C + 2), np.uint64) if pool is None else pool
    assert out.shape == (n_img, 2 * C + 2) and out.dtype == np.uint64
    for i in range(n_img):
        for y in range(h // r):
            for x in range(w // r):
                if filter_images is not None and int(filter_images[i, y, x]) != int(filter_class):
                    continue
                d = int(depth[i, y * r, x * r])
                if d == 0 or d == NO_PIXEL:
                    continue
                add_pixel(out[i], sums_of_pixel(depth[i], forest, x * r, y * r, scale, walk))
    return out


def raw_of(row, C, min_pixels):
    """Rule G6: (raw, conf) of one pool row, in Python integers."""
    soft = [int(v) for v in row[:C]]
    total = sum(soft)
    if int(row[2 * C]) < min_pixels or total == 0:
        return -1, 0
    best = 0
    for c in range(C):
        if soft[c] > soft[best]:
            best = c
    return best, (soft[best] * 65535) // total


def hold_step(state, raw, conf, min_conf, hold, release):
    """Rule G7 for one frame: (the new state, changed)."""
    held, candidate, run, miss = state
    changed = 0
    if raw != -1 and conf >= min_conf:
        miss = 0
        if raw == held:
            candidate, run = -1, 0
        else:
            if raw == candidate:
                run += 1
            else:
                candidate, run = raw, 1
            if run >= hold:
                held, candidate, run, changed = raw, -1, 0, 1
    else:
        candidate, run = -1, 0
        miss = min(miss + 1, MISS_MAX)
        if release > 0 and miss >= release and held != -1:
            held, changed = -1, 1
    return (held, candidate, run, miss), changed


def decide(pool, C, min_pixels=64, min_conf=0, hold=3, release=0, state=FRESH):
    """Rules G6 and G7 over the frames of pool uint64 [n, 2 C + 2], in index order.  Returns (out int32 [n, 4] = (raw, conf, held,
    changed), the state after the last frame as int32 [4])."""
    assert pool.ndim == 2 and pool.shape[1] == 2 * C + 2
    state = tuple(int(v) for v in state)
    out = np.zeros((pool.shape[0], 4), np.int32)
    for f in range(pool.shape[0]):
        raw, conf = raw_of(pool[f], C, min_pixels)
        state, changed = hold_step(state, raw, conf, min_conf, hold, release)
        out[f] = (raw, conf, state[0], changed)
    return out, np.array(state, np.int32)
