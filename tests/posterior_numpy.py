"""Plain numpy / fp32 restatement of the forest posterior, rules Q1 to Q7 of include/rdf_labels.h: `posterior` (per evaluated
pixel the class sums, the label, the confidence and the gate) and `confidence_counts` (the reliability histogram).  Written
from the rules for reading, one pixel at a time; the kernels of forest_posterior_hip.hip must match it bit for bit.  The walk
of rule Q2 is rule R2's, so it is refit_numpy.walk; tests/test_posterior.py pins this file to a case worked by hand and its
labels to the oracle's evaluator."""
import numpy as np

import refit_numpy as rn

NO_PIXEL = 65535
f32 = np.float32


def sums_of_pixel(frame, forest, x, y, scale):
    """Rule Q2: acc float32 [C] of depth pixel (x, y), the trees in index order, one rounded fp32 add per class and leaf."""
    T, D, C = rn.dims(forest)
    acc = np.zeros(C, f32)                                   # +0.0f
    for t in range(T):
        at = rn.walk(frame, forest[t], D, x, y, scale)
        if at is None:                                       # told to go on at level D - 1: nothing is added
            continue
        n, s = at
        with np.errstate(all="ignore"):
            for c in range(C):
                acc[c] = f32(acc[c] + forest[t, n, 7 + s * C + c])
    return acc


def label_of(acc):
    """Rule Q3: (label, best)."""
    best, label = f32(0.), 0
    for c in range(acc.shape[0]):
        if acc[c] > best:                                    # False for NaN
            best, label = acc[c], c
    return label, best


def confidence_of(acc, best):
    """Rule Q4."""
    with np.errstate(all="ignore"):
        S = f32(0.)
        for c in range(acc.shape[0]):
            S = f32(S + acc[c])
        if not (S > f32(0.)):
            return 0
        v = rn.floor_i32(f32(f32(best / S) * f32(65535.)))
    return min(max(v, 0), 65535)


def evaluated_mask(depth, labels_reduce=1, filter_images=None, filter_class=None):
    """Rule Q1: bool [n, Hl, Wl], the label pixels that are evaluated."""
    r = int(labels_reduce)
    n_img, h, w = depth.shape
    d = depth[:, :(h // r) * r:r, :(w // r) * r:r]
    keep = (d != 0) & (d != NO_PIXEL)
    if filter_images is not None:
        keep &= filter_images.astype(np.int64) == int(filter_class)
    return keep


def posterior(depth, forest, labels_reduce=1, scale=1., filter_images=None, filter_class=None, min_conf=0,
              labels=None, conf=None, sums=None, prefill=NO_PIXEL):
    """Rules Q1 to Q5 on depth uint16 [n, H, W].  labels, conf uint16 [n, Hl, Wl] and sums float32 [n, C, Hl, Wl] are written
    in place where given and made (filled with `prefill`) where not; returns (labels, conf, sums)."""
    T, D, C = rn.dims(forest)
    n_img, h, w = depth.shape
    r = int(labels_reduce)
    hl, wl = h // r, w // r
    labels = np.full((n_img, hl, wl), prefill, np.uint16) if labels is None else labels
    conf = np.full((n_img, hl, wl), prefill, np.uint16) if conf is None else conf
    sums = np.full((n_img, C, hl, wl), prefill, f32) if sums is None else sums
    assert labels.shape == conf.shape == (n_img, hl, wl) and sums.shape == (n_img, C, hl, wl)
    for i in range(n_img):
        for y in range(hl):
            for x in range(wl):
                if filter_images is not None and int(filter_images[i, y, x]) != int(filter_class):
                    continue
                d = int(depth[i, y * r, x * r])
                if d == 0 or d == NO_PIXEL:
                    continue
                acc = sums_of_pixel(depth[i], forest, x * r, y * r, scale)
                label, best = label_of(acc)
                k = confidence_of(acc, best)
                conf[i, y, x] = k
                sums[i, :, y, x] = acc
                if k >= min_conf:
                    labels[i, y, x] = label
    return labels, conf, sums


def gate(labels, conf, min_conf, evaluated, prefill=NO_PIXEL):
    """Rule Q5's label map for another threshold, from an ungated one: evaluated pixels below min_conf keep the pre-fill."""
    out = labels.copy()
    out[evaluated & (conf < min_conf)] = prefill
    return out


def confidence_counts(pred, conf, truth, labels_reduce=1, bins=64, counts=None):
    """Rule Q7.  Adds onto counts uint64 [2 * bins + 2] (made zero when not given) and returns it."""
    r = int(labels_reduce)
    n_img, hl, wl = pred.shape
    assert conf.shape == pred.shape and truth.shape[0] == n_img and (truth.shape[1] // r, truth.shape[2] // r) == (hl, wl)
    counts = np.zeros(2 * bins + 2, np.uint64) if counts is None else counts
    one = np.uint64(1)
    for i in range(n_img):
        for y in range(hl):
            for x in range(wl):
                p, k, t = int(pred[i, y, x]), int(conf[i, y, x]), int(truth[i, y * r, x * r])
                if t == 0:
                    continue
                counts[2 * bins + 1] += one
                if p == NO_PIXEL:
                    counts[2 * bins] += one
                else:
                    counts[2 * ((k * bins) >> 16) + (1 if p == t else 0)] += one
    return counts
