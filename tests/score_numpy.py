"""rdf_score_labels (include/rdf_labels.h) restated in plain numpy: the oracle of every GPU comparison in tests/test_score.py.

pred uint16 [N, H // r, W // r], truth uint16 [N, H, W] sampled at (x * r, y * r).  With C classes, index C of the matrix is
"none or unknown": min(v, C) takes the 65535 pre-fill and every id >= C there.  counts is the flat uint64 block of the C ABI:
(C + 1)^2 matrix cells, truth by prediction, then `equal` (raw values, so a (0, 0) pixel counts) and `labelled` (truth > 0)."""
import numpy as np


def sample_truth(truth, labels_reduce, label_shape):
    """The truth at the label map's own pixels: rows and columns 0, r, 2r, ... as far as the label map reaches."""
    r = int(labels_reduce)
    hl, wl = label_shape
    return np.asarray(truth)[:, :hl * r:r, :wl * r:r]


def score_counts(pred, truth, num_classes, labels_reduce=1, onto=None):
    """The counts block after one call that adds onto `onto` (zeros when None)."""
    C, r = int(num_classes), int(labels_reduce)
    pred, truth = np.asarray(pred, np.uint16), np.asarray(truth, np.uint16)
    n, h, w = truth.shape
    assert pred.shape == (n, h // r, w // r), (pred.shape, truth.shape, r)
    t = sample_truth(truth, r, pred.shape[1:])
    assert t.shape == pred.shape
    tc, pc = np.minimum(t, C).astype(np.int64), np.minimum(pred, C).astype(np.int64)
    cells = (C + 1) * (C + 1)
    counts = np.zeros(cells + 2, np.uint64) if onto is None else np.array(onto, np.uint64).reshape(-1).copy()
    assert counts.size == cells + 2
    counts[:cells] += np.bincount((tc * (C + 1) + pc).reshape(-1), minlength=cells).astype(np.uint64)
    counts[cells] += np.uint64(np.sum(pred == t))
    counts[cells + 1] += np.uint64(np.sum(t > 0))
    return counts


def score_per_image(pred, truth, labels_reduce=1, onto=None):
    """uint32 [N, 2] = {equal, labelled} of every image."""
    pred = np.asarray(pred, np.uint16)
    t = sample_truth(np.asarray(truth, np.uint16), labels_reduce, pred.shape[1:])
    out = np.zeros((pred.shape[0], 2), np.uint32) if onto is None else np.array(onto, np.uint32).copy()
    out[:, 0] += np.sum(pred == t, axis=(1, 2)).astype(np.uint32)
    out[:, 1] += np.sum(t > 0, axis=(1, 2)).astype(np.uint32)
    return out
