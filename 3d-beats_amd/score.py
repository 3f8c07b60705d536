"""How good a model is, without copying label maps to the host: `LabelScorer` accumulates the confusion matrix of predicted
against true label maps on the device (rdf_score_labels of librdf_labels.so, one pass over the two maps) and reads a few
hundred bytes back; `Score` is the host arithmetic on that matrix.

The reference scores with `np.sum(got == truth) / np.sum(truth > 0)` on host copies of both maps (src/train_model.py:104-107,
131-135, src/test_on_saved_model.py).  `Score.pct_matching` is that number bit for bit, quirk included: a pixel with truth 0
and prediction 0 is a match in the numerator and absent from the denominator.  `Score.accuracy` is what it approximates, and
the matrix also says which class is taken for which, per class and -- with per_image -- per test frame.  The prediction may be
smaller than the truth by labels_reduce, as the layered models' label maps are: the truth is then sampled at (x * r, y * r).
The semantics are in include/rdf_labels.h; tests/score_numpy.py restates them.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

MAX_CLASSES = 64


def _ratio(num, den):
    with np.errstate(all="ignore"):
        return np.asarray(num, np.float64) / np.asarray(den, np.float64)


class Score:
    """Plain host object.  confusion uint64 [C + 1, C + 1], truth by prediction; row and column C are "none or unknown" (the
    65535 pre-fill, an id the model does not have)."""

    def __init__(self, confusion, equal, labelled, per_image=None):
        self.confusion = np.ascontiguousarray(confusion, np.uint64)
        assert self.confusion.ndim == 2 and self.confusion.shape[0] == self.confusion.shape[1] >= 2
        self.num_classes = self.confusion.shape[0] - 1
        self.equal, self.labelled = int(equal), int(labelled)
        self.per_image = None if per_image is None else np.ascontiguousarray(per_image, np.uint32).reshape(-1, 2)

    @staticmethod
    def from_counts(counts, num_classes, per_image=None):
        """counts: the uint64 block rdf_score_labels fills, (C + 1)^2 cells then equal and labelled."""
        C = int(num_classes)
        counts = np.asarray(counts, np.uint64).reshape(-1)
        cells = (C + 1) * (C + 1)
        assert 1 <= C <= MAX_CLASSES and counts.size == cells + 2, (C, counts.size)
        return Score(counts[:cells].reshape(C + 1, C + 1).copy(), counts[cells], counts[cells + 1], per_image)

    @property
    def num_pixels(self):
        return int(self.confusion.sum())

    @property
    def pct_matching(self):
        """The reference's `pct. matching pixels`: nan for 0 / 0 and inf for k / 0, as numpy gives."""
        with np.errstate(all="ignore"):
            return float(np.float64(self.equal) / np.float64(self.labelled))

    @property
    def accuracy(self):
        """Of the pixels whose truth is one of the classes 1..C-1, the part predicted as that class."""
        C = self.num_classes
        rows = self.confusion[1:C]
        return float(_ratio(np.trace(self.confusion[1:C, 1:C]), rows.sum()))

    def _diag_row_col(self):
        m = self.confusion.astype(np.float64)
        return np.diag(m), m.sum(axis=1), m.sum(axis=0)

    @property
    def recall(self):
        d, row, _ = self._diag_row_col()
        return _ratio(d, row)

    @property
    def precision(self):
        d, _, col = self._diag_row_col()
        return _ratio(d, col)

    @property
    def iou(self):
        d, row, col = self._diag_row_col()
        return _ratio(d, row + col - d)

    def worst_images(self, k=None):
        """Image indices by rising equal / labelled (needs per_image); images without a labelled pixel come last."""
        assert self.per_image is not None, "scored without per_image"
        pct = _ratio(self.per_image[:, 0], self.per_image[:, 1])
        pct = np.where(self.per_image[:, 1] == 0, np.inf, pct)
        order = np.argsort(pct, kind="stable")
        return order if k is None else order[:int(k)]

    def __repr__(self):
        return (f"Score(classes={self.num_classes}, pixels={self.num_pixels}, pct_matching={self.pct_matching:.4f}, "
                f"accuracy={self.accuracy:.4f})")


def _arr(buf):
    return buf.cu() if hasattr(buf, "cu") and callable(buf.cu) else buf


def _maps(a, what):
    """A device uint16 [N, H, W] (or [H, W]) as (object, (N, H, W))."""
    a = _arr(a)
    shape = tuple(int(s) for s in a.shape)
    if len(shape) == 2:
        shape = (1,) + shape
    assert len(shape) == 3, f"{what}: [N, H, W] or [H, W], not {shape}"
    itemsize = a.element_size() if hasattr(a, "element_size") else np.dtype(a.dtype).itemsize
    assert itemsize == 2, f"{what}: 16-bit labels, not {a.dtype}"
    assert not hasattr(a, "is_contiguous") or a.is_contiguous(), f"{what}: not contiguous"
    return a, shape


class LabelScorer:
    def __init__(self, num_classes):
        """num_classes = C of the model (dataset.num_classes(): ids 0..C-1), 1..64."""
        self.num_classes = int(num_classes)
        assert 1 <= self.num_classes <= MAX_CLASSES, num_classes
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        nbytes = int(self._lb.rdf_score_counts_bytes(self.num_classes))
        assert nbytes == 8 * ((self.num_classes + 1) ** 2 + 2)
        self.counts_cu = DeviceArray((nbytes // 8,), np.uint64)
        self.per_image_cu = None
        self.reset()

    def reset(self):
        """Zero the counts (stream-ordered) and forget the per-image sums."""
        self.counts_cu.fill(np.uint64(0))
        self.per_image_cu = None
        return self

    def add(self, pred, truth, labels_reduce=1, per_image=False):
        """Enqueue the score of pred uint16 [N, H // r, W // r] against truth uint16 [N, H, W] on the current stream, adding
        onto what is there; nothing is read back.  DeviceArrays, torch tensors and .cu() buffers are taken.  per_image:
        also keep {equal, labelled} of each image (every add between two resets then has the same N)."""
        r = int(labels_reduce)
        assert r >= 1
        pred, (n, hl, wl) = _maps(pred, "pred")
        truth, (nt, h, w) = _maps(truth, "truth")
        assert nt == n and (hl, wl) == (h // r, w // r), f"pred {(n, hl, wl)} against truth {(nt, h, w)} at labels_reduce {r}"
        if per_image:
            if self.per_image_cu is None:
                self.per_image_cu = DeviceArray((n, 2), np.uint32).fill(0)
            assert self.per_image_cu.shape[0] == n, "per_image: another number of images; reset() first"
        from .decision_tree import _image_chunks
        p0, t0, st = device_ptr(pred), device_ptr(truth), self._rt.stream()
        for i0, cnt in _image_chunks(n, h * w):
            rc = self._lb.rdf_score_labels(cnt, w, h, r, self.num_classes, p0 + i0 * hl * wl * 2, t0 + i0 * h * w * 2,
                                           self.counts_cu.ptr, self.per_image_cu.ptr + i0 * 8 if per_image else None, st)
            _lib.check(self._lb, rc, "rdf_score_labels")
        self.counts_cu.mark_dirty()
        return self

    def result(self):
        """Read the counts back (synchronises) as a Score."""
        per_image = self.per_image_cu.get() if self.per_image_cu is not None else None
        return Score.from_counts(self.counts_cu.get(), self.num_classes, per_image)


class Calibration:
    """Plain host object: what a forest's confidence (rule Q4 of include/rdf_labels.h) is worth.  Bin b of `bins` holds the
    classified labelled pixels whose 16-bit confidence k has (k * bins) >> 16 == b.  count_by_bin, correct_by_bin (lists),
    labelled and unclassified are exact Python integers; every ratio below is one float64 division."""

    def __init__(self, count_by_bin, correct_by_bin, labelled, unclassified):
        self.count_by_bin = [int(v) for v in count_by_bin]
        self.correct_by_bin = [int(v) for v in correct_by_bin]
        self.bins = len(self.count_by_bin)
        assert self.bins >= 1 and len(self.correct_by_bin) == self.bins
        self.labelled, self.unclassified = int(labelled), int(unclassified)

    @staticmethod
    def from_counts(counts, bins):
        """counts: the uint64 block rdf_labels_confidence_counts fills: per bin {wrong, correct}, then unclassified, labelled."""
        bins = int(bins)
        counts = [int(v) for v in np.asarray(counts, np.uint64).reshape(-1)]
        assert len(counts) == 2 * bins + 2, (bins, len(counts))
        wrong, correct = counts[0:2 * bins:2], counts[1:2 * bins:2]
        return Calibration([w + c for w, c in zip(wrong, correct)], correct, counts[2 * bins + 1], counts[2 * bins])

    @property
    def classified(self):
        return sum(self.count_by_bin)

    @property
    def accuracy_by_bin(self):
        """float64 [bins]: correct / count, NaN for an empty bin."""
        return np.array([c / n if n else np.nan for c, n in zip(self.correct_by_bin, self.count_by_bin)], np.float64)

    @property
    def ece(self):
        """Expected calibration error: sum over the non-empty bins of n_b / N * |acc_b - (b + 1/2) / bins|, N the classified
        labelled pixels; NaN when there are none.  Over the common denominator 2 * bins * N the sum is one of integers,
        sum |2 * bins * c_b - n_b * (2 b + 1)|, so it is exact up to the one division."""
        N = self.classified
        if N == 0:
            return float("nan")
        num = sum(abs(2 * self.bins * c - n * (2 * b + 1)) for b, (c, n) in enumerate(zip(self.correct_by_bin, self.count_by_bin)))
        return num / (2 * self.bins * N)

    def coverage_curve(self):
        """(min_conf int64 [bins], coverage float64 [bins], accuracy float64 [bins]): min_conf[b] = ceil(b * 65536 / bins) is
        the smallest confidence of bin b; gating at it keeps the pixels of the bins >= b, `coverage` is their share of
        `labelled` and `accuracy` the share of them that is correct (NaN where nothing is kept or labelled)."""
        B = self.bins
        min_conf = np.array([-((-b * 65536) // B) for b in range(B)], np.int64)
        kept, right = [0] * B, [0] * B
        n = c = 0
        for b in range(B - 1, -1, -1):
            n, c = n + self.count_by_bin[b], c + self.correct_by_bin[b]
            kept[b], right[b] = n, c
        coverage = np.array([k / self.labelled if self.labelled else np.nan for k in kept], np.float64)
        accuracy = np.array([r / k if k else np.nan for r, k in zip(right, kept)], np.float64)
        return min_conf, coverage, accuracy

    def min_conf_for(self, accuracy):
        """The smallest threshold of coverage_curve() whose kept pixels reach `accuracy`, or None when none does."""
        min_conf, _, acc = self.coverage_curve()
        for m, a in zip(min_conf, acc):
            if a >= accuracy:           # (False for NaN)
                return int(m)
        return None

    def __repr__(self):
        return (f"Calibration(bins={self.bins}, labelled={self.labelled}, unclassified={self.unclassified}, ece={self.ece:.4f})")


class ConfidenceScorer:
    def __init__(self, bins=64):
        """bins: 1..1024 equal ranges of the 16-bit confidence."""
        self.bins = int(bins)
        assert 1 <= self.bins <= 1024, bins
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.counts_cu = DeviceArray((2 * self.bins + 2,), np.uint64)
        self.reset()

    def reset(self):
        """Zero the counts (stream-ordered)."""
        self.counts_cu.fill(np.uint64(0))
        return self

    def add(self, pred, conf, truth, labels_reduce=1):
        """Enqueue the counts of pred and conf uint16 [N, H // r, W // r] (what get_posteriors_forest wrote) against truth
        uint16 [N, H, W] on the current stream, adding onto what is there; nothing is read back."""
        r = int(labels_reduce)
        assert r >= 1
        pred, (n, hl, wl) = _maps(pred, "pred")
        conf, cshape = _maps(conf, "conf")
        truth, (nt, h, w) = _maps(truth, "truth")
        assert cshape == (n, hl, wl), f"conf {cshape} against pred {(n, hl, wl)}"
        assert nt == n and (hl, wl) == (h // r, w // r), f"pred {(n, hl, wl)} against truth {(nt, h, w)} at labels_reduce {r}"
        from .decision_tree import _image_chunks
        p0, c0, t0, st = device_ptr(pred), device_ptr(conf), device_ptr(truth), self._rt.stream()
        for i0, cnt in _image_chunks(n, h * w):
            rc = self._lb.rdf_labels_confidence_counts(cnt, w, h, r, self.bins, p0 + i0 * hl * wl * 2, c0 + i0 * hl * wl * 2,
                                                       t0 + i0 * h * w * 2, self.counts_cu.ptr, st)
            _lib.check(self._lb, rc, "rdf_labels_confidence_counts")
        self.counts_cu.mark_dirty()
        return self

    def result(self):
        """Read the counts back (synchronises) as a Calibration."""
        return Calibration.from_counts(self.counts_cu.get(), self.bins)
