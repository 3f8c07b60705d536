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
