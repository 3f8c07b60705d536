"""Leaf refit: a trained forest's leaf distributions re-estimated on the device from labelled depth frames, the tree
structure left as it is (rdf_labels_refit_count and rdf_labels_refit_apply of librdf_labels.so).

A forest trained on clean renders is run on what a camera reports; a forest's structure is found on the frames the trainer
can hold while more are at hand; the trainer's leaf rules (one-hot above 0.999 purity, the parent's PDF where nothing
separates) are not everyone's.  `LeafRefitter.add` walks every labelled pixel of a batch through every tree as inference
walks it and counts where it lands, per (tree, node, side, class), in 64-bit integers; counts of several batches simply add.
`apply` turns the counts into plain class frequencies, with a minimum support per leaf and a choice of what a leaf below it
gets.  The reference has no counterpart: the rules (R1 to R3) are in include/rdf_labels.h and tests/refit_numpy.py restates
them.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

FALLBACKS = {"keep": 0, "ancestor": 1}


def _floor_flags(flags):
    """floor of rule R2 on the two flag columns: float32 -> int64 with saturation, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        f = np.floor(flags.astype(np.float64))
    return np.clip(np.where(np.isnan(f), 0., f), -2147483648., 2147483647.).astype(np.int64)


class LeafRefitter:
    def __init__(self, forest):
        """forest: a DecisionForest; its forest_cu is read by add and rewritten by apply."""
        self.forest = forest
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.T, self.D, self.C = int(forest.num_trees), int(forest.max_depth), int(forest.num_classes)
        self.N = (1 << self.D) - 1
        assert tuple(forest.forest_cu.shape) == (self.T, self.N, 7 + 2 * self.C), forest.forest_cu.shape
        self.counts = DeviceArray((self.T, self.N, 2, self.C), np.uint64)
        self._totals = DeviceArray((4,), np.uint64)
        self._report = DeviceArray((4,), np.uint64)
        self._workspace = None
        self.reset()

    def reset(self):
        """Zero the counts and totals (stream-ordered)."""
        self.counts.fill(np.uint64(0))
        self._totals.fill(np.uint64(0))
        return self

    def add(self, depth, labels, scale_factor=1.):
        """Enqueue the count of depth uint16 [N, H, W] with its truth labels uint16 [N, H, W] (device arrays; [H, W] is one
        frame) on the current stream, adding onto what is there; nothing is read back.  A batch of 2^31 pixels and more goes
        in several calls."""
        from .decision_tree import _image_chunks
        from .score import _maps
        depth, (n, h, w) = _maps(depth, "depth")
        labels, shape = _maps(labels, "labels")
        assert shape == (n, h, w), f"labels {shape} against depth {(n, h, w)}"
        d0, l0, st = device_ptr(depth), device_ptr(labels), self._rt.stream()
        for i0, cnt in _image_chunks(n, h * w):
            rc = self._lb.rdf_labels_refit_count(d0 + i0 * h * w * 2, l0 + i0 * h * w * 2, cnt, w, h, device_ptr(self.forest.forest_cu),
                                                 self.T, self.D, self.C, float(scale_factor), self.counts.ptr, self._totals.ptr, st)
            _lib.check(self._lb, rc, "rdf_labels_refit_count")
        self.counts.mark_dirty()
        self._totals.mark_dirty()
        return self

    def totals(self):
        """Read the totals back (synchronises): pixels walked, pixels with a label the forest does not have, labelled pixels
        without depth, and walks that fell off the last level.  counts sums to T * walked - fell_off."""
        t = self._totals.get()
        return {"walked": int(t[0]), "unknown_label": int(t[1]), "no_depth": int(t[2]), "fell_off": int(t[3])}

    def apply(self, min_count=1, fallback="keep"):
        """Rewrite the PDFs of the forest's reachable leaf slots from the counts (rule R3).  A slot with fewer than min_count
        pixels keeps its PDF ('keep') or takes the class frequencies of the nearest ancestor whose subtree has that many
        ('ancestor').  forest_cu is marked written, so the packed table is made again at the next evaluation.  Returns the
        report (synchronises): slots written from their own counts, from an ancestor, kept, and their sum."""
        min_count = int(min_count)
        assert min_count >= 1, "min_count >= 1"
        assert fallback in FALLBACKS, f"fallback: one of {sorted(FALLBACKS)}, not {fallback!r}"
        if self._workspace is None:
            nbytes = int(self._lb.rdf_labels_refit_workspace_bytes(self.T, self.D, self.C))
            assert nbytes > 0
            self._workspace = DeviceArray((nbytes,), np.uint8)
        rc = self._lb.rdf_labels_refit_apply(device_ptr(self.forest.forest_cu), self.T, self.D, self.C, self.counts.ptr, min_count,
                                             FALLBACKS[fallback], self._workspace.ptr, self._report.ptr, self._rt.stream())
        _lib.check(self._lb, rc, "rdf_labels_refit_apply")
        self.forest.forest_cu.mark_dirty()
        self._report.mark_dirty()
        r = self._report.get()
        return {"own": int(r[0]), "ancestor": int(r[1]), "kept": int(r[2]), "leaf_slots": int(r[3])}

    def leaf_support(self):
        """Per level (host arithmetic on a read-back of the flags and the counts; synchronises): the reachable leaf slots, how
        many of them no pixel reached, and the pixels counted in them, as a list of dicts."""
        flags = _floor_flags(self.forest.forest_cu.get()[:, :, 5:7])
        per_slot = self.counts.get().sum(axis=3, dtype=np.uint64)
        reach = np.ones((self.T, 1), bool)
        out = []
        for j in range(self.D):
            lo, hi = (1 << j) - 1, (1 << (j + 1)) - 1
            leaf = reach[:, :, None] & (flags[:, lo:hi] != -1)
            s = per_slot[:, lo:hi]
            out.append({"level": j, "leaf_slots": int(leaf.sum()), "empty": int((leaf & (s == 0)).sum()),
                        "pixels": int(s[leaf].sum(dtype=np.uint64))})
            reach = (reach[:, :, None] & (flags[:, lo:hi] == -1)).reshape(self.T, -1)
        return out
