"""Pruning: a trained forest made smaller on the device by reduced-error (cost-complexity) pruning on held-out frames
(rdf_labels_prune_plan and rdf_labels_prune_apply of librdf_labels.so).

The trainer grows every tree until a side is pure or the depth is used up; most of the deep splits are asked for by a handful
of training pixels.  `ForestPruner.add` counts where the labelled pixels of frames the trainer has not seen land (a
LeafRefitter's counts), `plan` decides bottom-up which subtrees label those pixels no better than one leaf would -- with a
price per leaf, a minimum support and a depth limit on request -- and reports what would change, `apply` folds them, and
`truncated` gives the shallower forest that is left.  Each tree is pruned by its own errors, not by the forest's joint vote.
The reference has no counterpart: the rules (P1 to P4) are in include/rdf_labels.h and tests/prune_numpy.py restates them.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime
from .refit import LeafRefitter

REPORT = ("leaf_slots_before", "leaf_slots_after", "turned", "depth", "errors_before", "errors_after", "pixels", "nodes_after")


class ForestPruner:
    def __init__(self, forest):
        """forest: a DecisionForest; its forest_cu is read by add and plan and rewritten by apply."""
        self.forest = forest
        self.refitter = LeafRefitter(forest)
        self._rt = get_runtime()
        self._lb = self.refitter._lb
        self.T, self.D, self.C = self.refitter.T, self.refitter.D, self.refitter.C
        self.N = self.refitter.N
        self._report = DeviceArray((8,), np.uint64)
        self._workspace = None
        self._planned = None            # the versions of forest_cu and counts that the last plan read
        self.last_report = None

    @property
    def counts(self):
        return self.refitter.counts

    def reset(self):
        self.refitter.reset()
        return self

    def add(self, depth, labels, scale_factor=1.):
        """LeafRefitter.add: the labelled pixels of the frames are walked and counted, adding onto what is there."""
        self.refitter.add(depth, labels, scale_factor)
        return self

    def totals(self):
        return self.refitter.totals()

    def plan(self, cost_per_leaf=0, min_count=0, max_levels=None):
        """Rules P1 and P2 and the report P4, as a dict (synchronises): reachable leaf slots before and after, "go on" sides
        turned into leaf slots, the depth that is left, the counted pixels that each tree alone labels wrongly before and
        after (summed over the trees), the counted pixels, the reachable nodes that are left.  A subtree collapses when one
        leaf makes no more errors than it does plus cost_per_leaf for every leaf saved, when fewer than min_count pixels
        reach it, or when it starts at level max_levels or below.  Writes nothing but the workspace: forest and counts keep
        their bytes, and another plan may follow."""
        cost_per_leaf, min_count = int(cost_per_leaf), int(min_count)
        max_levels = self.D if max_levels is None else int(max_levels)
        assert 0 <= cost_per_leaf < 1 << 32, "0 <= cost_per_leaf < 2^32"
        assert 0 <= min_count < 1 << 64, "min_count >= 0"
        assert 1 <= max_levels <= self.D, f"1 <= max_levels <= {self.D}"
        if self._workspace is None:
            nbytes = int(self._lb.rdf_labels_prune_workspace_bytes(self.T, self.D, self.C))
            assert nbytes > 0
            self._workspace = DeviceArray((nbytes,), np.uint8)
        rc = self._lb.rdf_labels_prune_plan(device_ptr(self.forest.forest_cu), self.T, self.D, self.C, self.counts.ptr, cost_per_leaf,
                                            min_count, max_levels, self._workspace.ptr, self._report.ptr, self._rt.stream())
        _lib.check(self._lb, rc, "rdf_labels_prune_plan")
        self._workspace.mark_dirty()
        self._report.mark_dirty()
        self._planned = (self.forest.forest_cu.version, self.counts.version)
        self.last_report = dict(zip(REPORT, (int(v) for v in self._report.get())))
        return dict(self.last_report)

    def curve(self, costs):
        """One plan per cost_per_leaf of `costs`: the list of their reports.  Nothing is applied."""
        return [self.plan(cost_per_leaf=c) for c in costs]

    def decisions(self):
        """The last plan's byte per node (synchronises) as three bool arrays [T, N]: reachable before, collapse (made for the
        nodes reachable before), reachable after."""
        assert self._planned is not None, "plan first"
        state = self._workspace[:self.T * self.N].get().reshape(self.T, self.N)
        return (state & 1) != 0, (state & 2) != 0, (state & 4) != 0

    def apply(self):
        """Rule P3 by the last plan (stream-ordered): collapsed subtrees become leaf slots of their parents with the subtree's
        class frequencies and counts, the nodes below get records of zeros.  forest_cu and the counts are marked written, so
        the packed table is made again at the next evaluation; the folded counts can go straight into
        `self.refitter.apply(...)` without a second counting pass.  Returns the plan's report."""
        assert self._planned == (self.forest.forest_cu.version, self.counts.version), \
            "plan first: the forest or the counts were written since the last plan"
        rc = self._lb.rdf_labels_prune_apply(device_ptr(self.forest.forest_cu), self.T, self.D, self.C, self.counts.ptr,
                                             self._workspace.ptr, self._rt.stream())
        _lib.check(self._lb, rc, "rdf_labels_prune_apply")
        self.forest.forest_cu.mark_dirty()
        self.counts.mark_dirty()
        self._planned = None
        return dict(self.last_report)

    def truncated(self, depth=None):
        """A new DecisionForest of depth D' (the last plan's, after apply) holding the first 2^D' - 1 records of each tree: a
        device copy per tree, no kernel.  It labels every pixel as the pruned forest does."""
        from .decision_tree import DecisionForest
        depth = int(self.last_report["depth"] if depth is None else depth)
        assert 1 <= depth <= self.D
        out = DecisionForest(self.T, depth, self.C)
        n = (1 << depth) - 1
        for t in range(self.T):
            out.forest_cu[t].copy_from(self.forest.forest_cu[t][:n])
        return out
