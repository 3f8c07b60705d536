"""Joint votes: fingertip (or any joint's) positions regressed from a trained forest's leaves on the device
(rdf_labels_votes_count, rdf_labels_votes_fit and rdf_labels_votes_cast of librdf_labels.so).

Classification finds a fingertip where pixels of its class are seen: a tip under another finger, in the stereo shadow or
mislabelled has no position.  Here every leaf slot of the same trees also stores, per joint, a depth-normalised offset
towards the joint (Keskin et al., Shotton et al.'s offset-joint regression: the structure of a classification forest is
reused and only what the leaves hold is estimated again).  `VoteFitter.add` walks the hand pixels of frames whose joints
are known and sums their offsets per (tree, node, side, joint) in 64-bit integers; `fit` keeps, per leaf slot and joint, the
mean offset and a weight that falls with the offsets' spread -- a `VoteTable`; `JointVoter.vote` lets every hand pixel of a
frame, whatever its label, cast its leaves' votes into a coarse accumulator per joint and returns the accumulators' modes.
The reference has no counterpart: the rules (V1 to V6) are in include/rdf_labels.h and tests/votes_numpy.py restates them; all
arithmetic is in integers, so the device gives the same bytes whatever the order of the pixels.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime, to_device

MAX_JOINTS, MAX_RADIUS, MAX_CELL_SHIFT, MAX_BOX = 16, 255, 4, 4
# fit's default: the best of the sweep over powers of four in tests/perf/bench_joint_votes.py (profiles/joint_votes_bench.json)
DEFAULT_MAX_VAR = 1 << 20


def _forest_shape(forest):
    T, D, C = int(forest.num_trees), int(forest.max_depth), int(forest.num_classes)
    assert tuple(forest.forest_cu.shape) == (T, (1 << D) - 1, 7 + 2 * C), forest.forest_cu.shape
    return T, D, C


class VoteTable:
    """The votes of a forest's leaf slots: `.votes` device int32 [T, N, 2, J, 4] = (mx, my, mz, w), w == 0 for no vote;
    `.num_joints`; `.shape` = the forest's (T, D, C); `.report` (of the fit that made it, else None).  A table belongs to a
    forest's STRUCTURE: it is indexed by leaf slot, so it stays valid when the PDFs change (LeafRefitter.apply) and calls for
    a new fit when the structure does (ForestPruner.apply, ForestPruner.truncated, another training run).  Using it with a
    forest of another shape raises."""

    def __init__(self, votes, shape, report=None):
        self.shape = tuple(int(v) for v in shape)
        T, D, C = self.shape
        assert len(votes.shape) == 5 and tuple(votes.shape[:3]) == (T, (1 << D) - 1, 2) and votes.shape[4] == 4, votes.shape
        assert np.dtype(votes.dtype) == np.int32
        self.votes = votes
        self.num_joints = int(votes.shape[3])
        assert 1 <= self.num_joints <= MAX_JOINTS
        self.report = report

    def check_forest(self, forest):
        if _forest_shape(forest) != self.shape:
            raise ValueError(f"this vote table was fitted to a forest of (T, D, C) = {self.shape}, not {_forest_shape(forest)}: "
                             "fit it again")

    def save(self, path):
        """One .npy: int32 [4 + T N 2 J 4]: T, D, C, J, then the votes."""
        head = np.array(self.shape + (self.num_joints,), np.int32)
        with open(path, "wb") as fh:
            np.save(fh, np.concatenate([head, self.votes.get().reshape(-1)]))

    @classmethod
    def load(cls, path):
        flat = np.load(path)
        assert flat.dtype == np.int32 and flat.ndim == 1 and flat.size >= 4, "not a vote table"
        T, D, C, J = (int(v) for v in flat[:4])
        assert T >= 1 and 1 <= D <= 30 and C >= 1 and 1 <= J <= MAX_JOINTS and flat.size == 4 + T * ((1 << D) - 1) * 2 * J * 4, \
            "not a vote table"
        votes = flat[4:].reshape(T, (1 << D) - 1, 2, J, 4)
        assert ((votes[..., 3] >= 0) & (votes[..., 3] <= 256)).all(), "weights outside 0..256"
        return cls(to_device(votes), (T, D, C))


class VoteFitter:
    def __init__(self, forest, num_joints, radius=MAX_RADIUS):
        """forest: a DecisionForest, read only.  radius: a pixel sums its offset to a joint only when the joint is at most
        this many pixels away along x and along y (0..255)."""
        self.forest = forest
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.T, self.D, self.C = _forest_shape(forest)
        self.N = (1 << self.D) - 1
        self.J, self.radius = int(num_joints), int(radius)
        assert 1 <= self.J <= MAX_JOINTS, f"1 <= num_joints <= {MAX_JOINTS}"
        assert 0 <= self.radius <= MAX_RADIUS, f"0 <= radius <= {MAX_RADIUS}"
        self.sums = DeviceArray((self.T, self.N, 2, self.J, 5), np.uint64)
        self._totals = DeviceArray((4,), np.uint64)
        self._report = DeviceArray((4,), np.uint64)
        self.reset()

    def reset(self):
        """Zero the sums and totals (stream-ordered)."""
        self.sums.fill(np.uint64(0))
        self._totals.fill(np.uint64(0))
        return self

    def add(self, depth, labels, targets, scale_factor=1.):
        """Enqueue the count of depth uint16 [N, H, W] with labels uint16 [N, H, W] (device arrays; any label but 0 says
        "hand") and targets int32 [N, J, 3] = (tx, ty, tz) per frame and joint, host or device (tz outside 1..65534: the joint
        is absent from the frame), adding onto what is there; nothing is read back.  A batch of 2^31 pixels and more goes in
        several calls."""
        from .decision_tree import _image_chunks
        from .score import _maps
        depth, (n, h, w) = _maps(depth, "depth")
        labels, shape = _maps(labels, "labels")
        assert shape == (n, h, w), f"labels {shape} against depth {(n, h, w)}"
        if isinstance(targets, np.ndarray):
            assert targets.dtype == np.int32, targets.dtype
            targets = to_device(targets)
        assert tuple(int(s) for s in targets.shape) == (n, self.J, 3), f"targets {tuple(targets.shape)}, not {(n, self.J, 3)}"
        d0, l0, t0, st = device_ptr(depth), device_ptr(labels), device_ptr(targets), self._rt.stream()
        for i0, cnt in _image_chunks(n, h * w):
            rc = self._lb.rdf_labels_votes_count(d0 + i0 * h * w * 2, l0 + i0 * h * w * 2, t0 + i0 * self.J * 12, cnt, w, h,
                                                 device_ptr(self.forest.forest_cu), self.T, self.D, self.C, float(scale_factor),
                                                 self.J, self.radius, self.sums.ptr, self._totals.ptr, st)
            _lib.check(self._lb, rc, "rdf_labels_votes_count")
        self.sums.mark_dirty()
        self._totals.mark_dirty()
        return self

    def totals(self):
        """Read the totals back (synchronises): hand pixels walked, hand pixels without depth, walks that fell off the last
        level, and (pixel, tree, joint) offsets summed."""
        t = self._totals.get()
        return {"walked": int(t[0]), "no_depth": int(t[1]), "fell_off": int(t[2]), "offsets": int(t[3])}

    def fit(self, min_count=8, max_var=DEFAULT_MAX_VAR):
        """The vote table of the sums (rule V2; synchronises for the report).  A leaf slot votes for a joint when at least
        min_count pixels summed an offset there and the variance of their offsets -- in the normalised units, pixels times
        depth / 64, x and y together -- is at most max_var; the vote's weight falls from 256 at variance 0 to 1 at max_var.
        The default max_var is the best of the sweep over powers of four that tests/perf/bench_joint_votes.py records
        (profiles/joint_votes_bench.json; see DESIGN.md for what was and was not measured).  Returns a VoteTable whose
        `.report` holds: leaf_slots, votes, dropped_support, dropped_spread."""
        min_count, max_var = int(min_count), int(max_var)
        assert min_count >= 1, "min_count >= 1"
        assert 0 <= max_var <= 1 << 38, "0 <= max_var <= 2^38"
        votes = DeviceArray((self.T, self.N, 2, self.J, 4), np.int32)
        rc = self._lb.rdf_labels_votes_fit(device_ptr(self.forest.forest_cu), self.T, self.D, self.C, self.J, self.sums.ptr,
                                           min_count, max_var, votes.ptr, self._report.ptr, self._rt.stream())
        _lib.check(self._lb, rc, "rdf_labels_votes_fit")
        votes.mark_dirty()
        self._report.mark_dirty()
        r = self._report.get()
        report = {"leaf_slots": int(r[0]), "votes": int(r[1]), "dropped_support": int(r[2]), "dropped_spread": int(r[3])}
        return VoteTable(votes, (self.T, self.D, self.C), report)


class JointVoter:
    def __init__(self, forest, table, depth_dims, labels_reduce=1, cell_shift=2, box=1, min_support=1, max_frames=64):
        """forest: a DecisionForest; table: a VoteTable fitted to its structure; depth_dims = (DIM_Y, DIM_X).  The accumulator
        has cells of 2^cell_shift pixels (0..4); a joint is the cell whose (2 box + 1)^2 neighbourhood (box 0..4) holds the
        most weight, if that is at least min_support.  The workspace holds max_frames frames: longer batches go in chunks,
        with the same bytes per frame whatever max_frames is."""
        table.check_forest(forest)
        self.forest, self.table = forest, table
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.T, self.D, self.C = _forest_shape(forest)
        self.J = table.num_joints
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.labels_reduce, self.cell_shift, self.box = int(labels_reduce), int(cell_shift), int(box)
        self.min_support, self.max_frames = int(min_support), int(max_frames)
        assert self.labels_reduce >= 1 and 0 <= self.cell_shift <= MAX_CELL_SHIFT and 0 <= self.box <= MAX_BOX
        assert 0 <= self.min_support < 1 << 32 and self.max_frames >= 1
        nbytes = int(self._lb.rdf_labels_votes_workspace_bytes(self.max_frames, self.DIM_X, self.DIM_Y, self.J, self.cell_shift))
        assert nbytes > 0, "frame size or joints out of range"
        self._workspace = DeviceArray((nbytes,), np.uint8)

    def sibling(self):
        """A voter of the same forest, table and settings with a workspace of its own: what a second HandPipeline gets, so
        that the two hands of a frame can vote on two streams without sharing an accumulator."""
        return JointVoter(self.forest, self.table, (self.DIM_Y, self.DIM_X), self.labels_reduce, self.cell_shift, self.box,
                          self.min_support, self.max_frames)

    def vote(self, depth, gate=None, scale_factor=1., out=None):
        """depth: device uint16 [N, H, W] ([H, W] is one frame).  gate: None (every pixel with a depth votes: dataset frames,
        whose background is 65535) or a device uint16 [N, H // r, W // r] map whose values other than 0 and 65535 say "hand"
        -- a label map, a composite, a gated posterior's labels.  Returns a device int32 [N, J, 4] = (X, Y, Z, support) per
        frame and joint: X and Y in 1/16 pixel with a pixel's centre at +8, Z in depth units, (-1, -1, 0, 0) for a joint with
        too little support.  One clear and two launches per chunk on the current stream, nothing read back."""
        from .score import _maps
        depth, (n, h, w) = _maps(depth, "depth")
        assert (h, w) == (self.DIM_Y, self.DIM_X), f"frames of {(h, w)}, not {(self.DIM_Y, self.DIM_X)}"
        self.table.check_forest(self.forest)
        r = self.labels_reduce
        lpix = (h // r) * (w // r)
        g0 = None
        if gate is not None:
            gate, gshape = _maps(gate, "gate")
            assert gshape == (n, h // r, w // r), f"gate {gshape} against {(n, h // r, w // r)}"
            g0 = device_ptr(gate)
        out = DeviceArray((n, self.J, 4), np.int32) if out is None else out
        assert np.dtype(out.dtype) == np.int32 and int(np.prod(out.shape)) == n * self.J * 4, (out.shape, out.dtype)
        d0, o0, st = device_ptr(depth), device_ptr(out), self._rt.stream()
        for a in range(0, n, self.max_frames):
            b = min(n - a, self.max_frames)
            rc = self._lb.rdf_labels_votes_cast(d0 + a * h * w * 2, b, w, h, None if g0 is None else g0 + a * lpix * 2, r,
                                                device_ptr(self.forest.forest_cu), self.T, self.D, self.C, float(scale_factor),
                                                self.table.votes.ptr, self.J, self.cell_shift, self.box, self.min_support,
                                                self._workspace.ptr, o0 + a * self.J * 16, st)
            _lib.check(self._lb, rc, "rdf_labels_votes_cast")
        self._workspace.mark_dirty()
        if hasattr(out, "mark_dirty"):
            out.mark_dirty()
        return out

    @staticmethod
    def to_float(joints):
        """Host (x, y, z, support) of vote's output (synchronises): x and y float64 [N, J] in pixels -- a pixel's centre is
        at +0.5, the renderer's convention; subtract 0.5 to compare with integer pixel indices -- z float64 in depth units,
        all three NaN for a missing joint, and support int64."""
        j = joints.get() if hasattr(joints, "get") else np.asarray(joints)
        missing = j[..., 3] <= 0
        x, y, z = (np.where(missing, np.nan, j[..., k] / s) for k, s in ((0, 16.), (1, 16.), (2, 1.)))
        return x, y, z, j[..., 3].astype(np.int64)
