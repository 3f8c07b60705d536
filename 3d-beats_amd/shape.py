"""The hand's shape from a forest's pooled votes on the device (rdf_labels_shape_pool and rdf_labels_shape_decide of
librdf_labels.so).

Every other consumer of a trained forest is per pixel or per joint.  Here the forest is one trained on frames whose hand
pixels all carry the frame's SHAPE as their label (hand_scene.make_shape_dataset: open, fist, point, pinch ...; the shape
classification forest of Keskin et al.): every hand pixel of a frame casts its leaves' distributions as 16-bit shares of one
vote, `ShapeVoter.pool` adds the shares of a frame into one row of 64-bit integers, and `ShapeVoter.decide` names the class
with the greatest pooled share and keeps a decision that changes only after `hold` agreeing frames -- something a player can
switch octaves with.  The reference has no counterpart: the rules (G1 to G8) are in include/rdf_labels.h and
tests/shape_numpy.py restates them; everything added across pixels is an integer, so the device gives the same bytes whatever
the order of the pixels.  Everything is enqueued on the current stream and nothing is read back.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime
from .joint_votes import _forest_shape

MAX_CLASSES = 16
FRESH = (-1, -1, 0, 0)
SETTINGS = ("labels_reduce", "min_pixels", "min_conf", "hold", "release", "names")


class ShapeVoter:
    def __init__(self, forest, depth_dims, labels_reduce=1, min_pixels=64, min_conf=0, hold=3, release=0, max_frames=64,
                 names=None):
        """forest: a DecisionForest of at most 16 classes, read in the reference layout (`forest.forest_cu`: nothing is
        packed, and what LeafRefitter.apply or ForestPruner.apply wrote is what is read); depth_dims = (DIM_Y, DIM_X).  A frame
        with fewer than min_pixels voting pixels, or whose winning class holds less than min_conf / 65535 of the pooled vote,
        has no shape (raw -1, or not valid); the held shape changes after `hold` consecutive valid frames of another class
        and, with release > 0, lets go (-1) after `release` consecutive frames without a valid one.  max_frames: longer
        batches are pooled in chunks, with the same bytes per frame whatever max_frames is.  names: one name per class, for
        to_host."""
        self.forest = forest
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.T, self.D, self.C = _forest_shape(forest)
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.labels_reduce, self.min_pixels, self.min_conf = int(labels_reduce), int(min_pixels), int(min_conf)
        self.hold, self.release, self.max_frames = int(hold), int(release), int(max_frames)
        self.names = None if names is None else tuple(names)
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError(f"a shape forest has 1 .. {MAX_CLASSES} classes, not {self.C}")
        if self.labels_reduce < 1 or self.min_pixels < 0 or not 0 <= self.min_conf <= 65535:
            raise ValueError("labels_reduce >= 1, min_pixels >= 0, 0 <= min_conf <= 65535")
        if self.hold < 1 or self.release < 0 or self.max_frames < 1:
            raise ValueError("hold >= 1, release >= 0, max_frames >= 1")
        if self.names is not None and len(self.names) != self.C:
            raise ValueError(f"{len(self.names)} names for {self.C} classes")
        self.words = 2 * self.C + 2
        self._fresh = DeviceArray((4,), np.int32).set(np.array(FRESH, np.int32))
        self.state = DeviceArray((4,), np.int32)
        self._pool = DeviceArray((self.max_frames, self.words), np.uint64)
        self._out = DeviceArray((self.max_frames, 4), np.int32)
        self.reset()

    def settings(self):
        return dict(labels_reduce=self.labels_reduce, min_pixels=self.min_pixels, min_conf=self.min_conf, hold=self.hold,
                    release=self.release, max_frames=self.max_frames, names=self.names)

    def sibling(self):
        """A voter of the same forest and settings with a pool, a state and an output buffer of its own: what a second
        HandPipeline gets, so that the two hands of a frame hold their shapes apart on two streams."""
        return ShapeVoter(self.forest, (self.DIM_Y, self.DIM_X), **self.settings())

    def reset(self):
        """Put the held state back to fresh, (-1, -1, 0, 0) (a stream-ordered device copy)."""
        self.state.copy_from(self._fresh)
        return self

    def _buffer(self, name, n, shape, dtype):
        """A view of the first n rows of this object's own buffer, grown when a call needs more rows than any before."""
        buf = getattr(self, name)
        if buf.shape[0] < n:
            buf = DeviceArray((n,) + shape, dtype)
            setattr(self, name, buf)
        return buf[:n]

    def pool(self, depth, gate=None, gate_class=-1, scale_factor=1., out=None):
        """depth: device uint16 [N, H, W] ([H, W] is one frame).  gate: None (every pixel with a depth votes: dataset frames
        and a pipeline's prepared frames, whose background is 65535) or a device uint16 [N, H // r, W // r] map of which only
        the pixels equal to gate_class vote (rule G1's filter).  Returns a device uint64 [N, 2 C + 2]: C soft sums, C hard
        votes, the voting pixels and the dead ones (rule G4) -- `out`, or this object's own buffer (overwritten by the next
        call).  One stream-ordered fill and one launch per chunk of max_frames frames, nothing read back."""
        from .score import _maps
        depth, (n, h, w) = _maps(depth, "depth")
        assert (h, w) == (self.DIM_Y, self.DIM_X), f"frames of {(h, w)}, not {(self.DIM_Y, self.DIM_X)}"
        r = self.labels_reduce
        lpix = (h // r) * (w // r)
        g0, gate_class = None, int(gate_class)
        if gate is not None:
            gate, gshape = _maps(gate, "gate")
            assert gshape == (n, h // r, w // r), f"gate {gshape} against {(n, h // r, w // r)}"
            assert 0 <= gate_class <= 65535, "a gate needs its gate_class"
            g0 = device_ptr(gate)
        else:
            assert gate_class == -1, "gate_class without a gate"
        out = self._buffer("_pool", n, (self.words,), np.uint64) if out is None else out
        assert np.dtype(out.dtype) == np.uint64 and int(np.prod(out.shape)) == n * self.words, (out.shape, out.dtype)
        out.fill(np.uint64(0))
        d0, o0, st = device_ptr(depth), device_ptr(out), self._rt.stream()
        for a in range(0, n, self.max_frames):
            b = min(n - a, self.max_frames)
            rc = self._lb.rdf_labels_shape_pool(d0 + a * h * w * 2, b, w, h, device_ptr(self.forest.forest_cu), self.T, self.D,
                                                self.C, None if g0 is None else g0 + a * lpix * 2, gate_class, r,
                                                float(scale_factor), o0 + a * self.words * 8, st)
            _lib.check(self._lb, rc, "rdf_labels_shape_pool")
        if hasattr(out, "mark_dirty"):
            out.mark_dirty()
        return out

    def decide(self, pool, out=None):
        """pool: device uint64 [N, 2 C + 2], N frames in time order.  Returns a device int32 [N, 4] = (raw, conf, held, changed)
        per frame (rules G6 and G7) -- `out`, or this object's own buffer -- and advances this object's device state by the N
        frames.  One launch, nothing read back."""
        n = int(np.prod(pool.shape)) // self.words
        assert np.dtype(pool.dtype) == np.uint64 and int(np.prod(pool.shape)) == n * self.words, (pool.shape, pool.dtype)
        out = self._buffer("_out", n, (4,), np.int32) if out is None else out
        assert np.dtype(out.dtype) == np.int32 and int(np.prod(out.shape)) == n * 4, (out.shape, out.dtype)
        rc = self._lb.rdf_labels_shape_decide(device_ptr(pool), n, self.C, self.min_pixels, self.min_conf, self.hold,
                                              self.release, self.state.ptr, device_ptr(out), self._rt.stream())
        _lib.check(self._lb, rc, "rdf_labels_shape_decide")
        self.state.mark_dirty()
        if hasattr(out, "mark_dirty"):
            out.mark_dirty()
        return out

    def classify(self, depth, gate=None, gate_class=-1, scale_factor=1., out=None):
        """pool, then decide: device int32 [N, 4] = (raw, conf, held, changed) for N frames in time order."""
        return self.decide(self.pool(depth, gate, gate_class, scale_factor), out)

    def to_host(*args, as_array=False):
        """classify's rows on the host (synchronises), as `voter.to_host(rows)` or `ShapeVoter.to_host(rows)`: an int32 array
        [N, 4] with as_array, else one dict per frame: raw, conf (0..1), held, changed, and, called on a voter that was given
        `names`, raw_name and held_name (None for -1)."""
        voter, rows = args if len(args) == 2 else (None, args[0])
        names = None if voter is None else voter.names
        r = rows.get() if hasattr(rows, "get") else np.asarray(rows)
        r = np.ascontiguousarray(r, np.int32).reshape(-1, 4)
        if as_array:
            return r
        out = []
        for raw, conf, held, changed in r.tolist():
            d = dict(raw=raw, conf=conf / 65535., held=held, changed=bool(changed))
            if names is not None:
                d["raw_name"] = None if raw < 0 else names[raw]
                d["held_name"] = None if held < 0 else names[held]
            out.append(d)
        return out
