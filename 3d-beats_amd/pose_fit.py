"""The pose of the articulated hand of hand_model.py fitted to a depth frame and its forest labels, on the device
(librdf_labels.so: rdf_pose_fit): the reference's pose_fit.py with cuda/fit_mesh.cu, which perturbs one cylinder per GUI
frame, draws it through OpenGL and reads a float cost back.  Here a generation proposes `candidates` poses of the whole
hand around the incumbent, draws them with HandSceneRenderer's rasteriser, prices each against the frame with an integer
cost and keeps the best if it is strictly better -- five launches, nothing read back; `fit` enqueues any number of
generations in one C call.  The result is what mean shift cannot give: all five fingertips in 3-D, including fingers the
forest mislabels, and a pose to start the next frame from.  The rules (C, P, K, S) are in include/rdf_labels.h.

The default `sigma` and ranges are those of a prototype on rendered frames; THEY ARE UNMEASURED ON REAL DATA.
"""
import ctypes

import numpy as np

from . import _lib, hand_model
from .device import DeviceArray, device_ptr, get_runtime, to_device
from .hand_model import N_PARTS, POSE_SIZE, HandModel
from .hand_scene import Z_FAR, Z_NEAR

STATE_BYTES = 256
MAX_CANDIDATES = 4096
MAX_DIM = 32768
TERMS = ("missing", "extra", "label", "sq")
# per pose number: lengths in mm, angles in radians
DEFAULT_SIGMA = {"wrist": 8., "hand": 0.08, "spread": 0.05, "flexion": 0.12}
# (low, high): wide, and every angle within [-pi, pi] as rule P asks
DEFAULT_RANGES = {"x": (-1000., 1000.), "y": (-1000., 1000.), "height": (0., 1000.), "yaw": (-np.pi, np.pi),
                  "pitch": (-0.5 * np.pi, 0.5 * np.pi), "roll": (-0.5 * np.pi, 0.5 * np.pi), "spread": (-0.5, 0.5),
                  "flexion": (-0.3, 1.8)}


class _Config(ctypes.Structure):
    """RdfPoseFitConfig of include/rdf_labels.h."""
    _fields_ = [("candidates", ctypes.c_int32), ("mirrored", ctypes.c_int32), ("anneal_every", ctypes.c_int32),
                ("seed", ctypes.c_uint32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("ww", ctypes.c_int32),
                ("wh", ctypes.c_int32), ("w_boundary", ctypes.c_uint32), ("w_label", ctypes.c_uint32),
                ("target_mask", ctypes.c_uint64), ("f", ctypes.c_float), ("ppx", ctypes.c_float), ("ppy", ctypes.c_float),
                ("zmin", ctypes.c_float), ("zmax", ctypes.c_float), ("reserved", ctypes.c_float),
                ("sigma", ctypes.c_double * POSE_SIZE), ("lo", ctypes.c_double * POSE_SIZE), ("hi", ctypes.c_double * POSE_SIZE),
                ("cam_from_plane", ctypes.c_double * 12), ("geometry", ctypes.c_double * 30)]


assert ctypes.sizeof(_Config) == 1032


def geometry_of(model):
    """float64 [30], the `geometry` of RdfPoseFitConfig: per finger its base x, base y (depth units), rest splay (radians)
    and three phalanx lengths (depth units), the numbers HandModel's own chain uses."""
    u = model.units_per_mm
    return np.array([(hand_model.FINGER_BASE[f][0] * u, hand_model.FINGER_BASE[f][1] * u, hand_model.FINGER_REST_SPLAY[f]) +
                     tuple(hand_model.PHALANX_LENGTH[f][q] * u for q in range(3)) for f in range(5)], np.float64).reshape(30)


def pose_vector(values, units_per_mm):
    """float64 [26] from {"wrist", "hand", "spread", "flexion"} (DEFAULT_SIGMA's keys): mm become depth units."""
    v = np.empty(POSE_SIZE, np.float64)
    v[:3] = values["wrist"] * units_per_mm
    v[3:6] = values["hand"]
    for f in range(5):
        v[6 + 4 * f] = values["spread"]
        v[7 + 4 * f:10 + 4 * f] = values["flexion"]
    return v


def pose_ranges(ranges, units_per_mm):
    """(lo, hi) float64 [26] from DEFAULT_RANGES overridden entry by entry by `ranges`."""
    r = dict(DEFAULT_RANGES)
    unknown = set(ranges or {}) - set(r)
    if unknown:
        raise ValueError(f"unknown range names {sorted(unknown)}; the names are {sorted(r)}")
    r.update(ranges or {})
    lo, hi = np.empty(POSE_SIZE, np.float64), np.empty(POSE_SIZE, np.float64)
    for k, name in enumerate(("x", "y", "height")):
        lo[k], hi[k] = r[name][0] * units_per_mm, r[name][1] * units_per_mm
    for k, name in enumerate(("yaw", "pitch", "roll")):
        lo[3 + k], hi[3 + k] = r[name]
    for f in range(5):
        lo[6 + 4 * f], hi[6 + 4 * f] = r["spread"]
        lo[7 + 4 * f:10 + 4 * f], hi[7 + 4 * f:10 + 4 * f] = r["flexion"]
    return lo, hi


def reference_cost(terms):
    """The reference's float cost (fit_mesh.cu: 100 per boundary mismatch, 0.01 per squared depth unit) of integer terms
    (missing, extra, label, sq): with w_label = 0 and one target label the integer cost at w_boundary = 10000 is 100 times
    this.  The reference sums float32 atomics in arrival order; that sum is not reproduced."""
    t = [int(v) for v in np.asarray(terms).reshape(4)]
    return 100. * (t[0] + t[1]) + 0.01 * t[3]


def _parse_state(raw):
    raw = np.ascontiguousarray(raw, np.uint8).reshape(STATE_BYTES)
    counters = raw[248:256].view(np.uint32)
    return {"pose": raw[:208].view(np.float64).copy(), "cost": int(raw[208:216].view(np.uint64)[0]),
            "terms": raw[216:248].view(np.uint64).copy(), "generation": int(counters[0]), "accepted": int(counters[1])}


class PoseFitResult:
    """What one `fit` left, still on the device: `get()` reads it in one copy."""

    def __init__(self, fitter, buf, generations):
        self._fitter, self._buf, self.generations = fitter, buf, int(generations)
        self._host = None

    def get(self):
        """self, with pose float64 [26], cost (int), terms uint64 [4] = (missing, extra, label, sq), generation, accepted and
        history uint64 [generations] (the incumbent's cost after each generation) filled in."""
        if self._host is None:
            raw = self._buf.get()
            self._host = _parse_state(raw[:STATE_BYTES])
            self._host["history"] = raw[STATE_BYTES:].view(np.uint64).copy()
            self.__dict__.update(self._host)
        return self

    def fingertips(self, camera_space=True):
        """float64 [5, 3]: the end points of the fitted hand's fingertips, thumb to pinky, in camera space (plane space when
        not camera_space), depth units."""
        self.get()
        return self._fitter.model.fingertips(self.pose, self._fitter.cam_from_plane if camera_space else None)[0]

    @property
    def reference_cost(self):
        return reference_cost(self.get().terms)


class PoseTrackResult:
    """What `track` left: one row per frame on the device, read back once by `get()`."""

    def __init__(self, fitter, buf, n_frames, generations):
        self._fitter, self._buf, self.n_frames, self.generations = fitter, buf, int(n_frames), int(generations)
        self._host = None

    def get(self):
        """self, with poses float64 [N, 26], costs (list of int), terms uint64 [N, 4], accepted int [N] and history uint64
        [N, generations] filled in."""
        if self._host is None:
            raw = self._buf.get().reshape(self.n_frames, -1)
            rows = [_parse_state(r[:STATE_BYTES]) for r in raw]
            self._host = {"poses": np.array([r["pose"] for r in rows]).reshape(self.n_frames, POSE_SIZE),
                          "costs": [r["cost"] for r in rows],
                          "terms": np.array([r["terms"] for r in rows], np.uint64).reshape(self.n_frames, 4),
                          "accepted": np.array([r["accepted"] for r in rows], np.int64),
                          "history": np.ascontiguousarray(raw[:, STATE_BYTES:]).view(np.uint64).reshape(self.n_frames, self.generations)}
            self.__dict__.update(self._host)
        return self

    def fingertips(self, camera_space=True):
        """float64 [N, 5, 3]."""
        self.get()
        return self._fitter.model.fingertips(self.poses, self._fitter.cam_from_plane if camera_space else None)


class PoseFitter:
    def __init__(self, depth_dims, intrinsics, plane, model=None, mirrored=False, candidates=64, window=None, labels='fine',
                 target_labels=None, labels_reduce=1, w_boundary=10000, w_label=0, sigma=None, ranges=None, anneal_every=8,
                 seed=0):
        """depth_dims = (DIM_Y, DIM_X) and intrinsics = (focal, ppx, ppy) of the observed depth frames; plane: the table
        plane's matrix (camera space -> plane space, CalibratedPlane's), inverted here once.  model: a HandModel, whose
        dimensions are used; mirrored: fit the other hand (use two fitters for two hands).  window: (x0, y0, ww, wh), the
        part of the frame that is drawn and priced; default the whole frame (see window_around).  labels: the scheme the
        candidates are drawn with ('fine', 'coarse', 'tips' or a part -> id table), which should be the observed labels'
        scheme when w_label > 0.  target_labels: the observed ids that count as hand (each < 64); default 1..7.
        labels_reduce: the observed label map is [DIM_Y // r, DIM_X // r].  cost = w_boundary * (missing + extra) +
        w_label * label + sq.  sigma: float64 [26], the perturbation's scale per pose number (depth units and radians);
        default 8 mm for the wrist, 0.08 rad for yaw, pitch and roll, 0.05 for a spread and 0.12 for a flexion.  ranges:
        {name: (low, high)} over DEFAULT_RANGES (mm and radians; the names of HandModel.sample_poses), the same for either
        hand; every angle must stay within [-pi, pi].  The perturbation halves every anneal_every generations.
        These defaults come from a prototype on rendered frames and are unmeasured on real data.
        Nothing touches the device before the first fit."""
        self._lb = _lib.load("labels")
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        if not (1 <= self.DIM_X <= MAX_DIM and 1 <= self.DIM_Y <= MAX_DIM):
            raise ValueError(f"depth_dims {depth_dims} outside 1..{MAX_DIM}")
        self.f, self.ppx, self.ppy = (float(np.float32(v)) for v in np.asarray(intrinsics, np.float64).reshape(-1)[:3])
        if not (self.f > 0. and np.isfinite([self.f, self.ppx, self.ppy]).all()):
            raise ValueError(f"intrinsics {intrinsics}: the focal length must be positive and all three finite")
        plane = np.asarray(plane, np.float64).reshape(4, 4)
        self.cam_from_plane = np.linalg.inv(plane)
        if not np.isfinite(self.cam_from_plane).all():
            raise ValueError("the plane's matrix cannot be inverted")
        base = model or HandModel()
        self.model = base if base.is_mirrored == bool(mirrored) else HandModel(base.units_per_mm, bool(mirrored))
        self.candidates = int(candidates)
        if not 1 <= self.candidates <= MAX_CANDIDATES:
            raise ValueError(f"candidates {candidates} outside 1..{MAX_CANDIDATES}")
        self.labels_reduce = int(labels_reduce)
        if self.labels_reduce < 1 or self.DIM_X // self.labels_reduce < 1 or self.DIM_Y // self.labels_reduce < 1:
            raise ValueError(f"labels_reduce {labels_reduce} leaves no label pixel of {self.DIM_X}x{self.DIM_Y}")
        targets = list(range(1, 8)) if target_labels is None else [int(v) for v in np.asarray(target_labels).reshape(-1)]
        if not targets or min(targets) < 0 or max(targets) > 63:
            raise ValueError(f"target_labels {target_labels}: one id at least, each within 0..63")
        self.target_mask = sum(1 << v for v in set(targets))
        self.w_boundary, self.w_label = int(w_boundary), int(w_label)
        if not (0 <= self.w_boundary < 1 << 32 and 0 <= self.w_label < 1 << 32):
            raise ValueError("w_boundary and w_label are unsigned 32-bit integers")
        self.anneal_every = int(anneal_every)
        if self.anneal_every < 1:
            raise ValueError(f"anneal_every {anneal_every} < 1")
        self.seed = int(seed) & 0xFFFFFFFF
        u = self.model.units_per_mm
        self.sigma = pose_vector(DEFAULT_SIGMA, u) if sigma is None else np.array(sigma, np.float64).reshape(-1)
        if self.sigma.shape != (POSE_SIZE,) or not np.isfinite(self.sigma).all() or (self.sigma < 0.).any():
            raise ValueError("sigma: 26 finite numbers >= 0")
        self.lo, self.hi = pose_ranges(ranges, u)
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all() and (self.lo <= self.hi).all()):
            raise ValueError("ranges: every (low, high) finite with low <= high")
        if (self.lo[3:] < -np.pi).any() or (self.hi[3:] > np.pi).any():
            raise ValueError("ranges: every angle's range must lie within [-pi, pi]")
        table = HandModel.label_table(labels) if isinstance(labels, str) else np.asarray(labels, np.uint16).reshape(-1)
        if table.size != N_PARTS:
            raise ValueError(f"labels: a scheme's name or {N_PARTS} ids")
        self.tri_label = table[self.model.tri_part].astype(np.uint16)
        self._cfg = _Config()
        self._dev = None
        self._has_pose = False
        self.set_window(window)

    # ------------------------------------------------------------------ the window ------------------------------------------
    def set_window(self, window=None):
        """(x0, y0, ww, wh) inside the frame; None: the whole frame.  The next fit draws and prices that part only."""
        x0, y0, ww, wh = (0, 0, self.DIM_X, self.DIM_Y) if window is None else (int(v) for v in window)
        if x0 < 0 or y0 < 0 or ww < 1 or wh < 1 or x0 + ww > self.DIM_X or y0 + wh > self.DIM_Y:
            raise ValueError(f"window {window} is empty or leaves the {self.DIM_X}x{self.DIM_Y} frame")
        self.window = (x0, y0, ww, wh)
        c = self._cfg
        c.candidates, c.mirrored, c.anneal_every, c.seed = self.candidates, int(self.model.is_mirrored), self.anneal_every, self.seed
        c.x0, c.y0, c.ww, c.wh = self.window
        c.w_boundary, c.w_label, c.target_mask = self.w_boundary, self.w_label, self.target_mask
        c.f, c.ppx, c.ppy, c.zmin, c.zmax, c.reserved = self.f, self.ppx, self.ppy, Z_NEAR, Z_FAR, 0.
        for name, values in (("sigma", self.sigma), ("lo", self.lo), ("hi", self.hi),
                             ("cam_from_plane", self.cam_from_plane[:3].reshape(12)), ("geometry", geometry_of(self.model))):
            getattr(c, name)[:] = [float(v) for v in values]
        return self.window

    def window_around(self, pose, margin_mm=20.):
        """(x0, y0, ww, wh): the frame's part that the hand at `pose` can reach, from the projection (on the host) of a
        sphere about the wrist that holds the model in every pose, grown by margin_mm.  The whole frame when the sphere
        comes nearer than the near plane."""
        hm, u = hand_model, self.model.units_per_mm
        reach = max([np.hypot(*hm.FINGER_BASE[f]) + sum(hm.PHALANX_LENGTH[f]) + max(hm.PHALANX_RADIUS[f]) for f in range(5)] +
                    [np.hypot(hm.PALM_LENGTH, hm.PALM_HALF_WIDTH) + hm.PALM_HALF_THICKNESS])
        R = (reach + float(margin_mm)) * u
        pose = np.asarray(pose, np.float64).reshape(POSE_SIZE)
        c = self.cam_from_plane @ np.array([pose[0], pose[1], pose[2], 1.])
        if not c[2] - R > Z_NEAR:
            return (0, 0, self.DIM_X, self.DIM_Y)

        def extent(along, pp, size):
            # the sphere between the two planes through the camera and the image's other axis that touch it
            d = np.hypot(along, c[2])
            centre, half = np.arctan2(along, c[2]), np.arcsin(R / d)
            low = max(0, int(np.floor(self.f * np.tan(centre - half) + pp)))
            high = min(size, int(np.ceil(self.f * np.tan(centre + half) + pp)) + 1)
            return low, high
        x_lo, x_hi = extent(c[0], self.ppx, self.DIM_X)
        y_lo, y_hi = extent(c[1], self.ppy, self.DIM_Y)
        if x_hi <= x_lo or y_hi <= y_lo:
            raise ValueError("the hand at this pose is outside the frame")
        return (x_lo, y_lo, x_hi - x_lo, y_hi - y_lo)

    # ------------------------------------------------------------------ the device ------------------------------------------
    def workspace_bytes(self):
        return int(self._lb.rdf_pose_fit_workspace_bytes(self.candidates, self.window[2], self.window[3]))

    def _device(self):
        if self._dev is None:
            self._rt = get_runtime()
            m = self.model
            self._dev = {"verts": to_device(m.verts.astype(np.float32)), "vert_part": to_device(m.vert_part.astype(np.int32)),
                         "tris": to_device(m.tris.astype(np.int32)), "tri_label": to_device(self.tri_label),
                         "state": DeviceArray((STATE_BYTES,), np.uint8).fill(0), "workspace": None}
        need = self.workspace_bytes()
        ws = self._dev["workspace"]
        if ws is None or ws.nbytes < need:
            # the key planes start out empty (every byte 0xFF) and every call leaves them so
            self._dev["workspace"] = DeviceArray((need,), np.uint8).fill(0xFF)
        return self._dev

    def _frame(self, depth, labels):
        r = self.labels_reduce
        want = ((self.DIM_Y, self.DIM_X), (self.DIM_Y // r, self.DIM_X // r))
        out = []
        for a, shape, what in ((depth, want[0], "depth"), (labels, want[1], "labels")):
            if isinstance(a, np.ndarray):
                a = to_device(np.ascontiguousarray(a, np.uint16))
            if hasattr(a, "shape") and hasattr(a, "dtype"):
                if np.dtype(a.dtype) != np.uint16 or int(np.prod(a.shape)) != shape[0] * shape[1]:
                    raise ValueError(f"{what}: uint16 {shape} expected, got {a.dtype} {tuple(a.shape)}")
            out.append(a)
        return out

    def _run(self, depth, labels, generations, fresh, history_ptr):
        d = self._dev
        rc = self._lb.rdf_pose_fit(int(generations), int(bool(fresh)), ctypes.addressof(self._cfg), d["state"].ptr, self.DIM_X,
                                   self.DIM_Y, device_ptr(depth), device_ptr(labels), self.labels_reduce,
                                   int(d["verts"].shape[0]), d["verts"].ptr, d["vert_part"].ptr, int(d["tris"].shape[0]),
                                   d["tris"].ptr, d["tri_label"].ptr, d["workspace"].ptr, history_ptr, self._rt.stream())
        _lib.check(self._lb, rc, "rdf_pose_fit")
        d["state"].mark_dirty()
        d["workspace"].mark_dirty()

    def _checked_pose(self, init_pose, fresh):
        """The host's part of starting a fit: what init_pose must be, before anything touches the device."""
        if init_pose is None:
            if not self._has_pose:
                raise ValueError("the first fit needs init_pose")
            return None
        pose = np.array(init_pose, np.float64).reshape(-1)
        if pose.shape != (POSE_SIZE,) or not np.isfinite(pose).all():
            raise ValueError("init_pose: 26 finite numbers")
        if not fresh:
            raise ValueError("init_pose replaces the incumbent, whose cost is then unknown: that needs fresh=True")
        return pose

    def _start(self, pose):
        if pose is not None:
            self._dev["state"][0:POSE_SIZE * 8].set(pose.view(np.uint8))
            self._has_pose = True

    def fit(self, depth, labels, init_pose=None, generations=24, fresh=True):
        """Enqueue `generations` generations against one frame: depth uint16 [DIM_Y, DIM_X] and labels uint16 [DIM_Y // r,
        DIM_X // r] (device arrays; numpy arrays are uploaded).  init_pose float64 [26] replaces the incumbent (plane
        space, depth units and radians); without it the fit goes on from the last one's.  fresh: the frame is new -- the
        incumbent is priced against it as candidate 0 and the generation and accepted counters restart; fresh=False
        continues the last fit on the same frame, so that fit(a) then fit(b, fresh=False) is fit(a + b).  Nothing is read
        back: the returned PoseFitResult holds a device copy of the state and the history."""
        generations = int(generations)
        if generations < 0:
            raise ValueError(f"generations {generations} < 0")
        pose = self._checked_pose(init_pose, fresh)
        self._device()
        depth, labels = self._frame(depth, labels)
        self._start(pose)
        buf = DeviceArray((STATE_BYTES + 8 * generations,), np.uint8)
        self._run(depth, labels, generations, fresh, buf.ptr + STATE_BYTES if generations else None)
        buf[0:STATE_BYTES].copy_from(self._dev["state"])
        return PoseFitResult(self, buf, generations)

    def track(self, depth_frames, label_frames, init_pose, generations=24):
        """Fit frame after frame (sequences of frames as `fit` takes them, or device arrays [N, ...]): the first from
        init_pose, each later one from the frame before's incumbent, every one fresh.  Each frame's state and history go
        device to device into a row of the PoseTrackResult, which is read back once, by its get()."""
        generations, n = int(generations), len(depth_frames)
        if generations < 1 or n < 1 or len(label_frames) != n:
            raise ValueError("track: generations >= 1 and as many label frames as depth frames, one at least")
        pose = self._checked_pose(init_pose, True)
        self._device()
        row = STATE_BYTES + 8 * generations
        buf = DeviceArray((n, row), np.uint8)
        for i in range(n):
            depth, labels = self._frame(depth_frames[i], label_frames[i])
            self._start(pose if i == 0 else None)
            self._run(depth, labels, generations, True, buf.ptr + i * row + STATE_BYTES)
            buf[i][0:STATE_BYTES].copy_from(self._dev["state"])
        return PoseTrackResult(self, buf, n, generations)
