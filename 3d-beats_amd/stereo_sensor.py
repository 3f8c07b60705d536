"""A simulated active stereo depth camera behind the hand renderer (librdf_labels.so: rdf_stereo_sense): a clean left render
and a clean right render of one scene become the depth frame such a camera would report -- a shadow of missing depth left of
whatever stands in front of the table, depth fattened round silhouettes, depth steps that grow with Z^2, no depth without
texture.  The reference matches two Blender renders of its projector pattern with OpenCV for this (datagen/stereo_alg.py).

`StereoSensor.sense` takes device arrays and gives device arrays, five launches per chunk of `max_frames` on the current
stream, nothing read back.  HandSceneRenderer.render, make_dataset and camera_sequence take a sensor as `sensor=`; the rules
are in include/rdf_labels.h.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

FRAME_SEED_STEP = 0x9E3779B9        # rule I: frame n under seed s is frame 0 under seed s + n * this
PATTERN_SEED = 0x3D5EA75


class StereoSensor:
    def __init__(self, depth_dims, intrinsics, baseline_mm=50., projector_offset=0.4, max_disparity=128, dot_density=0.25,
                 ambient=16, ir_noise_amp=6, census_margin=16, uniqueness=10, lr_max=1, dq_min=16, pattern_seed=PATTERN_SEED,
                 units_per_mm=10., max_frames=64):
        """depth_dims = (DIM_Y, DIM_X); intrinsics = (focal, ppx, ppy) of the depth camera (the focal length is what the
        sensor needs).  baseline_mm: the right imager's offset along +x; projector_offset: the projector's, as a share of the
        baseline; dot_density: the share of projector texels that carry a dot.  The other numbers are RdfStereoConfig's.  The
        workspace holds max_frames frames: longer batches go in chunks."""
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.f = float(np.float32(np.asarray(intrinsics, np.float64).reshape(-1)[0]))
        self.baseline = float(baseline_mm) * float(units_per_mm)           # depth units: what the right render is moved by
        self.max_frames = int(max_frames)
        assert self.max_frames >= 1
        fb16 = int(round(16. * self.f * self.baseline))
        self.config = _lib.StereoConfig(
            fb16=fb16, fbp16=int(round(fb16 * float(projector_offset))), max_disparity=int(max_disparity),
            dot_threshold=min(max(int(float(dot_density) * 4294967296.), 0), 0xFFFFFFFF), pattern_seed=int(pattern_seed) & 0xFFFFFFFF,
            ambient=int(ambient), ir_noise_amp=int(ir_noise_amp), census_margin=int(census_margin), uniqueness=int(uniqueness),
            lr_max=int(lr_max), dq_min=int(dq_min))
        n = int(self._lb.rdf_stereo_workspace_bytes(self.max_frames, self.DIM_X, self.DIM_Y, self.config.max_disparity))
        if n == 0 and self.DIM_X * self.DIM_Y > 0:
            raise _lib.RdfError(f"StereoSensor: {self.DIM_X} x {self.DIM_Y} with max_disparity {max_disparity} is out of range")
        self._workspace = DeviceArray((max(n, 8),), np.uint8)

    def config_dict(self):
        """The config's integers by name (what tests/stereo_numpy.py takes)."""
        return {name: int(getattr(self.config, name)) for name, _ in self.config._fields_}

    def sense(self, depth_l, labels_l, depth_r, seed=0, empty_depth=65535, depth_out=None, labels_out=None, ir_out=None,
              dq_out=None, reason_out=None):
        """depth_l, labels_l, depth_r: device uint16 [N, H, W], the clean renders (depth_r from the camera moved by the
        baseline along +x).  Returns device (depth uint16 [N, H, W], labels uint16 [N, H, W]); every pixel of both is written.
        ir_out uint8 [N, 2, H, W], dq_out uint16 [N, H, W], reason_out uint8 [N, H, W] are filled when given.  Frame n of a
        long batch gets the same image whatever max_frames is."""
        H, W = self.DIM_Y, self.DIM_X
        N = int(depth_l.shape[0])
        for a in (depth_l, labels_l, depth_r):
            assert np.dtype(a.dtype) == np.uint16 and int(np.prod(a.shape)) == N * H * W, (a.shape, a.dtype)
        depth_out = DeviceArray((N, H, W), np.uint16) if depth_out is None else depth_out
        labels_out = DeviceArray((N, H, W), np.uint16) if labels_out is None else labels_out
        for o, dtype, per in ((depth_out, np.uint16, 1), (labels_out, np.uint16, 1), (ir_out, np.uint8, 2), (dq_out, np.uint16, 1),
                              (reason_out, np.uint8, 1)):
            assert o is None or (np.dtype(o.dtype) == dtype and int(np.prod(o.shape)) == N * per * H * W), (o.shape, o.dtype)
        ptrs = [device_ptr(o) for o in (depth_l, labels_l, depth_r, depth_out, labels_out, ir_out, dq_out, reason_out)]
        size = (2, 2, 2, 2, 2, 2, 2, 1)             # bytes per pixel and frame

        def at(k, a):
            return None if ptrs[k] is None else ptrs[k] + a * H * W * size[k]
        for a in range(0, N, self.max_frames):
            b = min(N - a, self.max_frames)
            rc = self._lb.rdf_stereo_sense(b, W, H, at(0, a), at(1, a), at(2, a), self.config,
                                           (int(seed) + a * FRAME_SEED_STEP) & 0xFFFFFFFF, int(empty_depth), self._workspace.ptr,
                                           at(3, a), at(4, a), at(5, a), at(6, a), at(7, a), self._rt.stream())
            _lib.check(self._lb, rc, "rdf_stereo_sense")
        for o in (self._workspace, depth_out, labels_out, ir_out, dq_out, reason_out):
            if hasattr(o, "mark_dirty"):
                o.mark_dirty()
        return depth_out, labels_out
