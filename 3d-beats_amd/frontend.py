"""Raw camera depth -> table-free depth on the device: the per-frame chain of /root/reference/src/3d_bz.py:163-212
(deproject_points, transform_points by the calibrated plane, filter_points_by_plane, remove_missing_3d_points_from_depth_image,
gaussian_depth_filter) as one launch of rdf_frame_front, and the plane calibration of 3d_bz.py:172-178.

`FrameFrontEnd.run` is what feeds `HandGrouping.make_group_image`.  Its plane never leaves the device: `calibrate` fits it
with `CalibratedPlane` and `run` reads it from there, so a frame goes from raw depth to fingertip heights stream-ordered,
and `calibrate_async` + `run` can be captured into a graph.
"""
import numpy as np

from . import _lib
from .calibrated_plane import CalibratedPlane
from .cuda.points_ops import gaussian_kernel
from .device import DeviceArray, device_ptr, get_runtime


class FrameFrontEnd:
    def __init__(self, depth_dims, intrinsics, plane_z_threshold, gauss_sigma=2.0, k_size=5, num_random_guesses=25000,
                 seed=None):
        """depth_dims = (DIM_Y, DIM_X); intrinsics = (focal, ppx, ppy) of the depth camera (rs_util.py:44-45);
        plane_z_threshold = PLANE_Z_OUTLIER_THRESHOLD (40 in the app), used both to fit the plane and to cut the table;
        gauss_sigma <= 0.1 turns the Gaussian off, as the app's `if self.gauss_sigma > 0.1` does; k_size odd, <= 41."""
        self._rt = get_runtime()
        self._fe = _lib.load("frontend")
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.focal, self.ppx, self.ppy = (float(v) for v in np.asarray(intrinsics, np.float64).reshape(-1)[:3])
        self.plane_z_threshold = float(plane_z_threshold)
        self.gauss_sigma, self.k_size = float(gauss_sigma), int(k_size)
        self._weights = None
        if self.gauss_sigma > 0.1:
            self._weights = DeviceArray((self.k_size, self.k_size), np.float32).set(gaussian_kernel(self.k_size, self.gauss_sigma))
        self.calibrated_plane = CalibratedPlane(num_random_guesses, self.plane_z_threshold, seed)
        self.pts_cu = DeviceArray((self.DIM_Y, self.DIM_X, 4), np.float32).fill(0)
        self._plane_on_device = False

    def _frames(self, buf):
        d = buf.cu() if hasattr(buf, "cu") else buf
        assert tuple(d.shape[-2:]) == (self.DIM_Y, self.DIM_X) and np.dtype(d.dtype) == np.uint16, (d.shape, d.dtype)
        return d, int(np.prod(d.shape[:-2])) if len(d.shape) > 2 else 1

    def _deproject(self, depth):
        d, _ = self._frames(depth)
        self.pts_cu.fill(0)
        rc = self._fe.rdf_deproject_points(1, self.DIM_X, self.DIM_Y, self.ppx, self.ppy, self.focal, device_ptr(d),
                                           self.pts_cu.ptr, self._rt.stream())
        _lib.check(self._fe, rc, "rdf_deproject_points")

    def calibrate(self, depth, start_mat=None, rand=None):
        """Fit the table plane to the (first) frame of `depth`, as the app does on its first frame and on "recalibrate
        plane" (with start_mat = the current plane).  Returns the 4x4 plane; raises AssertionError when none is found."""
        self._deproject(depth)
        plane = self.calibrated_plane.make(self.pts_cu, (self.DIM_X, self.DIM_Y), start_mat, rand)
        self._plane_on_device = True
        return plane

    def calibrate_async(self, depth, rand=None, from_current=False):
        """calibrate() without the read back (capturable when `rand` is a device array).  from_current: the current device
        plane competes as candidate 0.  The plane is replaced only when the fit succeeds; calibrated_plane.result() says."""
        self._deproject(depth)
        start = self.calibrated_plane.plane_cu if from_current else None
        self.calibrated_plane.make_async(self.pts_cu, (self.DIM_X, self.DIM_Y), start, rand)
        self._plane_on_device = True

    def set_plane(self, plane):
        """Use a known plane (row-major 4x4, the reference's CalibratedPlane.plane)."""
        self.calibrated_plane.plane_cu.set(np.ascontiguousarray(plane, np.float32).reshape(4, 4))
        self.calibrated_plane.plane = np.array(plane, np.float32).reshape(4, 4)
        self._plane_on_device = True

    def run(self, depth, depth_out, pts_out=None):
        """depth uint16 [DIM_Y, DIM_X] or [n, DIM_Y, DIM_X], 0 = no reading; depth_out the same shape (not the same buffer
        when the Gaussian is on); pts_out float32 [n,] DIM_Y, DIM_X, 4 or None.  All n frames use the current plane.
        Runs on the current stream and does not synchronise."""
        assert self._plane_on_device, "no plane: calibrate() or set_plane() first"
        d, n = self._frames(depth)
        o, n_out = self._frames(depth_out)
        assert n_out == n
        if pts_out is not None:
            p = pts_out.cu() if hasattr(pts_out, "cu") else pts_out
            assert np.dtype(p.dtype) == np.float32 and int(np.prod(p.shape)) == n * self.DIM_Y * self.DIM_X * 4, p.shape
        w = self._weights
        rc = self._fe.rdf_frame_front(device_ptr(d), n, self.DIM_X, self.DIM_Y, self.ppx, self.ppy, self.focal,
                                      self.calibrated_plane.plane_cu.ptr, self.plane_z_threshold,
                                      None if w is None else w.ptr, self.k_size if w is not None else 0, device_ptr(o),
                                      device_ptr(pts_out), self._rt.stream())
        _lib.check(self._fe, rc, "rdf_frame_front")
        for b in (o, pts_out):
            b = b.cu() if hasattr(b, "cu") else b
            if hasattr(b, "mark_dirty"):
                b.mark_dirty()
        return depth_out
