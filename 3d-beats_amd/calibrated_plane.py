"""The table plane, fitted on the device: the reference's `CalibratedPlane` (/root/reference/src/calibrated_plane.py) on
librdf_frontend.so.

Same names and the same call as there -- `CalibratedPlane(num_random_guesses, plane_z_outlier_threshold)`, `is_set()`,
`get_mat()`, `make(pts_gpu, img_dims, start_mat=None)`, `.plane`, and the three kernels as attributes that accept and
ignore `grid=` / `block=`.  `make` runs rdf_calibrate_plane (candidates, inlier counts, the winner and its recentring) on
the current stream and reads one 112-byte record back, where the reference reads every candidate's count.  The random
draws come from a seeded `torch.Generator` on the device (the reference's curand XORWOW stream cannot be reproduced), or
from the caller (`rand=`).  `make_async` leaves everything on the device and can be captured into a graph.  The exact
contract and its two deviations from the reference are in include/rdf_frontend.h.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

RESULT_DTYPE = np.dtype([("plane", np.float32, (16,)), ("best_index", np.int32), ("best_count", np.int32),
                         ("c", np.float64, (4,)), ("status", np.int32), ("reserved", np.int32)])
assert RESULT_DTYPE.itemsize == 112
PLANE_OK, PLANE_NONE = 0, 1


def _dims(img_dims):
    dim_x, dim_y = (int(v) for v in np.asarray(img_dims).reshape(-1)[:2])
    return dim_x, dim_y


class CalibratedPlane:
    def __init__(self, num_random_guesses, plane_z_outlier_threshold, seed=None):
        import torch
        self._rt = get_runtime()
        self._fe = _lib.load("frontend")
        self.num_random_guesses = int(num_random_guesses)
        self.plane_z_outlier_threshold = float(plane_z_outlier_threshold)
        G = self.num_random_guesses
        assert G > 0
        self._gen = torch.Generator(device="cuda")
        if seed is not None:
            self._gen.manual_seed(int(seed))
        else:
            self._gen.seed()
        self.rand_cu = DeviceArray((G, 32), np.float32)
        nbytes = int(self._fe.rdf_calibrate_plane_workspace_bytes(G))
        self._ws = DeviceArray((nbytes,), np.uint8)
        self.candidate_planes_cu = DeviceArray((G, 4, 4), np.float32, self._ws._st, self._ws._off)
        self.num_inliers_cu = DeviceArray((G,), np.int32, self._ws._st, self._ws._off + G * 64)
        self.plane_cu = DeviceArray((4, 4), np.float32).fill(0)     # the device copy of .plane (make_async writes it)
        self.result_cu = DeviceArray((RESULT_DTYPE.itemsize,), np.uint8)
        self._start_cu = DeviceArray((4, 4), np.float32)
        self.plane = None

    def is_set(self):
        return self.plane is not None

    def get_mat(self):
        assert self.is_set()
        return self.plane

    def draw(self):
        """Fill rand_cu with uniform [0, 1) draws from the seeded device generator (stream-ordered)."""
        import torch
        t = torch.rand((self.num_random_guesses, 32), generator=self._gen, device="cuda", dtype=torch.float32)
        self.rand_cu.torch_bytes().copy_(t.view(torch.uint8).reshape(-1))
        self.rand_cu.mark_dirty()
        return self.rand_cu

    def make_async(self, pts_gpu, img_dims, start_mat=None, rand=None):
        """Fit on the current stream without reading anything back.  start_mat: None, a host 4x4 (uploaded: not capturable),
        or a device array of 16 float32 (e.g. this object's plane_cu).  rand: None (draw from the generator) or a device
        array float32 [G, 32].  The plane lands in plane_cu only when the fit succeeds; result_cu holds the record."""
        dim_x, dim_y = _dims(img_dims)
        p = pts_gpu.cu() if hasattr(pts_gpu, "cu") else pts_gpu
        assert np.dtype(p.dtype) == np.float32 and int(np.prod(p.shape)) >= dim_x * dim_y * 4, (p.shape, dim_x, dim_y)
        if rand is None:
            rand = self.draw()
        elif not hasattr(rand, "ptr") and not hasattr(rand, "cu") and not hasattr(rand, "data_ptr"):
            rand = self.rand_cu.set(np.ascontiguousarray(rand, np.float32).reshape(self.num_random_guesses, 32))
        r = rand.cu() if hasattr(rand, "cu") else rand
        assert np.dtype(r.dtype) == np.float32 and int(np.prod(r.shape)) == self.num_random_guesses * 32, r.shape
        start_ptr = None
        if start_mat is not None:
            if isinstance(start_mat, np.ndarray):
                start_ptr = self._start_cu.set(np.ascontiguousarray(start_mat, np.float32).reshape(4, 4)).ptr
            else:
                start_ptr = device_ptr(start_mat)
        rc = self._fe.rdf_calibrate_plane(self.num_random_guesses, self.plane_z_outlier_threshold, dim_x, dim_y,
                                          device_ptr(rand), device_ptr(pts_gpu), start_ptr, self._ws.ptr, self.plane_cu.ptr,
                                          self.result_cu.ptr, self._rt.stream())
        _lib.check(self._fe, rc, "rdf_calibrate_plane")
        for a in (self._ws, self.plane_cu, self.result_cu):
            a.mark_dirty()
        return self.result_cu

    def result(self):
        """The record of the last fit, read back (synchronises): a numpy structured scalar of RESULT_DTYPE."""
        return self.result_cu.get().view(RESULT_DTYPE)[0]

    def make(self, pts_gpu, img_dims, start_mat=None, rand=None):
        """calibrated_plane.py:37-87.  Fails like the reference's assert when no plane is found (no inliers, or the camera's
        z axis does not meet the plane near its origin), and then leaves .plane as it was."""
        self.make_async(pts_gpu, img_dims, start_mat, rand)
        r = self.result()
        assert int(r["status"]) == PLANE_OK, (f"no plane: best candidate {int(r['best_index'])} has "
                                              f"{int(r['best_count'])} inliers, |c[2]| = {abs(float(r['c'][2]))}")
        self.plane = np.array(r["plane"], np.float32).reshape(4, 4)
        return self.plane

    # ---- the reference's kernel attributes (calibrated_plane.py:25-27), grid= / block= ignored ----
    def make_plane_candidates(self, num_candidates, dim_x, dim_y, rand, pts, plane_candidates, grid=None, block=None):
        rc = self._fe.rdf_make_plane_candidates(int(num_candidates), int(dim_x), int(dim_y), device_ptr(rand),
                                                device_ptr(pts), None, device_ptr(plane_candidates), None, self._rt.stream())
        _lib.check(self._fe, rc, "rdf_make_plane_candidates")
        _touch(plane_candidates)

    def find_plane_ransac(self, num_candidates, threshold, num_pts, pts, candidate_planes, num_inliers, grid=None,
                          block=None):
        rc = self._fe.rdf_plane_inliers(int(num_candidates), float(threshold), int(num_pts), device_ptr(pts),
                                        device_ptr(candidate_planes), device_ptr(num_inliers), self._rt.stream())
        _lib.check(self._fe, rc, "rdf_plane_inliers")
        _touch(num_inliers)

    def filter_points_by_plane(self, num_pts, threshold, pts, grid=None, block=None):
        rc = self._fe.rdf_filter_points_by_plane(int(num_pts), float(threshold), device_ptr(pts), self._rt.stream())
        _lib.check(self._fe, rc, "rdf_filter_points_by_plane")
        _touch(pts)


def _touch(buf):
    b = buf.cu() if hasattr(buf, "cu") else buf
    if hasattr(b, "mark_dirty"):
        b.mark_dirty()
