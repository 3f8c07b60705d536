"""The converter's augmentation on the device: a recorded frame's points, as a triangle mesh, scaled, skewed, rotated or
shifted about the scene's centre in table-plane space and drawn back into a new depth image and a new aligned colour image
(the reference's rerender_image, src/live_data_convert.py:207-282, which goes through OpenGL) on librdf_labels.so.

`SceneRerender.center` sums the points on the device (the reference reads every point back to average them on the host),
`make_transform` composes the reference's obj_tform on the host, `run` rasterises: two launches on the current stream,
nothing read back.  The rasteriser's rules -- mesh, snapping to 1/256 pixel, fill rule, perspective-correct attributes,
nearest fragment with ties to the lowest triangle id -- are in include/rdf_labels.h.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

Z_NEAR, Z_FAR = 50., 50000.         # the planes of the reference's rs_projection call (live_data_convert.py:248)


def _arr(buf):
    return buf.cu() if hasattr(buf, "cu") else buf


def _translate(v):
    m = np.identity(4, np.float64)
    m[:3, 3] = v
    return m


class SceneRerender:
    def __init__(self, depth_dims, intrinsics, z_near=Z_NEAR, z_far=Z_FAR):
        """depth_dims = (DIM_Y, DIM_X); intrinsics = (focal, ppx, ppy) of the depth camera."""
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.f, self.ppx, self.ppy = (float(np.float32(v)) for v in np.asarray(intrinsics, np.float64).reshape(-1)[:3])
        self.z_near, self.z_far = float(z_near), float(z_far)
        n_px = self.DIM_X * self.DIM_Y
        # the key buffer starts out empty (every byte 0xFF) and every run leaves it so
        self._keys = DeviceArray((max(int(self._lb.rdf_rerender_workspace_bytes(self.DIM_X, self.DIM_Y)), 8),), np.uint8).fill(0xFF)
        self._center_ws = DeviceArray((int(self._lb.rdf_points_center_workspace_bytes(n_px)),), np.uint8)
        self.center_cu = DeviceArray((4,), np.float64)

    def center(self, pts, num_pts=None):
        """The four component sums of float32 [n, 4] points as a device double[4] (stream-ordered, nothing read back): the
        mean point is sums[:3] / sums[3] where every valid point has w == 1 and every other is zero."""
        p = _arr(pts)
        n = int(np.prod(p.shape)) // 4 if num_pts is None else int(num_pts)
        assert np.dtype(p.dtype) == np.float32 and n * 4 <= int(np.prod(p.shape)), (p.shape, p.dtype, n)
        assert n <= self.DIM_X * self.DIM_Y, "more points than this object's frame"
        rc = self._lb.rdf_points_center(n, device_ptr(p), self._center_ws.ptr, self.center_cu.ptr, self._rt.stream())
        _lib.check(self._lb, rc, "rdf_points_center")
        self._center_ws.mark_dirty()
        self.center_cu.mark_dirty()
        return self.center_cu

    @staticmethod
    def make_transform(plane, center, scale=1., skew=(0., 0., 0.), rotate=0., translate=(0., 0., 0.)):
        """obj_tform of live_data_convert.py:267-274 as float32 [4, 4], composed in float64 with column vectors (p' = M p, as
        `plane @ pt`): inv(plane) T(center) T(translate) S(scale + skew) T(-center) plane Rz(rotate) -- rotate about the
        camera's axis, go to plane space, scale about the centre and shift there, come back.  plane: the table plane (camera
        to plane space); center: the scene's centre in plane space."""
        plane = np.asarray(plane, np.float64).reshape(4, 4)
        c = np.asarray(center, np.float64).reshape(-1)[:3]
        s = np.identity(4, np.float64)
        s[0, 0], s[1, 1], s[2, 2] = float(scale) + np.asarray(skew, np.float64).reshape(-1)[:3]
        cr, sr = np.cos(float(rotate)), np.sin(float(rotate))
        rz = np.identity(4, np.float64)
        rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = cr, -sr, sr, cr
        m = (np.linalg.inv(plane) @ _translate(c) @ _translate(np.asarray(translate, np.float64).reshape(-1)[:3]) @ s
             @ _translate(-c) @ plane @ rz)
        m[3] = (0., 0., 0., 1.)          # a product of affine maps; the inverse's rounding must not say otherwise
        return m.astype(np.float32)

    def run(self, pts, color, obj_tform, depth_out, color_out):
        """pts: device float32 [H, W, 4] in camera space; color: device uint8 [H, W, 3]; obj_tform: host 4x4.  Writes every
        pixel of depth_out (device uint16 [H, W], 0 where nothing is drawn) and color_out (device uint8 [H, W, 3], not
        `color`)."""
        H, W = self.DIM_Y, self.DIM_X
        p, c, d, o = _arr(pts), _arr(color), _arr(depth_out), _arr(color_out)
        assert np.dtype(p.dtype) == np.float32 and int(np.prod(p.shape)) == H * W * 4, (p.shape, p.dtype)
        assert np.dtype(c.dtype) == np.uint8 and int(np.prod(c.shape)) == H * W * 3, (c.shape, c.dtype)
        assert np.dtype(d.dtype) == np.uint16 and int(np.prod(d.shape)) == H * W, (d.shape, d.dtype)
        assert np.dtype(o.dtype) == np.uint8 and int(np.prod(o.shape)) == H * W * 3, (o.shape, o.dtype)
        m = np.ascontiguousarray(np.asarray(obj_tform, np.float32).reshape(16))
        rc = self._lb.rdf_rerender(W, H, device_ptr(p), device_ptr(c), m.ctypes.data, self.f, self.ppx, self.ppy, self.z_near,
                                   self.z_far, self._keys.ptr, device_ptr(d), device_ptr(o), self._rt.stream())
        _lib.check(self._lb, rc, "rdf_rerender")
        for a in (self._keys, d, o):
            if hasattr(a, "mark_dirty"):
                a.mark_dirty()
        return depth_out, color_out
