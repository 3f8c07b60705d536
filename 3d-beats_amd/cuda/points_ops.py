"""The element-wise kernels either side of the forest, callable the way the reference's
apps call their PyCUDA counterparts (/root/reference/src/cuda/points_ops.py:16-44;
src/3d_bz.py:396-456; src/run_live_layered.py:117-122): positional arguments as there, `grid=` and
`block=` accepted and ignored (launch geometry belongs to the library).  The kernels that
touch the forest's input and output live here, and the three around the hand grouping (8f-3: shrink_image,
write_pixel_groups_to_stencil_image, grow_groups), and the five of the depth front end (deproject_points,
transform_points, filter_points_by_plane, remove_missing_3d_points_from_depth_image, gaussian_depth_filter; they live in
librdf_frontend.so, and frontend.FrameFrontEnd fuses them), and the three of the glove-colour converter
(split_pixels_by_nearest_color, apply_point_mapping, depths_from_points; librdf_labels.so, fused by
color_labels.ColorLabeler).  Mesh generation stays out of scope."""
import numpy as np

from .. import _lib
from ..device import DeviceArray, device_ptr, get_runtime

MAX_FILTER_SIZE = 41


def gaussian_kernel(k_size, sigma):
    """points_ops.py:9-14 without scipy: scipy.stats.norm.pdf(x, 0, sigma) is exp(-((x - 0) / sigma)**2 / 2) / sqrt(2 pi)
    / sigma in float64, here in that order; the outer product is normalised by its sum and rounded to float32 [k, k]."""
    assert k_size % 2 == 1, 'kernel must be odd'
    h = k_size // 2
    y = (np.linspace(-h, h, k_size) - 0.) / sigma
    kern1d = np.exp(-y ** 2 / 2.0) / np.sqrt(2 * np.pi) / sigma
    kern2d = np.outer(kern1d, kern1d)
    return (kern2d / kern2d.sum()).astype(np.float32)


class PointsOps:
    def __init__(self):
        self._rt = get_runtime()
        self._lib = self._rt.lib
        self.MAX_FILTER_SIZE = MAX_FILTER_SIZE
        self._gaussian_filter = None
        self._cached_filter_params = None

    def _ok(self, rc, name, *touched, lib=None):
        """lib: the front-end or labels library the call went to.  The methods below open those on first use (_lib.load keeps
        them for the process), so a process that only evaluates forests never needs them."""
        _lib.check(lib or self._lib, rc, name)
        for t in touched:
            t = t.cu() if hasattr(t, "cu") else t
            if hasattr(t, "mark_dirty"):
                t.mark_dirty()

    def convert_0s_to_maxuint(self, num_pixels, depth, grid=None, block=None):
        self._ok(self._lib.rdf_convert_0s_to_maxuint(device_ptr(depth), int(num_pixels), self._rt.stream()),
                 "rdf_convert_0s_to_maxuint", depth)

    def setup_depth_image_for_forest(self, num_pixels, pts, depth, grid=None, block=None):
        self._ok(self._lib.rdf_setup_depth_image_for_forest(device_ptr(pts), device_ptr(depth), int(num_pixels),
                                                            self._rt.stream()),
                 "rdf_setup_depth_image_for_forest", depth)

    def stencil_depth_image_by_group(self, img_dim, mipmap_level, group, g_in, d_in, d_out, grid=None, block=None):
        dim_x, dim_y = (int(v) for v in np.asarray(img_dim).reshape(-1)[:2])
        self._ok(self._lib.rdf_stencil_depth_image_by_group(dim_x, dim_y, int(mipmap_level), int(group), device_ptr(g_in),
                                                            device_ptr(d_in), device_ptr(d_out), self._rt.stream()),
                 "rdf_stencil_depth_image_by_group", d_out)

    def prepare_hand_depth(self, img_dim, mipmap_level, group, g_in, d_in, d_out, flip_x):
        """fill(0) + stencil_depth_image_by_group + flip_x (or copy) + convert_0s_to_maxuint of 3d_bz.py:396-420 as one
        pass: d_out = the frame as the forest wants it for this hand.  No reference counterpart as a single kernel."""
        dim_x, dim_y = (int(v) for v in np.asarray(img_dim).reshape(-1)[:2])
        self._ok(self._lib.rdf_prepare_hand_depth(dim_x, dim_y, int(mipmap_level), int(group), device_ptr(g_in),
                                                  device_ptr(d_in), device_ptr(d_out), 1 if flip_x else 0, self._rt.stream()),
                 "rdf_prepare_hand_depth", d_out)

    def prepare_hand_depth_batch(self, n, img_dim, mipmap_level, group, g_in, d_in, d_out, flip_x):
        """prepare_hand_depth for n frames in one launch (rdf_prepare_hand_depth_batch): g_in [n, dim_y >> level,
        dim_x >> level], d_in and d_out [n, dim_y, dim_x]; frame f of d_out is what prepare_hand_depth makes of frame f."""
        dim_x, dim_y = (int(v) for v in np.asarray(img_dim).reshape(-1)[:2])
        self._ok(self._lib.rdf_prepare_hand_depth_batch(int(n), dim_x, dim_y, int(mipmap_level), int(group), device_ptr(g_in),
                                                        device_ptr(d_in), device_ptr(d_out), 1 if flip_x else 0,
                                                        self._rt.stream()),
                 "rdf_prepare_hand_depth_batch", d_out)

    def flip_x(self, img_dim, img_in, img_out, grid=None, block=None):
        dim_x, dim_y = (int(v) for v in np.asarray(img_dim).reshape(-1)[:2])
        self._ok(self._lib.rdf_flip_x(dim_x, dim_y, device_ptr(img_in), device_ptr(img_out), self._rt.stream()),
                 "rdf_flip_x", img_out)

    def make_rgba_from_labels(self, dim_x, dim_y, num_colors, labels, colors, color_image, grid=None, block=None):
        self._ok(self._lib.rdf_make_rgba_from_labels(int(dim_x), int(dim_y), int(num_colors), device_ptr(labels),
                                                     device_ptr(colors), device_ptr(color_image), self._rt.stream()),
                 "rdf_make_rgba_from_labels", color_image)

    # ---- the hand-group image's host round trip, kernel for kernel (3d_bz.py:213-258); HandGrouping fuses it ----
    def shrink_image(self, img_dim_in, mipmap_level, d_in, d_out, grid=None, block=None):
        dim_x, dim_y = (int(v) for v in np.asarray(img_dim_in).reshape(-1)[:2])
        self._ok(self._lib.rdf_shrink_image(dim_x, dim_y, int(mipmap_level), device_ptr(d_in), device_ptr(d_out),
                                            self._rt.stream()),
                 "rdf_shrink_image", d_out)

    def write_pixel_groups_to_stencil_image(self, coords, num_coords, stencil, stencil_dims, grid=None, block=None):
        """stencil_dims = (rows, cols), as the reference passes depth_mm_dims."""
        d0, d1 = (int(v) for v in np.asarray(stencil_dims).reshape(-1)[:2])
        self._ok(self._lib.rdf_write_pixel_groups_to_stencil_image(device_ptr(coords), int(num_coords), device_ptr(stencil),
                                                                   d0, d1, self._rt.stream()),
                 "rdf_write_pixel_groups_to_stencil_image", stencil)

    def grow_groups(self, img_dim, g_in, g_out, grid=None, block=None):
        dim_x, dim_y = (int(v) for v in np.asarray(img_dim).reshape(-1)[:2])
        self._ok(self._lib.rdf_grow_groups(dim_x, dim_y, device_ptr(g_in), device_ptr(g_out), self._rt.stream()),
                 "rdf_grow_groups", g_out)

    # ---- the depth front end, kernel for kernel (3d_bz.py:163-212); frontend.FrameFrontEnd fuses it ----
    def deproject_points(self, imgs_dim, pp, f, imgs, pts, grid=None, block=None):
        """imgs_dim = (num_images, dim_x, dim_y, -1) int32, pp = (ppx, ppy) float32 (points_ops.cu:5-36).  Pixels with
        depth 0 keep what pts held."""
        n, dim_x, dim_y = (int(v) for v in np.asarray(imgs_dim).reshape(-1)[:3])
        ppx, ppy = (float(v) for v in np.asarray(pp, np.float32).reshape(-1)[:2])
        fe = _lib.load("frontend")
        self._ok(fe.rdf_deproject_points(n, dim_x, dim_y, ppx, ppy, float(np.float32(f)), device_ptr(imgs), device_ptr(pts),
                                         self._rt.stream()),
                 "rdf_deproject_points", pts, lib=fe)

    def transform_points(self, num_pts, pts, t, grid=None, block=None):
        """t: the host 4x4 float32 plane, row-major (passed by value, as the reference passes a glm::mat4)."""
        m = np.ascontiguousarray(np.asarray(t, np.float32).reshape(16))
        fe = _lib.load("frontend")
        self._ok(fe.rdf_transform_points(int(num_pts), device_ptr(pts), m.ctypes.data, self._rt.stream()),
                 "rdf_transform_points", pts, lib=fe)

    def filter_points_by_plane(self, num_pts, threshold, pts, grid=None, block=None):
        fe = _lib.load("frontend")
        self._ok(fe.rdf_filter_points_by_plane(int(num_pts), float(threshold), device_ptr(pts), self._rt.stream()),
                 "rdf_filter_points_by_plane", pts, lib=fe)

    def remove_missing_3d_points_from_depth_image(self, num_pixels, pts, depth, grid=None, block=None):
        fe = _lib.load("frontend")
        self._ok(fe.rdf_remove_missing_3d_points_from_depth_image(int(num_pixels), device_ptr(pts), device_ptr(depth),
                                                                  self._rt.stream()),
                 "rdf_remove_missing_3d_points_from_depth_image", depth, lib=fe)

    def gaussian_depth_filter(self, d_in, d_out, sigma, k_size=5):
        """points_ops.py:68-104: one frame of dims d_in.shape[-2:] (the reference passes only dim_x, dim_y, so of a
        batch only the first frame is filtered).  The weights are computed once per (sigma, k_size) and kept on the device."""
        assert k_size <= self.MAX_FILTER_SIZE
        assert len(d_in.shape) in (2, 3)
        dim_y, dim_x = d_in.shape[-2:]
        assert tuple(d_in.shape) == tuple(d_out.shape)
        assert np.dtype(d_in.dtype) == np.uint16 and np.dtype(d_out.dtype) == np.uint16
        if self._cached_filter_params is None or self._cached_filter_params != (sigma, k_size):
            if self._gaussian_filter is None:
                self._gaussian_filter = DeviceArray((self.MAX_FILTER_SIZE * self.MAX_FILTER_SIZE,), np.float32)
            k = gaussian_kernel(k_size, sigma).reshape(-1)
            self._gaussian_filter[0:k.shape[0]].set(k)
            self._cached_filter_params = (sigma, k_size)
        fe = _lib.load("frontend")
        self._ok(fe.rdf_gaussian_depth_filter(int(dim_x), int(dim_y), int(k_size), self._gaussian_filter.ptr,
                                              device_ptr(d_in), device_ptr(d_out), self._rt.stream()),
                 "rdf_gaussian_depth_filter", d_out, lib=fe)

    # ---- glove colours to labels, kernel for kernel (live_data_convert.py:179-187, 377-382, 434-441); ColorLabeler fuses it ----
    def split_pixels_by_nearest_color(self, dim_x, dim_y, num_colors, colors, color_image, pixel_counts_per_group, grid=None,
                                      block=None):
        """Adds onto pixel_counts_per_group uint64 [K, 5] = (pixels, sum r, sum g, sum b, sum cost as a float64)."""
        lb = _lib.load("labels")
        self._ok(lb.rdf_split_pixels_by_nearest_color(int(dim_x), int(dim_y), int(num_colors), device_ptr(colors),
                                                      device_ptr(color_image), device_ptr(pixel_counts_per_group),
                                                      self._rt.stream()),
                 "rdf_split_pixels_by_nearest_color", pixel_counts_per_group, lib=lb)

    def apply_point_mapping(self, dim_x, dim_y, num_colors, colors, color_image, grid=None, block=None):
        lb = _lib.load("labels")
        self._ok(lb.rdf_apply_point_mapping(int(dim_x), int(dim_y), int(num_colors), device_ptr(colors),
                                            device_ptr(color_image), self._rt.stream()),
                 "rdf_apply_point_mapping", color_image, lib=lb)

    def depths_from_points(self, imgs_dim, imgs, pts, grid=None, block=None):
        """imgs_dim = (num_images, dim_x, dim_y, -1) int32 (points_ops.cu:39-63): depth = (uint16)z where w > 0."""
        n, dim_x, dim_y = (int(v) for v in np.asarray(imgs_dim).reshape(-1)[:3])
        lb = _lib.load("labels")
        self._ok(lb.rdf_depths_from_points(n, dim_x, dim_y, device_ptr(imgs), device_ptr(pts), self._rt.stream()),
                 "rdf_depths_from_points", imgs, lib=lb)
