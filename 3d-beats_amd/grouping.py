"""The hand-group image on the device: what `HandPipeline` takes as `depth_image_mm_groups`.

The reference makes it with a host round trip at the end of every frame (/root/reference/src/3d_bz.py:213-263):
shrink_image on the GPU, synchronise, copy the 1/f-resolution frame to the host, `CppGrouping().make_groups` (a
breadth-first connected-components pass in C++, src/cpp_grouping/grouping.cpp), upload the coordinate list,
write_pixel_groups_to_stencil_image, grow_groups.  `HandGrouping.make_group_image` is that whole chain as one call on the
current stream (rdf_hand_groups), bit for bit; it never synchronises, so a frame can go from the depth image to the fingertip
heights without leaving the device, and the call can be captured into a graph.  The exact contract, and its one documented
difference (the centroid of a side without a winner is 0 here, uninitialised there), is in include/rdf_hip.h.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

PATH_AUTO, PATH_RESIDENT, PATH_GLOBAL = 0, 1, 2


class HandGrouping:
    def __init__(self, depth_dims, depth_mm_level, group_min_size, max_frames=1):
        """depth_dims = (DIM_Y, DIM_X) of the depth frame; depth_mm_level = the mip level of the group image (3 in the app);
        group_min_size = the size filter's pct_thresh (0.06 in the app, 3d_bz.py:63); max_frames = the largest batch."""
        self._rt = get_runtime()
        self._lib = self._rt.lib
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.depth_mm_level = int(depth_mm_level)
        self.group_min_size = float(group_min_size)
        self.max_frames = int(max_frames)
        self.depth_mm_dims = (self.DIM_Y >> self.depth_mm_level, self.DIM_X >> self.depth_mm_level)
        nbytes = int(self._lib.rdf_hand_groups_workspace_bytes(self.max_frames, self.DIM_X, self.DIM_Y, self.depth_mm_level))
        self._ws = DeviceArray((max(nbytes, 8),), np.uint8)
        self._g_info = DeviceArray((self.max_frames, 2, 3), np.float32)

    def make_group_image(self, depth_image, groups_out, g_info_out=None, components_out=None, coords_out=None,
                         path=PATH_AUTO):
        """depth_image: uint16 [DIM_Y, DIM_X] or [n, DIM_Y, DIM_X] on the device (GpuBuffer / DeviceArray), 0 = no pixel;
        groups_out: uint16 [n,] depth_mm_dims -- the grown hand-group image; g_info_out: float32 [n,] 2, 3 -- {size, c_x, c_y}
        of group 1 then group 2 (kept in an internal buffer when None); components_out: int32 like groups_out -- each
        pixel's component as its minimum raster index, -1 for background; coords_out: int32 [n,] Hm*Wm, 3 -- (y, x, group)
        rows, group 1 then group 2, each in raster order.  Runs on the current stream and does not synchronise."""
        d = depth_image.cu() if hasattr(depth_image, "cu") else depth_image
        n = int(np.prod(d.shape[:-2])) if len(d.shape) > 2 else 1
        assert tuple(d.shape[-2:]) == (self.DIM_Y, self.DIM_X) and np.dtype(d.dtype) == np.uint16, d.shape
        assert 1 <= n <= self.max_frames, f"{n} frames > max_frames {self.max_frames}"
        hm, wm = self.depth_mm_dims
        for buf, dt, per in ((groups_out, np.uint16, hm * wm), (g_info_out, np.float32, 6),
                             (components_out, np.int32, hm * wm), (coords_out, np.int32, hm * wm * 3)):
            if buf is not None:
                b = buf.cu() if hasattr(buf, "cu") else buf
                assert np.dtype(b.dtype) == dt and int(np.prod(b.shape)) == n * per, (b.shape, b.dtype)
        g_info = g_info_out if g_info_out is not None else self._g_info
        rc = self._lib.rdf_hand_groups(device_ptr(d), n, self.DIM_X, self.DIM_Y, self.depth_mm_level, self.group_min_size,
                                       device_ptr(groups_out), device_ptr(g_info), device_ptr(components_out),
                                       device_ptr(coords_out), self._ws.ptr, int(path), self._rt.stream())
        _lib.check(self._lib, rc, "rdf_hand_groups")
        for buf in (groups_out, g_info, components_out, coords_out):
            b = buf.cu() if hasattr(buf, "cu") else buf
            if hasattr(b, "mark_dirty"):
                b.mark_dirty()
        return groups_out

    @property
    def g_info(self):
        """The internal g_info buffer (DeviceArray float32 [max_frames, 2, 3]) of calls that passed no g_info_out."""
        return self._g_info
