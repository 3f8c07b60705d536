"""Drop-in for the reference's compiled `cpp_grouping` module (/root/reference/src/cpp_grouping/cpp_grouping.pyx): the
same `CppGrouping().make_groups(in_arr, coords_arr, group_info_arr, pct_thresh)` on host numpy arrays, computed on the GPU
by rdf_hand_groups (level 0: `in_arr` is already the shrunk image).

Same results as grouping.cpp:82-183 bit for bit, with two documented differences: the coordinate rows of each group are
listed in raster order (the reference lists them in breadth-first order; its only consumer, 3d_bz.py:243-250, scatters
them into an image, so only the set matters), and the centroid of a side without a winner is written as 0.0 (the reference
leaves those two floats as they were).  `sys.modules["cpp_grouping"] = importlib.import_module("3d-beats_amd.cpp_grouping")`
lets `from cpp_grouping import CppGrouping` (3d_bz.py) find it; see INTEGRATION.md."""
import numpy as np

from . import _lib
from .device import DeviceArray, get_runtime


class CppGrouping:
    def __init__(self):
        self._rt = get_runtime()
        self._lib = self._rt.lib
        self._key = None

    def _buffers(self, dim_y, dim_x):
        if self._key != (dim_y, dim_x):
            p = dim_y * dim_x
            self._img = DeviceArray((max(p, 1),), np.uint16)
            self._groups = DeviceArray((max(p, 1),), np.uint16)
            self._coords = DeviceArray((max(p, 1), 3), np.int32)
            self._g_info = DeviceArray((2, 3), np.float32)
            nbytes = int(self._lib.rdf_hand_groups_workspace_bytes(1, dim_x, dim_y, 0))
            self._ws = DeviceArray((max(nbytes, 8),), np.uint8)
            self._key = (dim_y, dim_x)

    def make_groups(self, in_arr, coords_arr, group_info_arr, pct_thresh):
        """in_arr uint16 [dim_y, dim_x] (nonzero = foreground); coords_arr int32 [>= dim_y*dim_x, 3] receives (y, x, group)
        rows, group 1 then group 2; group_info_arr float32 [2, 3] receives {size, c_x, c_y} per group.  Both in place."""
        img = np.ascontiguousarray(in_arr, dtype=np.uint16)
        dim_y, dim_x = int(img.shape[0]), int(img.shape[1])
        assert coords_arr.dtype == np.int32 and group_info_arr.dtype == np.float32 and group_info_arr.size == 6
        self._buffers(dim_y, dim_x)
        p = dim_y * dim_x
        if p:
            self._img[:p].set(img.reshape(-1))
        rc = self._lib.rdf_hand_groups(self._img.ptr, 1, dim_x, dim_y, 0, float(np.float32(pct_thresh)), self._groups.ptr,
                                       self._g_info.ptr, None, self._coords.ptr, self._ws.ptr, 0, self._rt.stream())
        _lib.check(self._lib, rc, "rdf_hand_groups")
        self._coords.mark_dirty()
        self._g_info.mark_dirty()
        g_info = self._g_info.get()
        n = int(g_info[0, 0]) + int(g_info[1, 0])
        group_info_arr.reshape(2, 3)[...] = g_info
        if n:
            coords_arr.reshape(-1, 3)[:n] = self._coords[:n].get()
