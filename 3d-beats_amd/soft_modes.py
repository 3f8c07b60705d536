"""Soft modes: mean-shift mode finding on a label map in which every pixel pulls with a weight, the forest's confidence in it
(rules S of include/rdf_labels.h; `rdf_labels_weighted_modes` of librdf_labels.so).

`WeightedModes` mirrors `MeanShift` with one more map: `weights` uint16 of the labels' shape, or None (every weight 1).  For
a plain forest, `labels_out` and `conf_out` of `DecisionTreeEvaluator.get_posteriors_forest` go straight in; for a layered
stack `LayeredDecisionForest.composite_weights` makes the weight map of the composite.  Not in the reference, which keeps no
posterior.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime


class WeightedModes:
    def __init__(self):
        self._rt = get_runtime()
        self._lib = _lib.load("labels")
        self.means = None       # DeviceArray float64 [n, num_labels, 2] of the last run_device() without `out`
        self.list_cap = int(self._lib.rdf_labels_weighted_modes_list_cap())

    @staticmethod
    def _dims(labels, weights):
        shape = tuple(int(v) for v in labels.shape)
        n = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
        if weights is not None:
            assert tuple(int(v) for v in weights.shape) == shape and np.dtype(weights.dtype) == np.uint16, (weights.shape, shape)
        assert np.dtype(labels.dtype) == np.uint16, labels.dtype
        return n, shape[-2], shape[-1]

    def run_device(self, num_rounds, labels, weights, num_labels, variances, out=None):
        """Leaves the means on the device: DeviceArray float64 [num_labels, 2] for one frame ([dim_y, dim_x] or [1, dim_y,
        dim_x] maps), [n, num_labels, 2] for n; `out` = a float64 device array of n * num_labels * 2 elements that receives
        them instead of self.means."""
        n, dim_y, dim_x = self._dims(labels, weights)
        if out is None:
            shape = (num_labels, 2) if n == 1 else (n, num_labels, 2)
            if self.means is None or tuple(self.means.shape) != shape:
                self.means = DeviceArray(shape, np.float64)
            out = self.means
        assert int(np.prod(out.shape)) == n * 2 * int(num_labels) and np.dtype(out.dtype) == np.float64
        self._call(num_rounds, labels, weights, n, dim_x, dim_y, num_labels, variances, out.ptr)
        out.mark_dirty()
        return out

    def run(self, num_rounds, labels, weights, num_labels, variances):
        """The per-class modes as a host float64 array [num_labels, 2] = (x, y) ([n, num_labels, 2] for n frames)."""
        return self.run_device(num_rounds, labels, weights, num_labels, variances).get()

    def run_device_with_heights(self, num_rounds, labels, weights, num_labels, variances, class_ids, n_ids, depth_images,
                                labels_reduce, intrinsics, plane, means_out_ptr, heights_out_ptr, heights_stride=None):
        """Modes and fingertip heights of n >= 1 frames in ONE launch: labels and weights [n, dim_y, dim_x] (or one 2-D map),
        depth_images the frames' depth; class_ids int32 [n_ids] and plane float32 [4, 4] on the device.  The outputs are raw
        device-accessible pointers: means float64 [n, num_labels, 2] at means_out_ptr, the height of id i of frame f at
        heights_out_ptr + 8 * (f * heights_stride + i) (heights_stride defaults to n_ids).  Each frame is bit for bit what a
        call for it alone gives."""
        n, dim_y, dim_x = self._dims(labels, weights)
        ddy, ddx = (int(v) for v in depth_images.shape[-2:])
        assert int(np.prod(depth_images.shape)) == n * ddy * ddx, (labels.shape, depth_images.shape)
        self._call(num_rounds, labels, weights, n, dim_x, dim_y, num_labels, variances, int(means_out_ptr),
                   (device_ptr(class_ids), int(n_ids), device_ptr(depth_images), ddx, ddy, int(labels_reduce))
                   + tuple(float(v) for v in intrinsics)
                   + (device_ptr(plane), int(heights_out_ptr), int(n_ids if heights_stride is None else heights_stride)))

    def _call(self, num_rounds, labels, weights, n, dim_x, dim_y, num_labels, variances, means_ptr, heights=None):
        if heights is None:
            heights = (None, 0, None, 0, 0, 1, 0., 0., 0., 0., None, None, 0)
        rc = self._lib.rdf_labels_weighted_modes(device_ptr(labels), None if weights is None else device_ptr(weights), n, dim_x,
                                                 dim_y, int(num_labels), device_ptr(variances), int(num_rounds), means_ptr,
                                                 *heights, self._rt.stream())
        _lib.check(self._lib, rc, "rdf_labels_weighted_modes")
