"""Glove colours to class labels on the device: `make_color_mapping` and the per-frame labelling of the reference's
converter (the reference's src/live_data_convert.py:156-204, 413-458) on librdf_labels.so.

`ColorLabeler.make_color_mapping` runs every try and every iteration of the reference's EM loop in one stream-ordered call
(rdf_make_color_mapping: one read of the frame per iteration for all tries, the colour update and the choice of the best
try on the device) and reads 80 bytes + the mapping back, where the reference makes tries x iterations launches with a
read back and an upload between every two.  `label_frame` is one launch per frame: mask, snap to the mapping, label ids, the
RGBA debug image and the depth's 0 -> 65535.  The `_async` forms read nothing back and can be captured into a graph.
The semantics (integer arithmetic, ties, empty groups, which index labels a duplicate colour) are in include/rdf_labels.h.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

RESULT_DTYPE = np.dtype([("best_try", np.int32), ("tries", np.int32), ("best_cost", np.float64), ("cost", np.float64, (8,))])
assert RESULT_DTYPE.itemsize == 80
MAX_COLORS, MAX_TRIES = 16, 8


def _is_device(a):
    return hasattr(a, "ptr") or hasattr(a, "cu") or hasattr(a, "data_ptr")


def _arr(buf):
    return buf.cu() if hasattr(buf, "cu") else buf


def _touch(*bufs):
    for b in bufs:
        b = _arr(b)
        if hasattr(b, "mark_dirty"):
            b.mark_dirty()


class ColorLabeler:
    def __init__(self, num_colors, num_tries=8, num_iterations=32):
        """num_colors = --colors of the reference (1..16); num_tries, num_iterations = its COLOR_EM_NUM_TRIES (<= 8) and
        COLOR_EM_ITERATIONS."""
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.num_colors, self.num_tries, self.num_iterations = int(num_colors), int(num_tries), int(num_iterations)
        assert 1 <= self.num_colors <= MAX_COLORS and 1 <= self.num_tries <= MAX_TRIES and self.num_iterations >= 1
        K, T = self.num_colors, self.num_tries
        self._ws = DeviceArray((int(self._lb.rdf_color_mapping_workspace_bytes(T, K)),), np.uint8)
        self.try_colors_cu = DeviceArray((T, K, 3), np.uint8, self._ws._st, self._ws._off)   # every try's final colours
        self.init_cu = DeviceArray((T, K, 3), np.uint8)
        self.color_mapping_gpu = DeviceArray((K, 3), np.uint8).fill(0)       # the reference's name for the device copy
        self.result_cu = DeviceArray((RESULT_DTYPE.itemsize,), np.uint8)
        self.color_mapping = None
        self.costs = None
        self.best_try = None
        self._on_device = False
        self._image = None
        self._out = None

    def is_set(self):
        return self._on_device

    def draw_init_colors(self):
        """The reference's starting colours: np.random.uniform(0, 255, (K, 3)).astype(np.uint8) once per try, in try order,
        from numpy's global generator (live_data_convert.py:168)."""
        return np.stack([np.random.uniform(0, 255, (self.num_colors, 3)).astype(np.uint8) for _ in range(self.num_tries)])

    def _color_image(self, color_image):
        """A device uint8 [H, W, 3]; a host array is uploaded into a buffer of this object."""
        if _is_device(color_image):
            a = _arr(color_image)
        else:
            h = np.ascontiguousarray(color_image, np.uint8)
            if self._image is None or tuple(self._image.shape) != h.shape:
                self._image = DeviceArray(h.shape, np.uint8)
            a = self._image.set(h)
        assert np.dtype(a.dtype) == np.uint8 and len(a.shape) == 3 and a.shape[2] == 3, (a.shape, a.dtype)
        return a

    def make_color_mapping_async(self, color_image, init_colors=None):
        """Fit on the current stream without reading anything back.  init_colors: None (drawn as the reference draws them),
        a host uint8 [tries, K, 3] (both uploaded: not capturable), or a device array of that shape.  The mapping lands in
        color_mapping_gpu, the record in result_cu."""
        img = self._color_image(color_image)
        K, T = self.num_colors, self.num_tries
        if init_colors is None:
            init_colors = self.draw_init_colors()
        if not _is_device(init_colors):
            init_colors = self.init_cu.set(np.ascontiguousarray(init_colors, np.uint8).reshape(T, K, 3))
        init = _arr(init_colors)
        assert np.dtype(init.dtype) == np.uint8 and int(np.prod(init.shape)) == T * K * 3, init.shape
        rc = self._lb.rdf_make_color_mapping(int(img.shape[0]) * int(img.shape[1]), device_ptr(img), T, self.num_iterations, K,
                                             device_ptr(init), self._ws.ptr, self.color_mapping_gpu.ptr, self.result_cu.ptr,
                                             self._rt.stream())
        _lib.check(self._lb, rc, "rdf_make_color_mapping")
        _touch(self._ws, self.color_mapping_gpu, self.result_cu)
        self._on_device = True
        return self.color_mapping_gpu

    def result(self):
        """The record of the last fit, read back (synchronises): a numpy structured scalar of RESULT_DTYPE."""
        return self.result_cu.get().view(RESULT_DTYPE)[0]

    def make_color_mapping(self, color_image, init_colors=None):
        """live_data_convert.py:156-204: the best of num_tries fits of num_colors colours to the frame's non-black pixels, as
        uint8 [K, 3] (also kept on the device).  Afterwards .costs holds every try's cost and .best_try the winner."""
        self.make_color_mapping_async(color_image, init_colors)
        r = self.result()
        self.costs = np.array(r["cost"][:self.num_tries], np.float64)
        self.best_try = int(r["best_try"])
        self.color_mapping = self.color_mapping_gpu.get()
        return self.color_mapping

    def set_color_mapping(self, mapping):
        """Use a known mapping (uint8 [K, 3])."""
        self.color_mapping = np.ascontiguousarray(mapping, np.uint8).reshape(self.num_colors, 3).copy()
        self.color_mapping_gpu.set(self.color_mapping)
        self._on_device = True

    def mask_color_image(self, color_image, mask_labels, mask_label):
        """live_data_convert.py:421 on the device, in place: black where mask_labels != mask_label.  The first frame needs
        it before make_color_mapping (label_frame masks by itself)."""
        img = _arr(color_image)
        rc = self._lb.rdf_mask_color_image(int(img.shape[1]), int(img.shape[0]), device_ptr(img), device_ptr(mask_labels),
                                           int(mask_label), self._rt.stream())
        _lib.check(self._lb, rc, "rdf_mask_color_image")
        _touch(img)

    def label_frame(self, color_image, depth=None, mask_labels=None, mask_label=None, labels=None, labels_rgba=None):
        """live_data_convert.py:413-458 for one frame, one launch on the current stream, nothing read back.  color_image:
        device uint8 [H, W, 3], snapped in place (a host array is uploaded to a buffer of this object first).  depth: device
        uint16 [H, W] or None, 0 -> 65535 in place.  mask_labels (device uint16 [H, W]) with mask_label: pixels elsewhere
        become black first.  Returns (labels uint16 [H, W], labels_rgba uint8 [H, W, 4]) on the device: the caller's
        buffers when given, else buffers of this object that the next call overwrites."""
        assert self.is_set(), "no colour mapping: make_color_mapping() or set_color_mapping() first"
        assert (mask_labels is None) == (mask_label is None), "mask_labels and mask_label go together"
        img = self._color_image(color_image)
        H, W = int(img.shape[0]), int(img.shape[1])
        if labels is None or labels_rgba is None:
            if self._out is None or tuple(self._out[0].shape) != (H, W):
                self._out = (DeviceArray((H, W), np.uint16), DeviceArray((H, W, 4), np.uint8))
            labels = self._out[0] if labels is None else labels
            labels_rgba = self._out[1] if labels_rgba is None else labels_rgba
        for buf, n in ((depth, H * W), (mask_labels, H * W), (labels, H * W)):
            if buf is not None:
                b = _arr(buf)
                assert np.dtype(b.dtype) == np.uint16 and int(np.prod(b.shape)) == n, (b.shape, b.dtype)
        r = _arr(labels_rgba)
        assert np.dtype(r.dtype) == np.uint8 and int(np.prod(r.shape)) == H * W * 4, r.shape
        rc = self._lb.rdf_label_frame(W, H, self.num_colors, self.color_mapping_gpu.ptr, device_ptr(img),
                                      device_ptr(mask_labels), int(mask_label or 0), device_ptr(depth), device_ptr(labels),
                                      device_ptr(labels_rgba), self._rt.stream())
        _lib.check(self._lb, rc, "rdf_label_frame")
        _touch(img, labels, labels_rgba, *([depth] if depth is not None else []))
        return labels, labels_rgba

    def id_to_color(self):
        """The id_to_color table of config.json (live_data_convert.py:291-294): id 0 transparent, id i + 1 = mapping[i]."""
        assert self.color_mapping is not None, "make_color_mapping() first"
        table = {'0': [0, 0, 0, 0]}
        for c_id in range(self.num_colors):
            c = self.color_mapping[c_id]
            table[str(c_id + 1)] = [int(c[0]), int(c[1]), int(c[2]), 255]
        return table
