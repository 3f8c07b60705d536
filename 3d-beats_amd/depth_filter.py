"""The depth post-filter that stands between a stereo depth camera and `FrameFrontEnd` (librdf_frontend.so:
rdf_depth_filter): an edge-preserving spatial mean, a temporal filter with persistence and a row-wise hole fill, the chain a
depth camera's SDK runs on the host.  Here the frame stays on the device: `DepthPostFilter.run` is ONE launch for any number
of consecutive frames on the current stream, nothing is read back, and it can be captured into a graph.  The rules (S, T
and F, integer throughout) are in include/rdf_frontend.h.

`BeatsSession(..., post_filter=f)` passes every raw frame through `f` first.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime

FILL_MODES = {None: 0, "left": 1, "farthest": 2}
FLAG_BLENDED, FLAG_PERSISTED, FLAG_FILLED = 1, 2, 4


class DepthPostFilter:
    def __init__(self, depth_dims, spatial_radius=2, spatial_delta=60, temporal_alpha=0.4, temporal_delta=100, persistence=(2, 4),
                 fill="farthest", max_gap=32):
        """depth_dims = (DIM_Y, DIM_X).  spatial_radius 0, 1 or 2 (0 = no spatial stage), spatial_delta in depth units: the
        neighbours further than that from a pixel do not enter its mean.  temporal_alpha: the weight of the new reading (it is
        rounded to 256ths), None = no temporal stage; temporal_delta: a reading further than that from the filtered value
        restarts it; persistence = (need, span): a hole shows the filtered value while at least `need` of the last `span`
        frames had a reading.  fill: 'farthest' (the larger of the nearest readings left and right, i.e. the background),
        'left', or None; max_gap: how many columns away a reading may be.

        The defaults are the ones the rules were drafted with on simulated stereo frames (tests/stereo_cases.py's box scene);
        they have not been measured on a real camera's data."""
        self._rt = get_runtime()
        self._fe = _lib.load("frontend")
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        if fill not in FILL_MODES:
            raise ValueError(f"fill must be one of {list(FILL_MODES)}, not {fill!r}")
        need, span = persistence
        self.config = _lib.DepthFilterConfig(
            spatial_radius=int(spatial_radius), spatial_delta=int(spatial_delta), temporal=0 if temporal_alpha is None else 1,
            temporal_alpha=256 if temporal_alpha is None else int(round(float(temporal_alpha) * 256.)),
            temporal_delta=int(temporal_delta), persist_need=int(need), persist_span=int(span), fill_mode=FILL_MODES[fill],
            max_gap=int(max_gap))
        # the ranges are the library's to check: a call without frames checks them and launches nothing
        rc = self._fe.rdf_depth_filter(0, self.DIM_X, self.DIM_Y, None, ctypes.byref(self.config), None, None, None, None)
        _lib.check(self._fe, rc, "rdf_depth_filter (config)")
        self._state = None
        if self.config.temporal:
            n = int(self._fe.rdf_depth_filter_state_bytes(self.DIM_X, self.DIM_Y))
            self._state = DeviceArray((max(n // 4, 1),), np.uint32).fill(0)

    def config_dict(self):
        """The config's integers by name (what tests/depth_filter_numpy.py takes)."""
        return {name: int(getattr(self.config, name)) for name, _ in self.config._fields_}

    def reset(self):
        """Forget every pixel's history: the next frame is a first frame."""
        if self._state is not None:
            self._state.fill(0)

    def state(self):
        """The temporal state, uint32 [DIM_Y, DIM_X] on the host (waits for the device); None without a temporal stage."""
        return None if self._state is None else self._state.get()[:self.DIM_Y * self.DIM_X].reshape(self.DIM_Y, self.DIM_X)

    def run(self, depth, depth_out=None, flags_out=None):
        """depth: uint16 [DIM_Y, DIM_X] or [N, DIM_Y, DIM_X] on the device or the host (a host array is copied to the device
        first), 0 = no reading; the N frames are consecutive in time and follow the frames of the call before.  Returns
        depth_out, device uint16 of the same shape (allocated when None; not the input).  flags_out: device uint8 of the
        same shape, or None.  Runs on the current stream and does not synchronise."""
        d = depth.cu() if hasattr(depth, "cu") else depth
        if not (isinstance(d, DeviceArray) or hasattr(d, "__cuda_array_interface__") or hasattr(d, "data_ptr")):
            d = DeviceArray(np.shape(d), np.uint16).set(np.ascontiguousarray(d, np.uint16))
        shape = tuple(int(s) for s in d.shape)
        assert shape[-2:] == (self.DIM_Y, self.DIM_X) and len(shape) in (2, 3) and np.dtype(d.dtype) == np.uint16, (shape, d.dtype)
        n = shape[0] if len(shape) == 3 else 1
        if depth_out is None:
            depth_out = DeviceArray(shape, np.uint16)
        for o, dtype in ((depth_out, np.uint16), (flags_out, np.uint8)):
            o = o.cu() if hasattr(o, "cu") else o
            assert o is None or (np.dtype(o.dtype) == dtype and int(np.prod(o.shape)) == n * self.DIM_Y * self.DIM_X), (o.shape, o.dtype)
        rc = self._fe.rdf_depth_filter(n, self.DIM_X, self.DIM_Y, device_ptr(d), ctypes.byref(self.config),
                                       None if self._state is None else self._state.ptr, device_ptr(depth_out),
                                       device_ptr(flags_out), self._rt.stream())
        _lib.check(self._fe, rc, "rdf_depth_filter")
        for o in (self._state, depth_out, flags_out):
            o = o.cu() if hasattr(o, "cu") else o
            if hasattr(o, "mark_dirty"):
                o.mark_dirty()
        return depth_out
