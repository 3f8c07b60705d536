"""Fingertip heights -> note events on the device: the reference's `HandState` / `FingertipState`
(src/hand_state.py:4-86 of the reference, driven from its src/3d_bz.py:496-522) behind the same constructor.

The state of every fingertip lives in one block of device memory (include/rdf_frontend.h describes it) and one kernel,
rdf_hand_state_step, advances it from the heights where `HandPipeline` left them -- device memory or mapped pinned host
memory -- so a frame ends in note events without a host read.  Events land in a ring in pinned host memory; `poll()` waits for
the current stream, reads what is new there without a copy and calls `on_fn(note, velocity)` / `off_fn(note)` in order.

One documented difference from the reference: the mean of a note's "on" run adds its elements in arrival order where
np.sum adds pairwise, so a re-calibrated `z_thresh` can differ from the reference's in the last bits; events do not.
There is no `draw_imgui`.  Importing this module needs no GPU: the runtime is created by the first call that needs it.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, device_ptr, get_runtime, host_mapped_array

Z_THRESH, MIN_VELOCITY, MAX_VELOCITY, VELOCITY_SENSITIVE, Z_THRESH_OFFSET = range(5)
MAX_TIPS, MIN_POSITIONS = 64, 11
_HEADER, _DOUBLES, _INTS = 32, ("z_thresh", "min_velocity", "max_velocity", "on_last", "on_mid"), \
    ("midi_note", "note_on", "velocity_sensitive", "on_count", "steps", "pos_next")


def state_bytes(n_tips, num_positions):
    return _HEADER + n_tips * (8 * (len(_DOUBLES) + num_positions) + 4 * len(_INTS))


def parse_state(raw):
    """The fields of a state block (uint8 array, one device-to-host copy) as numpy arrays; `positions` [T, P] comes out
    oldest first, as the reference's list."""
    raw = np.ascontiguousarray(raw, np.uint8)
    T, P = (int(v) for v in raw[:8].view(np.int32))
    assert raw.size >= state_bytes(T, P), (raw.size, T, P)
    out = {"n_tips": T, "num_positions": P, "z_thresh_offset": float(raw[8:16].view(np.float64)[0]),
           "produced": int(raw[16:20].view(np.uint32)[0])}
    d = raw[_HEADER:_HEADER + 8 * T * (len(_DOUBLES) + P)].view(np.float64)
    for i, k in enumerate(_DOUBLES):
        out[k] = d[i * T:(i + 1) * T].copy()
    ring = d[len(_DOUBLES) * T:].reshape(P, T)
    at = _HEADER + 8 * T * (len(_DOUBLES) + P)
    ints = raw[at:at + 4 * T * len(_INTS)].view(np.int32)
    for i, k in enumerate(_INTS):
        out[k] = ints[i * T:(i + 1) * T].copy()
    out["positions"] = np.stack([np.roll(ring[:, t], -int(out["pos_next"][t])) for t in range(T)])
    return out


class FingertipView:
    """One fingertip of a HandState with the reference's attribute names.  Reads copy the state block from the device (and
    wait for the stream); writes are stream-ordered setters."""

    def __init__(self, hand, index):
        self._hand, self.index = hand, int(index)

    def _get(self, name):
        return self._hand.state()[name][self.index]

    num_positions = property(lambda self: self._hand.num_positions)
    midi_note = property(lambda self: int(self._get("midi_note")))
    note_on = property(lambda self: bool(self._get("note_on")))
    positions = property(lambda self: self._get("positions").tolist())
    z_thresh = property(lambda self: float(self._get("z_thresh")),
                        lambda self, v: self._hand.set_field(Z_THRESH, [v], self.index))
    min_velocity = property(lambda self: float(self._get("min_velocity")),
                            lambda self, v: self._hand.set_field(MIN_VELOCITY, [v], self.index))
    max_velocity = property(lambda self: float(self._get("max_velocity")),
                            lambda self, v: self._hand.set_field(MAX_VELOCITY, [v], self.index))
    velocity_sensitive = property(lambda self: bool(self._get("velocity_sensitive")),
                                  lambda self, v: self._hand.set_field(VELOCITY_SENSITIVE, [1. if v else 0.], self.index))

    def next_z_pos(self, z_pos, z_thresh_offset):
        """One frame of this fingertip alone (a one-fingertip launch)."""
        self._hand.step(np.array([z_pos], np.float64), z_thresh_offset, tip_first=self.index)

    def reset_positions(self):
        self._hand.step(np.array([np.nan]), tip_first=self.index)


class HandState:
    def __init__(self, defaults, on_fn, off_fn, is_rh=True, num_positions=50, capacity=4096):
        """defaults = [(z_thresh, midi_note), ...], one per fingertip (at most 64); on_fn(note, velocity) and off_fn(note) are
        called from poll(); num_positions >= 11; capacity = the event ring's length."""
        self.is_rh = is_rh
        self.on_fn, self.off_fn = on_fn, off_fn
        self._defaults = [(float(z), int(m)) for z, m in defaults]
        self.n_tips, self.num_positions, self.capacity = len(self._defaults), int(num_positions), int(capacity)
        if not 1 <= self.n_tips <= MAX_TIPS or self.num_positions < MIN_POSITIONS or self.capacity < 1:
            raise ValueError(f"HandState: 1..{MAX_TIPS} fingertips, num_positions >= {MIN_POSITIONS}, capacity >= 1")
        self.fingertips = [FingertipView(self, i) for i in range(self.n_tips)]
        self.lost = 0            # events overwritten in the ring before a poll() could deliver them
        self._seen = 0           # events delivered or counted as lost so far
        self._offset = 0.0
        self._rt = None

    # -- the device side, made by the first call that needs it --
    def _ensure(self):
        if self._rt is not None:
            return
        rt = get_runtime()
        fe = _lib.load("frontend")
        nbytes = int(fe.rdf_hand_state_bytes(self.n_tips, self.num_positions))
        if nbytes != state_bytes(self.n_tips, self.num_positions):
            raise _lib.RdfError(f"rdf_hand_state_bytes({self.n_tips}, {self.num_positions}) = {nbytes}")
        self._state = DeviceArray((nbytes,), np.uint8)
        # the ring and its count: pinned host memory the kernel writes and poll() reads in place; device memory and a copy
        # where the runtime has no mapped memory
        self._ring_host = None
        if getattr(rt, "alloc_host_mapped", None) is not None:
            self._ring, self._ring_host = host_mapped_array((self.capacity * 4 + 4,), np.int32)
            self._ring_host[:] = 0
        else:
            self._ring = DeviceArray((self.capacity * 4 + 4,), np.int32).fill(0)
        self._scratch = DeviceArray((self.n_tips,), np.float64)
        z = np.array([d[0] for d in self._defaults], np.float64)
        m = np.array([d[1] for d in self._defaults], np.int32)
        rc = fe.rdf_hand_state_init(self._state.ptr, self.n_tips, self.num_positions, z.ctypes.data, m.ctypes.data, rt.stream())
        _lib.check(fe, rc, "rdf_hand_state_init")
        self._fe, self._rt = fe, rt

    @property
    def state_ptr(self):
        self._ensure()
        return self._state.ptr

    @property
    def events_ptr(self):
        self._ensure()
        return self._ring.ptr

    @property
    def head_ptr(self):
        self._ensure()
        return self._ring.ptr + self.capacity * 16

    def state(self):
        """Every field of the state block (one device-to-host copy, which waits for the stream): a dictionary of arrays."""
        self._ensure()
        return parse_state(self._state.get())

    # -- setters --
    def set_field(self, field, values, tip_first=0):
        """Stream-ordered write of one field for fingertips tip_first .. (not while the stream is being captured)."""
        self._ensure()
        v = np.ascontiguousarray(values, np.float64).reshape(-1)
        rc = self._fe.rdf_hand_state_set(self._state.ptr, int(field), int(tip_first), int(v.size), v.ctypes.data,
                                         self._rt.stream())
        _lib.check(self._fe, rc, "rdf_hand_state_set")

    @property
    def z_thresh_offset(self):
        return self._offset

    @z_thresh_offset.setter
    def z_thresh_offset(self, value):
        self.set_field(Z_THRESH_OFFSET, [value])
        self._offset = float(value)

    # -- steps --
    def step_device(self, ptr, tip_first, n, n_frames=1):
        """The raw form: heights float64 [n_frames][n] at `ptr` (device or mapped pinned host memory, read when the kernel
        runs) advance fingertips tip_first .. tip_first + n - 1.  Enqueues on the current stream; capturable."""
        self._ensure()
        rc = self._fe.rdf_hand_state_step(self._state.ptr, int(ptr), int(n_frames), int(tip_first), int(n), self.events_ptr,
                                          self.head_ptr, self.capacity, self._rt.stream())
        _lib.check(self._fe, rc, "rdf_hand_state_step")

    def step(self, heights, z_thresh_offset=None, tip_first=0):
        """heights: float64 [n] or [F, n], a host array (copied to the device first) or a device array; z_thresh_offset is
        set first when it is given and differs from the current one."""
        self._ensure()
        if z_thresh_offset is not None and float(z_thresh_offset) != self._offset:
            self.z_thresh_offset = z_thresh_offset
        if isinstance(heights, DeviceArray) or hasattr(heights, "cu") or hasattr(heights, "data_ptr"):
            dev = heights.cu() if hasattr(heights, "cu") else heights
            assert "float64" in str(dev.dtype), dev.dtype
            shape = tuple(dev.shape)
        else:
            h = np.ascontiguousarray(heights, np.float64)
            shape = h.shape
            if self._scratch.size < h.size:
                self._scratch = DeviceArray((h.size,), np.float64)
            dev = self._scratch[:h.size].set(h.reshape(-1))
        assert len(shape) in (1, 2) and shape[-1] >= 1, shape
        self.step_device(device_ptr(dev), tip_first, shape[-1], shape[0] if len(shape) == 2 else 1)

    # -- events --
    def poll(self):
        """Waits for the current stream, then delivers every event since the last poll: on_fn(note, velocity) / off_fn(note)
        in order, and the list of (step, tip, note, velocity or -1).  When more than `capacity` arrived, the newest
        `capacity` are delivered and the number of the others is added to `.lost`."""
        self._ensure()
        if self._ring_host is not None:
            self._rt.synchronize()
            ring = self._ring_host
        else:
            ring = self._ring.get()
        head = int(ring[self.capacity * 4:].view(np.uint32)[0])
        new = (head - self._seen) & 0xffffffff
        if new > self.capacity:
            self.lost += new - self.capacity
            new = self.capacity
        first = (head - new) & 0xffffffff
        rows = ring[:self.capacity * 4].reshape(self.capacity, 4)
        events = [tuple(int(v) for v in rows[((first + i) & 0xffffffff) % self.capacity]) for i in range(new)]
        self._seen = head
        for _, _, note, velocity in events:
            if velocity >= 0:
                if self.on_fn is not None:
                    self.on_fn(note, velocity)
            elif self.off_fn is not None:
                self.off_fn(note)
        return events
