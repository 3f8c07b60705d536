"""The note state machine in plain Python / numpy: the rule of include/rdf_frontend.h (the reference's FingertipState,
src/hand_state.py:4-75, driven as src/3d_bz.py:496-522 drives it) restated field for field.  It is the yardstick for the
kernel (rdf_hand_state_step): same state, same events, bit for bit.

The one difference from the reference is the documented one: `on_mid` adds the on-run's middle elements in arrival order,
where the reference's np.sum adds pairwise from eight elements on."""
import math

import numpy as np

FIELDS = ("z_thresh", "min_velocity", "max_velocity", "on_last", "on_mid", "positions", "midi_note", "note_on",
          "velocity_sensitive", "on_count", "steps")


class HandStateNumpy:
    def __init__(self, z_thresh, midi_notes, num_positions=50):
        assert num_positions >= 11 and 1 <= len(z_thresh) <= 64 and len(z_thresh) == len(midi_notes)
        T = len(z_thresh)
        self.n_tips, self.num_positions = T, int(num_positions)
        self.z_thresh_offset = 0.0
        self.z_thresh = np.array(z_thresh, np.float64)
        self.min_velocity = np.full(T, 15., np.float64)
        self.max_velocity = np.full(T, 150., np.float64)
        self.on_last = np.zeros(T, np.float64)
        self.on_mid = np.zeros(T, np.float64)
        self.positions = np.zeros((T, self.num_positions), np.float64)      # oldest first, as the reference's list
        self.midi_note = np.array(midi_notes, np.int32)
        self.note_on = np.zeros(T, np.int32)
        self.velocity_sensitive = np.ones(T, np.int32)
        self.on_count = np.zeros(T, np.int32)
        self.steps = np.zeros(T, np.int32)
        self.events = []         # (step, tip, note, velocity or -1), every event since the start

    def _clear_run(self, t):
        self.on_count[t], self.on_last[t], self.on_mid[t] = 0, 0., 0.

    def _on(self, t, v):
        if not self.note_on[t]:
            self.note_on[t] = 1
            self.events.append((int(self.steps[t]), t, int(self.midi_note[t]), int(v * 127)))
            self._clear_run(t)

    def _off(self, t):
        if self.note_on[t]:
            self.note_on[t] = 0
            self.events.append((int(self.steps[t]), t, int(self.midi_note[t]), -1))
            if self.on_count[t] >= 4:
                on_z = float(self.on_mid[t]) / (int(self.on_count[t]) - 2.)
                if on_z > 70.:
                    self.z_thresh[t] = (1.0 - 0.1) * float(self.z_thresh[t]) + 0.1 * on_z
            self._clear_run(t)

    def step_tip(self, t, z):
        z = float(z)
        if math.isnan(z):
            self.positions[t] = 0.
            self._off(t)
        else:
            p = self.positions[t]
            p[:-1] = p[1:]
            p[-1] = z
            if z < float(self.z_thresh[t]) + self.z_thresh_offset:
                v1, v2 = float(p[-3]) - float(p[-2]), float(p[-2]) - float(p[-1])
                lo, hi = float(self.min_velocity[t]), float(self.max_velocity[t])
                if v1 > lo and v2 > lo:
                    with np.errstate(all="ignore"):      # (max_velocity == min_velocity: inf, clipped to 1, as in the reference)
                        v = float(np.float64((v1 + v2) / 2) / np.float64(hi - lo))
                    v = 0.4 + v * (1 - 0.4)
                    if v > 1:
                        v = 1.
                    if not self.velocity_sensitive[t]:
                        v = 1.
                    self._on(t, v)
            else:
                self._off(t)
            if self.note_on[t]:
                if self.on_count[t] >= 2:
                    self.on_mid[t] = float(self.on_mid[t]) + float(self.on_last[t])
                self.on_last[t] = z
                self.on_count[t] += 1
        self.steps[t] += 1

    def step(self, heights, tip_first=0):
        """heights [n] or [F, n] for fingertips tip_first .. tip_first + n - 1; frames in order, fingertips in order
        within a frame.  Returns the events of this call."""
        h = np.asarray(heights, np.float64)
        h = h.reshape(1, -1) if h.ndim == 1 else h
        assert tip_first >= 0 and tip_first + h.shape[1] <= self.n_tips
        first = len(self.events)
        for row in h:
            for i, z in enumerate(row):
                self.step_tip(tip_first + i, z)
        return self.events[first:]

    def state(self):
        return {k: np.array(getattr(self, k)) for k in FIELDS} | {"z_thresh_offset": float(self.z_thresh_offset),
                                                                  "produced": len(self.events) & 0xffffffff}


def same_state(got, want):
    """Every field of two state dictionaries (HandStateNumpy.state(), HandState.state()) equal by bytes; names the first
    that is not."""
    for k in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (k, a, b)
    assert np.float64(got["z_thresh_offset"]).tobytes() == np.float64(want["z_thresh_offset"]).tobytes()
    assert int(got["produced"]) == int(want["produced"])
    return True
