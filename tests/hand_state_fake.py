"""Stand-in for the rdf_hand_state_* entry points of librdf_frontend.so -- TEST DOUBLE, lives under tests/ only.

Same names and argument order as include/rdf_frontend.h, served by the restatement (tests/hand_state_numpy.py) on host
pointers: with tests/fake_runtime.py's HostRuntime installed, "device" memory is numpy memory, so the state block, the
heights, the event ring and its count are read and written in place.  It lets the host logic of HandState, and of
HandPipeline's hand_state wiring, run without a GPU."""
import ctypes

import numpy as np

from hand_state_numpy import HandStateNumpy

DOUBLES = ("z_thresh", "min_velocity", "max_velocity", "on_last", "on_mid")
INTS = ("midi_note", "note_on", "velocity_sensitive", "on_count", "steps")


def _at(ptr, n, ctype, dtype):
    return np.frombuffer((ctype * int(n)).from_address(int(ptr)), dtype=dtype)


def encode(model):
    """The state block of include/rdf_frontend.h for a HandStateNumpy (pos_next = 0: slot 0 holds the oldest height)."""
    T, P = model.n_tips, model.num_positions
    head = np.zeros(32, np.uint8)
    head[:8] = np.array([T, P], np.int32).view(np.uint8)
    head[8:16] = np.array([model.z_thresh_offset], np.float64).view(np.uint8)
    head[16:20] = np.array([len(model.events) & 0xffffffff], np.uint32).view(np.uint8)
    doubles = np.concatenate([np.asarray(getattr(model, k), np.float64) for k in DOUBLES] + [model.positions.T.reshape(-1)])
    ints = np.concatenate([np.asarray(getattr(model, k), np.int32) for k in INTS] + [np.zeros(T, np.int32)])
    return np.concatenate([head, doubles.view(np.uint8), ints.view(np.uint8)])


class FakeFrontendLib:
    def __init__(self):
        self.models = {}         # state pointer -> HandStateNumpy
        self.calls = []

    def _store(self, state):
        raw = encode(self.models[int(state)])
        _at(state, raw.size, ctypes.c_uint8, np.uint8)[:] = raw

    def rdf_hand_state_bytes(self, n_tips, num_positions):
        if not (1 <= n_tips <= 64 and 11 <= num_positions <= 4096):
            return 0
        return 32 + n_tips * (8 * (5 + num_positions) + 4 * 6)

    def rdf_hand_state_init(self, state, n_tips, num_positions, z_thresh, midi_notes, stream):
        self.calls.append(("rdf_hand_state_init", n_tips, num_positions))
        z = _at(z_thresh, n_tips, ctypes.c_double, np.float64).copy()
        m = _at(midi_notes, n_tips, ctypes.c_int32, np.int32).copy()
        self.models[int(state)] = HandStateNumpy(z, m, num_positions)
        self._store(state)
        return 0

    def rdf_hand_state_set(self, state, field, tip_first, n, values, stream):
        v = _at(values, n, ctypes.c_double, np.float64).copy()
        self.calls.append(("rdf_hand_state_set", field, tip_first, n, v.tolist()))
        model = self.models[int(state)]
        if field == 4:
            if tip_first != 0 or n != 1:
                return -1
            model.z_thresh_offset = float(v[0])
        elif tip_first < 0 or n < 1 or tip_first + n > model.n_tips or not 0 <= field <= 3:
            return -1
        elif field == 3:
            model.velocity_sensitive[tip_first:tip_first + n] = v != 0
        else:
            getattr(model, DOUBLES[field])[tip_first:tip_first + n] = v
        self._store(state)
        return 0

    def rdf_hand_state_step(self, state, heights, n_frames, tip_first, n, events, head, capacity, stream):
        self.calls.append(("rdf_hand_state_step", int(heights), n_frames, tip_first, n))
        model = self.models[int(state)]
        if n_frames < 1 or n < 1 or tip_first < 0 or tip_first + n > model.n_tips or capacity < 1:
            return -1
        h = _at(heights, n_frames * n, ctypes.c_double, np.float64).reshape(n_frames, n)
        seq = len(model.events)
        ring = _at(events, capacity * 4, ctypes.c_int32, np.int32).reshape(capacity, 4)
        for e in model.step(h, tip_first):
            ring[seq % capacity] = e
            seq += 1
        _at(head, 1, ctypes.c_uint32, np.uint32)[0] = seq & 0xffffffff
        self._store(state)
        return 0

    def rdf_frontend_error_string(self, code):
        return b"fake frontend error"

    error_string = rdf_frontend_error_string
