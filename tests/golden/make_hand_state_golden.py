#!/usr/bin/env python3
"""Records the reference's own note state machine into tests/golden/hand_state_v1.npz.

Runs in the build container only: it imports /root/reference/src/hand_state.py (FingertipState / HandState) with a stub
`imgui` module in sys.modules (the reference imports it for draw_imgui, which is never called here), drives it exactly as
src/3d_bz.py:496-522 does -- per frame and fingertip: velocity_sensitive / min_velocity / max_velocity set, then
reset_positions() for a NaN height, else next_z_pos(z, z_thresh_offset) -- and stores DATA only: the heights that went in, the
events that came out of on_fn / off_fn, and the final z_thresh, positions and note_on.  No reference source text.

Six sequences of 600 frames x 5 fingertips; each fingertip repeats hover (3-29 frames, N(300, 20)), descent (2-5 linear steps
down to a bottom drawn from U(60, 190)), hold (0-11 frames, for one tap in five up to 149; bottom + N(0, 3)) and, after 15 %
of the taps, a run of 1-3 NaN frames.  The sequences vary velocity_sensitive, z_thresh_offset and min / max velocity.

At record time it asserts that the restatement (tests/hand_state_numpy.py) gives the reference's events exactly, that every
sequence has at least 20 events, and that at least one threshold moved.

    python3 tests/golden/make_hand_state_golden.py        # rewrites tests/golden/hand_state_v1.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
F, T, P = 600, 5, 50
THRESHOLDS, FIRST_NOTE = [200., 160., 160., 160., 160.], 36
# (velocity_sensitive, z_thresh_offset, min_velocity, max_velocity)
SETTINGS = [(True, 0., 15., 120.), (True, 10., 10., 150.), (False, 20., 15., 120.), (True, 30., 10., 150.),
            (False, 0., 10., 150.), (True, 20., 15., 120.)]


def fingertip_trace(rng, n):
    out = []
    while len(out) < n:
        out += rng.normal(300., 20., int(rng.integers(3, 30))).tolist()
        bottom = float(rng.uniform(60., 190.))
        steps = int(rng.integers(2, 6))
        out += np.linspace(out[-1], bottom, steps + 1)[1:].tolist()
        hold = int(rng.integers(0, 150)) if rng.random() < 0.2 else int(rng.integers(0, 12))
        out += (bottom + rng.normal(0., 3., hold)).tolist()
        if rng.random() < 0.15:
            out += [np.nan] * int(rng.integers(1, 4))
    return np.array(out[:n], np.float64)


def reference_run(heights, setting):
    sys.modules.setdefault("imgui", types.ModuleType("imgui"))
    sys.path.insert(0, os.path.join(REF, "src"))
    try:
        import hand_state as ref
    finally:
        sys.path.pop(0)
    sensitive, offset, lo, hi = setting
    events, frame = [], [0]
    hs = ref.HandState([(THRESHOLDS[i], FIRST_NOTE + i) for i in range(T)],
                       lambda n, v: events.append((frame[0], n - FIRST_NOTE, n, v)),
                       lambda n: events.append((frame[0], n - FIRST_NOTE, n, -1)), is_rh=True, num_positions=P)
    for f in range(heights.shape[0]):
        frame[0] = f
        for i in range(T):
            tip = hs.fingertips[i]
            tip.velocity_sensitive, tip.min_velocity, tip.max_velocity = sensitive, lo, hi
            if np.isnan(heights[f, i]):
                tip.reset_positions()
            else:
                tip.next_z_pos(heights[f, i], offset)
    return (events, np.array([t.z_thresh for t in hs.fingertips], np.float64),
            np.array([t.positions for t in hs.fingertips], np.float64), np.array([t.note_on for t in hs.fingertips], np.int32))


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    from hand_state_numpy import HandStateNumpy
    rng = np.random.default_rng(20240)
    heights = np.stack([np.stack([fingertip_trace(rng, F) for _ in range(T)], 1) for _ in SETTINGS])
    ev_all, ev_seq, z_all, pos_all, on_all = [], [], [], [], []
    moved, worst = 0, 0.
    for s, setting in enumerate(SETTINGS):
        events, z, pos, on = reference_run(heights[s], setting)
        mine = HandStateNumpy(THRESHOLDS, [FIRST_NOTE + i for i in range(T)], P)
        mine.velocity_sensitive[:], mine.z_thresh_offset = int(setting[0]), setting[1]
        mine.min_velocity[:], mine.max_velocity[:] = setting[2], setting[3]
        mine.step(heights[s])
        assert mine.events == events, s
        assert np.array_equal(mine.positions, pos) and np.array_equal(mine.note_on, on), s
        assert len(events) >= 20, (s, len(events))
        worst = max(worst, float(np.abs(mine.z_thresh / z - 1).max()))
        moved += int((z != np.array(THRESHOLDS)).sum())
        ev_all += events
        ev_seq += [s] * len(events)
        z_all.append(z), pos_all.append(pos), on_all.append(on)
    assert moved >= 1
    out = os.path.join(HERE, "hand_state_v1.npz")
    np.savez_compressed(out, heights=heights, settings=np.array(SETTINGS, np.float64), thresholds=np.array(THRESHOLDS),
                        first_note=np.int32(FIRST_NOTE), events=np.array(ev_all, np.int32), event_seq=np.array(ev_seq, np.int32),
                        z_thresh=np.stack(z_all), positions=np.stack(pos_all), note_on=np.stack(on_all))
    print(f"{out}: {os.path.getsize(out)} bytes, {len(ev_all)} events, {moved} thresholds moved, "
          f"worst relative z_thresh difference of the restatement {worst:.2e}")


if __name__ == "__main__":
    main()
