"""Known answers for the note state machine, each worked out by hand from the reference's hand_state.py:4-75 (one fingertip,
at most 16 frames, positions start at 0), and the trace generators the CPU and GPU tests share.

Unless a case says otherwise: z_thresh 250, offset 0, min_velocity 15, max_velocity 150, velocity sensitive, note 60,
num_positions 11.  With heights 300, 232.5, 165 the two last velocities are 67.5 and 67.5: v = 67.5 / 135 = 0.5,
0.4 + 0.5 * 0.6 = 0.7, int(0.7 * 127 = 88.9) = 88, on frame 2 (frame 1 cannot trigger: p[-3] - p[-2] = 0 - 300)."""
import numpy as np

NOTE, P = 60, 11
NAN = float("nan")
TAP = [300., 232.5, 165.]
RECAL = (1.0 - 0.1) * 250. + 0.1 * 165.          # = 241.5: the mean of the middle two of 165, 160, 170, 180 is 165


def _case(name, heights, events, z_thresh=None, note_on=0, start=250., offset=0., lo=15., hi=150., sensitive=True,
          zeroed=False):
    z_thresh = start if z_thresh is None else z_thresh          # (unchanged unless the case re-calibrates)
    return dict(name=name, heights=heights, events=[(f, 0, NOTE, v) for f, v in events], z_thresh=z_thresh, note_on=note_on,
                start=start, offset=offset, lo=lo, hi=hi, sensitive=sensitive, zeroed=zeroed)


CASES = [
    # --- boundaries ---
    # 225 + 25 = 250 exactly: 250 < 250 is false, so the note goes off (run of 1: no re-calibration)
    _case("equal_to_threshold_turns_off", TAP + [250.], [(2, 88), (3, -1)], start=225., offset=25.),
    # velocities 15 and 15, then 15 and 16: not above min_velocity = 15
    _case("velocity_equal_to_minimum_does_not_trigger", [300., 285., 270., 254.], [], start=290.),
    # 15 then 85; and 100 then 10: only one of the last two above the minimum
    _case("first_velocity_too_small", [300., 285., 200.], [], start=290.),
    _case("second_velocity_too_small", [300., 200., 190.], []),
    # --- velocity values ---
    # velocities 200, 200: v = 200 / 135 = 1.48, 0.4 + 0.89 = 1.29, clipped to 1 -> 127
    _case("clipped_velocity", [400., 200., 0.], [(2, 127)], note_on=1),
    _case("not_velocity_sensitive", TAP, [(2, 127)], note_on=1, sensitive=False),
    _case("truncation_0_7_gives_88", TAP, [(2, 88)], note_on=1),
    # velocities 120, 120: v = 120 / 135 = 0.888.., 0.4 + 0.5333.. = 0.9333.., * 127 = 118.53 -> 118
    _case("truncation_118", [300., 180., 60.], [(2, 118)], note_on=1),
    # --- the on-run and the threshold ---
    # on-run 165, 160, 170 (3 frames): too short to re-calibrate
    _case("on_run_of_three_keeps_the_threshold", TAP + [160., 170., 260.], [(2, 88), (5, -1)]),
    # on-run 165, 160, 170, 180: mean of the middle two = 165 > 70: z_thresh = 0.9 * 250 + 0.1 * 165
    _case("on_run_of_four_recalibrates", TAP + [160., 170., 180., 260.], [(2, 88), (6, -1)], z_thresh=RECAL),
    # on-run 60, 65, 75, 70: mean of the middle two = 70, not above 70
    _case("on_z_of_70_keeps_the_threshold", [300., 180., 60., 65., 75., 70., 260.], [(2, 118), (6, -1)]),
    # --- reset ---
    _case("nan_while_on", TAP + [160., 170., 180., NAN], [(2, 88), (6, -1)], z_thresh=RECAL, zeroed=True),
    _case("nan_while_off", [300., 280., NAN], [], zeroed=True),
    # after the reset the positions are 0: 100 has velocities 0 and -100, then 20 has -100 and 80
    _case("first_frames_after_a_reset_cannot_trigger", [300., 232.5, NAN, 100., 20.], []),
]
assert all(len(c["heights"]) <= 16 for c in CASES)


def expected_positions(case):
    """The ring, oldest first: zeros, then the heights since the last NaN."""
    h = case["heights"]
    last_nan = max([i for i, z in enumerate(h) if z != z], default=-1)
    tail = h[last_nan + 1:]
    return np.array([0.] * (P - len(tail)) + tail, np.float64)


# One frame (frame 4) in which fingertips 0, 2, 5, 7 turn on and 3, 6 turn off; 1 and 4 do nothing.
_ON_AT_4, _OFF_AT_4, _IDLE = [300., 300.] + TAP, TAP + [160., 260.], [300.] * 5
TOGETHER = np.array([_ON_AT_4, _IDLE, _ON_AT_4, _OFF_AT_4, _IDLE, _ON_AT_4, _OFF_AT_4, _ON_AT_4], np.float64).T.copy()
TOGETHER_EVENTS = [(2, 3, NOTE + 3, 88), (2, 6, NOTE + 6, 88),
                   (4, 0, NOTE, 88), (4, 2, NOTE + 2, 88), (4, 3, NOTE + 3, -1), (4, 5, NOTE + 5, 88), (4, 6, NOTE + 6, -1),
                   (4, 7, NOTE + 7, 88)]


def traces(seed, n_frames, n_tips):
    """Tap sequences like the golden's: hover, a fast descent, a hold, now and then a few NaN frames.  [n_frames, n_tips]."""
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(n_tips):
        out = []
        while len(out) < n_frames:
            out += rng.normal(300., 20., int(rng.integers(3, 20))).tolist()
            bottom = float(rng.uniform(60., 190.))
            out += np.linspace(out[-1], bottom, int(rng.integers(2, 6)) + 1)[1:].tolist()
            out += (bottom + rng.normal(0., 3., int(rng.integers(0, 12)))).tolist()
            if rng.random() < 0.15:
                out += [NAN] * int(rng.integers(1, 4))
        cols.append(out[:n_frames])
    return np.array(cols, np.float64).T.copy()
