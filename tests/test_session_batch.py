"""BeatsSession.run_sequence(frames, batched=True): the per-hand chains take a whole block of frames (three calls a hand and
block, one note step a block) and must leave what the frame-by-frame path leaves -- heights, events and the state block, bit
for bit."""
import numpy as np
import pytest

import session_cases as sc
import test_session as ts
from hand_state_numpy import HandStateNumpy, same_state


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _buffers(s):
    """The addresses of everything the batched path allocates on first use."""
    out = []
    for pipe in (s.right, s.left):
        out += [pipe._depth_batch.ptr, pipe._labels_batch.ptr, pipe._means_batch.ptr, pipe.layered_rdf._batch_ptrs_cu.ptr]
        out += [b.ptr for b in pipe.layered_rdf.batch_label_images]
    return out


@pytest.mark.gpu
def test_batched_run_sequence_equals_the_frame_by_frame_one(rdf, gpu_runtime):
    """The scene of test_beats_session_equals_the_components_one_by_one: 12 frames of 240 x 424, max_frames 5, so blocks of
    5, 5 and 2; then the same 12 frames again on the same sessions (steps 12 to 24)."""
    H, W = sc.H, sc.W
    frames, intr = sc.frames()
    cfg4 = sc.forest_config(rdf)

    def session(**kw):
        return rdf.BeatsSession(ts._stack(rdf, (H, W), cfg4), (H, W), intr, num_random_guesses=4000, seed=3, max_frames=5, **kw)
    calls = []
    a = session()
    plane = a.calibrate(frames[0])
    b = session(on_fn=lambda n, v: calls.append((n, v)), off_fn=lambda n: calls.append((n, -1)))
    b.set_plane(plane)
    dev = rdf.to_device(frames)
    ev_a, h_a = a.run_sequence(dev)
    ev_b, h_b = b.run_sequence(dev, batched=True)
    assert h_b.shape == (12, 10) and [(n, v) for _, _, n, v in ev_b] == calls

    model = HandStateNumpy([200., 160., 160., 160., 160.] * 2, 36 + np.arange(10), 50)
    model.z_thresh_offset, model.min_velocity[:], model.max_velocity[:] = 25., 10., 120.
    model.step(h_a)
    print(f"batched session: {len(ev_b)} events (frame by frame {len(ev_a)}, model {len(model.events)}): {ev_b}; finite heights "
          f"per frame {np.isfinite(h_b).sum(1).tolist()}; heights differing {int((_bits(h_a) != _bits(h_b)).sum())}; "
          f"steps {b.hand_state.state()['steps'].tolist()}")
    # the scene is worth the comparison: fingertips found, fingertips lost, a note-on
    for hand in (h_a[:, :5], h_a[:, 5:]):
        assert (np.isfinite(hand).sum(1) >= 3).sum() >= 6
    assert np.isnan(h_a).any() and sum(1 for e in model.events if e[3] >= 0) >= 1
    assert np.array_equal(_bits(h_b), _bits(h_a))
    assert ev_b == ev_a == model.events
    assert same_state(b.hand_state.state(), a.hand_state.state()) and same_state(b.hand_state.state(), model.state())
    # the modes of the last block (frames 10 and 11) are where enqueue_batch says: those of the frame-by-frame chain's last frame
    assert b.right.means_batch.shape == (2, b.right._L, 2)
    for pa, pb in ((a.right, b.right), (a.left, b.left)):
        assert np.array_equal(_bits(pb.means_batch.get()[1]), _bits(pa._read()[0]))

    # ---- a second sequence on the same sessions: the notes go on from where they were, and nothing new is allocated ----
    before = _buffers(b)
    again = rdf.to_device(np.ascontiguousarray(frames[::-1]))          # the hands rise again
    ev_a2, h_a2 = a.run_sequence(again)
    ev_b2, h_b2 = b.run_sequence(again, batched=True)
    model.step(h_a2)
    assert _buffers(b) == before
    assert np.array_equal(_bits(h_b2), _bits(h_a2)) and np.array_equal(_bits(h_a2), _bits(h_a[::-1]))
    assert ev_b2 == ev_a2 == model.events[len(ev_a):] and len(ev_b2) >= 1
    assert all(12 <= e[0] < 24 for e in ev_b2)
    assert same_state(b.hand_state.state(), a.hand_state.state()) and same_state(b.hand_state.state(), model.state())
    assert b.hand_state.state()["steps"].tolist() == [24] * 10


@pytest.mark.gpu
def test_batched_needs_fused_io(rdf, gpu_runtime):
    frames, intr = sc.frames()
    s = rdf.BeatsSession(ts._stack(rdf, (sc.H, sc.W), sc.forest_config(rdf)), (sc.H, sc.W), intr, num_random_guesses=4000,
                         seed=3, max_frames=5, fused_io=False)
    with pytest.raises(ValueError):
        s.run_sequence(frames[:2], batched=True)
    with pytest.raises(ValueError):
        s.right.enqueue_batch(None, None, 1, False, None, 0, 10)
    assert s.hand_state.state()["steps"].tolist() == [0] * 10        # nothing ran
