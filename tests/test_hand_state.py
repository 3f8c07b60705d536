"""The note state machine (include/rdf_frontend.h: rdf_hand_state_*; 3d-beats_amd/hand_state.py).

CPU: the restatement (tests/hand_state_numpy.py) against a recording of the reference's own hand_state.py and against
hand-derived known answers; the host logic of HandState and of HandPipeline's hand_state wiring against a fake of the entry
points.  GPU: the kernel equals the restatement bit for bit -- state block and events -- in every stepping form."""
import importlib
import os
import sys

import numpy as np
import pytest

import hand_state_cases as hc
from hand_state_numpy import HandStateNumpy, same_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand_state_v1.npz")


def _golden():
    return np.load(GOLDEN, allow_pickle=False)


def _golden_model(z, s):
    sensitive, offset, lo, hi = z["settings"][s]
    m = HandStateNumpy(z["thresholds"], int(z["first_note"]) + np.arange(5), 50)
    m.velocity_sensitive[:], m.z_thresh_offset = int(sensitive), float(offset)
    m.min_velocity[:], m.max_velocity[:] = lo, hi
    return m


def _case_model(c):
    m = HandStateNumpy([c["start"]], [hc.NOTE], hc.P)
    m.z_thresh_offset, m.min_velocity[:], m.max_velocity[:] = c["offset"], c["lo"], c["hi"]
    m.velocity_sensitive[:] = int(c["sensitive"])
    return m


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_restatement_gives_the_references_recording():
    """Events, positions and note_on equal; z_thresh within a relative 1e-12.  The bound is derived: the only difference is
    the order of a sum of at most 150 doubles, about 150 x 1.1e-16 per re-calibration, and the 0.9 smoothing caps what
    accumulates at ten times that, 1.7e-13."""
    assert os.path.getsize(GOLDEN) < 400_000
    z = _golden()
    assert z["heights"].shape == (6, 600, 5) and np.isnan(z["heights"]).any()
    moved = 0
    for s in range(6):
        m = _golden_model(z, s)
        m.step(z["heights"][s])
        want = [tuple(int(v) for v in e) for e in z["events"][z["event_seq"] == s]]
        assert len(want) >= 20 and m.events == want, s
        assert np.array_equal(m.positions, z["positions"][s]) and np.array_equal(m.note_on, z["note_on"][s])
        assert np.abs(m.z_thresh / z["z_thresh"][s] - 1).max() <= 1e-12
        moved += int((z["z_thresh"][s] != z["thresholds"]).sum())
    assert moved >= 1


@pytest.mark.parametrize("case", hc.CASES, ids=[c["name"] for c in hc.CASES])
def test_restatement_gives_the_hand_derived_answers(case):
    m = _case_model(case)
    m.step(np.array(case["heights"]).reshape(-1, 1))
    assert m.events == case["events"]
    assert float(m.z_thresh[0]) == case["z_thresh"] and int(m.note_on[0]) == case["note_on"]
    assert np.array_equal(m.positions[0], hc.expected_positions(case))
    if case["zeroed"]:
        assert not m.positions.any()
    assert int(m.steps[0]) == len(case["heights"])


def test_restatement_orders_a_frames_events_by_fingertip():
    m = HandStateNumpy([250.] * 8, hc.NOTE + np.arange(8), hc.P)
    m.step(hc.TOGETHER)
    assert m.events == hc.TOGETHER_EVENTS
    assert abs(hc.RECAL - 241.5) < 1e-12


@pytest.fixture()
def fake_frontend(rdf, host_runtime, monkeypatch):
    import hand_state_fake
    _lib = importlib.import_module("3d-beats_amd._lib")
    fake = hand_state_fake.FakeFrontendLib()
    monkeypatch.setitem(_lib._loaded, "frontend", fake)
    return fake


def test_importing_and_constructing_hand_state_needs_no_gpu(rdf):
    prev = rdf.set_runtime(None)
    try:
        calls = []
        hs = rdf.HandState([(200., 36), (160., 37)], lambda n, v: calls.append((n, v)), lambda n: calls.append(n), is_rh=False)
        assert hs.n_tips == 2 and hs.num_positions == 50 and hs.capacity == 4096 and not hs.is_rh and len(hs.fingertips) == 2
        assert not hasattr(hs, "draw_imgui") and "HandState" in rdf.__all__ and "BeatsSession" in rdf.__all__
    finally:
        rdf.set_runtime(prev)
    with pytest.raises(ValueError):
        rdf.HandState([(200., 36)], None, None, num_positions=10)


def test_hand_state_delivers_events_in_order_and_once(rdf, fake_frontend):
    calls = []
    hs = rdf.HandState([(250., hc.NOTE + i) for i in range(8)], lambda n, v: calls.append(("on", n, v)),
                       lambda n: calls.append(("off", n)), num_positions=hc.P)
    hs.step(hc.TOGETHER[:3])                      # host [F, n]
    assert hs.poll() == hc.TOGETHER_EVENTS[:2]
    for row in hc.TOGETHER[3:]:
        hs.step(row)                              # host [n]
    got = hs.poll()
    assert got == hc.TOGETHER_EVENTS[2:]
    assert calls == [("on", n, v) if v >= 0 else ("off", n) for _, _, n, v in hc.TOGETHER_EVENTS]
    assert hs.poll() == [] and len(calls) == len(hc.TOGETHER_EVENTS) and hs.lost == 0
    want = HandStateNumpy([250.] * 8, hc.NOTE + np.arange(8), hc.P)
    want.step(hc.TOGETHER)
    assert same_state(hs.state(), want.state())
    assert [f.note_on for f in hs.fingertips] == [True, False, True, False, False, True, False, True]
    assert hs.fingertips[0].positions[-2:] == [232.5, 165.] and hs.fingertips[3].midi_note == hc.NOTE + 3


def test_ring_overflow_delivers_the_newest_and_counts_the_lost(rdf, fake_frontend):
    """Capacity 4, six events in one frame: the newest four, lost == 2."""
    hs = rdf.HandState([(250., 36 + i) for i in range(6)], None, None, num_positions=hc.P, capacity=4)
    hs.step(np.repeat(np.array(hc.TAP).reshape(3, 1), 6, axis=1))
    assert hs.poll() == [(2, t, 36 + t, 88) for t in (2, 3, 4, 5)]
    assert hs.lost == 2 and hs.poll() == [] and hs.lost == 2


def test_setters_and_single_fingertip_conveniences(rdf, fake_frontend):
    hs = rdf.HandState([(250., 36), (250., 37)], None, None, num_positions=hc.P)
    tip = hs.fingertips[1]
    tip.z_thresh, tip.min_velocity, tip.max_velocity, tip.velocity_sensitive = 290., 20., 120., False
    hs.z_thresh_offset = 25.
    s = hs.state()
    assert s["z_thresh"].tolist() == [250., 290.] and s["min_velocity"].tolist() == [15., 20.]
    assert s["max_velocity"].tolist() == [150., 120.] and s["velocity_sensitive"].tolist() == [1, 0]
    assert s["z_thresh_offset"] == 25. and hs.z_thresh_offset == 25.
    assert (tip.z_thresh, tip.min_velocity, tip.max_velocity, tip.velocity_sensitive) == (290., 20., 120., False)
    n_sets = sum(c[0] == "rdf_hand_state_set" for c in fake_frontend.calls)
    for z in hc.TAP:
        tip.next_z_pos(z, 25.)                    # (the same offset: no setter call)
    assert sum(c[0] == "rdf_hand_state_set" for c in fake_frontend.calls) == n_sets
    assert hs.poll() == [(2, 1, 37, 127)] and tip.note_on and not hs.fingertips[0].note_on
    assert hs.state()["steps"].tolist() == [0, 3]
    tip.reset_positions()
    assert hs.poll() == [(3, 1, 37, -1)] and not tip.note_on and not any(tip.positions)
    tip.next_z_pos(300., 30.)
    assert hs.state()["z_thresh_offset"] == 30.


def test_hand_pipeline_steps_its_own_fingertips(rdf, fake_frontend, monkeypatch):
    """HandPipeline(hand_state=, tip_first=5) ends a frame with a step of fingertips 5-9 reading the heights where the
    chain wrote them; without a hand_state nothing is stepped.  The chain itself is a stand-in here (the GPU tests run the
    real one): it writes scripted heights into the pipeline's result buffer."""
    pl = importlib.import_module("3d-beats_amd.pipeline")

    class Nothing:
        def __init__(self, *a, **k):
            pass

    class Stack:
        num_layered_classes = 7
    monkeypatch.setattr(pl, "PointsOps", Nothing)
    monkeypatch.setattr(pl, "MeanShift", Nothing)
    script = []

    def chain(self, depth_image, groups, g_id, flip_x, height_depth):
        out = np.full(self._L * 2 + 5, -1.)
        out[self._L * 2:] = script.pop(0)
        self._result.set(out)
    monkeypatch.setattr(pl.HandPipeline, "_chain", chain)
    hs = rdf.HandState([(250., 36 + i) for i in range(10)], None, None, num_positions=hc.P)
    args = ((480, 848), 2, 1.0, 6, np.full(7, 8., np.float32), [2, 3, 4, 5, 6], (420., 420., 424., 240.), np.eye(4))
    left = pl.HandPipeline(Stack(), *args, fused_io=False, hand_state=hs, tip_first=5)
    plain = pl.HandPipeline(Stack(), *args, fused_io=False)
    with pytest.raises(AssertionError):
        pl.HandPipeline(Stack(), *args, fused_io=False, hand_state=hs, tip_first=6)
    for z in hc.TAP:
        script.append([z, 300., 300., 300., z])
        means, heights = left.run(None, None, 2, True)
        assert heights.tolist() == [z, 300., 300., 300., z]
    script.append([0.] * 5)
    plain.run(None, None, 1, False)
    steps = [c for c in fake_frontend.calls if c[0] == "rdf_hand_state_step"]
    assert steps == [("rdf_hand_state_step", left.heights_ptr, 1, 5, 5)] * 3
    assert hs.poll() == [(2, 5, 41, 88), (2, 9, 45, 88)]
    assert hs.state()["steps"].tolist() == [0] * 5 + [3] * 5


def test_reference_import_line_resolves_to_this_package(rdf):
    names = rdf._REFERENCE_MODULE_NAMES
    assert "hand_state" in names
    before = {n: sys.modules.get(n) for n in names}
    try:
        rdf.install_reference_aliases(force=True)
        ns = {}
        exec("from hand_state import HandState", ns)
        assert ns["HandState"] is rdf.HandState
    finally:
        for n, m in before.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def test_state_block_size_is_the_headers(rdf):
    hsm = importlib.import_module("3d-beats_amd.hand_state")
    importlib.import_module("3d-beats_amd._build").build()
    lib = importlib.import_module("3d-beats_amd._lib").load("frontend")
    for T, P in ((1, 11), (5, 50), (10, 50), (64, 4096)):
        assert lib.rdf_hand_state_bytes(T, P) == hsm.state_bytes(T, P) == 32 + T * (8 * (5 + P) + 24)
    assert lib.rdf_hand_state_bytes(65, 50) == 0 and lib.rdf_hand_state_bytes(5, 10) == 0 and lib.rdf_hand_state_bytes(0, 50) == 0
    assert lib.rdf_hand_state_step(None, None, 1, 0, 1, None, None, 4, None) == -2
    assert lib.rdf_hand_state_step(None, None, 0, 0, 1, None, None, 4, None) == -1
    assert lib.rdf_hand_state_step(None, None, 1, 60, 5, None, None, 4, None) == -1
    assert lib.rdf_hand_state_set(None, 4, 1, 1, None, None) == -1 and lib.rdf_hand_state_set(None, 5, 0, 1, None, None) == -1
    assert b"captured" in lib.rdf_frontend_error_string(-6)


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _device_state(rdf, model, capacity=4096):
    """A HandState on the device with the model's settings."""
    hsm = importlib.import_module("3d-beats_amd.hand_state")
    hs = rdf.HandState(list(zip(model.z_thresh.tolist(), model.midi_note.tolist())), None, None,
                       num_positions=model.num_positions, capacity=capacity)
    hs.set_field(hsm.MIN_VELOCITY, model.min_velocity)
    hs.set_field(hsm.MAX_VELOCITY, model.max_velocity)
    hs.set_field(hsm.VELOCITY_SENSITIVE, model.velocity_sensitive.astype(np.float64))
    hs.z_thresh_offset = model.z_thresh_offset
    return hs


@pytest.mark.gpu
def test_kernel_equals_the_restatement_bit_for_bit(rdf, gpu_runtime):
    """The golden's inputs, the known answers, a full wave of 64 fingertips over 200 frames, one fingertip alone, and the
    frame in which four fingertips turn on and two turn off together."""
    z = _golden()
    runs = [(_golden_model(z, s), z["heights"][s]) for s in range(6)]
    runs += [(_case_model(c), np.array(c["heights"]).reshape(-1, 1)) for c in hc.CASES]
    full = HandStateNumpy(np.linspace(150., 220., 64), 20 + np.arange(64), 50)
    full.z_thresh_offset = 12.5
    full.min_velocity[::2], full.max_velocity[::3], full.velocity_sensitive[::5] = 10., 120., 0
    runs.append((full, hc.traces(77, 200, 64)))
    runs.append((HandStateNumpy([180.], [99], 11), hc.traces(78, 200, 1)))
    runs.append((HandStateNumpy([250.] * 8, hc.NOTE + np.arange(8), hc.P), hc.TOGETHER))
    total = 0
    for model, heights in runs:
        hs = _device_state(rdf, model)
        hs.step(heights)
        got = hs.poll()
        model.step(heights)
        assert got == model.events
        assert same_state(hs.state(), model.state())
        total += len(got)
    print(f"kernel against restatement: {len(runs)} runs, {total} events compared")
    assert runs[-1][0].events == hc.TOGETHER_EVENTS and total > 1000


@pytest.mark.gpu
def test_stepping_forms_leave_the_same_bytes(rdf, gpu_runtime):
    heights = hc.traces(5, 120, 10)
    model = HandStateNumpy([200., 160., 160., 160., 160.] * 2, 36 + np.arange(10), 50)
    model.z_thresh_offset = 25.
    one, many, pinned = (_device_state(rdf, model) for _ in range(3))
    one.step(heights)                                              # F frames in one launch
    for row in heights:
        many.step(rdf.to_device(row))                              # F launches, heights in device memory
    mapped, host = rdf.host_mapped_array(heights.shape, np.float64)  # ... and in mapped pinned host memory
    host[:] = heights
    pinned.step(mapped)
    events = one.poll()
    assert len(events) >= 20 and many.poll() == events and pinned.poll() == events
    raw = one._state.get()
    assert raw.tobytes() == many._state.get().tobytes() == pinned._state.get().tobytes()
    assert one._ring_host.tobytes() == many._ring_host.tobytes() == pinned._ring_host.tobytes()
    model.step(heights)
    assert events == model.events and same_state(one.state(), model.state())

    # fingertips 5-9 alone: 0-4 keep every byte
    left = _device_state(rdf, HandStateNumpy([200., 160., 160., 160., 160.] * 2, 36 + np.arange(10), 50))
    before = left.state()
    left.step(heights[:, 5:], tip_first=5)
    after, ev = left.state(), left.poll()
    want = HandStateNumpy([200., 160., 160., 160., 160.] * 2, 36 + np.arange(10), 50)
    want.step(heights[:, 5:], tip_first=5)
    assert ev == want.events and len(ev) >= 5 and all(e[1] >= 5 for e in ev) and same_state(after, want.state())
    for k in ("z_thresh", "positions", "steps", "note_on", "on_count", "on_mid", "on_last", "pos_next"):
        assert np.array_equal(after[k][:5], before[k][:5]), k
    assert after["steps"].tolist() == [0] * 5 + [120] * 5


@pytest.mark.gpu
def test_event_ring_wraps_and_overflows_in_pinned_memory(rdf, gpu_runtime):
    heights = hc.traces(9, 90, 6)
    model = HandStateNumpy([170.] * 6, 50 + np.arange(6), 50)
    model.z_thresh_offset = 20.
    model.step(heights)
    per_third = [sum(1 for e in model.events if a <= e[0] < a + 30) for a in (0, 30, 60)]
    capacity = max(per_third)          # every third fits, the three together do not: the ring wraps
    assert len(model.events) > capacity >= 4
    fresh = HandStateNumpy([170.] * 6, 50 + np.arange(6), 50)
    fresh.z_thresh_offset = 20.
    hs = _device_state(rdf, fresh, capacity=capacity)
    assert hs._ring_host is not None
    got = []
    for a in (0, 30, 60):
        hs.step(heights[a:a + 30])
        got += hs.poll()
    assert got == model.events and hs.lost == 0 and hs.poll() == []

    # capacity 4, six events in one frame: the newest four, lost == 2
    small = _device_state(rdf, HandStateNumpy([250.] * 6, 36 + np.arange(6), hc.P), capacity=4)
    small.step(np.repeat(np.array(hc.TAP).reshape(3, 1), 6, axis=1))
    assert small.poll() == [(2, t, 36 + t, 88) for t in (2, 3, 4, 5)] and small.lost == 2
    assert small.state()["produced"] == 6


@pytest.mark.gpu
def test_setter_is_refused_during_a_capture(rdf, gpu_runtime):
    import torch
    hs = _device_state(rdf, HandStateNumpy([250.], [36], hc.P))
    dev = rdf.to_device(np.array(hc.TAP[:1]))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hs.step(dev)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(rdf.RdfError, match="captured"):
            hs.z_thresh_offset = 5.
        hs.step(dev)
    assert hs.z_thresh_offset == 0.
    graph.replay()
    torch.cuda.synchronize()
    assert hs.state()["steps"].tolist() == [2] and hs.state()["z_thresh_offset"] == 0.
    del graph
