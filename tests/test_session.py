"""Depth frames to note events with no host read in between: HandPipeline with a hand_state (run, and captured into a
graph), the height_depth argument, and BeatsSession (tick / poll, run_sequence) against the components called one by one with
a host read per frame and the numpy state machine (tests/hand_state_numpy.py)."""
import importlib
import warnings

import numpy as np
import pytest

import session_cases as sc
import test_pipeline as tp
from hand_state_numpy import HandStateNumpy, same_state

TIPS = [3, 4, 5, 6, 7]
INTR = (421.3, 420.9, 423.1, 238.6)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _stack(rdf, dims, cfg4):
    f0, f1, conditions, colors = cfg4
    cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                      {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
           "conditions": conditions, "label_colors": colors}
    return rdf.LayeredDecisionForest(cfg, dims, 2)


_trace_cache = {}


def _pipeline_trace(rdf, pl, lf, plane, g_id, flip_x):
    """The six frames of one hand (its depth 10 mm further from the camera each frame) and the heights a pipeline WITHOUT a
    hand_state returns for them -- computed once per hand and shared."""
    if g_id not in _trace_cache:
        depth, groups = tp._scene(rdf)
        frames = []
        for k in range(6):
            d = depth.copy()
            d[groups == g_id] += np.uint16(10 * k)
            frames.append(d)
        plain = pl.HandPipeline(lf, (tp.H, tp.W), tp.R, 0.75, 5, np.linspace(20., 60., 7).astype(np.float32), TIPS, INTR, plane)
        dbuf, gbuf = rdf.GpuBuffer((tp.H, tp.W), np.uint16), rdf.GpuBuffer((tp.H, tp.W), np.uint16, groups)
        out = []
        for d in frames:
            dbuf.cu().set(d)
            out.append(plain.run(dbuf, gbuf, g_id, flip_x))
        _trace_cache[g_id] = (frames, groups, [m for m, _ in out], np.array([h for _, h in out]))
    return _trace_cache[g_id]


@pytest.mark.gpu
@pytest.mark.parametrize("fused_io", [True, False])
@pytest.mark.parametrize("g_id,flip_x", [(1, False), (2, True)])
def test_hand_pipeline_advances_the_notes_on_the_device(g_id, flip_x, fused_io, rdf, gpu_runtime):
    pl = importlib.import_module("3d-beats_amd.pipeline")
    hsm = importlib.import_module("3d-beats_amd.hand_state")
    lf = _stack(rdf, (tp.H, tp.W), tp._config(rdf))
    plane = (np.eye(4) + 0.05 * np.random.default_rng(3).standard_normal((4, 4))).astype(np.float32)
    frames, groups, want_means, want_h = _pipeline_trace(rdf, pl, lf, plane, g_id, flip_x)
    # thresholds from the observed trace: each fingertip's median height (0 for one that is never found); min_velocity 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (a fingertip that is NaN in all six frames)
        thr = np.nan_to_num(np.nanmedian(want_h, axis=0))
    first = 5 * (g_id - 1)          # the left hand drives fingertips 5-9 of a ten-fingertip state
    z0 = np.full(10, 1e9)
    z0[first:first + 5] = thr

    def model():
        m = HandStateNumpy(z0, 36 + np.arange(10), 50)
        m.min_velocity[:] = 0.
        return m

    def state():
        hs = rdf.HandState(list(zip(z0.tolist(), range(36, 46))), None, None)
        hs.set_field(hsm.MIN_VELOCITY, [0.] * 10)
        return hs
    want = model()
    want.step(want_h, tip_first=first)
    assert sum(1 for e in want.events if e[3] >= 0) >= 1, "a run without a note-on proves nothing"

    hs = state()
    pipe = pl.HandPipeline(lf, (tp.H, tp.W), tp.R, 0.75, 5, np.linspace(20., 60., 7).astype(np.float32), TIPS, INTR, plane,
                           fused_io=fused_io, hand_state=hs, tip_first=first)
    dbuf, gbuf = rdf.GpuBuffer((tp.H, tp.W), np.uint16), rdf.GpuBuffer((tp.H, tp.W), np.uint16, groups)
    for k, d in enumerate(frames):
        dbuf.cu().set(d)
        means, heights = pipe.run(dbuf, gbuf, g_id, flip_x)
        assert np.array_equal(_bits(means), _bits(want_means[k])) and np.array_equal(_bits(heights), _bits(want_h[k])), k
    got = hs.poll()
    print(f"hand {g_id} fused_io={fused_io}: {len(got)} events from run() (expected {len(want.events)}: {want.events}), "
          f"{int(np.isfinite(want_h).sum())} finite heights of {want_h.size}, steps {hs.state()['steps'].tolist()}")
    assert got == want.events
    assert same_state(hs.state(), want.state())

    # the same six frames through a captured graph: replay(read=False) x 6, then ONE poll
    hs2 = state()
    pipe2 = pl.HandPipeline(lf, (tp.H, tp.W), tp.R, 0.75, 5, np.linspace(20., 60., 7).astype(np.float32), TIPS, INTR, plane,
                            fused_io=fused_io, hand_state=hs2, tip_first=first)
    dbuf.cu().set(frames[0])
    replay = pipe2.capture(dbuf, gbuf, g_id, flip_x)
    assert hs2.state()["steps"].tolist() == [0] * 10          # capturing advanced nothing
    for d in frames:
        dbuf.cu().set(d)
        replay(read=False)
    got2 = hs2.poll()
    print(f"hand {g_id} fused_io={fused_io}: {len(got2)} events from 6 replays, steps {hs2.state()['steps'].tolist()}")
    assert got2 == want.events
    assert same_state(hs2.state(), want.state())
    m_last, h_last = replay.read()
    assert np.array_equal(_bits(h_last), _bits(want_h[-1])) and np.array_equal(_bits(m_last), _bits(want_means[-1]))
    del replay


@pytest.mark.gpu
@pytest.mark.parametrize("fused_io", [True, False])
def test_heights_follow_height_depth_and_a_device_plane(fused_io, rdf, gpu_runtime):
    """The chain reads the processed frame, the fingertip's depth is looked up in `height_depth` (the raw frame in the app):
    same means, other heights.  With plane = I the height is minus the depth at the fingertip's pixel, exactly, so a raw
    frame that is 7 mm further away wherever it has a reading gives heights 7 lower there."""
    pl = importlib.import_module("3d-beats_amd.pipeline")
    lf = _stack(rdf, (tp.H, tp.W), tp._config(rdf))
    depth, groups = tp._scene(rdf)
    raw = np.where(depth > 0, depth + 7, 0).astype(np.uint16)
    plane_cu = rdf.to_device(np.eye(4, dtype=np.float32))
    pipe = pl.HandPipeline(lf, (tp.H, tp.W), tp.R, 0.75, 5, np.linspace(20., 60., 7).astype(np.float32), TIPS, INTR, plane_cu,
                           fused_io=fused_io)
    dbuf, rbuf = rdf.GpuBuffer((tp.H, tp.W), np.uint16, depth), rdf.GpuBuffer((tp.H, tp.W), np.uint16, raw)
    gbuf = rdf.GpuBuffer((tp.H, tp.W), np.uint16, groups)
    m0, h0 = pipe.run(dbuf, gbuf, 1, False)
    m1, h1 = pipe.run(dbuf, gbuf, 1, False, height_depth=rbuf)
    ok = np.isfinite(h0)
    assert ok.sum() >= 3 and np.array_equal(_bits(m0), _bits(m1)) and np.array_equal(np.isfinite(h1), ok)
    d = -h0[ok]                                   # the depth at each fingertip's pixel (0 where the frame has no reading)
    assert (d > 0).sum() >= 1 and np.array_equal(h1[ok], -np.where(d > 0, d + 7., 0.))
    # the plane is read from the device every frame: a new plane reaches the heights without a new pipeline
    plane_cu.set(np.diag([1., 1., 2., 1.]).astype(np.float32))
    m2, h2 = pipe.run(dbuf, gbuf, 1, False)
    assert np.array_equal(_bits(m2), _bits(m0)) and np.array_equal(h2[ok], 2. * h0[ok])


@pytest.mark.gpu
def test_beats_session_equals_the_components_one_by_one(rdf, gpu_runtime):
    """240 x 424 frames, level 3, labels_reduce 2, 12 frames, two moving hands: run_sequence == tick() x 12 + poll() == the
    components called one by one with a host read per frame and the numpy state machine; heights [12, 10] bit for bit, NaN
    positions included, and the events."""
    pl = importlib.import_module("3d-beats_amd.pipeline")
    H, W = sc.H, sc.W
    frames, (focal, ppx, ppy) = sc.frames()
    cfg4 = sc.forest_config(rdf)

    def session(**kw):
        return rdf.BeatsSession(_stack(rdf, (H, W), cfg4), (H, W), (focal, ppx, ppy), num_random_guesses=4000, seed=3,
                                max_frames=5, **kw)
    calls = []
    a = session(on_fn=lambda n, v: calls.append((n, v)), off_fn=lambda n: calls.append((n, -1)))
    plane = a.calibrate(frames[0])
    ev_a, h_a = a.run_sequence(frames)                       # host frames, batches of 5, 5 and 2
    assert h_a.shape == (12, 10) and [(n, v) for _, _, n, v in ev_a] == calls

    b = session()
    b.set_plane(plane)
    dev = rdf.to_device(frames)
    for k in range(12):
        b.tick(dev[k])                                       # device frames: nothing is read or waited for
    ev_b = b.poll()
    assert b.poll() == []

    c = session(fused_io=False)
    c.set_plane(plane)
    ev_c, h_c = c.run_sequence(dev)

    # ---- the components, one by one ----
    fe = rdf.FrameFrontEnd((H, W), (focal, ppx, ppy), sc.PLANE_T, gauss_sigma=2.0)
    fe.set_plane(plane)
    hg = rdf.HandGrouping((H, W), sc.LEVEL, 0.06)
    lf = _stack(rdf, (H, W), cfg4)
    args = ((H, W), 2, W / 848, 6, [50., 8., 8., 8., 8., 8., 8.], [2, 3, 4, 5, 6], (focal, focal, ppx, ppy), plane)
    right, left = pl.HandPipeline(lf, *args, depth_mm_level=sc.LEVEL), pl.HandPipeline(lf, *args, depth_mm_level=sc.LEVEL)
    rawb, clean = rdf.GpuBuffer((H, W), np.uint16), rdf.GpuBuffer((H, W), np.uint16)
    groups = rdf.GpuBuffer((H >> sc.LEVEL, W >> sc.LEVEL), np.uint16)
    want_h = np.zeros((12, 10))
    for k in range(12):
        rawb.cu().set(frames[k])
        fe.run(rawb, clean)
        hg.make_group_image(clean, groups)
        g = groups.cu().get()
        assert (g == 1).any() and (g == 2).any(), k                                   # both groups, every frame
        want_h[k, :5] = right.run(clean, groups, 1, False, height_depth=rawb)[1]
        assert (right.labels_image.cu().get() != 65535).sum() >= 200, k               # labelled pixels per hand
        want_h[k, 5:] = left.run(clean, groups, 2, True, height_depth=rawb)[1]
        assert (left.labels_image.cu().get() != 65535).sum() >= 200, k
    model = HandStateNumpy([200., 160., 160., 160., 160.] * 2, 36 + np.arange(10), 50)
    model.z_thresh_offset, model.min_velocity[:], model.max_velocity[:] = 25., 10., 120.
    model.step(want_h)
    # the scene is worth the comparison: at least 3 fingertips found per hand in at least half the frames, a note-on
    for hand in (want_h[:, :5], want_h[:, 5:]):
        assert (np.isfinite(hand).sum(1) >= 3).sum() >= 6
    assert np.isnan(want_h).any() and sum(1 for e in model.events if e[3] >= 0) >= 1

    print(f"session: expected {len(model.events)} events {model.events}; run_sequence {len(ev_a)}, tick x 12 {len(ev_b)}, "
          f"unfused run_sequence {len(ev_c)}; finite heights per frame {np.isfinite(want_h).sum(1).tolist()}; "
          f"heights differing from the components: {int((_bits(h_a) != _bits(want_h)).sum())}, "
          f"{int((_bits(h_c) != _bits(want_h)).sum())}; first row {np.round(want_h[0], 2).tolist()}")
    for h in (h_a, h_c):
        assert np.array_equal(_bits(h), _bits(want_h))
    assert ev_a == model.events and ev_b == model.events and ev_c == model.events
    for s in (a, b, c):
        assert same_state(s.hand_state.state(), model.state())
