"""The depth post-filter (librdf_frontend.so: rdf_depth_filter; DepthPostFilter; BeatsSession's post_filter=) against the
restatement in tests/depth_filter_numpy.py.  The CPU tests pin the restatement to answers worked by hand from rules S, T and
F of include/rdf_frontend.h; every GPU comparison is bit for bit over depth, flags and the state after the call, with no
pixel or case left out."""
import ctypes
import importlib
import inspect
import os

import numpy as np
import pytest

import depth_filter_cases as dc
import depth_filter_numpy as dn
from abi_helpers import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rdf_frontend.h")


# ------------------------------------------------------------------ CPU: the restatement ------------------------------------
def test_rule_s_by_hand():
    f = np.full((5, 5), 1001, np.uint16)
    f[2, 2], f[0, 4] = 1000, 5000
    out = dn.spatial(f, 2, 60)
    # the centre sees all 25: 1000 + 23 x 1001 = 24023 over 24 is 1000.96 -> 1001; with the 5000 it would be 29023 / 25 -> 1161
    assert out[2, 2] == (2 * 24023 + 24) // 48 == 1001 and (29023 * 2 + 25) // 50 == 1161
    assert out[0, 4] == 5000                                                    # nothing within 60 of it but itself
    alone = np.zeros((5, 5), np.uint16)
    alone[1, 3] = 777
    assert np.array_equal(dn.spatial(alone, 2, 60), alone)                     # a reading among holes; and holes stay holes
    holes = np.full((5, 5), 900, np.uint16)
    holes[2, 2] = 0
    assert dn.spatial(holes, 2, 60)[2, 2] == 0 and (dn.spatial(holes, 2, 60)[holes != 0] == 900).all()
    corner = np.array([[10, 20, 99], [30, 40, 99], [99, 99, 99]], np.uint16)
    out = dn.spatial(corner, 1, 1000)
    assert out[0, 0] == 25 and out[1, 1] == 66                                  # (10 + 20 + 30 + 40) / 4; 595 / 9 = 66.1
    top = np.full((5, 5), 65535, np.uint16)
    assert (dn.spatial(top, 2, 60) == 65535).all() and (dn.spatial(top, 2, 65535) == 65535).all()
    assert dn.spatial(np.array([[10, 11]], np.uint16), 1, 60).tolist() == [[11, 11]]          # 10.5 rounds up
    assert dn.spatial(np.array([[6, 6, 9]], np.uint16), 1, 3).tolist() == [[6, 7, 8]]         # 6; 21 / 3; 7.5 rounds up
    assert dn.spatial(np.array([[6, 6, 9]], np.uint16), 1, 0).tolist() == [[6, 6, 9]]         # only equal values
    assert dn.spatial(np.array([[6, 6, 9]], np.uint16), 0, 60).tolist() == [[6, 6, 9]]        # r = 0: off


def _walk(seq, alpha=102, delta=100, need=2, span=4, state=0):
    """One pixel through rule T: (outs, flags, states after each frame)."""
    outs, flags, states = [], [], []
    st = np.array([[state]], np.uint32)
    for c in seq:
        o, f, st = dn.temporal(np.array([[c]], np.uint16), st, alpha, delta, need, span)
        outs.append(int(o[0, 0]))
        flags.append(int(f[0, 0]))
        states.append(int(st[0, 0]))
    return outs, flags, states


def test_rule_t_by_hand():
    outs, flags, states = _walk([1000, 1016, 1200, 0, 0, 0, 0, 0, 0, 0, 0, 1210])
    # 1000: v = 16000.  1016: 16000 + ((102 * 256 + 128) >> 8) = 16102 -> 1006.  1200: 3098 sixteenths off, beyond 1600: restart
    assert states[0] == (16000 << 8) | 1 and states[1] == (16102 << 8) | 3 and (102 * 256 + 128) >> 8 == 102
    assert states[2] == (19200 << 8) | 7
    # holes: hist & 15 is 0111, 1110, 1100 (two of four: held), 1000 (one short), then 0; the eighth hole forgets the value
    assert outs == [1000, 1006, 1200, 1200, 1200, 1200, 0, 0, 0, 0, 0, 1210]
    assert flags == [0, dn.FLAG_BLENDED, 0, dn.FLAG_PERSISTED, dn.FLAG_PERSISTED, dn.FLAG_PERSISTED, 0, 0, 0, 0, 0, 0]
    assert states[9] == (19200 << 8) | 128 and states[10] == 0
    # ... so that 1210 starts afresh; one hole fewer and it would have blended with 19200: 19200 + ((102 * 160 + 128) >> 8)
    kept, kept_flags, _ = _walk([1200, 0, 0, 0, 0, 0, 0, 0, 1210])
    assert kept[-1] == (19264 + 8) >> 4 == 1204 and kept_flags[-1] == dn.FLAG_BLENDED
    # the jump that is exactly delta_t blends, one more restarts
    assert _walk([1000, 1100])[1] == [0, dn.FLAG_BLENDED] and _walk([1000, 1101])[1] == [0, 0] and _walk([1000, 1101])[0][1] == 1101
    # sixteenths: a constant 1010 after 1000 is reached (v stops one sixteenth short); whole units would stall at 1009
    outs, _, states = _walk([1000] + [1010] * 40)
    assert outs[-1] == 1010 and states[-1] >> 8 == 16159 and all(b >= a for a, b in zip(outs, outs[1:]))
    # alpha 0 holds the first value; alpha 256 with need 9 is the identity
    assert _walk([1000, 1016, 1030], alpha=0)[0] == [1000, 1000, 1000]
    seq = [5, 0, 700, 65535, 0, 1, 1, 0, 0, 40000]
    assert _walk(seq, alpha=256, need=9)[0] == seq
    # need 0: a hole shows the value until it is forgotten -- also in the eighth hole, whose end forgets it
    outs, _, states = _walk([1000] + [0] * 9, need=0)
    assert outs == [1000] * 9 + [0] and states[8] == 0
    # span 1: only the frame before counts
    assert _walk([1000, 0, 0], need=1, span=1)[0] == [1000, 1000, 0]
    # the largest reading fits: 65535 * 16 in 24 bits
    assert _walk([65535, 65535])[2][1] == ((65535 * 16) << 8) | 3


def test_rule_f_by_hand():
    #             0  1    2  3    4  5  6  7    8  9 10 11 12   13 14     gaps of 2 (at the start), 1, 3, 4 and 1 (at the end)
    t = np.array([[0, 0, 500, 0, 700, 0, 0, 0, 900, 0, 0, 0, 0, 300, 0]], np.uint16)
    left, filled = dn.fill(t, 1, 3)
    assert left.tolist() == [[0, 0, 500, 500, 700, 700, 700, 700, 900, 900, 900, 900, 0, 300, 300]]
    assert filled.tolist() == [[False, False, False, True, False, True, True, True, False, True, True, True, False, False, True]]
    far, filled = dn.fill(t, 2, 3)
    assert far.tolist() == [[500, 500, 500, 700, 700, 900, 900, 900, 900, 900, 900, 900, 300, 300, 300]]
    assert filled.tolist() == (t == 0).tolist()
    # column 12 above is 4 from the 900 and next to a filled 900: a filled pixel is not a source
    assert dn.fill(np.array([[100, 0, 0]], np.uint16), 1, 1)[0].tolist() == [[100, 100, 0]]
    for mode, gap in ((0, 3), (1, 0), (2, 0)):
        out, filled = dn.fill(t, mode, gap)
        assert np.array_equal(out, t) and not filled.any()
    rows = np.array([[0, 0, 0], [7, 0, 9]], np.uint16)                           # row by row: nothing comes from another row
    assert dn.fill(rows, 2, 5)[0].tolist() == [[0, 0, 0], [7, 9, 9]]


def test_the_chain_on_a_sensed_scene():
    """The box of tests/stereo_cases.py sensed with IR seeds 100 .. 107 as eight consecutive frames, through the default chain.
    The figures this prints are the ones DESIGN.md quotes."""
    import stereo_cases as sc
    b = sc.BOX
    raw, truth = dc.box_frames()
    truth = truth.astype(np.int64)
    band = (slice(None), slice(b["y0"], b["y1"]), slice(b["x0"] - 5, b["x0"]))
    raw_valid, band_valid = (raw != 0).mean(), [(f[band[1:]] != 0).mean() for f in raw]
    print(f"raw: {raw_valid:.4f} valid, the shadow band {min(band_valid):.3f} .. {max(band_valid):.3f}")
    assert 0.85 < raw_valid < 0.88 and 0.05 < min(band_valid) and max(band_valid) < 0.15
    seen = (raw[-1] != 0) & (raw[-2] != 0)                   # the pixels the camera reported in both of the last two frames

    def error(frames, ok):
        e = np.abs(frames.astype(np.int64) - truth[None])
        return e[ok & (e <= 300)].mean()
    jitter_raw = np.abs(raw[-1].astype(np.int64) - raw[-2])[seen].mean()
    error_raw = error(raw, raw != 0)
    for mode, name in ((2, "farthest"), (1, "left")):
        out = dn.run(raw, dn.config(fill_mode=mode))
        d, filled = out["depth"], (out["flags"] & dn.FLAG_FILLED) != 0
        in_band = np.zeros_like(filled)
        in_band[band] = True
        near_table = (np.abs(d[filled & in_band].astype(np.int64) - b["Z_table"]) <= 100).mean()
        jitter = np.abs(d[-1].astype(np.int64) - d[-2])[seen].mean()
        err = error(d, (d != 0) & ~filled)
        print(f"{name}: {(d != 0).mean():.4f} valid, the band {(d[band] != 0).mean():.4f}, {near_table:.4f} of its {int((filled & in_band).sum())} "
              f"filled values within 100 of the table; last two frames differ by {jitter:.3f} (raw {jitter_raw:.3f}); "
              f"error of readings {err:.3f} (raw {error_raw:.3f})")
        assert (d[band] != 0).all() and near_table >= 0.99
        assert (d != 0).all() if mode == 2 else (d != 0).mean() >= 0.88
        assert jitter <= 0.5 * jitter_raw
        assert err <= error_raw


def test_a_sequence_does_not_depend_on_how_it_is_cut():
    c = dc.split_case()
    head = dn.run(c["frames"][:3], c["cfg"])
    tail = dn.run(c["frames"][3:], c["cfg"], state=head["state"])
    for k in ("depth", "flags"):
        assert np.array_equal(np.concatenate([head[k], tail[k]]), c["want"][k]), k
    assert np.array_equal(tail["state"], c["want"]["state"]) and not np.array_equal(head["state"], tail["state"])
    one_by_one, state = [], None
    for f in c["frames"]:
        r = dn.run(f[None], c["cfg"], state=state)
        state = r["state"]
        one_by_one.append(r["depth"][0])
    assert np.array_equal(np.stack(one_by_one), c["want"]["depth"]) and np.array_equal(state, c["want"]["state"])


def test_the_gpu_cases_decide_something():
    """The shapes of the GPU comparison reach every flag, every kind of pixel and every branch of the three rules."""
    seen = np.zeros(8, np.int64)
    for name in dc.GPU_SHAPES:
        c = dc.gpu_case(name)
        seen += np.bincount(c["want"]["flags"].reshape(-1), minlength=8)
        assert c["frames"].shape == (dc.GPU_SHAPES[name][2], dc.GPU_SHAPES[name][1], dc.GPU_SHAPES[name][0])
    assert seen[0] > 1000 and seen[dn.FLAG_BLENDED] > 1000 and seen[dn.FLAG_PERSISTED] > 100 and seen[dn.FLAG_FILLED] > 1000
    long_run = dc.gpu_case("20 frames of 13 x 5")
    reading, back = long_run["frames"] != 0, 0
    for t in range(9, len(reading)):            # a reading after eight holes or more that follow a reading: it starts afresh
        again = reading[t] & ~reading[t - 8:t].any(0) & reading[:t - 8].any(0)
        back += int(again.sum())
        assert not (long_run["want"]["flags"][t][again] & dn.FLAG_BLENDED).any()
    assert back >= 5
    assert ((long_run["want"]["flags"] & dn.FLAG_PERSISTED) != 0).any() and ((long_run["want"]["flags"] & dn.FLAG_FILLED) != 0).any()
    wide = dc.gpu_case("1280 wide")["want"]
    assert (wide["depth"] == 0).any() and ((wide["flags"] & dn.FLAG_FILLED) != 0).any()                # a gap wider than max_gap
    sp = dc.gpu_case("no hole, all holes, layered")
    assert (sp["frames"][:2] != 0).all() and (sp["frames"][2] == 0).all()
    assert (sp["want"]["depth"][2] != 0).all() and ((sp["want"]["flags"][2] & dn.FLAG_PERSISTED) != 0).all()
    assert dc.GPU_SHAPES["the widest frame, H 3"][0] == dc.MAX_WIDTH


def test_the_config_variants_do_what_their_names_say():
    base = dc.variant_case()
    assert base["cfg"] == dn.DEFAULTS
    ys, xs = dc.EXTREMES
    assert set(np.unique(base["frames"][0][ys, xs])) == {1, 65535}
    for name, over in dc.CONFIG_VARIANTS.items():
        v = dc.variant_case(name)
        assert all(v["cfg"][k] == over[k] for k in over) and all(v["cfg"][k] == base["cfg"][k] for k in base["cfg"] if k not in over)
        differing = [k for k in ("depth", "flags", "state") if not np.array_equal(v["want"][k], base["want"][k])]
        print(f"{name}: differs from the base in {differing}")
        assert differing or name == "max_gap 65535", name              # (a gap of 67 already reaches across the frame)
    assert np.array_equal(dc.variant_case("max_gap 65535")["want"]["depth"], dc.variant_case("max_gap 67")["want"]["depth"])
    assert np.array_equal(dc.variant_case("T off")["want"]["state"], base["state"]) and (base["state"] != 0).mean() > 0.5
    # delta_s 65535 averages 1s with 65535s: the sums of rule S at their largest
    wide = dc.variant_case("delta_s 65535")["want"]["depth"][0][ys, xs]
    assert ((wide > 1000) & (wide < 64000)).any()


# ------------------------------------------------------------------ CPU: the interface --------------------------------------
def _config(_lib, cfg):
    return _lib.DepthFilterConfig(**cfg)


def test_the_entry_points_reject_bad_and_null_arguments(rdf):
    _lib = importlib.import_module("3d-beats_amd._lib")
    importlib.import_module("3d-beats_amd._build").build()
    names = declared(HEADER)
    assert "rdf_depth_filter" in names and "rdf_depth_filter_state_bytes" in names
    lib = _lib.load("frontend")
    assert lib.rdf_frontend_abi_version() == _lib.BINDINGS["frontend"][0] == 2             # a pure addition
    sb = lib.rdf_depth_filter_state_bytes
    assert sb(848, 480) == 4 * 848 * 480 and sb(1, 1) == 4 and sb(0, 5) == 0 and sb(-1, 5) == 0 and sb(5, -1) == 0
    assert [name for name, _ in _lib.DepthFilterConfig._fields_] == list(dn.DEFAULTS) == list(dn.RANGES)
    assert ctypes.sizeof(_lib.DepthFilterConfig) == 36

    def call(n=1, W=8, H=4, depth=4096, state=8192, out=12288, flags=None, config=True, **kw):
        cfg = ctypes.byref(_config(_lib, dict(dn.DEFAULTS, **kw))) if config else None
        return lib.rdf_depth_filter(n, W, H, depth, cfg, state, out, flags, None)
    # rejected arguments launch nothing, so they can be checked without a device; so can a call without frames
    for field, (lo, hi) in dn.RANGES.items():
        assert call(**{field: lo - 1}) == -1 and call(**{field: hi + 1}) == -1, field
        assert call(n=0, **{field: lo}) == 0 and call(n=0, **{field: hi}) == 0, field
        assert call(n=0, **{field: hi + 1}) == -1, field
    assert call(n=-1) == -1 and call(W=-1) == -1 and call(H=-1) == -1
    assert call(n=0) == 0 and call(W=0) == 0 and call(H=0) == 0                      # no pixels: nothing to do
    assert call(n=0, depth=None, state=None, out=None) == 0
    assert call(W=dc.MAX_WIDTH + 1) == -1 and call(W=1 << 20) == -1
    assert call(n=1 << 10, W=dc.MAX_WIDTH, H=1 << 10) == -3 and call(n=1 << 20, W=dc.MAX_WIDTH, H=1 << 20) == -3       # 2^31, 2^51
    assert call(config=False) == -2 and call(depth=None) == -2 and call(out=None) == -2 and call(state=None) == -2
    assert call(state=None, temporal=0, W=dc.MAX_WIDTH + 1) == -1                   # (without T the state may be NULL)
    assert call(depth=4097) == -1 and call(out=12289) == -1 and call(state=8194) == -1                 # misaligned
    # depth_out overlapping depth: the same buffer, one byte pair of overlap at either end
    assert call(out=4096) == -1 and call(out=4096 + 62) == -1 and call(depth=4096 + 62, out=4096) == -1


def test_the_new_names_are_public(rdf):
    assert "DepthPostFilter" in rdf.__all__ and callable(rdf.DepthPostFilter.run) and callable(rdf.DepthPostFilter.reset)
    p = inspect.signature(rdf.DepthPostFilter.__init__).parameters
    assert [k for k in p][1:] == ["depth_dims", "spatial_radius", "spatial_delta", "temporal_alpha", "temporal_delta", "persistence",
                                  "fill", "max_gap"]
    got = {k: p[k].default for k in list(p)[2:]}
    assert got == {"spatial_radius": 2, "spatial_delta": 60, "temporal_alpha": 0.4, "temporal_delta": 100, "persistence": (2, 4),
                   "fill": "farthest", "max_gap": 32}
    assert [k for k in inspect.signature(rdf.DepthPostFilter.run).parameters][1:] == ["depth", "depth_out", "flags_out"]
    assert inspect.signature(rdf.BeatsSession.__init__).parameters["post_filter"].default is None
    assert "unmeasured" in rdf.DepthPostFilter.__init__.__doc__ or "not been measured" in rdf.DepthPostFilter.__init__.__doc__


class _FakeFilterLib:
    """rdf_depth_filter on host pointers, served by the restatement: with tests/fake_runtime.py's HostRuntime installed,
    "device" memory is numpy memory.  Records (name, n, depth pointer, depth_out pointer)."""

    def __init__(self, log):
        self.log = log

    def rdf_depth_filter_state_bytes(self, W, H):
        return 4 * W * H

    def rdf_depth_filter(self, n, W, H, depth, config, state, out, flags, stream):
        cfg = {name: int(getattr(config._obj, name)) for name, _ in config._obj._fields_}
        if any(not lo <= cfg[k] <= hi for k, (lo, hi) in dn.RANGES.items()):
            return -1
        if n == 0:
            return 0
        self.log.append(("rdf_depth_filter", n, int(depth), int(out)))

        def at(ptr, count, ctype, dtype):
            return np.frombuffer((ctype * count).from_address(int(ptr)), dtype=dtype)
        st = at(state, W * H, ctypes.c_uint32, np.uint32).reshape(H, W) if cfg["temporal"] else None
        r = dn.run(at(depth, n * W * H, ctypes.c_uint16, np.uint16).reshape(n, H, W), cfg, state=st)
        at(out, n * W * H, ctypes.c_uint16, np.uint16)[:] = r["depth"].reshape(-1)
        if st is not None:
            st[:] = r["state"]
        return 0

    def rdf_frontend_error_string(self, code):
        return b"fake frontend error"

    error_string = rdf_frontend_error_string


def _plumbing_session(rdf, host_runtime, monkeypatch, log, H, W, **kw):
    """A BeatsSession whose stages are stand-ins that write down what they are handed (the GPU tests run the real ones)."""
    _lib = importlib.import_module("3d-beats_amd._lib")
    session = importlib.import_module("3d-beats_amd.session")
    monkeypatch.setitem(_lib._loaded, "frontend", _FakeFilterLib(log))

    class FrontEnd:
        def __init__(self, *a, **k):
            self.calibrated_plane = type("P", (), {"plane_cu": None})()

        def run(self, depth, out):
            log.append(("rdf_frame_front", int(depth.shape[0]), depth.ptr))

        def calibrate(self, depth):
            log.append(("calibrate", depth.ptr))
            return np.eye(4, dtype=np.float32)

    class Grouping:
        depth_mm_dims = (H >> 3, W >> 3)

        def __init__(self, *a, **k):
            pass

        def make_group_image(self, clean, groups):
            pass

    class State:
        z_thresh_offset = 0.

        def __init__(self, *a, **k):
            pass

        def set_field(self, *a):
            pass

        def step_device(self, ptr, first, n, n_frames=1):
            log.append(("step", n_frames))

        def poll(self):
            return []

    class Pipe:
        fused_io, heights_ptr = True, 0

        def __init__(self, *a, tip_first=0, **k):
            self.tip_first = tip_first

        def enqueue(self, clean, groups, g_id, flip, height_depth=None):
            log.append(("heights", 1, height_depth.cu().ptr))

        def enqueue_batch(self, clean, groups, g_id, flip, height_depth, row, stride):
            log.append(("heights", int(height_depth.shape[0]), height_depth.ptr))
    for name, cls in (("FrameFrontEnd", FrontEnd), ("HandGrouping", Grouping), ("HandState", State), ("HandPipeline", Pipe)):
        monkeypatch.setattr(session, name, cls)
    monkeypatch.setattr(host_runtime.lib, "rdf_memcpy_device_async", lambda *a: 0, raising=False)
    return rdf.BeatsSession(None, (H, W), (200., W / 2, H / 2), max_frames=3, **kw)


def test_beats_session_filters_every_block_before_the_front_end(rdf, host_runtime, monkeypatch):
    H, W = 8, 16
    frames = dc.layered(W, H, 7, 5)
    log = []
    plain = _plumbing_session(rdf, host_runtime, monkeypatch, log, H, W)
    assert plain.post_filter is None and not hasattr(plain, "_filtered")
    plain.tick(frames[0])
    plain.run_sequence(frames)
    plain.run_sequence(frames, batched=True)
    assert not [e for e in log if e[0] == "rdf_depth_filter"]
    # without a filter the front end and the heights are handed the raw buffer
    assert {e[-1] for e in log if e[0] in ("rdf_frame_front", "heights")} == {plain._raw.ptr + i * H * W * 2 for i in range(3)}

    for batched in (False, True):
        del log[:]
        f = rdf.DepthPostFilter((H, W))
        s = _plumbing_session(rdf, host_runtime, monkeypatch, log, H, W, post_filter=f)
        assert s.post_filter is f
        s.run_sequence(frames, batched=batched)
        blocks = [e for e in log if e[0] in ("rdf_depth_filter", "rdf_frame_front")]
        # blocks of 3, 3 and 1: one filter call each, in front of the front end's, raw buffer in, filtered buffer out and on
        assert [(e[0], e[1]) for e in blocks] == [(name, n) for n in (3, 3, 1) for name in ("rdf_depth_filter", "rdf_frame_front")]
        for filt, front in zip(blocks[::2], blocks[1::2]):
            assert filt[2] == s._raw.ptr and filt[3] == s._filtered.ptr == front[2] != s._raw.ptr
        heights = [e for e in log if e[0] == "heights"]
        if batched:
            assert [e[1:] for e in heights] == [(n, s._filtered.ptr) for n in (3, 3, 1) for hand in range(2)]
        else:
            assert [e[2] for e in heights] == [s._filtered.ptr + (i % 3) * H * W * 2 for i in range(7) for hand in range(2)]
        # the filter's state ran on across the blocks: what is left is what the whole sequence leaves
        want = dn.run(frames, f.config_dict())
        assert np.array_equal(f.state(), want["state"])
        assert np.array_equal(s._filtered.get()[0], want["depth"][6])
        # tick and calibrate: one frame each through the filter, and on
        del log[:]
        s.tick(frames[0])
        s.calibrate(frames[1])
        assert [e[:2] for e in log if e[0] == "rdf_depth_filter"] == [("rdf_depth_filter", 1)] * 2
        assert [e for e in log if e[0] in ("rdf_frame_front", "calibrate")] == [("rdf_frame_front", 1, s._filtered.ptr), ("calibrate", s._filtered.ptr)]
        assert np.array_equal(f.state(), dn.run(frames[:2], f.config_dict(), state=want["state"])["state"])
        f.reset()
        assert (f.state() == 0).all()
    assert f.config_dict() == dn.DEFAULTS
    off = rdf.DepthPostFilter((H, W), temporal_alpha=None, fill=None, spatial_radius=0)
    assert off.config_dict() == dict(dn.DEFAULTS, temporal=0, temporal_alpha=256, fill_mode=0, spatial_radius=0) and off.state() is None
    assert rdf.DepthPostFilter((H, W), fill="left", persistence=(0, 8)).config_dict() == dict(dn.DEFAULTS, fill_mode=1, persist_need=0, persist_span=8)
    with pytest.raises(rdf.RdfError):
        rdf.DepthPostFilter((H, W), spatial_radius=3)
    with pytest.raises(ValueError):
        rdf.DepthPostFilter((H, W), fill="right")
    with pytest.raises(AssertionError):
        _plumbing_session(rdf, host_runtime, monkeypatch, log, H, W, post_filter=rdf.DepthPostFilter((H, W + 1)))


# ------------------------------------------------------------------ GPU -----------------------------------------------------
def _filter_raw(rdf, frames, cfg, state=None, with_state=True, with_flags=True, offset=0):
    """rdf_depth_filter on host arrays: (rc, {"depth", "flags", "state"}); the outputs are pre-filled with 7s.  `offset`
    elements in front of every buffer move it off its 16-byte alignment."""
    _lib = importlib.import_module("3d-beats_amd._lib")
    lib = _lib.load("frontend")
    N, H, W = frames.shape

    def buffer(count, dtype, init=None):
        whole = rdf.DeviceArray((count + offset,), dtype).fill(7)
        part = whole[offset:offset + count]
        if init is not None:
            part.set(np.ascontiguousarray(init, dtype).reshape(-1))
        return part
    d = buffer(N * H * W, np.uint16, frames)
    out = buffer(N * H * W, np.uint16)
    fl = buffer(N * H * W, np.uint8) if with_flags else None
    st = buffer(H * W, np.uint32, np.zeros((H, W), np.uint32) if state is None else state) if with_state else None
    rc = lib.rdf_depth_filter(N, W, H, d.ptr, ctypes.byref(_config(_lib, cfg)), None if st is None else st.ptr, out.ptr,
                              None if fl is None else fl.ptr, rdf.get_runtime().stream())
    got = {"depth": out.get().reshape(N, H, W)}
    if fl is not None:
        got["flags"] = fl.get().reshape(N, H, W)
    if st is not None:
        got["state"] = st.get().reshape(H, W)
    assert np.array_equal(d.get().reshape(N, H, W), frames)             # the input is left alone
    return rc, got


def _same(got, want, what):
    bad = {k: int((got[k] != want[k]).sum()) for k in got}
    print(f"{what}: differing {bad}")
    for k in got:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dc.GPU_SHAPES))
def test_the_device_matches_the_restatement_bit_for_bit(name, rdf, gpu_runtime):
    c = dc.gpu_case(name)
    rc, got = _filter_raw(rdf, c["frames"], c["cfg"])
    assert rc == 0 and sorted(got) == ["depth", "flags", "state"]
    _same(got, c["want"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nine rows", "nine rows, 16 bytes at a time"])
def test_buffers_off_their_alignment_take_the_element_path(name, rdf, gpu_runtime):
    c = dc.gpu_case(name)
    rc, got = _filter_raw(rdf, c["frames"], c["cfg"], offset=1)
    assert rc == 0
    _same(got, c["want"], name + ", one element off")


@pytest.mark.gpu
def test_seven_frames_as_three_and_four(rdf, gpu_runtime):
    c = dc.split_case()
    rc, head = _filter_raw(rdf, c["frames"][:3], c["cfg"])
    assert rc == 0
    _same(head, c["want_head"], "the first three")
    rc, tail = _filter_raw(rdf, c["frames"][3:], c["cfg"], state=head["state"])
    assert rc == 0
    _same({"depth": np.concatenate([head["depth"], tail["depth"]]), "flags": np.concatenate([head["flags"], tail["flags"]]),
           "state": tail["state"]}, c["want"], "three and four")
    rc, whole = _filter_raw(rdf, c["frames"], c["cfg"])
    assert rc == 0
    _same(whole, c["want"], "seven at once")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [None] + list(dc.CONFIG_VARIANTS))
def test_every_config_field_away_from_its_default(name, rdf, gpu_runtime):
    c = dc.variant_case(name)
    with_state = bool(c["cfg"]["temporal"])                  # T off: state NULL
    rc, got = _filter_raw(rdf, c["frames"], c["cfg"], state=c["state"], with_state=with_state)
    assert rc == 0 and ("state" in got) == with_state
    _same(got, c["want"], f"variant {name}")
    if name is None:
        rc, bare = _filter_raw(rdf, c["frames"], c["cfg"], state=c["state"], with_flags=False)
        assert rc == 0 and "flags" not in bare
        _same(bare, c["want"], "flags_out NULL")
    if name == "T off":
        # a state that is handed over all the same is not touched
        sevens = np.full(c["frames"].shape[1:], 0x07070707, np.uint32)
        rc, got = _filter_raw(rdf, c["frames"], c["cfg"], state=sevens)
        assert rc == 0 and np.array_equal(got["state"], sevens) and np.array_equal(got["depth"], c["want"]["depth"])


@pytest.mark.gpu
def test_depth_post_filter_takes_host_and_device_frames_and_resets(rdf, gpu_runtime):
    c = dc.gpu_case("nine rows")
    frames, want = c["frames"], c["want"]
    N, H, W = frames.shape
    f = rdf.DepthPostFilter((H, W))
    assert f.config_dict() == c["cfg"]
    flags = rdf.DeviceArray((N, H, W), np.uint8).fill(7)
    out = f.run(frames, flags_out=flags)                     # host frames
    assert isinstance(out, rdf.DeviceArray) and out.shape == (N, H, W) and out.dtype == np.uint16
    assert np.array_equal(out.get(), want["depth"]) and np.array_equal(flags.get(), want["flags"])
    assert np.array_equal(f.state(), want["state"])
    second = dn.run(frames[0][None], c["cfg"], state=want["state"])
    one = f.run(rdf.to_device(frames[0]))                    # a single device frame, [H, W]: it follows the three before
    assert one.shape == (H, W) and np.array_equal(one.get(), second["depth"][0]) and not np.array_equal(second["depth"][0], want["depth"][0])
    f.reset()
    given = rdf.DeviceArray((N, H, W), np.uint16).fill(7)
    assert f.run(rdf.to_device(frames), depth_out=given) is given             # device frames, from no history again
    assert np.array_equal(given.get(), want["depth"]) and np.array_equal(f.state(), want["state"])
    # no temporal stage: no state, and every frame is filtered on its own
    g = rdf.DepthPostFilter((H, W), temporal_alpha=None)
    assert g.state() is None
    assert np.array_equal(g.run(frames).get(), dn.run(frames, dn.config(temporal=0))["depth"])


@pytest.mark.gpu
def test_a_captured_filter_call_replays(rdf, gpu_runtime):
    """The call makes no synchronous HIP call: it can be recorded into a graph, and each replay is the next frame in time."""
    import torch
    c = dc.gpu_case("nine rows, 16 bytes at a time")
    frames = c["frames"]
    N, H, W = frames.shape
    f = rdf.DepthPostFilter((H, W))
    src, out = rdf.to_device(frames[0]), rdf.DeviceArray((H, W), np.uint16).fill(7)
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            f.run(src, depth_out=out)
    assert (f.state() == 0).all()                            # capturing ran nothing
    for k in range(N):
        src.set(frames[k])
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.get(), c["want"]["depth"][k]), k
    assert np.array_equal(f.state(), c["want"]["state"])
    del graph


@pytest.mark.gpu
def test_beats_session_with_a_post_filter(rdf, gpu_runtime):
    """post_filter=f gives what a session without a filter gives on frames that a second filter of the same config has
    filtered; run_sequence frame by frame, run_sequence in batches and a loop of tick with one poll agree bit for bit, and so do
    max_frames 8 and 5."""
    import session_cases as sc
    import test_session as ts
    H, W = sc.H, sc.W
    frames, intr = sc.frames()
    cfg4 = sc.forest_config(rdf)

    def bits(a):
        return np.ascontiguousarray(a, np.float64).view(np.uint64)

    def session(max_frames, **kw):
        return rdf.BeatsSession(ts._stack(rdf, (H, W), cfg4), (H, W), intr, num_random_guesses=4000, seed=3, max_frames=max_frames,
                                **kw)
    fa = rdf.DepthPostFilter((H, W))
    a = session(8, post_filter=fa)
    plane = a.calibrate(frames[0])                           # frame 0 goes through the filter, and then again as frame 0 below
    ev_a, h_a = a.run_sequence(frames)                       # host frames, blocks of 8 and 4

    pre = rdf.DepthPostFilter((H, W))
    first = pre.run(frames[0]).get()
    filtered = pre.run(frames).get()
    # the camera's frames have single holes (1 % of the pixels), each within max_gap of a reading: the filter closes them all
    assert np.array_equal(pre.state(), fa.state()) and (frames == 0).mean() > 0.005 and (filtered != 0).all()
    b = session(8)
    assert np.array_equal(b.calibrate(first), plane)         # the plane was fitted to the filtered frame
    ev_b, h_b = b.run_sequence(filtered)

    dev = rdf.to_device(frames)

    def after_the_calibration_frame():
        f = rdf.DepthPostFilter((H, W))
        f.run(dev[0])
        return f
    c = session(5, post_filter=after_the_calibration_frame())
    c.set_plane(plane)
    ev_c, h_c = c.run_sequence(dev, batched=True)            # blocks of 5, 5 and 2
    d = session(8, post_filter=after_the_calibration_frame())
    d.set_plane(plane)
    ev_d, h_d = d.run_sequence(dev, batched=True)
    e = session(5, post_filter=after_the_calibration_frame())
    e.set_plane(plane)
    for k in range(len(frames)):
        e.tick(dev[k])
    ev_e = e.poll()
    print(f"filtered session: {len(ev_a)} events {ev_a}; finite heights per frame {np.isfinite(h_a).sum(1).tolist()}; heights differing "
          f"from the pre-filtered run {int((bits(h_a) != bits(h_b)).sum())}, batched 5 {int((bits(h_a) != bits(h_c)).sum())}, "
          f"batched 8 {int((bits(h_a) != bits(h_d)).sum())}")
    assert np.isfinite(h_a).sum() >= 30
    for h in (h_b, h_c, h_d):
        assert np.array_equal(bits(h), bits(h_a))
    assert ev_a == ev_b == ev_c == ev_d == ev_e
    for s in (c, d, e):
        assert np.array_equal(s.post_filter.state(), fa.state())
