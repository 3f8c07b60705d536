"""The three batch entry points behind BeatsSession.run_sequence(batched=True) -- rdf_prepare_hand_depth_batch,
rdf_layered_run_hand_batch, rdf_mean_shift_heights_batch -- against their single-frame neighbours called frame by frame.
Every comparison is bit for bit: integers as they are, float64 viewed as uint64 so that NaNs compare."""
import importlib

import numpy as np
import pytest

import session_cases as sc
import test_session as ts

INTR = (421.3, 420.9, 423.1, 238.6)
FAKE = 4096         # a non-NULL address for calls that must return before they touch memory or the device


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def _lib():
    importlib.import_module("3d-beats_amd._build").build()
    return importlib.import_module("3d-beats_amd._lib").load()


def test_the_batch_entry_points_are_bound(rdf):
    table = importlib.import_module("3d-beats_amd._lib").SIGNATURES
    single = {"rdf_prepare_hand_depth_batch": "rdf_prepare_hand_depth", "rdf_layered_run_hand_batch": "rdf_layered_run_hand",
              "rdf_mean_shift_heights_batch": "rdf_mean_shift_heights"}
    for name, one in single.items():
        assert name in table
        # the batch form takes the single form's arguments and the frame count (the mean shift: and the heights' stride)
        assert len(table[name][1]) == len(table[one][1]) + (2 if "mean_shift" in name else 1), name
    assert importlib.import_module("3d-beats_amd._lib").ABI_VERSION == 5


def test_prepare_batch_rejects_before_any_launch(rdf):
    lib = _lib()
    assert lib.rdf_prepare_hand_depth_batch(-1, 8, 4, 0, 1, FAKE, FAKE, FAKE + 64, 0, None) == -1
    assert lib.rdf_prepare_hand_depth_batch(2, 8, 4, 31, 1, FAKE, FAKE, FAKE + 64, 0, None) == -1
    assert lib.rdf_prepare_hand_depth_batch(2, 8, 4, 0, 1, FAKE, FAKE, None, 0, None) == -2
    assert lib.rdf_prepare_hand_depth_batch(2, 8, 4, 0, 1, None, FAKE, FAKE + 64, 0, None) == -2
    assert lib.rdf_prepare_hand_depth_batch(2, 8, 4, 0, 1, FAKE, FAKE, FAKE, 1, None) == -1      # a flip in place
    assert lib.rdf_prepare_hand_depth_batch(0, 8, 4, 0, 1, None, None, None, 0, None) == 0       # nothing to do


def test_layered_batch_rejects_before_any_launch(rdf):
    lib = _lib()

    def call(n_img, dim_x, dim_y, out, r=1, n_layers=0):
        return lib.rdf_layered_run_hand_batch(FAKE, n_img, dim_x, dim_y, n_layers, None, None, None, None, None, None, None,
                                              None, None, None, 0, out, None, r, 1.0, 0, None, 0, None, None)
    assert call(-1, 8, 8, FAKE) == -1
    assert call(2, 8, 8, FAKE, r=0) == -1
    assert call(2, 8, 8, None) == -2
    assert call(2, 8, 8, FAKE, n_layers=2) == -2                  # the layers' host arrays are missing
    # 2 x 32768 x 32768 label pixels = 2^31
    assert call(2, 32768, 32768, FAKE) == -3
    assert call(8, 65536, 65536, FAKE, r=2) == -3                 # 8 x 32768 x 32768 label pixels


def test_mean_shift_batch_rejects_before_any_launch(rdf):
    lib = _lib()

    def call(n=2, L=7, n_ids=5, stride=10, means=FAKE, heights=FAKE, ids=FAKE, depth=FAKE, plane=FAKE, dim_x=53):
        return lib.rdf_mean_shift_heights_batch(FAKE, n, dim_x, 31, L, FAKE, 6, means, ids, n_ids, depth, 106, 62, 2,
                                                *INTR, plane, heights, stride, None)
    assert call(n=-1) == -1
    assert call(stride=4) == -1                                   # heights_stride < n_ids
    assert call(n_ids=0) == -1 and call(L=0) == -1                # no two-call fallback in the batch form
    assert call(dim_x=65536) == -1
    assert call(heights=None) == -2 and call(means=None) == -2
    assert call(ids=None) == -2 and call(depth=None) == -2 and call(plane=None) == -2
    assert call(n=0) == 0


# ------------------------------------------------------------------ GPU ------------------------------------------------------
_front_cache = {}


def _points_ops():
    return importlib.import_module("3d-beats_amd.cuda.points_ops").PointsOps()


def _front(rdf):
    """Five frames of the session scene after the front end and the grouping (level 3), on the device: raw, clean, groups;
    computed once and only read by the tests."""
    if not _front_cache:
        frames, intr = sc.frames()
        s = rdf.BeatsSession(ts._stack(rdf, (sc.H, sc.W), sc.forest_config(rdf)), (sc.H, sc.W), intr, num_random_guesses=4000,
                             seed=3, max_frames=5)
        s.calibrate(frames[0])
        raw = rdf.to_device(frames[:5])
        clean = rdf.DeviceArray((5, sc.H, sc.W), np.uint16)
        groups = rdf.DeviceArray((5, sc.H >> sc.LEVEL, sc.W >> sc.LEVEL), np.uint16)
        s.front_end.run(raw, clean)
        s.grouping.make_group_image(clean, groups)
        g = groups.get()
        assert all((g[k] == 1).any() and (g[k] == 2).any() for k in range(5))
        _front_cache.update(raw=raw, clean=clean, groups=groups)
    return _front_cache


def _prepared(rdf, g_id, flip):
    """The five frames stencilled for one hand, frame by frame with the single call (host uint16 [5, H, W])."""
    key = ("prep", g_id, flip)
    if key not in _front_cache:
        f = _front(rdf)
        po = _points_ops()
        out = rdf.DeviceArray((5, sc.H, sc.W), np.uint16).fill(1234)
        dims = np.array([sc.W, sc.H], np.int32)
        for k in range(5):
            po.prepare_hand_depth(dims, sc.LEVEL, g_id, f["groups"][k], f["clean"][k], out[k], flip)
        _front_cache[key] = out.get()
    return _front_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("g_id", [1, 2])
@pytest.mark.parametrize("flip", [False, True])
def test_prepare_batch_equals_five_single_calls(g_id, flip, rdf, gpu_runtime):
    f = _front(rdf)
    want = _prepared(rdf, g_id, flip)
    assert ((want != 65535).sum((1, 2)) >= 800).all(), "a hand in every frame, or the comparison shows nothing"
    out = rdf.DeviceArray((5, sc.H, sc.W), np.uint16).fill(4321)
    _points_ops().prepare_hand_depth_batch(5, np.array([sc.W, sc.H], np.int32), sc.LEVEL, g_id, f["groups"], f["clean"], out,
                                             flip)
    assert np.array_equal(out.get(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_prepare_batch_with_a_frame_stride_that_is_no_multiple_of_16_bytes(flip, rdf, gpu_runtime):
    """3 frames of 61 x 107 at level 2: 13 054 bytes a frame, rows of 107 pixels -- the scalar path, and a last lane of
    three pixels in every row.  The bytes behind the last frame stay as they were."""
    h, w, level, n = 61, 107, 2, 3
    assert (h * w * 2) % 16 != 0 and w % 8 != 0
    rng = np.random.default_rng(61)
    depth = rng.integers(0, 3000, (n, h, w)).astype(np.uint16)
    depth[rng.random((n, h, w)) < 0.2] = 0
    groups = rng.integers(0, 3, (n, h >> level, w >> level)).astype(np.uint16)
    dd, dg = rdf.to_device(depth), rdf.to_device(groups)
    po = _points_ops()
    dims = np.array([w, h], np.int32)
    guard = 64
    for g_id in (1, 2):
        want = rdf.DeviceArray((n, h, w), np.uint16).fill(1234)
        for k in range(n):
            po.prepare_hand_depth(dims, level, g_id, dg[k], dd[k], want[k], flip)
        want = want.get()
        assert (want != 65535).sum() >= 1000
        buf = rdf.DeviceArray((n * h * w + guard,), np.uint16).fill(0xABCD)
        po.prepare_hand_depth_batch(n, dims, level, g_id, dg, dd, buf[:n * h * w].reshape((n, h, w)), flip)
        got = buf.get()
        assert np.array_equal(got[:n * h * w].reshape(n, h, w), want)
        assert (got[n * h * w:] == 0xABCD).all()


def _frame_by_frame(rdf, lf, frames, scale, flip):
    """run_hand on each frame: (composites, layer-0 labels, layer-1 labels, RGBA images, bad pixels)."""
    n, (lh, lw) = len(frames), lf.labels_dims
    dbuf = rdf.GpuBuffer(frames.shape[1:], np.uint16)
    lab, rgba = rdf.GpuBuffer((lh, lw), np.uint16), rdf.GpuBuffer((lh, lw, 4), np.uint8)
    out = [np.zeros((n, lh, lw), np.uint16) for _ in range(3)] + [np.zeros((n, lh, lw, 4), np.uint8)]
    lf.eval.composite_bad_pixels()
    for k in range(n):
        dbuf.cu().set(frames[k])
        rgba.cu().fill(0x5A)
        lf.run_hand(dbuf, lab, scale, flip, rgba)
        out[0][k], out[3][k] = lab.cu().get(), rgba.cu().get()
        out[1][k], out[2][k] = lf.label_images[0].cu().get(), lf.label_images[1].cu().get()
    return out + [lf.eval.composite_bad_pixels()]


def _batch(rdf, lf, frames, scale, flip):
    n, (lh, lw) = len(frames), lf.labels_dims
    lab = rdf.DeviceArray((n, lh, lw), np.uint16).fill(77)
    rgba = rdf.DeviceArray((n, lh, lw, 4), np.uint8).fill(0x5A)
    lf.eval.composite_bad_pixels()
    lf.run_hand_batch(rdf.to_device(frames), lab, scale, flip, rgba)
    return [lab.get(), lf.batch_label_images[0][:n].get(), lf.batch_label_images[1][:n].get(), rgba.get(),
            lf.eval.composite_bad_pixels()]


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_layered_batch_equals_run_hand_frame_by_frame(flip, rdf, gpu_runtime):
    """The two-layer filtered stack on five stencilled hand frames of 240 x 424, labels_reduce 2: composite, both per-layer
    label images, the RGBA image and the bad-pixel total; and a batch of one."""
    frames = _prepared(rdf, 2 if flip else 1, flip)
    lf = ts._stack(rdf, (sc.H, sc.W), sc.forest_config(rdf))
    scale = sc.W / 848
    want = _frame_by_frame(rdf, lf, frames, scale, flip)
    comp, l0, l1 = want[:3]
    labelled = ((comp != 65535) & (comp != 0)).sum((1, 2))
    removed = int(((l0 != 65535) & (l0 != 3) & (l1 == 65535)).sum())
    print(f"flip={flip}: labelled pixels per frame {labelled.tolist()}, removed by layer 1's filter {removed}, "
          f"layer-1 labels {int((l1 != 65535).sum())}, bad {want[4]}")
    assert (labelled >= 200).all() and removed >= 1 and (l1 != 65535).any()
    single_labels = [b.cu().get() for b in lf.label_images]
    got = _batch(rdf, lf, frames, scale, flip)
    for k, name in enumerate(("composite", "layer 0", "layer 1", "rgba")):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
    assert got[4] == want[4]
    # the batch has its own per-layer buffers: the single-frame path's still hold the last single frame
    for b, before in zip(lf.label_images, single_labels):
        assert np.array_equal(b.cu().get(), before)
    one = _batch(rdf, lf, frames[:1], scale, flip)
    for k in range(4):
        assert np.array_equal(one[k], want[k][:1]), k
    # a sibling has batch buffers of its own, and a stack that cannot take the fused call refuses
    sib = lf.sibling()
    got_s = _batch(rdf, sib, frames[:2], scale, flip)
    assert np.array_equal(got_s[0], want[0][:2]) and sib.batch_label_images[0].ptr != lf.batch_label_images[0].ptr
    lf.fused = False
    with pytest.raises(ValueError):
        lf.run_hand_batch(rdf.to_device(frames[:2]), rdf.DeviceArray((2,) + tuple(lf.labels_dims), np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_layered_batch_with_unaligned_frame_strides(flip, rdf, gpu_runtime):
    """3 frames of 62 x 106, labels_reduce 2: label frames of 31 x 53 = 3 286 bytes, depth frames of 13 144 bytes (no
    multiple of 16 either way)."""
    h, w = 62, 106
    full = _prepared(rdf, 1, False)
    # the window round the right hand's fingers and palm; frames 0, 2, 4
    frames = np.ascontiguousarray(full[0:5:2, 90:90 + h, 75:75 + w])
    if flip:
        frames = np.ascontiguousarray(frames[:, :, ::-1])
    assert ((h // 2) * (w // 2) * 2) % 16 != 0 and (h * w * 2) % 16 != 0
    lf = ts._stack(rdf, (h, w), sc.forest_config(rdf))
    scale = sc.W / 848
    want = _frame_by_frame(rdf, lf, frames, scale, flip)
    labelled = ((want[0] != 65535) & (want[0] != 0)).sum((1, 2))
    print(f"flip={flip}: labelled pixels per frame {labelled.tolist()}, layer-1 labels {int((want[2] != 65535).sum())}")
    assert (labelled >= 200).all()
    got = _batch(rdf, lf, frames, scale, flip)
    for k, name in enumerate(("composite", "layer 0", "layer 1", "rgba")):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
    assert got[4] == want[4]


def _blobs(seed, n, h, w, L, absent=()):
    """Label maps [n, h, w]: one ellipse and three stray pixels a class; `absent` = (frame, class) pairs left out."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    lab = np.full((n, h, w), 65535, np.uint16)
    for f in range(n):
        for c in range(1, L + 1):
            if (f, c) in absent:
                continue
            cx, cy = rng.uniform(4, w - 4), rng.uniform(4, h - 4)
            a, b = rng.uniform(2, 6), rng.uniform(2, 6)
            lab[f][((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1] = c
            for _ in range(3):
                lab[f, rng.integers(0, h), rng.integers(0, w)] = c
        lab[f, 0, 0] = 0
    return lab


def _mean_shift_both_ways(rdf, lab, depth, L, r, ids, var, rounds, col0=5, stride=10):
    """(means, heights) frame by frame with rdf_mean_shift_heights, and the batch call's means and its whole heights block
    [n, stride] (pre-filled with 7.0, the ids' columns from col0)."""
    ms = importlib.import_module("3d-beats_amd.cuda.mean_shift").MeanShift()
    n = lab.shape[0]
    plane = (np.eye(4) + 0.1 * np.random.default_rng(5).standard_normal((4, 4))).astype(np.float32)
    dl, dd, dv = rdf.to_device(lab), rdf.to_device(depth), rdf.to_device(np.asarray(var, np.float32))
    d_ids, d_plane = rdf.to_device(np.asarray(ids, np.int32)), rdf.to_device(plane)
    want_m, want_h = np.zeros((n, L, 2)), np.zeros((n, len(ids)))
    for f in range(n):
        out = rdf.DeviceArray((2 * L + len(ids),), np.float64).fill(7.0)
        ms.run_device_with_heights(rounds, dl[f:f + 1], L, dv, d_ids, len(ids), dd[f], r, INTR, d_plane, out.ptr,
                                   out.ptr + 16 * L)
        o = out.get()
        want_m[f], want_h[f] = o[:2 * L].reshape(L, 2), o[2 * L:]
    means = rdf.DeviceArray((n, L, 2), np.float64).fill(7.0)
    block = rdf.DeviceArray((n, stride), np.float64).fill(7.0)
    ms.run_device_with_heights_batch(rounds, dl, L, dv, d_ids, len(ids), dd, r, INTR, d_plane, means.ptr,
                                     block.ptr + 8 * col0, stride)
    return want_m, want_h, means.get(), block.get()


@pytest.mark.gpu
def test_mean_shift_batch_equals_the_single_call_per_frame(rdf, gpu_runtime):
    """Labels [4][31][53], 7 classes; class 4 is absent from frame 2 (NaN mode, NaN height), id 9 names no class (NaN in
    every frame); the heights go to columns 5-9 of a [4][10] block whose columns 0-4 must survive."""
    n, h, w, L, r = 4, 31, 53, 7, 2
    lab = _blobs(31, n, h, w, L, absent=((2, 4),))
    depth = np.random.default_rng(32).integers(300, 900, (n, h * r, w * r)).astype(np.uint16)
    ids = [2, 3, 9, 5, 4]
    for rounds in (1, 6):
        want_m, want_h, got_m, block = _mean_shift_both_ways(rdf, lab, depth, L, r, ids, [50.] + [8.] * 6, rounds)
        assert np.isnan(want_m[2, 3]).all() and np.isnan(want_h[2, 4]) and np.isnan(want_h[:, 2]).all()
        assert np.isfinite(np.delete(want_m, 2, 0)).all() and np.isfinite(want_h[:, [0, 1, 3]]).all()
        assert len({want_h[f, 0] for f in range(n)}) > 1, "every frame the same height: the frame offset would not show"
        assert np.array_equal(_bits(got_m), _bits(want_m))
        assert np.array_equal(_bits(block[:, 5:]), _bits(want_h)), (block[:, 5:], want_h)
        assert (block[:, :5] == 7.0).all()


@pytest.mark.gpu
def test_mean_shift_batch_with_one_frame_on_the_rescan_path(rdf, gpu_runtime):
    """Labels [3][160][256]: class 1 of frame 1 has more pixels than a workgroup lists in LDS (32 768) and rescans the label
    image every round; the frames either side list theirs.  All three equal the single call."""
    n, h, w, L = 3, 160, 256, 3
    lab = _blobs(41, n, h, w, L)
    big = np.random.default_rng(42).random((h, w)) < 0.9
    big[60:80, 100:140] = False                     # (classes 2 and 3 keep a patch of their own in frame 1)
    lab[1][big] = 1
    lab[1, 62:70, 102:118], lab[1, 72:78, 120:136] = 2, 3
    assert (lab[1] == 1).sum() > 32768 and max((lab[f] == c).sum() for f in (0, 2) for c in (1, 2, 3)) < 32768
    depth = np.random.default_rng(43).integers(300, 900, (n, h, w)).astype(np.uint16)
    want_m, want_h, got_m, block = _mean_shift_both_ways(rdf, lab, depth, L, 1, [1, 2, 3], [80., 9., 5.], 5, col0=0, stride=3)
    assert np.isfinite(want_m).all() and np.isfinite(want_h).all()
    assert np.array_equal(_bits(got_m), _bits(want_m))
    assert np.array_equal(_bits(block), _bits(want_h))
