"""the element-wise kernels that define the forest's input convention and colour its output.
CPU: hand-derived answers for the numpy restatement.  GPU: byte-exact against the restatement."""
import importlib

import numpy as np
import pytest

from oracle import points_ops_numpy as po_np


def test_known_answers_numpy():
    d = np.array([[0, 5, 65535], [7, 0, 1]], np.uint16)
    assert po_np.convert_0s_to_maxuint(d.copy()).tolist() == [[65535, 5, 65535], [7, 65535, 1]]
    pts = np.ones((2, 3, 4), np.float32)
    pts[0, 1, 3] = 0.0                      # filtered point: w == 0 (points_ops.cu:160-162)
    assert po_np.setup_depth_image_for_forest(pts, d.copy()).tolist() == [[65535, 65535, 65535], [7, 65535, 1]]
    # stencil at mip level 1 on a 5x3 image: groups are 2x1 (integer division), the odd last row/column reads
    # out of bounds = group 0
    g = np.array([[1, 2]], np.uint16)
    din = np.arange(15, dtype=np.uint16).reshape(3, 5) + 100
    out = po_np.stencil_depth_image_by_group(5, 3, 1, 2, g, din, np.zeros((3, 5), np.uint16))
    assert out.tolist() == [[0, 0, 102, 103, 0], [0, 0, 107, 108, 0], [0, 0, 0, 0, 0]]
    out0 = po_np.stencil_depth_image_by_group(5, 3, 1, 0, g, din, np.zeros((3, 5), np.uint16))
    assert out0.tolist() == [[0, 0, 0, 0, 104], [0, 0, 0, 0, 109], [110, 111, 112, 113, 114]]
    assert po_np.flip_x(np.array([[1, 2, 3]], np.uint16), np.zeros((1, 3), np.uint16)).tolist() == [[3, 2, 1]]
    cols = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.uint8)
    img = po_np.make_rgba_from_labels(np.array([[0, 1, 2, 3, 65535]], np.uint16), cols, np.full((1, 5, 4), 9, np.uint8))
    assert img.tolist() == [[[9] * 4, [1, 2, 3, 4], [5, 6, 7, 8], [9] * 4, [9] * 4]]


@pytest.mark.gpu
def test_pointsops_byte_exact_on_gpu(rdf, gpu_runtime):
    pmod = importlib.import_module("3d-beats_amd.cuda.points_ops")
    ops = pmod.PointsOps()
    rng = np.random.default_rng(21)
    for (h, w) in [(480, 848), (37, 53), (1, 1), (240, 424)]:
        depth = rdf.synth.live_frame(5, h, w) if h > 8 else np.array([[0]], np.uint16)
        n = h * w
        # convert_0s_to_maxuint, also on unaligned sub-ranges
        for off in (0, 1, 3):
            if off >= n:
                continue
            dev = rdf.to_device(depth.reshape(-1))
            ops.convert_0s_to_maxuint(np.int32(n - off), dev.view(np.uint16)[off:] if off else dev)
            want = depth.reshape(-1).copy()
            po_np.convert_0s_to_maxuint(want[off:])
            assert np.array_equal(dev.get(), want), (h, w, off)
        # setup_depth_image_for_forest
        pts = rng.standard_normal((h, w, 4)).astype(np.float32)
        pts[..., 3] = (rng.random((h, w)) > 0.3).astype(np.float32)
        dev = rdf.to_device(depth)
        ops.setup_depth_image_for_forest(np.int32(n), rdf.to_device(pts), dev)
        assert np.array_equal(dev.get(), po_np.setup_depth_image_for_forest(pts, depth.copy()))
        # stencil by group at mip levels 0..3
        for level in (0, 1, 3):
            f = 1 << level
            gw, gh = max(w // f, 1), max(h // f, 1)
            groups = rng.integers(0, 3, size=(gh, gw)).astype(np.uint16)
            for group in (1, 0):
                out = rdf.to_device(np.full((h, w), 7, np.uint16))
                ops.stencil_depth_image_by_group(np.array([w, h], np.int32), np.int32(level), np.int32(group),
                                                 rdf.to_device(groups), rdf.to_device(depth), out)
                want = po_np.stencil_depth_image_by_group(w, h, level, group, groups if w // f and h // f else groups[:0],
                                                          depth, np.full((h, w), 7, np.uint16))
                assert np.array_equal(out.get(), want), (h, w, level, group)
        # flip_x
        out = rdf.DeviceArray((h, w), np.uint16)
        ops.flip_x(np.array([w, h], np.int32), rdf.to_device(depth), out)
        assert np.array_equal(out.get(), depth[:, ::-1])
        # make_rgba_from_labels
        labels = rng.integers(0, 9, size=(h, w)).astype(np.uint16)
        labels[rng.random((h, w)) < 0.2] = 65535
        cols = rng.integers(0, 256, size=(6, 4)).astype(np.uint8)
        img = rdf.to_device(np.full((h, w, 4), 3, np.uint8))
        ops.make_rgba_from_labels(np.uint32(w), np.uint32(h), np.uint32(6), rdf.to_device(labels), rdf.to_device(cols), img)
        assert np.array_equal(img.get(), po_np.make_rgba_from_labels(labels, cols, np.full((h, w, 4), 3, np.uint8)))


@pytest.mark.gpu
def test_prepare_hand_depth_equals_the_chain_it_replaces(rdf, gpu_runtime):
    """rdf_prepare_hand_depth == fill(0) -> stencil_depth_image_by_group -> flip_x (or copy) -> convert_0s_to_maxuint
    (3d_bz.py:396-420), byte for byte: vector and scalar widths, every mip level, both orientations, in place."""
    pmod = importlib.import_module("3d-beats_amd.cuda.points_ops")
    ops = pmod.PointsOps()
    rng = np.random.default_rng(33)
    for (h, w) in [(480, 848), (37, 53), (1, 1), (240, 424), (16, 8), (9, 24)]:
        depth = rdf.synth.live_frame(9, h, w) if h > 8 else rng.integers(0, 3, size=(h, w)).astype(np.uint16)
        depth[rng.random((h, w)) < 0.1] = 0
        for level in (0, 1, 3):
            f = 1 << level
            gw, gh = max(w // f, 1), max(h // f, 1)
            groups = rng.integers(0, 3, size=(gh, gw)).astype(np.uint16)
            g_host = groups if w // f and h // f else groups[:0]
            for group in (1, 2):
                for flip in (False, True):
                    want = po_np.stencil_depth_image_by_group(w, h, level, group, g_host, depth, np.zeros((h, w), np.uint16))
                    want = want[:, ::-1].copy() if flip else want
                    po_np.convert_0s_to_maxuint(want)
                    out = rdf.to_device(np.full((h, w), 7, np.uint16))
                    ops.prepare_hand_depth(np.array([w, h], np.int32), level, group, rdf.to_device(groups), rdf.to_device(depth),
                                           out, flip)
                    assert np.array_equal(out.get(), want), (h, w, level, group, flip)
            inplace = rdf.to_device(depth)
            ops.prepare_hand_depth(np.array([w, h], np.int32), level, 1, rdf.to_device(groups), inplace, inplace, False)
            want = po_np.convert_0s_to_maxuint(po_np.stencil_depth_image_by_group(w, h, level, 1, g_host, depth,
                                                                                  np.zeros((h, w), np.uint16)))
            assert np.array_equal(inplace.get(), want)
    d = rdf.to_device(np.ones((4, 8), np.uint16))
    rc = gpu_runtime.lib.rdf_prepare_hand_depth(8, 4, 0, 1, d.ptr, d.ptr, d.ptr, 1, gpu_runtime.stream())
    assert rc == -1      # a flip in place is refused


# ---- the branches no 16-byte-aligned, camera-sized input reaches ----

def _ops():
    return importlib.import_module("3d-beats_amd.cuda.points_ops").PointsOps()


def _at_offset(rdf, flat, k, shape=None):
    """`flat` on the device inside a larger buffer, starting k elements (2k bytes) past a 16-byte boundary: (the whole
    buffer, the view of `flat`)."""
    whole = rdf.to_device(np.concatenate([np.zeros(8 + k, np.uint16), flat.reshape(-1), np.zeros(8, np.uint16)]))
    view = whole.view(np.uint16)[8 + k:8 + k + flat.size]
    assert view.ptr % 16 == 2 * k
    return whole, view.reshape(shape) if shape else view


@pytest.mark.gpu
def test_convert_0s_short_ranges_at_every_alignment(rdf, gpu_runtime):
    """n = 1 .. 17 at every element offset 0 .. 7 from a 16-byte boundary: ranges shorter than the unaligned head (head > n),
    head only, head + one vector, head + vector + tail.  Every element of the range starts as 0 in one pass and as a mix in
    the other; the zeros on both sides of the range stay zero."""
    ops = _ops()
    rng = np.random.default_rng(41)
    for n in (1, 2, 3, 7, 8, 9, 15, 16, 17):
        for k in range(8):
            for data in (np.zeros(n, np.uint16), rng.choice(np.array([0, 0, 1, 77, 65535], np.uint16), size=n)):
                whole, view = _at_offset(rdf, data, k)
                ops.convert_0s_to_maxuint(n, view)
                want = np.concatenate([np.zeros(8 + k, np.uint16), po_np.convert_0s_to_maxuint(data.copy()),
                                       np.zeros(8, np.uint16)])
                assert np.array_equal(whole.get(), want), (n, k, whole.get(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1])
def test_convert_0s_second_trip_of_the_grid_stride_loops(rdf, gpu_runtime, k):
    """More vectors than the 2048 x 256 lanes of the capped grid: 2048 * 256 + 256 vectors plus a 5-element tail, aligned
    and one element off (a 7-element head)."""
    n = 2048 * 256 * 8 + 8 * 256 + 5
    rng = np.random.default_rng(42 + k)
    data = rng.integers(0, 4, size=n).astype(np.uint16) * np.uint16(21845)      # 0, 21845, 43690, 65535; a quarter zeros
    data[[0, 1, 6, 7, 8, n - 6, n - 5, n - 1, 2048 * 256 * 8, 2048 * 256 * 8 + 7]] = 0
    whole, view = _at_offset(rdf, data, k)
    _ops().convert_0s_to_maxuint(n, view)
    got = whole.get()
    assert not got[:8 + k].any() and not got[-8:].any()
    assert np.array_equal(got[8 + k:-8], po_np.convert_0s_to_maxuint(data.copy()))


@pytest.mark.gpu
def test_prepare_hand_depth_misaligned_pointers_at_vector_widths(rdf, gpu_runtime):
    """Widths that are multiples of 8 (one lane, two lanes, one block row of 512, one lane and one block more) take the
    16-byte path only when both pointers allow it: the input, the output, then both one element off a 16-byte boundary must
    give the bytes of the aligned call -- the chain fill(0) -> stencil -> flip or copy -> convert_0s -- and leave the rows
    before and after the output as they were."""
    ops = _ops()
    rng = np.random.default_rng(43)
    for w in (8, 16, 512, 520, 1032):
        for h in (1, 4, 5):
            depth = rng.integers(0, 4, size=(h, w)).astype(np.uint16) * rng.integers(1, 16384, size=(h, w)).astype(np.uint16)
            assert (depth == 0).any()
            ins = [_at_offset(rdf, depth, k, (h, w))[1] for k in (0, 1)]
            for level in (0, 1, 3):
                f = 1 << level
                gw, gh = max(w // f, 1), max(h // f, 1)
                groups = rng.integers(0, 3, size=(gh, gw)).astype(np.uint16)
                g_host = groups if w // f and h // f else groups[:0]
                d_groups = rdf.to_device(groups)
                for flip in (False, True):
                    want = po_np.stencil_depth_image_by_group(w, h, level, 1, g_host, depth, np.zeros((h, w), np.uint16))
                    want = want[:, ::-1].copy() if flip else want
                    po_np.convert_0s_to_maxuint(want)
                    for k_in, k_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
                        frame = np.full((h + 2, w), 7, np.uint16)            # a row before and a row after the output
                        whole, framed = _at_offset(rdf, frame, k_out, (h + 2, w))
                        out = framed[1:h + 1]
                        assert out.ptr % 16 == (2 * (k_out + w)) % 16 == 2 * k_out
                        ops.prepare_hand_depth(np.array([w, h], np.int32), level, 1, d_groups, ins[k_in], out, flip)
                        got = whole.get()
                        assert not got[:8 + k_out].any() and not got[-8:].any()
                        got = got[8 + k_out:-8].reshape(h + 2, w)
                        assert (got[0] == 7).all() and (got[-1] == 7).all(), (w, h, level, flip, k_in, k_out)
                        assert np.array_equal(got[1:-1], want), (w, h, level, flip, k_in, k_out)


@pytest.mark.gpu
def test_setup_depth_keeps_points_whose_w_is_tiny_or_nan(rdf, gpu_runtime):
    """w == 0.0f is true for -0.0 and for nothing else: NaN, the subnormals and the smallest normal numbers of either sign
    are points that stay (a build that flushed subnormals would drop them)."""
    tiny, sub = np.finfo(np.float32).tiny, np.float32(1e-45)
    ws = np.array([0.0, -0.0, np.nan, sub, -sub, np.float32(5.9e-39), np.float32(-5.9e-39), tiny, -tiny, 1.0, -np.nan],
                  np.float32)
    assert ws[3] > 0 and ws[5] < tiny and np.signbit(ws[1])
    n = 300                                                     # two blocks
    pts = np.random.default_rng(44).standard_normal((n, 4)).astype(np.float32)
    pts[:, 3] = ws[np.arange(n) % ws.size]
    depth = np.where(np.arange(n) % 13 == 0, 0, 1234).astype(np.uint16)
    want = po_np.setup_depth_image_for_forest(pts, depth.copy())
    keep = (depth != 0) & (np.arange(n) % ws.size >= 2)
    assert (want[keep] == 1234).all() and (want[~keep] == 65535).all()
    dev = rdf.to_device(depth)
    _ops().setup_depth_image_for_forest(n, rdf.to_device(pts), dev)
    assert np.array_equal(dev.get(), want), np.flatnonzero(dev.get() != want)


@pytest.mark.gpu
def test_rgba_without_colors_and_flip_x_at_the_block_width(rdf, gpu_runtime):
    """num_colors = 0 (no colour table at all): every label is beyond it and the image stays as it was.  flip_x at one
    column, and one under, at and over the 64 columns of a block."""
    ops = _ops()
    rng = np.random.default_rng(45)
    labels = rng.integers(0, 6, size=(5, 70)).astype(np.uint16)
    labels[2, 3:9] = 65535
    before = rng.integers(0, 256, size=(5, 70, 4)).astype(np.uint8)
    img = rdf.to_device(before)
    ops.make_rgba_from_labels(70, 5, 0, rdf.to_device(labels), None, img)
    assert np.array_equal(img.get(), before)
    assert np.array_equal(po_np.make_rgba_from_labels(labels, np.zeros((0, 4), np.uint8), before.copy()), before)
    for w in (1, 63, 64, 65):
        for h in (1, 5):
            src = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
            whole, out = _at_offset(rdf, np.full((h, w), 7, np.uint16), 0, (h, w))
            ops.flip_x(np.array([w, h], np.int32), rdf.to_device(src), out)
            got = whole.get()
            assert not got[:8].any() and not got[-8:].any()
            assert np.array_equal(got[8:-8].reshape(h, w), po_np.flip_x(src, np.zeros((h, w), np.uint16))), (w, h)
