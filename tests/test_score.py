"""Scoring label maps on the device (rdf_score_labels of librdf_labels.so, score.Score / score.LabelScorer, the dataset
functions on top of them) against the numpy restatement in tests/score_numpy.py.  The CPU tests pin the restatement and
Score's arithmetic to cases worked by hand and check the C entry points' argument checks, which launch nothing; every GPU
comparison is bit for bit, with no pixel left out."""
import ctypes
import importlib
import json

import numpy as np
import pytest

import score_numpy as snp


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _literal(got, truth):
    """The host expression of dataset.py, as it stands there."""
    with np.errstate(all="ignore"):
        return float(np.sum(got == truth) / np.sum(truth > 0))


def _same_float(a, b):
    return np.array_equal(np.array([a], np.float64).view(np.uint64), np.array([b], np.float64).view(np.uint64))


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_hand_worked_frame():
    C = 3
    truth = np.array([[[0, 1, 2], [2, 5, 1]]], np.uint16)
    pred = np.array([[[0, 1, 65535], [300, 5, 2]]], np.uint16)
    # (t, p) clamped: (0,0) (1,1) (2,3) / (2,3) (3,3) (1,2)
    want = np.zeros((4, 4), np.uint64)
    want[0, 0] = 1
    want[1, 1] = 1
    want[2, 3] = 2          # the 65535 pre-fill and the unknown id 300 are both "none"
    want[3, 3] = 1          # truth id 5 >= C against prediction 5: unknown by unknown
    want[1, 2] = 1
    counts = snp.score_counts(pred, truth, C)
    assert counts.dtype == np.uint64 and counts.shape == (18,)
    assert np.array_equal(counts[:16].reshape(4, 4), want)
    # equal compares raw values: (0, 0), (1, 1) and (5, 5); labelled leaves out the (0, 0) pixel
    assert counts[16] == 3 and counts[17] == 5
    assert counts[:16].sum() == pred.size
    assert snp.score_per_image(pred, truth).tolist() == [[3, 5]]
    # the call adds
    again = snp.score_counts(pred, truth, C, onto=counts)
    assert np.array_equal(again, 2 * counts)
    s = _mod("score").Score.from_counts(counts, C)
    assert _same_float(s.pct_matching, _literal(pred, truth)) and s.pct_matching == 0.6 and s.num_pixels == 6


def test_reduced_maps_read_only_the_even_coordinates():
    C, r = 3, 2
    truth = np.full((1, 5, 7), 9, np.uint16)          # whatever sits on an odd row or column must not be read
    truth[0, 0:4:2, 0:6:2] = [[1, 0, 2], [2, 2, 0]]
    pred = np.array([[[1, 0, 1], [65535, 2, 0]]], np.uint16)
    assert snp.sample_truth(truth, r, (2, 3)).tolist() == [[[1, 0, 2], [2, 2, 0]]]
    want = np.zeros((4, 4), np.uint64)
    want[1, 1] = 1
    want[0, 0] = 2
    want[2, 1] = 1
    want[2, 3] = 1
    want[2, 2] = 1
    counts = snp.score_counts(pred, truth, C, r)
    assert np.array_equal(counts[:16].reshape(4, 4), want) and counts[:16].sum() == 6
    assert counts[16] == 4 and counts[17] == 4
    other = truth.copy()
    other[0, 1::2] = 1
    other[0, :, 1::2] = 2
    other[0, 4] = 3                                   # row 4 = 2 * 2 is beyond the 2-row label map
    other[0, :, 6] = 3
    assert np.array_equal(snp.score_counts(pred, other, C, r), counts)


@pytest.mark.parametrize("seed", range(4))
def test_pct_matching_is_the_host_expression(seed):
    Score = _mod("score").Score
    rng = np.random.default_rng(seed)
    C = int(rng.integers(1, 9))
    truth = rng.integers(0, C + 2, (3, 9, 11)).astype(np.uint16)
    pred = rng.integers(0, C + 1, (3, 9, 11)).astype(np.uint16)
    pred[rng.random(pred.shape) < 0.3] = 65535
    for t in (truth, np.zeros_like(truth)):           # the second: labelled == 0, k / 0 = inf
        s = Score.from_counts(snp.score_counts(pred, t, C), C, snp.score_per_image(pred, t))
        assert _same_float(s.pct_matching, _literal(pred, t))
        assert s.equal == int(np.sum(pred == t)) and s.labelled == int(np.sum(t > 0))
        assert s.per_image[:, 0].sum() == s.equal and s.per_image[:, 1].sum() == s.labelled
    s = Score.from_counts(snp.score_counts(pred, np.zeros_like(truth), C), C)
    assert s.pct_matching == np.inf
    none = Score.from_counts(snp.score_counts(np.full_like(pred, 65535), np.zeros_like(truth), C), C)
    assert np.isnan(none.pct_matching) and _same_float(none.pct_matching, _literal(np.full_like(pred, 65535), np.zeros_like(truth)))


def test_metrics_on_a_hand_matrix():
    Score = _mod("score").Score
    C = 4
    m = np.zeros((5, 5), np.uint64)
    m[0] = [50, 1, 0, 0, 9]         # unlabelled truth
    m[1] = [2, 6, 2, 0, 0]          # class 1: 6 of 10 right
    m[2] = [0, 3, 9, 0, 8]          # class 2: 9 of 20 right
    #   class 3 never occurs in the truth and is never predicted; the "unknown" row and column C: no truth pixel
    counts = np.concatenate([m.reshape(-1), np.array([65, 30], np.uint64)])
    s = Score.from_counts(counts, C, per_image=np.array([[5, 10], [0, 0], [1, 10], [9, 10]], np.uint32))
    assert np.array_equal(s.confusion, m) and s.confusion.dtype == np.uint64 and s.num_classes == 4
    assert (s.equal, s.labelled) == (65, 30) and s.num_pixels == 90
    assert s.accuracy == 15 / 30                     # rows 1..3: (6 + 9 + 0) of 10 + 20 + 0
    assert s.recall[:3].tolist() == [50 / 60, 6 / 10, 9 / 20] and np.isnan(s.recall[3]) and np.isnan(s.recall[4])
    assert s.precision[:3].tolist() == [50 / 52, 6 / 10, 9 / 11] and np.isnan(s.precision[3]) and s.precision[4] == 0.
    assert s.iou[:3].tolist() == [50 / 62, 6 / 14, 9 / 22] and np.isnan(s.iou[3]) and s.iou[4] == 0.
    assert s.worst_images().tolist() == [2, 0, 3, 1] and s.worst_images(2).tolist() == [2, 0]
    empty = Score.from_counts(np.zeros(27, np.uint64), C)
    assert np.isnan(empty.accuracy) and np.isnan(empty.pct_matching) and np.isnan(empty.recall).all()
    with pytest.raises(AssertionError):
        empty.worst_images()
    with pytest.raises(AssertionError):
        Score.from_counts(np.zeros(26, np.uint64), C)


def test_counts_bytes_and_rejected_arguments(rdf):
    """Rejected arguments launch nothing, so they need no device; the pointers given here are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    assert [lib.rdf_score_counts_bytes(c) for c in (1, 3, 7, 64)] == [8 * 6, 8 * 18, 8 * 66, 8 * (65 * 65 + 2)]
    assert [lib.rdf_score_counts_bytes(c) for c in (0, -1, 65, 1 << 20)] == [0, 0, 0, 0]
    p, t, c = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000))
    BAD, NULL, LARGE = -1, -2, -3
    for C in (0, -3, 65):
        assert lib.rdf_score_labels(1, 8, 8, 1, C, p, t, c, None, None) == BAD
    assert lib.rdf_score_labels(1, 8, 8, 0, 3, p, t, c, None, None) == BAD
    assert lib.rdf_score_labels(1, 8, 8, -2, 3, p, t, c, None, None) == BAD
    for dims in ((-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        assert lib.rdf_score_labels(*dims, 1, 3, p, t, c, None, None) == BAD
    assert lib.rdf_score_labels(1, 8, 8, 1, 3, None, t, c, None, None) == NULL
    assert lib.rdf_score_labels(1, 8, 8, 1, 3, p, None, c, None, None) == NULL
    assert lib.rdf_score_labels(1, 8, 8, 1, 3, p, t, None, None, None) == NULL
    assert lib.rdf_score_labels(1, 65536, 32768, 1, 3, p, t, c, None, None) == LARGE
    assert lib.rdf_score_labels(32768, 256, 256, 4, 3, p, t, c, None, None) == LARGE
    assert lib.rdf_score_labels(1 << 30, 1 << 16, 1 << 16, 1, 3, p, t, c, None, None) == LARGE
    # pred and truth need 2-byte alignment, counts 8, per_image 4
    odd = ctypes.c_void_p(0x10001)
    assert lib.rdf_score_labels(1, 8, 8, 1, 3, odd, t, c, None, None) == BAD
    assert lib.rdf_score_labels(1, 8, 8, 1, 3, p, odd, c, None, None) == BAD
    assert lib.rdf_score_labels(1, 8, 8, 1, 3, p, t, ctypes.c_void_p(0x30004), None, None) == BAD
    assert lib.rdf_score_labels(1, 8, 8, 1, 3, p, t, c, ctypes.c_void_p(0x40002), None) == BAD
    # zero label pixels: a successful no-op, whatever the pointers
    assert lib.rdf_score_labels(0, 8, 8, 1, 3, None, None, None, None, None) == 0
    assert lib.rdf_score_labels(4, 0, 8, 1, 3, None, None, None, None, None) == 0
    assert lib.rdf_score_labels(4, 8, 3, 4, 3, None, None, None, None, None) == 0      # 3 // 4 rows
    assert b"score" in lib.rdf_labels_error_string(BAD)


def test_the_new_names_are_public(rdf):
    assert {"Score", "LabelScorer"} <= set(rdf.__all__)
    assert rdf.Score is _mod("score").Score and rdf.LabelScorer is _mod("score").LabelScorer
    for name in ("reset", "add", "result"):
        assert callable(getattr(rdf.LabelScorer, name))
    ds = _mod("dataset")
    assert callable(ds.score_saved_model) and callable(ds.score_layered_model) and ds.train_forest.last_score is None
    assert _mod("score").MAX_CLASSES == 64


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _maps(N, H, W, r, C, seed, background=0.0):
    """Random truth in 0..C+1 and predictions in 0..C (so both reach ids the model does not have), 65535 predictions, and
    about `background` of the label pixels (truth 0, prediction 65535)."""
    rng = np.random.default_rng(seed)
    hl, wl = H // r, W // r
    truth = rng.integers(0, C + 2, (N, H, W)).astype(np.uint16)
    pred = rng.integers(0, C + 1, (N, hl, wl)).astype(np.uint16)
    agree = rng.random(pred.shape) < 0.5
    pred[agree] = snp.sample_truth(truth, r, (hl, wl))[agree]
    pred[rng.random(pred.shape) < 0.1] = 65535
    pred[rng.random(pred.shape) < 0.02] = 300
    if background:
        yy, xx = np.mgrid[0:H, 0:W]
        blob = ((yy - H / 2) / (H * 0.22)) ** 2 + ((xx - W / 2) / (W * 0.22)) ** 2 < 1.       # ~15 % of the frame
        truth[:, ~blob] = 0
        pred[:, ~blob[:hl * r:r, :wl * r:r]] = 65535
    return pred, truth


def _check(rdf, pred, truth, C, r=1, per_image=True, to_pred=None, to_truth=None):
    scorer = rdf.LabelScorer(C)
    p = (to_pred or rdf.to_device)(pred)
    t = (to_truth or rdf.to_device)(truth)
    scorer.add(p, t, r, per_image=per_image)
    got = scorer.counts_cu.get()
    want = snp.score_counts(pred, truth, C, r)
    assert got.dtype == np.uint64 and np.array_equal(got, want), (np.flatnonzero(got != want)[:8], got[-2:], want[-2:])
    assert int(got[:-2].sum()) == pred.size
    s = scorer.result()
    assert np.array_equal(s.confusion, want[:-2].reshape(C + 1, C + 1)) and (s.equal, s.labelled) == (int(want[-2]), int(want[-1]))
    if per_image:
        assert s.per_image.dtype == np.uint32 and np.array_equal(s.per_image, snp.score_per_image(pred, truth, r))
    else:
        assert s.per_image is None
    return s


def _offset_view(rdf, a, off):
    """The array on the device, starting `off` elements into an allocation: 2 * off bytes past a 16-byte boundary."""
    flat = rdf.to_device(np.concatenate([np.full(off, 0xABCD, a.dtype), a.reshape(-1)]))
    return flat[off:].reshape(a.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("per_image", [True, False])
def test_odd_frames_with_image_boundaries_inside_a_vector(per_image, rdf, gpu_runtime):
    pred, truth = _maps(3, 5, 7, 1, 3, 1)
    s = _check(rdf, pred, truth, 3, 1, per_image)
    assert _same_float(s.pct_matching, _literal(pred, truth))


@pytest.mark.gpu
@pytest.mark.parametrize("per_image", [True, False])
def test_reduced_maps_with_odd_sizes(per_image, rdf, gpu_runtime):
    pred, truth = _maps(2, 37, 53, 2, 7, 2)
    assert pred.shape == (2, 18, 26)
    _check(rdf, pred, truth, 7, 2, per_image)
    pred, truth = _maps(3, 10, 9, 3, 4, 3)            # label images of 3 x 3: several images inside one lane's eight pixels
    _check(rdf, pred, truth, 4, 3, per_image)


@pytest.mark.gpu
def test_the_largest_histogram_and_the_smallest(rdf, gpu_runtime):
    C, H, W = 64, 72, 64
    k = np.arange(H * W)
    truth = (k % (65 * 65) // 65).astype(np.uint16).reshape(1, H, W)
    pred = (k % 65).astype(np.uint16).reshape(1, H, W)
    truth[truth == 64] = 70                           # an unknown truth id, as 65535 is an unknown prediction
    pred[pred == 64] = 65535
    s = _check(rdf, pred, truth, C)
    assert (s.confusion >= 1).all()
    for C in (31, 32):                                # the last size with a histogram per wave and the first without
        pred, truth = _maps(1, 72, 64, 1, C, C)
        _check(rdf, pred, truth, C)
    pred, truth = _maps(2, 31, 17, 1, 1, 4)
    s = _check(rdf, pred, truth, 1)
    assert s.confusion.shape == (2, 2)


@pytest.mark.gpu
def test_frames_of_one_cell(rdf, gpu_runtime):
    H, W, C = 480, 848, 7
    truth, pred = np.zeros((1, H, W), np.uint16), np.full((1, H, W), 65535, np.uint16)
    s = _check(rdf, pred, truth, C)
    assert s.confusion[0, C] == H * W and (s.equal, s.labelled) == (0, 0) and np.isnan(s.pct_matching)
    truth, pred = np.full((1, H, W), 3, np.uint16), np.full((1, H, W), 3, np.uint16)
    s = _check(rdf, pred, truth, C)
    assert s.confusion[3, 3] == H * W and s.pct_matching == 1.0 and s.accuracy == 1.0
    truth, pred = np.zeros((1, H, W), np.uint16), np.full((1, H, W), 65535, np.uint16)
    truth[0, 211, 503], pred[0, 211, 503] = 5, 2      # a single foreign pixel
    s = _check(rdf, pred, truth, C)
    assert s.confusion[5, 2] == 1 and s.confusion[0, C] == H * W - 1 and (s.equal, s.labelled) == (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(1, 1), (1, 0), (0, 1), (3, 6), (7, 7)])
def test_maps_that_are_only_2_byte_aligned(offsets, rdf, gpu_runtime):
    for (N, H, W, r, C) in ((3, 5, 7, 1, 3), (2, 37, 53, 2, 7)):
        pred, truth = _maps(N, H, W, r, C, 10 + offsets[0])
        _check(rdf, pred, truth, C, r, True, lambda a: _offset_view(rdf, a, offsets[0]), lambda a: _offset_view(rdf, a, offsets[1]))


@pytest.fixture(scope="module")
def live_like():
    pred, truth = _maps(8, 480, 848, 1, 7, 6, background=0.85)
    assert 0.8 < np.mean((truth == 0) & (pred == 65535)) < 0.9
    return pred, truth, snp.score_counts(pred, truth, 7), snp.score_per_image(pred, truth)


@pytest.mark.gpu
def test_live_like_batch(live_like, rdf, gpu_runtime):
    import torch
    pred, truth, want, want_images = live_like
    scorer = rdf.LabelScorer(7)
    p, t = rdf.to_device(pred), rdf.to_device(truth)
    scorer.add(p, t, per_image=True)
    first = scorer.counts_cu.get()
    assert np.array_equal(first, want) and np.array_equal(scorer.result().per_image, want_images)
    assert scorer.result().worst_images(3).tolist() == np.argsort(want_images[:, 0] / want_images[:, 1], kind="stable")[:3].tolist()
    # the same inputs scored again give identical bytes; torch tensors and .cu() buffers are taken as DeviceArrays are
    scorer.reset()
    scorer.add(torch.from_numpy(pred.view(np.int16)).cuda(), torch.from_numpy(truth.view(np.int16)).cuda())
    assert scorer.counts_cu.get().tobytes() == first.tobytes() and scorer.result().per_image is None
    buf = rdf.GpuBuffer(pred.shape, np.uint16)
    buf.cu().set(pred)
    assert rdf.LabelScorer(7).add(buf, t).counts_cu.get().tobytes() == first.tobytes()
    # at labels_reduce 2 on the same truth
    sub = np.ascontiguousarray(pred[:, ::2, ::2])
    _check(rdf, sub, truth, 7, 2)


@pytest.mark.gpu
def test_a_batch_whose_workgroups_take_several_sets_in_a_row(rdf, gpu_runtime):
    """From 2 x 512 workgroups x 256 groups of eight pixels on (2.1 Mpixel) a workgroup takes consecutive sets before it strides,
    one more set for every further 1.05 Mpixel: eleven frames make it four, with and without the per-image sums."""
    pred, truth = _maps(11, 480, 848, 1, 7, 9, background=0.85)
    assert pred.size // 8 >= 4 * 512 * 256
    _check(rdf, pred, truth, 7, 1, True)
    _check(rdf, pred, truth, 7, 1, False)


@pytest.mark.gpu
def test_accumulation_reset_and_graph_replay(rdf, gpu_runtime):
    import torch
    C = 5
    a_pred, a_truth = _maps(3, 37, 53, 1, C, 20)
    b_pred, b_truth = _maps(3, 37, 53, 1, C, 21)
    wa, wb = snp.score_counts(a_pred, a_truth, C), snp.score_counts(b_pred, b_truth, C)
    scorer = rdf.LabelScorer(C)
    assert not scorer.counts_cu.get().any()
    pa, ta, pb, tb = (rdf.to_device(x) for x in (a_pred, a_truth, b_pred, b_truth))
    scorer.add(pa, ta, per_image=True).add(pb, tb, per_image=True)
    s = scorer.result()
    assert np.array_equal(scorer.counts_cu.get(), wa + wb)
    assert np.array_equal(scorer.counts_cu.get(), snp.score_counts(b_pred, b_truth, C, onto=wa))
    assert np.array_equal(s.per_image, snp.score_per_image(b_pred, b_truth, onto=snp.score_per_image(a_pred, a_truth)))
    scorer.reset()
    assert not scorer.counts_cu.get().any() and scorer.result().per_image is None and scorer.result().num_pixels == 0
    # one add captured into a graph and replayed twice adds twice
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                       # warm-up
        scorer.add(pa, ta)
    side.synchronize()
    scorer.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        scorer.add(pa, ta)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(scorer.counts_cu.get(), 2 * wa)
    del graph


def _tiny_dataset(rdf, path, n=12, h=48, w=64, classes=4, seed=0):
    """Live-like and dense depth frames whose truth is a function of the position and the depth, so a tree finds something."""
    ds_mod = _mod("dataset")
    depth = rdf.synth.frames(["live" if i % 3 else "dense" for i in range(n)], 300 + seed, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    labels = (1 + (xx * (classes - 1) // w + (depth > 4000)) % (classes - 1)).astype(np.uint16)
    labels[depth == 65535] = 0
    ds_mod.write_dataset(str(path), depth, labels, {k: [40 * k, 255 - 40 * k, 7 * k, 255] for k in range(1, classes)})
    return depth, labels


@pytest.mark.gpu
def test_train_forest_scores_the_same_on_the_device(rdf, gpu_runtime, tmp_path):
    ds_mod = _mod("dataset")
    _tiny_dataset(rdf, tmp_path / "data")
    runs = []
    for device_score in (False, True):
        log = []
        model = tmp_path / f"forest_{int(device_score)}.npy"
        forest, pct = ds_mod.train_forest(str(tmp_path / "data"), 8, 4, 64, 32, 2, 4, str(model), trees_to_try=3,
                                          log=log.append, tree_seed=11, device_score=device_score)
        runs.append((forest, pct, log, np.load(model), ds_mod.train_forest.last_score))
    host, dev = runs
    assert host[0].tobytes() == dev[0].tobytes() and host[3].tobytes() == dev[3].tobytes()
    assert _same_float(host[1], dev[1]) and host[2] == dev[2] and len(host[2]) == 4 and host[2][-1].startswith("FOREST pct.")
    assert host[4] is None
    s = dev[4]
    assert _same_float(s.pct_matching, dev[1]) and s.num_classes == 4 and s.num_pixels == 4 * 48 * 64
    assert s.per_image.shape == (4, 2) and s.per_image[:, 0].sum() == s.equal and s.labelled > 0
    # the saved model through both harnesses, the same random images
    np.random.seed(5)
    want = ds_mod.evaluate_saved_model(str(tmp_path / "forest_1.npy"), str(tmp_path / "data"), 12)
    np.random.seed(5)
    s = ds_mod.score_saved_model(str(tmp_path / "forest_1.npy"), str(tmp_path / "data"), 12)
    assert _same_float(s.pct_matching, want) and s.num_pixels == 12 * 48 * 64 and s.per_image.shape == (12, 2)


@pytest.mark.gpu
def test_score_layered_model_matches_the_oracle_composite(rdf, gpu_runtime, oracle, tmp_path):
    """The two-layer stack of smoke() at labels_reduce 2: layer 1 filtered on class 3 of layer 0, composite ids 1..4."""
    ds_mod = _mod("dataset")
    n, h, w, r = 4, 120, 212, 2
    rng = np.random.default_rng(8)
    depth = rdf.synth.frames(["live", "dense", "live", "live"], 40, h, w)
    truth = rng.integers(1, 5, (n, h, w)).astype(np.uint16)
    truth[depth == 65535] = 0
    ds_mod.write_dataset(str(tmp_path / "data"), depth, truth, {k: [50 * k, 9, 200 - k, 255] for k in range(1, 5)})
    f0, f1 = rdf.synth.forest(2, 6, 4, "trained", 20), rdf.synth.forest(3, 7, 3, "trained", 30)
    np.save(tmp_path / "layer0.npy", f0)
    np.save(tmp_path / "layer1.npy", f1)
    cfg = {"layers": [{"model": "layer0.npy"}, {"model": "layer1.npy", "filter_model": 0, "filter_model_class": 3}],
           "conditions": [[0, 1], [0, 2], [1, 3], [0, 3], [0, 4]], "label_colors": [[0, 0, 0, 255]] * 4}
    with open(tmp_path / "layered.json", "w") as fh:
        fh.write(json.dumps(cfg))
    np.random.seed(3)
    s = ds_mod.score_layered_model(str(tmp_path / "layered.json"), str(tmp_path / "data"), n, r, 0.5)
    np.random.seed(3)
    order = list(range(n))
    np.random.shuffle(order)                          # the images DecisionTreeDatasetConfig drew
    d, t = depth[order], truth[order]
    l0 = np.full((n, h // r, w // r), 65535, np.uint16)
    l1, comp = l0.copy(), l0.copy()
    oracle.eval_forest(d, f0, l0, r, None, None, 0.5)
    oracle.eval_forest(d, f1, l1, r, l0, 3, 0.5)
    for i in range(n):
        oracle.composite([l0[i], l1[i]], np.array(cfg["conditions"], np.int32), comp[i:i + 1])
    C = 5
    want = snp.score_counts(comp, t, C, r)
    assert s.num_classes == C and np.array_equal(s.confusion, want[:-2].reshape(C + 1, C + 1))
    assert (s.equal, s.labelled) == (int(want[-2]), int(want[-1])) and np.array_equal(s.per_image, snp.score_per_image(comp, t, r))
    assert s.confusion[1:5, 1:5].sum() > 0 and s.num_pixels == n * (h // r) * (w // r)


@pytest.mark.gpu
def test_score_layered_model_with_gates_that_reject(rdf, gpu_runtime, oracle, tmp_path):
    """score_layered_model(min_conf=...) over the layered stack of tests/posterior_cases.py at the thresholds at which both of
    its gates reject (test_posterior.test_the_gated_stack_case_meets_its_conditions): the expected composite is the
    restatement gated per layer, then the oracle's composite; without min_conf the ungated one, and another score."""
    import posterior_cases as pc
    import posterior_numpy as pn
    ds_mod = _mod("dataset")
    case = pc.layered_case()
    f0, f1, conditions, colors, frames = case
    H, W, r, scale = pc.LAYERED["H"], pc.LAYERED["W"], 2, 0.75
    assert r == pc.LAYERED["R"]
    depth = np.concatenate([frames, rdf.synth.live_frame(302, 48, W)[None, 12:12 + H]])
    n = depth.shape[0]
    rng = np.random.default_rng(21)
    truth = rng.integers(1, 8, depth.shape).astype(np.uint16)
    truth[depth == 65535] = 0
    ds_mod.write_dataset(str(tmp_path / "data"), depth, truth, {k: [30 * k, 9, 200 - k, 255] for k in range(1, 8)})
    np.save(tmp_path / "layer0.npy", f0)
    np.save(tmp_path / "layer1.npy", f1)
    cfg = {"layers": [{"model": "layer0.npy"}, {"model": "layer1.npy", "filter_model": 0, "filter_model_class": pc.LAYERED_FILTER_CLASS}],
           "conditions": conditions, "label_colors": colors}
    with open(tmp_path / "layered.json", "w") as fh:
        fh.write(json.dumps(cfg))
    np.random.seed(3)
    order = list(range(n))
    np.random.shuffle(order)                          # the images DecisionTreeDatasetConfig draws
    assert sorted(order) == [0, 1, 2] and order != [0, 1, 2]
    d, t = depth[order], truth[order]
    C = 8
    scores, wants = {}, {}
    for min_conf in (pc.LAYERED_GATE, None):
        np.random.seed(3)
        s = ds_mod.score_layered_model(str(tmp_path / "layered.json"), str(tmp_path / "data"), n, r, scale, min_conf=min_conf)
        comp = np.stack([pc.stack_answer(pn, oracle, case, d[i], min_conf, scale)["composite"] for i in range(n)])
        want = snp.score_counts(comp, t, C, r)
        assert s.num_classes == C and np.array_equal(s.confusion, want[:-2].reshape(C + 1, C + 1)), min_conf
        assert (s.equal, s.labelled) == (int(want[-2]), int(want[-1])) and np.array_equal(s.per_image, snp.score_per_image(comp, t, r))
        assert s.confusion[1:8, 1:8].sum() > 0 and s.num_pixels == n * (H // r) * (W // r)
        scores[min_conf], wants[min_conf] = s, comp
    gated, plain = scores[pc.LAYERED_GATE], scores[None]
    assert not np.array_equal(gated.confusion, plain.confusion) and gated.confusion[1:8, C].sum() > plain.confusion[1:8, C].sum()
    assert all(not np.array_equal(wants[None][i], wants[pc.LAYERED_GATE][i]) for i in range(n))      # in every image


@pytest.mark.gpu
def test_label_scorer_one_image_per_call(rdf, gpu_runtime, monkeypatch):
    """LabelScorer.add splits a batch as the evaluator does and offsets both maps and the per-image sums (8 bytes an image) by
    hand: decision_tree._PIX_LIMIT patched down to a frame and a half makes it one image per call."""
    N, H, W, r, C = 3, 37, 53, 2, 7
    pred, truth = _maps(N, H, W, r, C, 31)
    per_image = snp.score_per_image(pred, truth, r)
    assert len({tuple(row) for row in per_image.tolist()}) == N                           # three different images
    whole = rdf.LabelScorer(C).add(rdf.to_device(pred), rdf.to_device(truth), r, per_image=True)
    dt = _mod("decision_tree")
    monkeypatch.setattr(dt, "_PIX_LIMIT", H * W * 3 // 2)
    assert dt._image_chunks(N, H * W) == [(0, 1), (1, 1), (2, 1)]
    s = _check(rdf, pred, truth, C, r, per_image=True)                                    # against score_numpy
    assert np.array_equal(s.per_image, whole.result().per_image) and np.array_equal(s.confusion, whole.result().confusion)
    chunked = rdf.LabelScorer(C).add(rdf.to_device(pred), rdf.to_device(truth), r, per_image=True)
    assert chunked.counts_cu.get().tobytes() == whole.counts_cu.get().tobytes()
    assert chunked.per_image_cu.get().tobytes() == whole.per_image_cu.get().tobytes()
    _check(rdf, pred, truth, C, r, per_image=False)
