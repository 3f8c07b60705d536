"""Forest posteriors (rdf_labels_forest_posterior / rdf_labels_confidence_counts of librdf_labels.so,
DecisionTreeEvaluator.get_posteriors_forest, score.ConfidenceScorer / Calibration, LayeredDecisionForest.min_conf,
dataset.calibrate_saved_model) against the numpy restatement in tests/posterior_numpy.py.  The CPU tests pin the restatement to
a case worked by hand and its labels to the oracle's evaluator, check the C entry points' argument checks (which launch
nothing) and the host arithmetic of Calibration; every GPU comparison is bit for bit, with no pixel left out."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import posterior_cases as pc
import posterior_numpy as pn
import session_cases as sc

NO = 65535


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# the feature's two entry points in the binding table: without them nothing in this module has anything to check
POSTERIOR_ARGS = _mod("_lib").BINDINGS["labels"][1]["rdf_labels_forest_posterior"][1]
COUNTS_ARGS = _mod("_lib").BINDINGS["labels"][1]["rdf_labels_confidence_counts"][1]


@functools.lru_cache(maxsize=None)
def _ref(name):
    """A parity case and the restatement's ungated answer, computed once, shared by the tests and left unchanged."""
    depth, forest, kw, prefill = pc.parity_case(name)
    labels, conf, sums = pn.posterior(depth, forest, prefill=prefill, **kw)
    evaluated = pn.evaluated_mask(depth, kw["labels_reduce"], kw["filter_images"], kw["filter_class"])
    for a in (depth, forest, labels, conf, sums, evaluated) + (() if kw["filter_images"] is None else (kw["filter_images"],)):
        a.setflags(write=False)
    return depth, forest, kw, prefill, labels, conf, sums, evaluated


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_hand_worked_case():
    depth, forest = pc.hand_case()
    labels, conf, sums = pn.posterior(depth, forest)
    # Tree 0 (A): f = d(x + 1, y) - d(x, y) >= 50 (or off the right border: 65535 - d) ends in the one-hot leaf [0, 1, 0]; else
    # node 1: d(x, y + 1) - d(x, y) < 50 ends in [.5, .5, 0], anything else (off the bottom border included) falls off level 1.
    # Tree 1 (B): d(x - 1, y) - d(x, y) >= 50 (column 0: off the left border) adds [.25, .25, .5], else the all-zero leaf.
    # (x, y)   A                         B          sums              label  S    q      conf = floor(q * 65535)
    # (0, 0)   0, 0: [.5, .5, 0]         border     [.75, .75, .5]    0 tie  2    .375   24575  (24575.625)
    # (1, 0)   1100 - 1000: one-hot      0: zero    [0, 1, 0]         1      1    1      65535
    # (2, 0)   -100, -100: [.5, .5, 0]   -100: zero [.5, .5, 0]       0 tie  1    .5     32767  (32767.5)
    # (3, 0)   border: one-hot           100        [.25, 1.25, .5]   1      2    .625   40959  (40959.375)
    # (0, 1)   0, 0: [.5, .5, 0]         border     [.75, .75, .5]    0      2    .375   24575
    # (1, 1)   0, 1200 - 1000: falls off 0: zero    [0, 0, 0]         0      0    -      0
    # (2, 1)   0, 0 - 1000: [.5, .5, 0]  0: zero    [.5, .5, 0]       0 tie  1    .5     32767
    # (3, 1)   border: one-hot           0: zero    [0, 1, 0]         1      1    1      65535
    # (0, 2)   1200 - 1000: one-hot      border     [.25, 1.25, .5]   1      2    .625   40959
    # (1, 2)   d = 1200: floor(1000 / 1200) = 0, both probes are the pixel: 0, 0: [.5, .5, 0]; B: floor(-1000 / 1200) = -1,
    #          1000 - 1200: zero         [.5, .5, 0]       0 tie  1    .5     32767
    # (2, 2)   depth 0, (3, 2) depth 65535: skipped
    # (0, 3)   0, bottom border: falls   border     [.25, .25, .5]    2      1    .5     32767
    # (1, 3)   0, bottom border: falls   0: zero    [0, 0, 0]         0      0    -      0          likewise (2, 3)
    # (3, 3)   border: one-hot           0: zero    [0, 1, 0]         1      1    1      65535
    want_labels = [[0, 1, 0, 1], [0, 0, 0, 1], [1, 0, NO, NO], [2, 0, 0, 1]]
    want_conf = [[24575, 65535, 32767, 40959], [24575, 0, 32767, 65535], [40959, 32767, NO, NO], [32767, 0, 0, 65535]]
    assert labels.dtype == conf.dtype == np.uint16 and sums.dtype == np.float32
    assert labels[0].tolist() == want_labels and conf[0].tolist() == want_conf
    assert sums[0, :, 0, 0].tolist() == [.75, .75, .5] and sums[0, :, 0, 1].tolist() == [0., 1., 0.]       # a tie, a one-hot vote
    assert sums[0, :, 0, 2].tolist() == [.5, .5, 0.] and sums[0, :, 0, 3].tolist() == [.25, 1.25, .5]
    assert sums[0, :, 1, 1].tolist() == [0., 0., 0.] and sums[0, :, 3, 0].tolist() == [.25, .25, .5]       # the fall-off at level D - 1
    assert sums[0, :, 2, 2].tolist() == [65535.] * 3 and sums[0, :, 2, 3].tolist() == [65535.] * 3         # skipped: the pre-fill
    # the gate: exactly the pixels with conf >= min_conf are written; conf and sums do not depend on it
    g_labels, g_conf, g_sums = pn.posterior(depth, forest, min_conf=32767, prefill=7)
    assert g_labels[0].tolist() == [[7, 1, 0, 1], [7, 7, 0, 1], [1, 0, 7, 7], [2, 7, 7, 1]]
    evaluated = pn.evaluated_mask(depth)
    assert np.array_equal(g_conf[evaluated], conf[evaluated]) and np.array_equal(g_sums[0][:, evaluated[0]], sums[0][:, evaluated[0]])
    assert np.array_equal(g_labels, np.where(evaluated, pn.gate(labels, conf, 32767, evaluated, 7), 7))
    assert (g_conf[~evaluated] == 7).all() and evaluated.sum() == 14
    # labels_reduce 2 reads depth pixels (0, 0), (2, 0), (0, 2), (2, 2): the last one is the hole
    l2, c2, s2 = pn.posterior(depth, forest, labels_reduce=2)
    assert l2[0].tolist() == [[0, 0], [1, NO]] and c2[0].tolist() == [[24575, 32767], [40959, NO]]


@pytest.mark.parametrize("name", sorted(pc.PARITY))
def test_restatement_labels_equal_the_oracles(name, oracle):
    depth, forest, kw, prefill, labels, conf, sums, evaluated = _ref(name)
    want = np.full(labels.shape, prefill, np.uint16)
    oracle.eval_forest(depth, forest, want, labels_reduce=kw["labels_reduce"], filter_images=kw["filter_images"],
                       filter_class=kw["filter_class"], scale_factor=kw["scale"])
    assert np.array_equal(labels, want)
    assert np.array_equal(want != prefill, evaluated) or prefill == 0        # (label 0 is the pre-fill 0)
    assert (conf[~evaluated] == prefill).all() and (sums.transpose(0, 2, 3, 1)[~evaluated] == np.float32(prefill)).all()
    assert evaluated.any() and (name in ("w1", "single_r2") or not evaluated.all())


def test_the_cases_contain_what_they_are_meant_to():
    C = sorted({pc.PARITY[k][7] for k in pc.PARITY})
    assert C == [1, 2, 3, 4, 5, 8, 9, 16] and {pc.PARITY[k][5] for k in pc.PARITY} == {1, 2, 5}
    assert {pc.PARITY[k][6] for k in pc.PARITY} == {1, 2, 6} and {pc.PARITY[k][3] for k in pc.PARITY} == {1, 2, 3}
    assert {pc.PARITY[k][2] for k in pc.PARITY} >= {1, 63, 64, 65, 130, 131} and {pc.PARITY[k][0] for k in pc.PARITY} == {1, 3}
    depth, forest, kw, prefill, labels, conf, sums, ev = _ref("awkward")
    s = sums.transpose(0, 2, 3, 1)[ev]
    k, l = conf[ev], labels[ev]
    assert np.isnan(s).any() and np.isinf(s).any() and (s < 0).any() and (s == 0).all(axis=1).any()
    assert ((s == [-1., 0., 2.]).all(axis=1) & (k == 65535) & (l == 2)).any()          # a share of 2: the confidence clamps
    assert (np.isnan(s).any(axis=1) & (k == 0)).any() and ((s[:, 0] == np.inf) & (k == 0) & (l == 0)).any()
    assert (np.isnan(s[:, 1]) & (l == 2)).any()                                         # NaN never wins
    for name in ("w64_n3", "w130_r2", "w131_r3"):                                       # frames with background and holes
        d = _ref(name)[0]
        assert (d == 0).any() and (d == NO).any()
        assert len(np.unique(_ref(name)[5][_ref(name)[7]])) >= 5                         # confidences of several values


def test_rejected_arguments_launch_nothing(rdf):
    """Rejected arguments launch nothing, so they need no device; the pointers given here are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    d, f, fl, lo, co, so, cn = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000))
    BAD, NULL, LARGE = -1, -2, -3
    post, counts = lib.rdf_labels_forest_posterior, lib.rdf_labels_confidence_counts
    assert len(POSTERIOR_ARGS) == 17 and len(COUNTS_ARGS) == 10 and lib.rdf_labels_abi_version() == 1

    def call(depth=d, n=1, w=8, h=8, forest=f, T=2, D=4, C=3, filt=None, fclass=-1, r=1, min_conf=0, lab=lo, conf=co, sums=so):
        return post(depth, n, w, h, forest, T, D, C, filt, fclass, r, 1., min_conf, lab, conf, sums, None)
    # Q6, row 1
    for kw in (dict(T=0), dict(T=-1), dict(D=0), dict(D=31), dict(C=0), dict(C=-3), dict(r=0), dict(n=-1), dict(w=-8), dict(h=-8),
               dict(filt=fl, fclass=-2), dict(filt=fl, fclass=65536), dict(min_conf=-1), dict(min_conf=65536),
               dict(depth=ctypes.c_void_p(0x10001)), dict(filt=ctypes.c_void_p(0x30001), fclass=1), dict(lab=ctypes.c_void_p(0x40001)),
               dict(conf=ctypes.c_void_p(0x50001)), dict(forest=ctypes.c_void_p(0x20002)), dict(sums=ctypes.c_void_p(0x60002))):
        assert call(**kw) == BAD, kw
    # row 2
    assert call(C=17) == LARGE and call(C=65535) == LARGE
    assert call(n=1, w=65536, h=32768) == LARGE and call(n=32768, w=256, h=256) == LARGE
    # row 3: zero label pixels, whatever the pointers
    assert call(n=0, depth=None, forest=None, lab=None, conf=None, sums=None) == 0
    assert call(w=3, r=4) == 0 and call(h=0) == 0 and call(w=0) == 0
    # row 4
    assert call(depth=None) == NULL and call(forest=None) == NULL and call(lab=None, conf=None, sums=None) == NULL
    assert call(filt=None, fclass=3) == NULL
    # Q7
    def cnt(n=1, w=8, h=8, r=1, bins=16, pred=lo, conf=co, truth=d, out=cn):
        return counts(n, w, h, r, bins, pred, conf, truth, out, None)
    for kw in (dict(bins=0), dict(bins=1025), dict(bins=-1), dict(r=0), dict(n=-1), dict(w=-8), dict(h=-8),
               dict(pred=ctypes.c_void_p(0x40001)), dict(conf=ctypes.c_void_p(0x50001)), dict(truth=ctypes.c_void_p(0x10001)),
               dict(out=ctypes.c_void_p(0x70004))):
        assert cnt(**kw) == BAD, kw
    assert cnt(n=0, pred=None, conf=None, truth=None, out=None) == 0 and cnt(w=3, r=4) == 0
    for k in ("pred", "conf", "truth", "out"):
        assert cnt(**{k: None}) == NULL, k
    assert cnt(n=1, w=65536, h=32768) == LARGE and cnt(n=32768, w=256, h=256) == LARGE


def test_calibration_arithmetic(rdf):
    Calibration = rdf.Calibration
    #          bin 0    bin 1   bin 2     bin 3    unclassified, labelled
    counts = [8, 2,    0, 0,   10, 10,   1, 9,    5, 45]
    c = Calibration.from_counts(np.array(counts, np.uint64), 4)
    assert c.count_by_bin == [10, 0, 20, 10] and c.correct_by_bin == [2, 0, 10, 9] and (c.labelled, c.unclassified) == (45, 5)
    assert all(type(v) is int for v in c.count_by_bin + c.correct_by_bin + [c.labelled, c.unclassified])
    acc = c.accuracy_by_bin
    assert acc[0] == 2 / 10 and np.isnan(acc[1]) and acc[2] == 10 / 20 and acc[3] == 9 / 10
    # 10/40 |.2 - .125| + 20/40 |.5 - .625| + 10/40 |.9 - .875| = (6 + 20 + 2) / (2 * 4 * 40)
    assert c.ece == 28 / 320 and abs(c.ece - 0.0875) < 1e-15
    min_conf, coverage, accuracy = c.coverage_curve()
    assert min_conf.tolist() == [0, 16384, 32768, 49152]
    assert coverage.tolist() == [40 / 45, 30 / 45, 30 / 45, 10 / 45] and accuracy.tolist() == [21 / 40, 19 / 30, 19 / 30, 9 / 10]
    assert (np.diff(coverage) <= 0).all() and coverage[-1] == c.count_by_bin[-1] / c.labelled       # monotone, ends at the top bin
    assert c.min_conf_for(0.5) == 0 and c.min_conf_for(0.6) == 16384 and c.min_conf_for(0.9) == 49152
    assert c.min_conf_for(0.95) is None
    # a threshold of the curve is the smallest confidence of its bin, for bins that do not divide 65536 too
    m3 = Calibration([1, 1, 1], [0, 0, 1], 3, 0).coverage_curve()[0].tolist()
    assert m3 == [0, 21846, 43691] and [(m * 3) >> 16 for m in m3] == [0, 1, 2] and [((m - 1) * 3) >> 16 for m in m3[1:]] == [0, 1]
    # exact integers beyond 2^53
    big = Calibration.from_counts(np.array([0, (1 << 60) + 1, 3, (1 << 60) + 1], np.uint64), 1)
    assert big.count_by_bin == [(1 << 60) + 1] and big.labelled == (1 << 60) + 1
    empty = Calibration([0, 0], [0, 0], 0, 0)
    assert np.isnan(empty.ece) and np.isnan(empty.accuracy_by_bin).all() and empty.min_conf_for(0.) is None
    assert np.isnan(empty.coverage_curve()[1]).all()


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _gpu_posterior(rdf, depth, forest, kw, prefill, min_conf=0, outputs=(True, True, True)):
    """get_posteriors_forest on pre-filled outputs; returns the three maps as numpy (None for an output not asked for)."""
    n, h, w = depth.shape
    r = kw["labels_reduce"]
    C = (forest.shape[2] - 7) // 2
    lshape = (n, h // r, w // r)
    lab = rdf.DeviceArray(lshape, np.uint16).fill(prefill) if outputs[0] else None
    conf = rdf.DeviceArray(lshape, np.uint16).fill(prefill) if outputs[1] else None
    sums = rdf.DeviceArray((n, C) + lshape[1:], np.float32).fill(np.float32(prefill)) if outputs[2] else None
    filt = None if kw["filter_images"] is None else rdf.to_device(kw["filter_images"])
    ret = rdf.DecisionTreeEvaluator().get_posteriors_forest(
        rdf.DecisionForest.from_numpy(forest), rdf.to_device(depth), lab, conf, sums, labels_reduce=r, filter_images=filt,
        filter_images_class=kw["filter_class"], scale_factor=kw["scale"], min_conf=min_conf)
    assert ret is None
    return tuple(None if a is None else a.get() for a in (lab, conf, sums))


def _same(got, want, what):
    same = got == want
    assert same.all(), f"{what}: {(~same).sum()} differ; first at {np.argwhere(~same)[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(pc.PARITY))
def test_parity_with_the_restatement(name, rdf, gpu_runtime):
    depth, forest, kw, prefill, labels, conf, sums, evaluated = _ref(name)
    got_l, got_c, got_s = _gpu_posterior(rdf, depth, forest, kw, prefill)
    _same(got_l, labels, "labels")
    _same(got_c, conf, "confidence")
    _same(_bits(got_s), _bits(sums), "sums")
    # skipped pixels keep the pre-fill in all three outputs (the restatement's arrays hold it there, checked on the CPU)
    assert (got_c[~evaluated] == prefill).all() and (got_l[~evaluated] == prefill).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w63", "w64_n3", "w130_r2", "w131_r3"])
def test_ungated_labels_equal_the_evaluators(name, rdf, gpu_runtime):
    depth, forest, kw, prefill, labels, conf, sums, evaluated = _ref(name)
    got = _gpu_posterior(rdf, depth, forest, kw, prefill, outputs=(True, False, False))[0]
    filt = None if kw["filter_images"] is None else rdf.to_device(kw["filter_images"])
    for packed in (True, False):
        out = rdf.DeviceArray(labels.shape, np.uint16).fill(prefill)
        rdf.DecisionTreeEvaluator(use_packed=packed).get_labels_forest(
            rdf.DecisionForest.from_numpy(forest), rdf.to_device(depth), out, labels_reduce=kw["labels_reduce"], filter_images=filt,
            filter_images_class=kw["filter_class"], scale_factor=kw["scale"])
        _same(got, out.get(), f"use_packed={packed}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w130_r2", "awkward"])
def test_gating(name, rdf, gpu_runtime):
    depth, forest, kw, prefill, labels, conf, sums, evaluated = _ref(name)
    for min_conf in (1, 32768, 65535):
        got_l, got_c, got_s = _gpu_posterior(rdf, depth, forest, kw, prefill, min_conf)
        written = evaluated & (conf >= min_conf)
        if min_conf == 32768 or name == "awkward":                                          # some pass the gate, some do not
            assert written.any() and (evaluated & ~written).any(), min_conf
        _same(got_l, np.where(written, labels, prefill), f"labels at min_conf {min_conf}")
        _same(got_c, conf, "confidence")
        _same(_bits(got_s), _bits(sums), "sums")
    # each output alone gives the bytes it has among all three
    want = _gpu_posterior(rdf, depth, forest, kw, prefill, 32768)
    for k in range(3):
        alone = _gpu_posterior(rdf, depth, forest, kw, prefill, 32768, tuple(j == k for j in range(3)))
        assert [a is None for a in alone] == [j != k for j in range(3)]
        assert alone[k].tobytes() == want[k].tobytes(), k
    with pytest.raises(AssertionError):
        _gpu_posterior(rdf, depth, forest, kw, prefill, outputs=(False, False, False))


def _counts_maps(name, min_conf):
    """Prediction (gated, 65535 where rejected or skipped), confidence and a seeded truth for a parity case."""
    depth, forest, kw, prefill, labels, conf, sums, evaluated = _ref(name)
    C = (forest.shape[2] - 7) // 2
    pred = np.where(evaluated & (conf >= min_conf), labels, NO).astype(np.uint16)
    k = np.where(evaluated, conf, 0).astype(np.uint16)
    rng = np.random.default_rng(len(name))
    truth = rng.integers(1, C, depth.shape).astype(np.uint16)
    truth[rng.random(depth.shape) < 0.3] = 0
    r = kw["labels_reduce"]
    at = truth[:, :pred.shape[1] * r:r, :pred.shape[2] * r:r]          # (a view: half of the classified pixels are made right)
    right = evaluated & (rng.random(pred.shape) < 0.5) & (at > 0) & (pred != NO) & (pred > 0)
    at[right] = pred[right]
    return pred, k, truth, r, C


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sharp", "w130_r2"])
def test_confidence_counts(name, rdf, gpu_runtime):
    pred, conf, truth, r, C = _counts_maps(name, 20000)
    assert {"sharp": 1, "w130_r2": 2}[name] == r
    p_cu, c_cu, t_cu = rdf.to_device(pred), rdf.to_device(conf), rdf.to_device(truth)
    at = truth[:, :pred.shape[1] * r:r, :pred.shape[2] * r:r]
    for bins in (1, 16, 256, 1024):
        want = pn.confidence_counts(pred, conf, truth, r, bins)
        scorer = rdf.ConfidenceScorer(bins).add(p_cu, c_cu, t_cu, r)
        got = scorer.counts_cu.get()
        assert got.dtype == np.uint64 and np.array_equal(got, want), bins
        scorer.add(p_cu, c_cu, t_cu, r)                                   # a second call adds on top
        assert np.array_equal(scorer.counts_cu.get(), 2 * want)
        cal = scorer.reset().add(p_cu, c_cu, t_cu, r).result()
        assert cal.unclassified == int(((pred == NO) & (at > 0)).sum()) > 0 and cal.labelled == int((at > 0).sum())
        assert sum(cal.count_by_bin) == cal.labelled - cal.unclassified and cal.count_by_bin == (want[0:2 * bins:2] + want[1:2 * bins:2]).tolist()
        # the correct column is the label scorer's diagonal over the classified labelled pixels
        score = rdf.LabelScorer(C).add(p_cu, t_cu, r).result()
        assert sum(cal.correct_by_bin) == int(np.trace(score.confusion[1:C, 1:C])) > 0
        assert sum(cal.correct_by_bin) < sum(cal.count_by_bin)
    assert len([n for n in cal.count_by_bin if n]) >= 4                   # (1024 bins: the pixels are spread over several)


def _stack(rdf, case, min_conf="never"):
    f0, f1, conditions, colors, _ = case
    cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                      {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
           "conditions": conditions, "label_colors": colors}
    lf = rdf.LayeredDecisionForest(cfg, (pc.LAYERED["H"], pc.LAYERED["W"]), pc.LAYERED["R"])
    if min_conf != "never":
        lf.min_conf = min_conf
    return lf


def _run_stack(rdf, lf, frame, hand=False, scale=0.75):
    """(composite, layer 0, layer 1, colours or None) of one frame."""
    H, W, R = pc.LAYERED["H"], pc.LAYERED["W"], pc.LAYERED["R"]
    dbuf = rdf.GpuBuffer((H, W), np.uint16, frame)
    lbuf = rdf.GpuBuffer((H // R, W // R), np.uint16)
    lbuf.cu().fill(7)
    cbuf = None
    if hand:
        cbuf = rdf.GpuBuffer((H // R, W // R, 4), np.uint8)
        cbuf.cu().fill(0)
        lf.run_hand(dbuf, lbuf, scale, flip_x=True, color_image=cbuf)
    else:
        lf.run(dbuf, lbuf, scale)
    return (lbuf.cu().get(), lf.label_images[0].cu().get(), lf.label_images[1].cu().get(), None if cbuf is None else cbuf.cu().get())


@pytest.mark.gpu
def test_layered_stacks(rdf, gpu_runtime, oracle):
    case = pc.layered_case()
    f0, f1, conditions, colors, frames = case
    R = pc.LAYERED["R"]
    plain = _stack(rdf, case)
    assert plain.min_conf is None and plain.conf_images is None and plain.fused          # nothing is allocated
    unset = _stack(rdf, case, (1, 2))
    unset.min_conf = None
    ungated = _stack(rdf, case, (0, 0))
    gated = _stack(rdf, case, (40000, 20000))
    assert gated.min_conf == (40000, 20000) and gated.sibling().min_conf == (40000, 20000) and plain.sibling().min_conf is None
    assert len(gated.conf_images) == 2 and gated.conf_images[0].shape == gated.labels_dims
    before = [rdf.device_ptr(b) for b in gated.conf_images]
    for bad in ((1,), (1, 2, 3), (-1, 0), (0, 65536)):
        with pytest.raises(AssertionError):
            plain.min_conf = bad
    assert plain.min_conf is None
    some_rejected = 0
    for frame in frames:
        want = _run_stack(rdf, plain, frame)
        assert (want[1] == 3).any() and (want[2] != NO).any() and (want[0] != NO).any()      # both layers take part
        for a, b in zip(_run_stack(rdf, unset, frame), want):
            assert a is b is None or a.tobytes() == b.tobytes()
        for a, b in zip(_run_stack(rdf, ungated, frame), want):
            assert a is b is None or a.tobytes() == b.tobytes()
        want_hand = _run_stack(rdf, plain, frame, hand=True)
        assert np.array_equal(want_hand[0], want[0][:, ::-1]) and want_hand[3].any()
        for a, b in zip(_run_stack(rdf, ungated, frame, hand=True), want_hand):
            assert a.tobytes() == b.tobytes()
        # per-layer thresholds: the restatement gated per layer, then the oracle's composite
        d3 = frame[None]
        l0, c0, _ = pn.posterior(d3, f0, R, 0.75, min_conf=40000)
        l1, c1, _ = pn.posterior(d3, f1, R, 0.75, filter_images=l0, filter_class=3, min_conf=20000)
        comp = np.full(l0.shape[1:], NO, np.uint16)
        oracle.composite([l0[0], l1[0]], conditions, comp)
        got = _run_stack(rdf, gated, frame)
        assert np.array_equal(got[1], l0[0]) and np.array_equal(got[2], l1[0]) and np.array_equal(got[0], comp)
        ev0 = pn.evaluated_mask(d3, R)
        ev1 = pn.evaluated_mask(d3, R, l0, 3)
        for buf, c, ev in ((gated.conf_images[0], c0, ev0), (gated.conf_images[1], c1, ev1)):
            assert np.array_equal(buf.cu().get(), np.where(ev[0], c[0], 0))                 # (0 where nothing was evaluated)
        some_rejected += int((ev0[0] & (l0[0] == NO)).sum() > 0) + int((ev1[0] & (l1[0] == NO)).sum() > 0)
        assert not np.array_equal(got[0], want[0])                                          # the gate changed the composite
    assert some_rejected >= 2 and [rdf.device_ptr(b) for b in gated.conf_images] == before  # allocated once, not per call


@pytest.mark.gpu
def test_session_over_an_ungated_stack(rdf, gpu_runtime):
    """min_conf = (0, 0) sends both hands through the step-by-step gated path with a gate that rejects nothing: same events and
    heights, bit for bit, as the plain stack's fused path, frame by frame and in frame batches."""
    import test_session as ts
    H, W = sc.H, sc.W
    frames, intr = sc.frames()
    frames = frames[:6]
    cfg4 = sc.forest_config(rdf)

    def session(gate):
        lf = ts._stack(rdf, (H, W), cfg4)
        if gate:
            lf.min_conf = (0, 0)
        return rdf.BeatsSession(lf, (H, W), intr, num_random_guesses=4000, seed=3, max_frames=4)
    first = session(False)
    plane = first.calibrate(frames[0])
    dev = rdf.to_device(frames)
    results = {}
    for gate in (False, True):
        for mode in ("tick", "sequence", "batched"):
            s = first if (gate, mode) == (False, "tick") else session(gate)
            s.set_plane(plane)
            assert (s.right.layered_rdf.min_conf, s.left.layered_rdf.min_conf) == (((0, 0),) * 2 if gate else (None, None))
            if mode == "tick":
                for k in range(len(frames)):
                    s.tick(dev[k])
                results[gate, mode] = (s.poll(), None)
            else:
                results[gate, mode] = s.run_sequence(dev, batched=mode == "batched")
            if gate and mode == "tick":
                with pytest.raises(NotImplementedError):
                    s.right.capture(None, None, 1, False)
    ev, h = results[False, "sequence"]
    assert h.shape == (6, 10) and np.isfinite(h).sum() >= 20
    for mode in ("tick", "sequence", "batched"):
        assert results[True, mode][0] == results[False, mode][0] == ev, mode
        if mode != "tick":
            assert np.array_equal(np.ascontiguousarray(results[True, mode][1]).view(np.uint64), np.ascontiguousarray(h).view(np.uint64)), mode


@pytest.mark.gpu
def test_calibrate_saved_model(rdf, gpu_runtime, tmp_path):
    ds_mod = _mod("dataset")
    C, r, bins = 4, 2, 32
    depth = pc.live_rows(400, 4, 12, 40)
    rng = np.random.default_rng(11)
    labels = np.where((depth != 0) & (depth != NO), rng.integers(1, C, depth.shape), 0).astype(np.uint16)
    forest = pc.trained_like(2, 5, C, 90)
    ds_mod.write_dataset(str(tmp_path / "data"), depth, labels, {1: [255, 0, 0, 255], 2: [0, 255, 0, 255], 3: [0, 0, 255, 255]})
    np.save(tmp_path / "model.npy", forest)
    np.random.seed(5)
    score, cal = ds_mod.calibrate_saved_model(str(tmp_path / "model.npy"), str(tmp_path / "data"), 3, labels_reduce=r, bins=bins)
    np.random.seed(5)
    want_score = ds_mod.score_saved_model(str(tmp_path / "model.npy"), str(tmp_path / "data"), 3, labels_reduce=r)
    assert np.array_equal(score.confusion, want_score.confusion) and (score.equal, score.labelled) == (want_score.equal, want_score.labelled)
    assert np.array_equal(score.per_image, want_score.per_image) and score.labelled > 0
    np.random.seed(5)
    idx = ds_mod.DecisionTreeDatasetConfig(str(tmp_path / "data"), num_images=3, imgs_name="test").img_idxes
    pred, conf, _ = pn.posterior(depth[idx], forest, r)
    conf[~pn.evaluated_mask(depth[idx], r)] = 0
    want = pn.confidence_counts(pred, conf, labels[idx], r, bins)
    assert isinstance(cal, rdf.Calibration) and cal.bins == bins
    assert (cal.unclassified, cal.labelled) == (int(want[2 * bins]), int(want[2 * bins + 1])) and cal.labelled > cal.unclassified
    assert cal.correct_by_bin == want[1:2 * bins:2].tolist() and cal.count_by_bin == (want[0:2 * bins:2] + want[1:2 * bins:2]).tolist()
