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
    if name == "layered0":                                   # layer 0 of the layered stack on its own: both frames, no filter
        f0, _, _, _, depth = pc.layered_case()
        forest, kw, prefill = f0, dict(labels_reduce=pc.LAYERED["R"], scale=0.75, filter_images=None, filter_class=None), NO
    else:
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
    assert {pc.PARITY[k][6] for k in pc.PARITY} == {1, 2, 6, 12} and {pc.PARITY[k][3] for k in pc.PARITY} == {1, 2, 3}
    assert [k for k in pc.PARITY if pc.PARITY[k][6] == 12] == ["walk_d12"] == sorted(pc.PARITY)[-1:]    # (the others' seeds stay)
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


def test_the_deep_case_walks_the_deep_levels():
    """walk_d12: leaves from level 9 on, so every walk passes the levels at which (1 << j) - 1 + g and n * E grow; one planted
    node of level 11 says "go on" to a pixel that reaches it (the fall-off at D - 1, at depth)."""
    depth, forest, kw, prefill, labels, conf, sums, ev = _ref("walk_d12")
    T, D, C = pn.rn.dims(forest)
    assert (T, D, C) == (2, 12, 5) and kw["labels_reduce"] == 1 and kw["filter_images"] is None
    ends = pc.walk_ends(depth, forest, 1, kw["scale"])
    assert len(ends) == T * int(ev.sum()) > 300
    levels = [pc.level_of(n) for *_, n, s in ends if n is not None]
    per_level = {lv: levels.count(lv) for lv in set(levels)}
    assert min(per_level) >= 9 and len(per_level) >= 3 and all(v >= 20 for v in per_level.values()), per_level
    fell = [e for e in ends if e[4] is None]
    assert len(fell) >= 1                                                               # the plant, reached
    clean = pc.deep_forest(T, D, C, 30 + 5 * sorted(pc.PARITY).index("walk_d12"))
    changed = np.argwhere(_bits(clean) != _bits(forest))
    assert len(changed) == 1 and pc.level_of(changed[0][1]) == D - 1 and changed[0][2] in (5, 6)
    t, n, e = changed[0]
    assert forest[t, n, e] == -1. and all(f[3] == t for f in fell)
    i, y, x = fell[0][:3]                                                               # without the plant that walk ends there
    assert pn.rn.walk(depth[i], clean[t], D, x, y, kw["scale"]) == (n, e - 5)
    assert len(np.unique(conf[ev])) >= 50                                               # confidences of many values


def test_the_gated_stack_case_meets_its_conditions(oracle):
    """layered_case() at pc.LAYERED_GATE, on the CPU: layer 0's gate changes what layer 1 evaluates, layer 1's gate rejects and
    keeps, and gating per layer is not gating the result."""
    case = pc.layered_case()
    f0, f1, conditions, colors, frames = case
    t0, t1 = pc.LAYERED_GATE
    assert (t0, t1) == (50000, 30000) and pc.LAYERED_FILTER_CLASS == 3
    want = {0: (87, 18, 16, 2), 1: (85, 21, 14, 7)}
    for k, frame in enumerate(frames):
        plain, gated = pc.stack_answer(pn, oracle, case, frame), pc.stack_answer(pn, oracle, case, frame, pc.LAYERED_GATE)
        u0, u1, l0, l1 = plain["labels"] + gated["labels"]
        rejected1 = gated["evaluated"][1] & (l1 == NO)
        kept1 = gated["evaluated"][1] & (l1 != NO)
        assert (int((u0 == 3).sum()), int(gated["evaluated"][1].sum()), int(rejected1.sum()), int(kept1.sum())) == want[k]
        # some pixel whose ungated layer-0 label is the filter class is rejected by layer 0
        assert ((u0 == 3) & (l0 == NO) & gated["evaluated"][0]).any()
        # layer 1's evaluated set is a strict subset of the ungated one
        assert not (gated["evaluated"][1] & ~plain["evaluated"][1]).any() and gated["evaluated"][1].sum() < plain["evaluated"][1].sum()
        assert np.array_equal(plain["evaluated"][1], u0 == 3)
        assert rejected1.any() and kept1.any()
        assert not np.array_equal(gated["composite"], plain["composite"])
        # gating the result: the plain composite, blanked where the layer that gave the pixel its answer (layer 1 where layer 0
        # says the filter class, else layer 0) is below its own threshold.  It keeps the pixels layer 1 is sure of but layer 0
        # was not: per-layer gating never shows them to layer 1
        decided_by_1 = plain["evaluated"][1]
        low = np.where(decided_by_1, plain["conf"][1] < t1, plain["evaluated"][0] & (plain["conf"][0] < t0))
        blanked = np.where(low, NO, plain["composite"]).astype(np.uint16)
        assert not np.array_equal(gated["composite"], blanked)
        assert ((blanked != NO) & (gated["composite"] == NO)).any() and not ((blanked == NO) & (gated["composite"] != NO)).any()
        # rule Q5's boundary occurs in layer 0: 43690 = floor(2 / 3 * 65535)
        assert (plain["conf"][0][plain["evaluated"][0]] == 43690).any()


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
@pytest.mark.parametrize("name", ["w63", "w64_n3", "w130_r2", "w131_r3", "walk_d12"])
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


# a confidence that occurs in each case (np.unique of the restatement's, asserted below) on pixels whose label is not the pre-fill
BOUNDARY = {"w130_r2": 32869, "awkward": 0, "layered0": 43690}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w130_r2", "awkward", "layered0"])
def test_gating(name, rdf, gpu_runtime):
    depth, forest, kw, prefill, labels, conf, sums, evaluated = _ref(name)
    edge = BOUNDARY[name]
    on_edge = evaluated & (conf == edge) & (labels != prefill)
    assert edge in np.unique(conf[evaluated]).tolist() and on_edge.sum() >= 2 and edge < 65535
    for min_conf in (1, 32768, 65535, edge, edge + 1):
        got_l, got_c, got_s = _gpu_posterior(rdf, depth, forest, kw, prefill, min_conf)
        written = evaluated & (conf >= min_conf)
        if (min_conf in (32768, edge + 1) or name == "awkward") and min_conf > 0:           # some pass the gate, some do not
            assert written.any() and (evaluated & ~written).any(), min_conf
        _same(got_l, np.where(written, labels, prefill), f"labels at min_conf {min_conf}")
        _same(got_c, conf, "confidence")
        _same(_bits(got_s), _bits(sums), "sums")
        # rule Q5 is >=: at the confidence itself those pixels are written, one above it they keep the pre-fill
        if min_conf == edge:
            assert (got_l[on_edge] == labels[on_edge]).all() and (got_l[on_edge] != prefill).all()
        if min_conf == edge + 1:
            assert (got_l[on_edge] == prefill).all()
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
    for bins in (3, 1000, 1, 16, 256, 1024):                              # (3 and 1000: (conf * bins) >> 16 for bins that do not divide 65536)
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(pc.COUNTS_STRIDE))
def test_confidence_counts_over_more_than_one_trip(name, rdf, gpu_runtime):
    """k_confidence_counts launches at most kCountBlocks = 512 workgroups of kThreads = 256 lanes: from 512 * 256 = 131072 label
    pixels on a workgroup makes further trips, its LDS histogram and its lanes' sums carried from trip to trip."""
    pred, conf, truth, r = pc.counts_stride_maps(name)
    n_lpx, lpix = pred.size, pred.shape[1] * pred.shape[2]
    assert pc.COUNTS_GRID_PIXELS == 512 * 256 == 131072                    # kCountBlocks * kThreads of forest_posterior_hip.hip
    assert n_lpx > 131072 and n_lpx - 131072 < 4 * 256 and (n_lpx - 131072) % 64 != 0      # few workgroups return; a partial wave
    assert {"one_image": (131327, 1), "two_images": (131838, 2)}[name] == (n_lpx, r) and pred.shape[0] == r
    assert name == "one_image" or (lpix % 64 != 0 and lpix < 131072)       # a wave spans the two images
    at = truth[:, :pred.shape[1] * r:r, :pred.shape[2] * r:r].reshape(-1)
    flat_c, flat_p = conf.reshape(-1), pred.reshape(-1)
    for i in (0, 131072, n_lpx - 1):                                        # the planted pixels count, at both ends of the range
        assert at[i] != 0 and flat_p[i] != NO and {int(flat_c[i]), int(flat_c[i + 1 if i < n_lpx - 1 else i - 1])} == {0, 65535}
    assert not at[131072 + 64:131072 + 192].any() and at[131072 + 192:].any()          # two whole waves of the second trip without truth
    assert 0.65 < (at == 0).mean() < 0.75 and 0.15 < (flat_p == NO).mean() < 0.25
    p_cu, c_cu, t_cu = rdf.to_device(pred), rdf.to_device(conf), rdf.to_device(truth)
    for bins in (3, 1000, 1024):
        want = pn.confidence_counts(pred, conf, truth, r, bins)
        assert int(want[2 * bins + 1]) == int((at != 0).sum()) and want[0] and want[2 * bins - 1]     # the lowest and the highest bin
        scorer = rdf.ConfidenceScorer(bins).add(p_cu, c_cu, t_cu, r)
        got = scorer.counts_cu.get()
        assert np.array_equal(got, want), (bins, np.flatnonzero(got != want)[:8].tolist(), got[-2:], want[-2:])


def _one_image_per_call(monkeypatch, n, pix):
    """decision_tree._PIX_LIMIT patched down to a frame and a half: every chunked call then takes one image."""
    dt = _mod("decision_tree")
    monkeypatch.setattr(dt, "_PIX_LIMIT", pix * 3 // 2)
    assert dt._image_chunks(n, pix) == [(i, 1) for i in range(n)] and n >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w64_n3", "w130_r2"])
def test_posteriors_one_image_per_call(name, rdf, gpu_runtime, monkeypatch):
    """get_posteriors_forest offsets the depth, the filter and the three outputs by hand for every chunk of a batch (the
    sums by C planes of label pixels an image)."""
    depth, forest, kw, prefill, labels, conf, sums, evaluated = _ref(name)
    assert depth.shape[0] == 3 and kw["filter_images"] is not None and sums.shape[1] == {"w64_n3": 4, "w130_r2": 8}[name]
    assert all(evaluated[i].any() and not np.array_equal(labels[i], labels[(i + 1) % 3]) for i in range(3))    # every image matters
    whole = _gpu_posterior(rdf, depth, forest, kw, prefill)
    _one_image_per_call(monkeypatch, 3, depth.shape[1] * depth.shape[2])
    chunked = _gpu_posterior(rdf, depth, forest, kw, prefill)
    for got, unchunked, want, what in zip(chunked, whole, (labels, conf, sums), ("labels", "confidence", "sums")):
        assert got.tobytes() == unchunked.tobytes(), what
        _same(_bits(got) if what == "sums" else got, _bits(want) if what == "sums" else want, what)
    for k in range(3):                                                      # each output alone is offset as it is among all three
        alone = _gpu_posterior(rdf, depth, forest, kw, prefill, 0, tuple(j == k for j in range(3)))
        assert alone[k].tobytes() == whole[k].tobytes(), k


@pytest.mark.gpu
def test_confidence_counts_one_image_per_call(rdf, gpu_runtime, monkeypatch):
    pred, conf, truth, r, C = _counts_maps("w130_r2", 20000)
    assert pred.shape[0] == 3 and r == 2
    per_image = [pn.confidence_counts(pred[i:i + 1], conf[i:i + 1], truth[i:i + 1], r, 16) for i in range(3)]
    assert all(int(c[-1]) > 0 and not np.array_equal(c, per_image[0]) for c in per_image[1:])       # every image matters
    p_cu, c_cu, t_cu = rdf.to_device(pred), rdf.to_device(conf), rdf.to_device(truth)
    whole = rdf.ConfidenceScorer(16).add(p_cu, c_cu, t_cu, r).counts_cu.get()
    _one_image_per_call(monkeypatch, 3, truth.shape[1] * truth.shape[2])
    chunked = rdf.ConfidenceScorer(16).add(p_cu, c_cu, t_cu, r).counts_cu.get()
    assert np.array_equal(chunked, whole) and np.array_equal(chunked, sum(per_image))


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


FILL = 0x5A         # the colour images' pre-fill: bytes a run must leave where it writes no label in 1..7

_answers = {}


def _gated_answers(oracle):
    """stack_answer of both layered frames at pc.LAYERED_GATE, computed once, shared and left unchanged."""
    if not _answers:
        case = pc.layered_case()
        for k, frame in enumerate(case[4]):
            _answers[k] = pc.stack_answer(pn, oracle, case, frame, pc.LAYERED_GATE, prefill_colors=FILL)
            for v in _answers[k].values():
                for a in (v if isinstance(v, list) else [v]):
                    a.setflags(write=False)
    return _answers


def _check_layers(lf, want, what):
    """The stack's per-layer label images (unflipped) and conf_images against one frame's answer."""
    for i in range(2):
        _same(lf.label_images[i].cu().get(), want["labels"][i], f"{what}: layer {i} labels")
        _same(lf.conf_images[i].cu().get(), want["conf"][i], f"{what}: layer {i} confidences")


@pytest.mark.gpu
def test_gated_stack_run_and_run_hand(rdf, gpu_runtime, oracle):
    """A stack whose gates reject (layer 0's changes what layer 1 evaluates: the CPU test above) through run(), run_hand() with
    the flip and the colours, and run_hand() without either, against the restatement gated per layer and the oracle's composite."""
    case = pc.layered_case()
    H, W, R = pc.LAYERED["H"], pc.LAYERED["W"], pc.LAYERED["R"]
    gated = _stack(rdf, case, pc.LAYERED_GATE)
    dbuf, lbuf = rdf.GpuBuffer((H, W), np.uint16), rdf.GpuBuffer((H // R, W // R), np.uint16)
    cbuf = rdf.GpuBuffer((H // R, W // R, 4), np.uint8)
    for k, frame in enumerate(case[4]):
        want = _gated_answers(oracle)[k]
        assert (want["composite"] != NO).any() and not np.array_equal(want["hand"], want["composite"])
        assert (want["hand_colors"] != FILL).any() and (want["hand_colors"] == FILL).all(axis=2).any()
        dbuf.cu().set(frame)
        for mode in ("run", "hand flipped with colours", "hand", "hand with colours"):
            lbuf.cu().fill(7)
            cbuf.cu().fill(FILL)
            if mode == "run":
                gated.run(dbuf, lbuf, 0.75)
            elif mode == "hand":
                gated.run_hand(dbuf, lbuf, 0.75, flip_x=False)
            else:
                gated.run_hand(dbuf, lbuf, 0.75, flip_x="flipped" in mode, color_image=cbuf)
            flipped = "flipped" in mode
            _same(lbuf.cu().get(), want["hand"] if flipped else want["composite"], f"frame {k}, {mode}: composite")
            colours = want["hand_colors"] if flipped else want["colors"] if "colours" in mode else np.full_like(want["colors"], FILL)
            _same(cbuf.cu().get(), colours, f"frame {k}, {mode}: colours")
            _check_layers(gated, want, f"frame {k}, {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("with_colors", [True, False])
def test_gated_stack_run_hand_batch(with_colors, rdf, gpu_runtime, oracle):
    """run_hand_batch over a gated stack goes frame by frame and copies each frame's layers into batch_label_images: both
    frames in one call, then one frame in a second call on the same buffers; the stack and a sibling give the same bytes."""
    case = pc.layered_case()
    frames = case[4]
    H, W, R = pc.LAYERED["H"], pc.LAYERED["W"], pc.LAYERED["R"]
    want = _gated_answers(oracle)
    gated = _stack(rdf, case, pc.LAYERED_GATE)
    results = []
    for lf in (gated, gated.sibling()):
        assert lf.min_conf == pc.LAYERED_GATE
        depth = rdf.to_device(frames)
        labels = rdf.DeviceArray((2, H // R, W // R), np.uint16).fill(7)
        colors = rdf.DeviceArray((2, H // R, W // R, 4), np.uint8).fill(FILL) if with_colors else None
        lf.run_hand_batch(depth, labels, 0.75, flip_x=True, color_images=colors)
        got = [labels.get()] + ([colors.get()] if with_colors else []) + [b.get() for b in lf.batch_label_images]
        for k in range(2):
            _same(got[0][k], want[k]["hand"], f"frame {k}: composite")
            if with_colors:
                _same(got[1][k], want[k]["hand_colors"], f"frame {k}: colours")
            for i in range(2):
                _same(lf.batch_label_images[i].get()[k], want[k]["labels"][i], f"frame {k}: layer {i} of the batch")
        _check_layers(lf, want[1], "after the batch: the last frame")
        # one frame, the first of the two, unflipped: the buffers of the first call serve it (capacity 2 >= 1)
        before = [b.ptr for b in lf.batch_label_images]
        one = rdf.DeviceArray((1, H // R, W // R), np.uint16).fill(7)
        one_colors = rdf.DeviceArray((1, H // R, W // R, 4), np.uint8).fill(FILL) if with_colors else None
        lf.run_hand_batch(depth[0:1], one, 0.75, flip_x=False, color_images=one_colors)
        assert [b.ptr for b in lf.batch_label_images] == before and lf.batch_label_images[0].shape[0] == 2
        _same(one.get()[0], want[0]["composite"], "one frame: composite")
        if with_colors:
            _same(one_colors.get()[0], want[0]["colors"], "one frame: colours")
        for i in range(2):
            _same(lf.batch_label_images[i].get()[0], want[0]["labels"][i], f"one frame: layer {i} of the batch")
            _same(lf.batch_label_images[i].get()[1], want[1]["labels"][i], f"one frame: layer {i}, the slot it did not use")
        _check_layers(lf, want[0], "after one frame")
        got += [one.get()] + [b.get() for b in lf.batch_label_images]
        results.append(got)
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()


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


# The session's prepared depth (the hand's stencilled, flipped frame the stack is given) exists only on the device, so these
# thresholds cannot be checked on the CPU.  They were taken from the confidences seen in conf_images in one ungated run of this
# scene's six frames on an MI355X: layer 0's evaluated pixels (about 3100 a hand and frame) lay in 17262..29293 with quartiles
# 18708, 21532, 23388 (both hands alike); layer 1's (1560 to 1940) in 14822..22223 with 16055 on more than half of them and
# the upper quartile at 16739.  Each threshold sits inside its layer's range, near the median, so that both gates reject and keep
# in every frame; the test asserts on the device's own outputs what they must bring about.
SESSION_GATE = (20000, 16500)


def _session_components(rdf, gate, frames, intr, plane, restate=(), oracle=None):
    """The components of a BeatsSession called one by one over a stack with min_conf = gate (None: the plain stack): per frame
    the heights [10] and, per hand and layer, (evaluated, kept, confidences of the evaluated pixels).  For the (hand, frame)
    pairs in `restate` the prepared depth is read back and the stack's outputs are checked against the restatement."""
    import test_session as ts
    pl = _mod("pipeline")
    H, W = sc.H, sc.W
    focal, ppx, ppy = intr
    cfg4 = sc.forest_config(rdf)
    f0, f1, conditions, colors = cfg4
    fe = rdf.FrameFrontEnd((H, W), (focal, ppx, ppy), sc.PLANE_T, gauss_sigma=2.0)
    fe.set_plane(plane)
    hg = rdf.HandGrouping((H, W), sc.LEVEL, 0.06)
    lf = ts._stack(rdf, (H, W), cfg4)
    lf.min_conf = gate
    scale = W / 848
    args = ((H, W), 2, scale, 6, [50., 8., 8., 8., 8., 8., 8.], [2, 3, 4, 5, 6], (focal, focal, ppx, ppy), plane)
    right, left = pl.HandPipeline(lf, *args, depth_mm_level=sc.LEVEL), pl.HandPipeline(lf, *args, depth_mm_level=sc.LEVEL)
    assert right.layered_rdf.min_conf == left.layered_rdf.min_conf == gate and right.layered_rdf is not left.layered_rdf
    rawb, clean = rdf.GpuBuffer((H, W), np.uint16), rdf.GpuBuffer((H, W), np.uint16)
    groups = rdf.GpuBuffer((H >> sc.LEVEL, W >> sc.LEVEL), np.uint16)
    heights, seen = np.zeros((len(frames), 10)), []
    for k in range(len(frames)):
        rawb.cu().set(frames[k])
        fe.run(rawb, clean)
        hg.make_group_image(clean, groups)
        row = {}
        for hand, (pipe, g_id, flip) in enumerate(((right, 1, False), (left, 2, True))):
            heights[k, 5 * hand:5 * hand + 5] = pipe.run(clean, groups, g_id, flip, height_depth=rawb)[1]
            if gate is None:
                continue
            stack = pipe.layered_rdf
            prepared = pipe.depth_image_2.cu().get()
            labels = [b.cu().get() for b in stack.label_images]
            conf = [b.cu().get() for b in stack.conf_images]
            ev = [pn.evaluated_mask(prepared[None], 2)[0], None]
            ev[1] = ev[0] & (labels[0] == 3)
            row[hand] = [(int(ev[i].sum()), int((ev[i] & (labels[i] != NO)).sum()), conf[i][ev[i]]) for i in range(2)]
            for i in range(2):
                assert not (~ev[i] & ((labels[i] != NO) | (conf[i] != 0))).any()          # nothing outside the evaluated set
            if (hand, k) in restate:
                d3 = prepared[None]
                l0, c0, _ = pn.posterior(d3, f0, 2, scale, min_conf=gate[0])
                l1, c1, _ = pn.posterior(d3, f1, 2, scale, filter_images=l0, filter_class=3, min_conf=gate[1])
                comp = np.full(l0.shape[1:], NO, np.uint16)
                assert oracle.composite([l0[0], l1[0]], conditions, comp) == 0
                what = f"hand {hand}, frame {k}"
                _same(labels[0], l0[0], what + ": layer 0 labels")
                _same(labels[1], l1[0], what + ": layer 1 labels")
                _same(conf[0], np.where(ev[0], c0[0], 0), what + ": layer 0 confidences")
                _same(conf[1], np.where(pn.evaluated_mask(d3, 2, l0, 3)[0], c1[0], 0), what + ": layer 1 confidences")
                _same(pipe.labels_image.cu().get(), comp[:, ::-1] if flip else comp, what + ": composite")
        seen.append(row)
    return heights, seen


@pytest.mark.gpu
def test_session_over_a_stack_whose_gates_reject(rdf, gpu_runtime, oracle):
    """BeatsSession over a stack whose gates reject pixels in both layers of both hands: tick, run_sequence and
    run_sequence(batched=True) agree with each other and with the components called one by one (HandPipeline.run over a gated
    stack, the numpy state machine), bit for bit; for one frame per hand the stack's per-layer labels, conf_images and composite
    equal the restatement's on the prepared depth read back from the pipeline."""
    import test_session as ts
    from hand_state_numpy import HandStateNumpy, same_state
    H, W = sc.H, sc.W
    frames, intr = sc.frames()
    frames = frames[:6]
    cfg4 = sc.forest_config(rdf)

    def session(gate):
        lf = ts._stack(rdf, (H, W), cfg4)
        lf.min_conf = gate
        return rdf.BeatsSession(lf, (H, W), intr, num_random_guesses=4000, seed=3, max_frames=4)
    first = session(SESSION_GATE)
    plane = first.calibrate(frames[0])
    dev = rdf.to_device(frames)
    results, states = {}, {}
    for mode in ("tick", "sequence", "batched"):
        s = first if mode == "tick" else session(SESSION_GATE)
        s.set_plane(plane)
        assert s.right.layered_rdf.min_conf == s.left.layered_rdf.min_conf == SESSION_GATE
        if mode == "tick":
            for k in range(len(frames)):
                s.tick(dev[k])
            results[mode] = (s.poll(), None)
        else:
            results[mode] = s.run_sequence(dev, batched=mode == "batched")
        states[mode] = s.hand_state.state()
    plain = session(None)
    plain.set_plane(plane)
    ev_plain, h_plain = plain.run_sequence(dev)

    want_h, seen = _session_components(rdf, SESSION_GATE, frames, intr, plane, restate={(0, 2), (1, 3)}, oracle=oracle)
    model = HandStateNumpy([200., 160., 160., 160., 160.] * 2, 36 + np.arange(10), 50)
    model.z_thresh_offset, model.min_velocity[:], model.max_velocity[:] = 25., 10., 120.
    model.step(want_h)
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    for mode in ("tick", "sequence", "batched"):
        assert results[mode][0] == model.events, mode
        assert same_state(states[mode], model.state()), mode
        if mode != "tick":
            assert results[mode][1].shape == (6, 10) and np.array_equal(bits(results[mode][1]), bits(want_h)), mode
    # what the thresholds must bring about: in at least half the frames each hand has a rejected and a kept pixel in each layer
    both = [all(0 < kept < evaluated for hand in (0, 1) for evaluated, kept, _ in row[hand]) for row in seen]
    print(f"gated session: evaluated / kept per frame, hand and layer {[[(e, k) for h in (0, 1) for e, k, _ in row[h]] for row in seen]}; "
          f"finite heights per frame {np.isfinite(want_h).sum(1).tolist()}, plain {np.isfinite(h_plain).sum(1).tolist()}")
    assert sum(both) >= 3, both
    finite = np.isfinite(want_h) & np.isfinite(h_plain)
    assert (want_h[finite] != h_plain[finite]).any()                                       # the gates move a fingertip
    for hand in (want_h[:, :5], want_h[:, 5:]):
        assert (np.isfinite(hand).sum(1) >= 3).sum() >= 3
