"""Pruning (rdf_labels_prune_plan / rdf_labels_prune_apply of librdf_labels.so, prune.ForestPruner, the dataset functions on top
of them) against the numpy restatement in tests/prune_numpy.py.  The CPU tests pin the restatement to a case worked by hand,
prove that the main case contains what it is meant to contain, check the restatement's properties on random forests and the C
entry points' argument checks, which launch nothing; every GPU comparison is of bytes, never within a tolerance."""
import ctypes
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import prune_cases as pc
import prune_numpy as pn
import refit_cases as rc
import refit_numpy as rn


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


REPORT = _mod("prune").REPORT           # the names ForestPruner.plan gives the eight words of rule P4


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_hand_worked_case():
    forest, counts, C = pc.hand_case()
    assert rn.dims(forest) == (1, 3, 3) and pc.HAND_COST == 1
    assert rn.reachable_nodes(forest).tolist() == [[True, True, True, True, False, False, True]]
    p = pn.plan(forest, counts, cost_per_leaf=1)
    # node 3: the slots answer class 1 (PDF 0, 1, 0) and class 2 (.2, .3, .5): 1 + 1 errors of 4 + 3 pixels; as one leaf [0, 4, 3]
    #   answers 1 and errs on 3 = 2 + 1 * (2 - 1): the tie collapses
    # node 6: both slots right (0 errors), as one leaf [0, 6, 4] it errs on 4 > 0 + 1: stays
    # node 1: left is node 3 collapsed (3 errors, one leaf), right is a slot of [0, 0, 5] whose stale PDF (0, 2, 1) answers 1: 5
    #   errors; 8 errors with 2 leaves (7 with 3 before any collapse); as one leaf [0, 4, 8] it errs on 4 <= 8 + 1: collapses
    # node 2: left is a slot of [0, 1, 1] whose PDF (NaN, .5, .5) answers 1: 1 error; right is node 6 (0 errors, 2 leaves); as one
    #   leaf [0, 7, 5] it errs on 5 > 1 + 1 * 2: stays
    # root: left node 1 collapsed (4 errors, one leaf), right node 2 (1 error, 3 leaves); the root never collapses
    assert p.sub[0].tolist() == [[0, 11, 13], [0, 4, 8], [0, 7, 5], [0, 4, 3], [0, 0, 0], [0, 0, 0], [0, 6, 4]]
    reach = [0, 1, 2, 3, 6]
    assert [p.err[0][n] for n in reach] == [5, 8, 1, 2, 0] and [p.errB[0][n] for n in reach] == [8, 7, 1, 2, 0]
    assert [p.leaves[0][n] for n in reach] == [4, 2, 3, 2, 2] and [p.leavesB[0][n] for n in reach] == [6, 3, 3, 2, 2]
    assert [bool(p.collapse[0, n]) for n in reach] == [False, True, False, True, False]
    assert p.reach_after.tolist() == [[True, False, True, False, False, False, True]]
    # leaf slots 6 -> 4, one side turned (the root's left: node 3 goes with node 1), depth 3 stays, errors 8 -> 5 of 24 pixels, 3 nodes
    assert p.report.tolist() == [6, 4, 1, 3, 8, 5, 24, 3]
    assert dict(zip(REPORT, p.report.tolist())) == dict(leaf_slots_before=6, leaf_slots_after=4, turned=1, depth=3, errors_before=8,
                                                        errors_after=5, pixels=24, nodes_after=3)
    out, cnt = pn.apply(forest, counts, p)
    want = forest.copy()
    want[0, 0, 5] = 0.
    want[0, 0, 7:10] = [0., np.float32(4) / np.float32(12), np.float32(8) / np.float32(12)]
    want[0, [1, 3, 4, 5]] = 0.
    assert np.array_equal(_bits(out), _bits(want))
    want_cnt = counts.copy()
    want_cnt[0, 0, 0] = [0, 4, 8]
    want_cnt[0, [1, 3]] = 0
    assert np.array_equal(cnt, want_cnt) and cnt.sum() == counts.sum() == 24
    # the same plan on the result collapses nothing, and its errors before are the errors after
    again = pn.plan(out, cnt, cost_per_leaf=1)
    assert again.report.tolist() == [4, 4, 0, 3, 5, 5, 24, 3]
    # without a price per leaf the tie at node 3 is none (3 > 2) and node 1 still collapses (4 <= 7)
    p0 = pn.plan(forest, counts)
    assert [bool(p0.collapse[0, n]) for n in reach] == [False, True, False, False, False] and p0.report.tolist() == [6, 4, 1, 3, 8, 5, 24, 3]
    # two levels: nodes 3 and 6 go whatever their errors (node 6 as one leaf errs on 4); node 2 then ties, 5 <= 1 + 4, and goes
    # too, as does node 1: the root's sides answer [0, 4, 8] and [0, 7, 5], 4 + 5 errors, one level.  A minimum support of 11
    # takes nodes 3 (7 pixels) and 6 (10 pixels) the same way
    p2 = pn.plan(forest, counts, 0, 0, 2)
    assert [bool(p2.collapse[0, n]) for n in reach] == [False, True, True, True, True] and p2.report.tolist() == [6, 2, 2, 1, 8, 9, 24, 1]
    assert pn.plan(forest, counts, 0, 11).report.tolist() == p2.report.tolist() == pn.plan(forest, counts, 0, 0, 1).report.tolist()


def _facts(forest, counts, params):
    """What the pruning of one case with one set of parameters contains, as a set of names."""
    T, D, C = rn.dims(forest)
    N = forest.shape[1]
    cost, min_count, max_levels = params
    p = pn.plan(forest, counts, *params)
    before, after = p.reach_before, p.reach_after
    seen = set()
    for t in range(T):
        kept_levels = set()
        for n in range(N):
            if not before[t, n]:
                continue
            j, Z = pn.level(n), pn._total(p.sub[t, n])
            by_error = pn._err_leaf(p.sub[t, n]) <= p.err[t][n] + cost * max(p.leaves[t][n] - 1, 0)
            if n and p.collapse[t, n]:
                if pn._err_leaf(p.sub[t, n]) == p.err[t][n] + cost * max(p.leaves[t][n] - 1, 0) and j < max_levels and Z >= min_count:
                    seen.add("tie")
                if not by_error and Z < min_count and j < max_levels:
                    seen.add("forced by min_count")
                if not by_error and j >= max_levels and Z >= min_count:
                    seen.add("forced by max_levels")
                a, chain = n, 1
                while a and p.collapse[t, (a - 1) // 2]:
                    a, chain = (a - 1) // 2, chain + 1
                if chain >= 3:
                    seen.add("chain of three")
                if after[t, (n - 1) // 2]:
                    a = n
                    while pn._total(p.sub[t, a]) < 1 and a:
                        a = (a - 1) // 2
                    if Z == 0 and a != n and pn._total(p.sub[t, a]) >= 1:
                        seen.add("Z == 0 takes an ancestor")
                    if pn._total(p.sub[t, a]) < 1:
                        seen.add("no ancestor has a pixel")
            if after[t, n] and j < D - 1:
                kids = [2 * n + 1 + s for s in (0, 1) if not rn.is_leaf_slot(forest[t, n], s)]
                if len(kids) == 2 and all(p.collapse[t, c] for c in kids):
                    seen.add("kept over two collapsed children")
                if any(after[t, c] for c in kids):
                    kept_levels.add(j)
            if j == D - 1 and after[t, (n - 1) // 2] and any(not rn.is_leaf_slot(forest[t, n], s) for s in (0, 1)):
                seen.add("go on at the last level under a kept node")
        if max_levels == D and kept_levels >= set(range(D - 1)):
            seen.add("a kept go on at every level")
    return seen, p


def test_main_case_meets_every_rule():
    forest, counts = pc.main_case()
    m = pc.MAIN
    T, D, C = rn.dims(forest)
    assert (T, D, C) == (m["T"], m["D"], m["C"]) and counts.shape == (T, forest.shape[1], 2, C)
    seen = set()
    for params in pc.MAIN_PARAMS:
        s, p = _facts(forest, counts, params)
        seen |= s
        assert p.report[2] > 0                              # (the case is of use: something collapses with every set)
    assert seen == {"tie", "forced by min_count", "forced by max_levels", "chain of three", "Z == 0 takes an ancestor",
                    "no ancestor has a pixel", "kept over two collapsed children", "go on at the last level under a kept node",
                    "a kept go on at every level"}, seen
    # flags and old PDFs, on reachable nodes
    reach = rn.reachable_nodes(forest)
    flags = forest[:, :, 5:7][reach]
    assert (flags == -0.5).any() and (flags == 0.5).any() and np.isnan(flags).any()
    p = pn.plan(forest, counts)
    kinds = set()
    for t, n, s in pc.reachable_leaf_slots(forest):
        pdf, cnt = forest[t, n, 7 + s * C:7 + (s + 1) * C], counts[t, n, s]
        if int(cnt.sum()) == 0:
            continue
        k = pn.argmax_e(pdf)
        if np.isnan(pdf).any():
            kinds.add("NaN")
        if not (pdf > 0).any() and not np.isnan(pdf).any():
            kinds.add("zeros")
            assert k == 0 and pn.slot_error(forest[t, n], cnt, s, C) == int(cnt.sum())
        if (pdf > 1).any() and int(cnt[k]) < int(cnt.max()):
            kinds.add("stale")                              # k* is not the class most pixels have: the error is not S - max
    assert kinds == {"NaN", "zeros", "stale"}, kinds
    # unreachable nodes with stale bytes and stale counts
    assert forest[~reach].any() and counts[~reach].any() and not counts[2].any()


@pytest.mark.parametrize("cost", [0, 1, 7])
@pytest.mark.parametrize("shape", [(2, 5, 4), (1, 7, 3)])
def test_properties_of_the_restatement(shape, cost):
    T, D, C = shape
    rng = np.random.default_rng(100 * D + cost)
    forest = rc.trained_like(T, D, C, first=200 + D, leaf_prob=0.3)
    counts = pc.random_counts(forest, rng)
    for min_count, max_levels in ((0, D), (5, D), (0, D - 2)):
        out, cnt, p = pn.prune(forest, counts, cost, min_count, max_levels)
        assert cnt.sum() == counts.sum()
        assert np.array_equal(rn.subtree_sums(out, cnt)[:, 0], p.sub[:, 0])
        assert int(p.report[6]) == int(counts.sum()) and int(p.report[3]) <= max_levels
        again = pn.plan(out, cnt, cost, min_count, max_levels)
        assert again.report[2] == 0 and again.report[0] == again.report[1] == p.report[1]
        assert again.report[4] == again.report[5] == p.report[5] and again.report[7] == p.report[7]
        assert np.array_equal(rn.reachable_nodes(out), p.reach_after)
        gone = ~p.reach_after
        assert not out[gone].any() and not cnt[gone].any() and not np.signbit(out[gone]).any()
        if min_count == 0 and max_levels == D:
            assert int(p.report[5]) <= int(p.report[4]) + cost * (int(p.report[0]) - int(p.report[1]))
        # truncation loses nothing
        small = pn.truncated(out, int(p.report[3]))
        assert np.array_equal(rn.reachable_nodes(small), p.reach_after[:, :small.shape[1]]) and not p.reach_after[:, small.shape[1]:].any()


def test_sparse_form_of_the_restatement():
    """plan(sparse=True) visits the reachable nodes only, for the forests of a million nodes that the device tests use; on the
    main case and on a random forest it gives what the plain form gives: forest bytes, counts, report, and on every reachable
    node the sums and the decisions."""
    cases = [pc.main_case() + (params,) for params in pc.MAIN_PARAMS]
    forest = rc.trained_like(2, 7, 3, first=500, leaf_prob=0.3)
    cases.append((forest, pc.random_counts(forest, np.random.default_rng(7)), (1, 2, 6)))
    for forest, counts, params in cases:
        a, b = pn.prune(forest, counts, *params), pn.prune(forest, counts, *params, sparse=True)
        reach = a[2].reach_before
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2].report.tolist() == b[2].report.tolist()
        assert np.array_equal(reach, b[2].reach_before) and np.array_equal(a[2].reach_after, b[2].reach_after)
        assert np.array_equal(a[2].collapse & reach, b[2].collapse) and np.array_equal(a[2].sub[reach], b[2].sub[reach])
        assert sorted(pn.reachable_order(forest)) == [tuple(i) for i in np.argwhere(reach).tolist()]


@pytest.mark.parametrize("cost", [0, 1, 7])
def test_errors_of_each_tree_alone_are_the_plans(cost):
    """On frames where no walk falls off: the pixels a tree alone labels wrongly (the refit's walk, then the row-E argmax of the
    slot's PDF) are errB(root) before and err(root) after."""
    rng = np.random.default_rng(cost)
    T, D, C = 2, 5, 4
    depth = rng.integers(300, 3000, (2, 11, 13)).astype(np.uint16)
    labels = rng.integers(0, C, depth.shape).astype(np.uint16)
    forest = rc.trained_like(T, D, C, first=70)
    forest[:, :, 0:4] /= 100.
    counts, totals = rn.count(depth, labels, forest, 1.5)
    assert totals[3] == 0 and totals[0] > 100
    out, cnt, p = pn.prune(forest, counts, cost)
    assert p.report[2] > 0
    for t in range(T):
        assert pn.tree_errors(depth, labels, forest[t], 1.5) == (p.errB[t][0], 0)
        assert pn.tree_errors(depth, labels, out[t], 1.5) == (p.err[t][0], 0)
    recount, _ = rn.count(depth, labels, out, 1.5)
    assert np.array_equal(recount, cnt)                    # the folded counts are what a second counting pass gives


def test_column_tree_of_the_issue():
    """Labels that depend on x >> 3 with 20 % noise under a tree that splits down to single columns: cost_per_leaf = 0 leaves the
    root and its two children, and the errors on those pixels are the planned ones."""
    depth, labels, forest = pc.column_case()
    counts, totals = rn.count(depth, labels, forest)
    assert int(rn.reachable_nodes(forest).sum()) == 31 and totals[3] == 0
    out, cnt, p = pn.prune(forest, counts, 0)
    assert p.report[1] < p.report[0] and p.report.tolist()[:4] == [32, 4, 4, 2] and p.report[7] == 3
    assert int(rn.reachable_nodes(out).sum()) == 3
    assert pn.tree_errors(depth, labels, forest[0]) == (int(p.report[4]), 0)
    assert pn.tree_errors(depth, labels, out[0]) == (int(p.report[5]), 0) and p.report[5] < p.report[4]
    again = pn.plan(out, cnt, 0)
    assert again.report[2] == 0 and again.report[0] == again.report[1] == 4 and cnt.sum() == counts.sum()


def test_rejected_arguments_launch_nothing(rdf):
    """Rejected arguments launch nothing, so they need no device; the pointers given here are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    f, c, w, r = (ctypes.c_void_p(a) for a in (0x30000, 0x40000, 0x60000, 0x50000))
    BAD, NULL = -1, -2
    plan, apply, ws = lib.rdf_labels_prune_plan, lib.rdf_labels_prune_apply, lib.rdf_labels_prune_workspace_bytes
    for shape in ((0, 4, 3), (2, 0, 3), (2, 31, 3), (2, 4, 0), (2, 4, 65536), (-1, 4, 3)):
        assert plan(f, *shape, c, 0, 0, 1, w, r, None) == BAD
        assert apply(f, *shape, c, w, None) == BAD
        assert ws(*shape) == 0
    assert plan(f, 2, 4, 3, c, 1 << 32, 0, 4, w, r, None) == BAD               # cost_per_leaf < 2^32
    assert plan(f, 2, 4, 3, c, 0, 0, 0, w, r, None) == BAD and plan(f, 2, 4, 3, c, 0, 0, 5, w, r, None) == BAD     # 1 <= max_levels <= D
    for k in range(4):
        ptrs = [f, c, w, r]
        ptrs[k] = None
        assert plan(ptrs[0], 2, 4, 3, ptrs[1], 0, 0, 4, ptrs[2], ptrs[3], None) == NULL
    for k in range(3):
        ptrs = [f, c, w]
        ptrs[k] = None
        assert apply(ptrs[0], 2, 4, 3, ptrs[1], ptrs[2], None) == NULL
    assert plan(ctypes.c_void_p(0x30002), 2, 4, 3, c, 0, 0, 4, w, r, None) == BAD
    assert plan(f, 2, 4, 3, ctypes.c_void_p(0x40004), 0, 0, 4, w, r, None) == BAD
    assert plan(f, 2, 4, 3, c, 0, 0, 4, ctypes.c_void_p(0x60004), r, None) == BAD
    assert plan(f, 2, 4, 3, c, 0, 0, 4, w, ctypes.c_void_p(0x50004), None) == BAD
    assert apply(f, 2, 4, 3, ctypes.c_void_p(0x40004), w, None) == BAD and apply(f, 2, 4, 3, c, ctypes.c_void_p(0x60004), None) == BAD
    nodes = 2 * 15                                                              # a byte, C sums and four integers per node
    assert ws(2, 4, 3) == 32 + nodes * 3 * 8 + nodes * 32 and ws(1, 1, 1) == 8 + 8 + 32
    n20 = 4 * ((1 << 20) - 1)
    assert ws(4, 20, 8) == ((n20 + 7) & ~7) + n20 * 8 * 8 + n20 * 32
    assert "ForestPruner" in rdf.__all__ and callable(rdf.ForestPruner.plan)


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _pruner(rdf, forest, counts):
    f = rdf.DecisionForest.from_numpy(forest)
    pr = rdf.ForestPruner(f)
    pr.counts.set(counts)
    return f, pr


def _check(rdf, forest, counts, params, want=None):
    """plan + apply on the device against the restatement: report, collapse decisions, forest bytes, counts."""
    out, cnt, p = pn.prune(forest, counts, *params) if want is None else want
    f, pr = _pruner(rdf, forest, counts)
    version = f.forest_cu.version
    report = pr.plan(*params)
    assert list(report.values()) == [int(v) for v in p.report], (report, p.report.tolist())
    before, collapse, after = pr.decisions()
    assert np.array_equal(before, p.reach_before) and np.array_equal(after, p.reach_after)
    assert np.array_equal(collapse, p.collapse & p.reach_before)
    assert f.forest_cu.version == version                                      # a plan writes neither
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(forest)) and np.array_equal(pr.counts.get(), counts)
    assert pr.apply() == report and f.forest_cu.version > version
    got, got_cnt = f.forest_cu.get(), pr.counts.get()
    same = _bits(got) == _bits(out)
    assert same.all(), f"{(~same).sum()} words differ; first at {np.argwhere(~same)[:5].tolist()}"
    assert np.array_equal(got_cnt, cnt), f"counts differ; first at {np.argwhere(got_cnt != cnt)[:5].tolist()}"
    return f, pr, p


@pytest.mark.gpu
def test_hand_case_on_the_device(rdf, gpu_runtime):
    forest, counts, C = pc.hand_case()
    f, pr, p = _check(rdf, forest, counts, (1, 0, 3))
    assert p.report.tolist() == [6, 4, 1, 3, 8, 5, 24, 3]
    assert pr.plan(1) == dict(zip(REPORT, [4, 4, 0, 3, 5, 5, 24, 3]))


@pytest.fixture(scope="module")
def main_ref():
    forest, counts = pc.main_case()
    ref = {params: pn.prune(forest, counts, *params) for params in pc.MAIN_PARAMS}
    forest.setflags(write=False)
    counts.setflags(write=False)
    return forest, counts, ref


@pytest.mark.gpu
@pytest.mark.parametrize("params", pc.MAIN_PARAMS, ids=str)
def test_main_case_on_the_device(params, main_ref, rdf, gpu_runtime):
    forest, counts, ref = main_ref
    _check(rdf, forest, counts, params, ref[params])


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 17])
@pytest.mark.parametrize("T,D", [(1, 1), (3, 1), (1, 2), (3, 4), (3, 11)])
def test_shapes(T, D, C, rdf, gpu_runtime):
    """(3, 11) crosses from the one workgroup's top levels (3 * 2^8 <= 1024) into the subtrees' launches, 1536 subtrees of two
    levels; D = 1 has nothing to prune, D' = 1, and its "go on" flags keep their bytes."""
    rng = np.random.default_rng(T * 100 + D * 10 + C)
    forest = rc.trained_like(T, D, C, first=300 + D, leaf_prob=0.2 if D > 4 else 0.3, min_leaf_level=min(2, D - 1))
    if D == 1:
        forest[0, 0, 5] = -1.
    counts = pc.random_counts(forest, rng)
    for params in ((0, 0, D), (3, 2, max(D - 1, 1))):
        f, pr, p = _check(rdf, forest, counts, params)
        if D == 1:
            assert p.report.tolist()[:4] == [2 * T - 1, 2 * T - 1, 0, 1] and np.array_equal(_bits(f.forest_cu.get()), _bits(forest))
    if D == 11:                                             # (the case is of use: the subtrees' launches have nodes to decide and to keep)
        assert p.reach_before[:, 511:].sum() > 64 and p.reach_after[:, 511:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("params", [(0, 0, 11), (2, 3, 9)], ids=str)
def test_subtrees_of_ten_levels(params, rdf, gpu_runtime):
    """T520/D11: level 0 alone is the one workgroup's, and the 1040 subtrees below it are ten levels deep, up to 512 nodes wide:
    several waves per level, two trips of a workgroup's 256 threads at the last one, barriers between levels that lanes of
    different waves depend on, subtrees that end at every level.  Bytes, counts, report and decisions against the restatement
    in its form that visits reachable nodes only (which test_sparse_form_of_the_restatement pins to the plain one)."""
    forest, counts = pc.deep_subtrees_case()
    want = pn.prune(forest, counts, *params, sparse=True)
    before, after = want[2].reach_before, want[2].reach_after
    # what the case is built to contain (by the restatement alone)
    last = 1023
    assert before[0, last:last + 512].sum() > 256 and before[0, last:last + 256].any() and before[0, last + 256:last + 512].any()
    assert not before[2, last:last + 256].any() and before[2, last + 256:last + 512].sum() > 64         # a first trip with no live lane
    assert not before[519, last:last + 512].any() and before[519, last + 512:].sum() > 256             # the last workgroup's subtree
    deepest = [max(pn.level(n) for n in np.nonzero(before[t])[0]) for t in (1, 40, 41)]
    assert deepest == [10, 1, 0]
    assert len({pn.level(n) for n in np.nonzero(before[1, :1023])[0] if not before[1, 2 * n + 1:2 * n + 3].any()}) >= 4
    if params[2] == 11:
        assert after[0, last:last + 512].any() and after[:, 1:].sum() > 1000                             # some subtrees stay deep
    _check(rdf, forest, counts, params, want)


@pytest.mark.gpu
def test_more_subtrees_than_one_grid_row(rdf, gpu_runtime):
    """T16385/D2: 32770 subtree workgroups, two more than the 32768 of a launch's first grid row."""
    forest, counts = pc.wide_forest_case()
    want = pn.prune(forest, counts, 0, 0, 2, sparse=True)
    assert want[2].reach_before[-3:, 1:].all() and want[2].report[2] > 0
    assert want[2].collapse[-3:, 1:].any() and not want[2].collapse[-3:, 1:].all()                      # in the second row: both answers
    _check(rdf, forest, counts, (0, 0, 2), want)


@pytest.mark.gpu
@pytest.mark.parametrize("cost", [0, 20])
def test_one_chain_in_a_deep_tree(cost, rdf, gpu_runtime):
    """(1, 12): below level 1 nothing is reachable but one root-to-leaf chain, so in every wave of the deep levels one lane is
    live next to 63 that leave, and whole waves and subtrees leave; the stale bytes beside the chain become zeros."""
    forest, counts = pc.chain_case()
    assert int(rn.reachable_nodes(forest).sum()) == 12
    f, pr, p = _check(rdf, forest, counts, (cost, 0, 12))
    assert p.report[7] == (11 if cost == 0 else 1) and p.report[3] == p.report[7]     # (at 20 a leaf the whole chain goes)
    assert not f.forest_cu.get()[0][~p.reach_after[0]].any()


@pytest.mark.gpu
def test_counts_near_2_40_and_the_largest_cost(rdf, gpu_runtime):
    """64-bit products (cost_per_leaf = 2^32 - 1 times the leaves) and the fp32 rounding of large counts: the PDFs are
    refit_numpy._pdf of the folded counts."""
    forest = rc.trained_like(2, 6, 4, first=400, leaf_prob=0.3)
    counts = pc.huge_counts(forest, np.random.default_rng(40))
    cost = (1 << 32) - 1
    f, pr, p = _check(rdf, forest, counts, (cost, 0, 6))
    assert 0 < p.report[2] and p.report[7] > 2 and int(p.report[6]) > 1 << 44  # some collapse at that price, not all
    got, cnt = f.forest_cu.get(), pr.counts.get()
    checked = 0
    for t in range(2):
        for n in np.nonzero(p.reach_after[t])[0]:
            for s in (0, 1):
                c = 2 * n + 1 + s
                if c < forest.shape[1] and not rn.is_leaf_slot(forest[t, n], s) and p.collapse[t, c]:
                    assert np.array_equal(_bits(got[t, n, 7 + s * 4:11 + s * 4]), _bits(rn._pdf(cnt[t, n, s])))
                    assert float(cnt[t, n, s].sum()) != float(np.float32(cnt[t, n, s].sum()))       # (the sum is not exact in fp32)
                    checked += 1
    assert checked == int(p.report[2])


@pytest.mark.gpu
def test_apply_uses_the_last_plan_and_a_plan_alone_writes_nothing(main_ref, rdf, gpu_runtime):
    forest, counts, ref = main_ref
    f, pr = _pruner(rdf, forest, counts)
    first, last = pc.MAIN_PARAMS[3], pc.MAIN_PARAMS[0]
    r1 = pr.plan(*first)
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(forest)) and np.array_equal(pr.counts.get(), counts)
    r2 = pr.plan(*last)
    assert r1 != r2 and list(r2.values()) == [int(v) for v in ref[last][2].report]
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(forest)) and np.array_equal(pr.counts.get(), counts)
    pr.apply()
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(ref[last][0])) and np.array_equal(pr.counts.get(), ref[last][1])
    with pytest.raises(AssertionError, match="plan first"):
        pr.apply()                                                              # the forest was written since the last plan
    # curve: a plan per cost, nothing applied
    f, pr = _pruner(rdf, forest, counts)
    costs = [0, 1, 2, 50]
    got = pr.curve(costs)
    assert [list(r.values()) for r in got] == [[int(v) for v in pn.plan(forest, counts, c).report] for c in costs]
    assert got[0]["leaf_slots_after"] >= got[1]["leaf_slots_after"] >= got[3]["leaf_slots_after"]
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(forest)) and np.array_equal(pr.counts.get(), counts)
    for bad in (dict(cost_per_leaf=-1), dict(cost_per_leaf=1 << 32), dict(min_count=-1), dict(max_levels=0), dict(max_levels=7)):
        with pytest.raises(AssertionError):
            pr.plan(**bad)


@pytest.mark.gpu
def test_rejected_arguments_leave_the_buffers_intact(main_ref, rdf, gpu_runtime):
    forest, counts, ref = main_ref
    T, D, C = rn.dims(forest)
    lib = _mod("_lib").load("labels")
    f = rdf.to_device(forest)
    c = rdf.to_device(counts)
    w = rdf.DeviceArray((int(lib.rdf_labels_prune_workspace_bytes(T, D, C)),), np.uint8).fill(0xA5)
    r = rdf.DeviceArray((8,), np.uint64).fill(np.uint64(0x5A5A5A5A5A5A5A5A))
    st = rdf.get_runtime().stream()
    calls = [lib.rdf_labels_prune_plan(f.ptr, T, D, C, c.ptr, 1 << 32, 0, D, w.ptr, r.ptr, st),
             lib.rdf_labels_prune_plan(f.ptr, T, D, C, c.ptr, 0, 0, D + 1, w.ptr, r.ptr, st),
             lib.rdf_labels_prune_plan(f.ptr, T, D, C, c.ptr, 0, 0, 0, w.ptr, r.ptr, st),
             lib.rdf_labels_prune_plan(f.ptr, T, 31, C, c.ptr, 0, 0, 1, w.ptr, r.ptr, st),
             lib.rdf_labels_prune_plan(f.ptr, T, D, C, None, 0, 0, D, w.ptr, r.ptr, st),
             lib.rdf_labels_prune_plan(f.ptr, T, D, C, c.ptr, 0, 0, D, w.ptr + 4, r.ptr, st),
             lib.rdf_labels_prune_apply(f.ptr, T, D, 0, c.ptr, w.ptr, st),
             lib.rdf_labels_prune_apply(f.ptr, T, D, C, c.ptr, None, st),
             lib.rdf_labels_prune_apply(f.ptr, T, D, C, c.ptr + 4, w.ptr, st)]
    assert calls == [-1, -1, -1, -1, -2, -1, -1, -2, -1]
    assert np.array_equal(_bits(f.get()), _bits(forest)) and np.array_equal(c.get(), counts)
    assert (w.get() == 0xA5).all() and (r.get() == np.uint64(0x5A5A5A5A5A5A5A5A)).all()


def _tree_errors_on_device(rdf, ev, forest_np, d_cu, depth, labels):
    """Per tree alone: the walked pixels that get_labels_forest on that tree labels wrongly (a walk that falls off gets label 0)."""
    C = (forest_np.shape[2] - 7) // 2
    walked = (labels > 0) & (labels < C) & (depth > 0) & (depth < 65535)
    out = []
    for t in range(forest_np.shape[0]):
        got = rdf.DeviceArray(depth.shape, np.uint16).fill(65535)
        ev.get_labels_forest(rdf.DecisionForest.from_numpy(forest_np[t][None]), d_cu, got)
        out.append(int((got.get() != labels)[walked].sum()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("use_packed", [True, False], ids=["packed", "reference_layout"])
def test_end_to_end_on_the_refit_frames(use_packed, rdf, gpu_runtime, oracle):
    """ForestPruner.add + plan + apply on the main refit frames (2 x 9 x 70, T3/D4/C5): after the automatic re-pack the
    evaluator gives the oracle's labels of the pruned forest, the truncated forest gives the same labels, and each tree's own
    errors on those frames are the report's."""
    depth, labels, forest = rc.main_case()
    counts, totals = rn.count(depth, labels, forest)
    out, cnt, p = pn.prune(forest, counts, 0)
    assert p.report[2] > 0 and totals[3] > 0
    f = rdf.DecisionForest.from_numpy(forest)
    ev = rdf.DecisionTreeEvaluator(use_packed=use_packed)
    d_cu = rdf.to_device(depth)
    before = rdf.DeviceArray(depth.shape, np.uint16).fill(65535)
    ev.get_labels_forest(f, d_cu, before)                                      # (packs the unpruned forest)
    pr = rdf.ForestPruner(f).add(d_cu, rdf.to_device(labels))
    assert np.array_equal(pr.counts.get(), counts) and pr.totals()["fell_off"] == int(totals[3])
    report = pr.plan()
    assert list(report.values()) == [int(v) for v in p.report]
    errors_before = _tree_errors_on_device(rdf, ev, forest, d_cu, depth, labels)
    pr.apply()
    pruned = f.forest_cu.get()
    assert np.array_equal(_bits(pruned), _bits(out)) and np.array_equal(pr.counts.get(), cnt)
    after = rdf.DeviceArray(depth.shape, np.uint16).fill(65535)
    ev.get_labels_forest(f, d_cu, after)
    want = np.full(depth.shape, 65535, np.uint16)
    oracle.eval_forest(depth, pruned, want)
    assert np.array_equal(after.get(), want)
    small = pr.truncated()
    assert small.max_depth == report["depth"] and np.array_equal(_bits(small.forest_cu.get()), _bits(pn.truncated(out, report["depth"])))
    again = rdf.DeviceArray(depth.shape, np.uint16).fill(65535)
    ev.get_labels_forest(small, d_cu, again)
    assert np.array_equal(again.get(), want)
    # each tree's own errors: walks fall off in tree 0 only, and a fallen walk is an error of the evaluator's (label 0) that no
    # count holds; after pruning, tree 0's errors are those of the restatement's walk over the pruned tree
    errors_after = _tree_errors_on_device(rdf, ev, pruned, d_cu, depth, labels)
    fell = [pn.tree_errors(depth, labels, forest[t])[1] for t in range(3)]
    assert fell == [int(totals[3]), 0, 0]
    for t in (1, 2):
        assert errors_before[t] == p.errB[t][0] and errors_after[t] == p.err[t][0]
    assert errors_before[0] - p.errB[0][0] == pr.totals()["fell_off"]
    assert sum(errors_before) == report["errors_before"] + pr.totals()["fell_off"]
    e0, fell0 = pn.tree_errors(depth, labels, pruned[0])
    assert errors_after[0] == e0 + fell0
    assert sum(errors_after) - errors_after[0] == report["errors_after"] - p.err[0][0]
    # the folded counts go straight into the refit
    want_refit, _ = rn.apply(out, cnt, 1, rn.KEEP)
    pr.refitter.apply(1)
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(want_refit))


def _training_frames(rdf, n, h, w, first):
    """test_refit's frames: synthetic live frames, every pixel with a depth labelled by its column and its depth."""
    depth = rdf.synth.frames(["live"] * n, first, h, w)
    labels = np.zeros((n, h, w), np.uint16)
    xx = np.mgrid[0:h, 0:w][1]
    for i in range(n):
        valid = (depth[i] != 0) & (depth[i] != 65535)
        cls = 1 + ((xx > w // 2).astype(int) + 2 * (depth[i] > 4000).astype(int)) % 3
        labels[i][valid] = cls[valid]
    return depth, labels


@pytest.mark.gpu
def test_dataset_functions(rdf, gpu_runtime, tmp_path):
    ds_mod = _mod("dataset")
    depth, labels = _training_frames(rdf, 8, 24, 32, 300)
    colors = {1: [255, 0, 0, 255], 2: [0, 255, 0, 255], 3: [0, 0, 255, 255]}
    ddir, pdir = tmp_path / "data", tmp_path / "held_out"
    ds_mod.write_dataset(str(ddir), depth, labels, colors)
    held, held_labels = depth[:3].copy(), labels[:3]
    held[held_labels > 0] += 7
    ds_mod.write_dataset(str(pdir), held, held_labels, colors)
    np.random.seed(5)
    plain, _ = ds_mod.train_forest(str(ddir), 5, 3, 32, 16, 2, 6, str(tmp_path / "plain.npy"), trees_to_try=2, log=lambda *_: None)
    lines = []
    np.random.seed(5)
    pruned, pct = ds_mod.train_forest(str(ddir), 5, 3, 32, 16, 2, 6, str(tmp_path / "pruned.npy"), trees_to_try=2, log=lines.append,
                                      prune_dir=str(pdir), prune_images=0, prune_cost=1)
    assert any(line.startswith("pruned on all images") for line in lines)
    counts, _ = rn.count(held, held_labels, plain)
    out, cnt, p = pn.prune(plain, counts, 1)
    D2 = int(p.report[3])
    assert np.array_equal(_bits(pruned), _bits(pn.truncated(out, D2))) and pruned.shape == (2, (1 << D2) - 1, 15)
    saved = np.load(tmp_path / "pruned.npy")
    assert np.array_equal(_bits(saved), _bits(pruned))
    assert rdf.DecisionForest.load(str(tmp_path / "pruned.npy")).max_depth == D2
    np.random.seed(9)
    score = ds_mod.score_saved_model(str(tmp_path / "pruned.npy"), str(pdir), 3)
    assert 0. < score.pct_matching <= 1.
    # prune_saved_model on the plain model gives the same file; untruncated, the full-depth forest
    report = ds_mod.prune_saved_model(str(tmp_path / "plain.npy"), str(pdir), 0, str(tmp_path / "again.npy"), cost_per_leaf=1)
    assert list(report.values()) == [int(v) for v in p.report]
    assert np.array_equal(_bits(np.load(tmp_path / "again.npy")), _bits(pruned))
    ds_mod.prune_saved_model(str(tmp_path / "plain.npy"), str(pdir), 3, str(tmp_path / "full.npy"), cost_per_leaf=1, truncate=False)
    assert np.array_equal(_bits(np.load(tmp_path / "full.npy")), _bits(out))
    out3, _, p3 = pn.prune(plain, counts, 0, 4, 3)
    ds_mod.prune_saved_model(str(tmp_path / "plain.npy"), str(pdir), 0, str(tmp_path / "three.npy"), min_count=4, max_levels=3)
    assert np.array_equal(_bits(np.load(tmp_path / "three.npy")), _bits(pn.truncated(out3, int(p3.report[3])))) and p3.report[3] <= 3


@pytest.mark.gpu
def test_train_forest_without_prune_dir_is_unchanged(rdf, gpu_runtime, tmp_path):
    """Without prune_dir no new code runs: the same seed saves the bytes that the commit before this one saved
    (tests/golden/train_forest_plain_v1.json), with the new arguments at their defaults as with none of them given, and no
    ForestPruner is made."""
    ds_mod = _mod("dataset")
    depth, labels = _training_frames(rdf, 8, 24, 32, 300)
    ds_mod.write_dataset(str(tmp_path / "data"), depth, labels, {1: [255, 0, 0, 255], 2: [0, 255, 0, 255], 3: [0, 0, 255, 255]})
    called = []
    real = rdf.ForestPruner.__init__
    rdf.ForestPruner.__init__ = lambda self, *a, **k: called.append(1) or real(self, *a, **k)
    try:
        np.random.seed(5)
        a, pa = ds_mod.train_forest(str(tmp_path / "data"), 5, 3, 32, 16, 2, 6, str(tmp_path / "a.npy"), trees_to_try=2, log=lambda *_: None)
        np.random.seed(5)
        b, pb = ds_mod.train_forest(str(tmp_path / "data"), 5, 3, 32, 16, 2, 6, str(tmp_path / "b.npy"), trees_to_try=2, log=lambda *_: None,
                                    prune_dir=None, prune_images=0, prune_cost=0, prune_min_count=0, prune_max_levels=None)
    finally:
        rdf.ForestPruner.__init__ = real
    assert not called and pa == pb
    assert (tmp_path / "a.npy").read_bytes() == (tmp_path / "b.npy").read_bytes() and a.shape == (2, 63, 15)
    # ... and they are the bytes that the commit before ForestPruner saved for these frames and this seed
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_forest_plain_v1.json")))
    assert list(a.shape) == golden["shape"] and hashlib.sha256(a.tobytes()).hexdigest() == golden["sha256_of_the_array_bytes"]
    assert hashlib.sha256((tmp_path / "a.npy").read_bytes()).hexdigest() == golden["sha256_of_the_saved_npy"]
