"""Leaf refit (rdf_labels_refit_count / rdf_labels_refit_apply of librdf_labels.so, refit.LeafRefitter, the dataset functions
on top of them) against the numpy restatement in tests/refit_numpy.py.  The CPU tests pin the restatement to a case worked by
hand, pin its walk to the oracle's evaluator through digit-coded leaf ids, and check the C entry points' argument checks, which
launch nothing; every GPU comparison is bit for bit, with no pixel left out."""
import ctypes
import importlib

import numpy as np
import pytest

import refit_cases as rc
import refit_numpy as rn


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_hand_worked_case():
    depth, labels, forest, C = rc.hand_case()
    assert rn.dims(forest) == (1, 2, 3)
    counts, totals = rn.count(depth, labels, forest)
    # (x, y): (0,0) f = 0 left, then 950 - 1000 < 0 left | (1,0) 1100 - 1000 >= 50 right | (2,0) d = 1100: both offsets floor to 0,
    # f = 0 left, f = 0 right | (3,0) off the right border, right | (1,1) lands on the 0: -900 left, then 1000 - 900 right |
    # (2,1) depth 0 | (3,1) label 7 | (0,2) left, then off the bottom border, right | (2,2) 65535 - 1000 right | (3,2) depth 65535
    want = np.zeros((1, 3, 2, 3), np.uint64)
    want[0, 0, 1] = [0, 1, 2]
    want[0, 1, 0] = [0, 1, 0]
    want[0, 1, 1] = [0, 2, 1]
    assert counts.dtype == np.uint64 and np.array_equal(counts, want)
    assert totals.tolist() == [7, 1, 2, 0] and counts.sum() == 1 * 7 - 0
    # the call adds
    again, t2 = rn.count(depth, labels, forest, counts=counts.copy(), totals=totals.copy())
    assert np.array_equal(again, 2 * want) and t2.tolist() == [14, 2, 4, 0]
    # a "go on" flag at the last level: pixel (0, 0) falls off and is counted nowhere
    off = forest.copy()
    off[0, 1, 5] = -1.
    c3, t3 = rn.count(depth, labels, off)
    want3 = want.copy()
    want3[0, 1, 0] = 0
    assert np.array_equal(c3, want3) and t3.tolist() == [7, 1, 2, 1] and c3.sum() == 7 - 1

    assert rn.reachable_nodes(forest).tolist() == [[True, True, False]]
    assert rn.subtree_sums(forest, counts)[0].tolist() == [[0, 4, 3], [0, 3, 1], [0, 0, 0]]
    f32 = np.float32
    third, two3 = f32(1) / f32(3), f32(2) / f32(3)

    def pdfs(f):
        return [f[0, 0, 7:10].tolist(), f[0, 0, 10:13].tolist(), f[0, 1, 7:10].tolist(), f[0, 1, 10:13].tolist()]
    old = pdfs(forest)
    assert old == [[.5, .25, .25], [.125, .125, .75], [0., 1., 0.], [0., 0., 1.]]
    out, report = rn.apply(forest, counts, 1, rn.KEEP)
    assert pdfs(out) == [old[0], [0., third, two3], [0., 1., 0.], [0., two3, third]] and report.tolist() == [3, 0, 0, 3]
    assert np.array_equal(_bits(out[0, :, :7]), _bits(forest[0, :, :7])) and np.array_equal(_bits(out[0, 2]), _bits(forest[0, 2]))
    out, report = rn.apply(forest, counts, 2, rn.KEEP)                     # the slot with one pixel keeps its PDF
    assert pdfs(out) == [old[0], [0., third, two3], old[2], [0., two3, third]] and report.tolist() == [2, 0, 1, 3]
    out, report = rn.apply(forest, counts, 2, rn.ANCESTOR)                 # ... or takes node 1's [0, 3, 1]
    assert pdfs(out) == [old[0], [0., third, two3], [0., .75, .25], [0., two3, third]] and report.tolist() == [2, 1, 0, 3]
    out, report = rn.apply(forest, counts, 4, rn.ANCESTOR)                 # the root's slot goes up to the root: [0, 4, 3]
    assert pdfs(out) == [old[0], [0., f32(4) / f32(7), f32(3) / f32(7)], [0., .75, .25], [0., .75, .25]]
    assert report.tolist() == [0, 3, 0, 3]
    out, report = rn.apply(forest, counts, 8, rn.ANCESTOR)                 # not even the root has eight pixels
    assert np.array_equal(_bits(out), _bits(forest)) and report.tolist() == [0, 0, 3, 3]
    out, report = rn.apply(off, c3, 1, rn.KEEP)                            # a "go on" side of the last level is no leaf slot
    assert report.tolist() == [2, 0, 0, 2] and out[0, 1, 7:10].tolist() == old[2]


def test_fp32_rounding_of_large_counts():
    cnt = np.array([0, (1 << 24) + 1, 3], np.uint64)
    pdf = rn._pdf(cnt)
    assert pdf[1] == np.float32(16777216.) / np.float32(16777220.)         # 2^24 + 1 -> 2^24, the sum 2^24 + 4 is exact


def _oracle_counts(oracle, depth, labels, forest, scale):
    """The counts and the fallen-off walks as the oracle's evaluator sees them, tree by tree, through digit-coded leaf ids."""
    T, D, C = rn.dims(forest)
    N = forest.shape[1]
    counts, fell = np.zeros((T, N, 2, C), np.uint64), 0
    for t in range(T):
        maps = []
        for tree in rc.digit_trees(forest[t], C):
            out = np.full(depth.shape, 65535, np.uint16)
            oracle.eval_forest(depth, tree[None], out, scale_factor=scale)
            maps.append(out)
        counts[t], f = rc.counts_from_slots(*rc.slots_from_digits(maps, C), labels, N, C)
        fell += f
    return counts, fell


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_main_case_meets_every_rule(scale, oracle):
    """The restatement's walk against independent code (the oracle's evaluator run on digit-coded copies of each tree), on
    the case the GPU tests use; and that case contains what it is meant to contain."""
    depth, labels, forest = rc.main_case()
    m = rc.MAIN
    assert depth.shape == (m["n"], m["H"], m["W"]) and rn.dims(forest) == (m["T"], m["D"], m["C"])
    counts, totals = rn.count(depth, labels, forest, scale)
    assert all(int(v) > 0 for v in totals), totals
    assert int(counts.sum()) == m["T"] * int(totals[0]) - int(totals[3])
    assert int(totals[0] + totals[1] + totals[2]) == int((labels > 0).sum())
    got, fell = _oracle_counts(oracle, depth, labels, forest, scale)
    assert np.array_equal(got, counts) and fell == int(totals[3])
    if scale != 1.0:
        return
    # what the probes of the three roots meet
    seen = set()
    for i, y, x in zip(*np.nonzero((labels > 0) & (labels < m["C"]) & (depth > 0) & (depth < 65535))):
        d = np.float32(depth[i, y, x])
        for t in range(3):
            q = [rn.floor_i32(np.float32(forest[t, 0, k] / d)) for k in range(4)]
            for px, py in ((x + q[0], y + q[1]), (x + q[2], y + q[3])):
                seen.add("left" if px < 0 else "right" if px >= m["W"] else "top" if py < 0 else "bottom" if py >= m["H"] else "in")
                if px >= m["W"] and y + 1 < m["H"]:
                    seen.add("x overflow that would wrap into the next row")
                if i == 1 and py < 0:
                    seen.add("a probe of image 1 that would reach image 0")
                if 0 <= px < m["W"] and 0 <= py < m["H"] and depth[i, py, px] == 0:
                    seen.add("a probe on a 0")
    assert len(seen) == 8, seen
    assert np.isnan(forest[2, 1, 4]) and counts[2, 1, 1].sum() > 0 and counts[2, 1, 0].sum() == 0        # NaN goes right
    assert forest[1, 1, 5] == -0.5 and forest[1, 1, 6] == 0.5 and counts[1, 1, 1].sum() > 0 and counts[1, 1, 0].sum() == 0
    assert counts[1, 3].sum() + counts[1, 7:9].sum() > 0                                                  # -0.5 went on


@pytest.mark.parametrize("shape", [(1, 1, 3), (2, 3, 4), (1, 5, 7)])
def test_restatement_walk_on_random_forests(shape, oracle):
    T, D, C = shape
    rng = np.random.default_rng(D)
    depth = rng.integers(300, 3000, (2, 11, 13)).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.1] = 0
    depth[rng.random(depth.shape) < 0.1] = 65535
    labels = rng.integers(0, C + 1, depth.shape).astype(np.uint16)
    forest = rc.trained_like(T, D, C, first=70)
    forest[:, :, 0:4] /= 100.                              # offsets of a few pixels: most probes stay inside
    if D > 1:
        forest[0, (1 << (D - 1)) - 1:, 5] = -1.            # every left side of the last level falls off
    counts, totals = rn.count(depth, labels, forest, 1.5)
    got, fell = _oracle_counts(oracle, depth, labels, forest, 1.5)
    assert np.array_equal(got, counts) and fell == int(totals[3])
    assert int(counts.sum()) == T * int(totals[0]) - int(totals[3])


def test_rejected_arguments_launch_nothing(rdf):
    """Rejected arguments launch nothing, so they need no device; the pointers given here are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    d, l, f, c, t, w = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))
    BAD, NULL, LARGE = -1, -2, -3
    count, apply, ws = lib.rdf_labels_refit_count, lib.rdf_labels_refit_apply, lib.rdf_labels_refit_workspace_bytes
    for dims in ((-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        assert count(d, l, *dims, f, 2, 4, 3, 1., c, t, None) == BAD
    for shape in ((0, 4, 3), (2, 0, 3), (2, 31, 3), (2, 4, 0), (2, 4, 65536), (-1, 4, 3)):
        assert count(d, l, 1, 8, 8, f, *shape, 1., c, t, None) == BAD
        assert apply(f, *shape, c, 1, 0, w, t, None) == BAD
        assert ws(*shape) == 0
    for k in range(5):
        ptrs = [d, l, f, c, t]
        ptrs[k] = None
        assert count(ptrs[0], ptrs[1], 1, 8, 8, ptrs[2], 2, 4, 3, 1., ptrs[3], ptrs[4], None) == NULL
    assert count(ctypes.c_void_p(0x10001), l, 1, 8, 8, f, 2, 4, 3, 1., c, t, None) == BAD
    assert count(d, l, 1, 8, 8, f, 2, 4, 3, 1., ctypes.c_void_p(0x40004), t, None) == BAD
    assert count(d, l, 1, 65536, 32768, f, 2, 4, 3, 1., c, t, None) == LARGE
    assert count(d, l, 32768, 256, 256, f, 2, 4, 3, 1., c, t, None) == LARGE
    assert count(d, l, 1, 8, 8, f, 1, 30, 8, 1., c, t, None) == LARGE          # (2^30 - 1) * 2 * 8 slots-by-class in one tree
    assert count(None, None, 0, 8, 8, None, 2, 4, 3, 1., None, None, None) == 0   # zero pixels: a no-op
    assert apply(f, 2, 4, 3, c, 0, 0, w, t, None) == BAD                        # min_count >= 1
    assert apply(f, 2, 4, 3, c, 1, 2, w, t, None) == BAD and apply(f, 2, 4, 3, c, 1, -1, w, t, None) == BAD
    for k in range(4):
        ptrs = [f, c, w, t]
        ptrs[k] = None
        assert apply(ptrs[0], 2, 4, 3, ptrs[1], 1, 0, ptrs[2], ptrs[3], None) == NULL
    assert apply(f, 2, 4, 3, c, 1, 1, ctypes.c_void_p(0x60004), t, None) == BAD
    nodes = 2 * 15
    assert ws(2, 4, 3) == nodes * 3 * 8 + 32 and ws(1, 1, 1) == 8 + 8
    assert ws(4, 20, 8) == 4 * ((1 << 20) - 1) * 8 * 8 + ((4 * ((1 << 20) - 1) + 7) & ~7)


# ------------------------------------------------------------------ GPU ------------------------------------------------------
@pytest.fixture(scope="module")
def main_ref():
    """The main case and the restatement's answers at both scales, computed once and left unchanged."""
    depth, labels, forest = rc.main_case()
    ref = {s: rn.count(depth, labels, forest, s) for s in (1.0, 0.5)}
    for a in (depth, labels, forest):
        a.setflags(write=False)
    return depth, labels, forest, ref


def _refitter(rdf, forest):
    f = rdf.DecisionForest.from_numpy(forest)
    return f, rdf.LeafRefitter(f)


def _check_count(rdf, depth, labels, forest, scale=1.0, want=None):
    want = rn.count(depth, labels, forest, scale) if want is None else want
    f, r = _refitter(rdf, forest)
    r.add(rdf.to_device(depth), rdf.to_device(labels), scale)
    got, totals = r.counts.get(), r.totals()
    assert got.dtype == np.uint64 and got.shape == want[0].shape
    assert np.array_equal(got, want[0]), f"{(got != want[0]).sum()} counts differ; first at {np.argwhere(got != want[0])[:5].tolist()}"
    assert list(totals.values()) == [int(v) for v in want[1]]
    assert int(got.sum()) == forest.shape[0] * totals["walked"] - totals["fell_off"]
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(forest))           # counting writes nothing into the forest
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_main_case_counts(scale, main_ref, rdf, gpu_runtime):
    depth, labels, forest, ref = main_ref
    _check_count(rdf, depth, labels, forest, scale, ref[scale])


@pytest.mark.gpu
def test_counts_equal_the_evaluators_leaf_ids(main_ref, rdf, gpu_runtime):
    """The same counts from existing device code: get_labels_forest on digit-coded copies of each tree."""
    depth, labels, forest, ref = main_ref
    T, D, C = rn.dims(forest)
    N = forest.shape[1]
    ev = rdf.DecisionTreeEvaluator()
    d_cu = rdf.to_device(depth)
    got, fell = np.zeros((T, N, 2, C), np.uint64), 0
    for t in range(T):
        maps = []
        for tree in rc.digit_trees(forest[t], C):
            out = rdf.DeviceArray(depth.shape, np.uint16).fill(65535)
            ev.get_labels_forest(rdf.DecisionForest.from_numpy(tree[None]), d_cu, out)
            maps.append(out.get())
        got[t], f = rc.counts_from_slots(*rc.slots_from_digits(maps, C), labels, N, C)
        fell += f
    assert np.array_equal(got, ref[1.0][0]) and fell == int(ref[1.0][1][3])


@pytest.mark.gpu
def test_aggregation_one_key_for_a_whole_wave(rdf, gpu_runtime):
    """All 64 lanes of a wave reach one (slot, class): at the root (the LDS histogram) and at level 10 of a chain, below the
    levels the histogram holds (one atomic for the wave)."""
    depth = np.full((1, 3, 128), 1000, np.uint16)
    labels = np.full(depth.shape, 2, np.uint16)
    labels[0, 2, 64:] = 1
    for D in (1, 11):
        forest = rc.chain_tree(D, 3)[None]
        r = _check_count(rdf, depth, labels, forest)
        assert r.counts.get()[0, (1 << (D - 1)) - 1, 0].tolist() == [0, 64, 320]


@pytest.mark.gpu
@pytest.mark.parametrize("T,C", [(1, 3), (3, 6)], ids=["lds_histogram", "wave_atomics"])
def test_aggregation_64_slots_in_one_wave(T, C, rdf, gpu_runtime):
    """A full D = 7 tree that sorts by column: the 64 lanes of a wave reach 64 different leaf slots of level 6.  T1/C3 keeps
    level 6 in the LDS histogram; T3/C6 (4572 cells for seven levels) leaves it to the per-lane atomics."""
    D, W = 7, 128
    depth = np.full((1, 2, W), 1000, np.uint16)
    labels = (1 + np.arange(2 * W) % (C - 1)).astype(np.uint16).reshape(1, 2, W)
    forest = np.stack([rc.column_tree(D, C, W)] * T)
    r = _check_count(rdf, depth, labels, forest)
    per_slot = r.counts.get().sum(axis=3)
    assert (per_slot[:, 63:] == 2).all() and not per_slot[:, :63].any()        # every one of the 128 slots: its column's two pixels


@pytest.mark.gpu
def test_aggregation_six_deep_keys_of_several_lanes_each(rdf, gpu_runtime):
    """One wave (a frame of 8 x 8) with more than kAggIters = 4 distinct keys below the LDS histogram, each held by several
    lanes: column k = 0..5 carries 8 - k labelled pixels of class 1 + k % 2 and ends in its own slot of level 6 (T3/D7/C6:
    3 * 63 * 12 = 2268 cells fit in the 4096, 3 * 127 * 12 = 4572 do not).  Four keys go through one add each, the lanes of
    the other two add one each."""
    depth = np.full((1, 8, 8), 1000, np.uint16)
    labels = np.zeros(depth.shape, np.uint16)
    for k in range(6):
        labels[0, :8 - k, k] = 1 + k % 2
    forest = np.stack([rc.column_tree(7, 6, 128)] * 3)
    r = _check_count(rdf, depth, labels, forest)
    assert r.totals()["walked"] == 33
    got = r.counts.get()[0]
    cells = {(63, 0, 1): 8, (63, 1, 2): 7, (64, 0, 1): 6, (64, 1, 2): 5, (65, 0, 1): 4, (65, 1, 2): 3}
    assert {tuple(i): int(got[tuple(i)]) for i in np.argwhere(got).tolist()} == cells


@pytest.mark.gpu
@pytest.mark.parametrize("T,D", [(1, 1), (1, 4), (3, 1)])
def test_small_forests(T, D, rdf, gpu_runtime):
    rng = np.random.default_rng(T * 8 + D)
    C = 4
    depth = rng.integers(300, 1500, (1, 7, 19)).astype(np.uint16)
    labels = rng.integers(0, C, depth.shape).astype(np.uint16)
    forest = rc.trained_like(T, D, C, first=90)
    forest[:, :, 0:4] /= 200.
    _check_count(rdf, depth, labels, forest)


@pytest.mark.gpu
def test_carry_into_the_high_word(main_ref, rdf, gpu_runtime):
    depth, labels, forest, ref = main_ref
    want = ref[1.0][0].copy()
    at = np.unravel_index(int(np.argmax(want)), want.shape)
    assert want[at] >= 2
    f, r = _refitter(rdf, forest)
    pre = np.zeros_like(want)
    pre[at] = (1 << 32) - 1
    r.counts.set(pre)
    r.add(rdf.to_device(depth), rdf.to_device(labels))
    got = r.counts.get()
    assert int(got[at]) == (1 << 32) - 1 + int(want[at]) and int(got[at]) >> 32 == 1
    assert np.array_equal(got, want + pre)


@pytest.mark.gpu
def test_accumulation_and_chunking(main_ref, rdf, gpu_runtime, monkeypatch):
    depth, labels, forest, ref = main_ref
    rng = np.random.default_rng(5)
    depth_b = rng.integers(400, 1201, depth.shape).astype(np.uint16)
    labels_b = rng.integers(0, 5, depth.shape).astype(np.uint16)
    both_d, both_l = np.concatenate([depth, depth_b]), np.concatenate([labels, labels_b])
    want = rn.count(depth_b, labels_b, forest, counts=ref[1.0][0].copy(), totals=ref[1.0][1].copy())
    f, r = _refitter(rdf, forest)
    r.add(rdf.to_device(depth), rdf.to_device(labels)).add(rdf.to_device(depth_b), rdf.to_device(labels_b))
    two = r.counts.get()
    assert np.array_equal(two, want[0]) and list(r.totals().values()) == [int(v) for v in want[1]]
    r.reset()
    assert not r.counts.get().any() and not any(r.totals().values())
    d4, l4 = rdf.to_device(both_d), rdf.to_device(both_l)
    r.add(d4, l4)
    assert r.counts.get().tobytes() == two.tobytes()
    # one image per call: the per-call pixel limit patched down to a frame and a half
    dt = _mod("decision_tree")
    monkeypatch.setattr(dt, "_PIX_LIMIT", depth.shape[1] * depth.shape[2] * 3 // 2)
    assert dt._image_chunks(4, depth.shape[1] * depth.shape[2]) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    r.reset().add(d4, l4)
    assert r.counts.get().tobytes() == two.tobytes() and list(r.totals().values()) == [int(v) for v in want[1]]


def _check_apply(rdf, forest, counts, min_count, fallback):
    want, want_report = rn.apply(forest, counts, min_count, rn.ANCESTOR if fallback == "ancestor" else rn.KEEP)
    f, r = _refitter(rdf, forest)
    r.counts.set(counts)
    version = f.forest_cu.version
    report = r.apply(min_count, fallback)
    got = f.forest_cu.get()
    assert f.forest_cu.version > version
    assert list(report.values()) == [int(v) for v in want_report] and report["own"] + report["ancestor"] + report["kept"] == report["leaf_slots"]
    same = _bits(got) == _bits(want)
    assert same.all(), f"{(~same).sum()} words differ; first at {np.argwhere(~same)[:5].tolist()}"
    return got, report


@pytest.mark.gpu
def test_apply_thresholds_fallbacks_and_untouched_bytes(rdf, gpu_runtime):
    forest, counts, (t, n, s) = rc.apply_case()
    C = rc.MAIN["C"]
    S = int(counts[t, n, s].sum())
    mine = slice(7 + s * C, 7 + (s + 1) * C)
    reach = rn.reachable_nodes(forest)
    assert not reach[2, 14] and not reach.all()
    for fallback in ("keep", "ancestor"):
        for min_count in (S - 1, S, S + 1):
            got, report = _check_apply(rdf, forest, counts, min_count, fallback)
            assert np.array_equal(_bits(got[:, :, :7]), _bits(forest[:, :, :7]))          # rec[0..6], NaN threshold included
            assert np.array_equal(_bits(got[~reach]), _bits(forest[~reach]))              # unreachable nodes
            own = min_count <= S
            if own:
                assert np.array_equal(got[t, n, mine], counts[t, n, s].astype(np.float32) / np.float32(S))
            elif fallback == "keep":
                assert np.array_equal(_bits(got[t, n, mine]), _bits(forest[t, n, mine]))  # the NaN and the stale 123.25 stay
                assert np.isnan(got[t, n, mine][0]) and got[t, n, mine][1] == 123.25
            else:
                sub = rn.subtree_sums(forest, counts)
                a = n
                while int(sub[t, a].sum()) < min_count:
                    a = (a - 1) // 2
                assert np.array_equal(got[t, n, mine], sub[t, a].astype(np.float32) / np.float32(sub[t, a].sum()))
    # the nearest sufficient ancestor is further up for a larger min_count; beyond the root's sum everything is kept
    sub = rn.subtree_sums(forest, counts)
    root = int(sub[t, 0].sum())
    got, report = _check_apply(rdf, forest, counts, root, "ancestor")
    assert report["ancestor"] > 0
    top = int(sub[:, 0].sum(axis=1).max()) + 1
    got, report = _check_apply(rdf, forest, counts, top, "ancestor")
    assert np.array_equal(_bits(got), _bits(forest)) and report["own"] == report["ancestor"] == 0
    got, report = _check_apply(rdf, forest, np.zeros_like(counts), 1, "keep")             # no pixel at all: nothing changes
    assert np.array_equal(_bits(got), _bits(forest)) and report["kept"] == report["leaf_slots"]
    f, r = _refitter(rdf, forest)
    with pytest.raises(AssertionError):
        r.apply(0)
    with pytest.raises(AssertionError):
        r.apply(1, "parent")


@pytest.mark.gpu
def test_apply_rounds_large_counts_as_fp32_does(rdf, gpu_runtime):
    forest, counts, (t, n, s) = rc.apply_case()
    counts = counts.copy()
    counts[t, n, s] = [0, (1 << 24) + 1, 3, (1 << 40) + (1 << 16) + 1, 0]       # 2^24 + 1 -> 2^24; 2^40 + 2^16 + 1 rounds up to 2^40 + 2^17
    got, _ = _check_apply(rdf, forest, counts, 1, "ancestor")
    C = rc.MAIN["C"]
    den = np.float32(counts[t, n, s].sum())
    assert got[t, n, 7 + s * C + 1] == np.float32(16777216.) / den and got[t, n, 7 + s * C + 3] == np.float32((1 << 40) + (1 << 17)) / den


@pytest.mark.gpu
def test_evaluation_after_apply_uses_the_new_pdfs(main_ref, rdf, gpu_runtime, oracle):
    """get_labels_forest on the default (packed) path after apply equals the oracle on the refitted forest read back: the
    packed table was made again."""
    depth, labels, forest, ref = main_ref
    f, r = _refitter(rdf, forest)
    ev = rdf.DecisionTreeEvaluator()
    assert ev.use_packed
    d_cu = rdf.to_device(depth)
    before = rdf.DeviceArray(depth.shape, np.uint16).fill(65535)
    ev.get_labels_forest(f, d_cu, before)                                      # packs the trained PDFs
    r.add(d_cu, rdf.to_device(labels)).apply(1, "ancestor")
    after = rdf.DeviceArray(depth.shape, np.uint16).fill(65535)
    ev.get_labels_forest(f, d_cu, after)
    refitted = f.forest_cu.get()
    want = np.full(depth.shape, 65535, np.uint16)
    oracle.eval_forest(depth, refitted, want)
    assert np.array_equal(after.get(), want)
    assert not np.array_equal(before.get(), want)                              # (the refit changed some pixel's label)
    support = r.leaf_support()
    assert [lv["level"] for lv in support] == [0, 1, 2, 3]
    assert sum(lv["pixels"] for lv in support) == int(ref[1.0][0].sum())
    reach = rn.reachable_nodes(forest)
    assert sum(lv["leaf_slots"] for lv in support) == sum(rn.is_leaf_slot(forest[t, n], s) and reach[t, n]
                                                           for t in range(3) for n in range(15) for s in (0, 1))


def _training_frames(rdf, n, h, w, first):
    """test_training.make_data's frames without its two labelled pixels on missing depth: every labelled pixel has a depth."""
    depth = rdf.synth.frames(["live"] * n, first, h, w)
    labels = np.zeros((n, h, w), np.uint16)
    xx = np.mgrid[0:h, 0:w][1]
    for i in range(n):
        valid = (depth[i] != 0) & (depth[i] != 65535)
        cls = 1 + ((xx > w // 2).astype(int) + 2 * (depth[i] > 4000).astype(int)) % 3
        labels[i][valid] = cls[valid]
    return depth, labels


class _ArrayDataset:
    def __init__(self, depth, labels, n_classes):
        self.depth, self.labels, self._c = depth, labels, n_classes
        self.num_images = self.images_per_block = depth.shape[0]

    def num_classes(self):
        return self._c

    def images_shape(self):
        return self.depth.shape

    def get_depth_block_cu(self, b, arr):
        arr.set(self.depth)

    def get_labels_block_cu(self, b, arr):
        arr.set(self.labels)


@pytest.mark.gpu
def test_refit_on_the_training_frames_never_lowers_their_accuracy(rdf, gpu_runtime):
    """One tree, refitted with min_count 1 on the frames it was trained on: every leaf then answers with the most frequent
    class of the pixels that reach it, which no other answer beats, so the accuracy on those frames cannot fall."""
    D, C, P = 6, 4, 16
    depth, labels = _training_frames(rdf, 6, 40, 56, 50)
    ds = _ArrayDataset(depth, labels, C)
    trainer = rdf.DecisionTreeTrainer(6, P)
    trainer.allocate(ds, 2 * P, D)
    tree = rdf.DecisionTree(D, C)
    np.random.seed(7)
    trainer.train(ds, tree)
    forest = rdf.DecisionForest.from_numpy(tree.tree_out_cu.get()[None])
    ev, scorer = rdf.DecisionTreeEvaluator(), rdf.LabelScorer(C)
    d_cu, l_cu = rdf.to_device(depth), rdf.to_device(labels)
    out = rdf.DeviceArray(depth.shape, np.uint16)

    def accuracy():
        out.fill(65535)
        ev.get_labels_forest(forest, d_cu, out)
        return scorer.reset().add(out, l_cu).result()
    before = accuracy()
    r = rdf.LeafRefitter(forest).add(d_cu, l_cu)
    totals = r.totals()
    assert totals == {"walked": int((labels > 0).sum()), "unknown_label": 0, "no_depth": 0, "fell_off": 0}
    report = r.apply(1)
    after = accuracy()
    print(f"accuracy {before.accuracy:.6f} -> {after.accuracy:.6f}; {report}")
    correct = lambda s: int(np.trace(s.confusion[1:C, 1:C]))
    assert int(before.confusion[1:C].sum()) == int(after.confusion[1:C].sum()) == totals["walked"]
    assert correct(after) >= correct(before) and after.accuracy >= before.accuracy
    # every leaf that pixels reach now holds their class frequencies
    got, counts = forest.forest_cu.get(), r.counts.get()
    want, _ = rn.apply(tree.tree_out_cu.get()[None], counts, 1, rn.KEEP)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.gpu
def test_dataset_functions(rdf, gpu_runtime, tmp_path):
    ds_mod = _mod("dataset")
    depth, labels = _training_frames(rdf, 10, 48, 64, 300)
    colors = {1: [255, 0, 0, 255], 2: [0, 255, 0, 255], 3: [0, 0, 255, 255]}
    ddir, rdir = tmp_path / "data", tmp_path / "sensed"
    ds_mod.write_dataset(str(ddir), depth, labels, colors)
    sensed, sensed_labels = depth[:3].copy(), labels[:3]                       # "what the camera sees": another dataset
    sensed[sensed_labels > 0] += 7
    ds_mod.write_dataset(str(rdir), sensed, sensed_labels, colors)
    np.random.seed(5)
    plain, _ = ds_mod.train_forest(str(ddir), 6, 4, 32, 16, 2, 6, str(tmp_path / "plain.npy"), trees_to_try=3, log=lambda *_: None)
    lines = []
    np.random.seed(5)
    refit, pct = ds_mod.train_forest(str(ddir), 6, 4, 32, 16, 2, 6, str(tmp_path / "refit.npy"), trees_to_try=3, log=lines.append,
                                     refit_dir=str(rdir), refit_images=3)
    assert any(line.startswith("refit on 3 images") for line in lines)
    assert refit.shape == plain.shape == (2, 63, 15)
    assert np.array_equal(_bits(refit[:, :, :7]), _bits(plain[:, :, :7])) and not np.array_equal(_bits(refit), _bits(plain))
    assert np.array_equal(_bits(np.load(tmp_path / "refit.npy")), _bits(refit))
    # refit_saved_model on the plain model and all three images of the same directory gives the same forest (the order in
    # which the images are drawn does not matter: counts add)
    report = ds_mod.refit_saved_model(str(tmp_path / "plain.npy"), str(rdir), 3, str(tmp_path / "again.npy"))
    assert np.array_equal(_bits(np.load(tmp_path / "again.npy")), _bits(refit))
    want_counts, _ = rn.count(sensed, sensed_labels, plain)
    want, want_report = rn.apply(plain, want_counts, 1, rn.KEEP)
    assert np.array_equal(_bits(refit), _bits(want)) and list(report.values()) == [int(v) for v in want_report]
    # (0 images: the whole directory)
    report = ds_mod.refit_saved_model(str(tmp_path / "plain.npy"), str(rdir), 0, str(tmp_path / "anc.npy"), min_count=50, fallback="ancestor")
    want, want_report = rn.apply(plain, want_counts, 50, rn.ANCESTOR)
    assert np.array_equal(_bits(np.load(tmp_path / "anc.npy")), _bits(want)) and list(report.values()) == [int(v) for v in want_report]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lds_histogram", "hash_table"])
def test_counts_over_more_than_one_trip(kind, rdf, gpu_runtime):
    """k_refit_count launches at most kMaxBlocks = 1024 workgroups of kThreads = 256 lanes: from 1024 * 256 = 262144 pixels on a
    workgroup makes further trips, with its LDS histogram (T2/D4/C4: every level is in it) and its table of deep cells (a
    column tree of depth 10, whose leaf slots lie on level 9, below the nine levels the histogram holds for T1/C4) carried
    from trip to trip.  One frame of 513 x 512 is 512 pixels more: workgroups 0 and 1 make a second trip, over the last row."""
    H, W, C = 513, 512, 4
    n_px = H * W
    assert n_px == 262656 > 1024 * 256 == 262144                            # kMaxBlocks * kThreads of forest_refit_hip.hip
    rng = np.random.default_rng(77)
    labelled = rng.random(n_px) < 0.02
    labelled[[0, 262143, 262144, 262145, n_px - 1]] = True                  # the first pixel, both sides of the second trip's start, the last
    labels = np.where(labelled, rng.integers(1, C, n_px), 0).astype(np.uint16).reshape(1, H, W)
    if kind == "lds_histogram":
        forest = rc.trained_like(2, 4, C, first=120)
        forest[:, :, 0:4] *= 100.                                           # offsets of a few pixels at these depths
        depth = rng.integers(400, 1201, n_px)                               # a reading under every label; around them background and holes
        depth[~labelled & (rng.random(n_px) < 0.3)] = 65535
        depth[~labelled & (rng.random(n_px) < 0.05)] = 0
        depth = depth.astype(np.uint16).reshape(1, H, W)
        assert 2 * 15 * 2 * C <= 4096
    else:
        forest = rc.column_tree(10, C, 1024)[None]                          # columns 0..511: the lower half of level 9's slots
        depth = np.full((1, H, W), 1000, np.uint16)
        assert 1 * 511 * 2 * C <= 4096 < 1 * 1023 * 2 * C                   # L = 9: level 9 is not in the histogram
    assert 0.015 < labelled.mean() < 0.025 and labelled[262144:].sum() >= 5
    r = _check_count(rdf, depth, labels, forest)
    got = r.counts.get()
    assert r.totals()["walked"] == int(labelled.sum()) and r.totals()["fell_off"] == 0
    if kind == "lds_histogram":
        assert (got.sum(axis=3) > 0).sum() >= 8                             # the walks end in many slots
    if kind == "hash_table":                                                # every column's slot of level 9, nothing above it
        per_slot = got[0].sum(axis=2)
        assert not per_slot[:511].any() and (per_slot[511:511 + 256] > 0).all() and not per_slot[511 + 256:].any()
