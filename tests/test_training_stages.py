"""The tree trainer's stages, one at a time, on inputs built for their edges (tests/train_stage_cases.py): more than 64
proposals per block (a lane of k_train_pick_best scans several), more than 1024 active nodes (a thread of
k_train_next_active walks a run), counts that (float) rounds, the 0.999 cutoff at equality, gains below zero, 1 and 64
classes, a second trip of the initialisation's grid-stride loop, and proposal counts off the batch of four.

CPU: the restatement's stages (oracle/train_numpy.py) give the values the cases state by hand, the vectorised gain equals
the scalar one bit for bit, and the restatement's winner is within a derived bound of the float64 maximum.
GPU (-m gpu): every entry point through the C ABI against the restatement's stage on the same pre-filled arrays, every
output word compared as an integer -- the sentinel words that must survive included."""
import numpy as np
import pytest

import train_stage_cases as tc
from oracle import train_numpy as tn

F32 = np.float32


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def assert_same_words(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    same = words(got) == words(want)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} words differ; first at {np.argwhere(~same)[:5].tolist()}"


def record(case, tree, i):
    return tree[(1 << case.level) - 1 + int(case.active[i])]


def is_sentinel(a):
    return words(a) == (tc.SENT32 if a.dtype.itemsize == 4 else tc.SENT64)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the builders' claims and the restatement's stages against what the cases state
# ---------------------------------------------------------------------------------------------------------------------
def test_case_list_is_complete():
    assert [c.name for c in tc.pick_cases()] == tc.PICK_IDS
    found = [len(pc) for pc, _, _ in tc.negative_gain_triples()]
    assert found == [236, 1212], found           # (C = 2 exhaustive; C = 3 in the parent's proportions) with pc sums <= 64


@pytest.mark.parametrize("name", tc.PICK_IDS)
def test_pick_best_case_holds_and_vectorised_gain_equals_scalar(name):
    """ls + rs = p_sum on every node (block_gains asserts it), the outputs start as sentinels, and the gain over
    (node, proposal) in float32 numpy array operations equals the scalar _gini_gain bit for bit -- as do the records."""
    case = tc.pick_case(name)
    assert is_sentinel(case.tree).all() and is_sentinel(case.next_counts).all()
    inside, pc, lc, rc = tc.children(case)
    assert (lc + rc == pc[:, None, :]).all()
    vec, scalar = tn.block_gains(pc, lc, rc, True), tn.block_gains(pc, lc, rc, False)
    assert_same_words(vec, scalar, "gains")
    if name != "many_nodes":                     # (its 72100 scalar gains take seconds: once, above)
        for a, b, what in zip(tc.run_pick_best(case, vectorised=True), tc.run_pick_best(case, vectorised=False),
                              ("tree", "next_counts", "best_gain")):
            assert_same_words(a, b, what)


@pytest.mark.parametrize("name", tc.PICK_IDS)
def test_restatement_winner_is_the_float64_maximum_within_the_bound(name, capsys):
    """Independent of the fp32 expression: the Gini gain in float64 from the integer counts.  The restatement's winner j*
    must satisfy g64[j*] >= max(g64) - 2 (12 C + 15) 2^-24 (tc.gain_eps: derived, not measured)."""
    case = tc.pick_case(name)
    _, pc, lc, rc = tc.children(case)
    g32, g64 = tn.block_gains(pc, lc, rc), tc.gains_f64(pc, lc, rc)
    assert np.isfinite(g64).all()
    winners = np.array([tn.first_best(row)[1] for row in g32])
    margin = g64.max(axis=1) - g64[np.arange(len(winners)), winners]
    with capsys.disabled():
        print(f"\n  {name}: largest max(g64) - g64[j*] = {margin.max():.3g} (eps {tc.gain_eps(case.C):.3g})", end="")
    assert (margin <= tc.gain_eps(case.C)).all(), (margin.max(), tc.gain_eps(case.C))


def test_placed_ties_name_the_stated_winners():
    case = tc.placed_ties()
    tree, _, best = tc.run_pick_best(case)
    assert [int(record(case, tree, i)[0]) for i in range(4)] == [2, 65, 3, 64] == list(case.expect["winner"])
    assert (best > 0).all()
    for i, pos in enumerate(tc.PLACED):          # the planted columns are identical and are the whole maximum
        _, pc, lc, _ = tc.children(case)
        g = tc.gains(pc, lc)[i]
        assert sorted(np.nonzero(g == g.max())[0].tolist()) == list(pos)
        assert (lc[i, list(pos)] == lc[i, pos[0]]).all()


@pytest.mark.parametrize("P", [p for p in tc.LANES_P if p > tc.WAVE])
def test_lanes_and_passes_first_node_is_won_by_the_lowest_of_a_lane_pair(P):
    """The builder's claim, read back: the first node's maximum is at a, a + 64 and in another lane; a must win."""
    for n in tc.LANES_N:
        case = tc.lanes_and_passes(P, n)
        _, pc, lc, _ = tc.children(case)
        tied = np.nonzero(tc.gains(pc, lc)[0] == tc.gains(pc, lc)[0].max())[0]
        assert len(tied) == 3 and tied[0] + tc.WAVE in tied and len(set((tied % tc.WAVE).tolist())) == 2
        tree, _, _ = tc.run_pick_best(case)
        assert int(record(case, tree, 0)[0]) == tied[0]


def test_no_split_is_a_leaf_with_the_parents_pdf_and_proposal_0():
    case = tc.no_split()
    tree, nxt, best = tc.run_pick_best(case)
    assert is_sentinel(nxt).all() and (best == 0).all()
    for i, pdf in enumerate(case.expect["pdf"]):
        rec = record(case, tree, i)
        assert np.array_equal(rec[0:5], case.props[0]) and rec[5] == 0 and rec[6] == 0
        assert rec[7:10].tolist() == list(pdf) and rec[10:13].tolist() == list(pdf)
    assert tc.NO_SPLIT_PDF == ((0.25, 0.5, 0.25), (0.5, 0.0, 0.5), (0.375, 0.5, 0.125))


def test_negative_gains_are_recorded_as_leaves():
    """-1 < gain < 0 beats the -1 of a fresh level, and `<= 0` makes the node a leaf with the parent's PDF."""
    assert len(tc.negative_gain()) == 2
    for case in tc.negative_gain():
        tree, nxt, best = tc.run_pick_best(case)
        assert ((best < 0) & (best > -1)).all() and is_sentinel(nxt).all()
        _, pc, lc, rc = tc.children(case)
        assert (tc.gains(pc, lc) < 0).all() and (lc.sum(axis=2) > 0).all() and (rc.sum(axis=2) > 0).all()
        for i in range(len(case.active)):
            rec = record(case, tree, i)
            assert rec[5] == 0 and rec[6] == 0 and not is_sentinel(rec).any()
            assert np.array_equal(rec[7:7 + case.C], rec[7 + case.C:])


def test_previous_gain_equal_or_above_leaves_the_record_alone():
    case = tc.previous_gain()
    tree, nxt, best = tc.run_pick_best(case)
    assert case.expect["untouched"] == [0, 1, 4, 5] and case.expect["written"] == [2, 3]
    for i in case.expect["untouched"]:
        assert is_sentinel(record(case, tree, i)).all() and best[i] == case.best_gain[i]
        assert is_sentinel(nxt[[2 * case.active[i], 2 * case.active[i] + 1]]).all()
    for i in case.expect["written"]:
        assert not is_sentinel(record(case, tree, i)[0:7]).any()
        assert best[i] == case.expect["block_best"][i] > case.best_gain[i]


def test_node_blocks_outside_the_window_keep_the_sentinel():
    case = tc.node_blocks()
    tree, nxt, best = tc.run_pick_best(case)
    outside = case.expect["outside"]
    assert [int(case.active[i]) for i in outside] == [0, 3, 14, 15, 24, 25, 31]
    for i in range(len(case.active)):
        rec, kids = record(case, tree, i), nxt[[2 * case.active[i], 2 * case.active[i] + 1]]
        if i in outside:
            assert is_sentinel(rec).all() and is_sentinel(kids).all() and words(best[i:i + 1])[0] == tc.SENT32
        else:
            assert not is_sentinel(rec[0:7]).any() and best[i] >= 0


@pytest.mark.parametrize("last_level", [False, True], ids=["inner", "last"])
@pytest.mark.parametrize("C", [2, 3])
def test_cutoff_classes(C, last_level):
    """[999, 1] and [1998, 2] meet 0.999f exactly, [998, 2] misses it, [0, 1000] and [1, 999, 0] name class 1: a leaf with
    a single 1.0 and the other PDF entries untouched.  A side below the cutoff gets the whole PDF on the last level, and the
    flag -1 with its counts (PDF untouched) above it."""
    case = tc.cutoff(C, last_level)
    assert (case.level == case.D - 1) == last_level
    tree, nxt, best = tc.run_pick_best(case)
    assert (best > 0).all()
    stated = {(999, 1): 0, (1998, 2): 0, (998, 2): None, (0, 1000): 1, (1, 999, 0): 1}
    assert tc.CUTOFF_CLASS == stated
    for i, (side, on_right) in enumerate(case.expect["sides"]):
        rec = record(case, tree, i)
        assert int(rec[0]) == 0
        for s, counts in ((on_right, side), (1 - on_right, tc.CUTOFF_OTHER[C])):
            cls = stated.get(counts)                                   # (the mixed other side is below the cutoff)
            pdf, child = rec[7 + s * C:7 + (s + 1) * C], int(case.active[i]) * 2 + s
            if cls is not None:
                assert rec[5 + s] == 0 and pdf[cls] == 1
                assert is_sentinel(np.delete(pdf, cls)).all() and is_sentinel(nxt[child]).all()
            elif last_level:
                assert rec[5 + s] == 0 and is_sentinel(nxt[child]).all()
                assert np.array_equal(pdf, np.array(counts, F32) / F32(sum(counts)))
            else:
                assert rec[5 + s] == -1 and is_sentinel(pdf).all() and nxt[child].tolist() == list(counts)


def test_class_limits():
    case = tc.class_limits(1)
    tree, nxt, best = tc.run_pick_best(case)
    assert (best == 0).all() and is_sentinel(nxt).all()
    for i in range(len(case.active)):
        assert record(case, tree, i).tolist() == case.props[0].tolist() + [0, 0, 1, 1]
    case = tc.class_limits(tc.MAX_CLASSES)
    assert case.tree.shape[1] == 135
    assert (tc.run_pick_best(case)[2] > 0).all()


def test_big_counts_round_as_stated():
    assert F32(np.uint64(2 ** 24 + 1)) == 2 ** 24 and F32(np.uint64(2 ** 24 + 3)) == 2 ** 24 + 4
    assert F32(np.uint64(2 ** 33 + 2 ** 9 + 1)) == 2 ** 33 + 2 ** 10 and F32(np.uint64(2 ** 33 + 2 ** 9)) == 2 ** 33
    case = tc.big_counts()
    extra = case.node_counts[case.active, 0] - np.array(tc.BIG, np.uint64)
    assert ((extra >= 1) & (extra < 40)).all()
    assert (tc.run_pick_best(case)[2] > 0).all()


@pytest.mark.parametrize("last_level", [False, True], ids=["inner", "last"])
def test_two_blocks_leave_stale_entries(last_level):
    """The second block wins on some nodes only, and where it wins it leaves entries of the first block's record behind."""
    first, second = tc.two_blocks(last_level)
    after_a = tc.run_pick_best(first)
    after_b = tc.run_pick_best(second, state=tuple(a.copy() for a in after_a))
    rewritten = [i for i in range(12) if int(record(first, after_b[0], i)[0]) != int(record(first, after_a[0], i)[0])
                 or after_b[2][i] != after_a[2][i]]
    assert 2 <= len(rewritten) <= 10 and (after_b[2] >= after_a[2]).all()
    fresh = tc.run_pick_best(second)             # the second block on untouched arrays: differs where entries are stale
    stale = [i for i in rewritten if not np.array_equal(words(record(first, after_b[0], i)), words(record(first, fresh[0], i)))]
    assert stale, "no node keeps an entry of the first block"


@pytest.mark.parametrize("n_active", tc.NEXT_N)
def test_next_active_empty_and_full_compactions(n_active):
    empty = tc.next_active_case(n_active, 0.0)
    buf, n = tc.run_next_active(empty)
    assert n[0] == 0 and (buf == tc.SENT_I32).all()
    full = tc.next_active_case(n_active, 1.0)
    buf, n = tc.run_next_active(full)
    a = full.active[:n_active].astype(np.int64)
    assert n[0] == 2 * n_active
    assert np.array_equal(buf[:2 * n_active], np.stack([2 * a, 2 * a + 1], axis=1).ravel())
    assert (buf[2 * n_active:] == tc.SENT_I32).all() and len(buf) == 2 * n_active + 8
    half, n = tc.run_next_active(tc.next_active_case(n_active, 0.5))
    assert (np.diff(half[:n[0]]) > 0).all() and (n_active < 1000 or 0.4 * n_active < n[0] / 2 < 0.6 * n_active)


@pytest.mark.parametrize("n_active", tc.NEXT_N)
def test_next_active_cases_need_the_run_loop(n_active):
    """The list walked the way the kernel's 1024 threads do, each a run of ceil(n / 1024) nodes, is the compaction; with
    runs of one node everything past node 1023 is lost, so the cases above 1024 nodes do exercise the run loop."""
    case = tc.next_active_case(n_active, 1.0)
    want = tc.run_next_active(case)
    as_kernel = tc.run_next_active(case, per=(n_active + tc.SCAN_THREADS - 1) // tc.SCAN_THREADS)
    assert np.array_equal(as_kernel[0], want[0]) and as_kernel[1] == want[1]
    runs_of_one = tc.run_next_active(case, per=1)
    assert (runs_of_one[1] != want[1]) == (n_active > tc.SCAN_THREADS)


def test_update_pixels_restatement_on_stated_pixels():
    """NaN thresholds never go left; retired pixels stay retired; a pixel goes on only where its side's flag is -1."""
    case = tc.update_pixels_case()
    out = tn.update_pixels(case.depth, case.nodes, case.tree, case.level, case.C)
    live = case.nodes >= 0
    rec = case.tree[(1 << case.level) - 1 + np.where(live, case.nodes, 0)]
    assert (out[~live] == -1).all() and 0.25 < (~live).mean() < 0.35
    nan_thr = live & np.isnan(rec[..., 4])
    assert nan_thr.sum() > 50
    assert (out[nan_thr & (rec[..., 6] == -1)] == 2 * case.nodes[nan_thr & (rec[..., 6] == -1)] + 1).all()
    assert (out[nan_thr & (rec[..., 6] == 0)] == -1).all()
    assert (out[live & (rec[..., 5] == 0) & (rec[..., 6] == 0)] == -1).all()
    both = live & (rec[..., 5] == -1) & (rec[..., 6] == -1)
    assert (out[both] >> 1 == case.nodes[both]).all() and 0.1 < (out[both] & 1).mean() < 0.9
    assert (case.depth == 0).any() and (case.depth == 65535).any() and np.isinf(rec[..., 0:4]).any()
    one = tc.update_pixels_case((1, 1, 1))
    assert tn.update_pixels(one.depth, one.nodes, one.tree, one.level, one.C).ravel()[0] in (-1, 10, 11)


def test_init_and_right_counts_expectations():
    case = tc.init_case(257, 4)
    nodes, root = tc.init_expected(case)
    assert nodes[0] == -1 and nodes[-1] == 0 and (root[4:] == tc.SENT64).all()
    assert int((root[:4] - case.root[:4]).sum()) == int(((case.labels > 0) & (case.labels < 4)).sum()) and root[0] == case.root[0]
    rc = tc.right_counts_case()
    want = tc.right_counts_expected(rc)
    changed = np.nonzero((want != rc.counts).any(axis=(0, 2)))[0] + rc.start
    inside = [int(p) for p in rc.active if 16 <= p <= 47]
    assert changed.tolist() == [2 * p + 1 for p in inside] and len(inside) < len(rc.active)


@pytest.mark.parametrize("P", tc.COUNT_P)
def test_plain_count_counts_every_live_pixel_once_per_proposal(P):
    case = tc.count_case(P)
    full = tc.plain_counts(P, tc.COUNT_WINDOWS[0])
    assert full.shape == (P, 16, case.C) and full.sum() == P * int(case.parents.sum())
    assert np.array_equal(full[:, 0::2] + full[:, 1::2], np.broadcast_to(case.parents, (P, 8, case.C)))
    start, end, NB = tc.COUNT_WINDOWS[1]
    assert np.array_equal(tc.plain_counts(P, tc.COUNT_WINDOWS[1]), full[:, start:end])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one entry point at a time through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def device_pick_best(rdf, rt, case, state):
    """rdf_train_pick_best on device copies of `state` = (tree, next_counts, best_gain); returns them as it left them."""
    d = [rdf.to_device(a) for a in (case.active, case.node_counts, case.counts, case.props, *state)]
    rc = rt.lib.rdf_train_pick_best(len(case.active), d[0].ptr, case.P, case.D, case.NB, case.start, case.end, case.C,
                                    case.level, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, rt.stream())
    assert rc == 0
    out = tuple(a.get() for a in d[4:])
    for a, src in zip(d[:4], (case.active, case.node_counts, case.counts, case.props)):
        assert_same_words(a.get(), src, "an input")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.PICK_IDS)
def test_device_pick_best_equals_restatement(name, rdf, gpu_runtime):
    case = tc.pick_case(name)
    want = tc.run_pick_best(case)
    got = device_pick_best(rdf, gpu_runtime, case, (case.tree, case.next_counts, case.best_gain))
    for g, w, what in zip(got, want, ("tree", "next_counts", "best_gain")):
        assert_same_words(g, w, f"{name} {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("last_level", [False, True], ids=["inner", "last"])
def test_device_pick_best_twice_keeps_the_restatements_stale_entries(last_level, rdf, gpu_runtime):
    first, second = tc.two_blocks(last_level)
    want = tc.run_pick_best(second, state=tuple(a.copy() for a in tc.run_pick_best(first)))
    got = device_pick_best(rdf, gpu_runtime, first, (first.tree, first.next_counts, first.best_gain))
    got = device_pick_best(rdf, gpu_runtime, second, got)
    for g, w, what in zip(got, want, ("tree", "next_counts", "best_gain")):
        assert_same_words(g, w, what)


@pytest.mark.gpu
@pytest.mark.parametrize("density", tc.NEXT_DENSITY)
@pytest.mark.parametrize("n_active", tc.NEXT_N)
def test_device_next_active_equals_ascending_compaction(n_active, density, rdf, gpu_runtime):
    case = tc.next_active_case(n_active, density)
    want_buf, want_n = tc.run_next_active(case)
    d_tree, d_active, d_next, d_n = (rdf.to_device(a) for a in (case.tree, case.active, case.next_active, case.n_next))
    assert gpu_runtime.lib.rdf_train_next_active(case.level, case.D, case.C, d_tree.ptr, d_active.ptr, n_active, d_next.ptr,
                                                 d_n.ptr, gpu_runtime.stream()) == 0
    assert_same_words(d_n.get(), want_n, "n_next")
    assert_same_words(d_next.get(), want_buf, "next_active")
    assert_same_words(d_tree.get(), case.tree, "tree")
    assert_same_words(d_active.get(), case.active, "active")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", tc.UPDATE_SHAPES, ids=["3x37x53", "1x1x1"])
def test_device_update_pixels_equals_restatement(shape, rdf, gpu_runtime):
    case = tc.update_pixels_case(shape)
    want = tn.update_pixels(case.depth, case.nodes, case.tree, case.level, case.C).astype(np.int32)
    d_depth, d_nodes, d_tree = (rdf.to_device(a) for a in (case.depth, case.nodes, case.tree))
    n, h, w = shape
    assert gpu_runtime.lib.rdf_train_update_pixels(d_depth.ptr, n, w, h, case.level, case.D, case.C, d_nodes.ptr, d_tree.ptr,
                                                   gpu_runtime.stream()) == 0
    assert_same_words(d_nodes.get(), want, "nodes")
    assert_same_words(d_tree.get(), case.tree, "tree")
    assert np.array_equal(d_depth.get(), case.depth)


@pytest.mark.gpu
@pytest.mark.parametrize("C", tc.INIT_C)
@pytest.mark.parametrize("n_px", tc.INIT_PX)
def test_device_init_equals_bincount(n_px, C, rdf, gpu_runtime):
    case = tc.init_case(n_px, C)
    want_nodes, want_root = tc.init_expected(case)
    d_labels, d_root = rdf.to_device(case.labels), rdf.to_device(case.root)
    d_nodes = rdf.to_device(np.full(n_px + 3, tc.SENT_I32, np.int32))
    assert gpu_runtime.lib.rdf_train_init(d_labels.ptr, n_px, C, d_nodes.ptr, d_root.ptr, gpu_runtime.stream()) == 0
    assert_same_words(d_root.get(), want_root, "root counts")
    assert_same_words(d_nodes.get(), np.concatenate([want_nodes, np.full(3, tc.SENT_I32, np.int32)]), "nodes")


@pytest.mark.gpu
def test_device_right_counts_equals_parent_minus_left(rdf, gpu_runtime):
    case = tc.right_counts_case()
    P, NB, C = case.counts.shape
    d_active, d_parents, d_counts = (rdf.to_device(a) for a in (case.active, case.node_counts, case.counts))
    assert gpu_runtime.lib.rdf_train_right_counts(len(case.active), d_active.ptr, P, NB, case.start, case.end, C,
                                                  d_parents.ptr, d_counts.ptr, gpu_runtime.stream()) == 0
    assert_same_words(d_counts.get(), tc.right_counts_expected(case), "counts")
    assert_same_words(d_parents.get(), case.node_counts, "parents")


@pytest.mark.gpu
@pytest.mark.parametrize("P", tc.COUNT_P)
def test_device_counts_equal_a_plain_count(P, rdf, gpu_runtime):
    """rdf_train_histogram; rdf_train_histogram_left (+ _ws with and without the parents' counts, workspace left zero) and
    the sorted rows (up to 1024 proposals), each followed by rdf_train_right_counts: all equal to count_children."""
    lib, st = gpu_runtime.lib, gpu_runtime.stream
    case = tc.count_case(P)
    n, h, w = case.depth.shape
    C, n_nodes = case.C, 1 << case.level
    d_depth, d_labels, d_nodes, d_props, d_parents = (rdf.to_device(a) for a in (case.depth, case.labels, case.nodes,
                                                                                 case.props, case.parents))
    d_active = rdf.to_device(np.arange(n_nodes, dtype=np.int32))
    row_bytes = int(lib.rdf_train_bits_row_bytes(P))
    assert row_bytes == {1: 8, 3: 8, 5: 8, 130: 32, 1025: 0}[P]
    n_live = int(case.parents.sum())
    pos = rdf.DeviceArray(case.depth.shape, np.int32)
    rowkey = rdf.DeviceArray((n_live,), np.int32)
    bits = rdf.DeviceArray((n_live * max(row_bytes, 8),), np.uint8)
    work = rdf.DeviceArray((int(lib.rdf_train_sort_workspace_bytes(n_nodes, C)),), np.uint8).fill(255)     # (the call zeroes it)
    bws = rdf.DeviceArray((int(lib.rdf_train_bits_workspace_bytes(P)),), np.uint8)
    assert lib.rdf_train_sort_pixels(d_labels.ptr, d_nodes.ptr, case.depth.size, C, n_nodes, pos.ptr, rowkey.ptr, work.ptr,
                                     st()) == 0
    rc_bits = lib.rdf_train_decision_bits(d_depth.ptr, pos.ptr, n, w, h, d_props.ptr, P, bits.ptr, bws.ptr, st())
    assert rc_bits == (0 if P <= 1024 else -1)                                      # RDF_ERR_BAD_ARG

    def with_right_counts(arr, start, end, NB):
        assert lib.rdf_train_right_counts(n_nodes, d_active.ptr, P, NB, start, end, C, d_parents.ptr, arr.ptr, st()) == 0
        return arr.get()

    for window in tc.COUNT_WINDOWS:
        start, end, NB = window
        want = tc.plain_counts(P, window)
        args = (d_depth.ptr, d_labels.ptr, d_nodes.ptr, n, w, h, d_props.ptr, P, C, start, end, NB)
        full = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
        assert lib.rdf_train_histogram(*args, full.ptr, st()) == 0
        assert_same_words(full.get(), want, f"rdf_train_histogram {window}")
        left = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
        assert lib.rdf_train_histogram_left(*args, left.ptr, st()) == 0
        want_left = want.copy()
        want_left[:, 1::2] = 0
        assert_same_words(left.get(), want_left, f"rdf_train_histogram_left {window}")
        assert_same_words(with_right_counts(left, *window), want, f"rdf_train_histogram_left + right_counts {window}")
        ws = rdf.DeviceArray((int(lib.rdf_train_histogram_workspace_bytes(P, NB, C)),), np.uint8).fill(0)
        for parents_ptr in (None, d_parents.ptr):
            packed = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
            assert lib.rdf_train_histogram_left_ws(*args, packed.ptr, ws.ptr, parents_ptr, st()) == 0
            assert_same_words(packed.get(), want_left, f"rdf_train_histogram_left_ws {window} parents={parents_ptr is not None}")
            assert not ws.get().any()
            assert_same_words(with_right_counts(packed, *window), want, f"rdf_train_histogram_left_ws + right_counts {window}")
        rows = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
        rc_rows = lib.rdf_train_count_rows(bits.ptr, rowkey.ptr, work.ptr, n_nodes, P, C, start, end, NB, rows.ptr, st())
        if P <= 1024:
            assert rc_rows == 0
            assert_same_words(rows.get(), want_left, f"sorted rows {window}")
            assert_same_words(with_right_counts(rows, *window), want, f"sorted rows + right_counts {window}")
        else:
            assert rc_rows == -1 and not rows.get().any()                           # RDF_ERR_BAD_ARG, nothing counted


@pytest.mark.gpu
def test_trainer_of_1025_proposals_drops_the_sorted_rows(rdf, gpu_runtime):
    from test_training import _ArrayDataset
    case = tc.count_case(1025)
    assert int(gpu_runtime.lib.rdf_train_bits_row_bytes(1025)) == 0 and int(gpu_runtime.lib.rdf_train_bits_row_bytes(1024)) == 128
    trainer = rdf.DecisionTreeTrainer(2, 1025)
    trainer.allocate(_ArrayDataset(case.depth, case.labels, case.C + 2, per_block=2), 1025, 3)
    assert trainer.use_sorted_rows is False
