"""The trainer's feature response -- depth[p + floor(u / d)] - depth[p + floor(v / d)] < thr -- where its three device
implementations can go wrong without the random proposals of the other training tests noticing: probes on the last staged
cell of a tile and on the first one beyond it (both halos), on the image's border and in the neighbouring image's rows;
numerators on floor boundaries and on both sides of the ranges the fast divides are verified for (so that the IEEE
fallbacks of k_train_histogram and k_train_bits run), NaN and infinities; thresholds equal to the response, denormal,
signed zeros, NaN; a 16-bit count field holding exactly 65535; the counting sort at 1, 16384 and 16388 keys.
Cases: tests/train_feature_cases.py.  Every comparison is on integers or bits and exact.

CPU: the cases meet the conditions they were built for -- probes counted by where they land, at least 32 per edge; each
wrong reading of the operation (a mutant of a copy of the restatement) changes the decisions of the case meant for it.
GPU (-m gpu): rdf_train_sort_pixels + rdf_train_decision_bits per pixel and proposal, every counting entry point, and
rdf_train_update_pixels, each against oracle/train_numpy.py through the C ABI.

Undefined in the reference and pinned here as train_numpy defines it: a pixel on a node whose label is >= C is counted
nowhere (the reference would index its histogram out of bounds) but is routed by update_pixels like any other; a NaN
quotient floors to 0; an infinite one saturates and the add wraps."""
import numpy as np
import pytest

import train_feature_cases as fc
from oracle import train_numpy as tn

F32 = np.float32
SENT64 = np.uint64(0xDEADBEEFCAFEF00D)


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    same = got == want
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} differ; first at {np.argwhere(~same)[:5].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the cases bite
# ---------------------------------------------------------------------------------------------------------------------
def test_frames_are_what_the_cases_need():
    fr = fc.frames()
    n, h, w = fr.depth.shape
    assert n >= 2 and w >= 130 and h >= 74 and w % fc.TILE_W and h % fc.TILE_H
    assert not np.array_equal(fr.depth[0], fr.depth[1])
    img, y, x = fr.live_pixels()
    d = fr.depth[img, y, x]
    assert set(np.unique(d).tolist()) == set(fc.DEPTHS) | {0, 65535}
    assert (d == 0).sum() >= 8 and (d == 65535).sum() >= 8
    assert all(fc.LCM % k == 0 for k in fc.DEPTHS)
    other = fr.depth[~fr.live]
    assert other.min() >= 1 and other.max() <= 65534 and len(np.unique(other)) > other.size // 4
    assert ((fr.nodes >= 0) & (fr.labels >= fr.C)).sum() >= 8 and (fr.labels[fr.live] == 0).any()
    # every lane of the 32 x 8 tile holds a live pixel somewhere; so do the first and last tile rows and columns, the
    # partial ones (x from 128, y from 72) included
    assert len(set(((y % fc.TILE_H) * fc.TILE_W + x % fc.TILE_W).tolist())) == fc.TILE_W * fc.TILE_H
    for i in range(n):
        one = fr.live[i]
        assert one[0].any() and one[h - 1].any() and one[:, 0].any() and one[:, w - 1].any()
        assert one[:fc.TILE_H, :fc.TILE_W].any() and one[h - h % fc.TILE_H:, w - w % fc.TILE_W:].any()
    assert int(fr.parents.sum()) == len(img) and (fr.parents > 0).all()


@pytest.mark.parametrize("name", fc.CASES)
def test_copy_of_the_restatement_is_the_restatement(name):
    """fc.response (all proposals at once, returns the probe positions) decides as tn.compute_feature does, and the counts
    that follow from its decisions are tn.count_children's, over both windows."""
    fr, props = fc.frames(), fc.case_props(name)
    want = fc.expected_bits(name)
    assert_same(fc.decisions(fr, props), want, name)
    img, y, x = fr.live_pixels()
    node, lab = fr.nodes[img, y, x].astype(np.int64), fr.labels[img, y, x].astype(np.int64)
    for window in fc.WINDOWS:
        start, end, NB = window
        inside = (node * 2 >= start) & (node * 2 + 1 < end)
        mine = np.zeros((len(props), NB, fr.C), np.uint64)
        for j in range(len(props)):
            child = node * 2 + np.where(want[:, j], 0, 1) - start
            np.add.at(mine[j], (child[inside], lab[inside]), 1)
        assert_same(mine, fc.expected_counts(name, window), f"{name} {window}")


def test_halo_case_reaches_every_edge(capsys):
    """At least 32 live (pixel, proposal, probe) triples on the last staged cell and on the first one beyond it, for both
    halos, both axes and both sides; on the image's border cells and the first ones outside; in the other image's rows."""
    fr, props = fc.frames(), fc.halo_props()
    assert len(props) == 70 and len(props) % 4 and len(props) > 64
    cov = fc.coverage(fr, props)
    with capsys.disabled():
        print("\n  halo: " + ", ".join(f"{k}: {v}" for k, v in cov.items()), end="")
    assert len(cov) == 16 + 8 + 3
    for k, v in cov.items():
        if k != "f == thr":
            assert v >= 32, (k, v)
    share = fc.expected_bits("halo").mean(axis=0)
    assert (share >= 0.2).all() and (share <= 0.8).all(), (share.min(), share.max())
    num = props[:, :4]
    whole = num == np.round(num / fc.LCM) * fc.LCM
    assert whole.sum() >= 64 and (~whole).sum() >= 64 and (props[:, 2:4] == 0).all(axis=1).sum() >= 14
    assert (num > 0).any(axis=0).all() and (num < 0).any(axis=0).all()
    assert ((num == 0) | ((np.abs(num) >= 2.0 ** -87) & (np.abs(num) < 2.0 ** 21))).all()       # both kernels' fast paths


def test_numerator_and_threshold_cases_hold_what_they_name(capsys):
    a = fc.numerator_props_a()
    num = a[:, :4]
    fine_hist = (num == 0) | ((np.abs(num) >= 2.0 ** -87) & (np.abs(num) < 2.0 ** 104))
    fine_bits = (num == 0) | ((np.abs(num) >= 2.0 ** -87) & (np.abs(num) < 2.0 ** 21))
    assert fine_hist.all() and fine_bits.all() and len(a) % 4 and len(a) > 32
    for v in (fc.BIG_IN, -fc.BIG_IN, fc.TINY_IN, -fc.TINY_IN):
        assert (num == v).any()
    assert fc.BIG_IN == 2097151.75 and fc.TINY_IN == 2.0 ** -87
    assert ((num == 0) & np.signbit(num)).any() and ((num == 0) & ~np.signbit(num)).any()
    assert ((num > -1) & (num < 0)).any() and ((num > 0) & (num < 1)).any()         # inside (-d, 0) and (0, d) at every depth
    for name, (value, slot) in fc.REPLACEMENTS.items():
        b = fc.numerator_props_b(name)
        j = fc.replaced_proposal(name)
        differs = b.view(np.uint32) != a.view(np.uint32)
        assert differs[:, :4].sum() == 1 and differs[j, slot] and not np.delete(differs, j, axis=0).any()
        in_hist = value == 0 or 2.0 ** -87 <= abs(value) < 2.0 ** 104
        in_bits = value == 0 or 2.0 ** -87 <= abs(value) < 2.0 ** 21
        assert not in_bits and in_hist == (name in ("2p21", "int_max_less_127"))
    assert sorted(fc.replaced_proposal(k) % 4 for k in list(fc.REPLACEMENTS)[:4]) == [0, 1, 2, 3]
    with np.errstate(over="ignore"):
        assert np.floor(F32(3e38) / F32(65535)) > 2.0 ** 31 and F32(1e-40) > 0 and F32(1e-40) < np.finfo(np.float32).tiny
    t = fc.threshold_props()
    thr = t[:, 4]
    assert np.isnan(thr).sum() == 4 and np.isposinf(thr).sum() == 4 and np.isneginf(thr).sum() == 4
    assert (thr.view(np.uint32) == 1).sum() >= 4 and (thr.view(np.uint32) == 0x80000001).sum() >= 4
    assert ((thr == 0) & np.signbit(thr)).sum() >= 4 and ((thr == 0) & ~np.signbit(thr)).sum() >= 4
    for v in (65535, -65535, 65536, -65536):
        assert (thr == v).sum() == 4
    fr = fc.frames()
    cov = fc.coverage(fr, t)
    with capsys.disabled():
        print(f"\n  thr: f == thr at {cov['f == thr']} (pixel, proposal) pairs", end="")
    assert cov["f == thr"] >= 32
    img, y, x = fr.live_pixels()
    f, _ = fc.response(fr.depth, img, y, x, t)
    for k in range(1, len(fc.THR_BASES)):          # (the first response is 0 everywhere: its threshold edges are 0, +-denormal)
        rows = slice(14 * k, 14 * k + 3)           # the value f takes, the float above, the float below
        hit = (f[rows] == thr[rows, None]).sum(axis=1)
        assert hit[0] >= 32 and hit[1] == 0 and hit[2] == 0
        assert (f[rows] < thr[rows, None]).sum(axis=1).tolist()[1] == (f[rows] <= thr[rows, None]).sum(axis=1).tolist()[0]
    assert (f[0] == 0).all()


@pytest.mark.parametrize("name", sorted(fc.KILLS))
def test_each_mutant_changes_the_case_meant_for_it(name, capsys):
    """A wrong reading of the operation that leaves a case's decisions unchanged would pass the GPU tests of that case."""
    fr, props = fc.frames(), fc.case_props(name)
    want = fc.expected_bits(name)
    killed = {}
    for m in fc.MUTANTS:
        changed = fc.decisions(fr, props, m) != want
        killed[m] = int(changed.sum())
        if m in fc.KILLS[name] and name.startswith("num_b_"):       # ... in the proposal that holds the replaced numerator
            assert changed[:, fc.replaced_proposal(name[6:])].any(), (name, m)
    with capsys.disabled():
        print(f"\n  {name}: decisions changed by " + ", ".join(f"{m}: {k}" for m, k in killed.items()), end="")
    for m in fc.KILLS[name]:
        assert killed[m] > 0, (name, m)


def test_every_mutant_is_met_by_some_case():
    assert set(m for ms in fc.KILLS.values() for m in ms) == set(fc.MUTANTS)


def test_limit_case_holds_exactly_65535_and_65536():
    fr, props = fc.limit_case()
    assert fr.depth.size == 132000 and fr.live.all()
    assert fr.parents.tolist() == [[0, 65535, 929], [0, 65536, 0]] and len(props) == 6
    want = fc.limit_counts()
    for j, left in ((0, True), (1, True), (2, False), (3, False)):        # the closed form: all left, or all right
        side = want[j].reshape(2, 2, fr.C)[:, 0 if left else 1]
        assert np.array_equal(side, fr.parents) and want[j].sum() == 132000
    for j in (4, 5):
        share = want[j, 0::2].sum() / 132000
        assert 0.05 < share < 0.95
        assert np.array_equal(want[j, 0::2] + want[j, 1::2], fr.parents)


@pytest.mark.parametrize("n_nodes,n_classes", fc.SORT_KEYS)
def test_sort_cases_hold_the_waves_they_name(n_nodes, n_classes):
    fr, _ = fc.sort_case(n_nodes, n_classes)
    n_keys = n_nodes * n_classes
    assert fr.depth.size % 64 == 37
    assert fc.sort_slot_shift(n_keys) == {1: 8, 16384: 0, 16388: 0}[n_keys]
    n_counters = n_keys << fc.sort_slot_shift(n_keys)
    per_thread = (n_counters + 1023) // 1024         # k_train_sort_scan: thread t takes counters [t * per, t * per + per)
    assert (n_counters, per_thread) == {1: (256, 1), 16384: (16384, 16), 16388: (16388, 17)}[n_keys]
    assert (1023 * per_thread >= n_counters) == (n_keys != 16384)                  # the last threads' runs are empty
    distinct = fc.distinct_keys_per_wave(fr)
    key = fr.nodes[fr.live].astype(np.int64) * fr.C + fr.labels[fr.live]
    assert key.min() == 0 and key.max() == n_keys - 1 and not fr.live.all()
    if n_keys == 1:
        assert set(distinct) <= {0, 1}
    else:
        assert distinct[:8] == [4] * 8 and distinct[8:16] == [1] * 8 and distinct[16:24] == [5] * 8
        assert max(distinct[24:]) >= 40
    start, end, NB = fc.sort_window(n_nodes)
    node = fr.nodes[fr.live]
    assert start % 2 == 0 and ((node * 2 >= start).any() and (node * 2 < start).any() or n_nodes == 1)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every entry point on a case's arrays, once; the tests below look at what came back
# ---------------------------------------------------------------------------------------------------------------------
def unpack_rows(raw, n_rows, P):
    """(bool [n_rows, P], uint32 words of the padding beyond P OR-ed together) from the row bytes."""
    words = raw.view(np.uint32).reshape(n_rows, -1)
    j = np.arange(P)
    got = ((words[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)
    pad = words.copy()
    pad[:, :P >> 5] = 0
    if P & 31:
        pad[:, P >> 5] &= ~np.uint32((1 << (P & 31)) - 1)
    return got, int(np.bitwise_or.reduce(pad, axis=None))


def sort_and_bits(rdf, rt, fr, props, d_depth, d_labels, d_nodes, d_props, n_nodes):
    """rdf_train_sort_pixels + rdf_train_decision_bits; the rows start as all ones."""
    lib, st = rt.lib, rt.stream
    n, h, w = fr.depth.shape
    P = len(props)
    n_live = int(fr.live.sum())
    row_bytes = int(lib.rdf_train_bits_row_bytes(P))
    pos = rdf.DeviceArray(fr.depth.shape, np.int32).fill(0x55)
    rowkey = rdf.DeviceArray((max(n_live, 1),), np.int32).fill(0x55)
    bits = rdf.DeviceArray((max(n_live, 1) * row_bytes,), np.uint8).fill(255)
    work = rdf.DeviceArray((int(lib.rdf_train_sort_workspace_bytes(n_nodes, fr.C)),), np.uint8).fill(255)
    bws = rdf.DeviceArray((int(lib.rdf_train_bits_workspace_bytes(P)),), np.uint8).fill(255)
    assert lib.rdf_train_sort_pixels(d_labels.ptr, d_nodes.ptr, fr.depth.size, fr.C, n_nodes, pos.ptr, rowkey.ptr, work.ptr,
                                     st()) == 0
    assert lib.rdf_train_decision_bits(d_depth.ptr, pos.ptr, n, w, h, d_props.ptr, P, bits.ptr, bws.ptr, st()) == 0
    return pos, rowkey, bits, work


_RUNS = {}


def device_run(name, rdf, rt):
    """Everything the device computes for one case of fc.CASES, each launch once.  Only return codes are checked here."""
    if name in _RUNS:
        return _RUNS[name]
    lib, st = rt.lib, rt.stream
    fr, props = fc.frames(), fc.case_props(name)
    n, h, w = fr.depth.shape
    P, C, n_nodes = len(props), fr.C, 1 << fr.level
    d_depth, d_labels, d_nodes, d_props, d_parents = (rdf.to_device(a) for a in (fr.depth, fr.labels, fr.nodes, props,
                                                                                 fr.parents))
    d_active = rdf.to_device(np.arange(n_nodes, dtype=np.int32))
    out = {}
    pos, rowkey, bits, work = sort_and_bits(rdf, rt, fr, props, d_depth, d_labels, d_nodes, d_props, n_nodes)
    out["pos"], out["rowkey"], out["bits"] = pos.get(), rowkey.get(), bits.get()

    def with_right_counts(arr, start, end, NB):
        assert lib.rdf_train_right_counts(n_nodes, d_active.ptr, P, NB, start, end, C, d_parents.ptr, arr.ptr, st()) == 0
        return arr.get()

    for window in fc.WINDOWS:
        start, end, NB = window
        args = (d_depth.ptr, d_labels.ptr, d_nodes.ptr, n, w, h, d_props.ptr, P, C, start, end, NB)
        res = out[window] = {}
        full = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
        assert lib.rdf_train_histogram(*args, full.ptr, st()) == 0
        res["rdf_train_histogram"] = (None, full.get())
        left = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
        assert lib.rdf_train_histogram_left(*args, left.ptr, st()) == 0
        res["rdf_train_histogram_left"] = (left.get(), with_right_counts(left, *window))
        ws = rdf.DeviceArray((int(lib.rdf_train_histogram_workspace_bytes(P, NB, C)),), np.uint8).fill(0)
        for parents_ptr, tag in ((None, "no parents"), (d_parents.ptr, "parents")):
            packed = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
            assert lib.rdf_train_histogram_left_ws(*args, packed.ptr, ws.ptr, parents_ptr, st()) == 0
            res[f"rdf_train_histogram_left_ws, {tag}"] = (packed.get(), with_right_counts(packed, *window))
            res[f"workspace, {tag}"] = bool(ws.get().any())
        rows = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
        assert lib.rdf_train_count_rows(bits.ptr, rowkey.ptr, work.ptr, n_nodes, P, C, start, end, NB, rows.ptr, st()) == 0
        res["rdf_train_count_rows"] = (rows.get(), with_right_counts(rows, *window))

    tree, level, D = fc.routing_tree(props, C)
    d_tree = rdf.to_device(tree)
    d_route = rdf.DeviceArray(fr.depth.shape, np.int32)
    routed = []
    for turn in range(P):
        d_route.set(fc.routing_nodes(fr, P, turn))
        assert lib.rdf_train_update_pixels(d_depth.ptr, n, w, h, level, D, C, d_route.ptr, d_tree.ptr, st()) == 0
        routed.append(d_route.get())
    out["routed"] = routed
    out["tree"] = d_tree.get()
    out["inputs"] = tuple(a.get() for a in (d_depth, d_labels, d_nodes, d_props, d_parents))
    _RUNS[name] = out
    return out


def describe(fr, props, i, j):
    """Where live pixel i's probes land under proposal j, for a failure message."""
    img, y, x = (a[i:i + 1] for a in fr.live_pixels())
    f, (ux, uy, vx, vy) = fc.response(fr.depth, img, y, x, props[j:j + 1])
    return (f"image {img[0]}, y {y[0]}, x {x[0]} (depth {fr.depth[img[0], y[0], x[0]]}), proposal {j} = {props[j].tolist()}: "
            f"u probe at (x {ux[0, 0]}, y {uy[0, 0]}), v probe at (x {vx[0, 0]}, y {vy[0, 0]}), f = {f[0, 0]}")


def device_bits(name, rdf, rt):
    """bool [n_live, P] in the order of fr.live_pixels(), read through pos."""
    fr, props = fc.frames(), fc.case_props(name)
    run = device_run(name, rdf, rt)
    n_live = int(fr.live.sum())
    rows = run["pos"][fr.live]
    assert_same(np.sort(rows), np.arange(n_live, dtype=np.int32), "pos is no permutation of the rows")
    got, pad = unpack_rows(run["bits"], n_live, len(props))
    return got[rows], pad


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.CASES)
def test_device_decision_bits_per_pixel(name, rdf, gpu_runtime):
    """Bit j of row pos[i] is compute_feature(...) < thr_j for every live pixel i; padding bits beyond P are zero."""
    fr, props = fc.frames(), fc.case_props(name)
    run = device_run(name, rdf, gpu_runtime)
    assert (run["pos"][~fr.live] == -1).all()
    got, pad = device_bits(name, rdf, gpu_runtime)
    want = fc.expected_bits(name)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{len(bad)} of {want.size} decisions differ (device {bool(got[tuple(bad[0])])}); first: " +
                           describe(fr, props, int(bad[0][0]), int(bad[0][1])))
    assert pad == 0, f"padding bits set: {pad:#x}"
    key = fr.nodes[fr.live] * fr.C + fr.labels[fr.live].astype(np.int32)
    assert_same(run["rowkey"][run["pos"][fr.live]], key, "rowkey")


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.CASES)
def test_device_counts_equal_count_children(name, rdf, gpu_runtime):
    """rdf_train_histogram; rdf_train_histogram_left, rdf_train_histogram_left_ws (with and without the parents' counts,
    workspace left zero) and rdf_train_count_rows, each then completed by rdf_train_right_counts: tn.count_children, over all
    children and over the window of nodes 1 and 2."""
    run = device_run(name, rdf, gpu_runtime)
    for window in fc.WINDOWS:
        want = fc.expected_counts(name, window)
        want_left = want.copy()
        want_left[:, 1::2] = 0
        assert want_left.sum() > 0 and want.sum() > want_left.sum()
        for entry, got in run[window].items():
            if entry.startswith("workspace"):
                assert got is False, f"{name} {window} {entry}: not left zero"
                continue
            left, both = got
            if left is not None:
                assert_same(left, want_left, f"{name} {window} {entry}")
            assert_same(both, want, f"{name} {window} {entry} (+ rdf_train_right_counts)")


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.CASES)
def test_device_update_pixels_routes_as_the_decision_bits_say(name, rdf, gpu_runtime):
    """One tree record per proposal, pixel i on node (i + turn) mod P: over P turns rdf_train_update_pixels answers every
    (pixel, proposal) pair.  It must equal tn.update_pixels, and send a pixel left exactly where its decision bit is set."""
    fr, props = fc.frames(), fc.case_props(name)
    run = device_run(name, rdf, gpu_runtime)
    bits, _ = device_bits(name, rdf, gpu_runtime)
    tree, level, D = fc.routing_tree(props, fr.C)
    P = len(props)
    live = fr.live
    for turn in range(P):
        before = fc.routing_nodes(fr, P, turn)
        want = tn.update_pixels(fr.depth, before, tree, level, fr.C).astype(np.int32)
        got = run["routed"][turn]
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{name} turn {turn}: {len(bad)} pixels differ; first (image, y, x) {bad[0].tolist()}: " \
                              f"node {before[tuple(bad[0])]} -> {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"
        assert (got[fr.nodes < 0] == -1).all() and (got[fr.nodes >= 0] >> 1 == before[fr.nodes >= 0]).all()
        went_left = (got[live] & 1) == 0
        said_left = bits[np.arange(len(bits)), before[live]]
        bad = np.nonzero(went_left != said_left)[0]
        assert len(bad) == 0, "routed against the decision bit: " + describe(fr, props, int(bad[0]), int(before[live][bad[0]]))
    assert_same(run["tree"].view(np.uint32), tree.view(np.uint32), "tree")


@pytest.mark.gpu
@pytest.mark.parametrize("name", fc.CASES)
def test_device_leaves_its_inputs_untouched(name, rdf, gpu_runtime):
    fr, props = fc.frames(), fc.case_props(name)
    run = device_run(name, rdf, gpu_runtime)
    for got, want, what in zip(run["inputs"], (fr.depth, fr.labels, fr.nodes, props, fr.parents),
                               ("depth", "labels", "nodes", "proposals", "parents")):
        assert got.tobytes() == want.tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(fc.REPLACEMENTS))
def test_device_fast_and_ieee_paths_answer_shared_proposals_alike(variant, rdf, gpu_runtime):
    """Block (b) is block (a) with one numerator out of k_train_bits' range: the whole launch takes the IEEE divide, and
    (but for 2^21 and 2^31 - 128) the changed proposal of k_train_histogram does.  Every proposal the two blocks share must get the same
    decision bits and the same counts from both launches."""
    a, b = device_run("num_a", rdf, gpu_runtime), device_run("num_b_" + variant, rdf, gpu_runtime)
    shared = np.delete(np.arange(fc.P_NUM), fc.replaced_proposal(variant))
    assert np.array_equal(fc.numerator_props_a()[shared].view(np.uint32), fc.numerator_props_b(variant)[shared].view(np.uint32))
    bits_a, _ = device_bits("num_a", rdf, gpu_runtime)
    bits_b, _ = device_bits("num_b_" + variant, rdf, gpu_runtime)
    assert_same(bits_b[:, shared], bits_a[:, shared], "decision bits")
    for window in fc.WINDOWS:
        for entry, got in b[window].items():
            if not entry.startswith("workspace"):
                assert_same(got[1][shared], a[window][entry][1][shared], f"{window} {entry}")


@pytest.mark.gpu
def test_device_quad_counters_hold_exactly_65535(rdf, gpu_runtime):
    """A (node, class) of exactly 65535 pixels counts in 16-bit fields, four proposals to a 64-bit word, and with every
    pixel going left a field ends at 0xFFFF next to fields at 0; one of 65536 pixels must take the 32-bit fields."""
    lib, st = gpu_runtime.lib, gpu_runtime.stream
    fr, props = fc.limit_case()
    want = fc.limit_counts()
    want_left = want.copy()
    want_left[:, 1::2] = 0
    assert want_left[0, 0].tolist() == [0, 65535, 929] and want_left[1, 2].tolist() == [0, 65536, 0] and not want_left[2:4].any()
    n, h, w = fr.depth.shape
    P, C, NB = len(props), fr.C, 4
    d_depth, d_labels, d_nodes, d_props, d_parents = (rdf.to_device(a) for a in (fr.depth, fr.labels, fr.nodes, props,
                                                                                 fr.parents))
    d_active = rdf.to_device(np.arange(2, dtype=np.int32))
    args = (d_depth.ptr, d_labels.ptr, d_nodes.ptr, n, w, h, d_props.ptr, P, C, 0, 4, NB)
    ws = rdf.DeviceArray((int(lib.rdf_train_histogram_workspace_bytes(P, NB, C)),), np.uint8).fill(0)
    for parents_ptr in (d_parents.ptr, None):
        packed = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
        assert lib.rdf_train_histogram_left_ws(*args, packed.ptr, ws.ptr, parents_ptr, st()) == 0
        assert_same(packed.get(), want_left, f"parents={parents_ptr is not None}")
        assert not ws.get().any()
        assert lib.rdf_train_right_counts(2, d_active.ptr, P, NB, 0, 4, C, d_parents.ptr, packed.ptr, st()) == 0
        assert_same(packed.get(), want, f"parents={parents_ptr is not None} + rdf_train_right_counts")
    for got, src in zip((d_depth, d_labels, d_nodes, d_props, d_parents), (fr.depth, fr.labels, fr.nodes, props, fr.parents)):
        assert got.get().tobytes() == src.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,n_classes", fc.SORT_KEYS)
def test_device_sort_at_the_key_count_edges(n_nodes, n_classes, rdf, gpu_runtime):
    """1 key (256 counters of its own), 16384 keys (16 per scan thread) and 16388 (ragged runs, the last scan threads
    empty): pos is a permutation of the rows on the live pixels and -1 elsewhere, rowkey[pos[i]] is pixel i's key, rowkey
    ascends, and rdf_train_count_rows over the upper half of the nodes is tn.count_children."""
    lib, st = gpu_runtime.lib, gpu_runtime.stream
    fr, props = fc.sort_case(n_nodes, n_classes)
    P, C = len(props), n_classes
    d_depth, d_labels, d_nodes, d_props = (rdf.to_device(a) for a in (fr.depth, fr.labels, fr.nodes, props))
    pos, rowkey, bits, work = sort_and_bits(rdf, gpu_runtime, fr, props, d_depth, d_labels, d_nodes, d_props, n_nodes)
    live = fr.live
    n_live = int(live.sum())
    got_pos, keys = pos.get(), rowkey.get()[:n_live]
    assert (got_pos[~live] == -1).all()
    assert_same(np.sort(got_pos[live]), np.arange(n_live, dtype=np.int32), "pos")
    assert (np.diff(keys) >= 0).all()
    assert_same(keys[got_pos[live]], (fr.nodes[live] * C + fr.labels[live].astype(np.int32)), "rowkey")
    n_counters = (n_nodes * C) << fc.sort_slot_shift(n_nodes * C)
    assert int(work.get().view(np.uint32)[3 * n_counters]) == n_live
    start, end, NB = fc.sort_window(n_nodes)
    want = tn.count_children(fr.depth, fr.labels, fr.nodes, props, start, end, NB, C)
    want[:, 1::2] = 0
    assert want.sum() > 0
    rows = rdf.DeviceArray((P, NB, C), np.uint64).fill(0)
    assert lib.rdf_train_count_rows(bits.ptr, rowkey.ptr, work.ptr, n_nodes, P, C, start, end, NB, rows.ptr, st()) == 0
    assert_same(rows.get(), want, "rdf_train_count_rows")
    for got, src in zip((d_depth, d_labels, d_nodes, d_props), (fr.depth, fr.labels, fr.nodes, props)):
        assert got.get().tobytes() == src.tobytes()


@pytest.mark.gpu
def test_device_sort_of_a_frame_without_a_live_pixel(rdf, gpu_runtime):
    """Every pixel off the tree or with a label >= C: no rows, pos -1 everywhere, rdf_train_count_rows adds nothing."""
    lib, st = gpu_runtime.lib, gpu_runtime.stream
    base, props = fc.sort_case(4096, 4)
    nodes = np.where(base.labels >= base.C, base.nodes, -1).astype(np.int32)
    nodes[0, 0, :7] = 3
    labels = base.labels.copy()
    labels[0, 0, :7] = base.C
    fr = fc.Frames(base.depth, labels, nodes, base.C, base.level, base.parents)
    assert not fr.live.any() and (nodes >= 0).any()
    P, C, n_nodes = len(props), fr.C, 4096
    d_depth, d_labels, d_nodes, d_props = (rdf.to_device(a) for a in (fr.depth, fr.labels, fr.nodes, props))
    pos, rowkey, bits, work = sort_and_bits(rdf, gpu_runtime, fr, props, d_depth, d_labels, d_nodes, d_props, n_nodes)
    assert (pos.get() == -1).all()
    assert int(work.get().view(np.uint32)[3 * n_nodes * C]) == 0
    assert (bits.get() == 255).all()
    start, end, NB = fc.sort_window(n_nodes)
    filled = np.full((P, NB, C), SENT64, np.uint64)
    rows = rdf.to_device(filled)
    assert lib.rdf_train_count_rows(bits.ptr, rowkey.ptr, work.ptr, n_nodes, P, C, start, end, NB, rows.ptr, st()) == 0
    assert_same(rows.get(), filled, "counts")
