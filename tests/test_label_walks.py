"""The two tree walks of librdf_labels.so -- k_refit_count (LeafRefitter.add, ForestPruner.add) and k_posterior
(get_posteriors_forest) -- on the inputs that break a walk, and the counting paths of k_refit_count that no other case reaches.
The cases are built by tests/walk_cases.py.

  1. The adversarial walk: offsets whose quotients are NaN, saturate, wrap the add or are denormal, probes past every border,
     thresholds equal to the response, NaN and infinite thresholds, flags that only `floor` reads right.
  2. The divide, one ulp at a time: numerators on and next to whole multiples of the pixel's depth.
  3. Counting: `lds_levels == 0` and the `<=` that decides it, class ids up to 2048, and cells of one workgroup that want the
     same bucket of its table (add_deep's fall-back to a global atomic).

Every CPU test here works on the restatements alone: it proves that a case contains what it is meant to contain (so that no GPU
test passes on a case that contains nothing) and pins refit_numpy / posterior_numpy to the oracle's evaluator on these very
inputs.  Every GPU comparison is exact -- integers or fp32 bits -- with no pixel left out; the restatements' answers are
computed once per module, shared and left unchanged.

Out of scope: `use_table == false` in k_refit_count needs T N 2C >= 2^32 - 1 cells, a counts array of 32 GiB."""
import ctypes
import functools
import importlib
from fractions import Fraction

import numpy as np
import pytest

import posterior_numpy as pn
import prune_numpy as prn
import refit_numpy as rn
import walk_cases as wc

NO = 65535
F32 = np.float32
# forest_refit_hip.hip's constants, restated
kLdsCells = 4096          # 32-bit counters of the LDS histogram
kAggIters = 4             # distinct keys a wave aggregates before its remaining lanes add one each
kThreads = 256


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def lds_levels(T, D, C):
    """rdf_labels_refit_count's L: the largest L <= D with T (2^L - 1) 2C <= kLdsCells."""
    L = 0
    while L < D and T * ((2 << L) - 1) * 2 * C <= kLdsCells:
        L += 1
    return L


# ------------------------------------------------------------------ the restatements' answers, once -------------------------
@functools.lru_cache(maxsize=None)
def _adv_ref(scale):
    """The adversarial case at one scale: refit_numpy's (counts, totals) and posterior_numpy's ungated (labels, conf, sums)."""
    depth, labels, forest, _ = wc.adversarial_case()
    counts, totals = rn.count(depth, labels, forest, scale)
    post = pn.posterior(depth, forest, 1, scale)
    _frozen(counts, totals, *post)
    return counts, totals, post


ADV_R2_SCALE = 0.5


@functools.lru_cache(maxsize=None)
def _adv_ref_r2():
    """The adversarial case at labels_reduce 2 under its filter image, scale 0.5: (labels, conf, sums)."""
    depth, _, forest, _ = wc.adversarial_case()
    return _frozen(*pn.posterior(depth, forest, 2, ADV_R2_SCALE, wc.adversarial_filter(), wc.ADV["filter_class"]))


@functools.lru_cache(maxsize=None)
def _adv_traces(scale):
    """Every live walk of the adversarial case at one scale, taken apart: [((image, y, x), tree, [(node, step)], end)]."""
    depth, labels, forest, _ = wc.adversarial_case()
    T, D, C = rn.dims(forest)
    return [((i, y, x), t) + wc.trace(depth[i], forest[t], D, x, y, scale)
            for i, y, x in wc.live_pixels(depth, labels, C) for t in range(T)]


@functools.lru_cache(maxsize=None)
def _div_ref(scale):
    depth, labels, filt, forest, _ = wc.divide_case()
    counts, totals = rn.count(depth, labels, forest, scale)
    post = pn.posterior(depth, forest, 1, scale, filt, 1)
    _frozen(counts, totals, *post)
    return counts, totals, post


@functools.lru_cache(maxsize=None)
def _counting_ref(name):
    return _frozen(*rn.count(*wc.counting_case(name)))


@functools.lru_cache(maxsize=None)
def _bucket_ref():
    return _frozen(*rn.count(*wc.bucket_case()))


# ------------------------------------------------------------------ CPU: 1. the adversarial walk -----------------------------
def _met(scale):
    """The names of what the live walks of the adversarial case meet at one scale."""
    depth, labels, forest, plants = wc.adversarial_case()
    H, W = wc.ADV["H"], wc.ADV["W"]
    tiny = np.finfo(np.float32).tiny
    met = set()
    for (i, y, x), t, seen, end in _adv_traces(scale):
        if end is None:
            met.add("a walk that falls off")
        for n, st in seen:
            rec = forest[t, n]
            for k in range(4):
                q, num = st["quot"][k], st["num"][k]
                if np.isnan(q):
                    met.add("a NaN quotient")
                elif q >= F32(2147483648.):
                    met.add("a quotient that saturates high")
                elif q < F32(-2147483648.):
                    met.add("a quotient that saturates low")
                if not -2 ** 31 <= st["sums"][k] < 2 ** 31:
                    met.add("an add that wraps")
                if num != 0 and abs(num) < tiny:
                    met.add("a denormal numerator")
                if np.isinf(num) and np.isfinite(rec[k]):
                    met.add("a numerator that s * u overflows")
            for (px, py), v in zip(st["at"], st["val"]):
                if W <= px < 2 * W and 0 <= py < H - 1:             # (y * W + x would be a pixel of the next row)
                    met.add("x past the right border with a row below it")
                if i == 1 and -H <= py < 0 and 0 <= px < W:         # (y * W + x below image 1 would be a pixel of image 0)
                    met.add("a probe of image 1 above row 0")
                if 0 <= px < W and 0 <= py < H:
                    assert v == depth[i, py, px]
                    if v in (0, NO):
                        met.add("a probe on depth 0" if v == 0 else "a probe on 65535")
            if st["f"] == rec[4]:
                met.add("f == thresh")
            if np.isnan(rec[4]):
                met.add("a NaN threshold")
                assert st["side"] == 1
            if np.isinf(rec[4]):
                met.add("a +inf threshold" if rec[4] > 0 else "a -inf threshold")
                assert st["side"] == (0 if rec[4] > 0 else 1)
            for pt, pn_, ps, flag in plants["flags"]:
                if (pt, pn_, ps) == (t, n, st["side"]):
                    met.add(f"the planted flag {flag}")
    return met


@pytest.mark.parametrize("scale", wc.SCALES)
def test_adversarial_case_meets_every_condition(scale):
    """What keeps the GPU tests from passing on a case that contains nothing: at every scale the restatement's live walks meet
    each of the inputs below, pass every planted offset and threshold, and spread over many leaf slots."""
    depth, labels, forest, plants = wc.adversarial_case()
    m = wc.ADV
    T, D, C = rn.dims(forest)
    assert depth.shape == (m["n"], m["H"], m["W"]) and (T, D, C) == (m["T"], m["D"], m["C"]) and depth.size <= 2000
    assert m["W"] % 8 and (m["H"] * m["W"]) % 64                               # a wave spans the two images
    counts, totals, _ = _adv_ref(scale)
    traces = _adv_traces(scale)
    # the walk taken apart ends where refit_numpy.walk ends: its ends give refit_numpy.count's counts
    mine = np.zeros_like(counts)
    for (i, y, x), t, seen, end in traces:
        if end is not None:
            mine[t, end[0], end[1], labels[i, y, x]] += np.uint64(1)
    assert np.array_equal(mine, counts) and sum(e[3] is None for e in traces) == int(totals[3])
    assert all(int(v) > 0 for v in totals) and int(counts.sum()) == T * int(totals[0]) - int(totals[3])
    want = {"a NaN quotient", "a quotient that saturates high", "a quotient that saturates low", "an add that wraps",
            "a denormal numerator", "x past the right border with a row below it", "a probe of image 1 above row 0",
            "a probe on depth 0", "a probe on 65535", "f == thresh", "a NaN threshold", "a +inf threshold", "a -inf threshold",
            "a walk that falls off"} | {f"the planted flag {flag}" for flag in wc.PLANTED_FLAGS}
    if scale == 3.0:
        want.add("a numerator that s * u overflows")
    assert _met(scale) == want
    assert (counts.sum(axis=3) > 0).sum() >= 40                               # distinct leaf slots that take a pixel
    # every planted offset and threshold sits on a node of levels 0 to 2 that live walks pass
    visited = {(t, n) for _, t, seen, _ in traces for n, _ in seen}
    top = (1 << wc.PLANT_LEVELS) - 1
    assert {(t, n) for t in range(T) for n in range(top)} <= visited
    planted = {v for v in _bits(forest[:, :top, 0:4]).ravel().tolist()}
    assert {int(v) for v in _bits(np.array(wc.ADVERSARIAL_OFFSETS, np.float32))} <= planted
    thresholds = {int(v) for v in _bits(forest[:, :top, 4]).ravel()}
    assert {int(v) for v in _bits(np.array(wc.SPECIAL_THRESHOLDS + (65535.5, -65535.0, -65534.5), np.float32))} <= thresholds
    assert (forest[:, top:, 0:4] != 0).any() and np.abs(forest[:, top:, 0:4]).max() < 20000.    # below: small offsets only
    # the flags: -0.5 goes on (its child is visited), the others end the walk in their slot; the "go on" of level D - 1
    for t, n, s, flag in plants["flags"]:
        assert _bits(forest[t, n, 5 + s]) == _bits(F32(flag))
        if flag == -0.5:
            assert (t, 2 * n + 1 + s) in visited and counts[t, n, s].sum() == 0
        else:
            assert counts[t, n, s].sum() > 0 and (t, 2 * n + 1 + s) not in visited
    t, n, s = plants["fall_off"]
    assert forest[t, n, 5 + s] == -1. and prn.level(n) == D - 1 and (t, n) in visited
    assert (forest[:, (1 << (D - 1)) - 1:, 5:7] == -1.).sum() == 1 and all(e[1] == t for e in traces if e[3] is None)


def test_adversarial_numerator_overflows_at_scale_3_only():
    """3e38 and -3e38 are finite numerators at scales 1.0 and 0.5 and infinite ones at 3.0, on nodes that walks pass at each."""
    depth, labels, forest, _ = wc.adversarial_case()
    where = np.argwhere(np.isin(forest[:, :, 0:4], np.array(wc.OVERFLOWS_AT_3, np.float32)))
    assert len(where) >= 2
    for scale in wc.SCALES:
        hits = [st["num"][k] for _, t, seen, _ in _adv_traces(scale) for n, st in seen for tt, nn, k in where.tolist() if (tt, nn) == (t, n)]
        assert hits and all(np.isinf(v) == (scale == 3.0) for v in hits), scale


@pytest.mark.parametrize("scale", wc.SCALES)
def test_adversarial_restatements_equal_the_oracle(scale, oracle):
    """refit_numpy.count against the oracle's evaluator through digit-coded trees, posterior_numpy's labels against
    oracle.eval_forest: the restatements say what the kernels must do on exactly these inputs."""
    from test_refit import _oracle_counts
    depth, labels, forest, _ = wc.adversarial_case()
    counts, totals, (lab, conf, sums) = _adv_ref(scale)
    got, fell = _oracle_counts(oracle, depth, labels, forest, scale)
    assert np.array_equal(got, counts) and fell == int(totals[3])
    want = np.full(depth.shape, NO, np.uint16)
    oracle.eval_forest(depth, forest, want, scale_factor=scale)
    assert np.array_equal(lab, want) and np.array_equal(want != NO, pn.evaluated_mask(depth))
    assert len(np.unique(lab[want != NO])) >= 3 and len(np.unique(conf[want != NO])) >= 20
    if scale == ADV_R2_SCALE:
        filt, cls = wc.adversarial_filter(), wc.ADV["filter_class"]
        lab2, conf2, _ = _adv_ref_r2()
        want = np.full(lab2.shape, NO, np.uint16)
        oracle.eval_forest(depth, forest, want, 2, filt, cls, scale)
        ev = pn.evaluated_mask(depth, 2, filt, cls)
        assert np.array_equal(lab2, want) and np.array_equal(want != NO, ev) and 50 < ev.sum() < ev.size


def test_adversarial_prune_has_something_to_do():
    """Rule P2 prices a "go on" at level D - 1 at no error and no leaf (walks fall off there), so the pruner takes this forest
    as it is, the fall-off plant included: no copy without the plant is needed."""
    depth, labels, forest, plants = wc.adversarial_case()
    counts, totals, _ = _adv_ref(1.0)
    out, cnt, p = prn.prune(forest, counts, 0)
    assert p.report[2] > 0 and p.report[1] < p.report[0] and int(p.report[6]) == int(counts.sum())
    assert not np.array_equal(_bits(out), _bits(forest)) and cnt.sum() == counts.sum()
    t, n, s = plants["fall_off"]
    assert p.reach_before[t, n]


# ------------------------------------------------------------------ CPU: 2. the divide ---------------------------------------
def test_divide_case_is_decided_by_the_last_ulp():
    """For every (numerator, depth, scale) the case was made for: the floor of the correctly rounded quotient is known by
    exact arithmetic, refit_numpy.walk goes to the side that floor gives, and for a third of them and more a quotient one ulp
    nearer to zero gives the other side."""
    depth, labels, filt, forest, combos = wc.divide_case()
    T, D, C = rn.dims(forest)
    assert D == 1 and C == wc.DIV_C and depth.shape == (1, len(wc.DIV_DEPTHS), wc.DIV_W)
    assert depth[0, :, wc.DIV_XC].tolist() == list(wc.DIV_DEPTHS) == [1, 2, 3, 7, 11, 12, 4000, 65534]
    assert sorted(wc.DIV_K) == [-5, -3, -2, -1, 1, 2, 3, 5] and sorted({c[2] for c in combos}) == [0.5, 1.0, 3.0]
    assert np.array_equal(labels > 0, filt == 1) and int((labels > 0).sum()) == len(wc.DIV_DEPTHS)
    changed, per_scale, rounded = 0, {s: 0 for s in wc.SCALES}, 0
    for t, row, scale in combos:
        d, u = wc.DIV_DEPTHS[row], forest[t, 0, 0]
        exact_product = Fraction(float(u)) * Fraction(scale)
        p = F32(np.float64(u) * np.float64(scale))               # (24 bits by 2: the double is exact, one rounding to fp32)
        rounded += Fraction(float(p)) != exact_product
        floor_q = wc.exact_floor_of_rounded_quotient(p, d)
        assert abs(floor_q) <= 6                                  # the probe stays in the row, on a neighbour or the pixel
        side = wc.div_side_of_offset(row, floor_q)
        assert rn.walk(depth[0], forest[t], 1, wc.DIV_XC, row, scale) == (0, side), (float(u), d, scale)
        with np.errstate(all="ignore"):
            towards_zero = np.nextafter(F32(p / F32(d)), F32(0.))
        if wc.div_side_of_offset(row, rn.floor_i32(towards_zero)) != side:
            changed += 1
            per_scale[scale] += 1
    print(f"{len(combos)} combinations on {T} trees; one ulp towards zero changes the side of {changed} ({per_scale}); "
          f"{rounded} products round")
    assert len(combos) >= 3 * 64 * 2 + 64 and rounded == sum(c[2] == 3.0 for c in combos) >= 64
    assert 3 * changed >= len(combos) and all(v > 0 for v in per_scale.values())
    # every tree decides both ways over the rows, and both classes' leaves take pixels
    for scale in wc.SCALES:
        counts, totals, (lab, conf, sums) = _div_ref(scale)
        assert totals.tolist() == [len(wc.DIV_DEPTHS), 0, 0, 0] and counts[:, 0, 0].sum() > 100 and counts[:, 0, 1].sum() > 100
        assert (lab != NO).sum() == len(wc.DIV_DEPTHS) and set(np.unique(lab[lab != NO]).tolist()) == {1, 2}


def test_divide_restatements_equal_the_oracle(oracle):
    depth, labels, filt, forest, _ = wc.divide_case()
    for scale in wc.SCALES:
        want = np.full(depth.shape, NO, np.uint16)
        oracle.eval_forest(depth, forest, want, 1, filt, 1, scale)
        assert np.array_equal(_div_ref(scale)[2][0], want)


# ------------------------------------------------------------------ CPU: 3. the counting paths -------------------------------
def test_lds_levels_of_the_counting_shapes():
    """The launcher's formula on both sides of its `<=`, and on the shapes whose L other tests state in words."""
    assert lds_levels(1, 3, 2048) == 1 and 1 * 1 * 2 * 2048 == kLdsCells       # the histogram exactly full
    assert lds_levels(1, 3, 2049) == 0 and 1 * 1 * 2 * 2049 == kLdsCells + 2
    assert lds_levels(3, 3, 700) == 0 and 3 * 1 * 2 * 700 == 4200 > kLdsCells
    assert lds_levels(1, 10, 4) == 9 and lds_levels(3, 7, 6) == 6 and lds_levels(2, 4, 4) == 4 and lds_levels(1, 1, 3) == 1
    assert lds_levels(wc.BUCKET_TREES, wc.BUCKET["D"], wc.BUCKET["C"]) == 6
    for name, L in (("t1_c2048", 1), ("t1_c2049", 0), ("t3_c700", 0)):
        m = wc.COUNTING[name]
        assert lds_levels(m["T"], m["D"], m["C"]) == L and rn.dims(wc.counting_case(name)[2]) == (m["T"], m["D"], m["C"])


@pytest.mark.parametrize("name", sorted(wc.COUNTING))
def test_counting_cases_contain_what_they_are_meant_to(name):
    depth, labels, forest = wc.counting_case(name)
    T, D, C = rn.dims(forest)
    counts, totals = _counting_ref(name)
    assert wc.find_counting_first(name) == wc.COUNTING_FIRST[name] and depth.shape == (1, 9, 130)
    assert set(np.unique(labels).tolist()) == {0, 1, 2, C // 2, C - 2, C - 1, C}
    assert all(int(v) > 0 for v in totals[:3]) and totals[3] == 0 and int(counts.sum()) == T * int(totals[0])
    per_level = [int(counts[:, (1 << j) - 1:(2 << j) - 1].sum()) for j in range(D)]
    assert per_level[0] > 100 and sum(per_level[1:]) > 100                     # root slots take pixels, and so do deeper ones
    assert (counts[:, 0].sum(axis=(1, 2)) > 0).all()                           # ... of every tree
    for l in (1, 2, C // 2, C - 2, C - 1):
        assert counts[..., l].sum() > 0
    # a wave's 64 pixels: more than kAggIters distinct root-level keys, and keys that several lanes share
    for t, (distinct, shared) in enumerate(wc.root_keys_per_wave(depth, labels, forest)):
        assert distinct > kAggIters and shared >= 3, (t, distinct, shared)


def test_bucket_case_shares_buckets():
    """Cells of one workgroup that want one bucket of its table, by the kernel's own hash: three pairs in a row, three cells in
    a bucket.  One column tree alone cannot give either (its cells under one label are an arithmetic progression, which
    Fibonacci hashing never folds), so the forest is the tree BUCKET_TREES times."""
    depth, labels, forest = wc.bucket_case()
    m = wc.BUCKET
    T, D, C = rn.dims(forest)
    assert (T, D, C) == (wc.BUCKET_TREES, 10, 4) and depth.shape == (1, m["H"], m["W"]) and m["W"] == kThreads
    assert all(len(set(row.tolist())) == 1 for row in labels[0]) and all(a[0] != b[0] for a, b in zip(labels[0], labels[0][1:]))
    assert wc.table_bucket(0) == 0 and wc.table_bucket(1) == 0x9E3779B1 >> 21 and wc.table_bucket((1 << 32) + 5) == wc.table_bucket(5)
    assert wc.bucket_sharing(1) == ([0] * m["H"], [1] * m["H"])               # one tree alone: no pair at all
    assert wc.find_bucket_trees() == wc.BUCKET_TREES
    pairs, most = wc.bucket_sharing(T)
    assert max(pairs) >= 3 and max(most) >= 3, (pairs, most)
    assert T * ((1 << D) - 1) * 2 * C < (1 << 32) - 1                          # use_table
    assert lds_levels(T, D, C) < D - 1                                         # level 9 is below the histogram's levels
    # the cells are the restatement's: the first row's pixels, counted alone
    counts, _ = rn.count(depth[:, :1], labels[:, :1], forest)
    cells = wc.bucket_cells(T)[0]
    assert np.flatnonzero(counts).tolist() == sorted(cells) and len(set(cells)) == T * m["W"] and (counts.ravel()[cells] == 1).all()


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _check_count(rdf, depth, labels, forest, scale, want):
    """LeafRefitter.add against refit_numpy.count: counts and totals, exactly.  Returns the refitter."""
    f = rdf.DecisionForest.from_numpy(forest)
    r = rdf.LeafRefitter(f)
    r.add(rdf.to_device(depth), rdf.to_device(labels), scale)
    got, totals = r.counts.get(), r.totals()
    assert got.dtype == np.uint64 and got.shape == want[0].shape
    assert np.array_equal(got, want[0]), f"{(got != want[0]).sum()} counts differ; first at {np.argwhere(got != want[0])[:5].tolist()}"
    assert list(totals.values()) == [int(v) for v in want[1]]
    assert np.array_equal(_bits(f.forest_cu.get()), _bits(forest))             # counting writes nothing into the forest
    return r


def _gpu_posterior(rdf, depth, forest, r, scale, filt=None, cls=None):
    """get_posteriors_forest with min_conf 0 on outputs pre-filled with 65535: (labels, conf, sums) as numpy."""
    n, h, w = depth.shape
    C = (forest.shape[2] - 7) // 2
    lshape = (n, h // r, w // r)
    lab = rdf.DeviceArray(lshape, np.uint16).fill(NO)
    conf = rdf.DeviceArray(lshape, np.uint16).fill(NO)
    sums = rdf.DeviceArray((n, C) + lshape[1:], np.float32).fill(np.float32(NO))
    rdf.DecisionTreeEvaluator().get_posteriors_forest(
        rdf.DecisionForest.from_numpy(forest), rdf.to_device(depth), lab, conf, sums, labels_reduce=r,
        filter_images=None if filt is None else rdf.to_device(filt), filter_images_class=cls, scale_factor=scale, min_conf=0)
    return lab.get(), conf.get(), sums.get()


def _gpu_labels(rdf, packed, depth, forest, r, scale, filt=None, cls=None):
    out = rdf.DeviceArray((depth.shape[0], depth.shape[1] // r, depth.shape[2] // r), np.uint16).fill(NO)
    rdf.DecisionTreeEvaluator(use_packed=packed).get_labels_forest(
        rdf.DecisionForest.from_numpy(forest), rdf.to_device(depth), out, labels_reduce=r,
        filter_images=None if filt is None else rdf.to_device(filt), filter_images_class=cls, scale_factor=scale)
    return out.get()


def _same(got, want, what):
    same = got == want
    assert same.all(), f"{what}: {(~same).sum()} differ; first at {np.argwhere(~same)[:5].tolist()}"


def _check_posterior(got, want, what):
    """As test_posterior.test_parity_with_the_restatement compares: labels and confidences as integers, sums bit for bit."""
    _same(got[0], want[0], what + ": labels")
    _same(got[1], want[1], what + ": confidence")
    _same(_bits(got[2]), _bits(want[2]), what + ": sums")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", wc.SCALES)
def test_adversarial_refit_counts(scale, rdf, gpu_runtime, monkeypatch):
    depth, labels, forest, _ = wc.adversarial_case()
    counts, totals, _ = _adv_ref(scale)
    r = _check_count(rdf, depth, labels, forest, scale, (counts, totals))
    # one image per call: the per-call pixel limit patched down to a frame and a half; the counts accumulate to the same
    dt = _mod("decision_tree")
    pix = depth.shape[1] * depth.shape[2]
    monkeypatch.setattr(dt, "_PIX_LIMIT", pix * 3 // 2)
    assert dt._image_chunks(depth.shape[0], pix) == [(0, 1), (1, 1)]
    r.reset().add(rdf.to_device(depth), rdf.to_device(labels), scale)
    assert np.array_equal(r.counts.get(), counts) and list(r.totals().values()) == [int(v) for v in totals]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", wc.SCALES)
def test_adversarial_posterior(scale, rdf, gpu_runtime):
    depth, _, forest, _ = wc.adversarial_case()
    T, D, C = rn.dims(forest)
    want = _adv_ref(scale)[2]
    got = _gpu_posterior(rdf, depth, forest, 1, scale)
    _check_posterior(got, want, f"r = 1, scale {scale}")
    # the packed table flags nodes for the exact numerators here, as test_concurrency.adversarial_forest's does
    exact = ctypes.c_int(-1)
    f = rdf.DecisionForest.from_numpy(forest)
    assert gpu_runtime.lib.rdf_forest_info(f.packed(scale).ptr, T, D, C, gpu_runtime.stream(), None, ctypes.byref(exact), None) == 0
    assert exact.value > 0, "the adversarial forest packs without a flagged node"
    # ungated labels are the evaluator's, on both of its paths
    for packed in (True, False):
        _same(got[0], _gpu_labels(rdf, packed, depth, forest, 1, scale), f"use_packed={packed}, scale {scale}")
    if scale == ADV_R2_SCALE:
        filt, cls = wc.adversarial_filter(), wc.ADV["filter_class"]
        got2 = _gpu_posterior(rdf, depth, forest, 2, scale, filt, cls)
        _check_posterior(got2, _adv_ref_r2(), f"r = 2 with a filter, scale {scale}")
        for packed in (True, False):
            _same(got2[0], _gpu_labels(rdf, packed, depth, forest, 2, scale, filt, cls), f"r = 2, use_packed={packed}")


@pytest.mark.gpu
def test_adversarial_prune(rdf, gpu_runtime, oracle):
    """ForestPruner.add, plan and apply on the adversarial forest and frames as they are (rule P2 takes the fall-off plant):
    report, bytes and counts are prune_numpy's of the restatement's counts, and the evaluator on the pruned forest gives the
    oracle's labels of the bytes read back."""
    depth, labels, forest, _ = wc.adversarial_case()
    counts, totals, _ = _adv_ref(1.0)
    out, cnt, p = prn.prune(forest, counts, 0)
    f = rdf.DecisionForest.from_numpy(forest)
    d_cu = rdf.to_device(depth)
    pr = rdf.ForestPruner(f).add(d_cu, rdf.to_device(labels))
    assert np.array_equal(pr.counts.get(), counts) and list(pr.totals().values()) == [int(v) for v in totals]
    report = pr.plan()
    assert list(report.values()) == [int(v) for v in p.report], (report, p.report.tolist())
    assert pr.apply() == report
    pruned = f.forest_cu.get()
    same = _bits(pruned) == _bits(out)
    assert same.all(), f"{(~same).sum()} words differ; first at {np.argwhere(~same)[:5].tolist()}"
    assert np.array_equal(pr.counts.get(), cnt)
    want = np.full(depth.shape, NO, np.uint16)
    oracle.eval_forest(depth, pruned, want)
    for packed in (True, False):
        got = rdf.DeviceArray(depth.shape, np.uint16).fill(NO)
        rdf.DecisionTreeEvaluator(use_packed=packed).get_labels_forest(f, d_cu, got)
        _same(got.get(), want, f"the pruned forest, use_packed={packed}")


@pytest.mark.gpu
@pytest.mark.parametrize("scale", wc.SCALES)
def test_divide_refit_counts(scale, rdf, gpu_runtime):
    depth, labels, filt, forest, _ = wc.divide_case()
    counts, totals, _ = _div_ref(scale)
    _check_count(rdf, depth, labels, forest, scale, (counts, totals))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", wc.SCALES)
def test_divide_posterior(scale, rdf, gpu_runtime):
    """One tree's side is one vote of the sums (whole numbers up to T, exact in fp32): they are compared bit for bit with the
    labels, so that no single wrong side hides behind the argmax."""
    depth, labels, filt, forest, _ = wc.divide_case()
    _check_posterior(_gpu_posterior(rdf, depth, forest, 1, scale, filt, 1), _div_ref(scale)[2], f"scale {scale}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wc.COUNTING))
def test_counting_paths(name, rdf, gpu_runtime):
    """L = 1 with the histogram exactly full, L = 0 (even the root's slots go through the wave's key groups and the table),
    L = 0 with trees whose first cell is not cell 0; class ids up to 2048."""
    depth, labels, forest = wc.counting_case(name)
    _check_count(rdf, depth, labels, forest, 1.0, _counting_ref(name))


@pytest.mark.gpu
def test_bucket_held_by_another_cell(rdf, gpu_runtime):
    """Cells of one workgroup that want the same bucket: whichever arrives first holds it and the others go to global memory
    as 64-bit atomics.  Which one holds it depends on arrival order; the counts must not, from run to run either."""
    depth, labels, forest = wc.bucket_case()
    want = _bucket_ref()
    r = _check_count(rdf, depth, labels, forest, 1.0, want)
    first = r.counts.get()
    r.reset()
    assert not r.counts.get().any()
    r.add(rdf.to_device(depth), rdf.to_device(labels))
    assert np.array_equal(r.counts.get(), first) and list(r.totals().values()) == [int(v) for v in want[1]]
