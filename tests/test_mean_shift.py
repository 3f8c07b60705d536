"""mean-shift modes of the composite label map + fingertip heights.
CPU: the numpy restatement against hand-derived answers.  GPU (-m gpu): rdf_mean_shift /
rdf_fingertip_heights against the restatement within 1e-9 (the reference's own fp64 atomics are
order-dependent, so this row has no bit-exact target), plus run-to-run bitwise reproducibility."""
import importlib

import numpy as np
import pytest

import mean_shift_cases as mc
from oracle import mean_shift_numpy as ms_np


def _label_map(seed=3, h=120, w=212, n_classes=6, absent=(5,)):
    rng = np.random.default_rng(seed)
    lab = np.full((h, w), 65535, dtype=np.uint16)
    yy, xx = np.mgrid[0:h, 0:w]
    for c in range(1, n_classes + 1):
        if c in absent:
            continue
        cx, cy = rng.uniform(20, w - 20), rng.uniform(15, h - 15)
        a, b = rng.uniform(4, 14), rng.uniform(4, 14)
        m = ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1
        lab[m] = c
        for _ in range(3):   # outliers that the kernel weighting should discount
            lab[rng.integers(0, h), rng.integers(0, w)] = c
    lab[0, 0] = 0
    lab[1, 1] = 60000        # label beyond num_classes: ignored here (the reference would fault)
    return lab


def test_known_answers_numpy():
    # one pixel per class: round 0 puts the mean on it, later rounds shift by exactly 0 (diff = 0, weight 1)
    lab = np.zeros((5, 7), np.uint16)
    lab[2, 3], lab[4, 6] = 1, 2
    m = ms_np.mean_shift(lab, 3, [1.0, 2.0, 3.0], 6)
    assert m[0].tolist() == [3.0, 2.0] and m[1].tolist() == [6.0, 4.0] and np.isnan(m[2]).all()
    # two pixels of a class, symmetric: the centroid is a fixed point (shifts cancel exactly)
    lab = np.zeros((1, 9), np.uint16)
    lab[0, 2] = lab[0, 6] = 1
    m = ms_np.mean_shift(lab, 1, [2.0], 4)
    assert m[0].tolist() == [4.0, 0.0]
    # zero rounds: the zero-initialised means come back (mean_shift.py:33)
    assert (ms_np.mean_shift(lab, 1, [2.0], 0) == 0).all()
    # height: identity plane => -z ; mean (10.9, 5.2) truncates to pixel (10, 5), times labels_reduce 2
    depth = np.arange(40 * 60, dtype=np.uint16).reshape(40, 60)
    hts = ms_np.fingertip_heights(np.array([[10.9, 5.2], [np.nan, 1.0], [100.0, 3.0]]), [1, 2, 3], depth, 2,
                                  400.0, 400.0, 30.0, 20.0, np.eye(4, dtype=np.float32))
    assert hts[0] == -float(depth[10, 20]) and np.isnan(hts[1]) and np.isnan(hts[2])


@pytest.mark.gpu
def test_mean_shift_matches_restatement_and_is_reproducible(rdf, gpu_runtime):
    msmod = importlib.import_module("3d-beats_amd.cuda.mean_shift")
    ms = msmod.MeanShift()
    for seed, (h, w), L in [(3, (120, 212), 6), (4, (240, 424), 7), (5, (33, 65), 2), (6, (480, 848), 6)]:
        lab = _label_map(seed, h, w, L, absent=(min(5, L),))
        var = np.linspace(6.0, 14.0, L).astype(np.float32)
        dl, dv = rdf.to_device(lab[None]), rdf.to_device(var)
        for rounds in (0, 1, 6):
            got = ms.run(rounds, dl, L, dv)
            want = ms_np.mean_shift(lab, L, var, rounds)
            assert got.shape == (L, 2) and got.dtype == np.float64
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.abs(got[ok] - want[ok]).max() < 1e-9, (seed, rounds, np.abs(got[ok] - want[ok]).max())
            again = ms.run(rounds, dl, L, dv)
            assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "not bitwise reproducible"


@pytest.mark.gpu
def test_fingertip_heights_match_restatement(rdf, gpu_runtime):
    msmod = importlib.import_module("3d-beats_amd.cuda.mean_shift")
    rng = np.random.default_rng(9)
    depth = rdf.synth.frames(["dense"], 77, 480, 848)[0]
    means = np.array([[100.7, 50.2], [423.9, 239.9], [424.0, 10.0], [-0.5, 3.0], [np.nan, 1.0], [12.0, 240.0], [0.0, 0.0]])
    plane = (np.eye(4) + 0.1 * rng.standard_normal((4, 4))).astype(np.float32)
    ids = [1, 2, 3, 4, 5, 6, 7]
    got = msmod.fingertip_heights(rdf.to_device(means), ids, rdf.to_device(depth), 2, 421.3, 420.9, 423.1, 238.6, plane)
    want = ms_np.fingertip_heights(means, ids, depth, 2, 421.3, 420.9, 423.1, 238.6, plane)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-6, atol=1e-6), (got, want)
    assert np.isnan(want[[2, 4, 5]]).all() and not np.isnan(want[[0, 1, 3, 6]]).any()


@pytest.mark.gpu
def test_mean_shift_class_bigger_than_the_lds_list(rdf, gpu_runtime):
    """A class with more pixels than one workgroup lists in LDS (32 768): the rest is rescanned from the label image every
    round -- same means (1e-9 px), still bitwise reproducible; a neighbouring small class is unaffected."""
    msmod = importlib.import_module("3d-beats_amd.cuda.mean_shift")
    ms = msmod.MeanShift()
    h, w, L = 240, 424, 3
    rng = np.random.default_rng(12)
    lab = np.full((h, w), 1, np.uint16)                 # class 1: ~97 000 pixels
    lab[rng.random((h, w)) < 0.03] = 65535
    lab[100:130, 200:260] = 2                           # class 2: 1 800 pixels; class 3 absent
    lab[0, 0] = 0
    var = np.array([80.0, 9.0, 5.0], np.float32)
    dl, dv = rdf.to_device(lab[None]), rdf.to_device(var)
    assert (lab == 1).sum() > 2 * 32768
    for rounds in (1, 5):
        got = ms.run(rounds, dl, L, dv)
        want = ms_np.mean_shift(lab, L, var, rounds)
        assert np.isnan(got[2]).all() and np.isnan(want[2]).all()
        assert np.abs(got[:2] - want[:2]).max() < 1e-9, np.abs(got[:2] - want[:2]).max()
        assert np.array_equal(got.view(np.uint64), ms.run(rounds, dl, L, dv).view(np.uint64))


@pytest.mark.gpu
def test_mean_shift_and_heights_in_one_launch_equal_the_two_calls(rdf, gpu_runtime):
    """rdf_mean_shift_heights (what HandPipeline uses): the same means and the same heights, bit for bit, as rdf_mean_shift
    followed by rdf_fingertip_heights -- with ids that name no class (0, L + 1), an id whose class has no pixel (NaN mode),
    repeated ids, outputs in device memory and in pinned host memory the kernel writes directly."""
    import torch
    msmod = importlib.import_module("3d-beats_amd.cuda.mean_shift")
    ms = msmod.MeanShift()
    h, w, L, r = 240, 424, 6, 2
    lab = _label_map(23, h, w, L, absent=(4,))
    depth = rdf.synth.frames(["dense"], 91, h * r, w * r)[0]
    var = np.full(L, 10.0, np.float32)
    plane = (np.eye(4) + 0.1 * np.random.default_rng(5).standard_normal((4, 4))).astype(np.float32)
    ids = np.array([1, 6, 4, 0, 7, 2, 2, 5, 3], np.int32)
    intr = (421.3, 420.9, 423.1, 238.6)
    dl, dv, dd = rdf.to_device(lab[None]), rdf.to_device(var), rdf.to_device(depth)
    d_ids, d_plane = rdf.to_device(ids), rdf.to_device(plane)
    for rounds in (1, 6):
        means = ms.run_device(rounds, dl, L, dv)
        want_m = means.get()
        want_h = msmod.fingertip_heights(means, [int(i) for i in ids], dd, r, *intr, plane)
        # device outputs
        out = rdf.DeviceArray((2 * L + len(ids),), np.float64).fill(7.0)
        ms.run_device_with_heights(rounds, dl, L, dv, d_ids, len(ids), dd, r, intr, d_plane, out.ptr, out.ptr + 16 * L)
        got = out.get()
        assert np.array_equal(got[:2 * L].view(np.uint64), want_m.reshape(-1).view(np.uint64))
        assert np.array_equal(got[2 * L:].view(np.uint64), np.asarray(want_h).view(np.uint64)), (got[2 * L:], want_h)
        assert np.isnan(want_h[[2, 3, 4]]).all() and not np.isnan(want_h[[0, 1, 5, 6, 7, 8]]).any()
        # pinned host outputs, written by the kernel
        host = gpu_runtime.alloc_host_mapped((2 * L + len(ids)) * 8)
        assert host is not None
        host[2].view(np.float64)[:] = 7.0
        ms.run_device_with_heights(rounds, dl, L, dv, d_ids, len(ids), dd, r, intr, d_plane, host[1], host[1] + 16 * L)
        torch.cuda.synchronize()
        assert np.array_equal(host[2].view(np.float64).view(np.uint64), got.view(np.uint64))


@pytest.mark.gpu
def test_null_labels_are_refused_not_dereferenced(rdf, gpu_runtime):
    """The one-launch kernel lists every class's pixels whatever the number of rounds: a NULL label image (or variances)
    is an argument error, also with num_rounds = 0."""
    lib = gpu_runtime.lib
    var = rdf.to_device(np.full(4, 10.0, np.float32))
    means = rdf.DeviceArray((4, 2), np.float64)
    lab = rdf.to_device(np.zeros((1, 8, 8), np.uint16))
    assert lib.rdf_mean_shift(None, 8, 8, 4, var.ptr, 0, means.ptr, None, gpu_runtime.stream()) == -2
    assert lib.rdf_mean_shift(lab.ptr, 8, 8, 4, None, 0, means.ptr, None, gpu_runtime.stream()) == -2
    assert lib.rdf_mean_shift(lab.ptr, 8, 8, 4, var.ptr, 0, means.ptr, None, gpu_runtime.stream()) == 0
    assert lib.rdf_mean_shift(None, 0, 8, 4, var.ptr, 0, means.ptr, None, gpu_runtime.stream()) == 0   # no pixel to read


# ---- the branches no camera-sized, 16-byte-aligned input reaches (inputs: tests/mean_shift_cases.py) ----

RDF_OK, RDF_ERR_BAD_ARG, RDF_ERR_NULL_PTR = 0, -1, -2      # include/rdf_hip.h
BOUND_PX = 1e-9                                            # the row's bound against the restatement (module docstring)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def _canon(a):
    """The bits, every NaN as the one quiet NaN: 0 / 0 has no sign or payload that both a CPU and a GPU must agree on."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


def _offset_labels(rdf, lab, k):
    """The label image on the device, starting k elements (2k bytes) past a 16-byte boundary."""
    flat = np.concatenate([np.full(k, 7, np.uint16), lab.reshape(-1)])
    return rdf.to_device(flat).view(np.uint16)[k:].reshape((1,) + lab.shape)


def _ms():
    return importlib.import_module("3d-beats_amd.cuda.mean_shift").MeanShift()


def _check_against_restatement(ms, dl, dv, case, name):
    """Every number of rounds of the case: NaN where the restatement has NaN, within 1e-9 px elsewhere, the same bits twice."""
    trace = mc.restatement_trace(name)
    got_by_rounds = {}
    for rounds in case.rounds:
        got = ms.run(rounds, dl, case.L, dv)
        want = trace[rounds - 1]
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, rounds, got, want)
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
        print(f"{name} rounds={rounds}: max |kernel - restatement| = {err:.3e} px")
        assert err < BOUND_PX, (name, rounds, err)
        assert np.array_equal(_bits(got), _bits(ms.run(rounds, dl, case.L, dv))), "not bitwise reproducible"
        got_by_rounds[rounds] = got
    return got_by_rounds


def test_restatement_inputs_meet_the_preconditions_and_its_own_error_is_small():
    """CPU.  The kernel's table weight exp(-a) * exp(-b) and the restatement's exp(-(a + b)) agree to a few ulp only while
    neither is subnormal, and a mode is weights' sum away from 0/0.  So for every part-2 input, class, round and pixel:
      - where the kernel uses its tables (dim_x + dim_y <= 3072 and v * v > 0) the exponent is above -600 (every factor and
        the product are normal numbers) or below -800 (the product and the single exponential are both exactly 0);
      - where it does not, kernel and restatement evaluate the same single exponential, and the band cannot separate them:
        there (the 65 535-pixel row and column of one class at variance 100 cross the band) the weights inside the band must
        move the mode by less than 1e-200 px in all;
      - every round's weight sum is 0 or at least 1e-6 -- or NaN where v * v == 0 puts a pixel on the mean (exp(-0/0)), which
        makes the mode NaN in any arithmetic.
    These are conditions on the inputs, not measurements.  Then the restatement's own rounding: each input again with
    np.longdouble coordinates and weights and math.fsum sums; the two agree within 1e-11 px, 100 times under the 1e-9 bound.
    (Where np.longdouble is fp64, the exact sums alone are the yardstick: they remove the error that grows with the pixels.)"""
    for name in mc.RESTATEMENT_CASES:
        case = mc.restatement_case(name)
        trace = mc.restatement_trace(name)
        R = max(case.rounds)
        tables = mc.uses_tables(case)
        for c in range(case.L):
            ys, xs = np.nonzero(case.labels == c + 1)
            if xs.size == 0:
                assert all(np.isnan(t[c]).all() for t in trace)
                continue
            v2 = np.float64(np.float32(case.variances[c] * case.variances[c]))
            for rnd in range(1, R):
                mx, my = trace[rnd - 1][c]
                if np.isnan(mx) or np.isnan(my):
                    assert np.isnan(trace[rnd][c]).all()     # NaN stays NaN whatever the weights
                    continue
                dx, dy = xs - mx, ys - my
                with np.errstate(invalid="ignore", divide="ignore"):
                    e = -((dx * dx) + (dy * dy)) / (2 * v2)
                    p = np.exp(e)
                if v2 == 0:
                    assert not tables[c] and (np.isnan(e) | (e == -np.inf)).all(), (name, c, rnd)
                elif tables[c]:
                    assert ((e > -600) | (e < -800)).all(), (name, c, rnd, e[(e <= -600) & (e >= -800)])
                else:
                    band = (e <= -600) & (e >= -800)
                    moved = (np.abs(dx[band]) + np.abs(dy[band])) @ p[band] / p.sum()
                    assert moved < 1e-200, (name, c, rnd, moved)
                sw = p.sum()
                assert sw == 0 or sw >= 1e-6 or (np.isnan(sw) and v2 == 0), (name, c, rnd, sw)
        longs = mc.mean_shift_long(case.labels, case.L, case.variances, R)
        for rnd in range(R):
            want, lng = trace[rnd], longs[rnd].astype(np.float64)
            assert np.array_equal(np.isnan(want), np.isnan(lng)), (name, rnd, want, lng)
            ok = ~np.isnan(want)
            if ok.any():
                assert np.abs(want[ok] - lng[ok]).max() <= 1e-11, (name, rnd, np.abs(want[ok] - lng[ok]).max())


def test_restatement_answers_the_issue_states():
    """CPU.  What the restatement gives for the underflow, symmetric and zero-variance inputs, as far as it is known by hand."""
    t = mc.restatement_trace("clean_underflow")
    assert t[0][0].tolist() == [286.5, 3.0] and np.isnan(t[1][0]).all() and np.isnan(t[2][0]).all()
    assert np.isfinite(t[2][1]).all()                                  # the class next to it is an ordinary one
    assert all(np.isfinite(r).all() for r in mc.restatement_trace("partial_underflow"))
    assert np.abs(mc.restatement_trace("row_65535")[2][0] - [32767.0, 0.0]).max() < 1e-9
    assert np.abs(mc.restatement_trace("column_65535")[2][0] - [0.0, 32767.0]).max() < 1e-9
    t = mc.restatement_trace("zero_variance")
    assert np.isfinite(t[0]).all()
    for r in (1, 2):
        assert np.isnan(t[r][:4]).all() and np.isfinite(t[r][4]).all()
    # the two table-boundary images hold the same blobs: same modes up to the rounding of the sums
    a, b = mc.restatement_trace("tables_3069"), mc.restatement_trace("no_tables_3070")
    assert np.array_equal(np.isnan(a[3]), np.isnan(b[3])) and np.nanmax(np.abs(a[3] - b[3])) < 1e-9
    # exact centroids: the restatement's round 0 is the integer answer too
    lab, picks = mc.one_pixel_per_class()
    w = lab.shape[1]
    assert mc.exact_centroids(lab, 64).tolist() == [[float(p % w), float(p // w)] for p in picks]
    for n1 in (mc.LIST_CAP - 1, mc.LIST_CAP, mc.LIST_CAP + 1):
        assert np.array_equal(_canon(mc.exact_centroids(mc.list_cap_image(n1), 3)), _canon(mc.restatement_trace(f"cap_{n1}")[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.RANDOM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_0_is_the_exact_centroid_random_images_at_the_class_limit(rdf, gpu_runtime, shape):
    """64 classes, labels 0, 65, 66 and 65535 to ignore, two classes absent, at label pointers 0 to 14 bytes past a 16-byte
    boundary (offset 0: the vector lister; the others: the scalar one): one round is float64(sum x) / float64(n) bit for
    bit.  Three rounds at every offset: the restatement within 1e-9 px, and the same bits whatever the pointer."""
    ms = _ms()
    h, w = shape
    name = f"random_{h}x{w}"
    case = mc.restatement_case(name)
    want = mc.exact_centroids(case.labels, case.L)
    assert np.isnan(want[[c - 1 for c in mc.RANDOM_ABSENT]]).all()
    dv = rdf.to_device(case.variances)
    later = None
    for k in mc.OFFSETS:
        dl = _offset_labels(rdf, case.labels, k)
        assert dl.ptr % 16 == 2 * k
        got = ms.run(1, dl, case.L, dv)
        assert np.array_equal(_canon(got), _canon(want)), (shape, k, np.flatnonzero(_canon(got) != _canon(want))[:8])
        got3 = _check_against_restatement(ms, dl, dv, case, name)[3]
        later = got3 if later is None else later
        assert np.array_equal(_bits(got3), _bits(later)), (shape, k, "the list order depends on the pointer")


@pytest.mark.gpu
def test_one_pixel_per_class_lands_on_the_pixel(rdf, gpu_runtime):
    """64 classes of one pixel each at the seams of the lister (lane, step, wave round, batch, tail, row ends): the mean is
    (p % w, p // w) exactly after one round, and after three (the shift is 0 / 1) -- with per-pixel exponentials on this
    image, and with the tables on the same pixels in a (36, 3036) image."""
    ms = _ms()
    lab, picks = mc.one_pixel_per_class()
    var = np.linspace(0.5, 9.0, 64).astype(np.float32)
    dv = rdf.to_device(var)
    for shape in (lab.shape, (36, 3036)):
        h, w = shape
        assert h * w >= lab.size and (h + w <= mc.TAB_CAP) == (shape != lab.shape)
        img = np.full(h * w, mc.NO_LABEL, np.uint16)
        img[:lab.size] = lab.reshape(-1)
        img = img.reshape(h, w)
        want = np.array([[p % w, p // w] for p in picks], np.float64)
        for k in (0, 3):
            dl = _offset_labels(rdf, img, k)
            for rounds in (1, 3):
                got = ms.run(rounds, dl, 64, dv)
                assert np.array_equal(_canon(got), _canon(want)), (shape, k, rounds, np.flatnonzero((got != want).any(1)))


@pytest.mark.gpu
def test_list_cap_edges_exact_centroids_and_later_rounds(rdf, gpu_runtime):
    """A class of 32 767, 32 768 (listed) and 32 769 pixels (not listed: rescanned), the cap inside one lane's eight pixels,
    and two classes over the cap at once: exact centroids after one round; four rounds against the restatement; the small
    class after the big one gives the same bits whether the big one overflows or not."""
    ms = _ms()
    small = []
    for name in [f"cap_{n}" for n in (mc.LIST_CAP - 1, mc.LIST_CAP, mc.LIST_CAP + 1)] + ["both_over_cap"]:
        case = mc.restatement_case(name)
        dv = rdf.to_device(case.variances)
        for k in (0, 1):
            dl = _offset_labels(rdf, case.labels, k)
            got = ms.run(1, dl, case.L, dv)
            assert np.array_equal(_canon(got), _canon(mc.exact_centroids(case.labels, case.L))), (name, k, got)
            got4 = _check_against_restatement(ms, dl, dv, case, name)[4]
            if name.startswith("cap_"):
                small.append(got4[1])
    assert all(np.array_equal(_bits(s), _bits(small[0])) for s in small), small


@pytest.mark.gpu
def test_round_loop_trip_edges(rdf, gpu_runtime):
    """A class of exactly n pixels around one entry per thread (1024) and one four-entry trip per thread (4096): exact
    centroid after one round, the restatement after three."""
    ms = _ms()
    for n in mc.TRIP_COUNTS:
        name = f"count_{n}"
        case = mc.restatement_case(name)
        assert (case.labels == 1).sum() == n
        dl, dv = _offset_labels(rdf, case.labels, 0), rdf.to_device(case.variances)
        got = ms.run(1, dl, case.L, dv)
        assert np.array_equal(_canon(got), _canon(mc.exact_centroids(case.labels, case.L))), (n, got)
        _check_against_restatement(ms, dl, dv, case, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tables_3069", "no_tables_3070", "row_65535", "column_65535", "zero_variance",
                                  "partial_underflow"])
def test_later_rounds_match_the_restatement(rdf, gpu_runtime, name):
    """Both sides of the table limit (dim_x + dim_y = 3072 and 3073) on the same blobs; the largest dim_x and dim_y with one
    class over every pixel (rescanned, one exp per pixel); v * v == 0 (NaN from the second round on, the same NaN pattern);
    one far pixel whose weight underflows to exactly 0."""
    case = mc.restatement_case(name)
    dl, dv = _offset_labels(rdf, case.labels, 0), rdf.to_device(case.variances)
    _check_against_restatement(_ms(), dl, dv, case, name)


@pytest.mark.gpu
def test_weights_that_all_underflow_reset_the_fingertip(rdf, gpu_runtime):
    """Two blobs 550 columns apart at variance 3: (286.5, 3) after one round, then every weight is 0 and the mode is NaN, as
    in the restatement -- and the fused call's height for that id is NaN, the neighbouring class's is a number."""
    ms = _ms()
    name = "clean_underflow"
    case = mc.restatement_case(name)
    dl, dv = _offset_labels(rdf, case.labels, 0), rdf.to_device(case.variances)
    got = _check_against_restatement(ms, dl, dv, case, name)
    assert got[1][0].tolist() == [286.5, 3.0] and np.isnan(got[2][0]).all() and np.isnan(got[3][0]).all()
    h, w = case.labels.shape
    depth = np.full((h, w), 1000, np.uint16)
    ids = np.array([1, 2], np.int32)
    out = rdf.DeviceArray((2 * case.L + 2,), np.float64).fill(7.0)
    ms.run_device_with_heights(3, dl, case.L, dv, rdf.to_device(ids), 2, rdf.to_device(depth), 1, (300.0, 300.0, 300.0, 4.0),
                               rdf.to_device(np.eye(4, dtype=np.float32)), out.ptr, out.ptr + 16 * case.L)
    res = out.get()
    assert np.array_equal(_bits(res[:4]), _bits(got[3]))
    assert np.isnan(res[4]) and res[5] == -1000.0, res


# ---- heights and argument limits ----

def _height_inputs(n_ids, r):
    """means [L, 2] with every kind of mode the kernel must refuse or truncate, ids with repeats, 0 and L + 1, a depth frame
    with 0 and 65535 under two of the modes."""
    rng = np.random.default_rng(100 + n_ids + r)
    h, w = 48, 80
    lw, lh = w // r, h // r                 # the label map's size: modes below it are on the frame
    inf = np.inf
    special = [(inf, 1.0), (1.0, -inf), (-inf, inf), (1e9, 1.0), (1.0, -1e9), (-1e9, 1.0), (999999999.0, 1.0),
               (1.0, 999999999.0), (np.nan, 1.0), (1.0, np.nan), (-0.5, -0.9), (-0.99, 3.2), (2.5, -0.25), (-1.0, 2.0),
               (3.7, -1.2), (float(lw), 1.0), (1.0, float(lh)), (lw - 0.01, lh - 0.01), (0.0, 0.0), (1.5, 2.5), (3.25, 1.75)]
    regular = np.stack([rng.uniform(0, lw, 12), rng.uniform(0, lh, 12)], axis=1)
    means = np.concatenate([np.array(special, np.float64), regular])
    L = means.shape[0]
    depth = rng.integers(1, 65535, size=(h, w)).astype(np.uint16)
    depth[int(2.5) * r, int(1.5) * r] = 0               # under mode (1.5, 2.5)
    depth[int(1.75) * r, int(3.25) * r] = 65535         # under mode (3.25, 1.75)
    ids = rng.integers(0, L + 2, size=n_ids).astype(np.int32)
    ids[:L + 2] = rng.permutation(L + 2)                # every class, 0 and L + 1 at least once; the rest repeats
    ids[-1] = 19                                        # (0, 0): a number, in the last block
    plane = (np.eye(4) + 0.1 * rng.standard_normal((4, 4))).astype(np.float32)
    return means, L, depth, ids, plane, (41.3, 40.9, 39.1, 23.6)


def _height_tolerance(means, ids, depth, r, intr, plane):
    """|error| of the four-term fp64 dot product whatever its order or fusing: 4 eps * sum |plane[2][k] * pt[k]| (the fp32
    steps before it are single IEEE operations, the same on both sides)."""
    fx, fy, ppx, ppy = (np.float32(v) for v in intr)
    tol = np.zeros(len(ids))
    for i, c in enumerate(ids):
        if not 1 <= c <= len(means) or not np.isfinite(means[c - 1]).all() or (np.abs(means[c - 1]) >= 1e9).any():
            continue
        px, py = int(means[c - 1][0]) * r, int(means[c - 1][1]) * r
        if 0 <= px < depth.shape[1] and 0 <= py < depth.shape[0]:
            z = np.float32(depth[py, px])
            pt = np.array([float(z * ((np.float32(px) - ppx) / fx)), float(z * ((np.float32(py) - ppy) / fy)), float(z), 1.0])
            tol[i] = 4 * np.finfo(np.float64).eps * np.abs(plane[2].astype(np.float64) * pt).sum()
    return tol


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("n_ids", [64, 65, 200])
def test_fingertip_heights_past_the_first_block_and_at_the_limits_of_a_mode(rdf, gpu_runtime, n_ids, r):
    """One, two and four blocks of 64 ids.  Modes that are infinite, NaN, 1e9 or beyond (NaN by the kernel's rule), 999999999
    (NaN through the bounds check), negative fractions (truncate to 0: on the frame), exactly one past the last pixel;
    depth 0 and 65535 under the mode; ids 0 and L + 1; labels_reduce 1 and 4.  Every id's height is written once, by its
    own thread."""
    means, L, depth, ids, plane, intr = _height_inputs(n_ids, r)
    want = ms_np.fingertip_heights(means, [int(i) for i in ids], depth, r, *intr, plane)
    by_class = ms_np.fingertip_heights(means, list(range(1, L + 1)), depth, r, *intr, plane)
    assert np.isnan(by_class[:10]).all() and np.isnan(by_class[13:17]).all()
    assert np.isfinite(by_class[10:13]).all() and np.isfinite(by_class[17:]).all()
    assert np.isnan(want[(ids == 0) | (ids == L + 1)]).all() and np.isfinite(want[-1])
    out = rdf.DeviceArray((n_ids + 2,), np.float64).fill(7.0)
    d_means, d_ids, d_depth, d_plane = (rdf.to_device(a) for a in (means, ids, depth, plane))
    rc = gpu_runtime.lib.rdf_fingertip_heights(d_means.ptr, L, d_ids.ptr, n_ids, d_depth.ptr, depth.shape[1], depth.shape[0],
                                               r, *intr, d_plane.ptr, out.ptr + 8, gpu_runtime.stream())
    assert rc == RDF_OK
    res = out.get()
    assert res[0] == 7.0 and res[-1] == 7.0
    got = res[1:-1]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (np.flatnonzero(np.isnan(got) != np.isnan(want)), got, want)
    ok = ~np.isnan(want)
    tol = _height_tolerance(means, ids, depth, r, intr, plane)
    assert (np.abs(got[ok] - want[ok]) <= tol[ok]).all(), (np.abs(got[ok] - want[ok]).max(), tol[ok].min())


@pytest.mark.gpu
def test_argument_limits_of_the_mean_shift_calls(rdf, gpu_runtime):
    """n_ids = 1024 (one per thread of a workgroup) in the fused call equals the two calls bit for bit, 1025 is refused;
    65 classes and a dimension of 65 536 are refused (64 classes and 65 535 run: the tests above); a refused call writes
    nothing."""
    msmod = importlib.import_module("3d-beats_amd.cuda.mean_shift")
    ms = msmod.MeanShift()
    lib, stream = gpu_runtime.lib, gpu_runtime.stream()
    L, r, n_ids = 6, 2, 1024
    lab = _label_map(31, 40, 70, L, absent=(3,))
    depth = np.random.default_rng(8).integers(0, 65536, size=(40 * r, 70 * r)).astype(np.uint16)
    ids = np.random.default_rng(9).integers(0, L + 2, size=n_ids + 1).astype(np.int32)
    plane = (np.eye(4) + 0.1 * np.random.default_rng(10).standard_normal((4, 4))).astype(np.float32)
    intr = (61.3, 60.9, 70.1, 38.6)
    dl, dv, dd = rdf.to_device(lab[None]), rdf.to_device(np.full(L, 6.0, np.float32)), rdf.to_device(depth)
    d_ids, d_plane = rdf.to_device(ids), rdf.to_device(plane)
    means = ms.run_device(3, dl, L, dv)
    want_m = means.get()
    want_h = msmod.fingertip_heights(means, [int(i) for i in ids[:n_ids]], dd, r, *intr, plane)
    assert np.isnan(want_h).any() and np.isfinite(want_h[-8:]).any()
    out = rdf.DeviceArray((2 * L + n_ids + 1,), np.float64).fill(7.0)
    ms.run_device_with_heights(3, dl, L, dv, d_ids, n_ids, dd, r, intr, d_plane, out.ptr, out.ptr + 16 * L)
    got = out.get()
    assert np.array_equal(_bits(got[:2 * L]), _bits(want_m)) and got[-1] == 7.0
    assert np.array_equal(_bits(got[2 * L:-1]), _bits(want_h)), np.flatnonzero(_bits(got[2 * L:-1]) != _bits(want_h))

    out.fill(7.0)
    args = (dv.ptr, 3, out.ptr, d_ids.ptr)
    tail = (dd.ptr, 70 * r, 40 * r, r, *intr, d_plane.ptr, out.ptr + 16 * L, stream)
    assert lib.rdf_mean_shift_heights(dl.ptr, 70, 40, L, *args, n_ids + 1, *tail) == RDF_ERR_BAD_ARG
    big = rdf.to_device(np.full(65, 6.0, np.float32))
    out65 = rdf.DeviceArray((2 * 65,), np.float64).fill(7.0)
    assert lib.rdf_mean_shift(dl.ptr, 70, 40, 65, big.ptr, 1, out65.ptr, None, stream) == RDF_ERR_BAD_ARG
    assert lib.rdf_mean_shift(dl.ptr, 65536, 1, L, dv.ptr, 1, out.ptr, None, stream) == RDF_ERR_BAD_ARG
    assert lib.rdf_mean_shift(dl.ptr, 1, 65536, L, dv.ptr, 1, out.ptr, None, stream) == RDF_ERR_BAD_ARG
    assert lib.rdf_mean_shift_heights(dl.ptr, 65536, 1, L, *args, 4, *tail) == RDF_ERR_BAD_ARG
    assert (out.get() == 7.0).all() and (out65.get() == 7.0).all()
    assert lib.rdf_mean_shift(dl.ptr, 70, 40, 64, big.ptr, 1, out65.ptr, None, stream) == RDF_OK
    m64 = out65.get()
    assert np.array_equal(_canon(m64[:2 * L]), _canon(mc.exact_centroids(lab, L))) and np.isnan(m64[2 * L:128]).all()
    assert (m64[128:] == 7.0).all()
