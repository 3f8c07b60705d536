"""Soft modes (rdf_labels_composite_weights / rdf_labels_weighted_modes of librdf_labels.so, soft_modes.WeightedModes,
LayeredDecisionForest.composite_weights[_batch], HandPipeline / BeatsSession with soft_modes=True) against the numpy restatement in
tests/soft_modes_numpy.py.  The CPU tests pin the restatement to answers worked by hand, check the preconditions under which the
kernel's factorised weights and the restatement's single exponential agree, the restatement's own rounding, the header, the
bindings and the argument checks (which launch nothing).  On the GPU the weights and round 0 are bit for bit, later rounds
within BOUND_PX = 1e-9 px (the bound of the mean-shift row), every result is the same bits twice, and without weights every
round is the mean shift's bits (one kernel body, csrc/rdf_modes.hpp)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import mean_shift_cases as mc
import posterior_cases as pc
import posterior_numpy as pn
import session_cases as sc
import soft_modes_cases as smc
import soft_modes_numpy as sn
from abi_helpers import declared, exported
from oracle import mean_shift_numpy as ms_np

NO = 65535
BOUND_PX = smc.BOUND_PX
NEW = ("rdf_labels_composite_weights", "rdf_labels_weighted_modes", "rdf_labels_weighted_modes_list_cap")


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def _canon(a):
    """The bits, every NaN as the one quiet NaN (0 / 0 has no sign or payload a CPU and a GPU must agree on)."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_hand_worked_modes():
    lab = np.zeros((1, 9), np.uint16)
    lab[0, 2] = lab[0, 6] = 1

    def round0(w2, w6):
        w = np.zeros((1, 9), np.uint16)
        w[0, 2], w[0, 6] = w2, w6
        return sn.weighted_modes(lab, w, 1, [2.0], 1)[0]
    assert round0(7, 7).tolist() == [4.0, 0.0] and round0(65535, 65535).tolist() == [4.0, 0.0]
    assert round0(3, 1).tolist() == [3.0, 0.0]                       # (3 * 2 + 1 * 6) / 4
    assert round0(9, 0).tolist() == [2.0, 0.0] and round0(65535, 0).tolist() == [2.0, 0.0]
    assert np.isnan(round0(0, 0)).all()
    assert sn.weighted_modes(lab, None, 1, [2.0], 1)[0].tolist() == [4.0, 0.0]          # no weights: every weight 1
    assert (sn.weighted_modes(lab, None, 1, [2.0], 0) == 0).all()                        # zero rounds: zeros
    # equal weights: the centroid is a fixed point of the later rounds (the shifts cancel exactly); one pixel stays put
    assert sn.weighted_modes(lab, np.full((1, 9), 5, np.uint16), 1, [2.0], 4)[0].tolist() == [4.0, 0.0]
    w = np.zeros((1, 9), np.uint16)
    w[0, 6] = 40000
    assert sn.weighted_modes(lab, w, 1, [2.0], 6)[0].tolist() == [6.0, 0.0]
    # the restatement without weights is the mean-shift restatement
    blob = smc.blob_labels(3, 40, 70, 3)
    a, b = sn.weighted_modes(blob, None, 3, [6., 7., 8.], 4), ms_np.mean_shift(blob, 3, [6., 7., 8.], 4)
    assert np.abs(a - b).max() < 1e-12


def test_hand_worked_weights():
    cond = [[0, 1], [1, 2], [0, 2], [0, 3]]           # layer 0: 1 final, 2 goes on at offset 2; layer 1: 1 and 2 final
    one = lambda v: np.full((1, 1), v, np.uint16)
    k = one(12345)
    out, written = sn.composite_weights([one(1)], [k], cond, prefill=7)
    assert out.tolist() == [[12345]] and written.all()                                   # one layer: w == conf
    out, _ = sn.composite_weights([one(2), one(1)], [one(65535), one(65535)], cond)
    assert out.tolist() == [[65535]]
    out, _ = sn.composite_weights([one(2), one(2)], [one(32768), one(32768)], cond)
    assert out.tolist() == [[(32768 * 32768 + 32767) // 65535]] == [[16384]]
    out, _ = sn.composite_weights([one(2), one(1)], [one(0), one(65535)], cond)
    assert out.tolist() == [[0]]                                                         # 0 absorbs
    out, _ = sn.composite_weights([one(2), one(1)], [one(40000), one(65535)], cond)
    assert out.tolist() == [[40000]]                                                     # 65535 is neutral
    # nothing is written: label 0, 65535, an entry off the table, a walk that falls off the last layer, a stop in layer 1
    for labs in ([one(0)], [one(NO)], [one(5)], [one(2)], [one(2), one(NO)], [one(2), one(3)]):
        out, written = sn.composite_weights(labs, [k] * len(labs), cond, prefill=7)
        assert out.tolist() == [[7]] and not written.any(), labs
    # the mirror
    labs = np.array([[1, 0, 2]], np.uint16)
    conf = np.array([[10, 20, 30]], np.uint16)
    out, written = sn.composite_weights([labs, np.array([[0, 0, 1]], np.uint16)], [conf, one(65535).repeat(3, 1)], cond, True, 7)
    assert out.tolist() == [[30, 7, 10]] and written.tolist() == [[True, False, True]]


def test_weight_cases_contain_what_they_are_meant_to(oracle):
    """The written set equals the set where the oracle's composite (plus the mirror) writes a label, for every shape, number of
    layers and mirror; every special confidence and every way of not being written occurs."""
    cond = np.array(smc.COND, np.int32)
    for shape in smc.WEIGHT_SHAPES:
        labels, conf = smc.weights_case(shape)
        for nl in (1, 2, 3):
            for flip in (False, True):
                out, written = smc.weights_answer(shape, nl, flip)
                for i in range(shape[0]):
                    comp = np.full(shape[1:], smc.PREFILL, np.uint16)
                    oracle.composite([a[i] for a in labels[:nl]], cond, comp)
                    comp = comp[:, ::-1] if flip else comp
                    assert np.array_equal(comp != smc.PREFILL, written[i]), (shape, nl, flip, i)
                assert (out[~written] == smc.PREFILL).all()
    labels, conf = smc.weights_case((2, 61, 130))
    assert set(smc.SPECIAL_CONF) <= set(np.unique(conf[0]).tolist()) and len(np.unique(conf[1])) > 1000
    assert {0, NO, 200} <= set(np.unique(labels[0]).tolist())
    out3, w3 = smc.weights_answer((2, 61, 130), 3, False)
    out1, w1 = smc.weights_answer((2, 61, 130), 1, False)
    assert w1.sum() < w3.sum() < w3.size and (out3[w3] == 0).any() and (out3[w3] == 65535).any()
    assert smc.weights_answer((1, 1, 1), 2, False)[0].tolist() == [[[16384]]] and not smc.weights_answer((1, 1, 1), 1, False)[1].any()


def test_mode_cases_meet_the_preconditions_and_the_restatements_error_is_small():
    """Conditions on the inputs, as for the unweighted row: where the kernel uses its tables every exponent is above -600 (factors
    and product are normal numbers) or below -800 (both forms are exactly 0); every sum of w g is 0 or at least 1e-6.  Then the
    restatement's own rounding: each input again in np.longdouble with math.fsum sums, within 1e-11 px, 100 times under the bound."""
    for name in smc.case_names():
        c = smc.case(name)
        tr = smc.trace(name)
        R = max(c.rounds)
        tables = smc.uses_tables(c)
        for k in range(c.L):
            ys, xs = np.nonzero((c.labels == k + 1) & (c.weights != 0))
            if xs.size == 0:
                assert all(np.isnan(t[k]).all() for t in tr)
                continue
            om = c.weights[ys, xs].astype(np.float64)
            v2 = np.float64(np.float32(c.variances[k] * c.variances[k]))
            if v2 == 0:       # exp(-d / 0): 0 off the mean, NaN on it -- NaN from the second round on in any arithmetic
                assert not tables[k] and np.isfinite(tr[0][k]).all() and all(np.isnan(t[k]).all() for t in tr[1:]), (name, k)
                continue
            for rnd in range(1, R):
                mx, my = tr[rnd - 1][k]
                assert np.isfinite(mx) and np.isfinite(my)
                dx, dy = xs - mx, ys - my
                e = -((dx * dx) + (dy * dy)) / (2 * v2)
                if tables[k]:
                    assert ((e > -600) | (e < -800)).all(), (name, k, rnd)
                else:
                    assert (e > -600).all(), (name, k, rnd)
                sw = (om * np.exp(e)).sum()
                assert sw == 0 or sw >= 1e-6, (name, k, rnd, sw)
        longs = sn.weighted_modes_long(c.labels, c.weights, c.L, c.variances, R)
        for rnd in range(R):
            want, lng = tr[rnd], longs[rnd].astype(np.float64)
            assert np.array_equal(np.isnan(want), np.isnan(lng)), (name, rnd)
            ok = ~np.isnan(want)
            assert np.abs(want[ok] - lng[ok]).max() <= 1e-11, (name, rnd, np.abs(want[ok] - lng[ok]).max())
    # what the cases are there for
    cap = smc.CAP_FOR_CPU
    counted = lambda n: int(((smc.case(n).labels == 1) & (smc.case(n).weights != 0)).sum())
    assert [counted(n) for n in ("cap_-1_zeros_0", "cap_+0_zeros_0", "cap_+1_zeros_0", "cap_+1_zeros_2", "cap_+2_zeros_2")] \
        == [cap - 1, cap, cap + 1, cap - 1, cap]
    assert int((smc.case("cap_+1_zeros_2").labels == 1).sum()) == cap + 1
    both = smc.case("both_over_cap")
    assert all(int(((both.labels == k) & (both.weights != 0)).sum()) > cap for k in (1, 2))
    assert smc.uses_tables(smc.case("tables_3069"))[0] and not smc.uses_tables(smc.case("no_tables_3070"))[0]
    assert np.isnan(smc.trace("blobs_120x212")[0][4]).all() and smc.case("narrow_45x7").labels.shape[1] < 8
    assert [smc.case(n).labels.shape for n in ("wrap_9x8", "wrap_7x9", "wrap_5x15")] == [(9, 8), (7, 9), (5, 15)]
    for name in ("blobs_33x65", "blobs_120x212", "blobs_240x424"):
        c = smc.case(name)
        on = c.weights[(c.labels >= 1) & (c.labels <= c.L)]
        assert (on == 0).any() and (on == 1).any() and (on == 65535).any() and len(np.unique(on)) > 50


def _prototypes():
    rec = _mod("_build").LIBRARIES["labels"]
    text = re.sub(r"/\*.*?\*/", "", open(rec.headers[0]).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int|uint32_t)\s+(rdf_labels_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if name not in NEW:
            continue
        args = []
        for p in (q.strip() for q in params.split(",")):
            if p == "void":
                continue
            args.append(ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float") else ctypes.c_int)
            assert "*" in p or p.split()[0] in ("float", "int"), p
        out[name] = ({"int": ctypes.c_int, "uint32_t": ctypes.c_uint32}[ret], args)
    return out


def test_header_bindings_and_exports_agree(rdf):
    build, lib_mod = _mod("_build"), _mod("_lib")
    build.build()
    rec = build.LIBRARIES["labels"]
    assert os.path.basename(rec.sources[-1]) == "soft_modes_hip.hip"
    names = declared(rec.headers[0])
    assert set(NEW) <= set(names) and exported(rec.so) == names == sorted(lib_mod.BINDINGS["labels"][1])
    protos = _prototypes()
    for name in NEW:
        assert lib_mod.BINDINGS["labels"][1][name] == protos[name], name
    assert len(protos[NEW[0]][1]) == 11 and len(protos[NEW[1]][1]) == 23 and protos[NEW[2]] == (ctypes.c_uint32, [])
    lib = lib_mod.load("labels")
    assert lib.rdf_labels_abi_version() == 1                                  # pure additions
    assert lib.rdf_labels_weighted_modes_list_cap() == smc.CAP_FOR_CPU >= 16384
    # the list and the per-round tables fit a compute unit's 160 KB
    assert smc.CAP_FOR_CPU * 6 + smc.TAB_CAP * 8 + 1024 <= 160 * 1024


def test_rejected_arguments_launch_nothing(rdf):
    """Rule S8, clause by clause.  Rejected arguments launch nothing, so they need no device; the pointers are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    P = lambda a: ctypes.c_void_p(a)
    BAD, NULL, LARGE = -1, -2, -3

    def cw(ll=P(0x10000), lc=P(0x20000), nl=2, n=1, w=8, h=8, cond=P(0x30000), nc=4, flip=0, out=P(0x40000)):
        return lib.rdf_labels_composite_weights(ll, lc, nl, n, w, h, cond, nc, flip, out, None)
    for kw in (dict(nl=0), dict(nl=-1), dict(n=-1), dict(w=-8), dict(h=-8), dict(nc=-1), dict(w=65536), dict(h=65536),
               dict(ll=P(0x10004)), dict(lc=P(0x20004)), dict(cond=P(0x30002)), dict(out=P(0x40001))):
        assert cw(**kw) == BAD, kw
    assert cw(n=32768, w=256, h=256) == LARGE and cw(n=1, w=65535, h=65535) == LARGE
    assert cw(n=0, ll=None, lc=None, cond=None, out=None) == 0 and cw(w=0) == 0 and cw(h=0) == 0
    for k in ("ll", "lc", "cond", "out"):
        assert cw(**{k: None}) == NULL, k

    def wm(lab=P(0x10000), wts=P(0x20000), n=1, w=8, h=8, L=3, var=P(0x30000), rounds=2, means=P(0x40000), ids=P(0x50000), n_ids=2,
           depth=P(0x60000), dw=16, dh=16, r=2, plane=P(0x70000), hts=P(0x80000), stride=2):
        return lib.rdf_labels_weighted_modes(lab, wts, n, w, h, L, var, rounds, means, ids, n_ids, depth, dw, dh, r, 1., 1., 0., 0.,
                                             plane, hts, stride, None)
    for kw in (dict(n=-1), dict(w=-8), dict(h=-8), dict(L=0), dict(L=65), dict(L=-1), dict(w=65536), dict(h=65536), dict(rounds=-1),
               dict(n_ids=-1), dict(n_ids=1025, stride=1025), dict(dw=-1), dict(dh=-1), dict(r=0), dict(stride=1),
               dict(lab=P(0x10001)), dict(wts=P(0x20001)), dict(var=P(0x30002)), dict(means=P(0x40004)), dict(ids=P(0x50002)),
               dict(depth=P(0x60001)), dict(plane=P(0x70002)), dict(hts=P(0x80004))):
        assert wm(**kw) == BAD, kw
    assert wm(n=32768, w=256, h=256) == LARGE and wm(n=65536, w=1, h=1) == LARGE and wm(n=2, dw=32768, dh=32768) == LARGE
    assert wm(n=0, lab=None, var=None, means=None, ids=None, depth=None, plane=None, hts=None) == 0 and wm(w=0) == 0 and wm(h=0) == 0
    for k in ("lab", "var", "means", "ids", "depth", "plane", "hts"):
        assert wm(**{k: None}) == NULL, k
    # without ids the height arguments are not looked at
    assert wm(n_ids=0, lab=None, ids=None, depth=None, plane=None, hts=None, r=0, stride=0, dw=-1) == NULL
    assert wm(n_ids=0, n=0, ids=None, depth=None, plane=None, hts=None, r=0, stride=0, dw=-1) == 0


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _offset(rdf, a, k):
    """The map on the device as [1, h, w], starting k elements (2k bytes) past a 16-byte boundary."""
    flat = np.concatenate([np.full(k, 7, np.uint16), a.reshape(-1)])
    dev = rdf.to_device(flat).view(np.uint16)[k:].reshape((1,) + a.shape[-2:])
    assert dev.ptr % 16 == 2 * k % 16
    return dev


def _wm(rdf):
    wm = rdf.WeightedModes()
    assert wm.list_cap == smc.CAP_FOR_CPU, "tests/soft_modes_cases.py builds its cap cases for another cap than the library's"
    return wm


@pytest.mark.gpu
@pytest.mark.parametrize("shape", smc.WEIGHT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_composite_weights_bit_exact(shape, rdf, gpu_runtime):
    lib = _mod("_lib").load("labels")
    labels, conf = smc.weights_case(shape)
    d_lab, d_conf = [rdf.to_device(a) for a in labels], [rdf.to_device(a) for a in conf]
    cond = rdf.to_device(np.array(smc.COND, np.int32))
    n, h, w = shape
    for nl in (1, 2, 3):
        tables = rdf.to_device(np.array([[a.ptr for a in d_lab[:nl]], [a.ptr for a in d_conf[:nl]]], np.int64))
        for flip in (False, True):
            want, written = smc.weights_answer(shape, nl, flip)
            out = rdf.DeviceArray((n * h * w + 2,), np.uint16).fill(smc.PREFILL)
            rc = lib.rdf_labels_composite_weights(tables.ptr, tables.ptr + 8 * nl, nl, n, w, h, cond.ptr, len(smc.COND), int(flip),
                                                  out.ptr + 2, gpu_runtime.stream())
            assert rc == 0
            got = out.get()
            assert got[0] == smc.PREFILL and got[-1] == smc.PREFILL
            got = got[1:-1].reshape(shape)
            same = got == want
            assert same.all(), (shape, nl, flip, int((~same).sum()), np.argwhere(~same)[:5].tolist())
            assert np.array_equal(got != smc.PREFILL, written) or (want[written] == smc.PREFILL).any()


@pytest.mark.gpu
def test_without_weights_and_with_uniform_weights_it_is_the_mean_shift(rdf, gpu_runtime):
    """Both kernels are one body (csrc/rdf_modes.hpp): with every weight 1 -- no weight map, or a map of ones -- the weighted
    policy multiplies by 1.0 where the unweighted one does nothing, and while a class is under both list caps it sums the same
    entries in the same order: the mean shift's bits at every round.  Other uniform weights round in the later rounds."""
    ms = _mod("cuda.mean_shift").MeanShift()
    wm = _wm(rdf)
    for seed, (h, w), L in ((5, (33, 65), 2), (3, (120, 212), 6)):
        lab = smc.blob_labels(seed, h, w, L, absent=(5,) if L > 4 else ())
        assert max(int((lab == k).sum()) for k in range(1, L + 1)) < min(wm.list_cap, mc.LIST_CAP) // 4      # far below both caps
        var = rdf.to_device(np.linspace(6.0, 14.0, L).astype(np.float32))
        dl = rdf.to_device(lab[None])
        ones = rdf.to_device(np.ones((1, h, w), np.uint16))
        for rounds in (1, 2, 6, 7):                                  # round 0 alone, then through rounds 1, 5 and 6
            want = ms.run(rounds, dl, L, var)
            got = wm.run(rounds, dl, None, L, var)
            assert got.shape == (L, 2) and got.dtype == np.float64
            assert np.array_equal(_canon(got), _canon(want)), (h, w, rounds, got, want)
            if rounds == 6:
                assert np.array_equal(_canon(wm.run(rounds, dl, ones, L, var)), _canon(want)), (h, w, got, want)
        unweighted = wm.run(1, dl, None, L, var)
        for k in (1, 7, 65535):
            got = wm.run(1, dl, rdf.to_device(np.full((1, h, w), k, np.uint16)), L, var)
            assert np.array_equal(_canon(got), _canon(unweighted)), k


@pytest.mark.gpu
def test_without_weights_heights_and_frames_are_the_mean_shifts(rdf, gpu_runtime):
    """Three frames in one launch with the heights riding on it: WeightedModes without a weight map against
    MeanShift.run_device_with_heights_batch, means and heights bit for bit."""
    ms = _mod("cuda.mean_shift").MeanShift()
    wm = _wm(rdf)
    h, w, L, r = 33, 65, 2, 2
    labs = rdf.to_device(np.stack([smc.blob_labels(5 + i, h, w, L) for i in range(3)]))
    depths = rdf.to_device(np.stack([smc.height_inputs(h, w, r, 80 + i)[0] for i in range(3)]))
    _, plane, intr = smc.height_inputs(h, w, r, 80)
    ids = np.array([2, 1, 3, 0, 2], np.int32)                        # 3 and 0 name no class
    d_ids, d_plane, dv = rdf.to_device(ids), rdf.to_device(plane), rdf.to_device(np.array([5.0, 7.0], np.float32))
    out = {}
    for name in ("weighted", "mean_shift"):
        means = rdf.DeviceArray((3, L, 2), np.float64).fill(7.0)
        hts = rdf.DeviceArray((3, len(ids)), np.float64).fill(7.0)
        if name == "weighted":
            wm.run_device_with_heights(6, labs, None, L, dv, d_ids, len(ids), depths, r, intr, d_plane, means.ptr, hts.ptr, len(ids))
        else:
            ms.run_device_with_heights_batch(6, labs, L, dv, d_ids, len(ids), depths, r, intr, d_plane, means.ptr, hts.ptr, len(ids))
        out[name] = (means.get(), hts.get())
    (m_w, h_w), (m_s, h_s) = out["weighted"], out["mean_shift"]
    assert np.isfinite(m_s).all() and np.isfinite(h_s[:, [0, 1, 4]]).all() and np.isnan(h_s[:, [2, 3]]).all()
    assert np.array_equal(_canon(m_w), _canon(m_s)), (m_w, m_s)
    assert np.array_equal(_canon(h_w), _canon(h_s)), (h_w, h_s)


@pytest.mark.gpu
def test_one_pixel_per_class_is_the_mode(rdf, gpu_runtime):
    wm = _wm(rdf)
    h, w, L = 37, 130, 9
    rng = np.random.default_rng(2)
    picks = [0, 7, 8, h * w - 1, w - 1, w, 511, 512] + [int(rng.integers(0, h * w))]
    lab = np.full(h * w, NO, np.uint16)
    lab[picks] = np.arange(1, L + 1)
    assert len(set(picks)) == L
    wts = rng.integers(1, 65536, h * w).astype(np.uint16)
    wts[picks[:3]] = (1, 65535, 2)
    want = np.array([[p % w, p // w] for p in picks], np.float64)
    var = rdf.to_device(np.linspace(0.5, 9.0, L).astype(np.float32))
    for k in (0, 3):
        dl, dw = _offset(rdf, lab.reshape(h, w), k), _offset(rdf, wts.reshape(h, w), k)
        for rounds in (1, 2, 6, 7):
            got = wm.run(rounds, dl, dw, L, var)
            assert np.array_equal(_bits(got), _bits(want)), (k, rounds, got)


def _check(wm, dl, dw, dv, c, name):
    """Every number of rounds of the case: round 0 the restatement's bits, later rounds NaN where it has NaN and within the bound
    elsewhere, the same bits twice.  Returns {rounds: means}."""
    tr = smc.trace(name)
    out = {}
    for rounds in c.rounds:
        got = wm.run(rounds, dl, dw, c.L, dv)
        want = tr[rounds - 1]
        assert got.shape == want.shape
        if rounds == 1:
            assert np.array_equal(_canon(got), _canon(want)), (name, got, want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, rounds, got, want)
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
        print(f"{name} rounds={rounds}: max |kernel - restatement| = {err:.3e} px")
        assert err < BOUND_PX, (name, rounds, err)
        assert np.array_equal(_bits(got), _bits(wm.run(rounds, dl, dw, c.L, dv))), "not bitwise reproducible"
        out[rounds] = got
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blobs_33x65", "blobs_120x212", "blobs_240x424", "narrow_45x7", "wrap_9x8", "wrap_7x9", "wrap_5x15"])
def test_random_blobs_and_weights(name, rdf, gpu_runtime):
    """(narrow_45x7: rows under eight pixels, the lister's write-out that wraps more than once; wrap_*: the narrowest rows of the
    unrolled write-out, a lane's eight pixels exactly a row or wrapping once.)"""
    wm = _wm(rdf)
    c = smc.case(name)
    dv = rdf.to_device(c.variances)
    base = _check(wm, _offset(rdf, c.labels, 0), _offset(rdf, c.weights, 0), dv, c, name)
    for k in smc.OFFSETS:                                            # the scalar lister gives a lane the same eight pixels
        dl, dw = _offset(rdf, c.labels, k), _offset(rdf, c.weights, 8 - k)
        for rounds in c.rounds:
            assert np.array_equal(_bits(wm.run(rounds, dl, dw, c.L, dv)), _bits(base[rounds])), (name, k, rounds)
    # labels aligned and weights not, and the other way round
    for kl, kw in ((0, 3), (5, 0)):
        got = wm.run(6, _offset(rdf, c.labels, kl), _offset(rdf, c.weights, kw), c.L, dv)
        assert np.array_equal(_bits(got), _bits(base[6])), (kl, kw)


@pytest.mark.gpu
def test_list_cap_edges(rdf, gpu_runtime):
    wm = _wm(rdf)
    cap = wm.list_cap
    small = []
    names = [n for n in smc.case_names(cap) if n.startswith("cap_")] + ["both_over_cap"]
    assert len(names) == 6
    for name in names:
        c = smc.case(name, cap)
        dv = rdf.to_device(c.variances)
        for k in (0, 1):
            got = _check(wm, _offset(rdf, c.labels, k), _offset(rdf, c.weights, k), dv, c, name)
            if name.startswith("cap_") and name.endswith("zeros_0"):
                small.append(got[4][1])
    # the small class next to the big one gives the same bits whether the big one is listed or rescanned
    assert len(small) == 6 and all(np.array_equal(_bits(s), _bits(small[0])) for s in small)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tables_3069", "no_tables_3070"])
def test_both_sides_of_the_table_limit(name, rdf, gpu_runtime):
    c = smc.case(name)
    _check(_wm(rdf), _offset(rdf, c.labels, 0), _offset(rdf, c.weights, 0), rdf.to_device(c.variances), c, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scattered_5x21301", "scattered_4x53253", "batches_cross_cap"])
def test_maps_of_more_than_one_lister_batch(name, rdf, gpu_runtime):
    """The lister takes 16 x 13 x 512 = 106 496 pixels a batch: one batch and a 9-pixel tail, two batches and a tail, and on the
    latter a class that crosses the cap inside batch 0, one that crosses it in batch 1 and one without a pixel in batch 0
    (asserted where the case is built).  The count carried from batch to batch gives every entry its slot: round 0 bit for bit,
    later rounds within the bound, the same bits twice and from misaligned pointers."""
    wm = _wm(rdf)
    c = smc.case(name, wm.list_cap)
    assert c.labels.size > smc.BATCH and not any(smc.uses_tables(c))
    dv = rdf.to_device(c.variances)
    base = _check(wm, _offset(rdf, c.labels, 0), _offset(rdf, c.weights, 0), dv, c, name)
    for kl, kw in ((3, 3), (0, 5), (7, 0)):
        got = wm.run(3, _offset(rdf, c.labels, kl), _offset(rdf, c.weights, kw), c.L, dv)
        assert np.array_equal(_bits(got), _bits(base[3])), (name, kl, kw)
    # without weights it is the mean shift on the same map: the same centroids, bit for bit
    ms = _mod("cuda.mean_shift").MeanShift()
    dl = rdf.to_device(c.labels[None])
    assert np.array_equal(_canon(wm.run(1, dl, None, c.L, dv)), _canon(ms.run(1, dl, c.L, dv)))


@pytest.mark.gpu
def test_zero_variance_is_nan_from_the_second_round_on(rdf, gpu_runtime):
    """v * v == 0 (the other side of `tables`): one exp per pixel, exp(-d / 0) is 0 off the mean and NaN on it; the NaN pattern of
    the restatement, and the ordinary class next to them within the bound."""
    c = smc.case("zero_variance")
    assert not any(smc.uses_tables(c)[:4]) and smc.uses_tables(c)[4]
    got = _check(_wm(rdf), _offset(rdf, c.labels, 0), _offset(rdf, c.weights, 0), rdf.to_device(c.variances), c, "zero_variance")
    for rounds in (2, 3):
        assert np.isnan(got[rounds][:4]).all() and np.isfinite(got[rounds][4]).all()
    assert np.isfinite(got[1]).all()


def _heights_call(rdf, wm, rounds, dl, dw, L, dv, ids, depth, r, intr, plane, n=1, stride=None):
    """(means [n, L, 2], heights buffer [n * stride + 2] with a guard element at both ends) of run_device_with_heights."""
    stride = len(ids) if stride is None else stride
    means = rdf.DeviceArray((n, L, 2), np.float64).fill(7.0)
    hts = rdf.DeviceArray((n * stride + 2,), np.float64).fill(7.0)
    wm.run_device_with_heights(rounds, dl, dw, L, dv, rdf.to_device(ids), len(ids), rdf.to_device(depth), r, intr, rdf.to_device(plane),
                               means.ptr, hts.ptr + 8, stride)
    return means, hts.get()


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 2])
def test_heights_are_fingertip_heights_of_the_same_means(r, rdf, gpu_runtime):
    msmod = _mod("cuda.mean_shift")
    wm = _wm(rdf)
    c = smc.case("blobs_120x212")
    h, w = c.labels.shape
    depth, plane, intr = smc.height_inputs(h, w, r, 70 + r)
    ids = np.array([1, 6, 5, 0, 7, 2, 2, 4, 3, -1], np.int32)           # class 5 absent; 0, 7 and -1 name no class
    dl, dw, dv = rdf.to_device(c.labels[None]), rdf.to_device(c.weights[None]), rdf.to_device(c.variances)
    for rounds in (1, 6):
        means, res = _heights_call(rdf, wm, rounds, dl, dw, c.L, dv, ids, depth, r, intr, plane)
        assert np.array_equal(_bits(means.get()), _bits(wm.run(rounds, dl, dw, c.L, dv)))
        want = msmod.fingertip_heights(means.reshape((c.L, 2)), [int(i) for i in ids], rdf.to_device(depth), r, *intr, plane)
        assert res[0] == 7.0 and res[-1] == 7.0
        assert np.array_equal(_bits(res[1:-1]), _bits(want)), (res[1:-1], want)
        assert np.isnan(want[[2, 3, 4, 9]]).all() and np.isfinite(want[[0, 1, 5, 6, 7, 8]]).all()
        ref = ms_np.fingertip_heights(means.get().reshape(c.L, 2), [int(i) for i in ids], depth, r, *intr, plane)
        assert np.array_equal(np.isnan(ref), np.isnan(want)) and np.allclose(ref[~np.isnan(ref)], want[~np.isnan(ref)], rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
def test_empty_classes_give_nan_modes_and_heights(rdf, gpu_runtime):
    wm = _wm(rdf)
    c = smc.case("blobs_33x65")
    h, w = c.labels.shape
    wts = c.weights.copy()
    wts[c.labels == 1] = 0                                          # class 1: pixels, all of weight 0; class 3: no pixels
    depth, plane, intr = smc.height_inputs(h, w, 1, 9)
    ids = np.array([1, 2, 3], np.int32)
    dv = rdf.to_device(np.array([5.0, 7.0, 6.0], np.float32))
    for rounds in (1, 6):
        means, res = _heights_call(rdf, wm, rounds, rdf.to_device(c.labels[None]), rdf.to_device(wts[None]), 3, dv, ids, depth, 1, intr, plane)
        m = means.get()[0]
        assert np.isnan(m[0]).all() and np.isfinite(m[1]).all() and np.isnan(m[2]).all()
        assert np.isnan(res[1]) and np.isfinite(res[2]) and np.isnan(res[3]) and res[0] == res[4] == 7.0
        want = sn.weighted_modes(c.labels, wts, 3, [5.0, 7.0, 6.0], rounds)
        assert np.abs(m[1] - want[1]).max() < BOUND_PX
    zero_rounds = wm.run(0, rdf.to_device(c.labels[None]), rdf.to_device(wts[None]), 3, dv)
    assert (zero_rounds == 0).all()


@pytest.mark.gpu
def test_three_frames_in_one_launch_equal_three_calls(rdf, gpu_runtime):
    wm = _wm(rdf)
    h, w, L, r = 33, 65, 2, 2                                       # 33 * 65 is odd: frames 1 and 2 start off a 16-byte boundary
    labs = np.stack([smc.blob_labels(5 + i, h, w, L) for i in range(3)])
    wts = np.stack([smc.random_weights(60 + i, (h, w)) for i in range(3)])
    depths = np.stack([smc.height_inputs(h, w, r, 80 + i)[0] for i in range(3)])
    _, plane, intr = smc.height_inputs(h, w, r, 80)
    ids = np.array([2, 1, 3], np.int32)
    dv = rdf.to_device(np.array([5.0, 7.0], np.float32))
    stride = 5
    for weighted in (True, False):
        dw = rdf.to_device(wts) if weighted else None
        means, res = _heights_call(rdf, wm, 6, rdf.to_device(labs), dw, L, dv, ids, depths, r, intr, plane, n=3, stride=stride)
        body = res[1:-1].reshape(3, stride)
        assert res[0] == 7.0 and res[-1] == 7.0 and (body[:, 3:] == 7.0).all()          # the gaps stay untouched
        for i in range(3):
            m1, r1 = _heights_call(rdf, wm, 6, rdf.to_device(labs[i:i + 1]), rdf.to_device(wts[i:i + 1]) if weighted else None, L, dv,
                                   ids, depths[i], r, intr, plane)
            assert np.array_equal(_bits(means.get()[i]), _bits(m1.get())), i
            assert np.array_equal(_bits(body[i, :3]), _bits(r1[1:-1])), i
            assert np.isfinite(r1[1:3]).all() and np.isnan(r1[3])
        got = wm.run(6, rdf.to_device(labs), dw, L, dv)
        assert got.shape == (3, L, 2) and np.array_equal(_bits(got), _bits(means.get()))


# ------------------------------------------------------------------ plumbing -------------------------------------------------
GATES = (pc.LAYERED_GATE, (0, 0))
_answers = {}


def _prepared(frame, flip):
    """What rdf_prepare_hand_depth hands the stack for a camera frame whose every reading belongs to the hand: 0 -> 65535,
    mirrored for the left hand."""
    d = np.where(frame == 0, NO, frame).astype(np.uint16)
    return np.ascontiguousarray(d[:, ::-1]) if flip else d


def _answer(oracle, k, gate, flip=False, prepared=False):
    """stack_answer of layered frame k (as given, or as the pipeline prepares it) plus the restatement's weight map of the
    composite (`weights`, `written`: mirrored when flip); computed once, shared, read-only."""
    key = (k, gate, flip, prepared)
    if key not in _answers:
        case = pc.layered_case()
        frame = _prepared(case[4][k], flip) if prepared else case[4][k]
        a = pc.stack_answer(pn, oracle, case, frame, gate)
        a["weights"], a["written"] = sn.composite_weights(a["labels"], a["conf"], case[2], flip, smc.PREFILL)
        for v in a.values():
            for arr in (v if isinstance(v, list) else [v]):
                arr.setflags(write=False)
        _answers[key] = a
    return _answers[key]


def _stack(rdf, gate):
    f0, f1, conditions, colors, _ = pc.layered_case()
    cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                      {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
           "conditions": conditions, "label_colors": colors}
    lf = rdf.LayeredDecisionForest(cfg, (pc.LAYERED["H"], pc.LAYERED["W"]), pc.LAYERED["R"])
    lf.min_conf = gate
    return lf


@pytest.mark.gpu
@pytest.mark.parametrize("gate", GATES, ids=["rejecting", "zero"])
def test_stack_composite_weights(gate, rdf, gpu_runtime, oracle):
    frames = pc.layered_case()[4]
    H, W, R = pc.LAYERED["H"], pc.LAYERED["W"], pc.LAYERED["R"]
    lf = _stack(rdf, gate)
    dbuf, lbuf = rdf.GpuBuffer((H, W), np.uint16), rdf.GpuBuffer((H // R, W // R), np.uint16)
    wbuf = rdf.GpuBuffer((H // R, W // R), np.uint16)
    for k, frame in enumerate(frames):
        dbuf.cu().set(frame)
        for flip in (False, True):
            want = _answer(oracle, k, gate, flip)
            assert want["written"].any() and not want["written"].all()
            assert gate != (0, 0) or len(np.unique(want["weights"][want["written"]])) >= 5      # (on the CPU: the reference's own)
            if flip:
                lf.run_hand(dbuf, lbuf, 0.75, flip_x=True)
            else:
                lf.run(dbuf, lbuf, 0.75)
            wbuf.cu().fill(smc.PREFILL)
            lf.composite_weights(wbuf, flip_x=flip)
            assert np.array_equal(lbuf.cu().get(), want["hand"] if flip else want["composite"])
            assert np.array_equal(wbuf.cu().get(), want["weights"]), (k, flip)
            assert np.array_equal(lbuf.cu().get() != NO, want["written"])           # a weight wherever the composite has a label
    # the batch: frames 0, 1, 0 mirrored
    order = (0, 1, 0)
    labels = rdf.DeviceArray((3, H // R, W // R), np.uint16).fill(7)
    weights = rdf.DeviceArray((3, H // R, W // R), np.uint16).fill(smc.PREFILL)
    lf.run_hand_batch(rdf.to_device(frames[list(order)]), labels, 0.75, flip_x=True)
    tables = lf._batch_weight_ptrs_cu.ptr
    lf.composite_weights_batch(3, weights, flip_x=True)
    for i, k in enumerate(order):
        want = _answer(oracle, k, gate, True)
        assert np.array_equal(weights.get()[i], want["weights"]) and np.array_equal(labels.get()[i], want["hand"]), i
        for layer in range(2):
            assert np.array_equal(lf.batch_conf_images[layer].get()[i], want["conf"][layer])
    lf.run_hand_batch(rdf.to_device(frames), labels[:2], 0.75, flip_x=False)       # a smaller batch: the tables are built once
    weights.fill(smc.PREFILL)
    lf.composite_weights_batch(2, weights[:2], flip_x=False)
    assert lf._batch_weight_ptrs_cu.ptr == tables
    for k in range(2):
        assert np.array_equal(weights.get()[k], _answer(oracle, k, gate, False)["weights"]), k
    with pytest.raises(ValueError):
        lf.composite_weights_batch(4, rdf.DeviceArray((4, H // R, W // R), np.uint16))
    plain = _stack(rdf, None)
    with pytest.raises(ValueError):
        plain.composite_weights(wbuf)
    with pytest.raises(ValueError):
        plain.composite_weights_batch(1, weights[:1])
    assert plain.conf_images is None and getattr(plain, "batch_conf_images", None) is None


PIPE_VARIANCES = (6., 5., 5., 4., 4., 4., 4.)
PIPE_TIPS = (2, 3, 4, 5, 6)
PIPE_INTR = (60., 61., 33.3, 11.6)


def _pipeline(rdf, lf, soft_modes=True, **kw):
    H, W, R = pc.LAYERED["H"], pc.LAYERED["W"], pc.LAYERED["R"]
    plane = (np.eye(4) + 0.05 * np.random.default_rng(3).standard_normal((4, 4))).astype(np.float32)
    pipe = _mod("pipeline").HandPipeline(lf, (H, W), R, 0.75, 6, list(PIPE_VARIANCES), list(PIPE_TIPS), PIPE_INTR, plane,
                                         soft_modes=soft_modes, **kw)
    return pipe, plane


def _camera(frame):
    """(camera frame: 0 = no reading, group image: 1 on every reading) of a layered frame."""
    cam = np.where(frame == NO, 0, frame).astype(np.uint16)
    return cam, (cam != 0).astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("gate", GATES, ids=["rejecting", "zero"])
def test_hand_pipeline_with_soft_modes(gate, rdf, gpu_runtime, oracle):
    frames = pc.layered_case()[4]
    H, W, R = pc.LAYERED["H"], pc.LAYERED["W"], pc.LAYERED["R"]
    pipe, plane = _pipeline(rdf, _stack(rdf, gate))
    L = pipe._L
    assert L == 7 and pipe.soft_modes and pipe.layered_rdf.min_conf == gate
    dbuf, gbuf = rdf.GpuBuffer((H, W), np.uint16), rdf.GpuBuffer((H, W), np.uint16)
    single = {}
    for k, frame in enumerate(frames):
        cam, groups = _camera(frame)
        dbuf.cu().set(cam)
        gbuf.cu().set(groups)
        for flip in (False, True):
            means, heights = pipe.run(dbuf, gbuf, 1, flip)
            want = _answer(oracle, k, gate, flip, prepared=True)
            assert np.array_equal(pipe.depth_image_2.cu().get(), _prepared(frame, flip))
            labels = want["hand"] if flip else want["composite"]
            assert np.array_equal(pipe.labels_image.cu().get(), labels)
            got_w = pipe.weights_image.cu().get()
            assert np.array_equal(got_w[want["written"]], want["weights"][want["written"]])
            want_m = sn.weighted_modes(labels, want["weights"], L, PIPE_VARIANCES, 6)
            assert np.array_equal(np.isnan(means), np.isnan(want_m)), (means, want_m)
            ok = ~np.isnan(want_m)
            assert ok.any() and np.abs(means[ok] - want_m[ok]).max() < BOUND_PX
            want_h = ms_np.fingertip_heights(means, list(PIPE_TIPS), cam, R, *PIPE_INTR, plane)
            assert np.array_equal(np.isnan(heights), np.isnan(want_h))
            okh = ~np.isnan(want_h)
            assert np.allclose(heights[okh], want_h[okh], rtol=1e-6, atol=1e-6)
            # the weights matter: the unweighted modes of the same composite lie elsewhere
            plain_m = ms_np.mean_shift(labels, L, PIPE_VARIANCES, 6)
            assert gate != (0, 0) or np.abs(plain_m[ok] - want_m[ok]).max() > 1.0      # (both on the CPU)
            again = pipe.run(dbuf, gbuf, 1, flip)
            assert np.array_equal(_bits(again[0]), _bits(means)) and np.array_equal(_bits(again[1]), _bits(heights))
            single[k, flip] = (means, heights)
    # enqueue_batch: frames 0, 1, 0 in one go equal the per-frame results bit for bit
    order = (0, 1, 0)
    cams = np.stack([_camera(frames[k])[0] for k in order])
    grps = np.stack([_camera(frames[k])[1] for k in order])
    n_t, stride = len(PIPE_TIPS), len(PIPE_TIPS) + 2
    for flip in (False, True):
        log = rdf.DeviceArray((3, stride), np.float64).fill(7.0)
        pipe.enqueue_batch(rdf.to_device(cams), rdf.to_device(grps), 1, flip, rdf.to_device(cams), log.ptr, stride)
        got_h, got_m = log.get(), pipe.means_batch.get()
        assert (got_h[:, n_t:] == 7.0).all()
        for i, k in enumerate(order):
            assert np.array_equal(_bits(got_m[i]), _bits(single[k, flip][0])), (flip, i)
            assert np.array_equal(_bits(got_h[i, :n_t]), _bits(single[k, flip][1])), (flip, i)


@pytest.mark.gpu
def test_soft_modes_refuses_what_it_cannot_serve_and_costs_nothing_when_off(rdf, gpu_runtime):
    with pytest.raises(ValueError):
        _pipeline(rdf, _stack(rdf, None))                           # no min_conf: the stack keeps no confidences
    with pytest.raises(ValueError):
        _pipeline(rdf, _stack(rdf, (0, 0)), fused_io=False)
    off, _ = _pipeline(rdf, _stack(rdf, (0, 0)), soft_modes=False)
    assert not off.soft_modes and not hasattr(off, "weights_image") and not hasattr(off, "weighted_modes")
    H, W = sc.H, sc.W
    with pytest.raises(ValueError):
        rdf.BeatsSession(smc.session_stack(rdf, (H, W), sc.forest_config(rdf)), (H, W), sc.frames()[1], num_random_guesses=4000, seed=3,
                         soft_modes=True)


@pytest.mark.gpu
@pytest.mark.parametrize("gate", [(20000, 16500), (0, 0)], ids=["rejecting", "zero"])
def test_session_with_soft_modes_batched_and_unbatched(gate, rdf, gpu_runtime):
    """BeatsSession(soft_modes=True) over the session scene (thresholds: test_posterior.SESSION_GATE, and none): the same events,
    heights and state frame by frame and in frame batches."""
    from hand_state_numpy import same_state
    H, W = sc.H, sc.W
    frames, intr = sc.frames()
    frames = frames[:6]
    cfg4 = sc.forest_config(rdf)

    def session(soft):
        lf = smc.session_stack(rdf, (H, W), cfg4)
        lf.min_conf = gate
        return rdf.BeatsSession(lf, (H, W), intr, num_random_guesses=4000, seed=3, max_frames=4, soft_modes=soft)
    first = session(True)
    assert first.right.soft_modes and first.left.soft_modes and first.right.layered_rdf is not first.left.layered_rdf
    plane = first.calibrate(frames[0])
    dev = rdf.to_device(frames)
    results, states = {}, {}
    for mode in ("sequence", "batched"):
        s = first if mode == "sequence" else session(True)
        s.set_plane(plane)
        results[mode] = s.run_sequence(dev, batched=mode == "batched")
        states[mode] = s.hand_state.state()
    ev, h = results["sequence"]
    assert h.shape == (6, 10) and np.isfinite(h).sum() >= 20
    assert results["batched"][0] == ev and np.array_equal(_bits(results["batched"][1]), _bits(h))
    assert same_state(states["batched"], states["sequence"])
