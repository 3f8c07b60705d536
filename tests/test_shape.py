"""The hand's shape (rdf_labels_shape_pool / rdf_labels_shape_decide of librdf_labels.so, shape.ShapeVoter, HandModel.shape_poses,
HandSceneRenderer.make_shape_dataset, dataset.read_shapes / score_shape_model, HandPipeline(shape_voter=), BeatsSession(shapes=))
against the numpy restatement in tests/shape_numpy.py.  The CPU tests pin the restatement to a case worked by hand and every
rounding rule to literals, ask of every case which wrong readings of the rules it notices, and check the argument checks of the
entry points and of the constructors, which launch nothing.  Every GPU comparison is byte for byte."""
import ctypes
import importlib
import os
import zlib

import numpy as np
import pytest

import mutants
import session_cases as sc
import shape_cases as shc
import shape_numpy as sn
import soft_modes_cases as smc

f32 = np.float32


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()}: {got[got != want][:5]} != {want[got != want][:5]}"


# the feature's entry points in the binding table: without them nothing in this module has anything to check
POOL_ARGS = _mod("_lib").BINDINGS["labels"][1]["rdf_labels_shape_pool"][1]
DECIDE_ARGS = _mod("_lib").BINDINGS["labels"][1]["rdf_labels_shape_decide"][1]

_true_outputs = {}


def _true(name):
    """A case's outputs from the restatement, computed once, shared by the tests and left unchanged."""
    if name not in _true_outputs:
        out = shc.outputs(sn, name)
        for a in out:
            a.setflags(write=False)
        _true_outputs[name] = out
    return _true_outputs[name]


# ------------------------------------------------------------------ CPU: the rules -------------------------------------------
def test_hand_worked_case():
    """shape_cases.hand_case(): one node, two classes, the row 1000 1000 1100 1000 1000 65535 0.  The root's probe is one pixel to
    the right at depth 1000 (floor(1000 / 1000) = 1) and the pixel itself at depth 1100 (floor(1000 / 1100) = 0); f < 50 goes
    left to [.75, .25], else right to [.5, .5].
      x  d      f = d(x + 1) - d(x)          leaf          S   shares floor(p * 65535)           label
      0  1000   0                            [.75, .25]    1   49151 (.25), 16383 (.75)          0
      1  1000   100                          [.5, .5]      1   32767 (.5), 32767                 0 (a tie: the lower class)
      2  1100   0 (the pixel itself)         [.75, .25]    1   49151, 16383                      0
      3  1000   0                            [.75, .25]    1   49151, 16383                      0
      4  1000   65535 - 1000                 [.5, .5]      1   32767, 32767                      0
      5, 6      65535 and 0: no pixels
    pool = [3 * 49151 + 2 * 32767, 3 * 16383 + 2 * 32767, 5 hard votes for class 0, 0 for class 1, 5 voting pixels, 0 dead]
         = [212987, 114683, 5, 0, 5, 0];  total 327670, raw 0, conf = floordiv(212987 * 65535, 327670) = 42598
         (13958103045 = 42598 * 327670 + 16385).
    Held at hold 2, min_pixels 5: frame 0 makes class 0 the candidate (run 1), frame 1 holds it (changed), frame 2 changes nothing;
    at min_pixels 6 the frame has no shape."""
    depth, forest = shc.hand_case()
    pool = sn.pool(depth, forest)
    assert pool.dtype == np.uint64 and pool.tolist() == [[212987, 114683, 5, 0, 5, 0]]
    assert 3 * 49151 + 2 * 32767 == 212987 and 3 * 16383 + 2 * 32767 == 114683 and 42598 * 327670 + 16385 == 212987 * 65535
    three = np.repeat(pool, 3, axis=0)
    out, state = sn.decide(three, 2, min_pixels=5, hold=2)
    assert out.dtype == state.dtype == np.int32
    assert out.tolist() == [[0, 42598, -1, 0], [0, 42598, 0, 1], [0, 42598, 0, 0]] and state.tolist() == [0, -1, 0, 0]
    out, state = sn.decide(three, 2, min_pixels=6, hold=2)
    assert out.tolist() == [[-1, 0, -1, 0]] * 3 and state.tolist() == [-1, -1, 0, 3]
    # the pool ADDS
    again = sn.pool(depth, forest, pool=pool.copy())
    assert again.tolist() == [[425974, 229366, 10, 0, 10, 0]]
    # labels_reduce 2 on two such rows reads depth pixels 0, 2 and 4 of the first; one row alone has no label pixel (1 // 2 = 0)
    two_rows = np.concatenate([depth, depth], axis=1)
    assert sn.pool(two_rows, forest, labels_reduce=2).tolist() == [[2 * 49151 + 32767, 2 * 16383 + 32767, 3, 0, 3, 0]]
    assert sn.pool(depth, forest, labels_reduce=2).tolist() == [[0] * 6]


def test_every_rounding_rule_on_literals():
    """G3.  The share is a floor: .75 * 65535 = 49151.25 -> 49151, .25 * 65535 = 16383.75 -> 16383 (they sum to 65534); one class
    alone gives 65535; a share above 1 (a negative PDF entry elsewhere) clamps to 65535 and a negative one to 0; NaN floors to 0.
    S == 0, S < 0 and S = NaN are dead.  G4: a dead pixel touches only the last word.  G6: see shape_cases.DECIDE."""
    acc = lambda *v: np.array(v, f32)                                       # noqa: E731
    assert sn.shares_of(acc(.75, .25)) == [49151, 16383] and sn.shares_of(acc(3., 1.)) == [49151, 16383]
    assert sn.shares_of(acc(0., 2.5)) == [0, 65535] and sn.shares_of(acc(1., 1., 1.)) == [21845, 21845, 21845]
    assert sn.shares_of(acc(-1., 0., 2.)) == [0, 0, 65535]                  # shares -1 and 2
    assert sn.shares_of(acc(0., 0.)) is None and sn.shares_of(acc(-1., .5)) is None and sn.shares_of(acc(np.nan, 1.)) is None
    assert sn.shares_of(acc(np.inf, 1.)) == [0, 0]                          # inf / inf = NaN -> 0; 1 / inf = 0
    assert sn.shares_of(acc(2. ** -24, 2. ** -24, 1.)) == [0, 0, 65534]     # S = 1 + 2^-23 in class order
    row = np.zeros(6, np.uint64)
    sn.add_pixel(row, acc(0., 0.))
    sn.add_pixel(row, acc(-3., 1.))
    assert row.tolist() == [0, 0, 0, 0, 0, 2]
    sn.add_pixel(row, acc(.5, .5))
    sn.add_pixel(row, acc(.25, .75))
    assert row.tolist() == [32767 + 16383, 32767 + 49151, 1, 1, 2, 2]      # the tie's hard vote goes to class 0
    # G6 on literals
    assert sn.raw_of(np.array([900, 100, 0, 0, 0, 0, 10, 0], np.uint64), 3, 10) == (0, 58981)      # 58981.5
    assert sn.raw_of(np.array([900, 100, 0, 0, 0, 0, 10, 0], np.uint64), 3, 11) == (-1, 0)
    assert sn.raw_of(np.array([0, 0, 0, 9, 9, 9, 50, 7], np.uint64), 3, 1) == (-1, 0)                # total == 0
    assert sn.raw_of(np.array([1, 1, 0, 0, 2, 0], np.uint64), 2, 0) == (0, 32767)                    # 32767.5; the tie
    assert sn.raw_of(np.array([0, 5, 0, 0, 0, 0], np.uint64), 2, 0) == (1, 65535)                    # min_pixels 0 asks nothing
    for name in shc.DECIDE:
        C, pool, settings, want = shc.decide_case(name)
        out, state = sn.decide(pool, C, **settings)
        assert out.tolist() == want.tolist(), name
        assert state[0] == want[-1, 2], name


def test_a_split_call_equals_one_call():
    for name, cut in shc.SPLITS.items():
        C, pool, settings, want = shc.decide_case(name)
        first, state = sn.decide(pool[:cut], C, **settings)
        assert tuple(state) != sn.FRESH, name                               # something is carried over
        second, state = sn.decide(pool[cut:], C, state=state, **settings)
        whole, want_state = sn.decide(pool, C, **settings)
        assert np.array_equal(np.concatenate([first, second]), whole) and np.array_equal(state, want_state), name
        fresh, _ = sn.decide(pool[cut:], C, **settings)
        assert not np.array_equal(fresh, second), name                      # and it matters


def test_the_cases_contain_what_they_are_meant_to():
    caps = sorted({shc.POOL[k][7] for k in shc.POOL})
    assert caps == [2, 3, 5, 9, 16] and {shc.POOL[k][3] for k in shc.POOL} == {1, 2, 3}
    depth, forest, kw = shc.pool_case("w67_n3")
    assert depth.shape == (3, 5, 67) and (5 * 67) % 64 != 0                  # waves straddle images
    for name in ("w131_r2_c5", "w131_r3_c16"):
        assert shc.POOL[name][2] % shc.POOL[name][3] != 0
    pool = _true("w67_c2")[0]
    assert pool[1].tolist() == [0] * 6 and pool[0, 4] > 0 and pool[2, 4] > 0 and _true("w67_c2")[1][:, 0].tolist()[1] == -1
    pool = _true("awkward")[0]
    assert (pool[:, 7] > 0).all() and (pool[:, 6] > 0).all()                 # dead pixels next to voting ones in every image
    for name in shc.POOL:
        p = _true(name)[0]
        C = shc.POOL[name][7]
        assert (p[:, C:2 * C].sum(axis=1) == p[:, 2 * C]).all() and p[:, 2 * C].sum() > 0, name
        assert (p[:, :C].sum(axis=1) <= 65535 * p[:, 2 * C]).all(), name
    # a filter that matters, and an adversarial walk that falls off
    depth, forest, kw = shc.pool_case("w131_r2_c5")
    assert not np.array_equal(sn.pool(depth, forest, kw["labels_reduce"], kw["scale"]), _true("w131_r2_c5")[0])
    depth, forest, want = shc.big_case()
    assert int(want[0, 0]) == 90000 * 65535 > 2 ** 32
    assert sn.pool(depth[:, :2, :3], forest).tolist() == [[6 * 65535, 6, 6, 0]]


# ------------------------------------------------------------------ CPU: do the cases bite? ----------------------------------
def test_an_unmutated_copy_gives_the_same_bytes():
    copy = shc.mutant(None)
    assert copy is not sn and copy.pool is not sn.pool
    for name in shc.KILLS:
        assert mutants.same(shc.outputs(copy, name), _true(name)), name


def test_a_mutant_that_no_longer_applies_fails_loudly():
    with pytest.raises(AssertionError, match="0 times"):
        mutants.load("shape_numpy", [("if soft[c] >= soft[best_]:", "x")])
    with pytest.raises(AssertionError, match="2 times"):
        mutants.load("shape_numpy", [("candidate, run = -1, 0", "pass")])


@pytest.mark.parametrize("name", list(shc.KILLS))
def test_each_mutant_changes_the_case_meant_for_it(name):
    """A wrong reading of a rule that leaves a case's outputs unchanged would pass the GPU test of that case.  KILLS is exact."""
    killed = {m for m in shc.MUTANTS if mutants.changed(shc.outputs(shc.mutant(m), name), _true(name))}
    assert killed == set(shc.KILLS[name]), name
    assert len(set(shc.KILLS[name])) == len(shc.KILLS[name])


def test_every_mutant_is_met_by_some_case():
    met = set(m for ms in shc.KILLS.values() for m in ms)
    assert met | set(shc.EQUIVALENT) == set(shc.MUTANTS) and len(shc.MUTANTS) >= 20
    assert set(shc.KILLS) == {"hand", "adds"} | set(shc.POOL) | {"decide:" + k for k in shc.DECIDE}
    for m, case in (("raw ties go up", "decide:ties"), ("label ties go up", "hand"), ("S in reverse class order", "order"),
                    ("shares not clamped above", "awkward"), ("the pool overwrites", "adds"), ("miss is never reset", "decide:release"),
                    ("hold is >", "decide:switch"), ("an interrupted candidate keeps its run", "decide:interrupted")):
        assert m in shc.KILLS[case], (m, case)


# ------------------------------------------------------------------ CPU: arguments -------------------------------------------
def test_rejected_arguments_launch_nothing(rdf):
    """Rejected arguments launch nothing, so they need no device; the pointers given here are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    P = ctypes.c_void_p
    d, f, fl, po, st, out = (P(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))
    BAD, NULL, LARGE = -1, -2, -3
    assert len(POOL_ARGS) == 14 and len(DECIDE_ARGS) == 10 and lib.rdf_labels_abi_version() == 1

    def pool(depth=d, n=1, w=8, h=8, forest=f, T=2, D=4, C=3, filt=None, fclass=-1, r=1, pool=po):
        return lib.rdf_labels_shape_pool(depth, n, w, h, forest, T, D, C, filt, fclass, r, 1., pool, None)
    for kw in (dict(C=0), dict(C=17), dict(C=-1), dict(C=65535), dict(T=0), dict(T=-1), dict(D=0), dict(D=31), dict(r=0), dict(r=-1),
               dict(n=-1), dict(w=-8), dict(h=-8), dict(filt=fl, fclass=-2), dict(filt=fl, fclass=65536),
               dict(depth=P(0x10001)), dict(filt=P(0x30001), fclass=1), dict(forest=P(0x20002)), dict(pool=P(0x40004))):
        assert pool(**kw) == BAD, kw
    assert pool(C=16, n=0) == 0 and pool(C=1, n=0) == 0
    assert pool(n=1, w=65536, h=32768) == LARGE and pool(n=32768, w=256, h=256) == LARGE
    assert pool(n=0, depth=None, forest=None, pool=None) == 0                # zero pixels, whatever the pointers
    assert pool(w=3, r=4) == 0 and pool(h=0) == 0 and pool(w=0) == 0
    assert pool(n=0, C=17) == BAD and pool(w=0, r=0) == BAD                  # a bad argument is one on zero pixels too
    for name in ("depth", "forest", "pool"):
        assert pool(**{name: None}) == NULL, name
    assert pool(filt=None, fclass=3) == NULL and pool(filt=fl, fclass=3, depth=None) == NULL

    def decide(pool=po, n=2, C=3, min_pixels=64, min_conf=0, hold=3, release=0, state=st, out=out):
        return lib.rdf_labels_shape_decide(pool, n, C, min_pixels, min_conf, hold, release, state, out, None)
    for kw in (dict(hold=0), dict(hold=-1), dict(release=-1), dict(min_conf=-1), dict(min_conf=65536), dict(min_pixels=-1), dict(C=0),
               dict(C=17), dict(n=-1), dict(pool=P(0x40004)), dict(state=P(0x50002)), dict(out=P(0x60002))):
        assert decide(**kw) == BAD, kw
    assert decide(n=0) == 0 and decide(n=0, pool=None, state=None, out=None) == 0 and decide(n=0, hold=0) == BAD
    for name in ("pool", "state", "out"):
        assert decide(**{name: None}) == NULL, name
    header = open(_mod("_build").LIBRARIES["labels"].headers[0]).read()
    assert "G1." in header and "G8." in header and "rdf_labels_shape_pool" in header and "#define RDF_POSTERIOR_MAX_CLASSES 16\n" in header
    assert any(p.endswith("forest_shape_hip.hip") for p in _mod("_build").LIBRARIES["labels"].sources)


def test_shape_poses(rdf):
    hm = _mod("hand_model")
    model = rdf.HandModel()
    assert {"open", "fist", "point", "pinch"} <= set(hm.SHAPES) and all(set(v) == set(hm.FINGERS) for v in hm.SHAPES.values())
    for shape, table in hm.SHAPES.items():
        a = model.shape_poses(shape, 9, np.random.default_rng(4))
        b = model.shape_poses(shape, 9, np.random.default_rng(4))
        assert a.shape == (9, hm.POSE_SIZE) and a.tobytes() == b.tobytes()                        # the same seed, the same poses
        assert a.tobytes() != model.shape_poses(shape, 9, np.random.default_rng(5)).tobytes()
        for k, finger in enumerate(hm.FINGERS):
            (s0, s1), (f0, f1) = table[finger]
            assert (a[:, 6 + 4 * k] >= s0).all() and (a[:, 6 + 4 * k] <= s1).all(), (shape, finger)
            assert (a[:, 7 + 4 * k:10 + 4 * k] >= f0).all() and (a[:, 7 + 4 * k:10 + 4 * k] <= f1).all(), (shape, finger)
        # the wrist and the hand's angles are sample_poses': one rng.random((n, 26)) call, the same columns
        plain = model.sample_poses(9, np.random.default_rng(4))
        assert a[:, :6].tobytes() == plain[:, :6].tobytes()
        # the mirrored model gives the mirror poses
        m = model.mirrored().shape_poses(shape, 9, np.random.default_rng(4))
        want = a.copy()
        want[:, (0, 3, 5)] *= -1.
        assert m.tobytes() == want.tobytes()
        # a table entry serves as a shape, and ranges reach the wrist
        assert model.shape_poses(table, 9, np.random.default_rng(4)).tobytes() == a.tobytes()
        moved = model.shape_poses(shape, 9, np.random.default_rng(4), ranges={"height": (10., 11.)})
        assert (moved[:, 2] >= 10. * model.units_per_mm).all() and (moved[:, 2] <= 11. * model.units_per_mm).all()
        assert moved[:, 6:].tobytes() == a[:, 6:].tobytes()
    # clearly different shapes: every finger but the thumb of a fist flexes more at every joint than any finger of an open hand
    fist, opened = model.shape_poses("fist", 20, np.random.default_rng(1)), model.shape_poses("open", 20, np.random.default_rng(1))
    assert fist[:, 10:].reshape(20, 4, 4)[:, :, 1:].min() > opened[:, 6:].reshape(20, 5, 4)[:, :, 1:].max()
    point = model.shape_poses("point", 20, np.random.default_rng(1))
    assert point[:, 11:14].max() <= 0.25 and point[:, 15:18].min() >= 1.0                         # index out, middle curled
    # sample_poses is what it was
    lo_hi = hm.SAMPLE_RANGES["flexion"]
    assert (plain[:, 7:10] >= lo_hi[0]).all() and (plain[:, 7:10] <= lo_hi[1]).all()


def test_frame_n_of_a_shape_dataset_is_shape_n_modulo_the_shapes(rdf):
    hm = _mod("hand_model")
    model = rdf.HandModel()
    shapes = ("fist", "open", "point")
    poses, index = model.shape_dataset_poses(11, np.random.default_rng(8), shapes)
    assert index.dtype == np.int32 and index.tolist() == [n % 3 for n in range(11)] and poses.shape == (11, 26)
    for n in range(11):
        for k, finger in enumerate(hm.FINGERS):
            f0, f1 = hm.SHAPES[shapes[n % 3]][finger][1]
            assert (poses[n, 7 + 4 * k:10 + 4 * k] >= f0).all() and (poses[n, 7 + 4 * k:10 + 4 * k] <= f1).all(), (n, finger)
    # one shape_poses call per shape, in the order of `shapes`, from the one generator
    rng = np.random.default_rng(8)
    for k, shape in enumerate(shapes):
        want = model.shape_poses(shape, len(range(k, 11, 3)), rng)
        assert poses[k::3].tobytes() == want.tobytes(), shape
    again, _ = model.shape_dataset_poses(11, np.random.default_rng(8), shapes)
    assert again.tobytes() == poses.tobytes()
    assert model.shape_dataset_poses(5, np.random.default_rng(8))[1].tolist() == [0, 1, 2, 3, 0] and tuple(hm.SHAPES)[:4] == ("open", "fist", "point", "pinch")
    with pytest.raises(AssertionError):
        model.shape_dataset_poses(4, np.random.default_rng(8), ("open", "claw"))


class _Host:
    def __init__(self, a):
        self._a = a

    def get(self):
        return self._a


def test_a_shape_dataset_directory(rdf, tmp_path):
    """make_shape_dataset with a stand-in for the render (no device): the labels are 1 + shape index on the drawn pixels,
    shapes.npy holds the truth, and read_shapes reads it back in the order asked for."""
    scene, ds = _mod("hand_scene"), _mod("dataset")
    H, W, n = 12, 20, 7
    r = scene.HandSceneRenderer.__new__(scene.HandSceneRenderer)
    r.f, r.ppx, r.ppy, r.z_near, r.z_far, r.DIM_Y, r.DIM_X = 75., 52.5, 29.5, 50., 50000., H, W
    r.model = rdf.HandModel()
    r.left_model = r.model.mirrored()
    seen = {}

    def render(tforms, labels, table, empty_depth, seed, hole_rate, noise_amp, sensor=None):
        rng = np.random.default_rng(zlib.crc32(np.asarray(tforms, np.float32).tobytes()))
        fine = rng.integers(0, 8, (len(tforms), H, W)).astype(np.uint16)
        seen["fine"], seen["args"] = fine, (labels, table, empty_depth, seed)
        return _Host(np.where(fine > 0, 4000, 65535).astype(np.uint16)), _Host(fine)
    r.render = render
    path = str(tmp_path / "shapes")
    depth, labels, index = r.make_shape_dataset(path, n, seed=6, shapes=("open", "fist"))
    assert seen["args"] == ("fine", None, 65535, 6) and index.tolist() == [0, 1, 0, 1, 0, 1, 0]
    for k in range(n):
        assert np.array_equal(labels[k], np.where(seen["fine"][k] > 0, 1 + k % 2, 0))
    assert sorted(os.listdir(path)) == sorted(["config.json", ds.SHAPES_FILE] + [f"{str(i).zfill(8)}_{k}.png" for i in range(n) for k in ("depth", "labels")])
    cfg = ds.DecisionTreeDatasetConfig(path, num_images=n, shuffle=False)
    assert cfg.num_classes() == 3 and cfg.img_dims == (W, H) and np.array_equal(cfg.get_block_cpu(0, "labels"), labels)
    assert len({tuple(cfg.id_to_color[k].tolist()) for k in (0, 1, 2)}) == 3                    # one colour per shape
    got = ds.read_shapes(path, [6, 1, 1, 0])
    assert got.dtype == np.int32 and got.tolist() == [0, 1, 1, 0] and ds.read_shapes(path, []).shape == (0,)
    with pytest.raises(IndexError):
        ds.read_shapes(path, [n])
    r.make_dataset(str(tmp_path / "plain"), 2, seed=6, plane=scene.look_down_plane(5500.))
    with pytest.raises(FileNotFoundError, match="no hand shapes"):
        ds.read_shapes(str(tmp_path / "plain"), [0])
    np.save(os.path.join(path, ds.SHAPES_FILE), index[:-1])
    with pytest.raises(ValueError):
        ds.read_shapes(path, [0])


def _stump(C=2):
    forest = np.zeros((1, 1, 7 + 2 * C), np.float32)
    forest[0, 0, 7:] = 1. / C
    return forest


def test_what_the_constructors_refuse(rdf, host_runtime):
    """Every ValueError comes before anything is allocated and before the stack or the voter is marked as a pipeline's."""
    _mod("_build").build()
    pl = _mod("pipeline")
    forest = rdf.DecisionForest.from_numpy(_stump())
    voter = rdf.ShapeVoter(forest, (48, 64), names=("a", "b"))
    assert (voter.C, voter.words, voter.hold, voter.release, voter.min_pixels, voter.min_conf, voter.max_frames) == (2, 6, 3, 0, 64, 0, 64)
    assert voter.state.get().tolist() == list(sn.FRESH)

    class Stack:
        num_layered_classes = 7
    args = ((48, 64), 2, 1.0, 6, np.full(7, 8., np.float32), [2, 3, 4, 5, 6], (60., 60., 32., 24.), np.eye(4))
    for kw in (dict(shape_voter=object()), dict(shape_voter=forest), dict(shape_voter=(forest,)),
               dict(shape_voter=rdf.ShapeVoter(forest, (64, 48))), dict(shape_voter=voter, fused_io=False)):
        stack = Stack()
        with pytest.raises(ValueError):
            pl.HandPipeline(stack, *args, **kw)
        assert not hasattr(stack, "_pipeline_owner") and not hasattr(voter, "_pipeline_owner"), kw
    sib = voter.sibling()
    assert sib is not voter and sib.forest is voter.forest and sib.settings() == voter.settings() and sib.names == ("a", "b")
    assert sib.state.ptr != voter.state.ptr and sib._pool.ptr != voter._pool.ptr and sib._out.ptr != voter._out.ptr
    for kw in (dict(labels_reduce=0), dict(min_pixels=-1), dict(min_conf=65536), dict(min_conf=-1), dict(hold=0), dict(release=-1),
               dict(max_frames=0), dict(names=("a",))):
        with pytest.raises(ValueError):
            rdf.ShapeVoter(forest, (48, 64), **kw)
    with pytest.raises(ValueError):
        rdf.ShapeVoter(rdf.DecisionForest.from_numpy(_stump(17)), (48, 64))
    # the session: refused before anything is built (the stack is never looked at)
    for shapes in ((), (forest, {}, 3), forest, (forest, dict(max_frames=4)), (forest, dict(cell_shift=2))):
        with pytest.raises(ValueError):
            rdf.BeatsSession(None, (48, 64), (60., 32., 24.), shapes=shapes)
    with pytest.raises(ValueError):
        rdf.BeatsSession(None, (48, 64), (60., 32., 24.), shapes=(forest,), fused_io=False)
    # to_host
    rows = np.array([[1, 65535, 0, 1], [-1, 0, -1, 0]], np.int32)
    assert rdf.ShapeVoter.to_host(rows, as_array=True).tolist() == rows.tolist()
    assert rdf.ShapeVoter.to_host(rows) == [dict(raw=1, conf=1., held=0, changed=True), dict(raw=-1, conf=0., held=-1, changed=False)]
    assert voter.to_host(rows)[0]["raw_name"] == "b" and voter.to_host(rows)[0]["held_name"] == "a" and voter.to_host(rows)[1]["held_name"] is None


# ------------------------------------------------------------------ GPU: the kernels -----------------------------------------
def _voter(rdf, forest, dims, **kw):
    return rdf.ShapeVoter(rdf.DecisionForest.from_numpy(np.ascontiguousarray(forest)), dims, **kw)


def _device_pool(rdf, depth, forest, kw, voter=None, out=None, **settings):
    voter = voter or _voter(rdf, forest, depth.shape[1:], labels_reduce=kw["labels_reduce"], **settings)
    gate = None if kw["filter_images"] is None else rdf.to_device(kw["filter_images"])
    return voter, voter.pool(rdf.to_device(depth), gate, -1 if gate is None else kw["filter_class"], kw["scale"], out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hand"] + list(shc.POOL))
def test_pool_and_decide_equal_the_restatement(name, rdf, gpu_runtime):
    depth, forest, kw = shc.hand_case() + (dict(labels_reduce=1, scale=1., filter_images=None, filter_class=None),) if name == "hand" \
        else shc.pool_case(name)
    want_pool, want_rows, want_state = _true(name)
    voter, pool = _device_pool(rdf, depth, forest, kw, min_pixels=5 if name == "hand" else 1, hold=1)
    _same(pool.get(), want_pool, "pool")
    rows = voter.decide(pool)
    _same(rows.get(), want_rows, "rows")
    _same(voter.state.get(), want_state, "state")
    if name == "hand":
        assert pool.get().tolist() == [[212987, 114683, 5, 0, 5, 0]] and rows.get().tolist() == [[0, 42598, 0, 1]]


@pytest.mark.gpu
def test_the_adversarial_walk(rdf, gpu_runtime):
    """The planted flags and off-range offsets of walk_cases.adversarial_case(): a walk that goes wrong ends in another leaf."""
    for depth, forest, kw in shc.adversarial_runs():
        want = sn.pool(depth, forest, **kw)
        assert want[:, 10].all() and want[:, :5].any()
        _, pool = _device_pool(rdf, depth, forest, kw)
        _same(pool.get(), want, f"pool at scale {kw['scale']}")


@pytest.mark.gpu
def test_the_pool_adds_and_a_rejected_call_leaves_it(rdf, gpu_runtime):
    depth, forest, kw = shc.pool_case("w67_n3")
    first, again = _true("adds")
    voter, pool = _device_pool(rdf, depth, forest, kw)
    _same(pool.get(), first, "one call")
    lib, d_cu = _mod("_lib").load("labels"), rdf.to_device(depth)
    n, h, w = depth.shape
    call = lambda C, hold: (lib.rdf_labels_shape_pool(d_cu.ptr, n, w, h, voter.forest.forest_cu.ptr, voter.T, voter.D, C, None, -1, 1, 1.,   # noqa: E731
                                                      pool.ptr, rdf.get_runtime().stream()),
                            lib.rdf_labels_shape_decide(pool.ptr, n, 3, 1, 0, hold, 0, voter.state.ptr, voter._out.ptr, rdf.get_runtime().stream()))
    assert call(3, 1) == (0, 0)                                              # the entry point itself ADDS
    _same(pool.get(), again, "two calls")
    assert (again == 2 * first).all()
    state, rows = voter.state.get(), voter._out.get()
    assert call(17, 0) == (-1, -1)
    _same(pool.get(), again, "after a rejected call")
    _same(voter.state.get(), state, "state after a rejected call")
    _same(voter._out.get(), rows, "rows after a rejected call")
    # ShapeVoter.pool zeroes what it returns: the same call again gives one call's row, also in a caller's array
    own = rdf.DeviceArray(first.shape, np.uint64).fill(np.uint64(7))
    _, got = _device_pool(rdf, depth, forest, kw, voter=voter, out=own)
    assert got is own
    _same(own.get(), first, "a caller's array")


@pytest.mark.gpu
def test_sums_beyond_32_bits(rdf, gpu_runtime):
    depth, forest, want = shc.big_case()
    voter, pool = _device_pool(rdf, depth, forest, dict(labels_reduce=1, scale=1., filter_images=None, filter_class=None))
    _same(pool.get(), want, "pool")
    assert voter.decide(pool).get().tolist() == [[0, 65535, -1, 0]]


@pytest.mark.gpu
def test_chunks_of_max_frames(rdf, gpu_runtime):
    depth, forest, kw = shc.chunk_case()
    want = sn.pool(depth, forest, **kw)
    assert depth.shape[0] == 5 and len({row.tobytes() for row in want}) == 5
    whole = _device_pool(rdf, depth, forest, kw, max_frames=8)[1].get()
    voter, chunked = _device_pool(rdf, depth, forest, kw, max_frames=2, min_pixels=1, hold=2)
    _same(whole, want, "one chunk")
    _same(chunked.get(), want, "chunks of two")
    assert chunked.shape == (5, 10) and voter._pool.shape[0] == 5            # the voter's own buffer grew to the call
    rows = voter.classify(rdf.to_device(depth), scale_factor=kw["scale"])
    _same(rows.get(), sn.decide(want, 4, min_pixels=1, hold=2)[0], "classify")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(shc.DECIDE))
def test_decide_on_literal_rows(name, rdf, gpu_runtime):
    C, pool, settings, want = shc.decide_case(name)
    voter = _voter(rdf, _stump(C), (4, 8), **settings)
    rows = voter.decide(rdf.to_device(pool)).get()
    _same(rows, want, "rows")
    _same(rows, _true("decide:" + name)[0], "the restatement's rows")
    _same(voter.state.get(), _true("decide:" + name)[1], "state")
    if name in shc.SPLITS:                                                   # a split call equals one call; reset() starts afresh
        cut = shc.SPLITS[name]
        voter.reset()
        _same(voter.state.get(), np.array(sn.FRESH, np.int32), "a reset state")
        first = voter.decide(rdf.to_device(pool[:cut])).get()
        second = voter.decide(rdf.to_device(pool[cut:])).get()
        _same(np.concatenate([first, second]), want, "two calls")


@pytest.mark.gpu
def test_two_siblings_hold_their_own_state(rdf, gpu_runtime):
    """Two streams of frames through a voter and its sibling, a few frames at a time in turn: each equals its own trace."""
    C, pool_a, settings, want_a = shc.decide_case("switch")
    _, pool_b, settings_b, want_b = shc.decide_case("interrupted")
    a = _voter(rdf, _stump(C), (4, 8), **settings)
    b = a.sibling()
    b.hold = settings_b["hold"]
    assert b.forest is a.forest and b.state.ptr != a.state.ptr
    pa, pb = rdf.to_device(pool_a), rdf.to_device(pool_b)
    got_a, got_b = [], []
    for k in range(0, 10, 2):
        if k < len(pool_a):
            got_a.append(a.decide(pa[k:k + 2]).get())
        got_b.append(b.decide(pb[k:k + 2]).get())
    _same(np.concatenate(got_a), want_a, "the voter")
    _same(np.concatenate(got_b), want_b, "its sibling")


# ------------------------------------------------------------------ GPU: the pipeline and the session ------------------------
TIPS = (2, 3, 4, 5, 6)
SHAPE_SETTINGS = dict(labels_reduce=2, min_pixels=16, hold=2)


def _hand_frame(k):
    """Frame k of the session scene with a full-resolution group image: what is nearer than the table is a hand, the left half
    group 1, the right half group 2."""
    depth, (focal, ppx, ppy) = sc.frame(k)
    hand = (depth > 0) & (depth < 500)
    groups = np.where(hand, np.where(np.arange(sc.W)[None, :] < sc.W // 2, 1, 2), 0).astype(np.uint16)
    assert (groups == 1).sum() > 2000 and (groups == 2).sum() > 2000
    return depth, groups, (focal, focal, ppx, ppy)


def _plane():
    return (np.eye(4) + 0.05 * np.random.default_rng(3).standard_normal((4, 4))).astype(np.float32)


def _pipe(rdf, **kw):
    stack = smc.session_stack(rdf, (sc.H, sc.W), sc.forest_config(rdf))
    return _mod("pipeline").HandPipeline(stack, (sc.H, sc.W), sc.R, sc.W / 848, 6, [50., 8., 8., 8., 8., 8., 8.], list(TIPS),
                                         _hand_frame(0)[2], _plane(), depth_mm_level=0, **kw)


def _shape_forest(rdf):
    """A forest to pool with on the session scene: the session stack's first layer, four classes."""
    return rdf.DecisionForest.from_numpy(sc.forest_config(rdf)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("g_id,flip", [(1, False), (2, True)])
def test_a_pipeline_with_a_shape_voter(g_id, flip, rdf, gpu_runtime):
    """`.shape` is ShapeVoter.classify on the pipeline's own prepared frame (mirrored for the left hand), frame after frame;
    enqueue_batch gives the frames' rows; means and heights are those of a pipeline without a voter."""
    FRAMES = 3
    frames = [_hand_frame(k) for k in range(FRAMES)]
    cams, grps = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    voter = rdf.ShapeVoter(_shape_forest(rdf), (sc.H, sc.W), max_frames=2, **SHAPE_SETTINGS)
    check = voter.sibling()
    plain, shaped = _pipe(rdf), _pipe(rdf, shape_voter=voter)
    assert plain.shape_voter is None and plain.shape is None and plain.shape_batch is None
    assert shaped.shape_voter is voter and _pipe(rdf, shape_voter=voter).shape_voter is not voter      # a second pipeline: a sibling
    dbuf, gbuf = rdf.GpuBuffer((sc.H, sc.W), np.uint16), rdf.GpuBuffer((sc.H, sc.W), np.uint16)
    single = []
    for k in range(FRAMES):
        dbuf.cu().set(cams[k])
        gbuf.cu().set(grps[k])
        want_m, want_h = plain.run(dbuf, gbuf, g_id, flip)
        got_m, got_h = shaped.run(dbuf, gbuf, g_id, flip)
        assert got_m.tobytes() == want_m.tobytes() and got_h.tobytes() == want_h.tobytes() and np.isfinite(want_h).sum() >= 2
        prepared = shaped.depth_image_2.cu().get()
        if k == 0:                                                          # the frame the forest sees: the hand alone, mirrored
            hand = np.where(grps[0] == g_id, cams[0], 0)
            hand = np.where(hand == 0, 65535, hand).astype(np.uint16)
            _same(prepared, hand[:, ::-1] if flip else hand, "the prepared frame")
        want = check.classify(rdf.to_device(prepared[None]), scale_factor=sc.W / 848).get()
        row = shaped.shape.get()
        _same(row, want[0], f"frame {k}")
        single.append(row)
    single = np.stack(single)
    assert (single[:, 0] >= 0).all() and single[:, 2].tolist()[0] == -1 and single[1, 3] + single[2, 3] >= 1      # hold 2: held from frame 1 or 2 on
    with pytest.raises(NotImplementedError):
        shaped.capture(dbuf, gbuf, g_id, flip)
    # the batch: a fresh state, the same rows; the heights beside those of the plain pipeline's batch
    voter.reset()
    logs = []
    for pipe in (plain, shaped):
        log = rdf.DeviceArray((FRAMES, len(TIPS)), np.float64).fill(-7.)
        pipe.enqueue_batch(rdf.to_device(cams), rdf.to_device(grps), g_id, flip, rdf.to_device(cams), log.ptr, len(TIPS))
        log.mark_dirty()
        logs.append((log.get(), pipe.means_batch.get()))
    assert logs[0][0].tobytes() == logs[1][0].tobytes() and logs[0][1].tobytes() == logs[1][1].tobytes()
    assert shaped.shape_batch.shape == (FRAMES, 4)
    _same(shaped.shape_batch.get(), single, "enqueue_batch")


@pytest.mark.gpu
def test_a_session_with_shapes(rdf, gpu_runtime):
    """BeatsSession(shapes=...): last_shapes is the same bytes from run_sequence in frame batches and frame by frame over more
    than one block, and from two calls over the halves of the sequence; events and heights are those of a session without
    shapes; on_shape_fn is called once per held change seen at poll()."""
    H, W = sc.H, sc.W
    frames, intr = sc.frames()
    frames = frames[:5]
    forest = _shape_forest(rdf)

    def session(**kw):
        return rdf.BeatsSession(smc.session_stack(rdf, (H, W), sc.forest_config(rdf)), (H, W), intr, num_random_guesses=4000, seed=3,
                                max_frames=4, **kw)
    calls = []
    a = session(shapes=(forest, SHAPE_SETTINGS), on_shape_fn=lambda hand, held: calls.append((hand, held)))
    assert a.right.shape_voter is not a.left.shape_voter and a.right.shape_voter.max_frames == a.left.shape_voter.max_frames == 4
    assert a.right.shape_voter.hold == 2 and a.last_shapes is None and len(frames) == a.max_frames + 1
    plane = a.calibrate(frames[0])
    dev = rdf.to_device(frames)
    ev_a, h_a = a.run_sequence(dev, batched=True)
    shapes_a = a.last_shapes
    assert shapes_a.dtype == np.int32 and shapes_a.shape == (5, 2, 4) and (shapes_a[:, :, 0] >= 0).all()
    assert (shapes_a[0, :, 2] == -1).all() and (shapes_a[-1, :, 2] >= 0).all()                     # held from the second frame on
    # run_sequence ends in a poll: one call a hand, its held shape
    assert calls == [(0, int(shapes_a[-1, 0, 2])), (1, int(shapes_a[-1, 1, 2]))]
    assert a.poll() == [] and len(calls) == 2                                                       # nothing changed since
    b = session(shapes=(forest, SHAPE_SETTINGS))
    b.set_plane(plane)
    ev_b, h_b = b.run_sequence(dev, batched=False)
    _same(b.last_shapes, shapes_a, "frame by frame")
    c = session(shapes=(forest, SHAPE_SETTINGS))
    c.set_plane(plane)
    c.run_sequence(dev[:2], batched=True)
    first = c.last_shapes
    c.run_sequence(dev[2:], batched=False)
    _same(np.concatenate([first, c.last_shapes]), shapes_a, "two calls")
    plain = session()
    plain.set_plane(plane)
    ev_p, h_p = plain.run_sequence(dev, batched=True)
    assert plain.last_shapes is None and plain.right.shape_voter is None
    assert ev_a == ev_b == ev_p and h_a.tobytes() == h_b.tobytes() == h_p.tobytes()
    # tick: the same held shapes; a reset voter is a change that the next poll delivers, once
    seen = []
    d = session(shapes=(forest, SHAPE_SETTINGS), on_shape_fn=lambda hand, held: seen.append((hand, held)))
    d.set_plane(plane)
    d.tick(dev[0])
    assert d.poll() is not None and seen == []                                                      # hold 2: nothing held after one frame
    for k in range(1, 5):
        d.tick(dev[k])
    d.poll()
    assert seen == calls
    _same(d.right.shape.get(), shapes_a[-1, 0], "tick, right hand")
    _same(d.left.shape.get(), shapes_a[-1, 1], "tick, left hand")
    d.left.shape_voter.reset()
    d.poll()
    d.poll()
    assert seen == calls + [(1, -1)]


# ------------------------------------------------------------------ GPU: end to end ------------------------------------------
@pytest.mark.gpu
def test_end_to_end_on_rendered_shapes(rdf, gpu_runtime, tmp_path):
    """make_shape_dataset of open hands and fists -> train_forest -> ShapeVoter on frames the trainer has not seen: the device's
    decisions are the restatement's.  The accuracy is printed, not asserted: tests/perf/bench_shape.py records it."""
    ds_mod = _mod("dataset")
    W, H, n_train, n_test, n_held, seed = 106, 60, 16, 4, 6, 5
    shapes = ("open", "fist")
    r = rdf.HandSceneRenderer((H, W), (75., 52.5, 29.5))
    depth, labels, index = r.make_shape_dataset(str(tmp_path / "train"), n_train + n_test, seed=31, shapes=shapes)
    assert depth.shape == (n_train + n_test, H, W) and ((labels == 0) == (depth == 65535)).all()
    for k in range(n_train + n_test):
        assert set(np.unique(labels[k]).tolist()) == {0, 1 + k % 2} and (labels[k] > 0).sum() > 200
    forest_np, pct = ds_mod.train_forest(str(tmp_path / "train"), n_train, n_test, 64, 32, 2, 6, str(tmp_path / "forest.npy"),
                                         log=lambda *_: None, tree_seed=seed)
    assert forest_np.shape == (2, 63, 7 + 2 * 3)
    held, _, held_index = r.make_shape_dataset(str(tmp_path / "held"), n_held, seed=77, shapes=shapes)
    settings = dict(min_pixels=16, hold=2)
    voter = rdf.ShapeVoter(rdf.DecisionForest.load(str(tmp_path / "forest.npy")), (H, W), names=("none",) + shapes, **settings)
    pool = voter.pool(rdf.to_device(held))
    rows = voter.decide(pool)
    want_pool = sn.pool(held, forest_np)
    want_rows, want_state = sn.decide(want_pool, 3, **settings)
    _same(pool.get(), want_pool, "pool")
    _same(rows.get(), want_rows, "rows")
    _same(voter.state.get(), want_state, "state")
    assert (want_pool[:, 6] > 200).all() and (want_rows[:, 0] >= 0).all()
    np.random.seed(seed)
    score = ds_mod.score_shape_model(str(tmp_path / "forest.npy"), str(tmp_path / "held"), n_held, min_pixels=16)
    assert score["frames"] == n_held and score["confusion"].shape == (3, 4) and score["confusion"].sum() == n_held
    assert sorted(score["raw"].tolist()) == sorted(want_rows[:, 0].tolist()) and sorted(score["truth"].tolist()) == sorted((held_index + 1).tolist())
    assert score["accuracy"] == float(np.mean(score["raw"] == score["truth"])) == np.trace(score["confusion"][:, :3]) / n_held
    print(f"pixels matching {pct:.3f}; held-out frames: soft {score['accuracy']:.3f}, hard {score['accuracy_hard']:.3f}; "
          f"rows {voter.to_host(rows)}")
