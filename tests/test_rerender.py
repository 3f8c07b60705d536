"""The converter's re-render (librdf_labels.so: rdf_points_center, rdf_rerender; SceneRerender; RecordingConverter(rerender=
True)) against the restatement in tests/rerender_numpy.py.  The CPU tests pin the restatement to answers worked by hand
from the rules in include/rdf_labels.h; every GPU comparison of images is bit for bit, with no pixel or case left out.

Hand-worked scenes use powers of two for the depths and the focal length, so that deprojection, projection and the
perspective division are exact in fp32 and the expected depth is the plane's own, not one below it after truncation."""
import importlib
import os

import numpy as np
import pytest

import frontend_numpy as fnp
import labels_numpy as lnp
import mutants
import rerender_cases as rc
import rerender_numpy as rn
from abi_helpers import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rdf_labels.h")
F = np.float32
PALETTE8 = np.array([[220, 40, 40], [40, 200, 60], [50, 60, 230], [230, 220, 50], [200, 50, 210], [40, 210, 220],
                     [250, 140, 30], [120, 120, 120]], np.uint8)
EYE = np.identity(4, np.float32)


_make_transform, _plane, _case = rc.make_transform, rc.plane, rc.case


def _flat(W, H, d, f=64., color=(10, 200, 30)):
    """A fronto-parallel plane at depth d filling the frame: (pts, colour, (f, ppx, ppy))."""
    ppx, ppy = (W - 1) / 2., (H - 1) / 2.
    pts = fnp.deproject(np.full((H, W), d, np.uint16), F(ppx), F(ppy), F(f))
    return pts, np.full((H, W, 3), color, np.uint8), (f, ppx, ppy)


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_identity_resamples_by_half_a_pixel_and_loses_the_last_row_and_column():
    W, H, d = 6, 5, 128
    pts, color, cam = _flat(W, H, d)
    depth, out, count = rn.rerender(pts, color, EYE, *cam)
    inside = np.zeros((H, W), bool)
    inside[:H - 1, :W - 1] = True
    # every pixel centre lies on the diagonal its quad's two triangles share: the fill rule gives it to exactly one
    assert np.array_equal(count, inside.astype(count.dtype))
    assert np.array_equal(depth, np.where(inside, d, 0)) and np.array_equal(out, np.where(inside[..., None], color, 0))


def test_one_invalid_point_removes_the_four_pixels_of_the_quads_around_it():
    W, H, d = 6, 5, 128
    pts, color, cam = _flat(W, H, d)
    pts[2, 3] = 0
    depth, out, count = rn.rerender(pts, color, EYE, *cam)
    want = np.zeros((H, W), bool)
    want[:H - 1, :W - 1] = True
    want[1:3, 2:4] = False
    assert np.array_equal(count, want.astype(count.dtype)) and np.array_equal(depth > 0, want)
    assert np.array_equal(out.any(-1), want)


def test_a_scaled_planar_mesh_has_no_crack_and_no_pixel_drawn_twice():
    W, H, d = 12, 10, 128
    pts, color, cam = _flat(W, H, d)
    color = np.random.default_rng(0).integers(1, 256, (H, W, 3)).astype(np.uint8)
    centre = rn.center_sums(pts)
    centre = centre[:3] / centre[3] + (0.7, -0.4, 0.)         # off the pixel grid
    M = _make_transform(EYE, centre, 1.37)
    depth, out, count = rn.rerender(pts, color, M, *cam)
    X, Y, _, _, ok = rn.vertices(pts, M, *cam)
    assert ok.all()
    cx, cy = np.arange(W) * 256 + 128, np.arange(H) * 256 + 128
    # inside the silhouette whatever the last bit of a snapped border vertex; left and top borders are in, right and bottom out
    in_x = (cx >= X[:, 0].max()) & (cx < X[:, -1].min())
    in_y = (cy >= Y[0].max()) & (cy < Y[-1].min())
    out_x = (cx < X[:, 0].min()) | (cx >= X[:, -1].max())
    out_y = (cy < Y[0].min()) | (cy >= Y[-1].max())
    assert in_x.sum() >= 8 and in_y.sum() >= 6 and X[:, 0].max() < 0 and Y[-1].min() > H * 256       # it leaves the frame
    assert (count[np.ix_(in_y, in_x)] == 1).all() and count.max() == 1
    assert not count[out_y].any() and not count[:, out_x].any()
    # (z' = 1.37 z + (1 - 1.37) 128 in fp32 is 128 to a few units in the last place, so the truncated depth is d or d - 1)
    assert np.isin(depth[count == 1], (d - 1, d)).all() and out[count == 1].any(-1).all()


def test_parallax_the_nearest_fragment_wins_over_the_stretched_triangles_of_the_step():
    W, H, f = 14, 6, 128.
    ppx, ppy = 6.5, 2.5
    d = np.full((H, W), 1024, np.uint16)
    d[:, 4:7] = 512                                     # the strip: three columns of points, two columns of quads
    pts = fnp.deproject(d, F(ppx), F(ppy), F(f))
    color = np.full((H, W, 3), (0, 0, 250), np.uint8)
    color[:, 4:7] = (250, 0, 0)
    M = EYE.copy()
    M[0, 3] = 16.                                       # 16 units in x: 4 pixels at z = 512, 2 pixels at z = 1024
    depth, out, count = rn.rerender(pts, color, M, f, ppx, ppy)
    X = rn.vertices(pts, M, f, ppx, ppy)[0]
    assert X[0, 4:7].tolist() == [8 * 256, 9 * 256, 10 * 256] and X[0, 3] == 5 * 256 and X[0, 7] == 9 * 256
    # the strip now covers pixels 8 and 9 of every row but the last; in y, z scales both the point and its projection: unchanged
    assert (depth[:H - 1, 8:10] == 512).all() and (out[:H - 1, 8:10] == (250, 0, 0)).all()
    # pixel 9 also lies under the folded triangles between the strip's right edge (at 10) and the plane's column 7 (at 9),
    # and under the plane's own quad 7..8 (at 9..10)
    assert (count[:H - 1, 9] >= 3).all()
    # left of the strip the step is stretched from 5 to 8, between the two depths
    assert ((depth[:H - 1, 5:8] > 512) & (depth[:H - 1, 5:8] < 1024)).all()
    assert (depth[:H - 1, 2:5] == 1024).all() and (depth[:H - 1, 10:W - 1] == 1024).all() and not depth[H - 1].any()


def test_resolve_nearest_first_then_the_lowest_id():
    # pixel 0: equal z, ids 9 and 3; pixel 1: z 7 with id 1 against z 6 with id 2; pixel 2: nothing
    winner = rn.resolve(3, [0, 0, 1, 1], np.array([5, 5, 7, 6], np.float32), [9, 3, 1, 2])
    assert winner.tolist() == [1, 3, -1]
    assert rn.resolve(1, [0, 0, 0], np.array([5, 5, 5], np.float32), [4, 2, 3]).tolist() == [1]
    # the order of arrival does not matter
    assert rn.resolve(3, [1, 0, 1, 0], np.array([6, 5, 7, 5], np.float32), [2, 3, 1, 9]).tolist() == [1, 0, -1]
    assert int(rn.depth_key(F(1.0), 7)) == (0x3F800000 << 32) | 7


def test_nothing_is_drawn_outside_the_depth_range_or_behind_the_camera():
    W, H = 6, 5
    for d in (40, 60000):
        pts, color, cam = _flat(W, H, d)
        depth, out, count = rn.rerender(pts, color, EYE, *cam, 50., 50000.)
        assert not depth.any() and not out.any() and not count.any(), d
    pts, color, cam = _flat(W, H, 64)                   # the bounds themselves are inside
    assert rn.rerender(pts, color, EYE, *cam, 64., 64.)[2].sum() == (W - 1) * (H - 1)
    assert not rn.rerender(pts, color, EYE, *cam, 64.5, 70.)[2].any() and not rn.rerender(pts, color, EYE, *cam, 60., 63.5)[2].any()
    pts, color, cam = _flat(W, H, 128)
    M = EYE.copy()
    M[2, 3] = -256.                                     # z' = -128
    depth, out, count = rn.rerender(pts, color, M, *cam)
    assert not depth.any() and not out.any() and not count.any()
    M[2, 3] = -128.                                     # z' = 0: not in front of the camera either
    assert not rn.rerender(pts, color, M, *cam)[2].any()


def test_make_transform():
    P = _plane()
    c = np.array([120., -340., 55.])
    M = _make_transform(P, c)
    assert M.dtype == np.float32 and M.shape == (4, 4)
    assert np.abs(M - EYE).max() <= 1e-5 and M[3].tolist() == [0., 0., 0., 1.]
    assert np.abs(_make_transform(P, c, 1., (0., 0., 0.), 0., (0., 0., 0.)) - EYE).max() <= 1e-5
    # a pure scale leaves the centre (in camera space: inv(P) c) where it is, to the fp32 rounding of M's entries
    M = _make_transform(P, c, 1.37)
    pc = np.linalg.inv(P.astype(np.float64)) @ np.append(c, 1.)
    M64 = M.astype(np.float64)
    assert (np.abs(M64 @ pc - pc) <= 2. ** -23 * (np.abs(M64) @ np.abs(pc)))[:3].all() and M[3].tolist() == [0., 0., 0., 1.]
    # and any other point moves away from it by the factor, in plane space
    p = np.array([10., 20., 700., 1.])
    moved = P.astype(np.float64) @ M64 @ p
    assert np.allclose(moved[:3] - c, 1.37 * ((P.astype(np.float64) @ p)[:3] - c), rtol=0, atol=1e-2)
    # column vectors: the rotation is about the camera's z axis and comes first, the translation is in plane space
    R = _make_transform(EYE, (0, 0, 0), rotate=0.3)
    assert np.allclose(R @ np.array([1, 0, 0, 1], np.float32), [np.cos(0.3), np.sin(0.3), 0, 1], atol=1e-7)
    T = _make_transform(EYE, (5, 6, 7), translate=(1, 2, 3))
    assert T[:3, 3].tolist() == [1., 2., 3.] and np.array_equal(T[:3, :3], EYE[:3, :3])
    Tp = np.identity(4, np.float32)
    Tp[:3, 3] = (10, 0, 0)
    S = _make_transform(Tp, (0, 0, 0), 2.)              # plane space = camera space + 10 in x: x -> 2 (x + 10) - 10
    assert np.allclose(S @ np.array([1, 1, 1, 1], np.float32), [12, 2, 2, 1])
    K = _make_transform(EYE, (0, 0, 0), 1., (0.5, 0., -0.25))
    assert np.diag(K).tolist() == [1.5, 1., 0.75, 1.]


def test_new_entry_points_reject_bad_and_null_arguments(rdf):
    _lib = importlib.import_module("3d-beats_amd._lib")
    importlib.import_module("3d-beats_amd._build").build()
    names = declared(HEADER)
    for must in ("rdf_points_center", "rdf_points_center_workspace_bytes", "rdf_rerender", "rdf_rerender_workspace_bytes"):
        assert must in names
    lib = _lib.load("labels")
    assert lib.rdf_labels_abi_version() == 1
    assert lib.rdf_rerender_workspace_bytes(848, 480) == 848 * 480 * 8 and lib.rdf_rerender_workspace_bytes(-1, 4) == 0
    assert lib.rdf_rerender_workspace_bytes(32769, 4) == 0 and lib.rdf_rerender_workspace_bytes(0, 4) == 0
    assert lib.rdf_points_center_workspace_bytes(1) == 32 and lib.rdf_points_center_workspace_bytes(257) == 64
    assert lib.rdf_points_center_workspace_bytes(848 * 480) == 1024 * 32 and lib.rdf_points_center_workspace_bytes(-1) == 0
    # rejected arguments launch nothing, so they can be checked without a device
    assert lib.rdf_points_center(-1, None, None, None, None) == -1
    assert lib.rdf_points_center(16, None, None, None, None) == -2
    m = np.identity(4, np.float32)
    cam = (64., 2.5, 2., 50., 50000.)
    assert lib.rdf_rerender(-1, 4, None, None, m.ctypes.data, *cam, None, None, None, None) == -1
    assert lib.rdf_rerender(4, 4, None, None, m.ctypes.data, 0., 2.5, 2., 50., 50000., None, None, None, None) == -1
    assert lib.rdf_rerender(4, 4, None, None, m.ctypes.data, 64., 2.5, 2., 0., 50000., None, None, None, None) == -1
    assert lib.rdf_rerender(4, 4, None, None, m.ctypes.data, 64., 2.5, 2., 50., 40., None, None, None, None) == -1
    assert lib.rdf_rerender(4, 40000, None, None, m.ctypes.data, *cam, None, None, None, None) == -3
    assert lib.rdf_rerender(4, 4, None, None, m.ctypes.data, *cam, None, None, None, None) == -2
    assert lib.rdf_rerender(4, 4, None, None, None, *cam, None, None, None, None) == -2
    assert lib.rdf_rerender(0, 4, None, None, None, *cam, None, None, None, None) == 0
    assert b"affine" in lib.rdf_labels_error_string(-1)


def test_the_new_names_are_public(rdf):
    for name in ("center", "make_transform", "run"):
        assert callable(getattr(rdf.SceneRerender, name)), name
    assert "SceneRerender" in rdf.__all__
    import inspect
    p = inspect.signature(rdf.RecordingConverter.__init__).parameters
    got = {k: p[k].default for k in ("rerender", "scale_variance", "scale_skew_variance", "rotate_variance",
                                     "translate_variance", "augment_seed")}
    assert got == {"rerender": False, "scale_variance": 0.1, "scale_skew_variance": 0., "rotate_variance": 0.,
                   "translate_variance": 0., "augment_seed": None}


def _want_draws(rng, frame, sv, kv, rv, tv):
    """live_data_convert.py:252-265 against one generator."""
    if not frame > 2:
        sv = kv = rv = tv = 0
    return (rng.normal(1, sv, 1)[0], rng.normal(0, kv, 3), rng.normal(0., rv, 1)[0], rng.normal(0., tv, 3))


def test_draw_order_and_the_two_unrandomised_first_frames():
    dc = importlib.import_module("3d-beats_amd.data_convert")
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    for frame in range(1, 7):
        scale, skew, rotate, translate = dc.draw_augmentation(a, frame, 0.1, 0.02, 0.3, 4.)
        w = _want_draws(b, frame, 0.1, 0.02, 0.3, 4.)
        assert scale == w[0] and np.array_equal(skew, w[1]) and rotate == w[2] and np.array_equal(translate, w[3])
        if frame <= 2:
            assert scale == 1. and not skew.any() and rotate == 0. and not translate.any()
        else:
            assert scale != 1. and skew.all() and rotate != 0. and translate.all()
    # the reference's defaults only scale
    scale, skew, rotate, translate = dc.draw_augmentation(np.random.default_rng(1), 3, 0.1, 0., 0., 0.)
    assert scale != 1. and not skew.any() and rotate == 0. and not translate.any()


# ------------------------------------------------------------------ CPU: the scenes of the device tests -------------------
def test_the_gpu_scenes_exercise_what_they_are_meant_to():
    pts, color, cam, cases = _case(33, 17)
    by = {name: want for name, _, want in cases}
    valid = pts[..., 3] > 0
    assert 0 < valid.sum() < valid.size and not valid[0, 0]
    assert by["identity"][2].max() == 1 and 0 < (by["identity"][0] > 0).sum() < valid.sum()
    assert (by["scale 1.25"][0] > 0).sum() > 1.4 * (by["identity"][0] > 0).sum() > 2.4 * (by["scale 0.8 with skew"][0] > 0).sum()
    moved = by["rotated and pushed out of the frame"]
    assert (moved[0] > 0).sum() < 0.9 * (by["identity"][0] > 0).sum() and moved[0][:, -1].any()
    assert moved[2].max() > 1                                   # the step's stretched triangles overlap the far side
    far = by["partly beyond zmax"][0]
    assert 0 < (far > 0).sum() < (by["identity"][0] > 0).sum() and far.max() <= 50000 and far[far > 0].min() > 40000


# ------------------------------------------------------------------ CPU: do the device cases bite? --------------------------
def _outputs(mod, name):
    """What the device test of case `name` compares, under the restatement module `mod`."""
    if name == "scenes 33 x 17":
        pts, color, cam, cases = rc.case(33, 17)
        return [a for _, M, _ in cases for a in mod.rerender(pts, color, M, *cam)[:2]]
    return list(rc.rerender_of(mod, rc.GRID_CASES[name]))


_true_outputs = {}


def _true(name):
    if name not in _true_outputs:
        with np.errstate(all="ignore"):
            _true_outputs[name] = _outputs(rn, name)
    return _true_outputs[name]


def test_the_unchanged_copy_is_the_restatement_bit_for_bit():
    copy = rc.mutant()
    assert copy is not rn and copy.rerender is not rn.rerender
    with np.errstate(all="ignore"):
        for name in rc.KILLS:
            assert mutants.same(_outputs(copy, name), _true(name)), name


def test_a_mutant_that_no_longer_applies_fails_loudly():
    with pytest.raises(AssertionError, match="0 times"):
        mutants.load("rerender_numpy", [("zz >= F(z_min)", "zz > F(z_min)")])
    with pytest.raises(AssertionError, match="2 times"):
        mutants.load("rerender_numpy", [("np.floor(((F(f) * ", "np.trunc(((F(f) * ")])


@pytest.mark.parametrize("name", list(rc.KILLS))
def test_each_mutant_changes_the_case_meant_for_it(name, capsys):
    """A wrong reading of a rule that leaves a case's images unchanged would pass the GPU test of that case."""
    killed = {}
    with np.errstate(all="ignore"):
        for m in rc.MUTANTS:
            killed[m] = mutants.changed(_outputs(rc.mutant(m), name), _true(name))
    with capsys.disabled():
        print(f"\n  {name}: outputs changed by " + ", ".join(f"{m}: {k}" for m, k in killed.items() if k), end="")
    for m in rc.KILLS[name]:
        assert killed[m] > 0, (name, m)
    for m in rc.EQUIVALENT:
        assert killed[m] == 0, (name, m)


def test_every_mutant_is_met_by_some_case():
    assert set(m for ms in rc.KILLS.values() for m in ms) | set(rc.EQUIVALENT) == set(rc.MUTANTS)
    assert not set(m for ms in rc.KILLS.values() for m in ms) & set(rc.EQUIVALENT)
    assert set(rc.KILLS) == {"scenes 33 x 17"} | set(rc.GRID_CASES) and all(len(why) > 40 for why in rc.EQUIVALENT.values())


def _aimed_vertices():
    """Points and an identity transform that put z' on +0, -0 and the smallest subnormal with x' and y' each of 0, finite,
    inf and NaN; one ordinary point, so that the comparison is not of nothing."""
    tiny = np.array([1], np.uint32).view(np.float32)[0]
    vals = (0., 3.5, -2., np.inf, -np.inf, np.nan)
    rows = [(x, y, z, 1.) for z in (0., -0., tiny) for x in vals for y in vals] + [(10., -20., 640., 1.)]
    return np.array(rows, np.float32).reshape(1, -1, 4)


def test_equivalent_z_ge_0_draws_no_other_vertex():
    m = rc.mutant("z' >= 0 drawable")
    pts = _aimed_vertices()
    with np.errstate(all="ignore"):
        for cam in ((64., 0., 0.), (64., 3.5, 2.25), (1e-30, 0., 0.), (3e38, 0., 0.)):
            want, got = rn.vertices(pts, EYE, *cam), m.vertices(pts, EYE, *cam)
            assert mutants.same(list(want), list(got)), cam
    # what is drawable: the ordinary point, and a subnormal z' only where x' = y' = 0 (any other finite x' overflows)
    ok = rn.vertices(pts, EYE, 64., 0., 0.)[4].reshape(-1)
    assert ok[-1] and ok.sum() == 2 and ok[72] and pts[0, 72].tolist()[:2] == [0., 0.] and not ok[:72].any()
    # and a grid that holds such points draws the same image
    grid_pts = np.zeros((8, 8, 4), np.float32)
    grid_pts[:, :] = pts.reshape(-1, 4)[:64].reshape(8, 8, 4)
    color = np.full((8, 8, 3), 9, np.uint8)
    with np.errstate(all="ignore"):
        assert mutants.same(list(rn.rerender(grid_pts, color, EYE, 64., 0., 0.)), list(m.rerender(grid_pts, color, EYE, 64., 0., 0.)))


def test_equivalent_a_kept_triangle_of_area_0_covers_nothing():
    m = rc.mutant("a triangle of area 0 kept")
    # quads whose triangles have no area: all four points on one screen position, on a horizontal, a vertical and a
    # diagonal line through pixel centres (where an e_k of 0 would count on a top or left edge), and one proper quad
    placed = {}
    for c, (dx, dy) in enumerate(((0., 0.), (1., 0.), (0., 1.), (1., 1.))):
        for k, (r, cc) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            placed[r + 2 * c, cc] = (1.5 + k * dx, 1.5 + k * dy, 256.)
    placed.update({(r + 8, c): (2.25 + 4 * c, 8.25 + 4 * r, 256.) for r in range(2) for c in range(2)})
    pts, color = rc.grid(16, 16, (64., 7.5, 7.25), placed)
    X, Y, _, has, ok = rn.vertices(pts, EYE, 64., 7.5, 7.25)
    ids, tris = rn.mesh(has)
    area = rn._edge(*(a.reshape(-1)[tris[:, k]] for k in (0, 1) for a in (X, Y)), X.reshape(-1)[tris[:, 2]], Y.reshape(-1)[tris[:, 2]])
    assert (area == 0).sum() >= 8 and (area != 0).sum() >= 2       # (the rows between the four also make quads)
    with np.errstate(all="ignore"):
        want, got = rn.rerender(pts, color, EYE, 64., 7.5, 7.25), m.rerender(pts, color, EYE, 64., 7.5, 7.25)
    assert mutants.same(list(want), list(got)) and want[2].sum() >= 16


def test_the_grid_cases_hold_what_they_name():
    for name, c in rc.GRID_CASES.items():
        depth, color, count = rc.grid_want(name)
        if c["depth"] is not None:                      # the images worked by hand
            assert np.array_equal(depth, c["depth"]), name
        assert c["W"] <= 16 and c["H"] <= 16
    X, Y, _, _, ok = rn.vertices(rc.GRID_CASES["edges on pixel centres"]["pts"], EYE, 64., 7.5, 7.25)
    assert sorted(set(X[:3, :3].ravel().tolist())) == [256 * i + 128 for i in (2, 6, 10)]
    assert sorted(set(Y[:3, :3].ravel().tolist())) == [256 * j + 128 for j in (3, 7, 11)]
    assert rc.grid_want("edges on pixel centres")[2].max() == 1           # no pixel twice, shared edges and diagonals included
    # the fold: every drawn pixel is reached by two fragments of one z, and the lower id's colour is not the higher's
    c = rc.GRID_CASES["folded back at one depth"]
    depth, color, count = rc.grid_want("folded back at one depth")
    assert (count[depth > 0] == 2).all() and (depth > 0).sum() == 64
    other = rc.mutant("depth ties to the highest id").rerender(c["pts"], c["color"], c["M"], *c["cam"])
    assert np.array_equal(other[0], depth) and (other[1] != color).any(-1)[depth > 0].mean() > 0.9
    # the limits: the far vertex snaps to +-2^20 exactly, or one beyond
    for axis, k in (("x", 0), ("y", 1)):
        for sign, s in ((1, "+"), (-1, "-")):
            for past in (0, 1):
                c = rc.GRID_CASES[f"{axis} snapped to {s}" + ("(2^20 + 1)" if past else "2^20")]
                with np.errstate(all="ignore"):
                    fx = np.floor(((F(64.) * c["pts"][..., k]) / c["pts"][..., 2]) * F(256) + F(0.5))
                assert (fx[:2, :2] == sign * (2 ** 20 + past)).sum() == 1, (axis, sign, past)
    # the fma literals: the rounded rows snap A and the point below it on column 2's centres, the contracted rows beyond
    c = rc.GRID_CASES["rows that a contraction would snap elsewhere"]
    X = rn.vertices(c["pts"], c["M"], *c["cam"])[0]
    Xc = rc.mutant("vertex rows contracted").vertices(c["pts"], c["M"], *c["cam"])[0]
    assert X[0, 0] == X[1, 0] == rc.FMA_X == 256 * 2 + 128 and Xc[0, 0] == Xc[1, 0] == rc.FMA_X_CONTRACTED
    depth = rc.grid_want("rows that a contraction would snap elsewhere")[0]
    assert (depth[:7, 2] > 0).all() and not depth[:, :2].any()
    # the sums: an edge function beyond 2^24
    c = rc.GRID_CASES["sums that another order would round elsewhere"]
    X, Y, _, _, _ = rn.vertices(c["pts"], EYE, *c["cam"])
    assert abs(int(rn._edge(X[0, 0], Y[0, 0], X[0, 1], Y[0, 1], X[1, 0], Y[1, 0]))) > 2 ** 24


# ------------------------------------------------------------------ GPU ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rc.GRID_CASES))
def test_rerender_of_the_grid_cases_matches_the_restatement_bit_for_bit(name, rdf, gpu_runtime):
    c = rc.GRID_CASES[name]
    W, H = c["W"], c["H"]
    want_depth, want_color, _ = rc.grid_want(name)
    rr = rdf.SceneRerender((H, W), c["cam"], z_near=c["zmin"], z_far=c["zmax"])
    p, col = rdf.to_device(c["pts"]), rdf.to_device(c["color"])
    depth, out = rdf.DeviceArray((H, W), np.uint16).fill(7), rdf.DeviceArray((H, W, 3), np.uint8).fill(7)
    rr.run(p, col, c["M"], depth, out)
    got_depth, got_color = depth.get(), out.get()
    print(f"{name}: {int((want_depth > 0).sum())} pixels drawn, {int((got_depth != want_depth).sum())} depths and "
          f"{int((got_color != want_color).any(-1).sum())} colours differ")
    if c["depth"] is not None:
        assert np.array_equal(got_depth, c["depth"]), name
    assert np.array_equal(got_depth, want_depth) and np.array_equal(got_color, want_color), name
    assert (rr._keys.get() == 0xFF).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", rc.SIZES)
def test_rerender_matches_the_restatement_bit_for_bit(W, H, rdf, gpu_runtime):
    pts, color, cam, cases = _case(W, H)
    rr = rdf.SceneRerender((H, W), cam)
    p, c = rdf.to_device(pts), rdf.to_device(color)
    depth, out = rdf.DeviceArray((H, W), np.uint16), rdf.DeviceArray((H, W, 3), np.uint8)
    for name, M, (want_depth, want_color, _) in cases:
        runs = []
        for _ in range(2):                              # the second run finds the key buffer as the first one left it
            depth.fill(7)
            out.fill(7)
            rr.run(p, c, M, depth, out)
            runs.append((depth.get(), out.get()))
        bad = int((runs[0][0] != want_depth).sum()), int((runs[0][1] != want_color).any(-1).sum())
        print(f"{W}x{H} {name}: {int((want_depth > 0).sum())} pixels drawn, {bad[0]} depths and {bad[1]} colours differ")
        assert np.array_equal(runs[0][0], want_depth) and np.array_equal(runs[0][1], want_color), name
        assert np.array_equal(runs[1][0], runs[0][0]) and np.array_equal(runs[1][1], runs[0][1]), name
        assert (rr._keys.get() == 0xFF).all(), name
    assert np.array_equal(c.get(), color) and np.array_equal(p.get(), pts)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 4097, 70 * 130])
def test_points_center_matches_float64_sums(n, rdf, gpu_runtime):
    rng = np.random.default_rng(n)
    pts = (rng.normal(0, 1, (n, 4)) * (300., 300., 900., 1.)).astype(np.float32)
    pts[:, 3] = rng.random(n) < 0.7
    pts[pts[:, 3] == 0] = 0
    if n == 1:
        pts[0] = (1.5, -2.25, 700.125, 1.)
    rr = rdf.SceneRerender((130, 70), (70., 34.5, 64.5))
    p = rdf.to_device(pts)
    got = rr.center(p).get()
    want = rn.center_sums(pts)
    bound = n * 2. ** -52 * np.abs(pts.astype(np.float64)).sum(0)
    print(f"n = {n}: |got - want| = {np.abs(got - want)}, bound {bound}")
    assert got.dtype == np.float64 and got.shape == (4,) and (np.abs(got - want) <= bound).all()
    assert got[3] == pts[:, 3].sum()
    again = rr.center(p).get()
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


def _recording(n, H, W, K):
    """n (depth, colour) pairs: the tilted table with two raised "hands" of tests/test_frontend.py, the hands painted in K
    vertical stripes of the palette (with noise), the rest of the colour image black (as tests/test_color_labels.py)."""
    from test_frontend import scene
    frames = []
    for i in range(n):
        depth, hand, fpp = scene(H, W, W / 2., tilt_deg=18. + 0.3 * i, box_h=80. + i, holes=0.02, seed=40 + i, hand_scale=1.5)
        rng = np.random.default_rng(900 + i)
        stripe = (np.arange(W)[None, :] * K // W + i) % K
        color = np.clip(PALETTE8[:K].astype(np.int64)[np.broadcast_to(stripe, (H, W))] + rng.integers(-8, 9, (H, W, 3)), 0, 255)
        color[~hand] = 0
        frames.append((depth, color.astype(np.uint8)))
    return frames, fpp


@pytest.mark.gpu
def test_recording_converter_rerenders_end_to_end(rdf, gpu_runtime, tmp_path):
    from PIL import Image
    n, H, W, K, T, G, seed = 4, 48, 64, 3, 40., 600, 21
    variances = (0.1, 0.03, 0.05, 3.)
    frames, fpp = _recording(n, H, W, K)
    out = tmp_path / "augmented"
    conv = rdf.RecordingConverter(str(out), (H, W), fpp, K, T, num_random_guesses=G, seed=12, rerender=True,
                                  scale_variance=variances[0], scale_skew_variance=variances[1],
                                  rotate_variance=variances[2], translate_variance=variances[3], augment_seed=seed)
    fits, tforms = [], []
    make, rerender_image = conv.calibrated_plane.make, conv._rerender_image

    def recording_make(*a, **kw):
        plane = make(*a, **kw)
        fits.append((conv.frame_count, conv.calibrated_plane.rand_cu.get(), plane.copy()))
        return plane

    def recording_rerender():
        got = rerender_image()
        tforms.append(conv.obj_tform.copy())
        return got
    conv.calibrated_plane.make = recording_make
    conv._rerender_image = recording_rerender
    init = np.random.default_rng(2).integers(0, 256, (8, K, 3)).astype(np.uint8)
    init[3] = PALETTE8[:K]
    assert conv.convert(frames, init) == n and len(tforms) == n and [f[0] for f in fits] == [1]

    f, ppx, ppy = np.float32(fpp[0]), np.float32(fpp[1]), np.float32(fpp[2])
    plane = fnp.calibrate(fits[0][1], fnp.deproject(frames[0][0], ppx, ppy, f), W, H, T)[0].reshape(4, 4)
    assert np.array_equal(plane.view(np.uint32), fits[0][2].view(np.uint32))
    rng = np.random.default_rng(seed)
    mapping, drawn = None, 0
    for i, (depth, color) in enumerate(frames):
        in_plane = fnp.filter_by_plane(fnp.transform(fnp.deproject(depth, ppx, ppy, f), plane), T)
        s = rn.center_sums(in_plane)
        scale, skew, rotate, translate = _want_draws(rng, i + 1, *variances)
        M = _make_transform(plane, s[:3] / s[3], scale, skew, rotate, translate)
        # the device's centre is these sums in another order of addition: n 2^-52 sum|v| / count, some 1e-9 for 3072 points
        # of magnitude 10^3, reaches an entry of the float64 product multiplied by at most |1 - scale| < 1; rounding to fp32
        # then moves an entry by one unit in its last place at most.  The images are compared for the matrix that was used.
        assert (np.abs(tforms[i] - M) <= 2. ** -23 * np.abs(M) + 1e-8).all(), i
        if i < 2:
            zero = _make_transform(plane, s[:3] / s[3])
            assert (np.abs(tforms[i] - zero) <= 2. ** -23 * np.abs(zero) + 1e-8).all(), i
            assert np.abs(tforms[i] - EYE).max() <= 1e-5
        else:
            assert np.abs(tforms[i] - EYE).max() > 1e-3
        pts = fnp.transform(in_plane, np.linalg.inv(plane))
        d, c, _ = rn.rerender(pts, color, tforms[i], f, ppx, ppy)
        drawn += int((d > 0).sum())
        if mapping is None:
            mapping = lnp.make_color_mapping(c, init, 32)[0]
            assert np.array_equal(conv.color_mapping, mapping)
        _, labels, rgba, d = lnp.label_frame(mapping, c, d)
        got_labels = np.array(Image.open(out / f"{i:08d}_labels.png")).astype(np.uint16)
        assert np.array_equal(np.array(Image.open(out / f"{i:08d}_depth.png")).astype(np.uint16), d), i
        assert np.array_equal(got_labels, labels), i
        assert np.array_equal(np.array(Image.open(out / f"{i:08d}_labels_rgba.png")), rgba), i
        assert set(np.unique(got_labels).tolist()) <= set(range(K + 1)) and (got_labels > 0).sum() > 50, i
    assert drawn > 400


@pytest.mark.gpu
def test_without_rerender_the_converter_writes_the_same_files(rdf, gpu_runtime, tmp_path):
    n, H, W, K, T, G = 3, 48, 64, 3, 40., 600
    frames, fpp = _recording(n, H, W, K)
    init = np.random.default_rng(2).integers(0, 256, (8, K, 3)).astype(np.uint8)
    init[3] = PALETTE8[:K]
    kws = ({}, {"rerender": False, "scale_variance": 0.3, "translate_variance": 5., "augment_seed": 1})
    for name, kw in zip(("plain", "off"), kws):
        conv = rdf.RecordingConverter(str(tmp_path / name), (H, W), fpp, K, T, num_random_guesses=G, seed=12, **kw)
        assert conv.convert(frames, init) == n and not hasattr(conv, "scene_rerender")
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "off")) and len(files) == 3 * n + 1
    for name in files:
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "off" / name).read_bytes(), name
