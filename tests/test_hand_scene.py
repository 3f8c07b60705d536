"""Labelled hand frames (librdf_labels.so: rdf_hand_scene_render; HandModel; HandSceneRenderer) against the restatement in
tests/hand_scene_numpy.py.  The CPU tests pin the restatement to answers worked by hand from the rules in
include/rdf_labels.h and the hand model to its own geometry; every GPU comparison of images is bit for bit, with no pixel
or case left out.

Hand-worked scenes use a focal length of 64 and depths that are powers of two, so that projection and snapping are exact."""
import importlib
import os

import numpy as np
import pytest

import hand_scene_cases as hc
import hand_scene_numpy as hs
import mutants
import rerender_cases as rc
from abi_helpers import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rdf_labels.h")
F = np.float32
EYE12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def _hm():
    return importlib.import_module("3d-beats_amd.hand_model")


def _screen(sx, sy, z, f=64., ppx=0., ppy=0.):
    return ((sx - ppx) * z / f, (sy - ppy) * z / f, z)


# ------------------------------------------------------------------ CPU: the restatement ------------------------------------
def test_one_triangle_covers_the_pixels_and_has_the_depth_worked_by_hand():
    # screen A = (1.25, 0.75) at 512, B = (6.25, 0.75) and C = (1.25, 5.75) at 1024: snapped (320, 192), (1600, 192), (320, 1472).
    # Area > 0.  Centres (i + .5, j + .5) inside: i + .5 >= 1.25, j + .5 >= .75 and (i + .5) + (j + .5) < 7; the centres with
    # i + j == 6 lie ON the edge B -> C, whose direction (-1280, +1280) is neither left (D.Y < 0) nor top: excluded.
    verts = np.array([_screen(1.25, 0.75, 512.), _screen(6.25, 0.75, 1024.), _screen(1.25, 5.75, 1024.)], np.float32)
    assert verts.tolist() == [[10., 6., 512.], [100., 12., 1024.], [20., 92., 1024.]]
    depth, labels, info = hs.render(9, 8, verts, [0, 0, 0], [[0, 1, 2]], [5], EYE12.reshape(1, 1, 12), None, 64., 0., 0.)
    want = np.zeros((8, 9), bool)
    for j in range(8):
        for i in range(9):
            want[j, i] = i >= 1 and j >= 1 and i + j <= 5
    assert want.sum() == 10
    assert np.array_equal(labels[0] == 5, want) and np.array_equal(labels[0] != 0, want) and np.array_equal(depth[0] != 65535, want)
    # pixel (2, 2), P = (640, 640): e0 = (-1280)(448) - (1280)(-960) = 655360, e1 = -(-1280)(320) = 409600, e2 = 1280 * 448 =
    # 573440, together 1280^2; q_k = e_k / z_k = 1280 (z 512), 400, 560 (z 1024); z = 1638400 / 2240 = 731.43
    assert depth[0, 2, 2] == 731
    # pixel (1, 1), P = (384, 384): e = (1310720, 81920, 245760), q = (2560, 80, 240), z = 1638400 / 2880 = 568.9
    assert depth[0, 1, 1] == 568
    fr = info[0]["fr"]
    assert len(fr["pix"]) == 10 and set(fr["tri"].tolist()) == {0}


def test_of_two_coincident_triangles_the_lower_index_wins():
    verts = np.array([_screen(1.25, 0.75, 512.), _screen(6.25, 0.75, 1024.), _screen(1.25, 5.75, 1024.)], np.float32)
    for label in ([3, 4], [4, 3]):
        depth, labels, info = hs.render(9, 8, verts, [0, 0, 0], [[0, 1, 2], [0, 1, 2]], label, EYE12.reshape(1, 1, 12), None,
                                        64., 0., 0.)
        assert len(info[0]["fr"]["pix"]) == 20 and (labels[0] != 0).sum() == 10
        assert set(np.unique(labels[0]).tolist()) == {0, label[0]}
    # the other winding of the same triangle covers the same pixels
    a = hs.render(9, 8, verts, [0, 0, 0], [[0, 1, 2]], [1], EYE12.reshape(1, 1, 12), None, 64., 0., 0.)
    b = hs.render(9, 8, verts, [0, 0, 0], [[0, 2, 1]], [1], EYE12.reshape(1, 1, 12), None, 64., 0., 0.)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_table_has_depth_d_over_nz_at_the_principal_point():
    W, H = 8, 6
    table = np.array([0.2, -0.1, 0.75, 1000.3], np.float32)
    none = np.zeros((0, 3), np.float32)
    for empty in (0, 65535):
        depth, labels, info = hs.render(W, H, none, [], np.zeros((0, 3), np.int32), [], np.zeros((1, 1, 12), np.float32), table,
                                        64., 3.5, 2.5, empty_depth=empty)
        assert depth[0, 2, 3] == 1333           # pixel (3, 2) is sampled at (3.5, 2.5): rx = ry = 0, 1000.3 / 0.75 = 1333.7
        assert not labels.any() and info[0]["table"].all()
        # one pixel to the right rx = 1 / 64: 1000.3 / (0.2 / 64 + 0.75) = 1328.2
        assert depth[0, 2, 4] == 1328 and depth[0, 3, 3] == 1336        # below: 1000.3 / (0.75 - 0.1 / 64) = 1336.5
    # a table behind the camera, or outside the depth range, is not there: every pixel is empty
    for tb in ((0., 0., -1., 1000.), (0., 0., 1., 40.), (0., 0., 1., 60000.)):
        depth, labels, info = hs.render(W, H, none, [], np.zeros((0, 3), np.int32), [], np.zeros((1, 1, 12), np.float32),
                                        np.array(tb, np.float32), 64., 3.5, 2.5, empty_depth=7)
        assert (depth == 7).all() and not labels.any() and not info[0]["table"].any()


def test_a_quad_that_dips_under_a_table_loses_exactly_where_it_is_deeper():
    W, H = 33, 17
    c = hc.case(W, H)
    depth, labels, info = c["want"][1, "table, clean, empty 65535"]
    fr, winner, zt = info[0]["fr"], info[0]["winner"], info[0]["zt"]
    assert info[0]["table"].all() and (zt == F(1000.)).all() and (winner >= 0).all()       # the quad fills the frame
    zm = fr["z"][winner]
    lab = c["mesh"][3][fr["tri"][winner]]
    under = zm > zt
    assert 100 < under.sum() < W * H - 100
    assert np.array_equal(labels[0].reshape(-1), np.where(under, 0, lab))
    assert np.array_equal(depth[0].reshape(-1), np.where(under, 1000, np.trunc(zm)).astype(np.uint16))
    # 1 / z is linear on the screen between 1 / 896 at x = -0.3 W and 1 / 1152 at x = 1.3 W: it is 1 / 1000 at
    u = (1 / 896 - 1 / 1000) / (1 / 896 - 1 / 1152)
    x_cross = -0.3 * W + u * 1.6 * W
    row = labels[0, H - 1]              # no other triangle reaches the last row
    assert (row[:int(x_cross - 0.5)] != 0).all() and (row[int(x_cross + 0.5) + 1:] == 0).all()


def test_an_index_out_of_range_drops_only_its_triangle():
    W, H = 33, 17
    c = hc.case(W, H)
    verts, part, tris, label = c["mesh"]
    bad = list(hc.TRI["bad"])
    for n_frames in (1, 3):
        depth, labels, info = c["want"][n_frames, "plain dataset frame"]
        good = hs.render(W, H, verts[:-1], part[:-1], np.delete(tris, bad, 0), np.delete(label, bad), c["tforms"][:n_frames],
                         None, *c["cam"])
        assert np.array_equal(depth, good[0]) and np.array_equal(labels, good[1])
        assert not (labels == 9).any() and not np.isin(info[0]["fr"]["tri"], bad).any()
    # the bad triangles would be visible if their indices were good
    fixed = tris.copy()
    fixed[bad[0]] = (4, 7, 8)
    assert (hs.render(W, H, verts, part, fixed, label, c["tforms"][:1], None, *c["cam"])[1] == 9).any()


def _mix_py(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_holes_and_noise_hit_the_pixels_the_written_out_hash_says():
    W, H, seed = 7, 5, 12345
    table = np.array([[0., 0., 1., 1000.], [0., 0., 1., 2000.]], np.float32)
    none = np.zeros((0, 3), np.float32)
    args = (W, H, none, [], np.zeros((0, 3), np.int32), [], np.zeros((2, 1, 12), np.float32), table, 64., 3., 2.)
    depth, labels, _ = hs.render(*args, empty_depth=0, seed=seed, hole_threshold=1 << 31)
    noisy, _, _ = hs.render(*args, empty_depth=0, seed=seed, noise_amp=3)
    both, _, _ = hs.render(*args, empty_depth=0, seed=seed, hole_threshold=1 << 31, noise_amp=3)
    assert _mix_py(0) == 0 and _mix_py(1) == 0x688990C0
    holes = 0
    for n in range(2):
        base = _mix_py(seed + n * 0x9E3779B9)
        for p in range(W * H):
            h = _mix_py(base ^ p)
            h2 = _mix_py(h ^ 0x85EBCA6B)
            clean = 1000 * (n + 1)
            j, i = divmod(p, W)
            assert depth[n, j, i] == (0 if h < (1 << 31) else clean), (n, p)
            assert noisy[n, j, i] == clean + h2 % 7 - 3, (n, p)
            assert both[n, j, i] == (0 if h < (1 << 31) else clean + h2 % 7 - 3), (n, p)
            holes += h < (1 << 31)
    assert 20 < holes < 50                  # about half of 70
    # frame 1 under this seed is frame 0 under seed + 0x9e3779b9: a batch can be split
    split, _, _ = hs.render(W, H, none, [], np.zeros((0, 3), np.int32), [], np.zeros((1, 1, 12), np.float32), table[1:], 64., 3., 2.,
                            empty_depth=0, seed=(seed + 0x9E3779B9) & 0xFFFFFFFF, hole_threshold=1 << 31, noise_amp=3)
    assert np.array_equal(split[0], both[1])
    # the clamp: noise never makes a drawn pixel look empty, whichever empty value is in use
    deep = np.array([[0., 0., 1., 65534.5]], np.float32)
    lo, _, _ = hs.render(W, H, none, [], np.zeros((0, 3), np.int32), [], np.zeros((1, 1, 12), np.float32), deep, 64., 3., 2.,
                         zmax=70000., seed=1, noise_amp=500)
    assert lo.max() == 65534 and lo.min() >= 65534 - 500


def test_the_gpu_scenes_exercise_what_they_are_meant_to():
    W, H = 33, 17
    c = hc.case(W, H)
    verts, part, tris, label = c["mesh"]
    for n_frames in (1, hc.MAX_FRAMES):
        depth, labels, info = c["want"][n_frames, "table, clean, empty 65535"]
        fr, winner, zt, mesh = info[0]["fr"], info[0]["winner"], info[0]["zt"], info[0]["mesh"]
        # mesh beats table and table beats mesh
        assert (mesh & info[0]["table"]).any() and ((winner >= 0) & ~mesh).any()
        assert (labels[0] != 0).any() and ((labels[0] == 0) & (depth[0] != 65535)).any()
        # a tie: both copies reach the depth test with the same key but for the index, and the lower index is shown
        t0, t1 = hc.TRI["tie"]
        p0, p1 = fr["pix"][fr["tri"] == t0], fr["pix"][fr["tri"] == t1]
        assert len(p0) > 20 and np.array_equal(np.sort(p0), np.sort(p1))
        assert np.array_equal(fr["z"][fr["tri"] == t0][np.argsort(p0)], fr["z"][fr["tri"] == t1][np.argsort(p1)])
        assert (labels[0].reshape(-1)[p0] == label[t0]).all() and not (labels == label[t1]).any()
        # pixels on a shared edge: their centres are on it, and exactly one of the two triangles takes each
        X, Y, _, ok = hs.vertices(verts, part, c["tforms"][0], *c["cam"])
        assert X[4] == X[5] == 256 * hc.EDGE_COLUMN + 128 and ok[4] and ok[5]
        e0, e1 = hc.TRI["edge"]
        for j in hc.EDGE_ROWS:
            assert Y[4] < 256 * j + 128 < Y[5]
            p = j * W + hc.EDGE_COLUMN
            assert ((fr["pix"] == p) & np.isin(fr["tri"], (e0, e1))).sum() == 1, j
        # a triangle clipped by each border: a vertex beyond it, fragments in the row or column along it
        quad = np.isin(fr["tri"], hc.TRI["quad"])
        qi, qj = fr["pix"][quad] % W, fr["pix"][quad] // W
        qv = tris[list(hc.TRI["quad"])].reshape(-1)
        assert X[qv].min() < 0 and (qi == 0).any() and X[qv].max() > 256 * W and (qi == W - 1).any()
        assert Y[qv].min() < 0 and (qj == 0).any() and Y[qv].max() > 256 * H and (qj == H - 1).any()
        # one triangle behind the camera: dropped in frame 0
        (behind,) = hc.TRI["behind"]
        z = hs.vertices(verts, part, c["tforms"][0], *c["cam"])[2]
        assert (z[tris[behind]] < 0).all() and not (fr["tri"] == behind).any() and not (labels[0] == label[behind]).any()
        # the variants differ from each other, and so do the frames
        images = [c["want"][n_frames, v[0]][0] for v in hc.VARIANTS]
        assert all(not np.array_equal(a, b) for k, a in enumerate(images) for b in images[k + 1:])
    depth, labels, info = c["want"][hc.MAX_FRAMES, "plain dataset frame"]
    assert (labels[1] == label[hc.TRI["behind"][0]]).any()
    assert not np.array_equal(labels[0], labels[1]) and not np.array_equal(labels[1], labels[2])
    holes = c["want"][hc.MAX_FRAMES, "camera frame with table, holes and noise"][0]
    assert 0.15 < (holes == 0).mean() < 0.35 and not np.array_equal(holes[0] == 0, holes[1] == 0)


def test_the_many_frames_case_reaches_the_frame_loop_and_its_settings_differ():
    c = hc.many_frames_case()
    N, p = hc.MANY_N, hc.MANY_PERIOD
    assert N > hc.MANY_ROWS and N - hc.MANY_ROWS == 6 and hc.MANY_ROWS % p == 1 and hc.MANY_ROWS % 3 == 0
    assert len(c["index"]) == N and c["index"][hc.MANY_ROWS] == 1 and c["tforms"].shape == (p, 3, 12) and c["tables"].shape == (p, 4)
    verts, part, tris, label = c["mesh"]
    (behind,) = hc.TRI["behind"]
    z = [hs.vertices(verts, part, c["tforms"][k], *c["cam"])[2][tris[behind]] for k in range(p)]
    assert [bool((v < 0).all()) for v in z] == [True, False, False, False, True, False, False] and all((v > 0).all() for v in z[1:4])
    for name, with_table, empty in hc.MANY_VARIANTS:
        depth, labels, info = c["want"][name]
        assert depth.shape == (p,) + hc.MANY_SIZE[::-1]
        for a in range(p):
            assert (labels[a] > 0).sum() > 20 and info[a]["mesh"].any(), (name, a)
            for b in range(a + 1, p):
                assert not np.array_equal(depth[a], depth[b]) and not np.array_equal(labels[a], labels[b]), (name, a, b)
        shown = {k for k in range(p) if (labels[k] == label[behind]).any()}
        assert shown and not shown & {0, 4}, name
        if with_table:      # mesh beats table and table beats mesh, in every setting
            assert all((i["mesh"] & i["table"]).any() and ((i["winner"] >= 0) & ~i["mesh"]).any() for i in info)
            assert ((labels == 0) & (depth != empty)).any()
        else:
            assert np.array_equal(depth == empty, labels == 0)
    assert not np.array_equal(c["want"]["without a table"][0], c["want"]["with the cycling tables"][0])


# ------------------------------------------------------------------ CPU: do the device cases bite? --------------------------
def _outputs(mod, name):
    """What the device test of case `name` compares, under the restatement module `mod`."""
    if name != "scene 33 x 17":
        return list(hc.render_of(mod, hc.grid_case(name[6:]) if name.startswith("grid: ") else hc.OWN_CASES[name]))
    c = hc.case(33, 17)
    m, out = c["mesh"], []
    with np.errstate(all="ignore"):
        alike = getattr(mod, "RASTERISES_ALIKE", False)         # (then the scene's own record of rules V and 3 to 6 serves)
        geometry = c["geometry"] if alike else mod.rasterise(33, 17, m[0], m[1], m[2], c["tforms"], *c["cam"])
        for _, with_table, empty, holes, noise in hc.VARIANTS:
            out += list(mod.render(33, 17, *m, c["tforms"], c["tables"] if with_table else None, *c["cam"], empty_depth=empty,
                                   seed=hc.SEED, hole_threshold=holes, noise_amp=noise, geometry=geometry)[:2])
    return out


_true_outputs = {}


def _true(name):
    if name not in _true_outputs:
        _true_outputs[name] = _outputs(hs, name)
    return _true_outputs[name]


def test_the_unchanged_copy_is_the_restatement_bit_for_bit():
    copy = hc.mutant()
    assert copy is not hs and copy.render is not hs.render and copy.fragments is not hs.fragments
    for name in hc.KILLS:
        assert mutants.same(_outputs(copy, name), _true(name)), name
    c = hc.case(33, 17)
    assert all(np.array_equal(a, b) for a, b in zip(_true("scene 33 x 17"), [x for v in hc.VARIANTS for x in c["want"][3, v[0]][:2]]))


def test_a_mutant_that_no_longer_applies_fails_loudly():
    with pytest.raises(AssertionError, match="0 times"):
        mutants.load("hand_scene_numpy", [("~(zm <= z_t)", "~(zm < z_t)")])
    with pytest.raises(AssertionError, match="2 times"):
        mutants.load("hand_scene_numpy", [(".astype(np.float32) + F(0.5))", ".astype(np.float32))")])


@pytest.mark.parametrize("name", list(hc.KILLS))
def test_each_mutant_changes_the_case_meant_for_it(name, capsys):
    """A wrong reading of a rule that leaves a case's images unchanged would pass the GPU test of that case."""
    killed = {m: mutants.changed(_outputs(hc.mutant(m), name), _true(name)) for m in hc.MUTANTS}
    with capsys.disabled():
        print(f"\n  {name}: outputs changed by " + ", ".join(f"{m}: {k}" for m, k in killed.items() if k), end="")
    for m in hc.KILLS[name]:
        assert killed[m] > 0, (name, m)
    for m in hc.EQUIVALENT:
        assert killed[m] == 0, (name, m)


def test_every_mutant_is_met_by_some_case():
    met = set(m for ms in hc.KILLS.values() for m in ms)
    assert met | set(hc.EQUIVALENT) == set(hc.MUTANTS) and not met & set(hc.EQUIVALENT)
    assert set(hc.KILLS) == {"scene 33 x 17"} | {"grid: " + n for n in rc.GRID_CASES} | set(hc.OWN_CASES)
    assert set(rc.FRAGMENT_EDITS) | set(rc.VERTEX_EDITS) <= set(hc.MUTANTS) and all(len(why) > 40 for why in hc.EQUIVALENT.values())


def test_equivalent_z_ge_0_and_area_0_draw_the_same_meshes():
    tiny = np.array([1], np.uint32).view(np.float32)[0]
    vals = (0., 3.5, -2., np.inf, -np.inf, np.nan)
    verts = np.array([(x, y, z) for z in (0., -0., tiny) for x in vals for y in vals] + [(10., -20., 640.), (60., -20., 640.), (10., 30., 640.)],
                     np.float32)
    n = len(verts)
    # every aimed vertex in a triangle with two ordinary ones; triangles without area: one point thrice, and three on a line
    tris = [(k, n - 3, n - 2) for k in range(n - 3)] + [(n - 3, n - 2, n - 1), (n - 3, n - 3, n - 3), (n - 3, n - 2, n - 2)]
    line = np.array([rc.grid(1, 1, (64., 0., 0.), {(0, 0): (1.5 + k, 1.5 + k, 256.)})[0][0, 0, :3] for k in range(3)], np.float32)
    verts = np.concatenate([verts, line])
    tris += [(n, n + 1, n + 2)]
    label = np.arange(1, len(tris) + 1, dtype=np.uint16)
    for name in ("z' >= 0 drawable", "a triangle of area 0 kept"):
        m = hc.mutant(name)
        for cam in ((64., 0., 0.), (64., 3.5, 2.25), (3e38, 0., 0.)):
            with np.errstate(all="ignore"):
                assert mutants.same(list(hs.vertices(verts, np.zeros(len(verts), np.int32), EYE12, *cam)),
                                    list(m.vertices(verts, np.zeros(len(verts), np.int32), EYE12, *cam))), (name, cam)
                want = hs.render(8, 8, verts, np.zeros(len(verts), np.int32), tris, label, EYE12.reshape(1, 1, 12), None, *cam)[:2]
                got = m.render(8, 8, verts, np.zeros(len(verts), np.int32), tris, label, EYE12.reshape(1, 1, 12), None, *cam)[:2]
            assert mutants.same(list(want), list(got)), (name, cam)
    with np.errstate(all="ignore"):
        X, Y, _, ok = hs.vertices(verts, np.zeros(len(verts), np.int32), EYE12, 64., 0., 0.)
        labels = hs.render(8, 8, verts, np.zeros(len(verts), np.int32), tris, label, EYE12.reshape(1, 1, 12), None, 64., 0., 0.)[1]
    assert ok[-6:].all() and ok[:n - 3].sum() == 1 and X[n:].tolist() == Y[n:].tolist() == [384, 640, 896]      # centres on the line
    assert (labels > 0).sum() >= 3                  # the ordinary triangle is drawn


def test_equivalent_table_t_ge_0_shows_no_other_table():
    m = hc.mutant("table t >= 0")
    none = np.zeros((0, 3), np.float32)
    cam = (64., 3.5, 2.5)               # pixel (3, 2) looks along rx = ry = 0
    rows = []
    for d in (0., -0., 5., -5., 1000., np.inf, -np.inf, np.nan):
        # t = +0 everywhere; -0 everywhere; +0 in column 3 only; -0 in column 3 (rx = +-0 times -1, plus -0); +0 at one pixel
        rows += [(0., 0., 0., d), (-0., -0., -0., d), (1., 0., 0., d), (-1., -0., -0., d), (1., 1., 0., d), (0., 0., 1., d)]
    tables = np.array(rows, np.float32)
    args = (8, 6, none, [], np.zeros((0, 3), np.int32), [], np.zeros((len(tables), 1, 12), np.float32), tables, *cam)
    with np.errstate(all="ignore"):
        for zmin, zmax in ((50., 50000.), (1e-30, 3e38)):
            want, got = hs.render(*args, zmin, zmax, 7)[:2], m.render(*args, zmin, zmax, 7)[:2]
            assert mutants.same(list(want), list(got))
            t0 = [hs.table_depth(tb, 8, 6, *cam, zmin, zmax) for tb in tables]
            t1 = [m.table_depth(tb, 8, 6, *cam, zmin, zmax) for tb in tables]
            assert all(mutants.same(a[1], b[1]) for a, b in zip(t0, t1))
    # the inputs are aimed: t is +0 and -0 at pixels of these tables, and an ordinary table among them shows
    j, i = np.mgrid[:6, :8]
    rx = ((i.astype(np.float32) + F(0.5)) - F(3.5)) / F(64.)
    assert rx[0, 3] == 0 and (want[0][5::6] != 7).any() and (want[0][:4] == 7).all()
    t = (F(-1.) * rx + F(-0.) * rx) + F(-0.)
    assert t[0, 3] == 0 and np.signbit(t[0, 3])


def test_the_own_cases_hold_what_they_name():
    inside = np.zeros((16, 16), bool)
    inside[hc.QUAD_PIXELS] = True
    depth, labels = hc.want_of("quad coplanar with the table")
    assert (depth == 512).all() and np.array_equal(labels[0] > 0, inside)                  # worked by hand: z == zt, the mesh shows
    depth, labels = hc.want_of("tables at the ends of the depth range")
    assert np.array_equal(depth[0], np.where(inside, 512, 1024)) and np.array_equal(depth[1], np.where(inside, 512, 7))
    assert (depth[2] == 256).all() and not labels[2].any() and np.array_equal(depth[3], depth[1])
    assert all(np.array_equal(l > 0, inside) for l in labels[[0, 1, 3]])
    c = hc.OWN_CASES["hole threshold on a pixel's own hash"]
    h = hs.hashes(c["seed"], 0, 256)[0]
    depth, labels = hc.want_of("hole threshold on a pixel's own hash")
    at = int(np.nonzero(h == c["holes"])[0][0])
    assert depth[0].reshape(-1)[at] != 0 and (depth[0].reshape(-1)[h < c["holes"]] == 0).all() and (h < c["holes"]).sum() == 128
    assert (depth[0].reshape(-1)[h >= c["holes"]] != 0).all()
    depth, labels = hc.want_of("noise against both clamps")
    assert depth[0].min() == 1 and (depth[0] == 1).sum() > 50 and depth[0].max() == 7
    assert depth[1].max() == 65534 and (depth[1] == 65534).sum() > 30 and depth[1][~inside].min() == 65528
    for name in rc.GRID_CASES:
        want = rc.GRID_CASES[name]["depth"]
        if want is not None:
            assert np.array_equal(hc.want_of("grid: " + name)[0][0], want), name
        # one grid, two restatements: the same depths, and the label of the triangle whose colour the re-render shows
        assert np.array_equal(hc.want_of("grid: " + name)[0][0], rc.grid_want(name)[0]), name


# ------------------------------------------------------------------ CPU: the model ------------------------------------------
def test_every_part_is_a_closed_consistently_wound_mesh():
    hm = _hm()
    for model in (hm.HandModel(), hm.HandModel().mirrored()):
        assert model.verts.dtype == np.float32 and model.tris.dtype == np.int32 and model.verts.shape[1] == 3
        assert 300 <= len(model.tris) <= 1100 and len(model.vert_part) == len(model.verts) and len(model.tri_part) == len(model.tris)
        assert (model.vert_part[model.tris] == model.tri_part[:, None]).all() and set(model.tri_part.tolist()) == set(range(16))
        for p in range(16):
            t = model.tris[model.tri_part == p]
            directed = np.concatenate([t[:, (0, 1)], t[:, (1, 2)], t[:, (2, 0)]])
            have = {(int(a), int(b)) for a, b in directed}
            assert len(have) == len(directed)                           # no directed edge twice
            assert all((b, a) in have for a, b in have), p              # and each has its opposite: two triangles per edge
            # outward: the volume enclosed by the triangles is positive
            v = model.verts[t].astype(np.float64)
            assert np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() > 0, p


def _planar_tip(hm, u, f, spread, flex):
    """The tip's end point in hand space by hand: the base, plus the three segment vectors of a planar chain."""
    a = np.cumsum(flex)
    in_plane = sum(hm.PHALANX_LENGTH[f][k] * u * np.array([np.cos(a[k]), -np.sin(a[k])]) for k in range(3))    # (along, up)
    s = hm.FINGER_REST_SPLAY[f] + spread
    return np.array([hm.FINGER_BASE[f][0] * u - np.sin(s) * in_plane[0], hm.FINGER_BASE[f][1] * u + np.cos(s) * in_plane[0],
                     in_plane[1]])


def test_fingertips_are_where_the_planar_chain_puts_them():
    hm = _hm()
    model = hm.HandModel(units_per_mm=10.)
    rest = model.rest_pose()
    flexed = model.rest_pose()
    for f in range(5):
        flexed[6 + 4 * f:10 + 4 * f] = (0.1 - 0.05 * f, 0.3 + 0.1 * f, 0.5, 0.2 * f)
    for pose in (rest, flexed):
        m = model.part_matrices(pose)
        tips = model.fingertips(pose)
        for f in range(5):
            want = _planar_tip(hm, 10., f, pose[6 + 4 * f], pose[7 + 4 * f:10 + 4 * f])
            got = m[0, model.tip_parts[f]] @ np.array([0., hm.PHALANX_LENGTH[f][2] * 10., 0., 1.])
            assert np.abs(got[:3] - want).max() <= 1e-9 * 2000. and np.array_equal(tips[0, f], got[:3]), f
    assert np.allclose(model.fingertips(rest)[0, 2], [-100., 980. + 970., 0.])         # the middle finger, straight
    # the wrist's pose and the camera come on top: T(wrist) Rz(yaw) Rx(pitch) Ry(roll), then cam_from_plane
    posed = flexed.copy()
    posed[:6] = (120., -340., 700., 0.4, -0.2, 0.3)
    cz, sz, cx, sx, cy, sy = np.cos(0.4), np.sin(0.4), np.cos(-0.2), np.sin(-0.2), np.cos(0.3), np.sin(0.3)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
         @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]))
    cam = np.identity(4)
    cam[:3, :3] = [[1, 0, 0], [0, -1, 0], [0, 0, -1]]
    cam[2, 3] = 5500.
    want = (R @ model.fingertips(flexed)[0].T).T + posed[:3]
    assert np.abs(model.fingertips(posed)[0] - want).max() <= 1e-8
    assert np.abs(model.fingertips(posed, cam)[0] - (want * (1, -1, -1) + (0, 0, 5500.))).max() <= 1e-8
    t = model.part_transforms(np.stack([rest, posed]), cam)
    assert t.dtype == np.float32 and t.shape == (2, 16, 12)
    assert np.array_equal(t, model.part_matrices(np.stack([rest, posed]), cam)[:, :, :3].reshape(2, 16, 12).astype(np.float32))


def test_sample_poses_and_press_sequence_are_reproducible_and_in_range():
    hm = _hm()
    model = hm.HandModel()
    a, b = model.sample_poses(9, np.random.default_rng(4)), model.sample_poses(9, np.random.default_rng(4))
    assert a.shape == (9, 26) and np.array_equal(a, b) and not np.array_equal(a, model.sample_poses(9, np.random.default_rng(5)))
    r = hm.SAMPLE_RANGES
    assert (a[:, 2] >= r["height"][0] * 10).all() and (a[:, 2] <= r["height"][1] * 10).all()
    assert (a[:, 7:10] >= 0).all() and (a[:, 7:10] <= r["flexion"][1]).all() and (np.abs(a[:, 6]) <= r["spread"][1]).all()
    narrow = model.sample_poses(4, np.random.default_rng(4), {"yaw": (0.25, 0.25)})
    assert (narrow[:, 3] == 0.25).all()
    # a press: the tip goes down by the stated speed per frame, stops one tip radius above the table, comes back
    n, f = 21, 1
    seq = model.press_sequence(n, "index", wrist=(0., 0., 450.), speed_mm=4.)
    assert seq.shape == (n, 26) and np.array_equal(seq, model.press_sequence(n, 1, wrist=(0., 0., 450.), speed_mm=4.))
    tip = model.fingertips(seq)[:, f, 2]
    touch = hm.PHALANX_RADIUS[f][2] * 10.
    want = np.maximum(touch, tip[0] - np.minimum(np.arange(n), n - 1 - np.arange(n)) * 40.)
    assert np.abs(tip - want).max() <= 1e-6 and (tip >= touch).all() and (tip[8:13] == tip[10]).all() and tip[10] - touch <= 1e-6
    others = np.delete(np.arange(26), 7 + 4 * f)
    assert (seq[:, others] == seq[0, others]).all() and (model.fingertips(seq)[:, 2] == model.fingertips(seq)[0, 2]).all()


def test_the_mirrored_hand_is_the_mirror_image():
    hm = _hm()
    right = hm.HandModel()
    left = right.mirrored()
    assert left.is_mirrored and not left.mirrored().is_mirrored
    assert np.array_equal(left.verts, right.verts * F((-1, 1, 1))) and np.array_equal(left.tris, right.tris[:, ::-1])
    pose = right.sample_poses(1, np.random.default_rng(2))[0]
    pose[[0, 3, 5]] = 0.                   # a pose that is its own mirror image: wrist on the plane x = 0, no yaw, no roll
    world = []
    for model in (right, left):
        m = model.part_matrices(pose)[0, model.vert_part]
        world.append(np.einsum("vij,vj->vi", m, np.concatenate([model.verts.astype(np.float64), np.ones((len(model.verts), 1))], 1)))
    assert np.abs(world[1][:, :3] - world[0][:, :3] * (-1, 1, 1)).max() <= 1e-9 * 3000.
    # and a general pose of the left hand is the mirror image of the right hand's mirrored pose
    a = right.sample_poses(3, np.random.default_rng(8))
    b = left.sample_poses(3, np.random.default_rng(8))
    assert np.array_equal(b, a * np.where(np.isin(np.arange(26), (0, 3, 5)), -1., 1.))
    assert np.abs(left.fingertips(b) - right.fingertips(a) * (-1, 1, 1)).max() <= 1e-9 * 3000.


def _hand_scene(n_parts, n_poses=1, seed=3, W=106, H=60):
    """Sampled poses of one hand or two under a camera 550 mm above the table, at W x H: everything render needs."""
    hm = _hm()
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    right = hm.HandModel()
    left = right.mirrored()
    cam = (W * 0.7, (W - 1) / 2., (H - 1) / 2.)
    plane = scene.look_down_plane(5500., 0.15)
    inv = np.linalg.inv(plane)
    rng = np.random.default_rng(seed)
    poses = right.sample_poses(n_poses, rng)
    if n_poses == 1:
        poses[0] = right.rest_pose((0., -700., 800.))
    t, verts, part, tris, tri_part = right.part_transforms(poses, inv), right.verts, right.vert_part, right.tris, right.tri_part
    if n_parts == 32:
        shift = np.where(np.arange(26) == 0, 1100., 0.)
        t = np.concatenate([right.part_transforms(poses + shift, inv), left.part_transforms(left.sample_poses(n_poses, rng) - shift, inv)], 1)
        verts, part = np.concatenate([verts, left.verts]), np.concatenate([part, left.vert_part + 16])
        tris, tri_part = np.concatenate([tris, left.tris + len(right.verts)]), np.concatenate([tri_part, left.tri_part])
    return {"cam": cam, "plane": plane, "tforms": t, "mesh": (verts, part, tris), "tri_part": tri_part, "table": scene.table_of_plane(plane)}


def test_a_rest_pose_render_shows_every_id_of_the_fine_scheme():
    hm = _hm()
    s = _hand_scene(16)
    fine, coarse, tips = (hm.HandModel.label_table(k) for k in ("fine", "coarse", "tips"))
    assert fine.tolist() == [1] + [2, 2, 3, 2, 2, 4, 2, 2, 5, 2, 2, 6, 2, 2, 7]
    depth, labels, _ = hs.render(106, 60, *s["mesh"], fine[s["tri_part"]], s["tforms"], None, *s["cam"])
    assert set(np.unique(labels).tolist()) == set(range(8))
    assert ((labels == 0) == (depth == 65535)).all() and 300 < (labels != 0).sum() < 106 * 60 // 2
    # the two-layer scheme: the composite of 'coarse' and 'tips' through the written conditions table is 'fine'
    cfg = hm.HandModel.layered_config("coarse.npy", "tips.npy")
    cond = cfg["conditions"]
    for p in range(16):
        kind, value = cond[coarse[p] - 1]
        if kind == 1:
            assert coarse[p] == cfg["layers"][1]["filter_model_class"] and tips[p] > 0
            kind, value = cond[value + tips[p] - 1]
        else:
            assert tips[p] == 0
        assert kind == 0 and value == fine[p], p
    assert len(cfg["label_colors"]) == max(v for k, v in cond if k == 0) == 7
    assert sorted(hm.HandModel.id_to_color("fine")) == list(range(1, 8)) and sorted(hm.HandModel.id_to_color("tips")) == list(range(1, 6))


# ------------------------------------------------------------------ CPU: the interface --------------------------------------
def test_new_entry_points_reject_bad_and_null_arguments(rdf):
    _lib = importlib.import_module("3d-beats_amd._lib")
    importlib.import_module("3d-beats_amd._build").build()
    names = declared(HEADER)
    for must in ("rdf_hand_scene_render", "rdf_hand_scene_workspace_bytes"):
        assert must in names
    lib = _lib.load("labels")
    assert lib.rdf_labels_abi_version() == 1
    ws = lib.rdf_hand_scene_workspace_bytes
    assert ws(64, 848, 480) == 64 * 848 * 480 * 8 and ws(1, 33, 17) == 33 * 17 * 8
    assert ws(0, 4, 4) == 0 and ws(1, -1, 4) == 0 and ws(1, 32769, 4) == 0 and ws(2, 0, 4) == 0
    assert ws(4, 32768, 32768) == 4 * 8 << 30             # beyond 32 bits

    def call(n_frames=1, W=4, H=4, n_verts=3, n_tris=1, n_parts=1, f=64., ppx=2., ppy=2., zmin=50., zmax=50000., noise=0,
             mesh=None, ws=None, out=(None, None)):
        m = [mesh] * 5
        return lib.rdf_hand_scene_render(n_frames, W, H, n_verts, m[0], m[1], n_tris, m[2], m[3], n_parts, m[4], None, f, ppx, ppy,
                                         zmin, zmax, 65535, 0, 0, noise, ws, out[0], out[1], None)
    # rejected arguments launch nothing, so they can be checked without a device
    assert call(n_frames=0) == -1 and call(W=-1) == -1 and call(n_tris=-1) == -1 and call(n_parts=-2) == -1 and call(n_verts=-1) == -1
    assert call(f=0.) == -1 and call(f=float("inf")) == -1 and call(zmin=0.) == -1 and call(zmax=40.) == -1
    assert call(zmax=float("inf")) == -1 and call(zmin=float("nan")) == -1 and call(noise=-1) == -1 and call(noise=40000) == -1
    assert call(H=40000) == -3
    assert call() == -2                                   # no workspace, no outputs
    assert call(ws=64, out=(128, 256)) == -2              # a mesh is announced and not given
    assert call(n_tris=0, ws=64, out=(128, None)) == -2
    assert call(n_tris=0, ws=4, out=(128, 256)) == -1 and call(n_tris=0, ws=64, out=(129, 256)) == -1      # misaligned
    assert call(n_tris=0, ws=64, out=(128, 128)) == -1    # one buffer for both images
    assert call(W=0) == 0 and call(H=0, ws=64) == 0       # no pixels: nothing to do


def test_the_new_names_are_public(rdf):
    for name in ("render", "make_dataset", "camera_sequence", "transforms", "tri_labels"):
        assert callable(getattr(rdf.HandSceneRenderer, name)), name
    for name in ("part_transforms", "part_matrices", "sample_poses", "press_sequence", "label_table", "layered_config", "mirrored"):
        assert callable(getattr(rdf.HandModel, name)), name
    assert "HandModel" in rdf.__all__ and "HandSceneRenderer" in rdf.__all__
    import inspect
    p = inspect.signature(rdf.HandSceneRenderer.render).parameters
    got = {k: p[k].default for k in ("labels", "table", "empty_depth", "seed", "hole_rate", "noise_amp", "depth_out", "labels_out")}
    assert got == {"labels": "fine", "table": None, "empty_depth": 65535, "seed": 0, "hole_rate": 0., "noise_amp": 0,
                   "depth_out": None, "labels_out": None}
    p = inspect.signature(rdf.HandSceneRenderer.__init__).parameters
    assert (p["model"].default, p["z_near"].default, p["z_far"].default) == (None, 50., 50000.) and "max_frames" in p
    assert inspect.signature(rdf.HandModel.__init__).parameters["units_per_mm"].default == 10.
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    plane = scene.look_down_plane(5500., 0.2)
    assert np.allclose(plane[:3, :3] @ plane[:3, :3].T, np.identity(3)) and np.isclose(np.linalg.det(plane[:3, :3]), 1.)
    assert np.allclose(plane @ (0., 0., 0., 1.), (0., 0., 5500., 1.))              # the camera is that high above the table
    tb = scene.table_of_plane(plane)
    on_table = np.linalg.inv(plane) @ (300., -200., 0., 1.)
    assert tb[3] > 0 and np.isclose(tb[:3] @ on_table[:3], tb[3], rtol=1e-6)


# ------------------------------------------------------------------ GPU -----------------------------------------------------
def _render_raw(rdf, W, H, mesh, tforms, table, cam, empty, seed, holes, noise, keys=None, runs=1, zmin=50., zmax=50000.):
    """rdf_hand_scene_render on an arbitrary mesh: [(depth, labels)] of `runs` calls in a row on one workspace, and the
    workspace's bytes after the last."""
    _lib = importlib.import_module("3d-beats_amd._lib")
    lib = _lib.load("labels")
    rt = rdf.get_runtime()
    verts, part, tris, label = mesh
    N, P = tforms.shape[:2]
    dev = [rdf.to_device(np.ascontiguousarray(a)) for a in (verts.astype(np.float32), part.astype(np.int32), tris.astype(np.int32),
                                                             label.astype(np.uint16), tforms.astype(np.float32))]
    tb = rdf.to_device(np.ascontiguousarray(table, np.float32)) if table is not None else None
    if keys is None:
        keys = rdf.DeviceArray((int(lib.rdf_hand_scene_workspace_bytes(N, W, H)),), np.uint8).fill(0xFF)
    depth, labels = rdf.DeviceArray((N, H, W), np.uint16), rdf.DeviceArray((N, H, W), np.uint16)
    out = []
    for _ in range(runs):
        depth.fill(7)
        labels.fill(7)
        rc = lib.rdf_hand_scene_render(N, W, H, len(verts), dev[0].ptr, dev[1].ptr, len(tris), dev[2].ptr, dev[3].ptr, P, dev[4].ptr,
                                       tb.ptr if tb is not None else None, *(float(v) for v in cam), float(zmin), float(zmax), empty, seed, holes,
                                       noise, keys.ptr, depth.ptr, labels.ptr, rt.stream())
        _lib.check(lib, rc, "rdf_hand_scene_render")
        out.append((depth.get(), labels.get()))
    return out, keys.get()


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [1, hc.MAX_FRAMES])
@pytest.mark.parametrize("W,H", hc.SIZES)
def test_hand_built_scenes_match_the_restatement_bit_for_bit(W, H, n_frames, rdf, gpu_runtime):
    c = hc.case(W, H)
    for name, with_table, empty, holes, noise in hc.VARIANTS:
        want_depth, want_labels, _ = c["want"][n_frames, name]
        runs, keys = _render_raw(rdf, W, H, c["mesh"], c["tforms"][:n_frames], c["tables"][:n_frames] if with_table else None,
                                 c["cam"], empty, hc.SEED, holes, noise, runs=2)
        bad = int((runs[0][0] != want_depth).sum()), int((runs[0][1] != want_labels).sum())
        print(f"{W}x{H} x {n_frames} {name}: {int((want_labels > 0).sum())} mesh pixels, {bad[0]} depths and {bad[1]} labels differ")
        assert np.array_equal(runs[0][0], want_depth) and np.array_equal(runs[0][1], want_labels), name
        # the workspace is left empty: the second call on it gives the same images
        assert np.array_equal(runs[1][0], runs[0][0]) and np.array_equal(runs[1][1], runs[0][1]), name
        assert (keys == 0xFF).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid: " + n for n in rc.GRID_CASES] + list(hc.OWN_CASES))
def test_one_rule_cases_match_the_restatement_bit_for_bit(name, rdf, gpu_runtime):
    c = hc.grid_case(name[6:]) if name.startswith("grid: ") else hc.OWN_CASES[name]
    want_depth, want_labels = hc.want_of(name)
    runs, keys = _render_raw(rdf, c["W"], c["H"], c["mesh"], c["tforms"], c["tables"], c["cam"], c["empty"], c["seed"], c["holes"],
                             c["noise"], zmin=c["zmin"], zmax=c["zmax"])
    depth, labels = runs[0]
    print(f"{name}: {int((want_labels > 0).sum())} mesh pixels, {int((depth != want_depth).sum())} depths and "
          f"{int((labels != want_labels).sum())} labels differ")
    if c.get("depth") is not None:                      # the images worked by hand
        assert np.array_equal(depth[0], c["depth"]), name
    if name == "quad coplanar with the table":
        inside = np.zeros((16, 16), bool)
        inside[hc.QUAD_PIXELS] = True
        assert (depth == 512).all() and np.array_equal(labels[0] > 0, inside)
    if name == "noise against both clamps":
        assert (depth[0] == 1).any() and (depth[1] == 65534).any()
    assert np.array_equal(depth, want_depth) and np.array_equal(labels, want_labels), name
    assert (keys == 0xFF).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name,with_table,empty", hc.MANY_VARIANTS)
def test_more_frames_than_the_grid_has_rows_match_the_restatement_bit_for_bit(name, with_table, empty, rdf, gpu_runtime):
    c = hc.many_frames_case()
    W, H = hc.MANY_SIZE
    N = hc.MANY_N
    want_depth, want_labels, _ = c["want"][name]
    want_depth, want_labels = np.take(want_depth, c["index"], axis=0), np.take(want_labels, c["index"], axis=0)
    tforms = np.take(c["tforms"], c["index"], axis=0)
    tables = np.take(c["tables"], c["index"], axis=0) if with_table else None
    runs, keys = _render_raw(rdf, W, H, c["mesh"], tforms, tables, c["cam"], empty, hc.SEED, 0, 0)
    depth, labels = runs[0]
    wrong = np.nonzero(((depth != want_depth) | (labels != want_labels)).reshape(N, -1).any(1))[0]
    print(f"{name}: {len(wrong)} of {N} frames differ" + (f", the first {wrong[:8].tolist()}" if len(wrong) else ""))
    assert depth.shape == (N, H, W) and np.array_equal(depth, want_depth) and np.array_equal(labels, want_labels)
    assert keys.size == N * W * H * 8 and (keys == 0xFF).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_parts", [16, 32])
def test_the_real_hand_matches_the_restatement_bit_for_bit(n_parts, rdf, gpu_runtime):
    W, H = 106, 60
    s = _hand_scene(n_parts, 5, seed=11)
    r = rdf.HandSceneRenderer((H, W), s["cam"], max_frames=8)
    geometry = hs.rasterise(W, H, *s["mesh"], s["tforms"], *s["cam"])
    for labels, table, empty, rate, noise in (("fine", None, 65535, 0., 0), ("coarse", s["table"], 0, 0.1, 12)):
        tri_label = r.tri_labels(n_parts, labels)
        assert np.array_equal(tri_label, rdf.HandModel.label_table(labels)[s["tri_part"]])
        want_depth, want_labels, _ = hs.render(W, H, *s["mesh"], tri_label, s["tforms"], None if table is None else np.tile(table, (5, 1)),
                                               *s["cam"], empty_depth=empty, seed=99, hole_threshold=int(rate * 2 ** 32),
                                               noise_amp=noise, geometry=geometry)
        for _ in range(2):
            depth, lab = r.render(s["tforms"], labels, table, empty, 99, rate, noise)
            got_depth, got_labels = depth.get(), lab.get()
            print(f"{n_parts} parts, {labels}: {int((want_labels > 0).sum())} mesh pixels, {int((got_depth != want_depth).sum())} depths "
                  f"and {int((got_labels != want_labels).sum())} labels differ")
            assert np.array_equal(got_depth, want_depth) and np.array_equal(got_labels, want_labels)
        assert (want_labels > 0).sum() > 5 * 150 * n_parts // 16 and (r._keys.get() == 0xFF).all()


@pytest.mark.gpu
def test_chunks_of_max_frames_give_the_images_of_one_call(rdf, gpu_runtime):
    W, H = 106, 60
    s = _hand_scene(32, 5, seed=12)
    whole = rdf.HandSceneRenderer((H, W), s["cam"], max_frames=8)
    chunked = rdf.HandSceneRenderer((H, W), s["cam"], max_frames=2)
    tables = np.tile(s["table"], (5, 1)) * np.linspace(1., 1.05, 5, dtype=np.float32)[:, None]
    args = (s["tforms"], "fine", tables, 0, 4242, 0.2, 9)
    a, b = whole.render(*args), chunked.render(*args)
    assert np.array_equal(a[0].get(), b[0].get()) and np.array_equal(a[1].get(), b[1].get())
    depth = a[0].get()
    assert all(not np.array_equal(depth[k] == 0, depth[k + 1] == 0) for k in range(4))      # each frame has its own holes
    # caller's buffers are used, and written whole
    d, l = rdf.DeviceArray((5, H, W), np.uint16).fill(3), rdf.DeviceArray((5, H, W), np.uint16).fill(3)
    got = chunked.render(*args, depth_out=d, labels_out=l)
    assert got[0] is d and got[1] is l and np.array_equal(d.get(), depth) and np.array_equal(l.get(), a[1].get())


@pytest.mark.gpu
def test_a_forest_trained_on_a_generated_dataset_beats_always_saying_the_commonest_class(rdf, gpu_runtime, tmp_path):
    """make_dataset -> train_forest -> pct. matching pixels against the share of the most frequent class among the
    labelled test pixels: the data is learnable.  No further margin."""
    ds_mod = importlib.import_module("3d-beats_amd.dataset")
    W, H, n_train, n_test, tree_seed = 212, 120, 40, 16, 5
    r = rdf.HandSceneRenderer((H, W), (150., 105.5, 59.5))
    depth, labels = r.make_dataset(str(tmp_path / "hands"), n_train + n_test, seed=31)
    assert depth.shape == labels.shape == (n_train + n_test, H, W) and ((labels == 0) == (depth == 65535)).all()
    assert all(set(np.unique(l).tolist()) >= {0, 1, 2} for l in labels) and set(np.unique(labels).tolist()) == set(range(8))
    cfg = ds_mod.DecisionTreeDatasetConfig(str(tmp_path / "hands"))
    assert cfg.img_dims == (W, H) and cfg.num_classes() == 8 and cfg.total_available_images == n_train + n_test
    forest, pct = ds_mod.train_forest(str(tmp_path / "hands"), n_train, n_test, 128, 64, 1, 10, str(tmp_path / "forest.npy"),
                                      log=lambda *_: None, tree_seed=tree_seed)
    # the test images train_forest drew: the same seed, the same two shuffles
    np.random.seed(tree_seed)
    _, test = ds_mod.DecisionTreeDatasetConfig.multiple(str(tmp_path / "hands"), [(n_train, None, 'train'), (n_test, None, 'test')])
    truth = labels[test.img_idxes]
    counts = np.bincount(truth[truth > 0].astype(np.int64), minlength=8)
    baseline = counts.max() / counts.sum()
    print(f"pct. matching pixels {pct:.4f}; the commonest class ({int(counts.argmax())}) is {baseline:.4f} of the labelled test pixels")
    assert pct > baseline
    np.random.seed(tree_seed + 1)
    score = ds_mod.score_saved_model(str(tmp_path / "forest.npy"), str(tmp_path / "hands"), n_test)
    assert 0. < score.pct_matching <= 1.


@pytest.mark.gpu
def test_camera_sequence_shows_a_finger_come_down_on_the_table(rdf, gpu_runtime):
    hm, scene = _hm(), importlib.import_module("3d-beats_amd.hand_scene")
    W, H, n = 106, 60, 9
    plane = scene.look_down_plane(5500.)
    r = rdf.HandSceneRenderer((H, W), (W * 0.7, (W - 1) / 2., (H - 1) / 2.), max_frames=4)
    poses = r.model.press_sequence(n, "index", wrist=(0., -900., 800.), speed_mm=10.)
    truth = rdf.DeviceArray((n, H, W), np.uint16)
    frames = r.camera_sequence(poses, plane, labels_out=truth)
    depth, lab = frames.get(), truth.get()
    assert depth.shape == (n, H, W) and (depth > 0).all()                   # the table fills the view, no holes asked for
    assert ((lab == 0) == (depth == 5500)).all()                            # the table, seen from straight above
    tip = [depth[k][lab[k] == 4].max() for k in range(n)]                   # the index fingertip's deepest pixel: nearest the table
    assert tip[n // 2] > tip[0] + 100 and tip[n // 2] == max(tip) and tip[-1] == tip[0] and tip[n // 2] <= 5500
    want, _, _ = hs.render(W, H, r.model.verts, r.model.vert_part, r.model.tris, r.tri_labels(16, "fine"), r.transforms(poses, plane),
                           np.tile(scene.table_of_plane(plane), (n, 1)), r.f, r.ppx, r.ppy, empty_depth=0)
    assert np.array_equal(depth, want)
    holes = r.camera_sequence(poses, plane, hole_rate=0.05, seed=3).get()
    assert 0.02 < (holes == 0).mean() < 0.08


# ------------------------------------------------------------------ two rasterisers, one rule set --------------------------------
_same = {}


def _same_triangles():
    """One grid of points as the re-render's frame and as the hand scene's mesh, and the two restatements' images.  67 x 6
    points: the quads cross the re-render's 64-quad tile edge in x and its 4-quad edge in y.  Two points without w and one
    behind the camera; an affine transform with a small rotation about y and a shift."""
    if not _same:
        import rerender_numpy as rn
        W, H = 67, 6
        f, ppx, ppy = 50., (W - 1) / 2., (H - 1) / 2.
        rng = np.random.default_rng(67 * 6)
        j, i = np.mgrid[:H, :W]
        pts = np.empty((H, W, 4), np.float32)
        pts[..., 0] = (i - ppx) * 60. + rng.uniform(-25., 25., (H, W))          # 60 units are one pixel at z = 3000
        pts[..., 1] = (j - ppy) * 60. + rng.uniform(-25., 25., (H, W))
        pts[..., 2] = 3000. + rng.uniform(-40., 40., (H, W))
        pts[..., 3] = 1.
        pts[2, 20, 3] = pts[4, 65, 3] = 0.
        pts[1, 40, 2] = -3000.
        a = np.deg2rad(4.)
        M = np.array([[np.cos(a), 0., np.sin(a), 45.], [0., 1., 0., -20.], [-np.sin(a), 0., np.cos(a), 120.], [0., 0., 0., 1.]],
                     np.float32)
        color = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        # rule 1's triangles in rule 1's order, so that an index into tris is the re-render's triangle id
        at = (j[:-1, :-1] * W + i[:-1, :-1]).reshape(-1)
        tris = np.stack([np.stack([at, at + 1, at + W], 1), np.stack([at + 1, at + W, at + W + 1], 1)], 1)
        has = pts[..., 3] > 0
        quad = (has[:-1, :-1] & has[:-1, 1:] & has[1:, :-1] & has[1:, 1:]).reshape(-1)
        tris[~quad] = 0                                                         # (0, 0, 0): no area, dropped
        tris = tris.reshape(-1, 3)
        mesh = (pts[..., :3].reshape(-1, 3).copy(), np.zeros(W * H, np.int32), tris.astype(np.int32),
                np.ones(len(tris), np.uint16))
        tforms = M[:3].reshape(1, 1, 12).copy()
        cam = (f, ppx, ppy)
        want_rr = rn.rerender(pts, color, M, *cam)
        want_hs = hs.render(W, H, *mesh, tforms, None, *cam, empty_depth=0)
        _same.update(W=W, H=H, pts=pts, color=color, M=M, mesh=mesh, tforms=tforms, cam=cam, want_rr=want_rr, want_hs=want_hs)
    return _same


def test_the_two_restatements_draw_the_same_triangles_alike():
    c = _same_triangles()
    depth_rr, depth_hs, labels_hs = c["want_rr"][0], c["want_hs"][0][0], c["want_hs"][1][0]
    assert len(c["mesh"][2]) == 2 * (c["W"] - 1) * (c["H"] - 1) and (c["mesh"][2] == 0).all(1).sum() == 2 * 8     # four quads a point
    drawn = int((depth_rr > 0).sum())
    print(f"{drawn} of {depth_rr.size} pixels drawn")
    assert 2 * drawn >= depth_rr.size and drawn < depth_rr.size
    assert np.array_equal(depth_rr, depth_hs)
    assert np.array_equal(labels_hs > 0, depth_rr > 0)


@pytest.mark.gpu
def test_rerender_and_hand_scene_draw_the_same_triangles_alike(rdf, gpu_runtime):
    c = _same_triangles()
    W, H = c["W"], c["H"]
    rr = rdf.SceneRerender((H, W), c["cam"])
    depth, out = rdf.DeviceArray((H, W), np.uint16).fill(7), rdf.DeviceArray((H, W, 3), np.uint8).fill(7)
    rr.run(rdf.to_device(c["pts"]), rdf.to_device(c["color"]), c["M"], depth, out)
    depth_rr = depth.get()
    runs, _ = _render_raw(rdf, W, H, c["mesh"], c["tforms"], None, c["cam"], 0, 0, 0, 0)
    depth_hs, labels_hs = runs[0][0][0], runs[0][1][0]
    drawn = int((depth_rr > 0).sum())
    print(f"{drawn} of {depth_rr.size} pixels drawn; {int((depth_rr != depth_hs).sum())} depths differ between the entry points, "
          f"{int((depth_rr != c['want_rr'][0]).sum())} from the restatement")
    assert 2 * drawn >= depth_rr.size
    assert np.array_equal(depth_rr, depth_hs)
    assert np.array_equal(depth_rr, c["want_rr"][0]) and np.array_equal(depth_hs, c["want_hs"][0][0])
    assert np.array_equal(out.get(), c["want_rr"][1])
    assert np.array_equal(labels_hs > 0, depth_rr > 0)
