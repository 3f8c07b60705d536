"""Joint votes (rdf_labels_votes_count / _fit / _cast of librdf_labels.so, joint_votes.VoteFitter, VoteTable and JointVoter,
HandSceneRenderer.fingertip_targets) against the restatement in tests/votes_numpy.py.  The CPU tests pin the restatement to a
case worked by hand and every rounding rule to literals, check fingertip_targets against a direct projection and the C entry
points' argument checks, which launch nothing; every GPU comparison is byte for byte."""
import ctypes
import importlib

import numpy as np
import pytest

import mutants
import refit_numpy as rn
import votes_cases as vc
import votes_numpy as vn
import walk_cases as wc


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_hand_worked_case():
    """Depth 64, so ox = floordiv(dx * 64, 64) = dx.  The joint is at (4, 2, 70), radius 3.
      (1, 1) left:  dx 3, dy 1 -> (3, 1, 6), squares 10     (2, 1) left:  dx 2, dy 1 -> (2, 1, 6), squares 5
      (0, 3) left:  dx 4 > radius: walked, nothing summed    (6, 2) right: dx -2, dy 0 -> (-2, 0, 6), squares 4
      (7, 0): depth 0, totals[1]
    left slot: 2, 5, 2, 12, 15 -> mx = floordiv(5, 2) = 2, my = 1, mz = 6, var = max(0, floordiv(15, 2) - (4 + 1)) = 2,
    w = 256 - floordiv(2 * 256, 3 + 1) = 128.    right slot: 1, -2, 0, 6, 4 -> (-2, 0, 6), var = 4 - 4 = 0, w = 256.
    Cast with the labels as gate, cells of 2 pixels: at depth 64 a vote moves by (mx, my) pixels.  (1, 1) -> (3, 2): cell (1, 1)
    += 128.  (2, 1) -> (4, 2): cell (2, 1) += 128.  (0, 3) -> (2, 4): below the frame, dropped.  (6, 2) -> (4, 2): cell (2, 1) +=
    256.  vz = 64 + 6 = 70 for all.  box 0: best 384 at cell (2, 1): X = 16 * 4 + 16 = 80, Y = 16 * 2 + 16 = 48, Z = 70.
    box 1: 512 for cells (1, 0), (2, 0), (1, 1), (2, 1); (1, 0) is first: X = (128 * 48 + 384 * 80) / 512 = 72."""
    depth, labels, targets, forest = vc.hand_case()
    h = vc.HAND
    assert rn.dims(forest) == (1, 1, 1) and rn.is_leaf_slot(forest[0, 0], 0) and rn.is_leaf_slot(forest[0, 0], 1)
    sums, totals = vn.count(depth, labels, targets, forest, radius=h["radius"])
    assert sums.dtype == np.uint64 and sums.shape == (1, 1, 2, 1, 5)
    assert sums[0, 0, 0, 0].tolist() == [2, 5, 2, 12, 15]
    assert sums[0, 0, 1, 0].tolist() == [1, 2 ** 64 - 2, 0, 6, 4]
    assert totals.tolist() == [4, 1, 0, 3]
    again, t2 = vn.count(depth, labels, targets, forest, radius=h["radius"], sums=sums.copy(), totals=totals.copy())       # the call adds
    assert again[0, 0, 0, 0].tolist() == [4, 10, 4, 24, 30] and again[0, 0, 1, 0].tolist() == [2, 2 ** 64 - 4, 0, 12, 8]
    assert t2.tolist() == [8, 2, 0, 6]
    votes, report = vn.fit(forest, sums, h["min_count"], h["max_var"])
    assert votes.dtype == np.int32 and votes[0, 0, :, 0].tolist() == [[2, 1, 6, 128], [-2, 0, 6, 256]]
    assert report.tolist() == [2, 2, 0, 0]
    v2, r2 = vn.fit(forest, sums, 2, 1)                     # the right slot has one pixel, the left one's variance is 2
    assert not v2.any() and r2.tolist() == [2, 0, 1, 1]
    acc, zacc = vn.cast(depth, forest, votes, gate=labels, shift=h["shift"])
    assert acc.shape == (1, 1, 2, 4) and acc[0, 0].tolist() == [[0, 0, 0, 0], [0, 128, 384, 0]]
    assert zacc[0, 0].tolist() == [[0, 0, 0, 0], [0, 128 * 70, 384 * 70, 0]]
    assert vn.modes(acc, zacc, h["shift"], 0, 1).tolist() == [[[80, 48, 70, 384]]]
    assert vn.modes(acc, zacc, h["shift"], 1, 1).tolist() == [[[72, 48, 70, 512]]]
    assert vn.modes(acc, zacc, h["shift"], 1, 513).tolist() == [[[-1, -1, 0, 0]]]
    # a "go on" flag at the last level: the pixels of the left side fall off
    off = forest.copy()
    off[0, 0, 5] = -1.
    s3, t3 = vn.count(depth, labels, targets, off, radius=h["radius"])
    assert not s3[0, 0, 0].any() and s3[0, 0, 1, 0].tolist() == [1, 2 ** 64 - 2, 0, 6, 4] and t3.tolist() == [4, 1, 3, 1]
    v3, r3 = vn.fit(off, s3, 1, 3)
    assert r3.tolist() == [1, 1, 0, 0] and not v3[0, 0, 0].any()


def test_every_rounding_rule_on_literals():
    # V1: floordiv towards minus infinity
    assert vn.offset(-1, 1) == -1 and vn.offset(1, 1) == 0 and vn.offset(-1, 64) == -1 and vn.offset(-2, 33) == -2
    assert vn.offset(-255, 65534) == -261113 and vn.offset(255, 65534) == 261112 and abs(vn.offset(-255, 65534)) < 1 << 18
    # V4: floordiv(128 m + d, 2 d) is round-half-up of 64 m / d.  d = 1: 128 m + 1 is just above a multiple of 2
    assert vn.vote_pixels(0, 1) == 0 and vn.vote_pixels(1, 1) == 64 and vn.vote_pixels(-1, 1) == -64
    # d = 65534, 2 d = 131068: 128 m + d is 131006 at m = 511 (just below 2 d: 0) and 131134 at m = 512 (just above: 1); the
    # multiple itself is met at d = 64: 128 m + 64 = 128 at m = 0.5 -- no such m; at d = 128, m = 1: 256 = 2 d exactly -> 1
    assert vn.vote_pixels(511, 65534) == 0 and vn.vote_pixels(512, 65534) == 1
    assert vn.vote_pixels(1, 128) == 1 and vn.vote_pixels(0, 128) == 0 and vn.vote_pixels(-1, 128) == 0 and vn.vote_pixels(-2, 128) == -1
    assert vn.vote_pixels(-3, 128) == -1                    # -1.5 rounds half up to -1
    assert vn.vote_pixels(-512, 65534) == -1 and vn.vote_pixels(-511, 65534) == 0 and vn.vote_pixels(-513, 65534) == -1
    # V4 inverts V1 wherever 64 / d < 1 / 2
    for d in (129, 1000, 65534):
        for dx in (-255, -1, 0, 1, 255):
            assert vn.vote_pixels(vn.offset(dx, d), d) == dx
    # V2: the mean is a floor, the variance is clamped at 0, the weight runs from 256 to 1
    word = lambda *v: np.array([x & vn.M64 for x in v], np.uint64)      # noqa: E731
    assert vn.fit_entry(word(2, -7, 7, -1, 100), 1, 1000) == ((-4, 3, -1, 256 - (25 * 256) // 1001), 1)
    assert vn.fit_entry(word(8, 24, 0, 0, 1), 1, 0) == ((3, 0, 0, 256), 1)                 # floordiv(1, 8) - 9 < 0: var 0
    assert vn.weight(0, 1000) == 256 and vn.weight(1000, 1000) == 1 and vn.weight(0, 0) == 256 and vn.weight(1 << 38, 1 << 38) == 1
    assert vn.weight(1001, 1000) == 0                       # why var = max_var + 1 must be dropped before the weight
    assert vn.fit_entry(word(4, 0, 0, 0, 4 * 1000 + 3), 1, 1000) == ((0, 0, 0, 1), 1)      # var = max_var
    assert vn.fit_entry(word(4, 0, 0, 0, 4 * 1001), 1, 1000) == ((0, 0, 0, 0), 3)          # var = max_var + 1
    assert vn.fit_entry(word(4, 0, 0, 0, 0), 5, 1000) == ((0, 0, 0, 0), 2)
    assert vn.fit_entry(word(1 << 26, 0, 0, 0, 0), 1, 1000) == ((0, 0, 0, 0), 2)
    assert vn.fit_entry(word((1 << 26) - 1, 0, 0, 0, 0), 1, 1000) == ((0, 0, 0, 256), 1)
    # V5: X, Y and Z are floors; a cell's centre is at 8 * 2^a sixteenths
    acc = np.array([[1, 2]], np.uint32)
    zacc = np.array([[10, 21]], np.uint64)
    assert vn.mode(acc, zacc, 0, 1, 1) == ((1 * 8 + 2 * 24) // 3, 8, 31 // 3, 3) == (18, 8, 10, 3)
    assert vn.mode(acc, zacc, 4, 0, 1) == (16 * 16 + 128, 128, 10, 2)
    assert vn.mode(np.zeros((3, 3), np.uint32), np.zeros((3, 3), np.uint64), 0, 4, 0) == (-1, -1, 0, 0)     # max(min_support, 1)
    # absent joints
    assert [vn.absent(z) for z in (-1, 0, 1, 65534, 65535, 70000)] == [True, True, False, False, True, True]


def test_the_cases_contain_what_they_are_meant_to():
    depth, labels = wc.adversarial_frames()
    px = set(vc.hand_pixels(depth, labels))
    assert any(int(labels[p]) >= wc.ADV["C"] for p in px)                       # a label the forest does not have is "hand" too
    for radius in (0, 255):
        t = vc.targets_for(16, radius)
        assert (0, int(t[0, 0, 1]), int(t[0, 0, 0]) - radius) in px and (0, int(t[0, 0, 1]), int(t[0, 0, 0]) - radius - 1) in px
        assert (1, int(t[1, 0, 1]) - radius, int(t[1, 0, 0])) in px
        assert (0, int(t[0, 4, 1]) - radius - 1, int(t[0, 4, 0])) in px
        assert [vn.absent(int(z)) for z in (t[0, 1, 2], t[1, 1, 2], t[1, 2, 2])] == [True] * 3
        assert t[0, 2, 0] < 0 and t[1, 3, 0] >= wc.ADV["W"] and t[1, 3, 1] < 0
    forest, sums, slots = vc.fit_case()
    votes, report = vn.fit(forest, sums, vc.FIT["min_count"], vc.FIT["max_var"])
    got = {k: votes[a[0], a[1], a[2], a[3]].tolist() for k, a in slots.items()}
    assert got == {"below_min_count": [0, 0, 0, 0], "at_min_count": [1, 1, 1, 254], "below_2_26": [3, 0, -1, 256],
                   "at_2_26": [0, 0, 0, 0], "var_at_max": [0, 0, 0, 1], "var_above_max": [0, 0, 0, 0],
                   "negative_sums": [-2, -3, -6667, 256], "var_clamped": [3, 0, 0, 256],
                   "large_means": [262143, -262143, 65533, 252], "unreachable": [0, 0, 0, 0]}
    assert int(report[1]) == 6 and int(report[3]) == 1 and int(report[1] + report[2] + report[3]) == vc.FIT["J"] * int(report[0])
    d, f, v, g1, g2 = vc.border_case()
    assert vn.vote(d, f, v, gate=g1, shift=0, box=0).tolist() == [[
        [120, 24, 64, 7], [-1, -1, 0, 0], [-1, -1, 0, 0], [88, 8, 64, 9], [-1, -1, 0, 0], [88, 24, 1, 11], [88, 24, 65534, 13],
        [-1, -1, 0, 0], [88, 24, 70, 100], [-1, -1, 0, 0]]]
    assert vn.vote(d, f, v, gate=g2, shift=0, box=0)[0, 8].tolist() == [24, 24, 70, 100]       # (1, 1) before (6, 2)
    d, f, v = vc.wave_case()
    acc, zacc = vn.cast(d, f, v, shift=0)
    assert np.count_nonzero(acc[0, 0]) == 2 and acc[0, 0, :, 32].tolist() == [2080, 2080] and (acc[0, 1] > 0).all()


def test_fingertip_targets_against_a_direct_projection(rdf):
    scene = _mod("hand_scene")
    H, W, f, ppx, ppy = 60, 106, 75., 52.5, 29.5
    r = scene.HandSceneRenderer.__new__(scene.HandSceneRenderer)               # fingertip_targets needs no device
    r.f, r.ppx, r.ppy, r.z_near, r.z_far = f, ppx, ppy, 50., 50000.
    r.model = rdf.HandModel()
    r.left_model = r.model.mirrored()
    plane = scene.look_down_plane(5500.)
    poses = r.model.sample_poses(3, np.random.default_rng(3))
    poses[1, 2] = 5900.                                     # the wrist 40 mm behind the camera: a tip nearer than z_near
    poses[2, 0] = 9000.                                     # 0.9 m to the side: outside the frame
    left = r.left_model.sample_poses(3, np.random.default_rng(4))
    got = r.fingertip_targets(poses, plane, left)
    assert got.dtype == np.int32 and got.shape == (3, 10, 3) and r.fingertip_targets(poses, plane).shape == (3, 5, 3)
    cam_from_plane = np.linalg.inv(plane)
    want = np.zeros((3, 10, 3), np.int64)
    for n in range(3):
        for j in range(10):
            model, pose = (r.model, poses[n]) if j < 5 else (r.left_model, left[n])
            X, Y, Z = model.fingertips(pose[None], cam_from_plane)[0, j % 5]
            if 50. <= Z <= 50000. and 1 <= round(Z) <= 65534:
                want[n, j] = (np.floor(f * X / Z + ppx), np.floor(f * Y / Z + ppy), round(Z))
    assert np.array_equal(got, want)
    assert (got[0, :, 2] > 0).all() and (got[0, :5, 0] >= 0).all() and (got[0, :5, 0] < W).all()        # seen, inside
    gone = got[1, :5, 2] == 0
    assert gone.any() and not got[1, :5][gone].any() and (got[1, 5:, 2] > 0).all()                       # absent: all three words 0
    assert (got[2, :5, 2] > 0).all() and (got[2, :5, 0] >= W).all()                                      # outside the frame, kept


def test_rejected_arguments_launch_nothing(rdf):
    """Rejected arguments launch nothing, so they need no device; the pointers given here are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    P = ctypes.c_void_p
    d, l, tg, f, s, t, v, w, o, g = (P(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0xa0000))
    BAD, NULL, LARGE = -1, -2, -3
    count, fit, ws, cast = lib.rdf_labels_votes_count, lib.rdf_labels_votes_fit, lib.rdf_labels_votes_workspace_bytes, lib.rdf_labels_votes_cast
    shapes = ((0, 4, 3), (2, 0, 3), (2, 31, 3), (2, 4, 0), (2, 4, 65536), (-1, 4, 3))

    # V1
    def c(depth=d, labels=l, targets=tg, dims=(1, 8, 8), forest=f, shape=(2, 4, 3), J=5, radius=255, sums=s, totals=t):
        return count(depth, labels, targets, *dims, forest, *shape, 1., J, radius, sums, totals, None)
    for dims in ((-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        assert c(dims=dims) == BAD
    for shape in shapes:
        assert c(shape=shape) == BAD
    for J in (0, -1, 17):
        assert c(J=J) == BAD
    for radius in (-1, 256):
        assert c(radius=radius) == BAD
    for name in ("depth", "labels", "targets", "forest", "sums", "totals"):
        assert c(**{name: None}) == NULL
    assert c(depth=P(0x10001)) == BAD and c(labels=P(0x20001)) == BAD and c(targets=P(0x30002)) == BAD
    assert c(forest=P(0x40002)) == BAD and c(sums=P(0x50004)) == BAD and c(totals=P(0x60004)) == BAD
    assert c(dims=(1, 65536, 32768)) == LARGE and c(dims=(32768, 256, 256)) == LARGE
    assert c(shape=(1, 30, 8), J=1) == LARGE                # (2^30 - 1) * 2 * 1 * 5 words in one tree
    assert c(shape=(1, 25, 8), J=16) == LARGE and c(shape=(1, 25, 8), J=1, depth=None) == NULL      # 160 * 2^25 words, and 10 * 2^25
    assert count(None, None, None, 0, 8, 8, None, 2, 4, 3, 1., 5, 255, None, None, None) == 0     # zero pixels: a no-op
    assert c(dims=(1, 0, 8), depth=None) == 0 and c(dims=(1, 8, 0), sums=None) == 0

    # V2
    def ft(forest=f, shape=(2, 4, 3), J=5, sums=s, min_count=8, max_var=1 << 20, votes=v, report=t):
        return fit(forest, *shape, J, sums, min_count, max_var, votes, report, None)
    for shape in shapes:
        assert ft(shape=shape) == BAD
    for J in (0, 17):
        assert ft(J=J) == BAD
    assert ft(min_count=0) == BAD and ft(max_var=(1 << 38) + 1) == BAD
    for name in ("forest", "sums", "votes", "report"):
        assert ft(**{name: None}) == NULL
    assert ft(forest=P(0x40002)) == BAD and ft(sums=P(0x50004)) == BAD and ft(votes=P(0x70008)) == BAD and ft(report=P(0x60004)) == BAD
    assert ft(shape=(1, 30, 8), J=1) == LARGE

    # V6: the workspace
    assert ws(2, 70, 13, 5, 2) == 2 * 5 * 4 * 18 * 12 and ws(1, 70, 13, 1, 0) == 70 * 13 * 12 and ws(3, 70, 13, 16, 4) == 3 * 16 * 5 * 8 + 3 * 16 * 5 * 4
    assert ws(1, 3, 1, 1, 0) == 3 * 8 + 16                  # acc's 12 bytes rounded up to 8
    assert ws(64, 848, 480, 10, 2) == 64 * 10 * 120 * 212 * 12
    for bad in ((-1, 8, 8, 5, 2), (1, -8, 8, 5, 2), (1, 8, -8, 5, 2), (1, 65536, 8, 5, 2), (1, 8, 65536, 5, 2), (1, 8, 8, 0, 2),
                (1, 8, 8, 17, 2), (1, 8, 8, 5, -1), (1, 8, 8, 5, 5)):
        assert ws(*bad) == 0

    # V3 to V6: the cast
    def cs(depth=d, dims=(1, 8, 8), gate=g, r=1, forest=f, shape=(2, 4, 3), votes=v, J=5, shift=2, box=1, support=1, workspace=w, out=o):
        return cast(depth, *dims, gate, r, forest, *shape, 1., votes, J, shift, box, support, workspace, out, None)
    for dims in ((-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        assert cs(dims=dims) == BAD
    for shape in shapes:
        assert cs(shape=shape) == BAD
    assert cs(r=0) == BAD and cs(J=0) == BAD and cs(J=17) == BAD
    assert cs(shift=-1) == BAD and cs(shift=5) == BAD and cs(box=-1) == BAD and cs(box=5) == BAD
    assert cs(depth=P(0x10001)) == BAD and cs(gate=P(0xa0001)) == BAD and cs(forest=P(0x40002)) == BAD
    assert cs(votes=P(0x70008)) == BAD and cs(workspace=P(0x80004)) == BAD and cs(out=P(0x90008)) == BAD
    assert cs(dims=(1, 65536, 1)) == LARGE and cs(dims=(1, 1, 65536)) == LARGE and cs(dims=(32768, 256, 256)) == LARGE
    assert cs(dims=(1, 4096, 4096)) == LARGE                # 2^24 label pixels * 2 trees * 256 >= 2^32
    assert cs(dims=(1, 4096, 4096), shape=(1, 4, 3), r=2, depth=None) == NULL                      # 2^22 * 1 * 256 < 2^32: not too large
    assert cs(dims=(1, 4096, 4096), shape=(1, 4, 3)) == LARGE and cs(dims=(1, 4096, 4095), shape=(1, 4, 3), depth=None) == NULL
    assert cs(dims=(1 << 27, 0, 0), J=16) == LARGE          # n_img * J >= 2^31
    for name in ("depth", "forest", "votes", "workspace", "out"):
        assert cs(**{name: None}) == NULL
    assert cast(None, 0, 8, 8, None, 1, None, 2, 4, 3, 1., None, 5, 2, 1, 1, None, None, None) == 0        # zero frames: a no-op


# ------------------------------------------------------------------ CPU: the newer cases -------------------------------------
def test_the_tie_layouts_are_worked_by_hand():
    """Every layout's joint as TIE_LAYOUTS states it, and the reading that each layout is there to tell from the rule."""
    m = vc.TIES
    assert (m["H"] * m["W"], vn.grid(m["H"], 0) * vn.grid(m["W"], 0)) == (800, 800) and 800 > 2 * 256     # a thread meets three cells and more
    assert vc._yx(4, 6, 100, 300, 44, 556) == ((0, 4), (0, 6), (2, 20), (7, 20), (1, 4), (13, 36))
    assert (300 - 256, 556 - 512) == (44, 44) and 100 > 300 - 256                 # cell 300 and cell 556 are thread 44's
    for name, (shift, box, pixels, want) in vc.TIE_LAYOUTS.items():
        depth, forest, votes, gate, shift, box = vc.tie_case(name)
        acc, zacc = vn.cast(depth, forest, votes, gate=gate, shift=shift)
        assert int(acc.sum()) == 100 * len(pixels) and int(zacc.sum()) == 7000 * len(pixels), name
        assert tuple(vn.modes(acc, zacc, shift, box, 1)[0, 0].tolist()) == want, name
        S = np.array([[int(acc[0, 0, max(cy - box, 0):cy + box + 1, max(cx - box, 0):cx + box + 1].sum()) for cx in range(acc.shape[3])]
                      for cy in range(acc.shape[2])])
        ties = np.argwhere(S == S.max())
        assert len(ties) >= 2 or "largest cell" in name, name                     # equal best sums
        if "largest cell" in name:
            cy, cx = np.unravel_index(np.argmax(acc[0, 0]), acc.shape[2:])
            wy, wx = ties[0]
            assert acc[0, 0].max() == 400 and S.max() == 900 and (abs(cy - wy) > box or abs(cx - wx) > box), name
    three = vc.TIE_LAYOUTS["three cells, the middle one leftmost"][2]
    assert sorted(three)[1] == (3, 2) == min(three, key=lambda p: (p[1], p[0]))   # the middle one in row-major order, the first in column-major
    # the two border layouts under the other order: the other tie wins, whose box another border clips
    d, f, v, g, shift, box = vc.tie_case("box 1: equal sums under the top and on the left border")
    assert vc.mutant("column-major ties").vote(d, f, v, gate=g, shift=shift, box=box)[0, 0].tolist() == [13, 168, 70, 300]       # (0, 10): columns 0..1
    d, f, v, g, shift, box = vc.tie_case("box 1: equal sums on the left and the right border")
    assert vc.mutant("last tie wins").vote(d, f, v, gate=g, shift=shift, box=box)[0, 0].tolist() == [(632 + 632 + 616) // 3, 184, 70, 300]   # (39, 11): columns 38..39
    acc, _ = vn.cast(d, f, v, gate=g, shift=shift)
    assert acc[0, 0].reshape(-1)[10 * 40 - 1] == 0 and acc[0, 0].reshape(-1)[11 * 40 - 1] == 100       # in memory, left of (0, 11) lies (39, 10): a vote


def test_the_new_cases_contain_what_they_are_meant_to():
    # a box sum above 2^31 - 1: the closed form against the restatement's cast at T = 2 on 48 x 48
    m = vc.SUM
    assert vc.SUM_BEST == 2149908480 and (1 << 31) - 1 < vc.SUM_BEST < 1 << 32 and m["H"] // 16 * (m["W"] // 16) == 81
    depth, forest, votes = vc.sum_case(2, 48, 48)
    acc, zacc = vn.cast(depth, forest, votes, shift=m["shift"])
    want = vc.full_grid(48, 48, 2, m["d"], m["mz"], m["shift"])
    assert mutants.same([acc, zacc], list(want)) and acc[0, 0, 1, 1] == 256 * 2 * 256
    acc, zacc = vc.full_grid(m["H"], m["W"], m["T"], m["d"], m["mz"], m["shift"])
    assert int(acc.sum(dtype=np.uint64)) == vc.SUM_BEST and int(acc[0, 0, 0, 0]) == 256 * 405 * 256 == 26542080
    got = [vn.modes(acc, zacc, m["shift"], box, support)[0, 0].tolist() for box, support in vc.SUM_RUNS]
    assert got == [[1152, 1152, 1007, 2147483647], [128, 128, 1007, 26542080], [1152, 1152, 1007, 2147483647], [-1, -1, 0, 0]]
    assert vn.M64 > 81 * 26542080 * (16 * 128 + 128) > 1 << 32                  # sx needs 64 bits
    # 128 m + d on both sides of +-2^31, column by column
    depth, forest, votes, gate = vc.wide_case()
    num = lambda j, i: 128 * vc.WIDE_JOINTS[j][0] + vc.WIDE_PIXELS[i][1]          # noqa: E731
    assert [num(0, 0), num(0, 1), num(1, 2), num(1, 3)] == [2 ** 31 - 1, 2 ** 31, -2 ** 31 + 1, -2 ** 31]
    moved = lambda j, i: vc.WIDE_PIXELS[i][0] + vn.vote_pixels(vc.WIDE_JOINTS[j][0], vc.WIDE_PIXELS[i][1])     # noqa: E731
    assert [moved(0, 0), moved(0, 1), moved(1, 2), moved(1, 3)] == [16431, 16447, 2591, 2607] and all(c % 16 == 15 for c in (16431, 16447, 2591, 2607))
    assert moved(2, 3) == 19024 + 24624 >= 20000 and 19024 + ((128 * 25165824 + 65408 - 2 ** 32) // (2 * 65408)) == 10816 < 20000
    got = vn.vote(depth, forest, votes, gate=gate, shift=vc.WIDE["shift"], box=0)
    none = [-1, -1, 0, 0]
    own = [[256 * (x >> 4) + 128, 128, d, 256] for x, d in vc.WIDE_PIXELS]       # joint 11: the pixel's own cell
    assert got[0].tolist() == [[256 * 1026 + 128, 128, 65407, 9]] + [none] * 10 + [own[0]]
    assert got[1].tolist() == [[256 * 1027 + 128, 128, 65408, 9]] + [none] * 10 + [own[1]]
    assert got[2].tolist() == [none, [256 * 161 + 128, 128, 65409, 9]] + [none] * 9 + [own[2]]
    assert got[3].tolist() == [none, [256 * 162 + 128, 128, 65408, 9]] + [none] * 9 + [own[3]]
    assert votes[0, 0, 0, 6:11, 3].tolist() == [257, -1, -256, 2 ** 31 - 1, -2 ** 31]
    # a fall-off in the second of three trees: three pixels fall off there and are summed in the first and the third
    depth, labels, targets, forest = vc.middle_case()
    sums, totals = vn.count(depth, labels, targets, forest, radius=vc.HAND["radius"])
    assert totals.tolist() == [4, 1, 3, 7] and sums[:, 0, :, 0, 0].tolist() == [[2, 1], [0, 1], [3, 0]]
    votes, report = vn.fit(forest, sums, **vc.MIDDLE_FIT)
    assert report.tolist() == [5, 4, 1, 0] and votes[2, 0, 0, 0].tolist() == [1, 0, 6, 181] and not votes[1, 0, 0].any()
    acc, _ = vn.cast(depth, forest, votes, gate=labels, shift=vc.HAND["shift"])
    assert int(acc.sum()) == 2 * 226 + 4 * 181 + 2 * 256        # all four through the third tree; (0, 3)'s vote of the first leaves the frame
    # min_support 0 on an accumulator without a vote
    depth, forest, votes, gate_one, _ = vc.border_case()
    got = vn.vote(depth, forest, votes, gate=gate_one, shift=0, box=0, min_support=0)
    assert got[0, 1].tolist() == none and got[0, 8].tolist() == [88, 24, 70, 100]


def test_the_sweep_cases_are_larger_than_one_sweep():
    """forest_votes_hip.hip, lines 32 to 34: kThreads = 256, kMaxBlocks = 1024, kMaxModeBlocks = 65536."""
    assert vc.SWEEP == 1024 * 256 == 262144 and vc.MODE_SWEEP == 65536
    # count
    depth, labels, targets, forest = vc.count_sweep_case()
    pix = depth.shape[1] * depth.shape[2]
    assert depth.shape == (2, 367, 401) and pix % 64 == 31 and depth.size == 294334 > vc.SWEEP and depth.size % 64 != 0
    flat = np.flatnonzero(labels)
    assert {0, vc.SWEEP - 1, vc.SWEEP, pix - 1, pix, depth.size - 1} <= set(flat.tolist()) and (pix - 1) // 64 == pix // 64
    assert (flat < vc.SWEEP).sum() >= 40 and (flat >= vc.SWEEP).sum() >= 40 and len(flat) < 100
    sums, totals = vn.count(depth, labels, targets, forest, radius=vc.COUNT_SWEEP["radius"])
    late = labels.copy()
    late.reshape(-1)[:vc.SWEEP] = 0
    late_sums, late_totals = vn.count(depth, late, targets, forest, radius=vc.COUNT_SWEEP["radius"])
    assert int(late_totals[3]) > 40 and int(totals[3]) > int(late_totals[3]) + 40 and int(totals[1]) > 0 and int(late_totals[1]) > 0
    assert (late_sums[0, 0, :, 0, 0] > 0).all() and (sums[0, 0, :, :, 0] > late_sums[0, 0, :, :, 0]).all()       # both slots, both joints, both sweeps
    assert int(sums[0, 0, :, 0, 0].sum()) == int(totals[0]) > int(sums[0, 0, :, 1, 0].sum()) > 0                    # joint 0 reaches every pixel
    # fit
    forest, sums, slots, leaf = vc.fit_sweep_case()
    T, N = forest.shape[:2]
    assert (T, N) == (5, 65535) and T * N == 327675 > vc.SWEEP and len(leaf) == 17 * T
    node = lambda slot: slot[0] * N + slot[1]                                     # noqa: E731
    assert sum(node(s) < vc.SWEEP for s in leaf) == 4 * 17 + 2 and sum(node(s) >= vc.SWEEP for s in leaf) == 15       # nodes 0 and 2 of tree 4 are before
    named = {k: node(v) for k, v in slots.items()}
    assert node(slots["unreachable"]) > vc.SWEEP and slots["unreachable"][:3] not in leaf and sums[slots["unreachable"]].all()
    assert all((named[k] >= vc.SWEEP) == k.endswith("tree 4") for k in named if k != "unreachable") and len(named) == 9 * T + 1
    votes, report = vn.fit(forest, sums, vc.FIT_SWEEP["min_count"], vc.FIT_SWEEP["max_var"])
    assert report.tolist() == [17 * T, 6 * T, 17 * T - 6 * T - T, T] and np.count_nonzero(votes.any(axis=-1)) == 6 * T
    for t in range(T):
        assert votes[slots[f"at_min_count in tree {t}"]].tolist() == [1, 1, 1, 254] and votes[slots[f"negative_sums in tree {t}"]].tolist() == [-2, -3, -6667, 256]
    # modes
    depth, forest, votes, kind = vc.modes_sweep_case()
    assert depth.shape == (4097, 2, 2) and depth.shape[0] * votes.shape[3] == 65552 > vc.MODE_SWEEP
    want = vc.vote_by_kind(vn)
    assert mutants.same(want[[0, 4096, 7]], vn.vote(depth[[0, 4096, 7]], forest, votes, shift=0, box=0))
    assert (want[0] != want[4096]).any(axis=1).all() and (want[0, :, 3] > 0).sum() >= 12 and (want[4096, :, 3] > 0).all()       # every joint of the pair differs
    assert len(set(kind.tolist())) == len(vc.MODE_KINDS) and (want[..., 3] == 0).any()


# ------------------------------------------------------------------ CPU: do the device cases bite? --------------------------
_true_outputs = {}


def _true(name):
    if name not in _true_outputs:
        _true_outputs[name] = vc.outputs(vn, name)
    return _true_outputs[name]


def test_the_unchanged_copy_is_the_restatement_bit_for_bit():
    copy = vc.mutant()
    assert copy is not vn and copy.cast is not vn.cast and not any(vc.reads_differently(copy, f) for f in ("count", "fit", "vote"))
    for name in vc.KILLS:
        assert mutants.same(vc.outputs(copy, name, rerun=True), _true(name)), name
    for m in vc.MUTANTS:                                    # every reading changes the code of some stage
        assert any(vc.reads_differently(vc.mutant(m), f) for f in ("count", "fit", "vote")), m


def test_a_mutant_that_no_longer_applies_fails_loudly():
    with pytest.raises(AssertionError, match="0 times"):
        mutants.load("votes_numpy", [("if S > best_:", "if S >= best:")])
    with pytest.raises(AssertionError, match="2 times"):
        mutants.load("votes_numpy", [("8 * (1 << shift)", "8")])


@pytest.mark.parametrize("name", list(vc.KILLS))
def test_each_mutant_changes_the_case_meant_for_it(name, capsys):
    """A wrong reading of a rule that leaves a case's outputs unchanged would pass the GPU test of that case.  KILLS is exact:
    a case that comes to notice more, or less, says so here."""
    killed = {m: mutants.changed(vc.outputs(vc.mutant(m), name), _true(name)) for m in vc.MUTANTS}
    with capsys.disabled():
        print(f"\n  {name}: outputs changed by " + ", ".join(f"{m}: {k}" for m, k in killed.items() if k), end="")
    assert {m for m, k in killed.items() if k} == set(vc.KILLS[name]), name
    assert len(set(vc.KILLS[name])) == len(vc.KILLS[name])


def test_every_mutant_is_met_by_some_case():
    met = set(m for ms in vc.KILLS.values() for m in ms)
    assert met | set(vc.EQUIVALENT) == set(vc.MUTANTS) and not met & set(vc.EQUIVALENT)
    assert all(len(why) > 40 for why in vc.EQUIVALENT.values()) and len(vc.MUTANTS) >= 42 and vc.ADV_FIT == ADV_FIT
    # set(KILLS) is the set of device cases: every GPU test of this file by name, every parametrisation but the scales
    gpu_tests = {k[5:] for k, v in globals().items() if k.startswith("test_") and any(mk.name == "gpu" for mk in getattr(v, "pytestmark", []))}
    assert {k.split("[")[0] for k in vc.KILLS} == gpu_tests and len(gpu_tests) >= 20
    assert {k for k in vc.KILLS if "[" in k} == ({f"adversarial_count_fit_cast[{J}-{r}]" for J, r in vc.ADV_PARAMS}
                                                 | {f"cast_cells_and_boxes[{s}-{b}]" for s, b in vc.CELLS_AND_BOXES}
                                                 | {f"mode_ties[{n}]" for n in vc.TIE_LAYOUTS})
    assert all(not vc.KILLS[k] and not vc.outputs(vn, k) for k in vc.DEVICE_ALONE) and set(vc.DEVICE_ALONE) <= set(vc.KILLS)
    # the readings that survived the cases of the first pull request, each with the new case that meets it
    for m, case in (("S in 32 bits", "box_sums_above_2_31"), ("support not clamped", "box_sums_above_2_31"),
                    ("128 m + d in 32 bits", "votes_that_need_64_bits_and_weights_that_are_none"),
                    ("w >= 1 votes", "votes_that_need_64_bits_and_weights_that_are_none"),
                    ("negative w votes", "votes_that_need_64_bits_and_weights_that_are_none"),
                    ("column-major ties", "mode_ties[three cells, the middle one leftmost]"), ("min_support 0 is 0", "min_support_0"),
                    ("a fall-off ends the pixel's sums", "a_fall_off_in_a_middle_tree"), ("gate 65535 passes", "cast_reduce_gates_and_support")):
        assert m in vc.KILLS[case], (m, case)


# ------------------------------------------------------------------ CPU: arguments the Python layer rejects -------------------
def test_a_vote_table_file_is_checked_on_load(rdf, tmp_path):
    """Every rejection comes before anything is put on a device."""
    T, D, C, J = 1, 2, 3, 2
    good = np.concatenate([np.array([T, D, C, J], np.int32), np.zeros(T * 3 * 2 * J * 4, np.int32)])
    cases = {"dtype": good.astype(np.int64), "short": good[:3], "size": good[:-1], "two tables": np.concatenate([good, good[4:]]),
             "two dimensions": good.reshape(2, -1), "J": np.concatenate([np.array([T, D, C, 17], np.int32), np.zeros(T * 3 * 2 * 17 * 4, np.int32)]),
             "D": np.array([1, 0, 3, 2], np.int32)}
    for w in (257, -1):
        bad = good.copy()
        bad[4 + 3 + 4 * 5] = w                              # the weight of the sixth entry
        cases[f"weight {w}"] = bad
    for name, flat in cases.items():
        path = str(tmp_path / f"{name.replace(' ', '_')}.npy")
        np.save(path, flat)
        with pytest.raises(AssertionError, match="weights outside" if name.startswith("weight") else "not a vote table"):
            rdf.VoteTable.load(path)


def test_shapes_and_types_the_python_layer_rejects(rdf, host_runtime):
    """On the host stand-in: every assertion comes before the entry point is called, which the stand-in does not have."""
    _mod("_build").build()
    depth, labels, forest, _ = wc.adversarial_case()
    n, H, W = depth.shape
    f = _forest(rdf, forest)
    d_cu, l_cu = rdf.to_device(depth), rdf.to_device(labels)
    fitter = rdf.VoteFitter(f, 5)
    targets = vc.targets_for(5, 255)
    for bad in (dict(labels=rdf.to_device(labels[:, :-1])), dict(labels=rdf.to_device(labels[:1])), dict(targets=targets.astype(np.int64)),
                dict(targets=vc.targets_for(16, 255)[:, :6]), dict(targets=targets[:1]), dict(depth=rdf.to_device(depth.astype(np.uint8)))):
        args = dict(depth=d_cu, labels=l_cu, targets=targets)
        args.update(bad)
        with pytest.raises(AssertionError):
            fitter.add(**args)
    for J, radius in ((0, 255), (17, 255), (5, -1), (5, 256)):
        with pytest.raises(AssertionError):
            rdf.VoteFitter(f, J, radius=radius)
    table = rdf.VoteTable(rdf.to_device(np.zeros(forest.shape[:2] + (2, 5, 4), np.int32)), rn.dims(forest))
    voter = rdf.JointVoter(f, table, (H, W), labels_reduce=2)
    gate = rdf.to_device(np.ones((n, H // 2, W // 2), np.uint16))
    for bad in (dict(depth=rdf.to_device(depth[:, :-1])), dict(gate=rdf.to_device(np.ones((n, H, W), np.uint16))),
                dict(gate=rdf.to_device(np.ones((1, H // 2, W // 2), np.uint16))), dict(out=rdf.DeviceArray((n, 5, 3), np.int32)),
                dict(out=rdf.DeviceArray((n, 5, 4), np.float32)), dict(out=rdf.DeviceArray((n + 1, 5, 4), np.int32))):
        args = dict(depth=d_cu, gate=gate)
        args.update(bad)
        with pytest.raises(AssertionError):
            voter.vote(**args)
    for kw in (dict(cell_shift=5), dict(box=5), dict(labels_reduce=0), dict(min_support=1 << 32), dict(min_support=-1), dict(max_frames=0)):
        with pytest.raises(AssertionError):
            rdf.JointVoter(f, table, (H, W), **kw)
    with pytest.raises(AssertionError):
        rdf.JointVoter(f, table, (H, 65536))                                    # the workspace of a frame too wide has no size
    with pytest.raises(AssertionError):
        rdf.VoteTable(rdf.to_device(np.zeros(forest.shape[:2] + (2, 5, 4), np.int64)), rn.dims(forest))


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _forest(rdf, forest):
    return rdf.DecisionForest.from_numpy(np.ascontiguousarray(forest))


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), f"{what}: {(got != want).sum()} words differ; first at {np.argwhere(got != want)[:5].tolist()}"


def _table(rdf, forest, votes):
    jv = _mod("joint_votes")
    return jv.VoteTable(rdf.to_device(np.ascontiguousarray(votes, np.int32)), rn.dims(forest))


@pytest.mark.gpu
def test_hand_worked_case_on_the_device(rdf, gpu_runtime):
    depth, labels, targets, forest = vc.hand_case()
    h = vc.HAND
    f = _forest(rdf, forest)
    fitter = rdf.VoteFitter(f, 1, radius=h["radius"]).add(rdf.to_device(depth), rdf.to_device(labels), targets)
    assert fitter.sums.get()[0, 0, :, 0].tolist() == [[2, 5, 2, 12, 15], [1, 2 ** 64 - 2, 0, 6, 4]]
    assert fitter.totals() == {"walked": 4, "no_depth": 1, "fell_off": 0, "offsets": 3}
    table = fitter.fit(h["min_count"], h["max_var"])
    assert table.votes.get()[0, 0, :, 0].tolist() == [[2, 1, 6, 128], [-2, 0, 6, 256]]
    assert table.report == {"leaf_slots": 2, "votes": 2, "dropped_support": 0, "dropped_spread": 0}
    for box, want in ((0, [80, 48, 70, 384]), (1, [72, 48, 70, 512])):
        voter = rdf.JointVoter(f, table, (4, 8), cell_shift=h["shift"], box=box)
        assert voter.vote(rdf.to_device(depth), gate=rdf.to_device(labels)).get().tolist() == [[want]]
    x, y, z, support = rdf.JointVoter.to_float(np.array([[[72, 48, 70, 512], [-1, -1, 0, 0]]], np.int32))
    assert x[0, 0] == 4.5 and y[0, 0] == 3. and z[0, 0] == 70. and support.tolist() == [[512, 0]]
    assert np.isnan(x[0, 1]) and np.isnan(y[0, 1]) and np.isnan(z[0, 1])


@pytest.fixture(scope="module")
def adv():
    depth, labels, forest, _ = wc.adversarial_case()
    return depth, labels, forest


ADV_FIT = dict(min_count=2, max_var=1 << 22)


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0, 255])
@pytest.mark.parametrize("J", [1, 5, 16])
@pytest.mark.parametrize("scale", wc.SCALES)
def test_adversarial_count_fit_cast(scale, J, radius, adv, rdf, gpu_runtime):
    """The forest and frames that break a walk (tests/walk_cases.py), through all three entry points; the device's table goes
    into the device's cast, the restatement's into the restatement's, so a difference anywhere shows in its own stage."""
    depth, labels, forest = adv
    targets = vc.targets_for(J, radius)
    want_sums, want_totals = vn.count(depth, labels, targets, forest, scale, radius, walk=vc.memo_walk)
    f = _forest(rdf, forest)
    d_cu = rdf.to_device(depth)
    fitter = rdf.VoteFitter(f, J, radius=radius).add(d_cu, rdf.to_device(labels), rdf.to_device(targets), scale)
    _same(fitter.sums.get(), want_sums, "sums")
    assert list(fitter.totals().values()) == [int(v) for v in want_totals]
    assert int(want_totals[0]) == len(vc.hand_pixels(depth, labels)) and int(want_totals[2]) > 0
    if radius == 255:
        assert int(want_totals[3]) > 1000
    else:
        assert 0 < int(want_totals[3]) <= 2 * forest.shape[0] * J
    want_votes, want_report = vn.fit(forest, want_sums, **ADV_FIT)
    table = fitter.fit(**ADV_FIT)
    _same(table.votes.get(), want_votes, "votes")
    assert list(table.report.values()) == [int(v) for v in want_report]
    if radius == 255:
        assert all(int(v) > 0 for v in want_report[:3])
    want = vn.vote(depth, forest, want_votes, scale, walk=vc.memo_walk)
    got = rdf.JointVoter(f, table, depth.shape[1:]).vote(d_cu, scale_factor=scale)
    _same(got.get(), want, "joints")
    assert np.array_equal(f.forest_cu.get().view(np.uint32), forest.view(np.uint32))        # nothing writes into the forest


@pytest.mark.gpu
def test_add_in_one_call_against_one_image_per_call(adv, rdf, gpu_runtime, monkeypatch):
    depth, labels, forest = adv
    targets = vc.targets_for(5, 255)
    f = _forest(rdf, forest)
    d_cu, l_cu = rdf.to_device(depth), rdf.to_device(labels)
    fitter = rdf.VoteFitter(f, 5).add(d_cu, l_cu, targets)
    whole, totals = fitter.sums.get(), fitter.totals()
    fitter.reset()
    assert not fitter.sums.get().any() and not any(fitter.totals().values())
    for i in range(depth.shape[0]):
        fitter.add(d_cu[i], l_cu[i], targets[i:i + 1])
    assert fitter.sums.get().tobytes() == whole.tobytes() and fitter.totals() == totals
    # ... and with the per-call pixel limit patched down to a frame and a half: add itself goes image by image
    dt = _mod("decision_tree")
    monkeypatch.setattr(dt, "_PIX_LIMIT", depth.shape[1] * depth.shape[2] * 3 // 2)
    assert dt._image_chunks(2, depth.shape[1] * depth.shape[2]) == [(0, 1), (1, 1)]
    fitter.reset().add(d_cu, l_cu, targets)
    assert fitter.sums.get().tobytes() == whole.tobytes() and fitter.totals() == totals
    fitter.add(d_cu, l_cu, targets)                         # the call adds
    twice = fitter.sums.get()
    assert np.array_equal(twice[..., 0], 2 * whole[..., 0]) and np.array_equal(twice, (whole + whole))


@pytest.mark.gpu
def test_fit_on_sums_written_directly(rdf, gpu_runtime):
    forest, sums, slots = vc.fit_case()
    f = _forest(rdf, forest)
    fitter = rdf.VoteFitter(f, vc.FIT["J"])
    fitter.sums.set(sums)
    for min_count, max_var in ((vc.FIT["min_count"], vc.FIT["max_var"]), (1, 0), (1, 1 << 38), (1 << 26, 17)):
        want, want_report = vn.fit(forest, sums, min_count, max_var)
        table = fitter.fit(min_count, max_var)
        _same(table.votes.get(), want, f"votes at {(min_count, max_var)}")
        assert list(table.report.values()) == [int(v) for v in want_report]
    table = fitter.fit(vc.FIT["min_count"], vc.FIT["max_var"])
    got = table.votes.get()
    at = lambda name: got[slots[name][0], slots[name][1], slots[name][2], slots[name][3]].tolist()      # noqa: E731
    assert at("at_min_count") == [1, 1, 1, 254] and at("below_min_count") == [0, 0, 0, 0]
    assert at("below_2_26") == [3, 0, -1, 256] and at("at_2_26") == [0, 0, 0, 0]
    assert at("var_at_max") == [0, 0, 0, 1] and at("var_above_max") == [0, 0, 0, 0]
    assert at("negative_sums") == [-2, -3, -6667, 256] and at("unreachable") == [0, 0, 0, 0]
    with pytest.raises(AssertionError):
        fitter.fit(0)
    with pytest.raises(AssertionError):
        fitter.fit(8, (1 << 38) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shift,box", [(0, 0), (0, 4), (2, 1), (2, 0), (4, 1), (4, 4)])
def test_cast_cells_and_boxes(shift, box, adv, rdf, gpu_runtime):
    """13 x 70 is no multiple of a cell of 4 or 16; at shift 4 the grid is 1 x 5 and a box of 4 covers it whole."""
    depth, labels, forest = adv
    votes, _ = vn.fit(forest, vn.count(depth, labels, vc.targets_for(5, 255), forest, walk=vc.memo_walk)[0], **ADV_FIT)
    want = vn.vote(depth, forest, votes, shift=shift, box=box, walk=vc.memo_walk)
    f = _forest(rdf, forest)
    got = rdf.JointVoter(f, _table(rdf, forest, votes), depth.shape[1:], cell_shift=shift, box=box).vote(rdf.to_device(depth))
    _same(got.get(), want, "joints")
    assert (want[..., 3] > 0).any()


@pytest.mark.gpu
def test_cast_reduce_gates_and_support(adv, rdf, gpu_runtime):
    depth, labels, forest = adv
    n, H, W = depth.shape
    votes, _ = vn.fit(forest, vn.count(depth, labels, vc.targets_for(5, 255), forest, walk=vc.memo_walk)[0], **ADV_FIT)
    f = _forest(rdf, forest)
    table = _table(rdf, forest, votes)
    d_cu = rdf.to_device(depth)
    gate = np.ascontiguousarray(labels[:, :H // 2 * 2:2, :W // 2 * 2:2])        # the truth at the pixels a reduce of 2 reads
    gate[0, 0, :3] = (65535, 0, 9)
    want = vn.vote(depth, forest, votes, gate=gate, r=2, walk=vc.memo_walk)
    voter = rdf.JointVoter(f, table, (H, W), labels_reduce=2)
    _same(voter.vote(d_cu, gate=rdf.to_device(gate)).get(), want, "joints at r = 2")
    assert (want[..., 3] > 0).any() and not np.array_equal(want, vn.vote(depth, forest, votes, walk=vc.memo_walk))
    # a gate that rejects everything, with both values that reject
    nothing = np.zeros_like(gate)
    nothing[:, ::2] = 65535
    out = rdf.DeviceArray((n, 5, 4), np.int32).fill(77)
    assert voter.vote(d_cu, gate=rdf.to_device(nothing), out=out) is out
    assert out.get().tolist() == [[[-1, -1, 0, 0]] * 5] * n
    # min_support one above the best
    plain = vn.vote(depth, forest, votes, walk=vc.memo_walk)
    best = int(plain[..., 3].max())
    at = np.argwhere(plain[..., 3] == best)
    for support, seen in ((best, True), (best + 1, False)):
        got = rdf.JointVoter(f, table, (H, W), min_support=support).vote(d_cu).get()
        _same(got, vn.vote(depth, forest, votes, min_support=support, walk=vc.memo_walk), f"joints at min_support {support}")
        assert all((got[i, j, 3] == best) == seen for i, j in at) and (got[..., 3] > 0).sum() == (len(at) if seen else 0)
    with pytest.raises(ValueError):
        rdf.JointVoter(_forest(rdf, forest[:, :31]), table, (H, W))                           # a forest of another depth


@pytest.mark.gpu
def test_votes_on_and_next_to_every_border(rdf, gpu_runtime):
    depth, forest, votes, gate_one, gate_two = vc.border_case()
    f = _forest(rdf, forest)
    voter = rdf.JointVoter(f, _table(rdf, forest, votes), depth.shape[1:], cell_shift=0, box=0)
    d_cu = rdf.to_device(depth)
    got = voter.vote(d_cu, gate=rdf.to_device(gate_one)).get()
    _same(got, vn.vote(depth, forest, votes, gate=gate_one, shift=0, box=0), "joints")
    assert got[0, :4].tolist() == [[120, 24, 64, 7], [-1, -1, 0, 0], [-1, -1, 0, 0], [88, 8, 64, 9]]             # vx = W - 1, W; vy = -1, 0
    assert got[0, 4:8].tolist() == [[-1, -1, 0, 0], [88, 24, 1, 11], [88, 24, 65534, 13], [-1, -1, 0, 0]]        # vz = 0, 1, 65534, 65535
    assert got[0, 8:].tolist() == [[88, 24, 70, 100], [-1, -1, 0, 0]]                                             # w = 0 is no vote
    got = voter.vote(d_cu, gate=rdf.to_device(gate_two)).get()
    _same(got, vn.vote(depth, forest, votes, gate=gate_two, shift=0, box=0), "joints")
    assert got[0, 8].tolist() == [24, 24, 70, 100]          # two cells of weight 100: the lower row-major index wins


@pytest.mark.gpu
def test_more_frames_than_the_workspace_holds(adv, rdf, gpu_runtime):
    depth, labels, forest = adv
    votes, _ = vn.fit(forest, vn.count(depth, labels, vc.targets_for(5, 255), forest, walk=vc.memo_walk)[0], **ADV_FIT)
    five = np.ascontiguousarray(np.concatenate([depth, depth[::-1], depth[:1]]))
    five[2:] = np.roll(five[2:], 3, axis=2)                 # frames 2 to 4 differ from 0 and 1
    f = _forest(rdf, forest)
    table = _table(rdf, forest, votes)
    d_cu = rdf.to_device(five)
    whole = rdf.JointVoter(f, table, depth.shape[1:], max_frames=8).vote(d_cu).get()
    chunked = rdf.JointVoter(f, table, depth.shape[1:], max_frames=2).vote(d_cu).get()
    assert chunked.tobytes() == whole.tobytes()
    _same(whole[:2], vn.vote(depth, forest, votes, walk=vc.memo_walk), "joints of the first two frames")
    assert not np.array_equal(whole[2], whole[1])


@pytest.mark.gpu
def test_a_wave_on_one_cell_and_on_64_cells(rdf, gpu_runtime):
    """Row 0 of the frame is one wave of k_votes_cast: its 64 lanes add to one cell of joint 0 and to 64 cells of joint 1."""
    depth, forest, votes = vc.wave_case()
    f = _forest(rdf, forest)
    table = _table(rdf, forest, votes)
    for shift, box in ((0, 0), (0, 1), (2, 1)):
        want = vn.vote(depth, forest, votes, shift=shift, box=box)
        got = rdf.JointVoter(f, table, depth.shape[1:], cell_shift=shift, box=box).vote(rdf.to_device(depth)).get()
        _same(got, want, f"joints at shift {shift}, box {box}")
    assert vn.vote(depth, forest, votes, shift=0, box=0).tolist() == [[[520, 8, 1022, 2080], [8, 8, 1000, 256]]]


@pytest.mark.gpu
def test_table_save_and_load(rdf, gpu_runtime, tmp_path):
    depth, forest, votes = vc.wave_case()
    table = _table(rdf, forest, votes)
    table.save(str(tmp_path / "votes.npy"))
    back = rdf.VoteTable.load(str(tmp_path / "votes.npy"))
    assert back.shape == table.shape == (1, 6, 1) and back.num_joints == 2 and back.votes.get().tobytes() == votes.tobytes()
    with pytest.raises(ValueError):
        back.check_forest(_forest(rdf, vc.all_left_stump()))


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
def test_end_to_end_on_rendered_hands(rdf, gpu_runtime):
    """Rendered frames, a forest of the package's own trainer, targets of fingertip_targets: fit on the training frames, vote on
    two frames the fit has not seen, device == restatement.  Nothing about accuracy is asserted here."""
    scene = _mod("hand_scene")
    H, W, n_train, n_test, T, D, C, P = 60, 106, 6, 2, 3, 5, 8, 16
    r = rdf.HandSceneRenderer((H, W), (75., 52.5, 29.5), max_frames=16)
    plane = scene.look_down_plane(5500.)
    poses = r.model.sample_poses(n_train + n_test, np.random.default_rng(31))
    depth_cu, labels_cu = r.render(r.transforms(poses, plane), "fine", None, 65535, 31)
    depth, labels = depth_cu.get(), labels_cu.get()
    targets = r.fingertip_targets(poses, plane)
    assert (targets[:, :, 2] > 0).all() and ((labels > 0).sum(axis=(1, 2)) > 200).all()
    ds = _ArrayDataset(depth[:n_train], labels[:n_train], C)
    trainer = rdf.DecisionTreeTrainer(n_train, P)
    trainer.allocate(ds, 2 * P, D)
    trees = []
    for k in range(T):
        tree = rdf.DecisionTree(D, C)
        np.random.seed(11 + k)
        trainer.train(ds, tree)
        trees.append(tree.tree_out_cu.get())
    forest = np.stack(trees)
    f = _forest(rdf, forest)
    fitter = rdf.VoteFitter(f, 5, radius=64).add(depth_cu[:n_train], labels_cu[:n_train], targets[:n_train])
    want_sums, want_totals = vn.count(depth[:n_train], labels[:n_train], targets[:n_train], forest, radius=64)
    _same(fitter.sums.get(), want_sums, "sums")
    assert list(fitter.totals().values()) == [int(v) for v in want_totals] and int(want_totals[3]) > 0
    table = fitter.fit(8, 1 << 22)
    want_votes, want_report = vn.fit(forest, want_sums, 8, 1 << 22)
    _same(table.votes.get(), want_votes, "votes")
    assert list(table.report.values()) == [int(v) for v in want_report] and int(want_report[1]) > 0
    got = rdf.JointVoter(f, table, (H, W)).vote(depth_cu[n_train:]).get()
    _same(got, vn.vote(depth[n_train:], forest, want_votes), "joints")
    x, y, z, support = rdf.JointVoter.to_float(got)
    print("voted tips", np.stack([x, y, z], -1).round(1).tolist(), "truth", targets[n_train:].tolist(), "support", support.tolist())


# ------------------------------------------------------------------ GPU: ties, 2^31, 64-bit votes, fall-offs -----------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(vc.TIE_LAYOUTS))
def test_mode_ties(name, rdf, gpu_runtime):
    """Equal cells and equal box sums: the first in row-major order wins, whichever thread of k_votes_modes holds it and on
    whichever of its trips.  The joint is TIE_LAYOUTS' literal, worked from V5 by hand."""
    depth, forest, votes, gate, shift, box = vc.tie_case(name)
    want = vn.vote(depth, forest, votes, gate=gate, shift=shift, box=box)
    assert want.tolist() == [[list(vc.TIE_LAYOUTS[name][3])]]
    voter = rdf.JointVoter(_forest(rdf, forest), _table(rdf, forest, votes), depth.shape[1:], cell_shift=shift, box=box)
    _same(voter.vote(rdf.to_device(depth), gate=rdf.to_device(gate)).get(), want, name)


@pytest.mark.gpu
def test_box_sums_above_2_31(rdf, gpu_runtime):
    """405 stumps on 144 x 144, every pixel 256 a tree onto its own cell of 16 x 16: each of the 81 cells holds 26542080 and the
    centre's box of 4 the whole grid, 2149908480: above 2^31 - 1, so the support is clamped, S and the centroid's sums need
    their 64 bits, and min_support (a uint32) is compared above 2^31.  The expected joints are V5 on the accumulator in closed
    form (the CPU tests hold that to the restatement's cast at T = 2).  Measured on the MI355X: the four casts of
    8.4 million votes each, onto 81 cells, take 87 ms together."""
    m = vc.SUM
    depth, forest, votes = vc.sum_case()
    acc, zacc = vc.full_grid(m["H"], m["W"], m["T"], m["d"], m["mz"], m["shift"])
    f, table, d_cu = _forest(rdf, forest), _table(rdf, forest, votes), rdf.to_device(depth)
    literal = ([1152, 1152, 1007, 2147483647], [128, 128, 1007, 26542080], [1152, 1152, 1007, 2147483647], [-1, -1, 0, 0])
    for (box, support), lit in zip(vc.SUM_RUNS, literal):
        want = vn.modes(acc, zacc, m["shift"], box, support)
        assert want.tolist() == [[lit]]
        got = rdf.JointVoter(f, table, depth.shape[1:], cell_shift=m["shift"], box=box, min_support=support).vote(d_cu).get()
        _same(got, want, f"the joint at box {box}, min_support {support}")


@pytest.mark.gpu
def test_votes_that_need_64_bits_and_weights_that_are_none(rdf, gpu_runtime):
    """128 m + d = 2^31 - 1 and -2^31 + 1 (the 32-bit division of vote_pixels), 2^31 and -2^31 (the 64-bit one), a vote that
    only a 32-bit 128 m + d would put into the frame, mx at both ends of int32, and weights of 257, -1, -256, 2^31 - 1 and
    -2^31, none of which is a vote.  The CPU tests state every column."""
    depth, forest, votes, gate = vc.wide_case()
    want = vn.vote(depth, forest, votes, gate=gate, shift=vc.WIDE["shift"], box=0)
    voter = rdf.JointVoter(_forest(rdf, forest), _table(rdf, forest, votes), depth.shape[1:], cell_shift=vc.WIDE["shift"], box=0)
    got = voter.vote(rdf.to_device(depth), gate=rdf.to_device(gate)).get()
    _same(got, want, "joints")
    assert (got[..., 3] > 0).sum() == 8 and got[0, 0].tolist() == [256 * 1026 + 128, 128, 65407, 9] and got[3, 1].tolist() == [256 * 162 + 128, 128, 65408, 9]


@pytest.mark.gpu
def test_min_support_0(rdf, gpu_runtime):
    """V5's max(min_support, 1): with min_support 0 a joint without a vote is (-1, -1, 0, 0), not a division by its best 0."""
    depth, forest, votes, gate_one, _ = vc.border_case()
    want = vn.vote(depth, forest, votes, gate=gate_one, shift=0, box=0, min_support=0)
    voter = rdf.JointVoter(_forest(rdf, forest), _table(rdf, forest, votes), depth.shape[1:], cell_shift=0, box=0, min_support=0)
    out = rdf.DeviceArray(want.shape, np.int32).fill(77)
    got = voter.vote(rdf.to_device(depth), gate=rdf.to_device(gate_one), out=out).get()
    _same(got, want, "joints")
    assert got[0, [1, 2, 4, 7, 9]].tolist() == [[-1, -1, 0, 0]] * 5 and got[0, 8].tolist() == [88, 24, 70, 100] and (got[0, [0, 3, 5, 6], 3] > 0).all()


@pytest.mark.gpu
def test_a_fall_off_in_a_middle_tree(rdf, gpu_runtime):
    """Three stumps; the second tells the hand pixels with x <= 5 to go on at level D - 1.  They are counted in totals[2] and
    still sum, and vote, through the first and the third tree."""
    depth, labels, targets, forest = vc.middle_case()
    radius, shift = vc.HAND["radius"], vc.HAND["shift"]
    want_sums, want_totals = vn.count(depth, labels, targets, forest, radius=radius)
    f, d_cu, l_cu = _forest(rdf, forest), rdf.to_device(depth), rdf.to_device(labels)
    fitter = rdf.VoteFitter(f, 1, radius=radius).add(d_cu, l_cu, targets)
    _same(fitter.sums.get(), want_sums, "sums")
    assert fitter.totals() == {"walked": 4, "no_depth": 1, "fell_off": 3, "offsets": 7} and want_totals.tolist() == [4, 1, 3, 7]
    assert want_sums[:, 0, :, 0, 0].tolist() == [[2, 1], [0, 1], [3, 0]]
    want_votes, want_report = vn.fit(forest, want_sums, **vc.MIDDLE_FIT)
    table = fitter.fit(**vc.MIDDLE_FIT)
    _same(table.votes.get(), want_votes, "votes")
    assert list(table.report.values()) == [int(v) for v in want_report] == [5, 4, 1, 0]
    for box in (0, 1):
        got = rdf.JointVoter(f, table, depth.shape[1:], cell_shift=shift, box=box).vote(d_cu, gate=l_cu).get()
        _same(got, vn.vote(depth, forest, want_votes, gate=labels, shift=shift, box=box), f"joints at box {box}")


# ------------------------------------------------------------------ GPU: past one sweep of each grid --------------------------
@pytest.mark.gpu
def test_count_past_one_sweep(rdf, gpu_runtime):
    """294334 pixels in two images: k_votes_count's grid of 1024 x 256 lanes takes a second trip, in which a wave holds the
    last pixels and lanes past them; the image boundary lies inside a wave of the first."""
    depth, labels, targets, forest = vc.count_sweep_case()
    radius = vc.COUNT_SWEEP["radius"]
    want_sums, want_totals = vn.count(depth, labels, targets, forest, radius=radius)
    f, d_cu, l_cu = _forest(rdf, forest), rdf.to_device(depth), rdf.to_device(labels)
    fitter = rdf.VoteFitter(f, vc.COUNT_SWEEP["J"], radius=radius).add(d_cu, l_cu, targets)
    _same(fitter.sums.get(), want_sums, "sums")
    assert list(fitter.totals().values()) == [int(v) for v in want_totals]
    whole = fitter.sums.get()
    fitter.reset()
    for i in range(depth.shape[0]):
        fitter.add(d_cu[i], l_cu[i], targets[i:i + 1])
    assert fitter.sums.get().tobytes() == whole.tobytes() and list(fitter.totals().values()) == [int(v) for v in want_totals]


@pytest.mark.gpu
def test_fit_past_one_sweep(rdf, gpu_runtime):
    """T5/D16: 327675 nodes, so k_votes_fit's grid takes a second trip, for the last tree from its node 4 on.  VoteFitter.fit
    makes a new array per call, so "every element is written" is asked of the entry point itself, given an array that holds a
    pattern."""
    forest, sums, slots, leaf = vc.fit_sweep_case()
    m = vc.FIT_SWEEP
    want, want_report = vn.fit(forest, sums, m["min_count"], m["max_var"])
    f = _forest(rdf, forest)
    fitter = rdf.VoteFitter(f, 1)
    fitter.sums.set(sums)
    table = fitter.fit(m["min_count"], m["max_var"])
    _same(table.votes.get(), want, "votes")
    assert list(table.report.values()) == [int(v) for v in want_report]
    votes = rdf.DeviceArray(want.shape, np.int32).fill(0x55555555)
    report = rdf.DeviceArray((4,), np.uint64).fill(np.uint64(77))
    lib = _mod("_lib").load("labels")
    rc = lib.rdf_labels_votes_fit(rdf.device_ptr(f.forest_cu), m["T"], m["D"], 1, 1, fitter.sums.ptr, m["min_count"], m["max_var"],
                                  votes.ptr, report.ptr, gpu_runtime.stream())
    assert rc == 0
    _same(votes.get(), want, "votes written over a pattern")
    assert report.get().tolist() == want_report.tolist()
    assert want[slots["negative_sums in tree 4"]].tolist() == [-2, -3, -6667, 256] and not want[slots["unreachable"]].any()


@pytest.mark.gpu
def test_modes_past_one_sweep(rdf, gpu_runtime):
    """4097 frames of 2 x 2 with 16 joints: 65552 (frame, joint) pairs, so 16 workgroups of k_votes_modes' grid of 65536 take a
    second pair, frame 4096's after frame 0's, and the two frames differ in every joint."""
    depth, forest, votes, kind = vc.modes_sweep_case()
    want = vc.vote_by_kind(vn)
    f, table, d_cu = _forest(rdf, forest), _table(rdf, forest, votes), rdf.to_device(depth)
    out = rdf.DeviceArray(want.shape, np.int32).fill(77)
    voter = rdf.JointVoter(f, table, depth.shape[1:], cell_shift=0, box=0, max_frames=vc.MODES["frames"])
    assert voter.vote(d_cu, out=out) is out
    whole = out.get()
    _same(whole, want, "joints")
    chunked = rdf.JointVoter(f, table, depth.shape[1:], cell_shift=0, box=0, max_frames=64).vote(d_cu).get()
    assert chunked.tobytes() == whole.tobytes()


@pytest.mark.gpu
def test_a_table_outlives_a_refit_of_the_pdfs(adv, rdf, gpu_runtime):
    """VoteTable's promise: a table is indexed by leaf slot, so LeafRefitter.apply, which rewrites the PDFs alone, leaves the
    votes of a frame as they were, and a new fit gives the same table.  A single [H, W] frame is a batch of one."""
    depth, labels, forest = adv
    targets = vc.targets_for(5, 255)
    f = _forest(rdf, forest)
    d_cu, l_cu = rdf.to_device(depth), rdf.to_device(labels)
    table = rdf.VoteFitter(f, 5).add(d_cu, l_cu, targets).fit(**ADV_FIT)
    voter = rdf.JointVoter(f, table, depth.shape[1:])
    before = voter.vote(d_cu).get()
    want_votes = vc.adv_table(5, 255)[1]
    _same(table.votes.get(), want_votes, "votes")
    _same(before, vn.vote(depth, forest, want_votes, walk=vc.memo_walk), "joints before the refit")
    assert (before[..., 3] > 0).any()
    report = rdf.LeafRefitter(f).add(d_cu, l_cu).apply()
    after = f.forest_cu.get()
    assert report["own"] > 0 and not np.array_equal(after.view(np.uint32), forest.view(np.uint32))
    assert np.array_equal(after[:, :, :7].view(np.uint32), forest[:, :, :7].view(np.uint32))          # the structure is as it was
    assert voter.vote(d_cu).get().tobytes() == before.tobytes()
    again = rdf.VoteFitter(f, 5).add(d_cu, l_cu, targets).fit(**ADV_FIT)
    assert again.votes.get().tobytes() == table.votes.get().tobytes() and again.report == table.report
    one = voter.vote(d_cu[1]).get()
    assert one.shape == (1, 5, 4) and one.tobytes() == before[1:].tobytes()
