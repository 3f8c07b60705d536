"""Voted fingertips: rdf_labels_vote_tips (rules T of include/rdf_labels.h) against the restatement in tests/vote_tips_numpy.py,
and the voter's way through HandPipeline and BeatsSession (joint_voter=, joint_votes=).  The CPU tests pin every rule to
literals, check that the cases hold what they are meant to, and the argument checks of the entry point and of the constructor,
which launch nothing.  Every GPU comparison is `==` with NaN positions equal."""
import ctypes
import importlib
import os
import zlib

import numpy as np
import pytest

import session_cases as sc
import soft_modes_cases as smc
import vote_tips_cases as tc
import vote_tips_numpy as tn
import votes_cases as vc
from oracle import mean_shift_numpy as ms_np


def _mod(name):
    return importlib.import_module("3d-beats_amd." + name)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), \
        f"{what}: differs at {np.argwhere(~((got == want) | ((got != got) & (want != want))))[:5].tolist()}"


# ------------------------------------------------------------------ CPU: the rules -------------------------------------------
def test_every_rule_on_literals():
    """T1.  trunc, not floor: 3.99 -> 3, -0.99 -> 0 (on the frame), -1.5 -> -1 (off it); times r after the truncation: 3.7 at
    r = 2 is 6, not 7.  1e9 is refused, the double below it is not (and is off the frame).
    T2.  floordiv(-1, 16) = -1 -> clamp 0; floordiv(15, 16) = 0; floordiv(16, 16) = 1.  Flipped at dim_x = 13: Xu = 208 - X, so
    X = 8 (centre of pixel 0) -> 200 -> pixel 12; X = 208 -> 0 -> pixel 0; X = 209 -> -1 -> floordiv -1 -> clamp 0.
    T3.  Distances are Chebyshev: (6, 4) against (8, 5) is 2.
    T4.  |zs - Z| <= z_tol on both sides; zs of 0 or 65535 is never taken, even when Z is 0 or 65535 itself.
    T5.  fx = fy = 2, pp = (1, 1), plane row (0.5, 0.25, -1, 10): pixel (3, 5) at z = 8: x = 1, y = 2, pt = (8, 16, 8, 1):
    height = -(4 + 4 - 8 + 10) = -10."""
    assert tn.mode_candidate(3.99, 0.5, 1, 13, 9) == (3, 0) and tn.mode_candidate(-0.99, 0.0, 1, 13, 9) == (0, 0)
    assert tn.mode_candidate(-1.5, 2.0, 2, 13, 9) is None and tn.mode_candidate(3.7, 2.2, 2, 13, 9) == (6, 4)
    assert tn.mode_candidate(6.0, 4.0, 2, 13, 9) == (12, 8) and tn.mode_candidate(6.5, 4.0, 2, 13, 9) == (12, 8)
    assert tn.mode_candidate(7.0, 4.0, 2, 13, 9) is None and tn.mode_candidate(6.0, 4.5, 2, 13, 8) is None
    assert tn.mode_candidate(float("nan"), 1.0, 1, 13, 9) is None and tn.mode_candidate(1.0, float("nan"), 1, 13, 9) is None
    assert tn.mode_candidate(float("inf"), 1.0, 1, 13, 9) is None and tn.mode_candidate(1.0, -float("inf"), 1, 13, 9) is None
    assert tn.mode_candidate(1e9, 1.0, 1, 2 ** 31, 9) is None and tn.mode_candidate(np.nextafter(1e9, 0), 1.0, 1, 2 ** 31, 9) == (999999999, 1)
    assert tn.mode_candidate(np.nextafter(1e9, 0), 1.0, 1, 13, 9) is None and tn.mode_candidate(0.0, 0.0, 1, 0, 9) is None
    assert tn.vote_candidate((-1, 15, 70, 1), 0, 13, 9) == (0, 0, 70) and tn.vote_candidate((16, 16 * 9 - 1, 70, 1), 0, 13, 9) == (1, 8, 70)
    assert tn.vote_candidate((16 * 13, 16 * 9, -5, 1), 0, 13, 9) == (12, 8, -5) and tn.vote_candidate((-10 ** 6, 10 ** 6, 1, 1), 0, 13, 9) == (0, 8, 1)
    assert tn.vote_candidate((8, 8, 70, 1), 1, 13, 9) == (12, 0, 70) and tn.vote_candidate((208, 8, 70, 1), 1, 13, 9) == (0, 0, 70)
    assert tn.vote_candidate((209, 8, 70, 1), 1, 13, 9) == (0, 0, 70) and tn.vote_candidate((-1, 8, 70, 1), 1, 13, 9) == (12, 0, 70)
    assert tn.vote_candidate((-2 ** 31, 2 ** 31 - 1, 70, 1), 1, 65535, 65535) == (65534, 65534, 70)
    assert tn.vote_candidate((8, 8, 70, 0), 0, 13, 9) is None and tn.vote_candidate((8, 8, 70, -3), 0, 13, 9) is None
    assert tn.vote_candidate((8, 8, 70, 1), 0, 0, 9) is None and tn.vote_candidate((8, 8, 70, 1), 0, 13, 0) is None
    m, v = (6, 4), (8, 5, 70)
    assert [tn.choose(m, v, p, 2) for p in (tn.FILL, tn.GUARD, tn.VOTES)] == ["mode", "mode", "vote"]
    assert tn.choose(m, v, tn.GUARD, 1) == "vote" and tn.choose(m, (6, 2, 70), tn.GUARD, 1) == "vote" and tn.choose(m, (7, 3, 70), tn.GUARD, 1) == "mode"
    assert tn.choose(m, (6, 4, 70), tn.GUARD, 0) == "mode" and tn.choose(m, (6, 5, 70), tn.GUARD, 0) == "vote"
    for p in (tn.FILL, tn.GUARD, tn.VOTES):
        assert tn.choose(m, None, p, 0) == "mode" and tn.choose(None, v, p, 0) == "vote" and tn.choose(None, None, p, 0) is None
    assert tn.vote_depth(700, 705, 5) == (700, 2) and tn.vote_depth(700, 705, 4) == (705, 3)
    assert tn.vote_depth(710, 705, 5) == (710, 2) and tn.vote_depth(711, 705, 5) == (705, 3)
    assert tn.vote_depth(0, 3, 5) == (3, 3) and tn.vote_depth(65535, 65534, 5) == (65534, 3) and tn.vote_depth(0, 0, 0) == (0, 3)
    assert tn.vote_depth(65535, 65535, 0) == (65535, 3) and tn.vote_depth(1, -7, 8) == (1, 2) and tn.vote_depth(65534, 0, 65535) == (65534, 2)
    plane = np.zeros((4, 4), np.float32)
    plane[2] = (0.5, 0.25, -1., 10.)
    assert tn.height_at(3, 5, 8, (2., 2., 1., 1.), plane) == -10.
    # fp32 deprojection: (1 - 0.1f) / 3f in float, not in double
    x = (np.float32(1) - np.float32(0.1)) / np.float32(3)
    plane[2] = (1., 0., 0., 0.)
    assert tn.height_at(1, 0, 7, (3., 1., 0.1, 0.), plane) == -np.float64(np.float32(7) * x) != -7 * (1 - 0.1) / 3


def test_the_flip_maps_pixel_centres_onto_pixel_centres():
    for dim_x in (1, 2, 13, 424, 65535):
        for p in {0, min(1, dim_x - 1), dim_x // 2, dim_x - 1}:
            assert tn.flipped(tc.centre(p), dim_x) == tc.centre(dim_x - 1 - p)
            assert tn.vote_candidate((tc.centre(p), 8, 1, 1), 1, dim_x, 1) == (dim_x - 1 - p, 0, 1)
    # ... and the left edge of pixel p onto the right edge of its mirror, which belongs to the next pixel: floordiv, not a mirror
    assert tn.vote_candidate((16 * 5, 8, 1, 1), 1, 13, 1)[0] == 8 and tn.vote_candidate((16 * 5 + 1, 8, 1, 1), 1, 13, 1)[0] == 7


def test_the_centre_of_a_border_cell_clamps():
    """13 pixels in cells of 4 (cell_shift 2): the last cell starts at pixel 12 and its centre, rule V5's 16 * 12 + 8 * 4 = 224,
    is in pixel 14; 9 rows: the last cell starts at row 8, centre 160 -> row 10.  Flipped, 224 maps to -16: pixel -1."""
    X, Y = 16 * 12 + 8 * 4, 16 * 8 + 8 * 4
    assert (X // 16, Y // 16) == (14, 10)
    assert tn.vote_candidate((X, Y, 5, 1), 0, 13, 9) == (12, 8, 5) and tn.vote_candidate((X, Y, 5, 1), 1, 13, 9) == (0, 8, 5)


def test_a_mode_sourced_height_is_the_existing_routes():
    """FILL with every tip's mode present: the heights of oracle/mean_shift_numpy.py's fingertip_heights.  That one takes the
    plane's row with numpy's matrix product, whose order of adding the four terms is numpy's own; the kernels and rule T5 add
    them from 0.0 in index order, so the two may differ in the last bits, and no more: each of the four roundings is half an
    ulp of a partial sum, and the partial sums here stay below 2^10 while the results are above 2^5.  (That a mode-sourced
    height is bit for bit the mode launch's is the device test's, test_a_voter_without_votes_changes_nothing.)"""
    means, joints, depth = tc.kernel_case()
    ids = (1, 5, 6)
    got, tips = tn.vote_tips(means[:1], ids, (0, 1, 2), joints[:1], 0, depth[:1], tc.R, tc.INTR, tc.plane(), tn.FILL, 0, 0)
    want = ms_np.fingertip_heights(means[0], list(ids), depth[0], tc.R, *tc.INTR, tc.plane())
    assert not np.isnan(want).any() and (np.abs(want) > 32).all() and tips[0, :, 3].tolist() == [1, 1, 1]
    assert (np.abs(got[0] - want) <= 4 * np.spacing(1024.)).all()


def test_the_cases_contain_what_they_are_meant_to():
    case = tc.kernel_case()
    means, joints, depth = case
    assert means.shape == (3, tc.L, 2) and joints.shape == (3, tc.J, 4) and depth.shape == (3, tc.H, tc.W)
    out = {run: tc.run(tn, case, *run) for run in tc.RUNS}
    for (flip, policy, md, zt), (h, t) in out.items():
        assert np.array_equal(np.isnan(h), t[..., 3] == 0) and (t[t[..., 3] == 0] == tn.NONE).all()
        assert set(t[..., 3].reshape(-1).tolist()) <= {0, 1, 2, 3}
        assert t[0, 3].tolist() == list(tn.NONE) and t[1, 4].tolist() == list(tn.NONE)           # no class and support 0; 1e9 and joint -1
        assert t[0, 4].tolist() == [2, 6, 0, 1] and t[0, 1].tolist() == [10 if flip else 2, 1, 3, 3]        # depth 0 as it is; zs = 0
        assert t[0, 2].tolist() == [9 if flip else 3, 7, 65533, 3]                                    # zs = 65535
        assert t[1, 1, :2].tolist() == ([0, 0] if flip else [12, 0])                                # X clamps on each side, Y at 0
        assert t[1, 3].tolist() == ([11, 5, 800, 3] if flip else [1, 5, 803, 2])
    assert sorted({int(s) for h, t in out.values() for s in t[..., 3].reshape(-1)}) == [0, 1, 2, 3]
    for flip in (0, 1):
        vote = 4 if flip else 8
        assert out[flip, tn.FILL, 2, 5][1][0, 0].tolist() == [6, 4, 650, 1] == out[flip, tn.GUARD, 2, 5][1][0, 0].tolist()
        assert out[flip, tn.GUARD, 1, 5][1][0, 0].tolist() == [vote, 5, 710 if flip else 700, 2]    # max_dist one below the distance
        assert out[flip, tn.VOTES, 2, 5][1][0, 0].tolist() == [vote, 5, 710 if flip else 700, 2]
        assert out[flip, tn.VOTES, 2, 4][1][0, 0].tolist() == [vote, 5, 705, 3]                     # z_tol one below the difference
        assert out[flip, tn.VOTES, 2, 5][1][1, 0].tolist()[:2] == [12 if flip else 0, 8]            # X = -40, Y = 147
        assert out[flip, tn.FILL, 2, 5][1][1, 2].tolist() == [10, 6, 65535, 1]                      # a mode on 65535, as it is
        assert out[flip, tn.FILL, 2, 5][1][2, 0, :2].tolist() == [0, 4] and out[flip, tn.FILL, 2, 5][1][2, 4, :2].tolist() == [12, 8]
        assert out[flip, tn.VOTES, 2, 4][1][1, 2].tolist() == [6, 2, int(depth[1, 2, 6]), 2]
    # the policies and the flips give different answers on the drawn frame too
    assert len({out[run][1].tobytes() for run in tc.RUNS}) >= 8
    # a stride beyond the tips keeps what lies between the rows
    h, _ = tc.run(tn, case, 0, tn.VOTES, 2, 5, stride=tc.STRIDE)
    assert h.shape == (3, tc.STRIDE) and (h[:, 5:] == tc.SENTINEL).all() and np.array_equal(h[:, :5], out[0, tn.VOTES, 2, 5][0], equal_nan=True)
    # the sweep
    means, joints, depth = tc.sweep_case()
    assert means.shape[0] * len(tc.SWEEP_IDS) == 1500 > tc.SWEEP_LANES
    for run in tc.SWEEP_RUNS:
        h, t = tc.run_sweep(tn, (means, joints, depth), *run)
        late = t.reshape(-1, 4)[tc.SWEEP_LANES:, 3]
        assert set(late.tolist()) == {0, 1, 2, 3} if run[1] != tn.FILL else {0, 1} < set(late.tolist())


# ------------------------------------------------------------------ CPU: arguments -------------------------------------------
def test_rejected_arguments_launch_nothing(rdf):
    """Rejected arguments launch nothing, so they need no device; the pointers given here are never followed."""
    _mod("_build").build()
    lib = _mod("_lib").load("labels")
    P = ctypes.c_void_p
    m, ids, tj, jt, d, pl, h, t = (P(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000))
    BAD, NULL, LARGE = -1, -2, -3

    def call(means=m, n=2, L=6, class_ids=ids, tip_joints=tj, n_ids=5, joints=jt, J=6, flip=0, depth=d, dims=(13, 9), r=2, plane=pl,
             policy=0, max_dist=8, z_tol=30, heights=h, stride=5, tips=t):
        return lib.rdf_labels_vote_tips(means, n, L, class_ids, tip_joints, n_ids, joints, J, flip, depth, *dims, r, 1., 1., 0., 0., plane,
                                        policy, max_dist, z_tol, heights, stride, tips, None)
    for kw in (dict(n=-1), dict(L=0), dict(L=-1), dict(n_ids=0), dict(n_ids=-1), dict(J=0), dict(J=17), dict(J=-1), dict(dims=(-1, 9)),
               dict(dims=(13, -1)), dict(dims=(65536, 9)), dict(dims=(13, 65536)), dict(r=0), dict(r=-2), dict(policy=-1), dict(policy=3),
               dict(max_dist=-1), dict(max_dist=65536), dict(z_tol=-1), dict(z_tol=65536), dict(stride=4), dict(n_ids=6)):
        assert call(**kw) == BAD, kw
    for kw in (dict(means=P(0x10004)), dict(class_ids=P(0x20002)), dict(tip_joints=P(0x30002)), dict(joints=P(0x40008)),
               dict(depth=P(0x50001)), dict(plane=P(0x60002)), dict(heights=P(0x70004)), dict(tips=P(0x80008))):
        assert call(**kw) == BAD, kw
    assert call(n=1 << 27, n_ids=16, stride=16, dims=(1, 1)) == LARGE and call(n=32768, dims=(256, 256)) == LARGE
    for name in ("means", "class_ids", "tip_joints", "joints", "depth", "plane", "heights"):
        assert call(**{name: None}) == NULL, name
    assert call(n=0, means=None, class_ids=None, tip_joints=None, joints=None, depth=None, plane=None, heights=None, tips=None) == 0
    assert call(n=0, policy=3) == BAD and call(n=0, stride=4) == BAD          # a bad argument is one on zero frames too
    assert call(means=None, tips=None) == NULL                                 # (tips may be NULL: the next check is met)
    for name in ("RDF_TIPS_FILL 0", "RDF_TIPS_GUARD 1", "RDF_TIPS_VOTES 2"):
        assert f"#define {name}\n" in open(_mod("_build").LIBRARIES["labels"].headers[0]).read()
    assert _mod("pipeline").TIP_POLICIES == tn.POLICIES


def test_what_the_constructor_refuses(rdf, host_runtime):
    """Every ValueError comes before anything is allocated and before the stack is marked as the pipeline's."""
    _mod("_build").build()
    pl = _mod("pipeline")
    forest = rdf.DecisionForest.from_numpy(vc.all_left_stump())
    table = rdf.VoteTable(rdf.to_device(np.zeros((1, 1, 2, 5, 4), np.int32)), (1, 1, 1))
    voter = rdf.JointVoter(forest, table, (48, 64))

    class Stack:
        num_layered_classes = 7
    args = ((48, 64), 2, 1.0, 6, np.full(7, 8., np.float32), [2, 3, 4, 5, 6], (60., 60., 32., 24.), np.eye(4))
    for kw in (dict(joint_voter=object()), dict(joint_voter=table), dict(joint_voter=(forest, table)),
               dict(joint_voter=rdf.JointVoter(forest, table, (64, 48))), dict(joint_voter=voter, fused_io=False),
               dict(joint_voter=voter, tip_policy="always"), dict(joint_voter=voter, tip_policy=0),
               dict(joint_voter=voter, tip_joints=[0, 1, 2, 3]), dict(joint_voter=voter, tip_joints=[0, 1, 2, 3, 5]),
               dict(joint_voter=voter, tip_joints=[0, 1, 2, 3, -2]), dict(joint_voter=voter, tip_max_dist=-1),
               dict(joint_voter=voter, tip_max_dist=65536), dict(joint_voter=voter, tip_z_tol=65536)):
        stack = Stack()
        with pytest.raises(ValueError):
            pl.HandPipeline(stack, *args, **kw)
        assert not hasattr(stack, "_pipeline_owner") and not hasattr(voter, "_pipeline_owner"), kw
    sib = voter.sibling()
    assert sib is not voter and sib.table is voter.table and sib.forest is voter.forest and sib._workspace.ptr != voter._workspace.ptr
    assert (sib.DIM_Y, sib.DIM_X, sib.labels_reduce, sib.cell_shift, sib.box, sib.min_support, sib.max_frames) == \
        (voter.DIM_Y, voter.DIM_X, voter.labels_reduce, voter.cell_shift, voter.box, voter.min_support, voter.max_frames)


# ------------------------------------------------------------------ CPU: targets beside a dataset ----------------------------
class _Host:
    def __init__(self, a):
        self._a = a

    def get(self):
        return self._a


def _renderer(rdf, H, W):
    """A HandSceneRenderer without a device: make_dataset's render is a stand-in that draws from the transforms' bytes."""
    scene = _mod("hand_scene")
    r = scene.HandSceneRenderer.__new__(scene.HandSceneRenderer)
    r.f, r.ppx, r.ppy, r.z_near, r.z_far, r.DIM_Y, r.DIM_X = 75., 52.5, 29.5, 50., 50000., H, W
    r.model = rdf.HandModel()
    r.left_model = r.model.mirrored()

    def render(tforms, labels, table, empty_depth, seed, hole_rate, noise_amp, sensor=None):
        rng = np.random.default_rng(zlib.crc32(np.asarray(tforms, np.float32).tobytes()))
        n = len(tforms)
        return _Host(rng.integers(0, 65536, (n, H, W)).astype(np.uint16)), _Host(rng.integers(0, 9, (n, H, W)).astype(np.uint16))
    r.render = render
    return r, scene


@pytest.mark.parametrize("two_hands", [False, True])
def test_targets_beside_a_dataset(two_hands, rdf, tmp_path):
    ds = _mod("dataset")
    H, W, n = 12, 20, 5
    r, scene = _renderer(rdf, H, W)
    plane = scene.look_down_plane(5500.)
    plain, with_t = str(tmp_path / "plain"), str(tmp_path / "targets")
    r.make_dataset(plain, n, seed=9, plane=plane, two_hands=two_hands)
    r.make_dataset(with_t, n, seed=9, plane=plane, two_hands=two_hands, targets=True)
    # without targets: the files a dataset directory always had, and the same bytes in both
    names = sorted(["config.json"] + [f"{str(i).zfill(8)}_{k}.png" for i in range(n) for k in ("depth", "labels")])
    assert sorted(os.listdir(plain)) == names and sorted(os.listdir(with_t)) == sorted(names + [ds.TARGETS_FILE])
    for name in names:
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(with_t, name), "rb").read(), name
    # the targets: fingertip_targets of the poses make_dataset samples, for the plane it rendered with
    rng = np.random.default_rng(9)
    poses = r.model.sample_poses(n, rng, None)
    left = None
    if two_hands:
        shift = np.zeros(poses.shape[1])
        shift[0] = 110. * r.model.units_per_mm
        left = r.left_model.sample_poses(n, rng, None) - shift
        poses = poses + shift
    want = r.fingertip_targets(poses, plane, left)
    assert want.shape == (n, 10 if two_hands else 5, 3) and (want[..., 2] > 0).any()
    got = ds.read_targets(with_t, range(n))
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes()
    assert ds.read_targets(with_t, [3, 0, 3]).tobytes() == want[[3, 0, 3]].tobytes() and ds.read_targets(with_t, []).shape == (0,) + want.shape[1:]
    with pytest.raises(FileNotFoundError, match="no joint targets"):
        ds.read_targets(plain, [0])
    with pytest.raises(IndexError):
        ds.read_targets(with_t, [n])
    np.save(os.path.join(with_t, ds.TARGETS_FILE), want[:-1])
    with pytest.raises(ValueError):
        ds.read_targets(with_t, [0])


# ------------------------------------------------------------------ GPU: the kernel alone ------------------------------------
def _device_tips(rdf, case, ids, tip_joints, r, flip, policy, max_dist, z_tol, stride=None, with_tips=True):
    means, joints, depth = case
    lib, rt = _mod("_lib").load("labels"), rdf.get_runtime()
    n, L = means.shape[:2]
    H, W = depth.shape[1:]
    stride = len(ids) if stride is None else stride
    heights = rdf.DeviceArray((n, stride), np.float64).fill(tc.SENTINEL)
    tips = rdf.DeviceArray((n, len(ids), 4), np.int32).fill(77)
    dev = [rdf.to_device(np.ascontiguousarray(a)) for a in (means, np.asarray(ids, np.int32), np.asarray(tip_joints, np.int32), joints,
                                                            depth, tc.plane())]
    rc = lib.rdf_labels_vote_tips(dev[0].ptr, n, L, dev[1].ptr, dev[2].ptr, len(ids), dev[3].ptr, joints.shape[1], flip, dev[4].ptr, W, H,
                                  r, *tc.INTR, dev[5].ptr, policy, max_dist, z_tol, heights.ptr, stride, tips.ptr if with_tips else None,
                                  rt.stream())
    assert rc == 0, rc
    heights.mark_dirty()
    tips.mark_dirty()
    return heights.get(), tips.get()


@pytest.mark.gpu
def test_the_kernel_against_the_restatement(rdf, gpu_runtime):
    case = tc.kernel_case()
    for run in tc.RUNS:
        want_h, want_t = tc.run(tn, case, *run)
        got_h, got_t = _device_tips(rdf, case, tc.CLASS_IDS, tc.TIP_JOINTS, tc.R, *run)
        _same(got_h, want_h, f"heights of {run}")
        _same(got_t, want_t, f"tips of {run}")
    # a stride beyond the tips: the sentinels between the rows survive; and without tips_out: the same heights, nothing written there
    run = (1, tn.VOTES, 2, 5)
    want_h, _ = tc.run(tn, case, *run, stride=tc.STRIDE)
    got_h, got_t = _device_tips(rdf, case, tc.CLASS_IDS, tc.TIP_JOINTS, tc.R, *run, stride=tc.STRIDE, with_tips=False)
    _same(got_h, want_h, "heights at a stride of 7")
    assert (got_h[:, 5:] == tc.SENTINEL).all() and (got_t == 77).all()


@pytest.mark.gpu
def test_more_pairs_than_one_sweep_of_the_grid(rdf, gpu_runtime):
    case = tc.sweep_case()
    for flip, policy in tc.SWEEP_RUNS:
        want_h, want_t = tc.run_sweep(tn, case, flip, policy)
        got_h, got_t = _device_tips(rdf, case, tc.SWEEP_IDS, tc.SWEEP_JOINTS, tc.SWEEP["r"], flip, policy, 3, 6)
        _same(got_h, want_h, f"heights of {(flip, policy)}")
        _same(got_t, want_t, f"tips of {(flip, policy)}")


# ------------------------------------------------------------------ GPU: the pipeline ----------------------------------------
TIPS = (2, 3, 4, 5, 6)
FRAMES = 3
VOTER = dict(labels_reduce=2)
# every leaf votes one fixed offset per joint (at a hand's depth of about 400, 64 m / d pixels: 16 pixels for m = 100); joint 4
# votes 3000 units behind the hand: its depth is never the sensor's; joint 2 stays on the voting pixel: the densest cell of the hand
STUMP_VOTES = ((-250, -100, -4, 256), (-120, -220, 3, 256), (0, 0, 0, 256), (120, -220, 8, 256), (250, -100, 3000, 256))


def _hand_frame(k):
    """Frame k of the session scene with a full-resolution group image: what is nearer than the table is a hand, the left half
    group 1, the right half group 2 (frames 0 to 2: the hands end below 500, the table begins above 570)."""
    depth, (focal, ppx, ppy) = sc.frame(k)
    hand = (depth > 0) & (depth < 500)
    groups = np.where(hand, np.where(np.arange(sc.W)[None, :] < sc.W // 2, 1, 2), 0).astype(np.uint16)
    assert (groups == 1).sum() > 2000 and (groups == 2).sum() > 2000
    return depth, groups, (focal, focal, ppx, ppy)


def _plane():
    return (np.eye(4) + 0.05 * np.random.default_rng(3).standard_normal((4, 4))).astype(np.float32)


def _pipe(rdf, stack=None, **kw):
    stack = smc.session_stack(rdf, (sc.H, sc.W), sc.forest_config(rdf)) if stack is None else stack
    intr = _hand_frame(0)[2]
    return _mod("pipeline").HandPipeline(stack, (sc.H, sc.W), sc.R, sc.W / 848, 6, [50., 8., 8., 8., 8., 8., 8.], list(TIPS), intr, _plane(),
                                         depth_mm_level=0, **kw)


def _stump_voter(rdf, **kw):
    forest = vc.all_left_stump()
    votes = np.zeros((1, 1, 2, len(STUMP_VOTES), 4), np.int32)
    votes[0, 0, 0] = STUMP_VOTES
    f = rdf.DecisionForest.from_numpy(forest)
    table = rdf.VoteTable(rdf.to_device(votes), (1, 1, 1))
    settings = dict(VOTER)
    settings.update(kw)
    return rdf.JointVoter(f, table, (sc.H, sc.W), **settings), f, table


@pytest.mark.gpu
@pytest.mark.parametrize("g_id,flip", [(1, False), (2, True)])
def test_a_voter_without_votes_changes_nothing(g_id, flip, rdf, gpu_runtime):
    depth, groups, _ = _hand_frame(0)
    f0 = sc.forest_config(rdf)[0]
    forest = rdf.DecisionForest.from_numpy(f0)
    table = rdf.VoteTable(rdf.to_device(np.zeros(f0.shape[:2] + (2, 5, 4), np.int32)), (f0.shape[0], 9, 4))
    voter = rdf.JointVoter(forest, table, (sc.H, sc.W), **VOTER)
    plain, voted = _pipe(rdf), _pipe(rdf, joint_voter=voter)
    assert plain.joint_voter is None and plain.tips is None and plain.tips_batch is None and not hasattr(plain, "_joints")
    assert voted.joint_voter is voter and voted.tip_policy == "fill" and voted.tip_joints == [0, 1, 2, 3, 4]
    dbuf, gbuf = rdf.GpuBuffer((sc.H, sc.W), np.uint16, depth), rdf.GpuBuffer((sc.H, sc.W), np.uint16, groups)
    want_m, want_h = plain.run(dbuf, gbuf, g_id, flip)
    got_m, got_h = voted.run(dbuf, gbuf, g_id, flip)
    assert np.isfinite(want_h).sum() >= 2
    assert got_m.tobytes() == want_m.tobytes() and got_h.tobytes() == want_h.tobytes()
    tips = voted.tips.get()
    assert tips.shape == (5, 4) and (tips[:, 3] <= 1).all() and np.array_equal(tips[:, 3] == 1, np.isfinite(want_h))
    assert (voted._joints.get() == (-1, -1, 0, 0)).all()
    with pytest.raises(NotImplementedError):
        voted.capture(dbuf, gbuf, g_id, flip)


@pytest.mark.gpu
@pytest.mark.parametrize("g_id,flip", [(1, False), (2, True)])
def test_votes_that_bite(g_id, flip, rdf, gpu_runtime):
    """The stump forest with a table whose every leaf votes one fixed offset per joint: under 'votes' and 'guard', means, tips
    and heights are the restatement's on the output of JointVoter.vote for the frame the forest saw.  The tips asked for include
    a class without a pixel in the frame: the label route gives NaN there, the vote a height."""
    depth, groups, intr = _hand_frame(0)
    raw = np.where(depth > 0, depth + 3, 0).astype(np.uint16)                  # heights are looked up in another frame
    dbuf, gbuf = rdf.GpuBuffer((sc.H, sc.W), np.uint16, depth), rdf.GpuBuffer((sc.H, sc.W), np.uint16, groups)
    rbuf = rdf.GpuBuffer((sc.H, sc.W), np.uint16, raw)
    probe = _mod("pipeline").HandPipeline(smc.session_stack(rdf, (sc.H, sc.W), sc.forest_config(rdf)), (sc.H, sc.W), sc.R, sc.W / 848, 6,
                                          [50., 8., 8., 8., 8., 8., 8.], list(range(1, 8)), intr, _plane(), depth_mm_level=0)
    all_m, all_h = probe.run(dbuf, gbuf, g_id, flip, height_depth=rbuf)
    absent = [c for c in range(1, 8) if np.isnan(all_m[c - 1]).any()]
    found = [c for c in range(1, 8) if np.isfinite(all_h[c - 1])]
    print(f"hand {g_id}: classes without a pixel {absent}, with a height {found}")
    assert absent and len(found) >= 4, "the scene no longer has a class without a pixel next to four with one"
    tips = found[:4] + absent[:1]
    voter, f, table = _stump_voter(rdf)
    check = voter.sibling()
    args = ((sc.H, sc.W), sc.R, sc.W / 848, 6, [50., 8., 8., 8., 8., 8., 8.], tips, intr, _plane())
    stack = smc.session_stack(rdf, (sc.H, sc.W), sc.forest_config(rdf))
    plain = _mod("pipeline").HandPipeline(stack, *args, depth_mm_level=0)
    want_m, plain_h = plain.run(dbuf, gbuf, g_id, flip, height_depth=rbuf)
    assert np.isnan(plain_h[4]) and np.isfinite(plain_h[:4]).all()
    sources = set()
    for policy, max_dist, z_tol in (("votes", 8, 30), ("guard", 8, 30), ("guard", 60, 2), ("fill", 8, 30)):
        pipe = _mod("pipeline").HandPipeline(stack, *args, depth_mm_level=0, joint_voter=voter, tip_policy=policy, tip_max_dist=max_dist,
                                             tip_z_tol=z_tol)
        # the stack serves `plain`; the voter is the first pipeline's own and serves it when the next one is built
        assert pipe.layered_rdf is not stack and (pipe.joint_voter is voter) == (policy == "votes")
        got_m, got_h = pipe.run(dbuf, gbuf, g_id, flip, height_depth=rbuf)
        assert got_m.tobytes() == want_m.tobytes()
        joints = check.vote(pipe.depth_image_2.cu(), scale_factor=sc.W / 848).get()
        _same(pipe._joints.get(), joints, "joints")
        assert (joints[0, :, 3] > 0).all()
        want_h, want_t = tn.vote_tips(got_m[None], tips, range(5), joints, int(flip), raw[None], sc.R, intr, _plane(), policy, max_dist, z_tol)
        _same(got_h, want_h[0], f"heights under {policy}")
        _same(pipe.tips.get(), want_t[0], f"tips under {policy}")
        assert np.isfinite(got_h[4]) and want_t[0, 4, 3] >= 2, policy                    # the tip the label route lost
        if policy == "fill":
            assert got_h[:4].tobytes() == plain_h[:4].tobytes() and (want_t[0, :4, 3] == 1).all()
        if policy == "votes":
            assert (want_t[0, :, 3] >= 2).all() and (got_h[:4] != plain_h[:4]).any()
        sources |= set(want_t[0, :, 3].tolist())
        voter = pipe.joint_voter            # keeps the pipeline's own alive: the next one takes a sibling again
    assert sources == {1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("soft", [False, True], ids=["mean shift", "soft modes"])
def test_a_batch_equals_its_frames(soft, rdf, gpu_runtime):
    """enqueue_batch of 3 frames with a voter whose workspace holds 2 equals three enqueue calls, bit for bit."""
    frames = [_hand_frame(k) for k in range(FRAMES)]
    cams, grps = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    raws = np.where(cams > 0, cams + 3, 0).astype(np.uint16)
    n_t, stride = len(TIPS), len(TIPS) + 2
    for g_id, flip in ((1, False), (2, True)):
        stack = smc.session_stack(rdf, (sc.H, sc.W), sc.forest_config(rdf))
        if soft:
            stack.min_conf = (0, 0)
        voter, _, _ = _stump_voter(rdf, max_frames=2)
        pipe = _pipe(rdf, stack, joint_voter=voter, tip_policy="guard", tip_max_dist=12, tip_z_tol=6, soft_modes=soft)
        dbuf, gbuf, rbuf = (rdf.GpuBuffer((sc.H, sc.W), np.uint16) for _ in range(3))
        single = []
        for k in range(FRAMES):
            dbuf.cu().set(cams[k])
            gbuf.cu().set(grps[k])
            rbuf.cu().set(raws[k])
            pipe.enqueue(dbuf, gbuf, g_id, flip, height_depth=rbuf)
            m, h = pipe._read()
            single.append((m, h, pipe.tips.get(), pipe._joints.get()))
        log = rdf.DeviceArray((FRAMES, stride), np.float64).fill(tc.SENTINEL)
        pipe.enqueue_batch(rdf.to_device(cams), rdf.to_device(grps), g_id, flip, rdf.to_device(raws), log.ptr, stride)
        log.mark_dirty()
        got_h, got_m, got_t, got_j = log.get(), pipe.means_batch.get(), pipe.tips_batch.get(), pipe.joints_batch.get()
        assert (got_h[:, n_t:] == tc.SENTINEL).all() and got_t.shape == (FRAMES, n_t, 4)
        for k in range(FRAMES):
            assert got_m[k].tobytes() == single[k][0].tobytes() and got_h[k, :n_t].tobytes() == single[k][1].tobytes(), (g_id, k)
            assert got_t[k].tobytes() == single[k][2].tobytes() and got_j[k].tobytes() == single[k][3][0].tobytes(), (g_id, k)
        assert (got_t[..., 3] >= 2).any() and len({got_t[k].tobytes() for k in range(FRAMES)}) >= 2


@pytest.mark.gpu
def test_a_session_with_joint_votes(rdf, gpu_runtime):
    """BeatsSession(joint_votes=...): the same events, heights and state from run_sequence in frame batches, frame by frame, and
    from tick; the voted heights are not the label route's."""
    from hand_state_numpy import same_state
    H, W = sc.H, sc.W
    frames, intr = sc.frames()
    frames = frames[:6]
    _, f, table = _stump_voter(rdf)

    def session(**kw):
        return rdf.BeatsSession(smc.session_stack(rdf, (H, W), sc.forest_config(rdf)), (H, W), intr, num_random_guesses=4000, seed=3,
                                max_frames=4, **kw)
    votes = dict(joint_votes=(f, table, VOTER), tip_policy="votes", tip_z_tol=12)
    a = session(**votes)
    assert a.right.joint_voter is not a.left.joint_voter and a.right.joint_voter.max_frames == a.left.joint_voter.max_frames == 4
    assert a.right.joint_voter.labels_reduce == 2 and a.right.tip_policy == a.left.tip_policy == "votes" and a.left.tip_z_tol == 12
    plane = a.calibrate(frames[0])
    dev = rdf.to_device(frames)
    ev_a, h_a = a.run_sequence(dev, batched=True)
    assert (a.right.tips_batch.get()[..., 3] >= 2).any() and (a.left.tips_batch.get()[..., 3] >= 2).any()
    b = session(**votes)
    b.set_plane(plane)
    ev_b, h_b = b.run_sequence(dev, batched=False)
    c = session(**votes)
    c.set_plane(plane)
    for k in range(len(frames)):
        c.tick(dev[k])
    ev_c = c.poll()
    assert h_a.shape == (6, 10) and np.isfinite(h_a).sum() >= 40
    assert h_b.tobytes() == h_a.tobytes() and ev_b == ev_a and ev_c == ev_a
    assert same_state(b.hand_state.state(), a.hand_state.state()) and same_state(c.hand_state.state(), a.hand_state.state())
    plain = session()
    plain.set_plane(plane)
    assert plain.right.joint_voter is None and plain.left.tips is None
    _, h_p = plain.run_sequence(dev, batched=True)
    assert h_p.tobytes() != h_a.tobytes() and np.isfinite(h_a).sum() >= np.isfinite(h_p).sum()
    with pytest.raises(NotImplementedError):
        a.right.capture(None, None, 1, False)
    with pytest.raises(ValueError):
        session(joint_votes=(f, table), fused_io=False)
    with pytest.raises(ValueError):
        session(joint_votes=(f, table, dict(max_frames=2)))
    with pytest.raises(ValueError):
        session(joint_votes=(f,))


# ------------------------------------------------------------------ GPU: a table for a saved model ---------------------------
@pytest.mark.gpu
def test_fit_votes_saved_model(rdf, gpu_runtime, tmp_path):
    """A 16-frame rendered dataset with targets: fit_votes_saved_model equals VoteFitter driven by hand on the same random
    images, and the file it saves loads into a JointVoter."""
    ds_mod, scene = _mod("dataset"), _mod("hand_scene")
    H, W, n, pick = 60, 106, 16, 12
    r = rdf.HandSceneRenderer((H, W), (75., 52.5, 29.5), max_frames=16)
    data = str(tmp_path / "hands")
    depth, labels = r.make_dataset(data, n, seed=31, plane=scene.look_down_plane(5500.), targets=True)
    assert ((labels > 0).sum(axis=(1, 2)) > 200).all()
    forest = rdf.synth.forest(3, 6, 8, "trained", 13)
    model = str(tmp_path / "forest.npy")
    np.save(model, forest)
    np.random.seed(5)
    report = ds_mod.fit_votes_saved_model(model, data, pick, str(tmp_path / "votes.npy"), min_count=4, max_var=1 << 22, radius=64, chunk=5)
    np.random.seed(5)
    ds = ds_mod.DecisionTreeDatasetConfig(data, num_images=pick, imgs_name="votes")
    assert sorted(ds.img_idxes) != ds.img_idxes                 # a shuffled subset: the targets must follow the images
    targets = ds_mod.read_targets(data, ds.img_idxes)
    f = rdf.DecisionForest.from_numpy(forest)
    idx = np.asarray(ds.img_idxes)
    want = rdf.VoteFitter(f, 5, radius=64).add(rdf.to_device(depth[idx]), rdf.to_device(labels[idx]), targets).fit(4, 1 << 22)
    assert report == want.report and report["votes"] > 0
    back = rdf.VoteTable.load(str(tmp_path / "votes.npy"))
    assert back.shape == (3, 6, 8) and back.num_joints == 5 and back.votes.get().tobytes() == want.votes.get().tobytes()
    joints = rdf.JointVoter(f, back, (H, W)).vote(rdf.to_device(depth[:2])).get()
    assert joints.shape == (2, 5, 4) and (joints[..., 3] > 0).any()
    # all images when num_images is 0
    np.random.seed(6)
    whole = ds_mod.fit_votes_saved_model(model, data, 0, str(tmp_path / "all.npy"), min_count=4, max_var=1 << 22, radius=64)
    assert whole["leaf_slots"] == report["leaf_slots"] and rdf.VoteTable.load(str(tmp_path / "all.npy")).num_joints == 5


# ------------------------------------------------------------------ CPU: do the device cases bite? --------------------------
def test_an_unchanged_copy_gives_the_same_outputs():
    import mutants
    assert mutants.same(tc.device_outputs(mutants.load("vote_tips_numpy")), tc.device_outputs(tn))


@pytest.mark.parametrize("name", list(tc.EDITS))
def test_every_wrong_reading_changes_what_the_device_test_compares(name):
    """A wrong reading of a rule that left kernel_case()'s outputs unchanged would pass the device test."""
    import mutants
    assert mutants.changed(tc.device_outputs(tc.mutant(name)), tc.device_outputs(tn)) > 0, name
