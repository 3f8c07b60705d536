"""The stereo depth sensor (librdf_labels.so: rdf_stereo_ir, rdf_stereo_sense; StereoSensor; HandSceneRenderer's sensor=)
against the restatement in tests/stereo_numpy.py.  The CPU tests pin the restatement to answers worked by hand from rules I,
N, M, W and Z of include/rdf_labels.h; every GPU comparison is bit for bit, with no pixel or case left out."""
import importlib
import inspect
import os

import numpy as np
import pytest

import hand_scene_numpy as hs
import stereo_cases as sc
import stereo_numpy as sn
from abi_helpers import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rdf_labels.h")
OUTPUTS = ("depth", "labels", "ir", "dq", "reason")


# ------------------------------------------------------------------ CPU: the restatement ------------------------------------
def test_a_fronto_parallel_plane_comes_back_exactly():
    # fb16 = 16 d Z and fbp16 = 2/5 of it: s = -(6.4 d) for the left camera and +(9.6 d) for the right, both whole sixteenths
    # of a pixel and 16 d apart, so the right image is the left one moved by exactly d columns (no IR noise)
    W, H, d, Z, D = 96, 24, 10, 4000, 32
    depth_l, labels, depth_r, cfg = sc.plane(W, H, d, Z, D, ir_noise_amp=0)
    ir = sn.ir_images(depth_l, depth_r, cfg)
    assert np.array_equal(ir[0, 1, :, :W - d], ir[0, 0, :, d:])
    assert 0.15 < (ir[0, 0] > cfg["ambient"]).mean() < 0.5                 # dots at about the default density, spread by fr
    out = sn.sense(depth_l, labels, depth_r, cfg, keep=True)
    m = out["frames"][0]
    # x >= d + 4 and the 5 x 5 box inside the image: every pixel of the box has a partner, the winner is d and the pixel valid
    box = np.zeros((H, W), bool)
    box[2:H - 2, d + 4:W - 2] = True
    assert (m["d"][box] == d).all() and (out["reason"][0][box] == 0).all() and (out["labels"][0][box] == 1).all()
    # where also every 9 x 7 window of the box lies inside BOTH images (a window that leaves one image reads 0 there and the
    # scene in the other: x - 2 - d - 4 >= 0 and x + 2 + 4 <= W - 1) the two census images agree bit for bit: C* = 0, dq = 16 d
    # and Z comes back exactly.  Rows need no such margin: both images leave the frame together
    clear = np.zeros((H, W), bool)
    clear[2:H - 2, d + 6:W - 6] = True
    assert (m["c"][clear] == 0).all() and (out["dq"][0][clear] == 16 * d).all() and (out["depth"][0][clear] == Z).all()
    assert (m["c"][2:H - 2, d + 5] != 0).any() and (m["c"][2:H - 2, W - 6] != 0).any()


def test_an_empty_frame_has_no_valid_pixel():
    # no surface: I = ambient + noise, the margin of 16 is above twice the noise, so every census is 0 and every cost of a d
    # with partners is 0: d* = 0 with C* = 0 ties with second = 0, 0 < 0 fails -> not unique.  In columns 0..3 d >= 2 has no
    # partner for part of the box, second > 0 and the pixel is unique; dq = 0 < dq_min rejects it (as every other pixel)
    W, H = 80, 20
    empty = np.full((1, H, W), 65535, np.uint16)
    for background in (empty, np.zeros_like(empty)):
        out = sn.sense(background, np.ones_like(empty), background, sn.config(16 * 100000, 16 * 40000, max_disparity=48), empty_depth=9)
        assert (out["reason"] != 0).all() and (out["depth"] == 9).all() and (out["labels"] == 0).all()
        assert (out["reason"][0, :, 4:] & sn.REASON_UNIQUE).all() and (out["reason"] & sn.REASON_DQ_MIN).all()
        assert not (out["reason"][0, 2:-2, :4] & sn.REASON_UNIQUE).any()
    # without the margin, noise alone makes matches: the margin does real work
    plain = sn.sense(empty, np.ones_like(empty), empty, sn.config(16 * 100000, 16 * 40000, max_disparity=48, census_margin=0))
    assert (plain["reason"] == 0).mean() > 0.02


def test_the_winner_is_the_lowest_of_equals_and_uniqueness_looks_two_away():
    w = sn.winners(np.array([9, 4, 7, 4, 8]))
    assert (w["d"], w["c"], w["second"], w["cm"], w["cp"]) == (1, 4, 4, 9, 7)         # d = 3 ties: the lower d wins, and is `second`
    assert not sn.is_unique(w["c"], w["second"], 10)
    w = sn.winners(np.array([9, 5, 4, 5, 8]))
    assert (w["d"], w["second"]) == (2, 8)                                          # the neighbours do not count
    assert sn.is_unique(w["c"], w["second"], 10) and sn.is_unique(w["c"], w["second"], 49) and not sn.is_unique(w["c"], w["second"], 50)
    w = sn.winners(np.array([3, 1]))
    assert (w["d"], w["second"], w["cp"]) == (1, sn.NONE, sn.NONE) and sn.is_unique(w["c"], w["second"], 100)      # no d two away
    w = sn.winners(np.array([[5, 0], [5, 0], [5, 7]]))
    assert w["d"].tolist() == [0, 0] and w["second"].tolist() == [5, 7] and w["cm"].tolist() == [sn.NONE, sn.NONE]
    assert sn.is_unique(w["c"], w["second"], 10).tolist() == [False, True]          # 0 * 100 < 7 * 90


def test_the_sub_pixel_fit_is_the_equiangular_one_floored():
    f = sn.subpixel
    assert f(10, 4, 10) == 0                    # symmetric: floor(6 / 12)
    assert f(10, 4, 7) == 4                     # den 6: floor((48 + 6) / 12) = 4   (the parabola gives 16 * 3 / 18 = 2.7)
    assert f(7, 4, 10) == -4                    # floor((-48 + 6) / 12) = floor(-3.5): the floor, not a truncation to -3
    assert f(5, 4, 10) == -7                    # floor((-80 + 6) / 12) = floor(-6.17)
    assert f(10, 4, 4) == 8 and f(4, 4, 10) == -8                   # the ends: floor(102 / 12), floor(-90 / 12) = -7.5 -> -8
    assert f(4, 4, 4) == 0                      # a flat minimum: den = 0
    assert f(10, 0, 7) == 0 and f(10, 1, 7) == 3                    # an exact match stays whole; floor((48 + 9) / 18) otherwise
    assert f(9, 4, 8) == 2 and f(8, 4, 9) == -2                     # floor(21 / 10), floor(-11 / 10) = -1.1 -> -2
    assert sn.subpixel(np.array([10, 7]), np.array([4, 4]), np.array([7, 10])).tolist() == [4, -4]
    for cm, c, cp in ((1550, 0, 0), (0, 0, 1550), (31, 30, 1550)):
        assert -8 <= f(cm, c, cp) <= 8


def test_the_right_referenced_cost_is_the_left_one_re_indexed():
    c = sc.box_case()
    cost = c["want"]["frames"][0]["cost"]
    D, H, W = cost.shape[0], cost.shape[1], sc.BOX["W"]
    right = sn.right_costs(cost, W)
    ham = sn.hamming(sn.census(c["want"]["ir"][0, 0], 16), sn.census(c["want"]["ir"][0, 1], 16), D)

    def direct(xr, y, d):           # rule M written out: the box round (xr + d, y)
        total = 0
        for j in range(-2, 3):
            for i in range(-2, 3):
                x, yy = xr + d + i, y + j
                total += int(ham[d, yy, x]) if 0 <= x < W and 0 <= yy < H else 62
        return total
    for xr, y in ((0, 0), (1, 5), (W - 1, 0), (W - 1, H - 1), (W - 2, 7), (0, H - 1), (W - 3, H - 2), (50, 0)):
        for d in (0, 1, 2, 7, D - 1):
            assert right[d, y, xr] == direct(xr, y, d), (xr, y, d)
    assert (right[D - 1, :, W - 1] == 1550).all()            # beyond the left image altogether


def test_the_band_the_right_camera_cannot_see_is_rejected_by_the_left_right_check():
    b, c = sc.BOX, sc.box_case()
    width = b["fB"] // b["Z_box"] - b["fB"] // b["Z_table"]
    assert width == 5
    reason = c["want"]["reason"][0]
    rows = slice(b["y0"] + 4, b["y1"] - 4)
    left, right = reason[rows, b["x0"] - width:b["x0"]], reason[rows, b["x1"]:b["x1"] + width]
    print(f"valid: left band {(left == 0).mean():.3f}, right band {(right == 0).mean():.3f}, frame {(reason == 0).mean():.3f}")
    assert (left == 0).mean() <= 0.25 and (right == 0).mean() >= 0.75
    assert ((left & sn.REASON_LR) != 0).mean() >= 0.75
    depth, truth = c["want"]["depth"][0].astype(np.int64), c["in"][0][0].astype(np.int64)
    inside = np.zeros_like(reason, bool)
    inside[b["y0"] + 4:b["y1"] - 4, b["x0"] + 5:b["x1"] - 5] = True
    assert (reason[inside] == 0).all() and (c["want"]["labels"][0][inside] == 3).all()
    assert np.median(np.abs(depth - truth)[inside]) < b["Z_box"] ** 2 / (4 * b["fB"])          # a quarter pixel of disparity: 44


def _erode(mask, r):
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out &= np.roll(np.roll(mask, dy, 0), dx, 1)
    out[:r], out[-r:], out[:, :r], out[:, -r:] = False, False, False, False
    return out


def test_a_hand_over_a_table_keeps_its_core_and_the_tables_interior():
    hm, scene = importlib.import_module("3d-beats_amd.hand_model"), importlib.import_module("3d-beats_amd.hand_scene")
    W, H, f, B, D = 424, 240, 212., 500., 48
    model = hm.HandModel()
    plane = scene.look_down_plane(5500.)
    t = model.part_transforms(model.rest_pose((0., -300., 800.))[None], np.linalg.inv(plane))
    table = scene.table_of_plane(plane).astype(np.float64)
    right_t = t.astype(np.float64)
    right_t[:, :, 3] -= B
    right_table = table.copy()
    right_table[3] -= right_table[0] * B
    tri_label = hm.HandModel.label_table("fine")[model.tri_part]
    cam = (f, (W - 1) / 2., (H - 1) / 2.)
    mesh = (model.verts, model.vert_part, model.tris, tri_label)
    depth_l, labels_l, info = hs.render(W, H, *mesh, t, table[None].astype(np.float32), *cam)
    depth_r, _, _ = hs.render(W, H, *mesh, right_t.astype(np.float32), right_table[None].astype(np.float32), *cam)
    cfg = sn.config(round(16 * f * B), round(16 * f * B * 0.4), max_disparity=D)
    out = sn.sense(depth_l, labels_l, depth_r, cfg)
    valid, err = out["reason"][0] == 0, np.abs(out["depth"][0].astype(np.int64) - depth_l[0])
    hand = labels_l[0] > 0
    core = _erode(hand, 3)
    interior = _erode(~hand, 12)                # the table, clear of the hand, its shadow and the matching windows ...
    interior[:, :D] = False                     # ... and of the columns whose partners lie beyond the right image
    interior[:8], interior[-8:], interior[:, -8:] = False, False, False
    assert core.sum() > 1000 and interior.sum() > 40000
    z_hand = float(np.median(depth_l[0][core]))
    print(f"hand core: {valid[core].mean():.4f} valid, median error {np.median(err[core & valid])}, p99 {np.percentile(err[core & valid], 99)}"
          f" (bound {z_hand ** 2 / (4 * f * B):.1f}); table interior: {valid[interior].mean():.4f} valid, median error "
          f"{np.median(err[interior & valid])} (bound {5500. ** 2 / (4 * f * B):.1f}); frame {valid.mean():.4f} valid")
    assert valid[core].all()
    assert np.median(err[core]) < z_hand ** 2 / (4 * f * B)
    assert np.median(err[interior & valid]) < 5500. ** 2 / (4 * f * B) and 71 < 5500. ** 2 / (4 * f * B) < 72
    assert (out["labels"][0][core] == labels_l[0][core]).all()


# ------------------------------------------------------------------ CPU: the interface --------------------------------------
def _config(_lib, cfg):
    return _lib.StereoConfig(**cfg)


def test_the_entry_points_reject_bad_and_null_arguments(rdf):
    _lib = importlib.import_module("3d-beats_amd._lib")
    importlib.import_module("3d-beats_amd._build").build()
    names = declared(HEADER)
    for must in ("rdf_stereo_workspace_bytes", "rdf_stereo_ir", "rdf_stereo_sense"):
        assert must in names
    lib = _lib.load("labels")
    assert lib.rdf_labels_abi_version() == 1
    ws = lib.rdf_stereo_workspace_bytes
    assert ws(64, 848, 480, 128) == 64 * 848 * 480 * 21 and ws(1, 33, 17, 1) == 33 * 17 * 21
    assert ws(0, 4, 4, 8) == 0 and ws(1, -1, 4, 8) == 0 and ws(1, 32769, 4, 8) == 0 and ws(1, 4, 4, 0) == 0 and ws(1, 4, 4, 257) == 0
    good = sn.config(16 * 1000, 16 * 400, max_disparity=8)

    def sense(n=1, W=4, H=4, ptrs=(64, 128, 192, 256, 320, 384), **kw):
        p = list(ptrs)
        return lib.rdf_stereo_sense(n, W, H, p[0], p[1], p[2], _config(_lib, dict(good, **kw)), 0, 0, p[3], p[4], p[5], None, None,
                                    None, None)

    def ir(n=1, W=4, H=4, ptrs=(64, 128, 192), **kw):
        return lib.rdf_stereo_ir(n, W, H, ptrs[0], ptrs[1], _config(_lib, dict(good, **kw)), 0, ptrs[2], None)
    # rejected arguments launch nothing, so they can be checked without a device
    for call in (sense, ir):
        assert call(n=0) == -1 and call(W=-1) == -1 and call(H=-1) == -1 and call(H=40000) == -3
        assert call(n=1 << 21, W=1 << 9, H=1 << 9) == -3                    # 2^39 pixels
        assert call(max_disparity=0) == -1 and call(max_disparity=257) == -1 and call(fbp16=-1) == -1 and call(fbp16=16001) == -1
        assert call(fb16=(1 << 31) - (1 << 15)) == -1 and call(ambient=256) == -1 and call(ir_noise_amp=-1) == -1
        assert call(census_margin=256) == -1 and call(uniqueness=101) == -1 and call(lr_max=-1) == -1 and call(dq_min=0) == -1
        assert call(W=0) == 0 and call(H=0) == 0                            # no pixels: nothing to do
    for k in range(6):
        assert sense(ptrs=[None if j == k else 64 * (j + 1) for j in range(6)]) == -2, k
    for k in range(3):
        assert ir(ptrs=[None if j == k else 64 * (j + 1) for j in range(3)]) == -2, k
    assert sense(ptrs=(65, 128, 192, 256, 320, 384)) == -1 and sense(ptrs=(64, 128, 192, 260, 320, 384)) == -1     # misaligned
    assert sense(ptrs=(64, 128, 192, 256, 320, 320)) == -1                  # one buffer for both images


def test_the_new_names_are_public(rdf):
    assert "StereoSensor" in rdf.__all__ and callable(rdf.StereoSensor.sense)
    p = inspect.signature(rdf.StereoSensor.__init__).parameters
    got = {k: p[k].default for k in ("baseline_mm", "projector_offset", "max_disparity", "dot_density", "ambient", "ir_noise_amp",
                                     "census_margin", "uniqueness", "lr_max", "dq_min", "units_per_mm", "max_frames")}
    assert got == {"baseline_mm": 50., "projector_offset": 0.4, "max_disparity": 128, "dot_density": 0.25, "ambient": 16,
                   "ir_noise_amp": 6, "census_margin": 16, "uniqueness": 10, "lr_max": 1, "dq_min": 16, "units_per_mm": 10.,
                   "max_frames": 64}
    p = inspect.signature(rdf.StereoSensor.sense).parameters
    assert [k for k in p][1:] == ["depth_l", "labels_l", "depth_r", "seed", "empty_depth", "depth_out", "labels_out", "ir_out",
                                  "dq_out", "reason_out"]
    assert (p["seed"].default, p["empty_depth"].default) == (0, 65535)
    for name in ("render", "make_dataset", "camera_sequence"):
        assert inspect.signature(getattr(rdf.HandSceneRenderer, name)).parameters["sensor"].default is None
    # the restatement's defaults are the sensor's
    assert sn.DEFAULTS["dot_threshold"] == int(0.25 * 2 ** 32)
    assert sn.DEFAULTS["pattern_seed"] == importlib.import_module("3d-beats_amd.stereo_sensor").PATTERN_SEED


# ------------------------------------------------------------------ GPU -----------------------------------------------------
def _sense_raw(rdf, arrays, cfg, seed, empty, outputs=OUTPUTS, frames=None):
    """rdf_stereo_sense on host arrays: {name: host array} of the outputs asked for, each pre-filled with 7."""
    _lib = importlib.import_module("3d-beats_amd._lib")
    lib = _lib.load("labels")
    N, H, W = arrays[0].shape
    dev = [rdf.to_device(np.ascontiguousarray(a)) for a in arrays]
    ws = rdf.DeviceArray((max(int(lib.rdf_stereo_workspace_bytes(frames or N, W, H, cfg["max_disparity"])), 8),), np.uint8)
    shape = {"depth": ((N, H, W), np.uint16), "labels": ((N, H, W), np.uint16), "ir": ((N, 2, H, W), np.uint8),
             "dq": ((N, H, W), np.uint16), "reason": ((N, H, W), np.uint8)}
    out = {k: rdf.DeviceArray(*shape[k]).fill(7) for k in outputs}
    rc = lib.rdf_stereo_sense(N, W, H, dev[0].ptr, dev[1].ptr, dev[2].ptr, _config(_lib, cfg), seed, empty, ws.ptr, out["depth"].ptr,
                              out["labels"].ptr, *(out[k].ptr if k in out else None for k in ("ir", "dq", "reason")),
                              rdf.get_runtime().stream())
    return rc, {k: v.get() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.GPU_SHAPES))
def test_the_device_matches_the_restatement_bit_for_bit(name, rdf, gpu_runtime):
    _lib = importlib.import_module("3d-beats_amd._lib")
    lib = _lib.load("labels")
    c = sc.gpu_case(name)
    want = c["want"]
    N, H, W = c["in"][0].shape
    # rule I on its own
    dl, dr = rdf.to_device(c["in"][0]), rdf.to_device(c["in"][2])
    ir = rdf.DeviceArray((N, 2, H, W), np.uint8).fill(7)
    _lib.check(lib, lib.rdf_stereo_ir(N, W, H, dl.ptr, dr.ptr, _config(_lib, c["cfg"]), sc.SEED, ir.ptr, gpu_runtime.stream()),
               "rdf_stereo_ir")
    assert np.array_equal(ir.get(), want["ir"])
    # the whole chain with every optional output, and with none
    rc, got = _sense_raw(rdf, c["in"], c["cfg"], sc.SEED, sc.EMPTY)
    assert rc == 0
    bad = {k: int((got[k] != want[k]).sum()) for k in OUTPUTS}
    print(f"{name}: {W}x{H} x {N}, D {c['cfg']['max_disparity']}: {int((want['reason'] == 0).sum())} of {N * H * W} valid, "
          f"reasons {np.bincount(want['reason'].reshape(-1), minlength=8).tolist()}, differing {bad}")
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
    rc, bare = _sense_raw(rdf, c["in"], c["cfg"], sc.SEED, sc.EMPTY, outputs=("depth", "labels"))
    assert rc == 0 and np.array_equal(bare["depth"], want["depth"]) and np.array_equal(bare["labels"], want["labels"])


def test_the_column_0_case_holds_a_winner_left_of_the_right_image():
    """x - d* == -1 at one pixel that is unique and has dq >= dq_min: it fails for the left-right check's first clause alone,
    and a reading that accepts x - d* == -1 (comparing dR at the clamped column, within lr_max = 255) would show it."""
    import mutants
    c = sc.column0_case()
    y, x = sc.COLUMN0_PIXEL
    frame, want = c["want"]["frames"][0], c["want"]
    assert c["in"][0].shape == (1, 5, 9) and x == 0 and frame["d"][y, x] == 1 and x - frame["d"][y, x] == -1
    assert want["reason"][0, y, x] == sn.REASON_LR and want["depth"][0, y, x] == sc.EMPTY and want["labels"][0, y, x] == 0
    assert want["dq"][0, y, x] >= c["cfg"]["dq_min"] and (want["reason"] == 0).sum() > 20
    loose = mutants.load("stereo_numpy", [("lr = (xr >= 0) &", "lr = (xr >= -1) &")])
    got = loose.sense(*c["in"], c["cfg"], seed=sc.SEED, empty_depth=sc.EMPTY)
    differ = {k: np.argwhere(got[k] != want[k]).tolist() for k in ("depth", "labels", "dq", "reason")}
    assert differ == {"depth": [[0, y, x]], "labels": [[0, y, x]], "dq": [], "reason": [[0, y, x]]}
    assert got["reason"][0, y, x] == 0 and got["labels"][0, y, x] == 3
    # and no other device case of the sensor tells the two readings apart
    for name in sc.GPU_SHAPES:
        g = sc.gpu_case(name)
        other = loose.sense(*g["in"], g["cfg"], seed=sc.SEED, empty_depth=sc.EMPTY)
        assert all(np.array_equal(other[k], g["want"][k]) for k in ("depth", "labels", "dq", "reason")), name


@pytest.mark.gpu
def test_a_winner_left_of_the_right_image_fails_the_left_right_check(rdf, gpu_runtime):
    c = sc.column0_case()
    want = c["want"]
    y, x = sc.COLUMN0_PIXEL
    rc, got = _sense_raw(rdf, c["in"], c["cfg"], sc.SEED, sc.EMPTY)
    assert rc == 0
    print(f"pixel ({x}, {y}): dq {int(got['dq'][0, y, x])}, reason {int(got['reason'][0, y, x])}, depth {int(got['depth'][0, y, x])}; "
          f"differing {({k: int((got[k] != want[k]).sum()) for k in OUTPUTS})}")
    assert got["reason"][0, y, x] == sn.REASON_LR and got["depth"][0, y, x] == sc.EMPTY and got["labels"][0, y, x] == 0
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k


def test_the_gpu_cases_decide_something():
    """The shapes of the GPU comparison reach valid and invalid pixels of every kind, and their frames differ."""
    seen = np.zeros(8, np.int64)
    for name in sc.GPU_SHAPES:
        seen += np.bincount(sc.gpu_case(name)["want"]["reason"].reshape(-1), minlength=8)
    assert seen[0] > 3000 and (seen[[1, 2, 4]] > 0).all() and seen[1:].sum() > 3000
    want = sc.gpu_case("three frames, no multiple of any tile")["want"]
    assert not np.array_equal(want["depth"][0], want["depth"][1]) and not np.array_equal(want["depth"][1], want["depth"][2])
    near = sc.gpu_case("several tiles, a surface nearer than fB / D")
    assert ((near["in"][1] == 9) & (near["want"]["reason"] != 0)).sum() > 20


def test_the_many_frames_case_reaches_the_frame_loops_and_its_frames_differ():
    c = sc.many_frames_case()
    N, p = sc.MANY_N, sc.MANY_PERIOD
    assert N > sc.MANY_PLANES and 2 * N > sc.MANY_PLANES and N - sc.MANY_PLANES == 6        # frames and images both wrap
    assert sc.MANY_PLANES % p == 1 and len(c["index"]) == N and c["index"][sc.MANY_PLANES] == 1 and c["index"][-1] == (N - 1) % p
    assert c["cfg"]["ir_noise_amp"] == 0 and c["cfg_ir"]["ir_noise_amp"] == 6 and sc.MANY_IR_SEED != 0
    want = c["want"]
    assert want["depth"].shape == (p, sc.MANY_H, sc.MANY_W)
    for a in range(p):
        for b in range(a + 1, p):
            assert not np.array_equal(want["depth"][a], want["depth"][b]), (a, b)
            assert not np.array_equal(want["reason"][a], want["reason"][b]), (a, b)
            assert not np.array_equal(want["ir"][a], want["ir"][b]) and not np.array_equal(want["dq"][a], want["dq"][b]), (a, b)
    assert (want["reason"] == 0).sum() > 50 and (want["labels"] > 0).any()
    for bit in (sn.REASON_UNIQUE, sn.REASON_LR, sn.REASON_DQ_MIN):
        assert (want["reason"] & bit).any(), bit
    # without noise a frame does not depend on its index: the restated sense of frames 65535.. is that of frames 1..
    cfg = c["cfg"]
    for k in range(p):
        for camera in (0, 1):
            depth = c["distinct"][2 * camera][k]
            assert np.array_equal(sn.ir_image(depth, camera, k + p * 9362, cfg, sc.SEED), want["ir"][k, camera])
    # with noise it does: the frames rdf_stereo_ir is compared on differ although their depth repeats
    ir = c["want_ir"]
    assert sorted(ir) == [0, 1, 65534, 65535, 65536, N - 1] and 65535 % p == 1 and not np.array_equal(ir[1], ir[65535])
    assert all(not np.array_equal(ir[n], want["ir"][n % p]) for n in ir)


def test_the_config_variants_do_what_their_names_say():
    base = sc.variant_case()
    assert base["cfg"] == dict(sn.DEFAULTS, fb16=base["cfg"]["fb16"], fbp16=base["cfg"]["fbp16"], max_disparity=24,
                               pattern_seed=base["cfg"]["pattern_seed"])
    print(f"base: reasons {np.bincount(base['want']['reason'].reshape(-1), minlength=8).tolist()}")
    x = np.arange(sc.VARIANT_SHAPE[0])[None, :]
    for name, over in sc.CONFIG_VARIANTS.items():
        v = sc.variant_case(name)
        assert all(v["cfg"][k] == over[k] for k in over) and all(v["cfg"][k] == base["cfg"][k] for k in base["cfg"] if k not in over)
        differing = [k for k in OUTPUTS if not np.array_equal(v["want"][k], base["want"][k])]
        print(f"{name}: {int((v['want']['reason'] == 0).sum())} valid, reasons "
              f"{np.bincount(v['want']['reason'].reshape(-1), minlength=8).tolist()}, differs from the base in {differing}")
        assert differing, name
    want = {name: sc.variant_case(name)["want"] for name in sc.CONFIG_VARIANTS}
    # uniqueness 0: best * 100 < second * 100 wherever C* < second; uniqueness 100: best * 100 < 0 never, and every pixel of a
    # D = 24 frame has a d two away
    for m, reason in zip(want["uniqueness 0"]["frames"], want["uniqueness 0"]["reason"]):
        strictly = (m["second"] != sn.NONE) & (m["c"] < m["second"])
        assert strictly.sum() > 500 and not (reason[strictly] & sn.REASON_UNIQUE).any()
        assert (reason[m["c"] == m["second"]] & sn.REASON_UNIQUE).all()          # a tie is still not unique
    assert any((m["c"] == m["second"]).any() for m in want["uniqueness 0"]["frames"])
    assert all((m["second"] != sn.NONE).all() for m in want["uniqueness 100"]["frames"])
    assert (want["uniqueness 100"]["reason"] & sn.REASON_UNIQUE).all() and not (want["uniqueness 100"]["reason"] == 0).any()
    assert 0 < (want["uniqueness 50"]["reason"] == 0).sum() < (base["want"]["reason"] == 0).sum()
    # lr_max 255: |dR - d| <= 255 always, so only a partner left of the image fails; lr_max 0 rejects more than 1 does
    for m, reason in zip(want["lr_max 255"]["frames"], want["lr_max 255"]["reason"]):
        assert np.array_equal((reason & sn.REASON_LR) != 0, x - m["d"] < 0) and (x - m["d"] >= 0).sum() > 500
        assert (np.abs(np.take_along_axis(m["dR"], np.maximum(x - m["d"], 0), 1) - m["d"]) > 1).any()      # lr_max 1 rejects here
    assert((want["lr_max 0"]["reason"] & sn.REASON_LR) != 0).sum() > ((base["want"]["reason"] & sn.REASON_LR) != 0).sum()
    # dq_min
    assert (want["dq_min 65535"]["reason"] & sn.REASON_DQ_MIN).all() and (want["dq_min 200"]["reason"] & sn.REASON_DQ_MIN).all()
    assert not (want["dq_min 1"]["reason"][want["dq_min 1"]["dq"] >= 1] & sn.REASON_DQ_MIN).any()
    assert ((want["dq_min 1"]["dq"] >= 1) & (want["dq_min 1"]["dq"] < 16)).any() and (want["dq_min 1"]["dq"] == 0).any()
    # a margin of 255 and no dots (ambient and noise alone, below the default margin) empty every census
    for name in ("census_margin 255", "dot_threshold 0"):
        margin = sc.variant_case(name)["cfg"]["census_margin"]
        assert not any(sn.census(image, margin).any() for frame in want[name]["ir"] for image in frame), name
        assert not (want[name]["reason"] == 0).any(), name
    assert any(sn.census(image, 16).any() for frame in base["want"]["ir"] for image in frame)
    assert want["dot_threshold 0"]["ir"].min() >= 16 - 6 and want["dot_threshold 0"]["ir"].max() <= 16 + 6
    surface = np.stack([(d > 0) & (d < 65535) for d in (base["in"][0], base["in"][2])], 1)
    everywhere, nowhere = want["dot_threshold 0xFFFFFFFF"]["ir"].astype(int), want["dot_threshold 0"]["ir"].astype(int)
    assert (everywhere[surface] - nowhere[surface] >= 64).all() and np.array_equal(everywhere[~surface], nowhere[~surface])
    # the clamp at 255: the base's IR image is nowhere clamped (10 <= 16 + dots + noise <= 16 + 191 + 6), so ambient 255 is the
    # base moved up by 239 and cut off.  A surface pixel is 255 unless it has no dot to outweigh a negative noise draw (the
    # noise keeps its default of 6 in this row, so 249 is the least)
    assert base["want"]["ir"].max() <= 16 + 191 + 6 and base["want"]["ir"].min() >= 16 - 6
    bright = want["ambient 255"]["ir"]
    assert np.array_equal(bright, np.minimum(base["want"]["ir"].astype(int) + 239, 255))
    assert (bright[surface & (base["want"]["ir"] >= 16)] == 255).all() and (bright[surface] == 255).mean() > 0.5 and bright.min() == 249
    # the clamp at 0 and at 255 in one image
    wild = want["ambient 0, ir_noise_amp 255"]["ir"]
    assert (wild == 0).sum() > 1000 and (wild == 255).sum() > 100 and ((wild > 0) & (wild < 255)).any()
    quiet = want["ir_noise_amp 0"]["ir"]
    assert (quiet[~surface] == 16).all() and np.abs(quiet.astype(int) - base["want"]["ir"]).max() == 6
    # the numeric limit: valid pixels, all at the clamp of rule Z, and columns at Z = 1, 2, 3 and 65534
    for name in sc.LIMIT_VARIANTS:
        v = sc.variant_case(name)
        valid = v["want"]["reason"] == 0
        assert valid.sum() > 100 and (v["want"]["depth"][valid] == 65534).all(), name
        assert v["cfg"]["fb16"] == 2 ** 31 - 2 ** 15 - 1 and v["cfg"]["fb16"] + 32767 == 2 ** 31 - 2         # the numerator's limit
        assert (v["in"][0][:, :, 10] == 1).all() and (v["in"][0][:, :, 30] == 2).all()
        assert (v["in"][2][:, :, 20] == 3).all() and (v["in"][2][:, :, 50] == 65534).all()
    assert sc.variant_case(sc.LIMIT_VARIANTS[0])["cfg"]["fbp16"] == 0
    assert sc.variant_case(sc.LIMIT_VARIANTS[1])["cfg"]["fbp16"] == sc.FB16_MAX


@pytest.mark.gpu
def test_more_frames_than_the_grid_has_planes_match_the_restatement_bit_for_bit(rdf, gpu_runtime):
    _lib = importlib.import_module("3d-beats_amd._lib")
    lib = _lib.load("labels")
    c = sc.many_frames_case()
    N, H, W = sc.MANY_N, sc.MANY_H, sc.MANY_W
    arrays = [np.take(a, c["index"], axis=0) for a in c["distinct"]]
    rc, got = _sense_raw(rdf, arrays, c["cfg"], sc.SEED, sc.EMPTY)
    assert rc == 0
    for k in OUTPUTS:
        want = np.take(c["want"][k], c["index"], axis=0)
        wrong = np.nonzero((got[k] != want).reshape(N, -1).any(1))[0]
        print(f"{k}: {len(wrong)} of {N} frames differ" + (f", the first {wrong[:8].tolist()}" if len(wrong) else ""))
        assert got[k].shape == want.shape and np.array_equal(got[k], want), k
    # rule I's per-frame hash at large n: the default noise, on its own
    dl, dr = rdf.to_device(arrays[0]), rdf.to_device(arrays[2])
    ir = rdf.DeviceArray((N, 2, H, W), np.uint8).fill(7)
    _lib.check(lib, lib.rdf_stereo_ir(N, W, H, dl.ptr, dr.ptr, _config(_lib, c["cfg_ir"]), sc.MANY_IR_SEED, ir.ptr,
                                      gpu_runtime.stream()), "rdf_stereo_ir")
    ir = ir.get()
    for n in sc.MANY_IR_FRAMES:
        assert np.array_equal(ir[n], c["want_ir"][n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.CONFIG_VARIANTS))
def test_every_config_field_matches_the_restatement_bit_for_bit(name, rdf, gpu_runtime):
    _lib = importlib.import_module("3d-beats_amd._lib")
    lib = _lib.load("labels")
    c = sc.variant_case(name)
    want = c["want"]
    N, H, W = c["in"][0].shape
    dl, dr = rdf.to_device(c["in"][0]), rdf.to_device(c["in"][2])
    ir = rdf.DeviceArray((N, 2, H, W), np.uint8).fill(7)
    _lib.check(lib, lib.rdf_stereo_ir(N, W, H, dl.ptr, dr.ptr, _config(_lib, c["cfg"]), sc.SEED, ir.ptr, gpu_runtime.stream()),
               "rdf_stereo_ir")
    assert np.array_equal(ir.get(), want["ir"])
    rc, got = _sense_raw(rdf, c["in"], c["cfg"], sc.SEED, sc.EMPTY)
    assert rc == 0
    bad = {k: int((got[k] != want[k]).sum()) for k in OUTPUTS}
    print(f"{name}: {int((want['reason'] == 0).sum())} of {N * H * W} valid, reasons "
          f"{np.bincount(want['reason'].reshape(-1), minlength=8).tolist()}, differing {bad}")
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.gpu
def test_rejected_arguments_leave_the_outputs_untouched(rdf, gpu_runtime):
    c = sc.gpu_case("D = 2")
    for cfg, arrays, code in ((dict(c["cfg"], max_disparity=0), c["in"], -1), (dict(c["cfg"], dq_min=0), c["in"], -1)):
        rc, got = _sense_raw(rdf, arrays, cfg, sc.SEED, sc.EMPTY, frames=1)
        assert rc == code and all((v == 7).all() for v in got.values())


@pytest.mark.gpu
def test_chunks_of_max_frames_give_the_frames_of_one_call(rdf, gpu_runtime):
    W, H, N, D = 67, 9, 5, 24
    depth_l, labels, depth_r, cfg = sc.layered(W, H, N, D, 41)
    want = sn.sense(depth_l, labels, depth_r, cfg, seed=5, empty_depth=0)
    fB = cfg["fb16"] / 16.
    s = rdf.StereoSensor((H, W), (fB / 500., 0., 0.), max_disparity=D, pattern_seed=cfg["pattern_seed"], max_frames=2)
    assert s.config_dict() == cfg
    dev = [rdf.to_device(a) for a in (depth_l, labels, depth_r)]
    outs = {"ir_out": rdf.DeviceArray((N, 2, H, W), np.uint8), "dq_out": rdf.DeviceArray((N, H, W), np.uint16),
            "reason_out": rdf.DeviceArray((N, H, W), np.uint8)}
    depth, lab = s.sense(*dev, seed=5, empty_depth=0, **outs)
    got = {"depth": depth.get(), "labels": lab.get(), "ir": outs["ir_out"].get(), "dq": outs["dq_out"].get(),
           "reason": outs["reason_out"].get()}
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
    d, l = rdf.DeviceArray((N, H, W), np.uint16).fill(3), rdf.DeviceArray((N, H, W), np.uint16).fill(3)
    back = s.sense(*dev, seed=5, empty_depth=0, depth_out=d, labels_out=l)
    assert back[0] is d and back[1] is l and np.array_equal(d.get(), want["depth"]) and np.array_equal(l.get(), want["labels"])


def _renderer_scene(rdf):
    hm, scene = importlib.import_module("3d-beats_amd.hand_model"), importlib.import_module("3d-beats_amd.hand_scene")
    W, H, D = 106, 60, 24
    cam = (53., (W - 1) / 2., (H - 1) / 2.)
    r = rdf.HandSceneRenderer((H, W), cam, max_frames=2)
    s = rdf.StereoSensor((H, W), cam, max_disparity=D, max_frames=2)
    plane = scene.look_down_plane(5500.)
    poses = r.model.press_sequence(3, "index", wrist=(0., -300., 800.), speed_mm=10.)
    return hm, scene, r, s, plane, poses


def _restated(r, s, t, table, labels, seed, empty):
    W, H = r.DIM_X, r.DIM_Y
    N = len(t)
    right = t.astype(np.float64)
    right[:, :, 3] -= s.baseline
    tables = right_tables = None
    if table is not None:
        tables = np.tile(np.asarray(table, np.float32), (N, 1))
        right_tables = tables.astype(np.float64)
        right_tables[:, 3] -= right_tables[:, 0] * s.baseline
        right_tables = right_tables.astype(np.float32)
    mesh = (r.model.verts, r.model.vert_part, r.model.tris, r.tri_labels(16, labels))
    dl, ll, _ = hs.render(W, H, *mesh, t, tables, r.f, r.ppx, r.ppy, empty_depth=empty)
    dr, _, _ = hs.render(W, H, *mesh, right.astype(np.float32), right_tables, r.f, r.ppx, r.ppy, empty_depth=empty)
    return sn.sense(dl, ll, dr, s.config_dict(), seed=seed, empty_depth=empty)


@pytest.mark.gpu
def test_the_renderers_three_paths_go_through_the_sensor(rdf, gpu_runtime, tmp_path):
    hm, scene, r, s, plane, poses = _renderer_scene(rdf)
    t, table = r.transforms(poses, plane), scene.table_of_plane(plane)
    # render
    want = _restated(r, s, t, table, "coarse", 11, 0)
    depth, lab = r.render(t, "coarse", table, 0, 11, sensor=s)
    assert np.array_equal(depth.get(), want["depth"]) and np.array_equal(lab.get(), want["labels"])
    valid = want["reason"] == 0
    assert 0.5 < valid.mean() < 1. and (want["labels"] > 0).sum() > 100
    # camera_sequence: raw frames over the table, empty pixels 0, and the truth labels of what is left
    truth = rdf.DeviceArray((3,) + depth.shape[1:], np.uint16)
    frames = r.camera_sequence(poses, plane, seed=4, labels_out=truth, sensor=s)
    want = _restated(r, s, t, table, "fine", 4, 0)
    assert np.array_equal(frames.get(), want["depth"]) and np.array_equal(truth.get(), want["labels"])
    # make_dataset: no table, background 65535, and a directory the dataset reader takes
    ds_mod = importlib.import_module("3d-beats_amd.dataset")
    depth, lab = r.make_dataset(str(tmp_path / "sensed"), 3, seed=8, sensor=s)
    sampled = r.model.sample_poses(3, np.random.default_rng(8))
    want = _restated(r, s, r.transforms(sampled, scene.look_down_plane(5500.)), None, "fine", 8, 65535)
    assert np.array_equal(depth, want["depth"]) and np.array_equal(lab, want["labels"])
    assert ((lab == 0) | (depth != 65535)).all() and (lab > 0).sum() > 100
    cfg = ds_mod.DecisionTreeDatasetConfig(str(tmp_path / "sensed"))
    assert cfg.img_dims == (r.DIM_X, r.DIM_Y) and cfg.total_available_images == 3
    # the sensor replaces rule H
    for kw in ({"hole_rate": 0.1}, {"noise_amp": 3}):
        with pytest.raises(ValueError):
            r.render(t, "fine", table, 0, 0, sensor=s, **kw)


@pytest.mark.gpu
def test_without_a_sensor_nothing_changes(rdf, gpu_runtime):
    hm, scene, r, s, plane, poses = _renderer_scene(rdf)
    t, table = r.transforms(poses, plane), scene.table_of_plane(plane)
    a, b = r.render(t, "fine", table, 0, 9, 0.1, 5), r.render(t, "fine", table, 0, 9, 0.1, 5, sensor=None)
    assert a[0].get().tobytes() == b[0].get().tobytes() and a[1].get().tobytes() == b[1].get().tobytes()
    a = r.camera_sequence(poses, plane, hole_rate=0.1, noise_amp=5, seed=2)
    b = r.camera_sequence(poses, plane, hole_rate=0.1, noise_amp=5, seed=2, sensor=None)
    assert a.get().tobytes() == b.get().tobytes()
