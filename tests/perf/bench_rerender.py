#!/usr/bin/env python3
"""Times the converter's re-render (librdf_labels.so: rdf_points_center + rdf_rerender) on one 848x480 synthetic hand scene
-- the tilted table with two raised hands of tests/test_frontend.py, the hands painted in glove colours -- and, beside it,
the converter's other per-frame device steps.  Prints one JSON line (hipEvent times between two events on the stream,
medians after warm-up, 20 repetitions per sample):
  center_us          one rdf_points_center over the frame's points in plane space
  rerender_us        one rdf_rerender (raster + resolve) with a transform of the converter's default variance (scale 1.1)
  rerender_identity_us   the same with the identity (frames 1 and 2)
  augment_us         center + rerender as the converter issues them
  other_steps_us     what RecordingConverter.tick() launches besides: clear + deproject_points, transform_points into the
                     plane, filter_points_by_plane, transform_points back, clear + depths_from_points, label_frame (K = 4)
  rerender_share     augment_us / (augment_us + other_steps_us)
Uploads, the plane fit (first and every 20th frame), the colour mapping (first frame) and the PNG encoder are in neither.
The re-rendered images are checked against the restatement on a 212x120 copy of the scene first.  `--out FILE` also writes
the JSON there.  Standalone: bench.py does not run it."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, K, T, REPS = 480, 848, 4, 40., 20
PALETTE = np.array([[220, 40, 40], [40, 200, 60], [50, 60, 230], [230, 220, 50]], np.uint8)


def _events(torch, fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def _frame(h, w):
    """(depth, colour, (f, ppx, ppy), plane) of the hand scene at h x w."""
    import frontend_numpy as fnp
    from test_frontend import scene
    depth, hand, fpp = scene(h, w, w / 2., tilt_deg=18., box_h=80., holes=0.02, seed=40, hand_scale=1.5)
    rng = np.random.default_rng(900)
    stripe = np.arange(w)[None, :] * K // w
    color = np.clip(PALETTE.astype(np.int64)[np.broadcast_to(stripe, (h, w))] + rng.integers(-8, 9, (h, w, 3)), 0, 255)
    color[~hand] = 0
    f, ppx, ppy = (np.float32(v) for v in fpp)
    rand = np.random.default_rng(1).random((2000, 32), dtype=np.float32)
    plane, _, _, _, status = fnp.calibrate(rand, fnp.deproject(depth, ppx, ppy, f), w, h, T)[:5]
    assert status == 0
    return depth, color.astype(np.uint8), (f, ppx, ppy), plane.reshape(4, 4)


def _check(rdf):
    """The device's images on a small copy of the scene equal the restatement's."""
    import frontend_numpy as fnp
    import rerender_numpy as rn
    h, w = 120, 212
    depth, color, (f, ppx, ppy), plane = _frame(h, w)
    in_plane = fnp.filter_by_plane(fnp.transform(fnp.deproject(depth, ppx, ppy, f), plane), T)
    s = rn.center_sums(in_plane)
    M = rdf.SceneRerender.make_transform(plane, s[:3] / s[3], 1.1)
    pts = fnp.transform(in_plane, np.linalg.inv(plane))
    rr = rdf.SceneRerender((h, w), (f, ppx, ppy))
    d, c = rdf.DeviceArray((h, w), np.uint16), rdf.DeviceArray((h, w, 3), np.uint8)
    rr.run(rdf.to_device(pts), rdf.to_device(color), M, d, c)
    want_d, want_c, _ = rn.rerender(pts, color, M, f, ppx, ppy)
    assert np.array_equal(d.get(), want_d) and np.array_equal(c.get(), want_c)
    return int((want_d > 0).sum())


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    po = importlib.import_module("3d-beats_amd.cuda.points_ops").PointsOps()
    torch.cuda.set_device(0)
    out = {"frame": [H, W], "checked_pixels_212x120": _check(rdf)}

    depth_np, color_np, (f, ppx, ppy), plane = _frame(H, W)
    inv_plane = np.linalg.inv(plane)
    n_px = H * W
    dims = np.array([1, W, H, -1], np.int32)
    pp = np.array([ppx, ppy], np.float32)
    depth_in = rdf.to_device(depth_np.reshape(1, H, W))
    depth = rdf.DeviceArray((1, H, W), np.uint16)
    pts = rdf.DeviceArray((H, W, 4), np.float32)
    color_in = rdf.to_device(color_np)
    color = rdf.DeviceArray((H, W, 3), np.uint8)
    depth_rr, color_rr = rdf.DeviceArray((1, H, W), np.uint16), rdf.DeviceArray((H, W, 3), np.uint8)
    labels, rgba = rdf.DeviceArray((H, W), np.uint16), rdf.DeviceArray((H, W, 4), np.uint8)
    lab = rdf.ColorLabeler(K)
    lab.set_color_mapping(PALETTE)
    rr = rdf.SceneRerender((H, W), (f, ppx, ppy))

    def to_plane():
        pts.fill(0)
        po.deproject_points(dims, pp, f, depth_in, pts)
        po.transform_points(n_px, pts, plane)
        po.filter_points_by_plane(n_px, T, pts)

    def to_camera_and_label():
        po.transform_points(n_px, pts, inv_plane)
        depth.fill(np.uint16(0))
        po.depths_from_points(dims, depth, pts)
        color.copy_from(color_in)                   # label_frame snaps in place: start from the frame's colours each time
        lab.label_frame(color, depth, labels=labels, labels_rgba=rgba)

    # the state the re-render sees: points filtered in plane space for the centre, back in camera space for the draw
    to_plane()
    plane_pts = rdf.DeviceArray((H, W, 4), np.float32).copy_from(pts)
    sums = rr.center(plane_pts).get()
    center = sums[:3] / sums[3]
    out["points"] = int(sums[3])
    to_camera_and_label()
    M = rdf.SceneRerender.make_transform(plane, center, 1.1)
    eye = np.identity(4, np.float32)

    def other_steps():
        for _ in range(REPS):
            to_plane()
            to_camera_and_label()

    def centers():
        for _ in range(REPS):
            rr.center(plane_pts)

    def rerenders(m):
        def run():
            for _ in range(REPS):
                rr.run(pts, color_in, m, depth_rr, color_rr)
        return run

    def augment():
        for _ in range(REPS):
            rr.center(plane_pts)
            rr.run(pts, color_in, M, depth_rr, color_rr)

    for name, fn in (("center_us", centers), ("rerender_us", rerenders(M)), ("rerender_identity_us", rerenders(eye)),
                     ("augment_us", augment), ("other_steps_us", other_steps)):
        for _ in range(3):
            fn()
        out[name] = round(_events(torch, fn, 20) * 1e3 / REPS, 2)
    out["drawn_pixels"] = int((depth_rr.get() > 0).sum())
    out["rerender_share"] = round(out["augment_us"] / (out["augment_us"] + out["other_steps_us"]), 3)
    line = json.dumps({"rerender": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
