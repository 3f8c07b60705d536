#!/usr/bin/env python3
"""Times one generation of the pose fit (librdf_labels.so: rdf_pose_fit) at 64 candidates on a 256x256 window of an 848x480
camera frame of one hand over the table, labelled by truth.  Prints one JSON line (hipEvent times between two events on
the stream, medians after warm-up, REPS calls per sample):
  generation_us        rdf_pose_fit of REPS generations / REPS: propose, raster, resolve, cost, select
  propose_us, render_us, cost_us, select_us
                       each of the four groups of launches alone, through its own entry point on buffers of its own
                       (render_us is rdf_hand_scene_render of the 64 candidates at window size: two launches)
  parent_render_us     HandSceneRenderer.render of the same 64 transforms at window size, transforms uploaded per call: the
                       part of a generation that existed before the fit
  host_loop_us         a host-driven generation: numpy kinematics of 64 poses, that render, rdf_pose_cost, and the terms read
                       back (wall clock, synchronised)
  cost_floor_us        rule C's read floor: (K * ww * wh * 4 B of candidates + ww * wh * 4 B of the observed window) over the
                       copy bandwidth measured here with rdf_memcpy_device_async on 2 x 52 MB
  quality              the fit from a start 10 mm and 6 mm off in the wrist, 0.15 rad in yaw and 0.2 rad in every knuckle,
                       after 24 and 96 generations: cost, accepted, the wrist's and the fingertips' distance from the truth
                       in mm.  One run of one seed: the spread is not measured.
The device's fit is checked against the restatement at 120x90 first.  `--out FILE` also writes the JSON there.
Standalone: bench.py does not run it."""
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, REPS, K, WIN, SEED = 480, 848, 20, 64, 256, 7
FOCAL = 600.                    # about the D415's at this resolution
CAMERA_HEIGHT = 7000.           # depth units: 700 mm above the table, so that the hand fits the window


def _events(torch, fn, samples=20):
    times = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def _check(rdf):
    """The device's fit of tests/pose_fit_cases.py's scene equals the restated one: history, pose, accepted count."""
    import pose_fit_cases as pc
    c, ref = pc.fit_case(), pc.fit_reference()
    f = rdf.PoseFitter((pc.FRAME_H, pc.FRAME_W), pc.CAM, c["plane"], candidates=pc.K_FIT, window=pc.WINDOW, seed=pc.SEED)
    got = f.fit(c["depth"], c["labels"], c["start"], generations=pc.G_FIT).get()
    assert got.history.tolist() == ref["history"] and got.accepted == ref["state"]["accepted"]
    assert np.array_equal(got.pose.view(np.uint64), ref["state"]["pose"].view(np.uint64))
    return ref["history"][-1]


def main():
    import torch
    import pose_fit_cases as pc
    rdf = importlib.import_module("3d-beats_amd")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    _lib = importlib.import_module("3d-beats_amd._lib")
    torch.cuda.set_device(0)
    rt = rdf.get_runtime()
    lb = _lib.load("labels")
    out = {"frame": [H, W], "window": [WIN, WIN], "candidates": K, "seed": SEED, "checked_final_cost_120x90": _check(rdf)}

    n_copy = 64 * H * W * 2
    src, dst = rdf.DeviceArray((n_copy,), np.uint8).fill(1), rdf.DeviceArray((n_copy,), np.uint8)

    def copies():
        for _ in range(REPS):
            _lib.check(rt.lib, rt.lib.rdf_memcpy_device_async(dst.ptr, src.ptr, n_copy, rt.stream()), "rdf_memcpy_device_async")
    for _ in range(3):
        copies()
    copy_us = _events(torch, copies) * 1e3 / REPS
    bandwidth = 2 * n_copy / (copy_us * 1e-6)
    out["copy_52MB_us"] = round(copy_us, 2)
    out["copy_TB_per_s"] = round(bandwidth / 1e12, 2)

    # the observed frame: the true pose over the table, labelled by truth
    cam = (FOCAL, (W - 1) / 2., (H - 1) / 2.)
    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    renderer = rdf.HandSceneRenderer((H, W), cam)
    truth = pc.true_pose(renderer.model)
    labels = rdf.DeviceArray((1, H, W), np.uint16)
    depth = renderer.camera_sequence(truth[None], plane, labels_out=labels)
    hand = np.argwhere(labels.get()[0] > 0)
    out["hand_pixels"] = int(len(hand))
    x0 = int(np.clip((hand[:, 1].min() + hand[:, 1].max()) // 2 - WIN // 2, 0, W - WIN)) | 1      # odd: rows not 16-byte aligned
    y0 = int(np.clip((hand[:, 0].min() + hand[:, 0].max()) // 2 - WIN // 2, 0, H - WIN))
    window = (min(x0, W - WIN), y0, WIN, WIN)
    assert window[0] <= hand[:, 1].min() and hand[:, 1].max() < window[0] + WIN and y0 <= hand[:, 0].min() and hand[:, 0].max() < y0 + WIN
    out["window_origin"] = [window[0], window[1]]
    fitter = rdf.PoseFitter((H, W), cam, plane, candidates=K, window=window, seed=SEED)
    start = pc.start_pose(fitter.model)

    # ---- quality: one run
    quality = {}
    tips_true = fitter.model.fingertips(truth)[0]
    for G in (24, 96):
        r = fitter.fit(depth[0], labels[0], start, generations=G).get()
        tips = fitter.model.fingertips(r.pose)[0]
        u = fitter.model.units_per_mm
        quality[f"after_{G}"] = {"cost": r.cost, "first_cost": int(r.history[0]), "accepted": r.accepted,
                                 "wrist_mm": round(float(np.linalg.norm(r.pose[:3] - truth[:3]) / u), 2),
                                 "fingertips_mm": [round(float(v), 2) for v in np.linalg.norm(tips - tips_true, axis=1) / u]}
    out["quality"] = quality

    # ---- one generation through rdf_pose_fit
    fitter.fit(depth[0], labels[0], start, generations=8)
    d = fitter._dev

    def generations():
        fitter._run(depth[0], labels[0], REPS, False, None)
    for _ in range(3):
        generations()
    out["generation_us"] = round(_events(torch, generations) * 1e3 / REPS, 2)

    # ---- the four groups, each alone, on buffers of its own
    n_px = WIN * WIN
    poses, tforms = rdf.DeviceArray((K, 26), np.float64), rdf.DeviceArray((K, 16, 12), np.float32)
    terms = rdf.DeviceArray((K, 4), np.uint64).fill(0)
    cd, cl = rdf.DeviceArray((K, WIN, WIN), np.uint16), rdf.DeviceArray((K, WIN, WIN), np.uint16)
    keys = rdf.DeviceArray((int(lb.rdf_hand_scene_workspace_bytes(K, WIN, WIN)),), np.uint8).fill(0xFF)
    state = rdf.DeviceArray((256,), np.uint8)
    state.copy_from(d["state"])
    cfg = ctypes.addressof(fitter._cfg)
    s = rt.stream()
    ppx, ppy = float(np.float32(cam[1]) - np.float32(window[0])), float(np.float32(cam[2]) - np.float32(window[1]))

    def propose():
        _lib.check(lb, lb.rdf_pose_propose(cfg, state.ptr, 0, poses.ptr, tforms.ptr, terms.ptr, s), "rdf_pose_propose")

    def render():
        _lib.check(lb, lb.rdf_hand_scene_render(K, WIN, WIN, int(d["verts"].shape[0]), d["verts"].ptr, d["vert_part"].ptr,
                                                int(d["tris"].shape[0]), d["tris"].ptr, d["tri_label"].ptr, 16, tforms.ptr, None,
                                                fitter.f, ppx, ppy, scene.Z_NEAR, scene.Z_FAR, 0, 0, 0, 0, keys.ptr, cd.ptr, cl.ptr, s),
                   "rdf_hand_scene_render")

    def cost():
        _lib.check(lb, lb.rdf_pose_cost(W, H, depth.ptr, labels.ptr, 1, *window, K, cd.ptr, cl.ptr, fitter.target_mask, terms.ptr, s),
                   "rdf_pose_cost")

    def select():
        _lib.check(lb, lb.rdf_pose_select(K, terms.ptr, poses.ptr, fitter.w_boundary, fitter.w_label, 0, state.ptr, None, s),
                   "rdf_pose_select")
    for name, fn in (("propose_us", propose), ("render_us", render), ("cost_us", cost), ("select_us", select)):
        def many(fn=fn):
            for _ in range(REPS):
                fn()
        for _ in range(3):
            many()
        out[name] = round(_events(torch, many) * 1e3 / REPS, 2)
    out["cost_floor_us"] = round((K * n_px * 4 + n_px * 4) / bandwidth * 1e6, 2)
    out["dominant"] = max(("propose", "render", "cost", "select"), key=lambda n: out[n + "_us"])

    # ---- what existed before: the renderer's own render() of the same transforms at window size
    small = rdf.HandSceneRenderer((WIN, WIN), (FOCAL, ppx, ppy), max_frames=K)
    t_host = tforms.get()
    cd2, cl2 = rdf.DeviceArray((K, WIN, WIN), np.uint16), rdf.DeviceArray((K, WIN, WIN), np.uint16)

    def parent():
        for _ in range(REPS):
            small.render(t_host, "fine", None, 0, depth_out=cd2, labels_out=cl2)
    for _ in range(3):
        parent()
    out["parent_render_us"] = round(_events(torch, parent) * 1e3 / REPS, 2)
    assert np.array_equal(cd2.get(), cd.get()) and np.array_equal(cl2.get(), cl.get())

    # ---- a host-driven generation: numpy kinematics, render, cost, terms read back
    host_poses = poses.get()
    cam_from_plane = np.linalg.inv(plane)

    def host_generation():
        t = fitter.model.part_transforms(host_poses, cam_from_plane)
        small.render(t, "fine", None, 0, depth_out=cd2, labels_out=cl2)
        terms.fill(0)
        _lib.check(lb, lb.rdf_pose_cost(W, H, depth.ptr, labels.ptr, 1, *window, K, cd2.ptr, cl2.ptr, fitter.target_mask, terms.ptr, s),
                   "rdf_pose_cost")
        return terms.get()
    for _ in range(3):
        host_generation()
    rt.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        host_generation()
    out["host_loop_us"] = round((time.perf_counter() - t0) * 1e6 / REPS, 1)

    line = json.dumps({"pose_fit": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
