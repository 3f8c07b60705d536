#!/usr/bin/env python3
"""Times the stereo sensor (librdf_labels.so: rdf_stereo_sense) for two hands over a table at 848x480, D = 128, batches of 1
and 64, next to rdf_hand_scene_render of the same batch in the same run: what switching the sensor on costs per frame.
Prints one JSON line (hipEvent times between two events on the stream, medians after warm-up, REPS calls per sample) and
writes it to `--out FILE` (profiles/stereo_bench.json is such a run).  Per batch size B:
  render_us            one rdf_hand_scene_render of B clean frames (transforms already on the device)
  sense_us             one rdf_stereo_sense of B frames: all five launches
  ir_us                rdf_stereo_ir alone: rule I
  census_resolve_us    rdf_stereo_sense with D = 1, minus ir_us: the census and resolve launches (and two matcher launches of
                       one disparity each)
  match_us             sense_us minus the D = 1 call: the matcher's two launches, by difference
  sensor_per_frame_us  (render_us + sense_us) / B: a sensed frame costs a second render and the sensor
  render_per_frame_us  render_us / B
  match_steps          2 N H W D: the popcount-and-add steps of both directions
  match_gsteps_per_s   match_steps / match_us
  lane_cycles_per_step at `--clock-ghz` (default 2.4) and 256 CUs x 64 lanes: the lane cycles the matcher spends per step
The device's result at 106x60 is checked against the restatement first.  Standalone: bench.py does not run it."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, D, REPS = 480, 848, 128, 5
FOCAL = 600.                    # about the D415's at this resolution: the table 550 mm away has a disparity of 54.5
CAMERA_HEIGHT = 5500.
LANES = 256 * 64


def _events(torch, fn, samples=9):
    times = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def _poses(r, n, seed):
    rng = np.random.default_rng(seed)
    shift = np.where(np.arange(26) == 0, 1100., 0.)
    return r.model.sample_poses(n, rng) + shift, r.left_model.sample_poses(n, rng) - shift


def _check(rdf, scene):
    """Two hands over the table at 106x60 through render(sensor=) equal the restatement fed by hand_scene_numpy."""
    import hand_scene_numpy as hs
    import stereo_numpy as sn
    h, w = 60, 106
    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    cam = (w * 0.7, (w - 1) / 2., (h - 1) / 2.)
    r = rdf.HandSceneRenderer((h, w), cam, max_frames=2)
    s = rdf.StereoSensor((h, w), cam, max_disparity=24, max_frames=2)
    right, left = _poses(r, 3, 1)
    t = r.transforms(right, plane, left)
    table = np.tile(scene.table_of_plane(plane), (3, 1))
    depth, labels = r.render(t, "fine", table, 0, 7, sensor=s)
    t_r = t.astype(np.float64)
    t_r[:, :, 3] -= s.baseline
    table_r = table.astype(np.float64)
    table_r[:, 3] -= table_r[:, 0] * s.baseline
    verts, part, tris, _ = r._mesh[32]
    mesh = (verts, part, tris, r.tri_labels(32, "fine"))
    dl, ll, _ = hs.render(w, h, *mesh, t, table, r.f, r.ppx, r.ppy, empty_depth=0)
    dr, _, _ = hs.render(w, h, *mesh, t_r.astype(np.float32), table_r.astype(np.float32), r.f, r.ppx, r.ppy, empty_depth=0)
    want = sn.sense(dl, ll, dr, s.config_dict(), seed=7, empty_depth=0)
    assert np.array_equal(depth.get(), want["depth"]) and np.array_equal(labels.get(), want["labels"])
    return round(float((want["reason"] == 0).mean()), 4)


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    _lib = importlib.import_module("3d-beats_amd._lib")
    torch.cuda.set_device(0)
    rt = rdf.get_runtime()
    clock = float(sys.argv[sys.argv.index("--clock-ghz") + 1]) if "--clock-ghz" in sys.argv else 2.4
    out = {"frame": [H, W], "max_disparity": D, "checked_valid_share_106x60": _check(rdf, scene)}
    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    table = scene.table_of_plane(plane)
    cam = (FOCAL, (W - 1) / 2., (H - 1) / 2.)
    r = rdf.HandSceneRenderer((H, W), cam, max_frames=64)
    s = rdf.StereoSensor((H, W), cam, max_disparity=D, max_frames=64)
    lb = _lib.load("labels")
    verts, part, tris = r._device_mesh(32)
    tri_label = rdf.to_device(r.tri_labels(32, "fine"))
    one = _lib.StereoConfig(**dict(s.config_dict(), max_disparity=1))
    for B in (1, 64):
        right, left = _poses(r, B, 100 + B)
        t = r.transforms(right, plane, left)
        t_cu, table_cu = rdf.to_device(t), rdf.to_device(np.tile(table, (B, 1)))
        depth_l, labels_l, depth_r = (rdf.DeviceArray((B, H, W), np.uint16) for _ in range(3))
        r.render(t, "fine", table, 0, depth_out=depth_l, labels_out=labels_l)
        t_r = t.astype(np.float64)
        t_r[:, :, 3] -= s.baseline
        table_r = table.astype(np.float64)
        table_r[3] -= table_r[0] * s.baseline
        r.render(t_r.astype(np.float32), "fine", table_r.astype(np.float32), 0, depth_out=depth_r)
        depth, labels = rdf.DeviceArray((B, H, W), np.uint16), rdf.DeviceArray((B, H, W), np.uint16)
        ir = rdf.DeviceArray((B, 2, H, W), np.uint8)

        def render():
            for _ in range(REPS):
                rc = lb.rdf_hand_scene_render(B, W, H, int(verts.shape[0]), verts.ptr, part.ptr, int(tris.shape[0]), tris.ptr,
                                              tri_label.ptr, 32, t_cu.ptr, table_cu.ptr, r.f, r.ppx, r.ppy, r.z_near, r.z_far, 0, 0,
                                              0, 0, r._keys.ptr, depth.ptr, labels.ptr, rt.stream())
                _lib.check(lb, rc, "rdf_hand_scene_render")

        def sense(config):
            def run():
                for _ in range(REPS):
                    rc = lb.rdf_stereo_sense(B, W, H, depth_l.ptr, labels_l.ptr, depth_r.ptr, config, 5, 0, s._workspace.ptr,
                                             depth.ptr, labels.ptr, None, None, None, rt.stream())
                    _lib.check(lb, rc, "rdf_stereo_sense")
            return run

        def ir_only():
            for _ in range(REPS):
                _lib.check(lb, lb.rdf_stereo_ir(B, W, H, depth_l.ptr, depth_r.ptr, s.config, 5, ir.ptr, rt.stream()), "rdf_stereo_ir")
        res = {}
        for name, fn in (("render_us", render), ("sense_us", sense(s.config)), ("sense_d1_us", sense(one)), ("ir_us", ir_only)):
            for _ in range(2):
                fn()
            res[name] = round(_events(torch, fn) * 1e3 / REPS, 2)
        sense(s.config)()
        res["valid_share"] = round(float((depth.get() > 0).mean()), 4)
        res["census_resolve_us"] = round(res["sense_d1_us"] - res["ir_us"], 2)
        res["match_us"] = round(res["sense_us"] - res["sense_d1_us"], 2)
        res["sensor_per_frame_us"] = round((res["render_us"] + res["sense_us"]) / B, 2)
        res["render_per_frame_us"] = round(res["render_us"] / B, 2)
        steps = 2 * B * H * W * D
        res["match_steps"] = steps
        res["match_gsteps_per_s"] = round(steps / (res["match_us"] * 1e-6) / 1e9, 1)
        res["lane_cycles_per_step"] = round(res["match_us"] * 1e-6 * clock * 1e9 * LANES / steps, 2)
        out[f"batch_{B}"] = res
    line = json.dumps({"stereo": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
