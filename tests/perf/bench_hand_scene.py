#!/usr/bin/env python3
"""Times HandSceneRenderer.render (librdf_labels.so: rdf_hand_scene_render) for two hands at 848x480, batches of 1 and 64
sampled poses over the table, as camera frames (table drawn, holes and noise on).  Prints one JSON line (hipEvent times
between two events on the stream, medians after warm-up, REPS calls per sample).  Per batch size B:
  render_us            one render() of B frames: the transforms' upload, raster and resolve
  kernels_us           one rdf_hand_scene_render on transforms that are already on the device (both launches)
  resolve_us           the same call with n_tris = 0: the resolve pass alone, every key empty (it then skips the key
                       reset, 8 of its 12 bytes per mesh pixel; mesh pixels are `mesh_share` of the frame)
  raster_us            kernels_us - resolve_us: the raster pass, by difference (a kernel trace gives it directly)
  frames_per_s         B / render_us
  resolve_floor_us     the resolve pass's memory floor: (8 B key read + 2 x 2 B written per pixel + 8 B key reset per mesh
                       pixel) over the copy bandwidth measured here with rdf_memcpy_device_async on 2 x 52 MB
  dominant             the larger of raster_us and resolve_us
The device's images are checked against the restatement at 106x60 first.  `--out FILE` also writes the JSON there.
`--trace B` is for a run under a kernel tracer: nothing but warm-up and the kernels_us loop of batch B, so that the trace's
per-kernel averages are those of one shape.  Standalone: bench.py does not run it."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, REPS = 480, 848, 20
FOCAL = 600.                    # about the D415's at this resolution
CAMERA_HEIGHT = 5500.           # depth units: 550 mm above the table


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


def _poses(r, n, seed):
    rng = np.random.default_rng(seed)
    shift = np.where(np.arange(26) == 0, 1100., 0.)
    return r.model.sample_poses(n, rng) + shift, r.left_model.sample_poses(n, rng) - shift


def _check(rdf, scene):
    """Two hands over the table at 106x60, five poses, holes and noise on, equal the restatement's images."""
    import hand_scene_numpy as hs
    h, w = 60, 106
    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    r = rdf.HandSceneRenderer((h, w), (w * 0.7, (w - 1) / 2., (h - 1) / 2.), max_frames=4)
    right, left = _poses(r, 5, 1)
    t = r.transforms(right, plane, left)
    table = scene.table_of_plane(plane)
    depth, labels = r.render(t, "fine", table, 0, 7, 0.05, 6)
    verts, part, tris, _ = r._mesh[32]
    want = hs.render(w, h, verts, part, tris, r.tri_labels(32, "fine"), t, np.tile(table, (5, 1)), r.f, r.ppx, r.ppy,
                     empty_depth=0, seed=7, hole_threshold=int(0.05 * 2 ** 32), noise_amp=6)
    assert np.array_equal(depth.get(), want[0]) and np.array_equal(labels.get(), want[1])
    return int((want[1] > 0).sum())


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    _lib = importlib.import_module("3d-beats_amd._lib")
    torch.cuda.set_device(0)
    rt = rdf.get_runtime()
    trace = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else None
    out = {"frame": [H, W]}
    if trace is None:
        out["checked_mesh_pixels_106x60"] = _check(rdf, scene)

    # the yardstick the project quotes: a device-to-device copy of 52 MB (read + written)
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

    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    table = scene.table_of_plane(plane)
    r = rdf.HandSceneRenderer((H, W), (FOCAL, (W - 1) / 2., (H - 1) / 2.), max_frames=64)
    lb = _lib.load("labels")
    verts, part, tris = r._device_mesh(32)
    out["triangles"] = int(tris.shape[0])
    for B in (1, 64) if trace is None else (trace,):
        right, left = _poses(r, B, 100 + B)
        t = r.transforms(right, plane, left)
        depth, labels = rdf.DeviceArray((B, H, W), np.uint16), rdf.DeviceArray((B, H, W), np.uint16)
        t_cu, table_cu = rdf.to_device(t), rdf.to_device(np.tile(table, (B, 1)))
        tri_label = rdf.to_device(r.tri_labels(32, "fine"))
        threshold = int(0.02 * 2 ** 32)

        def render():
            for _ in range(REPS):
                r.render(t, "fine", table, 0, 5, 0.02, 8, depth_out=depth, labels_out=labels)

        def call(n_tris):
            def run():
                for _ in range(REPS):
                    rc = lb.rdf_hand_scene_render(B, W, H, int(verts.shape[0]), verts.ptr, part.ptr, n_tris, tris.ptr, tri_label.ptr,
                                                  32, t_cu.ptr, table_cu.ptr, r.f, r.ppx, r.ppy, r.z_near, r.z_far, 0, 5, threshold, 8,
                                                  r._keys.ptr, depth.ptr, labels.ptr, rt.stream())
                    _lib.check(lb, rc, "rdf_hand_scene_render")
            return run
        res = {}
        for name, fn in (("render_us", render), ("kernels_us", call(int(tris.shape[0]))), ("resolve_us", call(0))):
            if trace is not None and name != "kernels_us":
                continue
            for _ in range(3):
                fn()
            res[name] = round(_events(torch, fn) * 1e3 / REPS, 2)
        if trace is not None:
            out[f"batch_{B}"] = res
            continue
        render()
        mesh_px = int((labels.get() > 0).sum())
        res["mesh_share"] = round(mesh_px / (B * H * W), 4)
        res["raster_us"] = round(res["kernels_us"] - res["resolve_us"], 2)
        res["frames_per_s"] = round(B / (res["render_us"] * 1e-6), 1)
        floor_bytes = B * H * W * 12 + mesh_px * 8
        res["resolve_floor_us"] = round(floor_bytes / bandwidth * 1e6, 2)
        res["dominant"] = "raster" if res["raster_us"] > res["resolve_us"] else "resolve"
        out[f"batch_{B}"] = res
    line = json.dumps({"hand_scene": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
