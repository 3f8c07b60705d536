#!/usr/bin/env python3
"""Times the depth post-filter (librdf_frontend.so: rdf_depth_filter) on 848x480 frames of two hands over a table, sensed by
StereoSensor at D = 128, in batches of 1 and 64 consecutive frames.  Prints one JSON line (hipEvent times between two events
on the stream, REPS calls per sample, medians after warm-up with the lowest and highest sample next to them) and writes it to
`--out FILE` (profiles/depth_filter_bench.json is such a run; `--commit TEXT` records what it was measured on).  Per batch B:
  call_us              one rdf_depth_filter of B frames, the default chain, flags written
  s_only_us            the same with T and F off; t_only_us, f_only_us likewise
  front_us             rdf_frame_front of the same B frames (Gaussian on), for scale
  floor_us             B * W * H * (2 + 2 + 1) bytes of frames in, frames out and flags plus 8 * W * H bytes of state, over the
                       copy rate measured here (rdf_memcpy_device_async on 2 x 52 MB; bytes read plus bytes written)
  ratio_to_floor       call_us / floor_us
  per_frame_us         call_us / B
and once:
  empty_call_us        a call with n = 0 through the binding: the Python and ctypes overhead, wall clock
  launches_per_call    1: what the entry point enqueues, whatever B is
  tick_added_us        batch_1's call_us: what BeatsSession.tick gains on the device with post_filter=
The device's result at 72x9 is checked against the restatement first.  Standalone: bench.py does not run it."""
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

H, W, D, REPS = 480, 848, 128, 5
FOCAL = 600.
CAMERA_HEIGHT = 5500.


def _events(torch, fn, samples=9):
    """(median, lowest, highest) in ms."""
    times = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def _us(torch, fn):
    for _ in range(2):
        fn()
    return [round(v * 1e3 / REPS, 2) for v in _events(torch, fn)]


def _check(rdf):
    import depth_filter_cases as dc
    c = dc.gpu_case("nine rows, 16 bytes at a time")
    N, h, w = c["frames"].shape
    f = rdf.DepthPostFilter((h, w))
    flags = rdf.DeviceArray((N, h, w), np.uint8)
    out = f.run(c["frames"], flags_out=flags)
    assert np.array_equal(out.get(), c["want"]["depth"]) and np.array_equal(flags.get(), c["want"]["flags"])
    assert np.array_equal(f.state(), c["want"]["state"])
    return [w, h, N]


def _sensed(rdf, scene, B):
    """B frames of two hands over the table through the stereo sensor, 0 = no reading: device uint16 [B, H, W]."""
    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    table = scene.table_of_plane(plane)
    cam = (FOCAL, (W - 1) / 2., (H - 1) / 2.)
    r = rdf.HandSceneRenderer((H, W), cam, max_frames=64)
    s = rdf.StereoSensor((H, W), cam, max_disparity=D, max_frames=64)
    rng = np.random.default_rng(100 + B)
    shift = np.where(np.arange(26) == 0, 1100., 0.)
    right, left = r.model.sample_poses(B, rng) + shift, r.left_model.sample_poses(B, rng) - shift
    t = r.transforms(right, plane, left)
    depth, _ = r.render(t, "fine", table, 0, 5, sensor=s)
    return depth, plane, cam


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    _lib = importlib.import_module("3d-beats_amd._lib")
    torch.cuda.set_device(0)
    rt = rdf.get_runtime()
    fe = _lib.load("frontend")
    out = {"frame": [H, W], "max_disparity": D, "checked_against_the_restatement": _check(rdf), "launches_per_call": 1}
    if "--commit" in sys.argv:
        out["commit"] = sys.argv[sys.argv.index("--commit") + 1]

    n_copy = 52 * 1024 * 1024
    src, dst = rdf.DeviceArray((n_copy,), np.uint8).fill(1), rdf.DeviceArray((n_copy,), np.uint8)

    def copies():
        for _ in range(REPS):
            _lib.check(rt.lib, rt.lib.rdf_memcpy_device_async(dst.ptr, src.ptr, n_copy, rt.stream()), "rdf_memcpy_device_async")
    copy_us = _us(torch, copies)
    rate = 2 * n_copy / (copy_us[0] * 1e-6)                  # bytes moved per second
    out["copy_us"], out["copy_gb_per_s"] = copy_us, round(rate / 1e9, 1)

    chain = rdf.DepthPostFilter((H, W))
    cfg = chain.config_dict()
    stages = {"call_us": cfg, "s_only_us": dict(cfg, temporal=0, fill_mode=0), "t_only_us": dict(cfg, spatial_radius=0, fill_mode=0),
              "f_only_us": dict(cfg, spatial_radius=0, temporal=0)}
    none = ctypes.byref(chain.config)
    t0 = time.perf_counter()
    for _ in range(2000):
        fe.rdf_depth_filter(0, W, H, None, none, None, None, None, None)
    out["empty_call_us"] = round((time.perf_counter() - t0) / 2000 * 1e6, 2)

    for B in (1, 64):
        depth, plane, cam = _sensed(rdf, scene, B)
        res = {"valid_share_in": round(float((depth.get() != 0).mean()), 4)}
        filtered, flags = rdf.DeviceArray((B, H, W), np.uint16), rdf.DeviceArray((B, H, W), np.uint8)
        state = rdf.DeviceArray((H * W,), np.uint32).fill(0)

        def call(config):
            c = _lib.DepthFilterConfig(**config)

            def run():
                for _ in range(REPS):
                    rc = fe.rdf_depth_filter(B, W, H, depth.ptr, ctypes.byref(c), state.ptr, filtered.ptr, flags.ptr, rt.stream())
                    _lib.check(fe, rc, "rdf_depth_filter")
            return run
        for name, config in stages.items():
            res[name] = _us(torch, call(config))
        state.fill(0)
        call(cfg)()
        res["valid_share_out"] = round(float((filtered.get() != 0).mean()), 4)
        front = rdf.FrameFrontEnd((H, W), cam, 40., gauss_sigma=2.0)
        front.set_plane(plane)
        clean = rdf.DeviceArray((B, H, W), np.uint16)

        def front_end():
            for _ in range(REPS):
                front.run(depth, clean)
        res["front_us"] = _us(torch, front_end)
        floor_bytes = B * W * H * 5 + 8 * W * H
        res["floor_bytes"] = floor_bytes
        res["floor_us"] = round(floor_bytes / rate * 1e6, 2)
        res["ratio_to_floor"] = round(res["call_us"][0] / res["floor_us"], 2)
        res["per_frame_us"] = round(res["call_us"][0] / B, 2)
        out[f"batch_{B}"] = res
    out["tick_added_us"] = out["batch_1"]["call_us"][0]
    line = json.dumps({"depth_filter": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
