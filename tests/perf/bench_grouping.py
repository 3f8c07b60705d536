#!/usr/bin/env python3
"""Times rdf_hand_groups and prints one JSON line:
  resident_us_per_frame  848x480 at level 3 (106x60, the app's size), N = 1, one call replayed from a captured graph:
                         median of hipEvent times over the replays
  resident_frames_per_s  the same size, N = 128 frames in one call
  global_us_per_frame    848x480 at level 0 (407 040 pixels: the global path), N = 1, direct calls
  host_route_us          for context: what the reference's route costs here -- shrink on the device, device-to-host copy,
                         the numpy restatement of make_groups + grow, host-to-device copy (wall clock, synchronised)
Standalone: bench.py does not run it."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 848


def _frame(rdf, idx):
    f = rdf.synth.live_frame(idx, H, W)
    return np.where(f == 65535, 0, f).astype(np.uint16)


def _events(torch, fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def main():
    import torch
    import grouping_numpy as gnp
    rdf = importlib.import_module("3d-beats_amd")
    torch.cuda.set_device(0)
    out = {}

    # resident path, N = 1, graph replay
    hg = rdf.HandGrouping((H, W), 3, 0.06)
    d = rdf.GpuBuffer((H, W), np.uint16, _frame(rdf, 7000))
    g = rdf.GpuBuffer((H >> 3, W >> 3), np.uint16)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hg.make_group_image(d, g)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hg.make_group_image(d, g)
    for _ in range(20):
        graph.replay()
    out["resident_us_per_frame"] = round(_events(torch, graph.replay, 200), 2)

    # resident path, N = 128
    n = 128
    hb = rdf.HandGrouping((H, W), 3, 0.06, max_frames=n)
    frames = np.stack([_frame(rdf, 7100 + k % 16) for k in range(n)])
    db = rdf.to_device(frames)
    gb = rdf.DeviceArray((n, H >> 3, W >> 3), np.uint16)
    gi = rdf.DeviceArray((n, 2, 3), np.float32)
    for _ in range(5):
        hb.make_group_image(db, gb, gi)
    us = _events(torch, lambda: hb.make_group_image(db, gb, gi), 50)
    out["resident_batch128_us"] = round(us, 1)
    out["resident_frames_per_s"] = round(n / (us * 1e-6), 0)

    # global path, 848x480 at level 0
    h0 = rdf.HandGrouping((H, W), 0, 0.06)
    g0 = rdf.GpuBuffer((H, W), np.uint16)
    for _ in range(5):
        h0.make_group_image(d, g0)
    out["global_us_per_frame"] = round(_events(torch, lambda: h0.make_group_image(d, g0), 50), 1)

    # the reference's route: shrink on the device, copy down, group on the host, copy up
    po = importlib.import_module("3d-beats_amd.cuda.points_ops").PointsOps()
    mm = rdf.GpuBuffer((H >> 3, W >> 3), np.uint16)
    up = rdf.GpuBuffer((H >> 3, W >> 3), np.uint16)
    walls = []
    for _ in range(30):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        po.shrink_image(np.array((W, H), np.int32), np.int32(3), d.cu(), mm.cu())
        mm_h = mm.cu().get()
        gi_h, st, _ = gnp.make_groups(mm_h, 0.06)
        up.cu().set(gnp.grow(st))
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e6)
    out["host_route_us"] = round(float(np.median(walls)), 1)
    assert np.array_equal(up.cu().get(), g.cu().get())
    print(json.dumps({"grouping": out}))


if __name__ == "__main__":
    main()
