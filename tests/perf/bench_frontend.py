#!/usr/bin/env python3
"""Times the depth front end (librdf_frontend.so) and prints one JSON line:
  calibrate_ms           rdf_calibrate_plane at 848x480 x 25 000 candidates (candidates, inlier counts, winner):
                         median of hipEvent times over direct calls
  inliers_ms             k_plane_inliers alone (rdf_plane_inliers on the same candidates)
  point_plane_tests      valid points x candidates of that call
  valu_bound_ms          7 lane-ops per test over 256 CUs x 64 lanes at 2.4 GHz (the unpacked bound)
  inliers_frac_of_bound  valu_bound_ms / inliers_ms
  front_us_per_frame     rdf_frame_front at 848x480, Gaussian k = 5, N = 1 (one call replayed from a captured graph) and
                         N = 128 (one call, per frame)
Standalone: bench.py does not run it."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, G, T = 480, 848, 25000, 40.


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


def main():
    import torch
    import frontend_numpy as fnp
    from test_frontend import scene
    rdf = importlib.import_module("3d-beats_amd")
    _lib = importlib.import_module("3d-beats_amd._lib")
    pom = importlib.import_module("3d-beats_amd.cuda.points_ops")
    torch.cuda.set_device(0)
    fe = _lib.load("frontend")
    s = rdf.get_runtime().stream()
    out = {}

    depth, _, (f, ppx, ppy) = scene(H, W, 420.)
    pts_np = fnp.deproject(depth, ppx, ppy, f)
    pts = rdf.to_device(pts_np)
    rand = rdf.to_device(np.random.default_rng(0).random((G, 32), dtype=np.float32))
    ws = rdf.DeviceArray((int(fe.rdf_calibrate_plane_workspace_bytes(G)),), np.uint8)
    plane = rdf.DeviceArray((16,), np.float32).fill(0)
    res = rdf.DeviceArray((112,), np.uint8)

    def calib():
        _lib.check(fe, fe.rdf_calibrate_plane(G, T, W, H, rand.ptr, pts.ptr, None, ws.ptr, plane.ptr, res.ptr, s),
                            "rdf_calibrate_plane")
    for _ in range(3):
        calib()
    out["calibrate_ms"] = round(_events(torch, calib, 20), 3)
    cand = ws.ptr
    counts = rdf.DeviceArray((G,), np.int32).fill(0)     # zeroed once: after k calls it holds k x the counts

    def inliers():
        _lib.check(fe, fe.rdf_plane_inliers(G, T, H * W, pts.ptr, cand, counts.ptr, s), "rdf_plane_inliers")
    inliers()
    ms = _events(torch, inliers, 20)
    once = np.maximum(ws.get()[G * 64:G * 68].view(np.int32), 0)     # calibrate's counts (-1 = invalid, never added to)
    assert np.array_equal(counts.get(), 21 * once)
    tests = int((pts_np[..., 3] == 1).sum()) * G
    bound = tests * 7 / (256 * 64 * 2.4e9) * 1e3
    out["inliers_ms"] = round(ms, 3)
    out["point_plane_tests"] = tests
    out["valu_bound_ms"] = round(bound, 3)
    out["inliers_frac_of_bound"] = round(bound / ms, 3)

    ff = rdf.FrameFrontEnd((H, W), (f, ppx, ppy), T, gauss_sigma=2.0, k_size=5, num_random_guesses=2000, seed=1)
    dbuf = rdf.GpuBuffer((H, W), np.uint16, depth)
    ff.calibrate(dbuf)
    o = rdf.GpuBuffer((H, W), np.uint16)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ff.run(dbuf, o)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ff.run(dbuf, o)
    for _ in range(20):
        graph.replay()
    out["front_us_per_frame_n1"] = round(_events(torch, graph.replay, 200) * 1e3, 2)
    n = 128
    db = rdf.to_device(np.stack([depth] * n))
    ob = rdf.DeviceArray((n, H, W), np.uint16)
    for _ in range(3):
        ff.run(db, ob)
    out["front_us_per_frame_n128"] = round(_events(torch, lambda: ff.run(db, ob), 20) * 1e3 / n, 2)
    want = fnp.frame_front(depth, ppx, ppy, f, ff.calibrated_plane.get_mat(), T, pom.gaussian_kernel(5, 2.0))[0]
    assert np.array_equal(o.cu().get(), want) and np.array_equal(ob.get()[n - 1], want)
    print(json.dumps({"frontend": out}))


if __name__ == "__main__":
    main()
