#!/usr/bin/env python3
"""Times the glove-colour labelling (librdf_labels.so) on one 848x480 synthetic glove frame, K = 4, 8 tries x 32 iterations,
and prints one JSON line (hipEvent times, medians after warm-up):
  mapping_one_call_ms    ColorLabeler.make_color_mapping_async: rdf_make_color_mapping, 65 launches, no host round trip
  mapping_host_loop_ms   the reference's shape (live_data_convert.py:166-197) on this library's single-step entry point:
                         256 x (upload colours, zero counts, split_pixels_by_nearest_color, read counts back, update on the
                         host).  It already has the privatised kernel, so it understates the gain over the reference's atomics.
  single_step_us         one split_pixels_by_nearest_color launch (device time between events, 20 launches per sample)
  label_frame_us         one rdf_label_frame with depth and RGBA outputs (20 launches per sample)
Both mappings are checked against each other and against the restatement.  `--out FILE` also writes the JSON there.
Standalone: bench.py does not run it."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, K, TRIES, ITERATIONS = 480, 848, 4, 8, 32
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


def main():
    import torch
    import labels_numpy as lnp
    rdf = importlib.import_module("3d-beats_amd")
    po = importlib.import_module("3d-beats_amd.cuda.points_ops").PointsOps()
    torch.cuda.set_device(0)
    out = {"frame": [H, W], "colors": K, "tries": TRIES, "iterations": ITERATIONS}

    frame, _ = lnp.glove_scene(H, W, PALETTE, 8, seed=1)
    out["lit_pixels"] = int((frame.sum(-1) > 0).sum())
    init = np.random.default_rng(0).integers(0, 256, (TRIES, K, 3)).astype(np.uint8)
    img = rdf.to_device(frame)
    lab = rdf.ColorLabeler(K, TRIES, ITERATIONS)
    init_cu = rdf.to_device(init)

    def one_call():
        lab.make_color_mapping_async(img, init_cu)
    for _ in range(3):
        one_call()
    out["mapping_one_call_ms"] = round(_events(torch, one_call, 20), 3)
    got = lab.color_mapping_gpu.get()
    costs = np.array(lab.result()["cost"][:TRIES])

    colors_gpu = rdf.GpuBuffer((K, 3), dtype=np.uint8)
    counts_gpu = rdf.GpuBuffer((K, 5), dtype=np.uint64)
    state = {}

    def host_loop():
        best_diffs, best = np.inf, None
        tries_cost = []
        for t in range(TRIES):
            colors = init[t].copy()
            for _ in range(ITERATIONS):
                colors_gpu.cu().set(colors)
                counts_gpu.cu().fill(np.uint64(0))
                po.split_pixels_by_nearest_color(np.int32(W), np.int32(H), np.int32(K), colors_gpu.cu(), img, counts_gpu.cu())
                c = counts_gpu.cu().get()
                cost = np.sum(c[:, 4].view(np.float64))
                with np.errstate(all="ignore"):
                    colors = (c[:, 1:4].T / c[:, 0]).T.astype(np.uint8)
            tries_cost.append(cost)
            if cost < best_diffs:
                best_diffs, best = cost, colors.copy()
        state["best"], state["costs"] = best, np.array(tries_cost)
    host_loop()
    out["mapping_host_loop_ms"] = round(_events(torch, host_loop, 5), 3)
    want, _, want_costs, _ = lnp.make_color_mapping(frame, init, ITERATIONS)
    assert np.array_equal(got, want) and np.array_equal(state["best"], want)
    assert np.array_equal(costs, want_costs) and np.array_equal(state["costs"], want_costs)
    out["speedup"] = round(out["mapping_host_loop_ms"] / out["mapping_one_call_ms"], 2)

    colors_gpu.cu().set(want)

    def steps():
        for _ in range(20):
            po.split_pixels_by_nearest_color(W, H, K, colors_gpu.cu(), img, counts_gpu.cu())
    steps()
    out["single_step_us"] = round(_events(torch, steps, 20) * 1e3 / 20, 2)

    lab.set_color_mapping(want)
    depth = rdf.DeviceArray((H, W), np.uint16).fill(0)
    labels, rgba = rdf.DeviceArray((H, W), np.uint16), rdf.DeviceArray((H, W, 4), np.uint8)

    def label():
        for _ in range(20):
            lab.label_frame(img, depth, labels=labels, labels_rgba=rgba)
    label()
    out["label_frame_us"] = round(_events(torch, label, 20) * 1e3 / 20, 2)
    assert np.array_equal(labels.get(), lnp.label_frame(want, frame)[1])
    line = json.dumps({"labels": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
