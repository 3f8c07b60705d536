#!/usr/bin/env python3
"""Times the device score of label maps (rdf_score_labels of librdf_labels.so, score.LabelScorer) on 64 synthetic live-like
848x480 frames (about 85 % of the pixels truth 0 against prediction 65535), C = 7, and prints one JSON line (hipEvent times,
medians after warm-up):
  add_us, add_gbps            one LabelScorer.add of the batch: both maps read once, 4 bytes per pixel
  add_per_image_us            the same with the per-image sums
  add_reduce2_us              a [N, 240, 424] prediction against the same truth at labels_reduce 2
  d2d_copy_us, d2d_copy_gbps  the yardstick: rdf_memcpy_device_async of one map, which moves the same bytes (2 read + 2
                              written per pixel)
  host_path_ms                what the score replaces: two .get() and np.sum(got == truth) / np.sum(truth > 0)
  device_path_ms              reset + add + result (the read back of the counts included), wall clock
  train_forest_*_s            dataset.train_forest on a small written dataset, device_score off and on (wall clock; same
                              forest and pct, checked)
The counts are checked against tests/score_numpy.py.  `--out FILE` also writes the JSON there.  Standalone: bench.py does not
run it."""
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W, C = 64, 480, 848, 7


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


def _wall(torch, fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def live_like_maps(n, h, w, classes, seed=0):
    """Truth 0 and prediction 65535 outside each frame's ellipse (~15 % of the frame, as synth.live_frame's); inside, truth in
    1..classes-1 in vertical bands and a prediction that agrees on about two pixels of three."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = np.zeros((n, h, w), np.uint16)
    pred = np.full((n, h, w), 65535, np.uint16)
    for i in range(n):
        cy, cx = rng.uniform(0.35, 0.65) * h, rng.uniform(0.35, 0.65) * w
        blob = ((yy - cy) / (h * 0.22)) ** 2 + ((xx - cx) / (w * 0.22)) ** 2 < 1.
        bands = (1 + (xx // 16 + i) % (classes - 1)).astype(np.uint16)
        truth[i][blob] = bands[blob]
        noisy = np.where(rng.random((h, w)) < 0.67, bands, rng.integers(0, classes, (h, w))).astype(np.uint16)
        pred[i][blob] = noisy[blob]
    return pred, truth


def main():
    import torch
    import score_numpy as snp
    rdf = importlib.import_module("3d-beats_amd")
    ds_mod = importlib.import_module("3d-beats_amd.dataset")
    torch.cuda.set_device(0)
    lib = rdf.get_runtime().lib
    out = {"frames": [N, H, W], "classes": C}

    pred, truth = live_like_maps(N, H, W, C)
    out["background"] = round(float(np.mean((truth == 0) & (pred == 65535))), 4)
    want = snp.score_counts(pred, truth, C)
    p, t = rdf.to_device(pred), rdf.to_device(truth)
    scorer = rdf.LabelScorer(C)
    scorer.add(p, t, per_image=True)
    assert np.array_equal(scorer.counts_cu.get(), want)
    assert np.array_equal(scorer.result().per_image, snp.score_per_image(pred, truth))
    for _ in range(3):
        scorer.add(p, t)
    out["add_us"] = round(_events(torch, lambda: scorer.add(p, t), 30) * 1e3, 2)
    out["add_gbps"] = round((pred.nbytes + truth.nbytes) / out["add_us"] / 1e3, 1)
    out["add_per_image_us"] = round(_events(torch, lambda: scorer.add(p, t, per_image=True), 30) * 1e3, 2)

    sub = np.ascontiguousarray(pred[:, ::2, ::2])
    ps = rdf.to_device(sub)
    half = rdf.LabelScorer(C).add(ps, t, 2)
    assert np.array_equal(half.counts_cu.get(), snp.score_counts(sub, truth, C, 2))
    out["add_reduce2_us"] = round(_events(torch, lambda: half.add(ps, t, 2), 30) * 1e3, 2)

    dst = rdf.DeviceArray(pred.shape, np.uint16)
    st = rdf.get_runtime().stream()

    def copy():
        assert lib.rdf_memcpy_device_async(dst.ptr, p.ptr, pred.nbytes, st) == 0
    for _ in range(3):
        copy()
    out["d2d_copy_us"] = round(_events(torch, copy, 30) * 1e3, 2)
    out["d2d_copy_gbps"] = round(2 * pred.nbytes / out["d2d_copy_us"] / 1e3, 1)
    out["add_over_copy"] = round(out["add_us"] / out["d2d_copy_us"], 2)

    state = {}

    def host_path():
        got, tr = p.get(), t.get()
        state["pct"] = float(np.sum(got == tr) / np.sum(tr > 0))

    def device_path():
        state["score"] = scorer.reset().add(p, t).result()
    host_path()
    device_path()
    out["host_path_ms"] = round(_wall(torch, host_path, 5) * 1e3, 2)
    out["device_path_ms"] = round(_wall(torch, device_path, 20) * 1e3, 3)
    assert state["score"].pct_matching == state["pct"] and np.array_equal(scorer.counts_cu.get(), want)
    out["pct_matching"] = round(state["pct"], 4)
    out["accuracy"] = round(state["score"].accuracy, 4)

    # train_forest with the score on the host and on the device: 16 training and 32 test frames of 424x240
    n, h, w = 48, 240, 424
    depth = rdf.synth.frames(["live" if i % 4 else "dense" for i in range(n)], 700, h, w)
    xx = np.mgrid[0:h, 0:w][1]
    labels = (1 + (xx * 3 // w + (depth > 4000)) % 3).astype(np.uint16)
    labels[depth == 65535] = 0
    with tempfile.TemporaryDirectory() as tmp:
        ds_mod.write_dataset(tmp, depth, labels, {k: [60 * k, 255 - 60 * k, k, 255] for k in (1, 2, 3)})
        runs = {}
        for device_score in (False, True, False, True):          # the first pair warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[device_score] = ds_mod.train_forest(tmp, 16, 32, 64, 32, 2, 8, None, trees_to_try=4, log=lambda *_: None,
                                                     tree_seed=3, device_score=device_score)
            torch.cuda.synchronize()
            out["train_forest_device_score_s" if device_score else "train_forest_host_score_s"] = round(time.perf_counter() - t0, 3)
        assert runs[False][0].tobytes() == runs[True][0].tobytes() and runs[False][1] == runs[True][1]
    out["train_forest"] = {"train": 16, "test": 32, "frame": [h, w], "depth": 8, "proposals": 64, "candidates": 4}
    line = json.dumps({"score": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
