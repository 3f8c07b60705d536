#!/usr/bin/env python3
"""Times the hand's shape (rdf_labels_shape_pool / rdf_labels_shape_decide of librdf_labels.so; shape.ShapeVoter) beside the way
to the same answer that existed before it, records how often the pooled vote is right, and prints one JSON line.  `--out
FILE` also writes it there (profiles/shape_bench.json); `--time-only` skips the second part.  Standalone: bench.py does not
run it.

time: one-hand 848x480 frames of HandSceneRenderer in dataset convention (background 65535) -- what a HandPipeline's prepared
frame looks like -- labels_reduce 2, a T3/D12/C5 trained-like forest (four shapes and class 0).  Two routes to the frames'
(raw, conf), each timed by the host clock around work that ends with its result on the host, the two ALTERNATING in the same run,
for a batch of 64 frames and for one frame at a time:
  fused        ShapeVoter.classify (a fill, the pool launch, the decide launch) and the read of the [N, 4] rows
  alternative  DecisionTreeEvaluator.get_posteriors_forest(sums_out=...) into a zeroed float plane per class, a torch reduction
               (each pixel's shares floor(acc / S * 65535), summed per frame and class, the argmax and the winner's share) and the
               read of its result
and `classify_event_us`: classify alone by device events, nothing read back.  The alternative's shares are summed in int64, so its
raw classes must equal the fused route's: checked, not timed.
accuracy: a forest of the package's own trainer on a make_shape_dataset directory (424x240, the four shapes of
hand_model.SHAPES), then dataset.score_shape_model on a held-out directory of another seed: the frame accuracy of the pooled
soft vote, of the hard vote, and the confusion matrix.  Recorded, not asserted."""
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, H, W, R = 64, 480, 848, 2
T, D, C = 3, 12, 5
FOCAL, CAMERA_HEIGHT = 600., 5500.


def _host_us(torch, fn, reps, warm=3):
    """Median host time of fn(), which ends with its result on the host, in microseconds."""
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e6


def _event_us(torch, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)) * 1e3


def timing(rdf, torch):
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    r = rdf.HandSceneRenderer((H, W), (FOCAL, (W - 1) / 2., (H - 1) / 2.), max_frames=64)
    poses, index = r.model.shape_dataset_poses(N, np.random.default_rng(164))
    depth, labels = r.render(r.transforms(poses, scene.look_down_plane(CAMERA_HEIGHT, 0.1)), "fine", None, 65535, 5)
    forest = rdf.DecisionForest.from_numpy(rdf.synth.forest(T, D, C, "trained"))
    out = {"frames": [N, H, W], "labels_reduce": R, "forest": [T, D, C], "hand_pixels": round(float((labels.get() > 0).mean()), 4)}
    voter = rdf.ShapeVoter(forest, (H, W), labels_reduce=R, min_pixels=1, hold=1, max_frames=N)
    ev = rdf.DecisionTreeEvaluator()
    sums = rdf.DeviceArray((N, C, H // R, W // R), np.float32)
    sums_t = sums.torch_bytes().view(torch.float32).reshape(N, C, H // R, W // R)

    def fused(n):
        return voter.classify(depth[:n]).get()

    def alternative(n):
        sums[:n].fill(np.float32(0))
        ev.get_posteriors_forest(forest, depth[:n], None, None, sums[:n], labels_reduce=R)
        acc = sums_t[:n]
        S = acc.sum(1, keepdim=True)
        q = torch.where(S > 0, torch.floor(acc / S * 65535.0), torch.zeros_like(acc)).clamp_(0, 65535).to(torch.int64)
        pooled = q.sum((2, 3))
        best = pooled.max(1)
        conf = best.values * 65535 // pooled.sum(1).clamp(min=1)
        return torch.stack([best.indices, conf], 1).cpu().numpy()

    rows, alt = fused(N), alternative(N)
    assert rows.shape == (N, 4) and (rows[:, 0] >= 0).all()
    # (S by torch's reduction is not rule Q4's ordered sum: a share may differ by one; the pooled argmax does not on these frames)
    out["raw_equal"] = bool(np.array_equal(rows[:, 0], alt[:, 0]))
    out["conf_max_abs_diff"] = int(np.abs(rows[:, 1].astype(np.int64) - alt[:, 1]).max())
    voter.reset()
    assert np.array_equal(fused(N), rows)                                  # the same bytes from run to run, from a fresh state
    samples = {k: [] for k in ("fused_64", "alternative_64", "fused_1", "alternative_1")}
    for _ in range(5):                                                      # alternating: other work shares the machine
        samples["fused_64"].append(_host_us(torch, lambda: fused(N), 7))
        samples["alternative_64"].append(_host_us(torch, lambda: alternative(N), 7))
        samples["fused_1"].append(_host_us(torch, lambda: fused(1), 15))
        samples["alternative_1"].append(_host_us(torch, lambda: alternative(1), 15))
    for k, v in samples.items():
        out[k + "_us"] = round(float(np.median(v)), 1)
        out[k + "_us_samples"] = [round(x, 1) for x in v]
    out["fused_per_frame_us"] = round(out["fused_64_us"] / N, 2)
    out["alternative_per_frame_us"] = round(out["alternative_64_us"] / N, 2)
    out["alternative_over_fused_64"] = round(out["alternative_64_us"] / out["fused_64_us"], 2)
    out["alternative_over_fused_1"] = round(out["alternative_1_us"] / out["fused_1_us"], 2)
    out["classify_event_us_64"] = round(_event_us(torch, lambda: voter.classify(depth), 9), 1)
    out["classify_event_us_1"] = round(_event_us(torch, lambda: voter.classify(depth[:1]), 15), 1)
    out["posterior_sums_event_us_64"] = round(_event_us(torch, lambda: ev.get_posteriors_forest(forest, depth, None, None, sums, labels_reduce=R), 9), 1)
    return out


def accuracy(rdf, torch):
    ds_mod = importlib.import_module("3d-beats_amd.dataset")
    hm = importlib.import_module("3d-beats_amd.hand_model")
    h, w, focal = 240, 424, 300.
    n_train, n_test, n_held, trees, levels = 128, 32, 128, 3, 12
    shapes = tuple(hm.SHAPES)
    r = rdf.HandSceneRenderer((h, w), (focal, (w - 1) / 2., (h - 1) / 2.), max_frames=64)
    out = {"frames": [n_held, h, w], "shapes": list(shapes), "forest": [trees, levels, len(shapes) + 1], "train_frames": n_train}
    with tempfile.TemporaryDirectory() as tmp:
        train, held, model = os.path.join(tmp, "train"), os.path.join(tmp, "held"), os.path.join(tmp, "forest.npy")
        r.make_shape_dataset(train, n_train + n_test, seed=41, shapes=shapes)
        r.make_shape_dataset(held, n_held, seed=123, shapes=shapes)
        _, pct = ds_mod.train_forest(train, n_train, n_test, 128, 64, trees, levels, model, trees_to_try=trees, log=lambda *_: None,
                                     tree_seed=9)
        out["trained_pct_pixels"] = round(float(pct), 4)
        for reduce in (1, 2):
            np.random.seed(7)
            s = ds_mod.score_shape_model(model, held, n_held, labels_reduce=reduce, min_pixels=64)
            out[f"labels_reduce_{reduce}"] = {"accuracy_soft": round(s["accuracy"], 4), "accuracy_hard": round(s["accuracy_hard"], 4),
                                             "confusion_truth_by_raw_then_none": s["confusion"][1:].tolist()}
    return out


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    torch.cuda.set_device(0)
    out = {"time": timing(rdf, torch)}
    if "--time-only" not in sys.argv:
        out["accuracy"] = accuracy(rdf, torch)
    line = json.dumps({"shape": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
