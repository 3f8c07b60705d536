#!/usr/bin/env python3
"""Times the pruning (rdf_labels_prune_plan / rdf_labels_prune_apply of librdf_labels.so, prune.ForestPruner) and records what
pruning buys a forest of this repo's trainer.  Prints one JSON line; `--out FILE` also writes it there.  Standalone: bench.py
does not run it.

`--timing` (the setup of bench_refit.py: 64 two-hand 848x480 frames of HandSceneRenderer, synth.forest(4, 20, 8, "trained"),
hipEvent medians after warm-up, forest and counts put back from device copies before every timed call):
  refit_apply_ancestor_us  the yardstick, same run, same forest and counts: LeafRefitter.apply(32, 'ancestor'), the same
                           two-direction level sweep with one launch per level and direction, its report read back
  plan_us                  ForestPruner.plan(cost_per_leaf=1), the report read back
  plan_apply_us            plan + apply
  apply_us                 apply alone (by its own events inside the pair)
  ratio                    plan_apply_us / refit_apply_ancestor_us
  each as the list of `--runs` (3) measurements of one process, their median under the plain name.
`--trained` (no bar: the record is the deliverable): T4/D20/C8 trees trained by DecisionTreeTrainer on 128 such frames with
sensor noise and holes, pruned on 64 other frames, reported on 64 others for a short curve of cost_per_leaf (and two depth
limits at cost_per_leaf 1): pct. matching pixels, reachable leaf slots, depth, packed table bytes, and the time of get_labels_forest over the 64 frames, the unpruned
forest and each truncated pruned one tuned (DecisionForest.tune) on the same 32 frames."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W = 64, 480, 848
T, D, C = 4, 20, 8
FOCAL, CAMERA_HEIGHT = 600., 5500.
COSTS = (0, 1, 4, 16, 64)
LIMITS = (16, 12)                 # max_levels, each with cost_per_leaf 1: what a shallower table buys


def _events(torch, fn, reps, before=None):
    times = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)) * 1e3


def _frames(rdf, scene, renderer, n, seed, noise_amp=0, hole_rate=0.):
    rng = np.random.default_rng(seed)
    shift = np.where(np.arange(26) == 0, 1100., 0.)
    right, left = renderer.model.sample_poses(n, rng) + shift, renderer.left_model.sample_poses(n, rng) - shift
    return renderer.render(renderer.transforms(right, scene.look_down_plane(CAMERA_HEIGHT, 0.1), left), "fine", None, 65535, seed,
                           hole_rate, noise_amp)


def timing(torch, rdf, scene, renderer, runs):
    out = {"frames": [N, H, W], "forest": [T, D, C], "cost_per_leaf": 1}
    depth, labels = _frames(rdf, scene, renderer, N, 164)
    forest_np = rdf.synth.forest(T, D, C, "trained")
    forest = rdf.DecisionForest.from_numpy(forest_np)
    saved_forest = rdf.to_device(forest_np)
    pruner = rdf.ForestPruner(forest).add(depth, labels)
    refit = pruner.refitter
    saved_counts = rdf.DeviceArray(refit.counts.shape, np.uint64)
    saved_counts.copy_from(refit.counts)
    totals = pruner.totals()
    assert int(refit.counts.get().sum()) == T * totals["walked"] - totals["fell_off"]

    def restore():
        forest.forest_cu.copy_from(saved_forest)
        refit.counts.copy_from(saved_counts)
    report = pruner.plan(1)
    out["report"] = report
    pruner.apply()
    after = rdf.ForestPruner(forest)
    after.counts.copy_from(refit.counts)
    again = after.plan(1)                                    # the same plan on the result collapses nothing
    assert again["turned"] == 0 and again["leaf_slots_before"] == again["leaf_slots_after"] == report["leaf_slots_after"], again
    assert again["errors_before"] == again["errors_after"] == report["errors_after"] and again["pixels"] == report["pixels"]
    assert int(refit.counts.get().sum()) == report["pixels"]
    del after
    restore()

    apply_times = []

    def plan_apply():
        pruner.plan(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pruner.apply()
        b.record()
        apply_times.append((a, b))
    keys = ("refit_apply_ancestor_us", "plan_us", "plan_apply_us", "apply_us")
    series = {k: [] for k in keys}
    for _ in range(runs):                                      # the three alternate, as one process sees them
        for _ in range(2):
            refit.apply(32, "ancestor")
        series["refit_apply_ancestor_us"].append(round(_events(torch, lambda: refit.apply(32, "ancestor"), 10), 1))
        restore()
        for _ in range(2):
            pruner.plan(1)
        series["plan_us"].append(round(_events(torch, lambda: pruner.plan(1), 10), 1))
        plan_apply()
        del apply_times[:]
        series["plan_apply_us"].append(round(_events(torch, plan_apply, 10, before=restore), 1))
        torch.cuda.synchronize()
        series["apply_us"].append(round(float(np.median([a.elapsed_time(b) for a, b in apply_times])) * 1e3, 1))
        restore()
    for k in keys:
        out[k + "_runs"] = series[k]
        out[k] = float(np.median(series[k]))
    out["ratio_runs"] = [round(p / r, 3) for p, r in zip(series["plan_apply_us"], series["refit_apply_ancestor_us"])]
    out["ratio"] = round(out["plan_apply_us"] / out["refit_apply_ancestor_us"], 3)
    return out


class _DeviceDataset:
    """What DecisionTreeTrainer asks of a dataset, over frames that are on the device already."""

    def __init__(self, depth, labels, n_classes):
        self.depth, self.labels, self._c = depth, labels, n_classes
        self.num_images = self.images_per_block = depth.shape[0]
        self.img_dims = (depth.shape[2], depth.shape[1])

    def num_classes(self):
        return self._c

    def images_shape(self):
        return self.depth.shape

    def get_depth_block_cu(self, b, arr):
        arr.copy_from(self.depth)

    def get_labels_block_cu(self, b, arr):
        arr.copy_from(self.labels)


def trained(torch, rdf, scene, renderer, n_train, proposals):
    out = {"train_frames": n_train, "prune_frames": N, "report_frames": N, "forest": [T, D, C], "proposals": proposals,
           "noise_amp": 8, "hole_rate": 0.02}
    big = rdf.HandSceneRenderer((H, W), (FOCAL, (W - 1) / 2., (H - 1) / 2.), max_frames=n_train) if n_train > N else renderer
    train_d, train_l = _frames(rdf, scene, big, n_train, 1001, 8, 0.02)
    prune_d, prune_l = _frames(rdf, scene, renderer, N, 2002, 8, 0.02)
    test_d, test_l = _frames(rdf, scene, renderer, N, 3003, 8, 0.02)
    ds = _DeviceDataset(train_d, train_l, C)
    trainer = rdf.DecisionTreeTrainer(n_train, proposals)
    trainer.allocate(ds, proposals, D)
    tree = rdf.DecisionTree(D, C)
    forest_np = np.zeros((T, (1 << D) - 1, 7 + 2 * C), np.float32)
    t0 = time.perf_counter()
    for k in range(T):
        np.random.seed(1000 + k)
        trainer.train(ds, tree)
        forest_np[k] = tree.tree_out_cu.get()
    out["train_seconds"] = round(time.perf_counter() - t0, 2)
    del trainer, ds, train_d, train_l
    ev, scorer = rdf.DecisionTreeEvaluator(), rdf.LabelScorer(C)
    labels_out = rdf.DeviceArray((N, H, W), np.uint16)

    def measure(forest):
        tune = forest.tune(test_d[0:32])
        for _ in range(3):
            ev.get_labels_forest(forest, test_d, labels_out)
        us = _events(torch, lambda: ev.get_labels_forest(forest, test_d, labels_out), 15)
        labels_out.fill(65535)
        ev.get_labels_forest(forest, test_d, labels_out)
        score = scorer.reset().add(labels_out, test_l).result()
        return {"eval_us": round(us, 1), "deep_from": tune["deep_from"], "table_bytes": int(forest.packed().nbytes),
                "pct_matching": round(float(score.pct_matching), 5), "depth": int(forest.max_depth)}
    out["unpruned"] = measure(rdf.DecisionForest.from_numpy(forest_np))
    curve = []
    for cost, limit in [(c, None) for c in COSTS] + [(1, m) for m in LIMITS]:
        forest = rdf.DecisionForest.from_numpy(forest_np)
        pruner = rdf.ForestPruner(forest).add(prune_d, prune_l)
        report = pruner.plan(cost, 0, limit)
        pruner.apply()
        small = pruner.truncated()
        row = {"cost_per_leaf": cost, "max_levels": limit or D, "report": report}
        row.update(measure(small))
        row["eval_over_unpruned"] = round(row["eval_us"] / out["unpruned"]["eval_us"], 3)
        curve.append(row)
        del pruner, forest, small
    out["curve"] = curve
    return out


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    torch.cuda.set_device(0)
    args = sys.argv[1:]
    both = "--timing" not in args and "--trained" not in args
    runs = int(args[args.index("--runs") + 1]) if "--runs" in args else 3
    n_train = int(args[args.index("--train-frames") + 1]) if "--train-frames" in args else 128
    proposals = int(args[args.index("--proposals") + 1]) if "--proposals" in args else 256
    renderer = rdf.HandSceneRenderer((H, W), (FOCAL, (W - 1) / 2., (H - 1) / 2.), max_frames=64)
    out = {}
    if both or "--timing" in args:
        out["timing"] = timing(torch, rdf, scene, renderer, runs)
    if both or "--trained" in args:
        out["trained"] = trained(torch, rdf, scene, renderer, n_train, proposals)
    line = json.dumps({"prune": out})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
