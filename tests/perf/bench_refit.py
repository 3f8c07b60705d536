#!/usr/bin/env python3
"""Times the leaf refit (rdf_labels_refit_count / rdf_labels_refit_apply of librdf_labels.so, refit.LeafRefitter) on 64
two-hand 848x480 frames of HandSceneRenderer in dataset convention (background 65535, 'fine' labels: C = 8) and a T4/D20/C8
trained-like forest of synth.forest, and prints one JSON line (hipEvent times, medians after warm-up):
  add_us                   one LeafRefitter.add of the batch: every labelled pixel through every tree, counted
  eval_reference_us        the yardstick, same run, same frames and forest: DecisionTreeEvaluator(use_packed=False)
                           .get_labels_forest -- the walk over the same reference-layout records, the same nodes visited (the
                           labelled pixels are the pixels with a depth), ending in an argmax where the refit ends in atomics
  eval_packed_us           the packed path on the same frames, for scale
  add_over_eval_reference  the ratio
  apply_keep_us, apply_ancestor_us   LeafRefitter.apply with min_count 1 / 'keep' and min_count 32 / 'ancestor' (2D launches
                           against D, the read-back of the report included)
  levels                   LeafRefitter.leaf_support(): per level the reachable leaf slots, the empty ones, the pixels counted
The counts are checked by their invariant (counts.sum() == T * walked - fell_off), by a second add giving exactly twice the
first, and the apply by the report's sums.  `--out FILE` also writes the JSON there.  Standalone: bench.py does not run it."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W = 64, 480, 848
T, D, C = 4, 20, 8
FOCAL, CAMERA_HEIGHT = 600., 5500.


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
    rdf = importlib.import_module("3d-beats_amd")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    torch.cuda.set_device(0)
    out = {"frames": [N, H, W], "forest": [T, D, C]}

    r = rdf.HandSceneRenderer((H, W), (FOCAL, (W - 1) / 2., (H - 1) / 2.), max_frames=64)
    rng = np.random.default_rng(164)
    shift = np.where(np.arange(26) == 0, 1100., 0.)
    right, left = r.model.sample_poses(N, rng) + shift, r.left_model.sample_poses(N, rng) - shift
    depth, labels = r.render(r.transforms(right, scene.look_down_plane(CAMERA_HEIGHT, 0.1), left), "fine", None, 65535, 5)
    lab = labels.get()
    out["labelled"] = round(float((lab > 0).mean()), 4)
    assert int(lab.max()) < C and np.array_equal(lab > 0, depth.get() != 65535)
    del lab

    forest = rdf.DecisionForest.from_numpy(rdf.synth.forest(T, D, C, "trained"))
    refit = rdf.LeafRefitter(forest)
    refit.add(depth, labels)
    totals = refit.totals()
    first = refit.counts.get()
    assert int(first.sum()) == T * totals["walked"] - totals["fell_off"] and totals["unknown_label"] == 0
    refit.add(depth, labels)
    assert np.array_equal(refit.counts.get(), 2 * first)
    del first
    out["totals"] = totals
    out["add_us"] = round(_events(torch, lambda: refit.add(depth, labels), 15) * 1e3, 1)

    labels_out = rdf.DeviceArray((N, H, W), np.uint16).fill(65535)
    for key, packed in (("eval_reference_us", False), ("eval_packed_us", True)):
        ev = rdf.DecisionTreeEvaluator(use_packed=packed)
        for _ in range(3):
            ev.get_labels_forest(forest, depth, labels_out)
        out[key] = round(_events(torch, lambda: ev.get_labels_forest(forest, depth, labels_out), 15) * 1e3, 1)
    out["add_over_eval_reference"] = round(out["add_us"] / out["eval_reference_us"], 3)

    refit.reset().add(depth, labels)
    out["levels"] = [lv for lv in refit.leaf_support() if lv["leaf_slots"]]
    for key, args in (("apply_keep", (1, "keep")), ("apply_ancestor", (32, "ancestor"))):
        report = refit.apply(*args)
        assert report["own"] + report["ancestor"] + report["kept"] == report["leaf_slots"] == sum(lv["leaf_slots"] for lv in out["levels"])
        out[key + "_report"] = report
        out[key + "_us"] = round(_events(torch, lambda: refit.apply(*args), 10) * 1e3, 1)
    line = json.dumps({"refit": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
