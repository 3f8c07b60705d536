#!/usr/bin/env python3
"""Times the forest posterior (rdf_labels_forest_posterior of librdf_labels.so, DecisionTreeEvaluator.get_posteriors_forest) on
the frames and forest of bench_refit.py -- 64 two-hand 848x480 frames of HandSceneRenderer in dataset convention (background
65535) and a T4/D20/C8 trained-like forest of synth.forest -- and prints one JSON line (hipEvent times, medians after warm-up):
  posterior_labels_us, posterior_labels_conf_us, posterior_all_us
                           one get_posteriors_forest of the batch with the label map alone, with the confidence map too, and
                           with the C planes of sums as well
  eval_reference_us        the yardstick, same run, same frames and forest: DecisionTreeEvaluator(use_packed=False)
                           .get_labels_forest -- the walk over the same reference-layout records, ending in the argmax alone
  eval_packed_us           the packed default on the same frames, for scale
  labels_over_eval_reference   posterior_labels_us / eval_reference_us
  confidence_counts_us     one ConfidenceScorer.add of the batch's maps against its truth, 64 bins
  layered_fused_us, layered_gated_us
                           ONE 848x480 frame through a two-layer stack of HandModel.layered_config's shape (T4/D16, C = 4 and
                           C = 6) at labels_reduce 2: the fused run() of a plain stack next to run() with min_conf = (0, 0), the
                           step-by-step gated path (fills, one posterior launch a layer, the composite)
The ungated label map is checked against get_labels_forest's bytes and the gated composite against the fused one.
`--out FILE` also writes the JSON there.  Standalone: bench.py does not run it."""
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
    depth, truth = r.render(r.transforms(right, scene.look_down_plane(CAMERA_HEIGHT, 0.1), left), "fine", None, 65535, 5)
    out["evaluated"] = round(float((depth.get() != 65535).mean()), 4)

    forest = rdf.DecisionForest.from_numpy(rdf.synth.forest(T, D, C, "trained"))
    labels = rdf.DeviceArray((N, H, W), np.uint16).fill(65535)
    conf = rdf.DeviceArray((N, H, W), np.uint16).fill(0)
    sums = rdf.DeviceArray((N, C, H, W), np.float32).fill(np.float32(0.))
    ev = rdf.DecisionTreeEvaluator()
    for key, args in (("posterior_labels_us", (labels, None, None)), ("posterior_labels_conf_us", (labels, conf, None)),
                      ("posterior_all_us", (labels, conf, sums))):
        for _ in range(3):
            ev.get_posteriors_forest(forest, depth, *args)
        out[key] = round(_events(torch, lambda: ev.get_posteriors_forest(forest, depth, *args), 15) * 1e3, 1)
    got = labels.get()

    labels_ref = rdf.DeviceArray((N, H, W), np.uint16).fill(65535)
    for key, packed in (("eval_reference_us", False), ("eval_packed_us", True)):
        e = rdf.DecisionTreeEvaluator(use_packed=packed)
        for _ in range(3):
            e.get_labels_forest(forest, depth, labels_ref)
        out[key] = round(_events(torch, lambda: e.get_labels_forest(forest, depth, labels_ref), 15) * 1e3, 1)
        assert np.array_equal(labels_ref.get(), got), key
    del got
    out["labels_over_eval_reference"] = round(out["posterior_labels_us"] / out["eval_reference_us"], 3)

    scorer = rdf.ConfidenceScorer(64)
    scorer.add(labels, conf, truth)
    cal = scorer.result()
    assert sum(cal.count_by_bin) == cal.labelled - cal.unclassified and cal.labelled > 0
    out["confidence_counts_us"] = round(_events(torch, lambda: scorer.add(labels, conf, truth), 15) * 1e3, 1)

    # one live frame through a two-layer stack, labels_reduce 2
    coarse = rdf.DecisionForest.from_numpy(rdf.synth.forest(4, 16, 4, "trained", 60))
    tips = rdf.DecisionForest.from_numpy(rdf.synth.forest(4, 16, 6, "trained", 70))
    cfg = rdf.HandModel.layered_config(coarse, tips)
    plain, gated = rdf.LayeredDecisionForest(cfg, (H, W), 2), rdf.LayeredDecisionForest(cfg, (H, W), 2)
    gated.min_conf = (0, 0)
    frame = rdf.GpuBuffer((H, W), np.uint16)
    frame.cu().copy_from(depth[0])
    comp = {}
    for key, stack in (("layered_fused_us", plain), ("layered_gated_us", gated)):
        buf = rdf.GpuBuffer((H // 2, W // 2), np.uint16)
        for _ in range(3):
            stack.run(frame, buf, 1.0)
        out[key] = round(_events(torch, lambda: stack.run(frame, buf, 1.0), 25) * 1e3, 1)
        comp[key] = buf.cu().get()
    assert np.array_equal(comp["layered_fused_us"], comp["layered_gated_us"]) and (comp["layered_fused_us"] != 65535).any()

    line = json.dumps({"posterior": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
