#!/usr/bin/env python3
"""Times the joint votes (rdf_labels_votes_count / _fit / _cast of librdf_labels.so; joint_votes.VoteFitter and JointVoter) and
records what they buy, and prints one JSON line.  `--out FILE` also writes it there; `--cost-only` skips the second part.
Standalone: bench.py does not run it.

cost: 64 two-hand 848x480 frames of HandSceneRenderer in dataset convention (background 65535), the ten fingertips of
fingertip_targets, the T4/D20/C8 trained-like forest of bench_refit.py.  hipEvent times, medians after warm-up, per call:
  add_us        one VoteFitter.add of the batch (one launch)
  fit_us        one VoteFitter.fit (a memset, one launch, the read-back of the report)
  vote_us       one JointVoter.vote of the batch (a clear, the vote launch, the mode launch), cells of 4 pixels, box 1
  posterior_us  DecisionTreeEvaluator.get_posteriors_forest on the same frames and forest (labels and confidence): the same
                walk of the same pixels without the scatter
  vote_over_posterior, and the totals, the fit's report and how many joints got a position.
effect: a forest of the package's own trainer on rendered 'fine' frames (424x240), votes fitted on further frames, then held-out
frames, clean and through StereoSensor.  Per fingertip: how many frames give a position, and the median and 90th-percentile
distance in pixels from the true tip's projection -- for the voter at every max_var of the sweep, and for the existing route
beside it (the forest's labels, then the mean-shift mode of the tip's class).  `best_max_var`: the sweep's lowest mean (over
the tips and both kinds of frame) median error among the settings that find at least 99 % of what the most generous one
finds.  Recorded, not asserted."""
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, H, W = 64, 480, 848
T, D, C = 4, 20, 8
FOCAL, CAMERA_HEIGHT = 600., 5500.
SWEEP = [4 ** k for k in range(7, 14)] + [1 << 38]
VARIANCES = (50., 8., 8., 8., 8., 8., 8.)       # bench_soft_modes.py's: palm, finger, the five tips
ROUNDS = 6


def _events(torch, fn, reps, warm=3):
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
    return float(np.median(times))


def cost(rdf, torch):
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    out = {"frames": [N, H, W], "forest": [T, D, C], "joints": 10}
    r = rdf.HandSceneRenderer((H, W), (FOCAL, (W - 1) / 2., (H - 1) / 2.), max_frames=64)
    rng = np.random.default_rng(164)
    shift = np.where(np.arange(26) == 0, 1100., 0.)
    right, left = r.model.sample_poses(N, rng) + shift, r.left_model.sample_poses(N, rng) - shift
    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    depth, labels = r.render(r.transforms(right, plane, left), "fine", None, 65535, 5)
    targets = rdf.to_device(r.fingertip_targets(right, plane, left))
    out["hand_pixels"] = round(float((labels.get() > 0).mean()), 4)

    forest = rdf.DecisionForest.from_numpy(rdf.synth.forest(T, D, C, "trained"))
    fitter = rdf.VoteFitter(forest, 10)
    fitter.add(depth, labels, targets)
    first, totals = fitter.sums.get(), fitter.totals()
    assert int(first[..., 0].sum()) == totals["offsets"] and totals["offsets"] <= T * 10 * totals["walked"]
    fitter.add(depth, labels, targets)
    assert np.array_equal(fitter.sums.get(), first + first)              # integers: twice the batch is twice the sums
    del first
    out["totals"] = totals
    out["add_us"] = round(_events(torch, lambda: fitter.add(depth, labels, targets), 7, 1) * 1e3, 1)
    fitter.reset().add(depth, labels, targets)
    table = fitter.fit()
    out["report"] = table.report
    assert table.report["votes"] + table.report["dropped_support"] + table.report["dropped_spread"] == 10 * table.report["leaf_slots"]
    out["fit_us"] = round(_events(torch, lambda: fitter.fit(), 7, 1) * 1e3, 1)

    voter = rdf.JointVoter(forest, table, (H, W), max_frames=N)
    joints = rdf.DeviceArray((N, 10, 4), np.int32)
    voter.vote(depth, out=joints)
    again = joints.get()
    voter.vote(depth, out=joints)
    assert np.array_equal(joints.get(), again)                           # the same bytes from run to run
    out["joints_found"] = int((again[..., 3] > 0).sum())
    ev = rdf.DecisionTreeEvaluator()
    lab, conf = (rdf.DeviceArray((N, H, W), np.uint16).fill(v) for v in (65535, 0))
    samples = {"vote": [], "posterior": []}
    for _ in range(5):                                                    # alternating: other work shares the machine
        samples["vote"].append(_events(torch, lambda: voter.vote(depth, out=joints), 5, 2))
        samples["posterior"].append(_events(torch, lambda: ev.get_posteriors_forest(forest, depth, lab, conf), 5, 2))
    out["vote_us"] = round(float(np.median(samples["vote"])) * 1e3, 1)
    out["posterior_us"] = round(float(np.median(samples["posterior"])) * 1e3, 1)
    out["vote_us_samples"] = [round(v * 1e3, 1) for v in samples["vote"]]
    out["posterior_us_samples"] = [round(v * 1e3, 1) for v in samples["posterior"]]
    out["vote_over_posterior"] = round(out["vote_us"] / out["posterior_us"], 3)
    return out


def _errors(xy, found, want):
    """Per tip: frames with a position, median and p90 distance in pixels."""
    out = []
    for f in range(5):
        ok = found[:, f]
        e = np.hypot(xy[ok, f, 0] - want[ok, f, 0], xy[ok, f, 1] - want[ok, f, 1])
        out.append({"found": int(ok.sum()), "median_px": round(float(np.median(e)), 2) if ok.any() else None,
                    "p90_px": round(float(np.percentile(e, 90)), 2) if ok.any() else None})
    return out


def effect(rdf, torch):
    ds_mod = importlib.import_module("3d-beats_amd.dataset")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    h, w, focal = 240, 424, 300.
    cam = (focal, (w - 1) / 2., (h - 1) / 2.)
    n_train, n_test, n_fit, n_eval, trees, levels = 64, 16, 256, 128, 3, 12
    r = rdf.HandSceneRenderer((h, w), cam, max_frames=64)
    sensor = rdf.StereoSensor((h, w), cam, max_disparity=64, max_frames=64)
    plane = scene.look_down_plane(550. * r.model.units_per_mm)
    with tempfile.TemporaryDirectory() as tmp:
        r.make_dataset(tmp, n_train + n_test, seed=41, labels="fine", plane=plane)
        forest_np, pct = ds_mod.train_forest(tmp, n_train, n_test, 128, 64, trees, levels, None, trees_to_try=trees,
                                             log=lambda *_: None, tree_seed=9)
    forest = rdf.DecisionForest.from_numpy(forest_np)
    out = {"frames": [n_eval, h, w], "forest": [trees, levels, 8], "trained_pct": round(float(pct), 4), "fit_frames": n_fit,
           "sweep": SWEEP, "kinds": {}}
    ev, wm = rdf.DecisionTreeEvaluator(), rdf.WeightedModes()
    var = rdf.to_device(np.array(VARIANCES, np.float32))
    inv = np.linalg.inv(plane)
    score = {v: [] for v in SWEEP}
    for kind, sens in (("clean", None), ("stereo", sensor)):
        poses = r.model.sample_poses(n_fit, np.random.default_rng(77))
        depth, labels = r.render(r.transforms(poses, plane), "fine", None, 65535, 77, sensor=sens)
        fitter = rdf.VoteFitter(forest, 5).add(depth, labels, r.fingertip_targets(poses, plane))
        poses = r.model.sample_poses(n_eval, np.random.default_rng(123))
        depth, _ = r.render(r.transforms(poses, plane), "fine", None, 65535, 123, sensor=sens)
        tip = r.model.fingertips(poses, inv)
        want = np.stack([focal * tip[..., 0] / tip[..., 2] + cam[1], focal * tip[..., 1] / tip[..., 2] + cam[2]], -1)
        res = {"fit_totals": fitter.totals(), "votes": {}}
        for max_var in SWEEP:
            table = fitter.fit(8, max_var)
            x, y, _, support = rdf.JointVoter.to_float(rdf.JointVoter(forest, table, (h, w), max_frames=n_eval).vote(depth))
            res["votes"][str(max_var)] = {"report": table.report, "tips": _errors(np.stack([x, y], -1), support > 0, want)}
        # the existing route: the forest's labels, then the mean-shift mode of the tip's class (3..7); a pixel's centre at +0.5
        lab = rdf.DeviceArray((n_eval, h, w), np.uint16).fill(65535)
        ev.get_labels_forest(forest, depth, lab)
        modes = wm.run(ROUNDS, lab, None, 7, var)[:, 2:] + 0.5
        res["labels_then_mean_shift"] = _errors(modes, np.isfinite(modes).all(-1), want)
        out["kinds"][kind] = res
        most = max(sum(t["found"] for t in v["tips"]) for v in res["votes"].values())
        for max_var in SWEEP:
            tips = res["votes"][str(max_var)]["tips"]
            if sum(t["found"] for t in tips) >= 0.99 * most and all(t["median_px"] is not None for t in tips):
                score[max_var].append(float(np.mean([t["median_px"] for t in tips])))
    full = {v: float(np.mean(s)) for v, s in score.items() if len(s) == 2}
    out["best_max_var"] = min(full, key=full.get) if full else None
    out["mean_median_px_by_max_var"] = {str(v): round(s, 3) for v, s in full.items()}
    return out


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    torch.cuda.set_device(0)
    out = {"cost": cost(rdf, torch)}
    if "--cost-only" not in sys.argv:
        out["effect"] = effect(rdf, torch)
    line = json.dumps({"joint_votes": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
