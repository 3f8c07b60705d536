#!/usr/bin/env python3
"""Times the voted fingertips (HandPipeline(joint_voter=...): JointVoter.vote and rdf_labels_vote_tips behind the chain) and
records what they buy, and prints one JSON line.  `--out FILE` also writes it there; `--time-only` skips the second part.
Standalone: bench.py does not run it.

time: 64 two-hand 848x480 frames of HandSceneRenderer as the camera delivers them (0 = no reading) with full-resolution group
images (1: the right hand, 2: the left), the two-layer stack of the pipeline tests, a vote table fitted to the stack's first
forest on the same frames with min_count 1 and no spread limit (the densest table that forest can have).  One sample is both hands' HandPipeline.enqueue_batch of the 64 frames (the left hand mirrored), with
the voter and without, ALTERNATING in one run; hipEvent medians after warm-up.  The voter-off pipeline runs the code a pipeline
built without the argument runs: that is the baseline.
  batch_off_us, batch_on_us, batch_added_us_per_hand_frame    the same for one frame through enqueue(): single_*
  vote_us       JointVoter.vote of one hand's 64 prepared frames alone (the clear, the cast, the modes)
  clear_us      a memset of the voter's workspace alone
  empty_vote_us vote of 64 frames without a pixel (every wave of the cast leaves at once): the clear and the modes
  cast_us = vote_us - empty_vote_us, modes_us = empty_vote_us - clear_us: by difference, not by a trace
  tips_us       rdf_labels_vote_tips of the 64 frames alone
effect: bench_joint_votes.py's set-up -- a T3/D12/C8 forest of the package's trainer on 424x240 'fine' renders, the table fitted
on 256 further frames, 128 held-out frames, clean and through StereoSensor.  Labels, the mean-shift modes, the cast, then
rdf_labels_vote_tips per policy: per tip the frames with a height, the median and 90th-percentile pixel error of the chosen pixel
against the true tip's projection and of the height against the true tip's height above the plane (depth units), the share of
each source code, and how many tips the label route left NaN that now have a height.  `guard` is swept over tip_max_dist 2..32
and every policy over tip_z_tol a decade either side of 100.  best_tip_max_dist: the guard setting with the lowest mean (over the
tips) median pixel error on the stereo frames; best_tip_z_tol: the lowest mean median height error under 'votes' there (ties: the
smaller).  Recorded, not asserted."""
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, H, W, R = 64, 480, 848, 2
FOCAL, CAMERA_HEIGHT = 600., 5500.
VARIANCES = (50., 8., 8., 8., 8., 8., 8.)
ROUNDS = 6
MAX_DISTS = (2, 4, 8, 16, 32)
Z_TOLS = (10, 22, 46, 100, 215, 464, 1000)
POLICIES = {"fill": 0, "guard": 1, "votes": 2}


def _median_us(torch, fn, reps, inner=1):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return round(float(np.median(times)) * 1e3, 1)


def _stack(rdf):
    synth = rdf.synth
    f0, f1 = synth.forest(3, 9, 4, "trained", 60), synth.forest(3, 10, 5, "trained", 70)
    cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                      {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
           "conditions": [[0, 1], [0, 2], [1, 3], [0, 3], [0, 4], [0, 5], [0, 6], [0, 7]],
           "label_colors": [[10 * i, 255 - 10 * i, i, 255] for i in range(1, 8)]}
    return rdf.LayeredDecisionForest(cfg, (H, W), R), f0


def time_cost(rdf, torch):
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    pl = importlib.import_module("3d-beats_amd.pipeline")
    r = rdf.HandSceneRenderer((H, W), (FOCAL, (W - 1) / 2., (H - 1) / 2.), max_frames=64)
    rng = np.random.default_rng(164)
    shift = np.where(np.arange(26) == 0, 1100., 0.)
    right, left = r.model.sample_poses(N, rng) + shift, r.left_model.sample_poses(N, rng) - shift
    plane = scene.look_down_plane(CAMERA_HEIGHT, 0.1)
    both, labels = r.render(r.transforms(right, plane, left), "fine", None, 65535, 5)
    alone, _ = r.render(r.transforms(right, plane), "fine", None, 65535, 5)
    both_np, alone_np = both.get(), alone.get()
    cams = np.where(both_np == 65535, 0, both_np).astype(np.uint16)
    groups = np.where(cams == 0, 0, np.where(both_np == alone_np, 1, 2)).astype(np.uint16)
    out = {"frames": [N, H, W], "hand_pixels": [round(float((groups == g).mean()), 4) for g in (1, 2)]}

    stack, f0 = _stack(rdf)
    forest = rdf.DecisionForest.from_numpy(f0)
    targets = r.fingertip_targets(right, plane)
    # every leaf slot that saw a pixel votes (min_count 1, no spread limit): the densest table this forest can have, so the
    # cast is not timed on the handful of votes the default fit leaves of an untrained forest
    table = rdf.VoteFitter(forest, 5).add(both, labels, targets).fit(1, 1 << 38)
    out["table"] = table.report
    intr = (FOCAL, FOCAL, (W - 1) / 2., (H - 1) / 2.)
    args = ((H, W), R, 1.0, ROUNDS, list(VARIANCES), [3, 4, 5, 6, 7], intr, plane.astype(np.float32))

    def pipes(voter):
        kw = {} if voter is None else dict(joint_voter=voter, tip_policy="votes")
        return [pl.HandPipeline(stack, *args, depth_mm_level=0, **kw) for _ in range(2)]
    off, on = pipes(None), pipes(rdf.JointVoter(forest, table, (H, W), labels_reduce=R, max_frames=N))
    cams_cu, groups_cu = rdf.to_device(cams), rdf.to_device(groups)
    log = rdf.DeviceArray((N, 10), np.float64)

    def batch(ps):
        ps[0].enqueue_batch(cams_cu, groups_cu, 1, False, cams_cu, log.ptr, 10)
        ps[1].enqueue_batch(cams_cu, groups_cu, 2, True, cams_cu, log.ptr + 40, 10)
    frame = [rdf.GpuBuffer((H, W), np.uint16, a[0]) for a in (cams, groups)]

    def single(ps):
        ps[0].enqueue(frame[0], frame[1], 1, False)
        ps[1].enqueue(frame[0], frame[1], 2, True)
    for fn in (batch, single):
        for _ in range(3):
            fn(off)
            fn(on)
    t = {"batch_off": [], "batch_on": [], "single_off": [], "single_on": []}
    for _ in range(9):                                      # alternating: both see the same clocks and the same neighbours
        t["batch_off"].append(_median_us(torch, lambda: batch(off), 1))
        t["batch_on"].append(_median_us(torch, lambda: batch(on), 1))
        t["single_off"].append(_median_us(torch, lambda: single(off), 1, 10))
        t["single_on"].append(_median_us(torch, lambda: single(on), 1, 10))
    for k, v in t.items():
        out[k + "_us"] = round(float(np.median(v)), 1)
        out[k + "_us_samples"] = v
    out["batch_added_us_per_hand_frame"] = round((out["batch_on_us"] - out["batch_off_us"]) / (2 * N), 2)
    out["single_added_us_per_hand_frame"] = round((out["single_on_us"] - out["single_off_us"]) / 2, 1)
    out["batch_on_over_off"] = round(out["batch_on_us"] / out["batch_off_us"], 3)
    tips = on[0].tips_batch.get()
    out["sources_right_hand"] = [int((tips[..., 3] == s).sum()) for s in range(4)]

    # the pieces, one hand's 64 prepared frames
    p = on[0]
    prepared, joints = p._depth_batch[:N], p.joints_batch
    empty = rdf.DeviceArray((N, H, W), np.uint16).fill(65535)
    ws = p.joint_voter._workspace
    out["workspace_bytes"] = int(ws.nbytes)
    pieces = {"vote": lambda: p._vote(prepared, joints), "empty_vote": lambda: p._vote(empty, joints), "clear": lambda: ws.fill(0),
              "tips": lambda: p._vote_tips(N, p.means_batch.ptr, joints, False, cams_cu.ptr, log.ptr, 10, p.tips_batch)}
    samples = {k: [] for k in pieces}
    for _ in range(9):
        for k, fn in pieces.items():
            samples[k].append(_median_us(torch, fn, 1, 5))
    p._vote(prepared, joints)
    for k, v in samples.items():
        out[k + "_us"] = round(float(np.median(v)), 1)
    out["cast_us"] = round(out["vote_us"] - out["empty_vote_us"], 1)
    out["modes_us"] = round(out["empty_vote_us"] - out["clear_us"], 1)
    return out


def _stats(e):
    return (round(float(np.median(e)), 2), round(float(np.percentile(e, 90)), 2)) if len(e) else (None, None)


def _tips_call(rdf, lb, dev, n, L, h, w, intr, policy, max_dist, z_tol, heights, tips):
    rc = lb.rdf_labels_vote_tips(dev["means"].ptr, n, L, dev["ids"].ptr, dev["tip_joints"].ptr, 5, dev["joints"].ptr, 5, 0, dev["depth"].ptr,
                                 w, h, 1, *intr, dev["plane"].ptr, policy, max_dist, z_tol, heights.ptr, 5, tips.ptr, rdf.get_runtime().stream())
    assert rc == 0, rc
    heights.mark_dirty()
    tips.mark_dirty()
    return heights.get(), tips.get()


def effect(rdf, torch):
    ds_mod = importlib.import_module("3d-beats_amd.dataset")
    scene = importlib.import_module("3d-beats_amd.hand_scene")
    lb = importlib.import_module("3d-beats_amd._lib").load("labels")
    h, w, focal = 240, 424, 300.
    cam = (focal, (w - 1) / 2., (h - 1) / 2.)
    intr = (focal, focal, cam[1], cam[2])
    n_train, n_test, n_fit, n_eval, trees, levels, L = 64, 16, 256, 128, 3, 12, 7
    r = rdf.HandSceneRenderer((h, w), cam, max_frames=64)
    sensor = rdf.StereoSensor((h, w), cam, max_disparity=64, max_frames=64)
    plane = scene.look_down_plane(550. * r.model.units_per_mm)
    with tempfile.TemporaryDirectory() as tmp:
        r.make_dataset(tmp, n_train + n_test, seed=41, labels="fine", plane=plane)
        forest_np, pct = ds_mod.train_forest(tmp, n_train, n_test, 128, 64, trees, levels, None, trees_to_try=trees,
                                             log=lambda *_: None, tree_seed=9)
    forest = rdf.DecisionForest.from_numpy(forest_np)
    out = {"frames": [n_eval, h, w], "forest": [trees, levels, 8], "trained_pct": round(float(pct), 4), "fit_frames": n_fit,
           "max_dists": list(MAX_DISTS), "z_tols": list(Z_TOLS), "kinds": {}}
    ev, wm = rdf.DecisionTreeEvaluator(), rdf.WeightedModes()
    var = rdf.to_device(np.array(VARIANCES, np.float32))
    inv = np.linalg.inv(plane)
    for kind, sens in (("clean", None), ("stereo", sensor)):
        poses = r.model.sample_poses(n_fit, np.random.default_rng(77))
        depth, labels = r.render(r.transforms(poses, plane), "fine", None, 65535, 77, sensor=sens)
        table = rdf.VoteFitter(forest, 5).add(depth, labels, r.fingertip_targets(poses, plane)).fit()
        poses = r.model.sample_poses(n_eval, np.random.default_rng(123))
        depth, _ = r.render(r.transforms(poses, plane), "fine", None, 65535, 123, sensor=sens)
        tip = r.model.fingertips(poses, inv)
        want_px = np.stack([focal * tip[..., 0] / tip[..., 2] + cam[1], focal * tip[..., 1] / tip[..., 2] + cam[2]], -1)
        tip_h = np.concatenate([tip, np.ones(tip.shape[:2] + (1,))], -1)
        want_h = -(tip_h @ np.asarray(plane, np.float64)[2])
        lab = rdf.DeviceArray((n_eval, h, w), np.uint16).fill(65535)
        ev.get_labels_forest(forest, depth, lab)
        means = wm.run_device(ROUNDS, lab, None, L, var)
        joints = rdf.JointVoter(forest, table, (h, w), max_frames=n_eval).vote(depth)
        dev = {"means": means, "joints": joints, "depth": depth, "ids": rdf.to_device(np.array([3, 4, 5, 6, 7], np.int32)),
               "tip_joints": rdf.to_device(np.arange(5, dtype=np.int32)), "plane": rdf.to_device(np.asarray(plane, np.float32))}
        heights, tips = rdf.DeviceArray((n_eval, 5), np.float64), rdf.DeviceArray((n_eval, 5, 4), np.int32)

        def measure(dev, policy, max_dist, z_tol, parent=None):
            hs, ts = _tips_call(rdf, lb, dev, n_eval, L, h, w, intr, POLICIES[policy], max_dist, z_tol, heights, tips)
            per_tip = []
            for f in range(5):
                ok = ts[:, f, 3] > 0
                e_px = np.hypot(ts[ok, f, 0] + 0.5 - want_px[ok, f, 0], ts[ok, f, 1] + 0.5 - want_px[ok, f, 1])
                e_h = np.abs(hs[ok, f] - want_h[ok, f])
                (mp, pp), (mh, ph) = _stats(e_px), _stats(e_h)
                per_tip.append({"found": int(ok.sum()), "median_px": mp, "p90_px": pp, "median_height": mh, "p90_height": ph})
            res = {"tips": per_tip, "sources": [round(float((ts[..., 3] == s).mean()), 4) for s in range(4)]}
            if parent is not None:
                res["filled"] = int((np.isnan(parent) & np.isfinite(hs)).sum())
            return res, hs
        # the label route alone: FILL with votes that never apply is what the mode launch writes; here: no joint has support
        none = rdf.DeviceArray((n_eval, 5, 4), np.int32).fill(0)
        dev_plain = dict(dev, joints=none)
        parent_h, _ = _tips_call(rdf, lb, dev_plain, n_eval, L, h, w, intr, 0, 0, 0, heights, tips)
        res = {"table": table.report, "label_route_nan": int(np.isnan(parent_h).sum()), "policies": {}}
        res["label_route"], _ = measure(dev_plain, "fill", 0, 0)
        for policy in POLICIES:
            runs = {}
            for md in (MAX_DISTS if policy == "guard" else (8,)):
                for zt in Z_TOLS:
                    runs[f"{md},{zt}"], _ = measure(dev, policy, md, zt, parent_h)
            res["policies"][policy] = runs
        out["kinds"][kind] = res

    def mean_of(run, key):
        v = [t[key] for t in run["tips"]]
        return float(np.mean(v)) if all(x is not None for x in v) else float("inf")
    stereo = out["kinds"]["stereo"]["policies"]
    by_md = {md: min(mean_of(stereo["guard"][f"{md},{zt}"], "median_px") for zt in Z_TOLS) for md in MAX_DISTS}
    by_zt = {zt: mean_of(stereo["votes"][f"8,{zt}"], "median_height") for zt in Z_TOLS}
    out["mean_median_px_by_max_dist"] = {str(k): round(v, 3) for k, v in by_md.items()}
    out["mean_median_height_by_z_tol"] = {str(k): round(v, 2) for k, v in by_zt.items()}
    out["best_tip_max_dist"] = min(MAX_DISTS, key=lambda k: (by_md[k], k))
    out["best_tip_z_tol"] = min(Z_TOLS, key=lambda k: (by_zt[k], k))
    return out


def main():
    import torch
    rdf = importlib.import_module("3d-beats_amd")
    torch.cuda.set_device(0)
    out = {"time": time_cost(rdf, torch)}
    if "--time-only" not in sys.argv:
        out["effect"] = effect(rdf, torch)
    line = json.dumps({"vote_tips": out})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
