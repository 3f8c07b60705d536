#!/usr/bin/env python3
"""Frames per second of BeatsSession.run_sequence(dev) and run_sequence(dev, batched=True) for max_frames 8, 16 and 32, at
240 x 424 (the frames and forests of tests/perf/bench_session.py) and at the app's 480 x 848 (the same frames, every pixel
doubled).  One process, one device; every call ends in its one synchronisation; device events bracket the same work as a
check on the host clock.  Prints one JSON line.

    python tests/perf/bench_session_batch.py [--frames 240] [--repeat 5]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-frames", type=int, nargs="+", default=[8, 16, 32])
    args = ap.parse_args()
    import torch        # (before the package, as the other scripts here do: the HIP runtime that gets loaded is torch's)
    import session_cases as sc
    rdf = importlib.import_module("3d-beats_amd")
    torch.cuda.set_device(0)
    base, (focal, ppx, ppy) = sc.frames()
    small = np.stack([base[k % sc.FRAMES] for k in range(args.frames)])
    f0, f1, conditions, colors = sc.forest_config(rdf)

    def stack(dims):
        cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                          {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
               "conditions": conditions, "label_colors": colors}
        return rdf.LayeredDecisionForest(cfg, dims, 2)

    def timed(fn):
        fn()                                        # warm-up (and the batch buffers' allocation)
        host, device, n_events = [], [], 0
        for _ in range(args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t = time.perf_counter()
            n_events = len(fn())
            host.append(time.perf_counter() - t)
            e1.record()
            e1.synchronize()
            device.append(e0.elapsed_time(e1) / 1e3)
        return {"frames_per_s": round(args.frames / min(host), 1),
                "frames_per_s_median": round(args.frames / sorted(host)[len(host) // 2], 1),
                "frames_per_s_by_device_events": round(args.frames / min(device), 1), "events": n_events}

    out = {}
    # a pixel (x, y) of the doubled frame looks along the ray of pixel (x // 2, y // 2) of the small one
    big = np.repeat(np.repeat(small, 2, axis=1), 2, axis=2)
    for frames, intr in ((small, (focal, ppx, ppy)), (big, (2 * focal, 2 * ppx + 0.5, 2 * ppy + 0.5))):
        H, W = frames.shape[1:]
        dev = rdf.to_device(frames)
        plane, res = None, {}
        for mf in args.max_frames:
            session = rdf.BeatsSession(stack((H, W)), (H, W), intr, num_random_guesses=4000, seed=3, max_frames=mf)
            if plane is None:
                plane = session.calibrate(frames[0])
            session.set_plane(plane)
            res[f"max_frames_{mf}"] = {"frame_by_frame": timed(lambda: session.run_sequence(dev)[0]),
                                       "batched": timed(lambda: session.run_sequence(dev, batched=True)[0])}
            del session
        out[f"{H}x{W}"] = res
        del dev
    print(json.dumps({"bench": "session_batch", "frames": args.frames, "repeat": args.repeat, **out}))


if __name__ == "__main__":
    main()
