#!/usr/bin/env python3
"""Frames per second of BeatsSession.run_sequence (depth frames to note events, one synchronisation at the end) and of the
same frames driven the old way: FrameFrontEnd, HandGrouping and HandPipeline.run() per hand with a host read per hand and
frame, and the numpy state machine (tests/hand_state_numpy.py) on the host.  Prints one JSON line.

    python tests/perf/bench_session.py [--frames 240] [--repeat 5]
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
    args = ap.parse_args()
    import torch        # (before the package, as the other scripts here do: the HIP runtime that gets loaded is torch's)
    import session_cases as sc
    from hand_state_numpy import HandStateNumpy
    rdf = importlib.import_module("3d-beats_amd")
    torch.cuda.set_device(0)
    pl = importlib.import_module("3d-beats_amd.pipeline")
    H, W = sc.H, sc.W
    base, (focal, ppx, ppy) = sc.frames()
    frames = np.stack([base[k % sc.FRAMES] for k in range(args.frames)])
    f0, f1, conditions, colors = sc.forest_config(rdf)

    def stack():
        cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                          {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
               "conditions": conditions, "label_colors": colors}
        return rdf.LayeredDecisionForest(cfg, (H, W), 2)
    session = rdf.BeatsSession(stack(), (H, W), (focal, ppx, ppy), num_random_guesses=4000, seed=3)
    plane = session.calibrate(frames[0])
    dev = rdf.to_device(frames)

    fe = rdf.FrameFrontEnd((H, W), (focal, ppx, ppy), sc.PLANE_T, gauss_sigma=2.0)
    fe.set_plane(plane)
    hg = rdf.HandGrouping((H, W), sc.LEVEL, 0.06)
    lf = stack()
    pargs = ((H, W), 2, W / 848, 6, [50., 8., 8., 8., 8., 8., 8.], [2, 3, 4, 5, 6], (focal, focal, ppx, ppy), plane)
    right, left = pl.HandPipeline(lf, *pargs, depth_mm_level=sc.LEVEL), pl.HandPipeline(lf, *pargs, depth_mm_level=sc.LEVEL)
    clean, groups = rdf.GpuBuffer((H, W), np.uint16), rdf.GpuBuffer((H >> sc.LEVEL, W >> sc.LEVEL), np.uint16)

    class Frame:
        def __init__(self, a):
            self._a, self.shape, self.dtype = a, a.shape, a.dtype

        def cu(self):
            return self._a

    def old_way():
        model = HandStateNumpy([200., 160., 160., 160., 160.] * 2, 36 + np.arange(10), 50)
        model.z_thresh_offset, model.min_velocity[:], model.max_velocity[:] = 25., 10., 120.
        for k in range(args.frames):
            raw = Frame(dev[k])
            fe.run(raw, clean)
            hg.make_group_image(clean, groups)
            model.step(right.run(clean, groups, 1, False, height_depth=raw)[1], 0)
            model.step(left.run(clean, groups, 2, True, height_depth=raw)[1], 5)
        return model.events

    def new_way():
        return session.run_sequence(dev)[0]

    out = {}
    for name, fn in (("run_sequence", new_way), ("components_and_host_state_machine", old_way)):
        fn()                                        # warm-up
        host, device, n_events = [], [], 0
        for _ in range(args.repeat):
            # both end in a synchronisation (poll() / the last frame's read); device events bracket the same work, as a
            # check on the host clock
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t = time.perf_counter()
            n_events = len(fn())
            host.append(time.perf_counter() - t)
            e1.record()
            e1.synchronize()
            device.append(e0.elapsed_time(e1) / 1e3)
        out[name] = {"frames_per_s": round(args.frames / min(host), 1),
                     "frames_per_s_median": round(args.frames / sorted(host)[len(host) // 2], 1),
                     "frames_per_s_by_device_events": round(args.frames / min(device), 1), "events": n_events}
    print(json.dumps({"bench": "session", "frames": args.frames, "dims": [H, W], **out}))


if __name__ == "__main__":
    main()
