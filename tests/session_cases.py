"""The scene of the BeatsSession tests: 12 raw camera frames of 240 x 424 (the camera's half-resolution mode) with a tilted
table and two "hands" that drift sideways and come down towards the table, and the forests of tests/test_pipeline.py."""
import numpy as np

H, W, R, LEVEL, FRAMES = 240, 424, 2, 3, 12
FOCAL = 210.
PLANE_T = 40.


def frame(k, seed=40):
    """Frame k: a table tilted by 25 degrees 600 mm from the camera and two boxes with five fingers each, 270 - 15 k mm
    above it (a descent of 15 mm per frame: above the app's min_velocity of 10), drifting 2 pixels per frame.
    Returns (depth uint16 [H, W], (focal, ppx, ppy))."""
    ppx, ppy = (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2
    t = np.deg2rad(25.)
    n = np.array([0., -np.sin(t), np.cos(t)])
    yy, xx = np.mgrid[:H, :W]
    ray = np.stack([(xx - ppx) / FOCAL, (yy - ppy) / FOCAL, np.ones((H, W))], -1) @ n
    z = 600. / ray
    box_h = 270. - 15. * k
    for cx, drift in ((0.3, 2), (0.7, -2)):
        c = cx * W + drift * k
        m = (np.abs(xx - c) < W * 0.13) & (np.abs(yy - 0.6 * H) < H * 0.17)
        for j in range(5):
            m |= (np.abs(xx - (c + (j - 2) * 0.045 * W)) < W * 0.016) & (yy > 0.2 * H) & (yy < 0.6 * H)
        z[m] = (600. - box_h) / ray[m]
    d = np.round(z).astype(np.uint16)
    d[np.random.default_rng(seed + k).random((H, W)) < 0.01] = 0
    return d, (FOCAL, ppx, ppy)


def frames():
    return np.stack([frame(k)[0] for k in range(FRAMES)]), frame(0)[1]


def forest_config(rdf):
    synth = rdf.synth
    f0, f1 = synth.forest(3, 9, 4, "trained", 60), synth.forest(3, 10, 5, "trained", 70)
    conditions = [[0, 1], [0, 2], [1, 3], [0, 3], [0, 4], [0, 5], [0, 6], [0, 7]]
    colors = [[10 * i, 255 - 10 * i, i, 255] for i in range(1, 8)]
    return f0, f1, conditions, colors
