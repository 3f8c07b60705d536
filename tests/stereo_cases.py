"""The shared scenes of tests/test_stereo.py.  Depths are chosen so that disparities are whole pixels: with fB = f * B and a
surface at Z = fB / d, the right render is the left one moved by exactly d columns.

`plane`    a fronto-parallel plane at disparity d.
`box`      a box at disparity 25 in front of a plane at disparity 20 (fB = 110 000, Z = 4400 and 5500): the 5 columns of plane
           left of the box are what the right camera cannot see.
`layered`  what the GPU comparisons run on: per frame a plane, boxes in front of it at other disparities (one nearer than
           fB / D where asked), a strip of missing depth in both conventions (0 and 65535), different in every frame.
Every expected result is computed once and shared."""
import numpy as np

import stereo_numpy as sn


def plane(W, H, d, Z, D, **kw):
    """(depth_l, labels_l, depth_r [1, H, W], cfg) of a plane at depth Z whose disparity is exactly d."""
    depth = np.full((1, H, W), Z, np.uint16)
    return depth, np.ones((1, H, W), np.uint16), depth.copy(), sn.config(16 * d * Z, (16 * d * Z * 2) // 5, max_disparity=D, **kw)


BOX = dict(W=200, H=64, x0=90, x1=140, y0=12, y1=52, fB=110000, Z_table=5500, Z_box=4400, D=48)


def box():
    b = BOX
    depth_l = np.full((1, b["H"], b["W"]), b["Z_table"], np.uint16)
    depth_r = depth_l.copy()
    shift = b["fB"] // b["Z_box"]
    depth_l[0, b["y0"]:b["y1"], b["x0"]:b["x1"]] = b["Z_box"]
    depth_r[0, b["y0"]:b["y1"], b["x0"] - shift:b["x1"] - shift] = b["Z_box"]
    labels = (depth_l == b["Z_box"]).astype(np.uint16) * 3
    return depth_l, labels, depth_r, sn.config(16 * b["fB"], (16 * b["fB"] * 2) // 5, max_disparity=b["D"])


def layered(W, H, N, D, seed, near=False):
    """(depth_l, labels_l, depth_r uint16 [N, H, W], cfg)."""
    rng = np.random.default_rng(seed)
    fB = 24000 * max(D, 4)
    d_plane = max(D // 3, 1)
    depth_l = np.empty((N, H, W), np.uint16)
    depth_r = np.empty((N, H, W), np.uint16)
    labels = np.zeros((N, H, W), np.uint16)
    for n in range(N):
        z = min(fB // (d_plane + n), 65000)
        depth_l[n], depth_r[n] = z, z
        boxes = [(d_plane + n + 1 + int(rng.integers(0, max(D // 2, 1))), k + 1) for k in range(2)]
        if near:
            boxes.append((D + 3, 9))
        for d, label in sorted(boxes):
            w, h = int(rng.integers(3, max(W // 3, 4))), int(rng.integers(1, max(H // 2, 2)))
            x0, y0 = int(rng.integers(0, max(W - w, 1))), int(rng.integers(0, max(H - h, 1)))
            depth_l[n, y0:y0 + h, x0:x0 + w] = fB // d
            labels[n, y0:y0 + h, x0:x0 + w] = label
            a, b = max(x0 - d, 0), max(x0 + w - d, 0)
            depth_r[n, y0:y0 + h, a:b] = fB // d
        gap = int(rng.integers(0, max(W - 3, 1)))
        depth_l[n, :, gap:gap + 2] = 0 if n % 2 else 65535
        depth_r[n, :, max(gap - d_plane, 0):max(gap + 2 - d_plane, 0)] = 65535 if n % 2 else 0
    cfg = sn.config(16 * fB, (16 * fB * 2) // 5, max_disparity=D, pattern_seed=seed * 7919 + 1)
    return depth_l, labels, depth_r, cfg


# name -> (W, H, N, D, near); the matcher's tile is 60 columns x 32 rows (8 per wave), the census tile 64 x 4
GPU_SHAPES = {
    "one more than a tile each way": (61, 33, 1, 16, False),
    "three frames, no multiple of any tile": (67, 9, 3, 24, False),
    "narrower than the disparity range": (20, 12, 1, 48, False),
    "lower than the census window, one more than its tile wide": (65, 5, 1, 8, False),
    "one row": (70, 1, 2, 8, False),
    "D = 1": (37, 11, 1, 1, False),
    "D = 2": (37, 11, 1, 2, False),
    "D = 256": (300, 16, 1, 256, False),
    "several tiles, a surface nearer than fB / D": (130, 40, 2, 32, True),
}
SEED, EMPTY = 77, 0

_cache = {}


def gpu_case(name):
    """{"in": (depth_l, labels_l, depth_r), "cfg", "want": sn.sense's record}, computed once."""
    if name not in _cache:
        W, H, N, D, near = GPU_SHAPES[name]
        depth_l, labels, depth_r, cfg = layered(W, H, N, D, 1 + list(GPU_SHAPES).index(name), near)
        _cache[name] = {"in": (depth_l, labels, depth_r), "cfg": cfg,
                        "want": sn.sense(depth_l, labels, depth_r, cfg, seed=SEED, empty_depth=EMPTY)}
    return _cache[name]


def box_case():
    if "box" not in _cache:
        depth_l, labels, depth_r, cfg = box()
        _cache["box"] = {"in": (depth_l, labels, depth_r), "cfg": cfg, "want": sn.sense(depth_l, labels, depth_r, cfg, keep=True)}
    return _cache["box"]
