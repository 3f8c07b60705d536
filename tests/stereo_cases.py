"""The shared scenes of tests/test_stereo.py.  Depths are chosen so that disparities are whole pixels: with fB = f * B and a
surface at Z = fB / d, the right render is the left one moved by exactly d columns.

`plane`    a fronto-parallel plane at disparity d.
`box`      a box at disparity 25 in front of a plane at disparity 20 (fB = 110 000, Z = 4400 and 5500): the 5 columns of plane
           left of the box are what the right camera cannot see.
`layered`  what the GPU comparisons run on: per frame a plane, boxes in front of it at other disparities (one nearer than
           fB / D where asked), a strip of missing depth in both conventions (0 and 65535), different in every frame.

`gpu_case`          a `layered` batch at each of GPU_SHAPES: tile edges, D = 1, 2 and 256, one row; at most 3 frames.
`many_frames_case`  65541 frames of 13 x 5 that cycle through seven `layered` frames: more frames than the census and the
                    matcher have planes in their grids, so that their frame loops come round.
`variant_case`      the second GPU shape under each row of CONFIG_VARIANTS: every field of the config away from its default,
                    one at a time, and rule I's numerator at its 32-bit limit.
`box_case`          the `box` with sn.sense's record of its one frame.
`column0_case`      a 9 x 5 frame in which a disparity beyond the left border wins at column 0: x - d* = -1.
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


# ------------------------------------------------------------------ more frames than the grid has planes ---------------------
# k_stereo_census strides images and k_stereo_match frames over gridDim.z, capped at 65535: six frames more make the loop
# bodies run twice.  Frame n is distinct frame n % 7, and 65535 % 7 = 1: a kernel that indexed by plane, not by frame, would
# land on another distinct frame.  No IR noise, so that a frame's result does not depend on its index.
MANY_N, MANY_PERIOD, MANY_PLANES = 65541, 7, 65535
MANY_W, MANY_H, MANY_D = 13, 5, 6
MANY_IR_SEED = 0x5EED5
MANY_IR_FRAMES = (0, 1, 65534, 65535, 65536, MANY_N - 1)


def many_frames_case():
    """{"distinct": the 7 distinct (depth_l, labels_l, depth_r), "cfg" (no IR noise), "want": sn.sense of the 7,
    "index": int [MANY_N] = n % 7, "cfg_ir" (the default noise), "want_ir": {n: uint8 [2, H, W]} of MANY_IR_FRAMES}."""
    if "many" not in _cache:
        depth_l, labels, depth_r, cfg = layered(MANY_W, MANY_H, MANY_PERIOD, MANY_D, 5)
        cfg = dict(cfg, ir_noise_amp=0)
        cfg_ir = dict(cfg, ir_noise_amp=sn.DEFAULTS["ir_noise_amp"])
        index = np.arange(MANY_N) % MANY_PERIOD
        want_ir = {n: np.stack([sn.ir_image(depth_l[n % MANY_PERIOD], 0, n, cfg_ir, MANY_IR_SEED),
                                sn.ir_image(depth_r[n % MANY_PERIOD], 1, n, cfg_ir, MANY_IR_SEED)]) for n in MANY_IR_FRAMES}
        _cache["many"] = {"distinct": (depth_l, labels, depth_r), "cfg": cfg, "index": index, "cfg_ir": cfg_ir, "want_ir": want_ir,
                          "want": sn.sense(depth_l, labels, depth_r, cfg, seed=SEED, empty_depth=EMPTY)}
    return _cache["many"]


# ------------------------------------------------------------------ every config field ---------------------------------------
# The second GPU shape under a config changed one row at a time.  The last two rows run rule I's 32-bit numerator at its
# limit: the largest fb16 the entry points accept, divided by Z = 1, 2 and 3 (and 65534, the largest Z / 2 added to it).
VARIANT_SHAPE, VARIANT_SEED = (67, 9, 3, 24), 2
FB16_MAX = 2 ** 31 - 2 ** 15 - 1
LIMIT_COLUMNS = {"left": ((10, 1), (30, 2)), "right": ((20, 3), (50, 65534))}       # (column, Z)
CONFIG_VARIANTS = {
    "uniqueness 0": dict(uniqueness=0),
    "uniqueness 50": dict(uniqueness=50),
    "uniqueness 100": dict(uniqueness=100),
    "lr_max 0": dict(lr_max=0),
    "lr_max 255": dict(lr_max=255),
    "dq_min 1": dict(dq_min=1),
    "dq_min 200": dict(dq_min=200),
    "dq_min 65535": dict(dq_min=65535),
    "census_margin 0": dict(census_margin=0),
    "census_margin 255": dict(census_margin=255),
    "ambient 255": dict(ambient=255),
    "ambient 0, ir_noise_amp 255": dict(ambient=0, ir_noise_amp=255),
    "ir_noise_amp 0": dict(ir_noise_amp=0),
    "dot_threshold 0": dict(dot_threshold=0),
    "dot_threshold 0xFFFFFFFF": dict(dot_threshold=0xFFFFFFFF),
    "fb16 at its limit, fbp16 0": dict(fb16=FB16_MAX, fbp16=0),
    "fb16 at its limit, fbp16 = fb16": dict(fb16=FB16_MAX, fbp16=FB16_MAX),
}
LIMIT_VARIANTS = ("fb16 at its limit, fbp16 0", "fb16 at its limit, fbp16 = fb16")


def variant_case(name=None):
    """gpu_case's record (with sn.sense's "frames") of one row of CONFIG_VARIANTS; of the unchanged base without a name."""
    key = ("variant", name)
    if key not in _cache:
        W, H, N, D = VARIANT_SHAPE
        depth_l, labels, depth_r, cfg = layered(W, H, N, D, VARIANT_SEED)
        if name is not None:
            cfg = dict(cfg, **CONFIG_VARIANTS[name])
        if name in LIMIT_VARIANTS:
            for x, z in LIMIT_COLUMNS["left"]:
                depth_l[:, :, x] = z
            for x, z in LIMIT_COLUMNS["right"]:
                depth_r[:, :, x] = z
        _cache[key] = {"in": (depth_l, labels, depth_r), "cfg": cfg,
                       "want": sn.sense(depth_l, labels, depth_r, cfg, seed=SEED, empty_depth=EMPTY, keep=True)}
    return _cache[key]


def box_case():
    if "box" not in _cache:
        depth_l, labels, depth_r, cfg = box()
        _cache["box"] = {"in": (depth_l, labels, depth_r), "cfg": cfg, "want": sn.sense(depth_l, labels, depth_r, cfg, keep=True)}
    return _cache["box"]


# ------------------------------------------------------------------ a winner left of the right image -------------------------
# Rule W's left-right check asks x - d* >= 0 first.  The box of a d = x + 1 holds at least 15 cells of 62, and in no other
# case of this module does such a d win at a pixel that is otherwise valid.  These two renders (found by a seeded
# hill-climb on the CPU over per-pixel depths; dense dots, no census margin, no noise) make d* = 1 win at pixel (0, 4),
# uniquely and with dq >= dq_min: the pixel fails the check for x - d* = -1 alone.  lr_max = 255, so a kernel that went on
# to compare dR at a clamped column would pass it.
COLUMN0_PIXEL = (4, 0)               # (y, x)
COLUMN0_LEFT = ((12000, 2000, 4000, 12000, 5000, 2000, 1500, 6000, 2500),
                (16000, 4000, 5000, 1500, 16000, 2000, 12000, 4000, 8000),
                (16000, 0, 16000, 12000, 6000, 12000, 32000, 2500, 6000),
                (65535, 6000, 65535, 3500, 12000, 2000, 3000, 65535, 2500),
                (0, 12000, 65535, 2000, 6000, 32000, 12000, 0, 3000))
COLUMN0_RIGHT = ((3500, 32000, 16000, 32000, 6000, 2500, 8000, 5000, 8000),
                 (32000, 2500, 4000, 4000, 8000, 3500, 2000, 65535, 16000),
                 (12000, 3500, 65535, 8000, 3000, 16000, 16000, 0, 0),
                 (2000, 0, 2500, 2000, 4000, 12000, 3000, 1500, 65535),
                 (2000, 65535, 12000, 12000, 16000, 12000, 3000, 32000, 8000))


def column0_case():
    """gpu_case's record (with sn.sense's "frames") of the 9 x 5 frame above, every pixel labelled 3."""
    if "column 0" not in _cache:
        depth_l, depth_r = np.array([COLUMN0_LEFT], np.uint16), np.array([COLUMN0_RIGHT], np.uint16)
        labels = np.full(depth_l.shape, 3, np.uint16)
        cfg = sn.config(64000, 25600, max_disparity=4, dot_threshold=0xC0000000, pattern_seed=988811432, ambient=64, ir_noise_amp=0,
                        census_margin=0, uniqueness=0, lr_max=255, dq_min=1)
        _cache["column 0"] = {"in": (depth_l, labels, depth_r), "cfg": cfg,
                              "want": sn.sense(depth_l, labels, depth_r, cfg, seed=SEED, empty_depth=EMPTY, keep=True)}
    return _cache["column 0"]
