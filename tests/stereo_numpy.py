"""CPU restatement of the stereo depth sensor (include/rdf_labels.h: rdf_stereo_ir, rdf_stereo_sense): rules I, N, M, W and Z
in numpy, integer throughout (int64 / uint32 / uint64 where the header says integer), vectorised over a frame.  No device.
`sense` returns what the kernels write plus what the scene tests ask about (costs, winners)."""
import numpy as np

from hand_scene_numpy import FRAME_STEP, mix

CAMERA_STEP = 0x632BE5AB
HAM_OUTSIDE = 62
NONE = 1 << 20              # "there is no such cost": above every cost (<= 1550)
REASON_UNIQUE, REASON_LR, REASON_DQ_MIN = 1, 2, 4

DEFAULTS = dict(max_disparity=128, dot_threshold=1 << 30, pattern_seed=0x3D5EA75, ambient=16, ir_noise_amp=6, census_margin=16,
                uniqueness=10, lr_max=1, dq_min=16)


def config(fb16, fbp16, **kw):
    """The config as a dict: the integers of RdfStereoConfig."""
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, fb16=int(fb16), fbp16=int(fbp16), **kw)


def _mix1(x):
    return int(mix(np.array([x & 0xFFFFFFFF], np.uint64))[0])


# ------------------------------------------------------------------ rule I
def texels(u, y, cfg):
    """tex(u, y) for int64 arrays u and y of one shape."""
    row = mix((cfg["pattern_seed"] + (y.astype(np.uint64) * np.uint64(FRAME_STEP))) & np.uint64(0xFFFFFFFF))
    h = mix(row.astype(np.uint64) ^ (u.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64))
    return np.where(h < np.uint32(cfg["dot_threshold"]), 64 + (h & np.uint32(127)), 0).astype(np.int64)


def ir_image(depth, camera, n, cfg, seed):
    """Rule I for one camera (0 left, 1 right) of frame n: uint8 [H, W] of depth uint16 [H, W]."""
    H, W = depth.shape
    Z = depth.astype(np.int64)
    surface = (Z > 0) & (Z < 65535)
    Zs = np.where(surface, Z, 1)
    y, x = np.mgrid[:H, :W].astype(np.int64)
    if camera == 0:
        s = -((cfg["fbp16"] + Zs // 2) // Zs)
    else:
        s = ((cfg["fb16"] - cfg["fbp16"]) + Zs // 2) // Zs
    sq = 16 * x + s
    u, fr = sq >> 4, sq & 15
    dots = ((16 - fr) * texels(u, y, cfg) + fr * texels(u + 1, y, cfg)) >> 4
    v = cfg["ambient"] + np.where(surface, dots, 0)
    a = cfg["ir_noise_amp"]
    if a > 0:
        base = _mix1(seed + n * FRAME_STEP + camera * CAMERA_STEP)
        h = mix(np.arange(H * W, dtype=np.uint64) ^ np.uint64(base)).reshape(H, W)
        v = v + (h % np.uint32(2 * a + 1)).astype(np.int64) - a
    return np.clip(v, 0, 255).astype(np.uint8)


def ir_images(depth_l, depth_r, cfg, seed=0):
    """uint8 [N, 2, H, W]: what rdf_stereo_ir writes."""
    depth_l, depth_r = np.asarray(depth_l), np.asarray(depth_r)
    return np.stack([np.stack([ir_image(depth_l[n], 0, n, cfg, seed), ir_image(depth_r[n], 1, n, cfg, seed)])
                     for n in range(depth_l.shape[0])]) if depth_l.shape[0] else np.zeros((0, 2) + depth_l.shape[1:], np.uint8)


# ------------------------------------------------------------------ rule N
def census(image, margin):
    """uint64 [H, W] of uint8 [H, W]: bit k over dy = -3..3 (outer), dx = -4..4 (inner) without the centre."""
    H, W = image.shape
    padded = np.zeros((H + 6, W + 8), np.int64)
    padded[3:3 + H, 4:4 + W] = image
    bar = image.astype(np.int64) + margin
    bits = np.zeros((H, W), np.uint64)
    k = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            bits |= (padded[3 + dy:3 + dy + H, 4 + dx:4 + dx + W] > bar).astype(np.uint64) << np.uint64(k)
            k += 1
    assert k == 62
    return bits


# ------------------------------------------------------------------ rule M
def hamming(census_l, census_r, D):
    """ham(x, y, d) as int64 [D, H, W]: 62 where x - d < 0."""
    H, W = census_l.shape
    ham = np.full((D, H, W), HAM_OUTSIDE, np.int64)
    for d in range(min(D, W)):
        ham[d, :, d:] = np.bitwise_count(census_l[:, d:] ^ census_r[:, :W - d])
    return ham


def costs(ham, extra=0):
    """C(x, y, d) as int64 [D, H, W + extra] for 0 <= x < W + extra: the 5 x 5 box sum of ham, 62 outside the image."""
    D, H, W = ham.shape
    padded = np.full((D, H + 4, W + extra + 4), HAM_OUTSIDE, np.int64)
    padded[:, 2:2 + H, 2:2 + W] = ham
    c = np.zeros((D, H, W + extra), np.int64)
    for dy in range(5):
        for dx in range(5):
            c += padded[:, dy:dy + H, dx:dx + W + extra]
    return c


def right_costs(c_extended, W):
    """C_R(xr, y, d) = C(xr + d, y, d) from costs(ham, extra=D - 1): int64 [D, H, W]."""
    return np.stack([c_extended[d, :, d:d + W] for d in range(c_extended.shape[0])])


# ------------------------------------------------------------------ rule W
def winners(c):
    """The winner of a cost array whose first axis is d: {"d", "c", "second" (NONE where there is no d two or more away),
    "cm", "cp" (the winner's neighbours, NONE beyond the range)}, each of the remaining axes' shape."""
    c = np.asarray(c, np.int64)
    D = c.shape[0]
    d = np.argmin(c, 0)                        # the first of equals
    best = np.take_along_axis(c, d[None], 0)[0]
    ds = np.arange(D).reshape((D,) + (1,) * (c.ndim - 1))
    second = np.where(np.abs(ds - d[None]) >= 2, c, NONE).min(0)
    cm = np.where(d >= 1, np.take_along_axis(c, np.maximum(d - 1, 0)[None], 0)[0], NONE)
    cp = np.where(d <= D - 2, np.take_along_axis(c, np.minimum(d + 1, D - 1)[None], 0)[0], NONE)
    return {"d": d, "c": best, "second": second, "cm": cm, "cp": cp}


def is_unique(best, second, uniqueness):
    return (second == NONE) | (best * 100 < second * (100 - uniqueness))


def subpixel(cm, best, cp):
    """sub of rule W for a winner that has both neighbours (1 <= d* <= D - 2); 0 for an exact match (C* = 0)."""
    cm, best, cp = (np.asarray(v, np.int64) for v in (cm, best, cp))
    den = np.maximum(cm - best, cp - best)
    safe = np.where(den > 0, den, 1)
    sub = np.floor_divide(16 * (cm - cp) + safe, 2 * safe)          # numpy's // floors, also below zero
    return np.where((den > 0) & (best > 0), np.clip(sub, -8, 8), 0)


def match(census_l, census_r, cfg):
    """Rules M and W for one frame: {"dq", "reason", "d", "c", "second", "dR", "cost" [D, H, W + D - 1]}."""
    H, W = census_l.shape
    D = cfg["max_disparity"]
    cost = costs(hamming(census_l, census_r, D), extra=D - 1)
    left = winners(cost[:, :, :W])
    dR = winners(right_costs(cost, W))["d"]
    d = left["d"]
    inner = (d >= 1) & (d <= D - 2)
    sub = np.where(inner, subpixel(np.where(inner, left["cm"], 0), left["c"], np.where(inner, left["cp"], 0)), 0)
    dq = 16 * d + sub
    x = np.arange(W)[None, :]
    xr = x - d
    lr = (xr >= 0) & (np.abs(np.take_along_axis(dR, np.maximum(xr, 0), 1) - d) <= cfg["lr_max"])
    reason = (np.where(is_unique(left["c"], left["second"], cfg["uniqueness"]), 0, REASON_UNIQUE)
              | np.where(lr, 0, REASON_LR) | np.where(dq >= cfg["dq_min"], 0, REASON_DQ_MIN))
    return {"dq": dq.astype(np.uint16), "reason": reason.astype(np.uint8), "d": d, "c": left["c"], "second": left["second"],
            "dR": dR, "cost": cost}


# ------------------------------------------------------------------ rule Z, and the whole chain
def sense(depth_l, labels_l, depth_r, cfg, seed=0, empty_depth=65535, keep=False):
    """What rdf_stereo_sense writes: {"depth", "labels" uint16 [N, H, W], "ir" uint8 [N, 2, H, W], "dq" uint16, "reason"
    uint8}; with keep, "frames": match's record of every frame."""
    depth_l, labels_l, depth_r = np.asarray(depth_l), np.asarray(labels_l), np.asarray(depth_r)
    N, H, W = depth_l.shape
    ir = ir_images(depth_l, depth_r, cfg, seed)
    out = {"depth": np.empty((N, H, W), np.uint16), "labels": np.empty((N, H, W), np.uint16), "ir": ir,
           "dq": np.empty((N, H, W), np.uint16), "reason": np.empty((N, H, W), np.uint8), "frames": []}
    for n in range(N):
        m = match(census(ir[n, 0], cfg["census_margin"]), census(ir[n, 1], cfg["census_margin"]), cfg)
        valid = m["reason"] == 0
        dq = np.where(valid, m["dq"], 1).astype(np.int64)
        out["depth"][n] = np.where(valid, np.clip((cfg["fb16"] + dq // 2) // dq, 1, 65534), empty_depth)
        out["labels"][n] = np.where(valid, labels_l[n], 0)
        out["dq"][n], out["reason"][n] = m["dq"], m["reason"]
        if keep:
            out["frames"].append(m)
    return out
