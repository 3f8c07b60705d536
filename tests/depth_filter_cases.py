"""The shared cases of tests/test_depth_filter.py; every expected result is computed once (tests/depth_filter_numpy.py) and
shared.

`layered`   what most GPU comparisons run on: per frame a plane with a few units of noise (so that rules S and T have
            something to average), boxes at other depths, a strip of holes that moves from frame to frame, a hole strip as
            wide as the default max_gap, one wider and one more than twice as wide where the frame is wide enough, and scattered
            single holes.
`flicker`   pixels that come and go: per pixel a schedule of readings and holes, with runs of more than eight holes (so that a
            value is forgotten), short gaps (so that persistence holds) and jumps beyond temporal_delta.

`gpu_case`      a batch at each of GPU_SHAPES.  The kernel gives a workgroup one whole row and its halo rows, a thread a
                chunk of 8 pixels; rows go to the device 16 bytes at a time when the width is a multiple of 8.
`variant_case`  67 x 9 x 3 under each row of CONFIG_VARIANTS: every field away from its default, one at a time, from a state
                with history in it.  The frames carry a patch of readings of 1 next to readings of 65535.
`box_frames`    the box scene of tests/stereo_cases.py sensed eight times (IR seeds 100 .. 107, empty_depth 0)."""
import numpy as np

import depth_filter_numpy as dn

MAX_WIDTH = 2048


def layered(W, H, N, seed):
    """uint16 [N, H, W]."""
    rng = np.random.default_rng(seed)
    frames = np.empty((N, H, W), np.uint16)
    for n in range(N):
        f = 5000 + 3 * n + rng.integers(-4, 5, (H, W))
        for k in range(3):
            w, h = int(rng.integers(1, max(W // 3, 2))), int(rng.integers(1, max(H // 2, 2)))
            x0, y0 = int(rng.integers(0, max(W - w, 1))), int(rng.integers(0, max(H - h, 1)))
            f[y0:y0 + h, x0:x0 + w] = 3000 + 400 * k + 20 * n + rng.integers(-4, 5, (min(h, H - y0), min(w, W - x0)))
        f[rng.random((H, W)) < 0.08] = 0
        gap = int(rng.integers(0, max(W - 3, 1)))
        f[:, gap:gap + 1 + n % 3] = 0
        if W > 80:
            a = int(rng.integers(0, W - 70))
            f[: (H + 1) // 2, a:a + 32] = 0                 # exactly the default max_gap
            f[H // 2:, a + 36:a + 36 + 33] = 0              # one more
        if W > 200:
            a = int(rng.integers(0, W - 66))
            f[0, a:a + 65] = 0                              # out of reach from either side in its middle
        if n % 2:
            f[:, :2 + n] = 0                                # a gap at the row's start ...
        else:
            f[:, W - 1 - n:] = 0                            # ... and at its end
        frames[n] = f
    return frames


def flicker(W, H, N, seed):
    rng = np.random.default_rng(seed)
    base = 4000 + rng.integers(-3, 4, (N, H, W))
    kind = rng.integers(0, 5, (H, W))
    on = np.ones((N, H, W), bool)
    t = np.arange(N)[:, None, None]
    start = rng.integers(1, 6, (H, W))[None]
    on &= ~((kind[None] == 1) & (t >= start) & (t < start + 9 + rng.integers(0, 4, (H, W))[None]))   # a long absence: forgotten
    on &= ~((kind[None] == 2) & (rng.random((N, H, W)) < 0.5))                                       # coin flips
    on &= ~((kind[None] == 3) & (t % 4 != 0))                                                        # one reading in four
    base = np.where((kind[None] == 4) & (t >= N // 2), base + 500, base)                             # a jump beyond temporal_delta
    return np.where(on, base, 0).astype(np.uint16)


def special(W, H):
    """Four frames: two without a hole, one of holes only (every pixel persists), one layered."""
    frames = layered(W, H, 4, 99)
    for n in (0, 1):
        frames[n] = np.where(frames[n] == 0, 5000 + n, frames[n])
    frames[2] = 0
    return frames


# name -> (W, H, N, generator)
GPU_SHAPES = {
    "one column": (1, 7, 3, layered),
    "W 63": (63, 5, 1, layered),
    "W 64, rows that go 16 bytes at a time": (64, 6, 3, layered),
    "W 65": (65, 5, 3, layered),
    "the widest frame, H 3": (MAX_WIDTH, 3, 1, layered),
    "the widest frame, four rows": (MAX_WIDTH, 4, 2, layered),
    "one past the widest multiple of 8 below the limit": (MAX_WIDTH - 7, 5, 2, layered),
    "H 1": (70, 1, 3, layered),
    "H = r": (37, 2, 1, layered),
    "H = r + 1": (37, 3, 3, layered),
    "five rows": (40, 5, 3, layered),
    "nine rows": (67, 9, 3, layered),
    "nine rows, 16 bytes at a time": (72, 9, 3, layered),
    "1280 wide": (1280, 6, 2, layered),
    "20 frames of 13 x 5": (13, 5, 20, flicker),
    "20 frames of 24 x 9": (24, 9, 20, flicker),
    "no hole, all holes, layered": (33, 6, 4, lambda W, H, N, seed: special(W, H)),
}
SPLIT_SHAPE = (45, 6, 7)            # 7 frames, run as 3 + 4

_cache = {}


def gpu_case(name):
    """{"frames", "cfg", "want": dn.run's record from no history}."""
    if name not in _cache:
        W, H, N, make = GPU_SHAPES[name]
        frames = make(W, H, N, 1 + list(GPU_SHAPES).index(name))
        cfg = dn.config()
        _cache[name] = {"frames": frames, "cfg": cfg, "want": dn.run(frames, cfg)}
    return _cache[name]


def split_case():
    """{"frames" [7], "cfg", "want": the whole run, "want_head": the run of the first 3}."""
    if "split" not in _cache:
        W, H, N = SPLIT_SHAPE
        frames = np.concatenate([flicker(W, H, 4, 31), layered(W, H, 3, 32)])
        cfg = dn.config()
        _cache["split"] = {"frames": frames, "cfg": cfg, "want": dn.run(frames, cfg), "want_head": dn.run(frames[:3], cfg)}
    return _cache["split"]


VARIANT_SHAPE = (67, 9, 3)
CONFIG_VARIANTS = {
    "r 0": dict(spatial_radius=0),
    "r 1": dict(spatial_radius=1),
    "delta_s 0": dict(spatial_delta=0),
    "delta_s 65535": dict(spatial_delta=65535),
    "alpha 0": dict(temporal_alpha=0),
    "alpha 256": dict(temporal_alpha=256),
    "delta_t 0": dict(temporal_delta=0),
    "delta_t 65535": dict(temporal_delta=65535),
    "need 0": dict(persist_need=0),
    "need 9": dict(persist_need=9),
    "span 1": dict(persist_span=1),
    "span 8": dict(persist_span=8),
    "fill left": dict(fill_mode=1),
    "fill off": dict(fill_mode=0),
    "max_gap 0": dict(max_gap=0),
    "max_gap 1": dict(max_gap=1),
    "max_gap 67": dict(max_gap=67),
    "max_gap 65535": dict(max_gap=65535),
    "T off": dict(temporal=0),
}
EXTREMES = (slice(1, 6), slice(40, 48))          # the patch of 1s and 65535s in every variant frame
WIDE_GAP_ROWS = slice(7, 9)


def variant_frames():
    if "variant frames" not in _cache:
        W, H, N = VARIANT_SHAPE
        frames = np.concatenate([layered(W, H, 2, 41), flicker(W, H, 1, 42)])
        frames[1] = np.where(flicker(W, H, 1, 43)[0] == 0, 0, frames[1])
        yy, xx = np.mgrid[:H, :W]
        for n in range(N):
            patch = np.where((yy + xx + n) % 2 == 0, 1, 65535).astype(np.uint16)
            frames[n][EXTREMES] = patch[EXTREMES]
        frames[2][3, 43] = 0
        frames[:, WIDE_GAP_ROWS, :W - 1], frames[:, WIDE_GAP_ROWS, W - 1] = 0, 5000       # a gap only max_gap >= W - 1 closes
        _cache["variant frames"] = frames
    return _cache["variant frames"]


def variant_history():
    """The state the variant frames start from: what six flickering frames leave under the default config, so that the three
    frames have eight frames of history behind them (persist_span 8 sees further back than 4)."""
    if "variant history" not in _cache:
        W, H, _ = VARIANT_SHAPE
        state = dn.run(flicker(W, H, 6, 44), dn.config())["state"]
        state[WIDE_GAP_ROWS] = 0                            # nothing persists in the wide gap
        _cache["variant history"] = state
    return _cache["variant history"]


def variant_case(name=None):
    """gpu_case's record (with "state", the state before the call) of one row of CONFIG_VARIANTS; of the default config
    without a name."""
    key = ("variant", name)
    if key not in _cache:
        frames = variant_frames()
        cfg = dn.config(**(CONFIG_VARIANTS[name] if name else {}))
        _cache[key] = {"frames": frames, "cfg": cfg, "state": variant_history(), "want": dn.run(frames, cfg, state=variant_history())}
    return _cache[key]


def box_frames():
    """(raw uint16 [8, H, W], truth uint16 [H, W]) of stereo_cases.box()."""
    if "box" not in _cache:
        import stereo_cases as sc
        import stereo_numpy as sn
        depth_l, labels, depth_r, cfg = sc.box()
        raw = np.concatenate([sn.sense(depth_l, labels, depth_r, cfg, seed=100 + i, empty_depth=0)["depth"] for i in range(8)])
        _cache["box"] = (raw, depth_l[0])
    return _cache["box"]
