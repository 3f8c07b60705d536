"""CPU restatement of the depth post-filter (include/rdf_frontend.h: rdf_depth_filter): rules S, T and F in numpy, integer
throughout (int64), one function per rule and `run` for the chain over consecutive frames.  No device."""
import numpy as np

FLAG_BLENDED, FLAG_PERSISTED, FLAG_FILLED = 1, 2, 4

DEFAULTS = dict(spatial_radius=2, spatial_delta=60, temporal=1, temporal_alpha=102, temporal_delta=100, persist_need=2,
                persist_span=4, fill_mode=2, max_gap=32)
# field -> (lowest, highest) accepted value
RANGES = dict(spatial_radius=(0, 2), spatial_delta=(0, 65535), temporal=(0, 1), temporal_alpha=(0, 256), temporal_delta=(0, 65535),
              persist_need=(0, 9), persist_span=(1, 8), fill_mode=(0, 2), max_gap=(0, 65535))


def config(**kw):
    """The config as a dict: the integers of RdfDepthFilterConfig."""
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    cfg = dict(DEFAULTS, **{k: int(v) for k, v in kw.items()})
    for k, (lo, hi) in RANGES.items():
        assert lo <= cfg[k] <= hi, (k, cfg[k])
    return cfg


def new_state(H, W):
    return np.zeros((H, W), np.uint32)


# ------------------------------------------------------------------ rule S
def spatial(frame, r, delta):
    """uint16 [H, W] of uint16 [H, W]."""
    c = np.asarray(frame).astype(np.int64)
    if r == 0:
        return c.astype(np.uint16)
    H, W = c.shape
    padded = np.zeros((H + 2 * r, W + 2 * r), np.int64)          # outside the frame: no reading
    padded[r:r + H, r:r + W] = c
    s, k = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            n = padded[dy:dy + H, dx:dx + W]
            take = (n != 0) & (np.abs(n - c) <= delta)
            s += np.where(take, n, 0)
            k += take
    k = np.where(c != 0, k, 1)
    return np.where(c != 0, (2 * s + k) // (2 * k), 0).astype(np.uint16)


# ------------------------------------------------------------------ rule T
def temporal(frame, state, alpha, delta, need, span):
    """One frame: (out uint16 [H, W], flags uint8 [H, W], the new state uint32 [H, W])."""
    c = np.asarray(frame).astype(np.int64)
    st = np.asarray(state).astype(np.int64)
    v, hist = st >> 8, st & 255
    reading = c != 0
    c16 = 16 * c
    blend = reading & (v != 0) & (np.abs(c16 - v) <= 16 * delta)
    nv = np.where(blend, (alpha * c16 + (256 - alpha) * v + 128) >> 8, c16)
    recent = np.bitwise_count((hist & ((1 << span) - 1)).astype(np.uint8)).astype(np.int64)
    persist = ~reading & (v != 0) & (recent >= need)
    out = np.where(reading, (nv + 8) >> 4, np.where(persist, (v + 8) >> 4, 0))
    v2 = np.where(reading, nv, v)
    hist2 = ((hist << 1) | reading) & 255
    v2 = np.where(~reading & (hist2 == 0), 0, v2)
    flags = np.where(blend, FLAG_BLENDED, 0) | np.where(persist, FLAG_PERSISTED, 0)
    return out.astype(np.uint16), flags.astype(np.uint8), ((v2 << 8) | hist2).astype(np.uint32)


# ------------------------------------------------------------------ rule F
def fill(frame, mode, max_gap):
    """(out uint16 [H, W], filled bool [H, W]) of T's output."""
    t = np.asarray(frame).astype(np.int64)
    H, W = t.shape
    if mode == 0:
        return t.astype(np.uint16), np.zeros((H, W), bool)
    x = np.arange(W)[None, :]
    # the column of the last reading at or left of x (-1: none), and of the first at or right of x (W: none)
    last = np.maximum.accumulate(np.where(t != 0, x, -1), axis=1)
    first = np.minimum.accumulate(np.where(t != 0, x, W)[:, ::-1], axis=1)[:, ::-1]
    L = np.where((last >= 0) & (x - last <= max_gap), np.take_along_axis(t, np.maximum(last, 0), 1), 0)
    R = np.where((first < W) & (first - x <= max_gap), np.take_along_axis(t, np.minimum(first, W - 1), 1), 0)
    value = L if mode == 1 else np.maximum(L, R)
    hole = t == 0
    return np.where(hole, value, t).astype(np.uint16), hole & (value != 0)


# ------------------------------------------------------------------ the chain
def run(frames, cfg, state=None):
    """frames uint16 [N, H, W], consecutive in time -> {"depth" uint16 [N, H, W], "flags" uint8 [N, H, W], "state" uint32
    [H, W] after the last frame}.  `state` is left as it was; None = no history.  With T off the state comes back unchanged."""
    frames = np.asarray(frames)
    N, H, W = frames.shape
    state = new_state(H, W) if state is None else np.array(state, np.uint32)
    depth, flags = np.zeros((N, H, W), np.uint16), np.zeros((N, H, W), np.uint8)
    for i in range(N):
        d = spatial(frames[i], cfg["spatial_radius"], cfg["spatial_delta"])
        if cfg["temporal"]:
            d, flags[i], state = temporal(d, state, cfg["temporal_alpha"], cfg["temporal_delta"], cfg["persist_need"],
                                          cfg["persist_span"])
        depth[i], filled = fill(d, cfg["fill_mode"], cfg["max_gap"])
        flags[i] |= np.where(filled, FLAG_FILLED, 0).astype(np.uint8)
    return {"depth": depth, "flags": flags, "state": state}
