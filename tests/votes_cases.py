"""The cases of tests/test_joint_votes.py: seeded numpy builders, cached and frozen, that the CPU tests and the GPU tests both
call, so that both see the same arrays.

  hand_case()            the D = 1 stump on one 8 x 4 frame of depth 64 whose sums, votes, cells and joint the test writes out.
  targets_for(...)       targets for the adversarial frames of walk_cases: absent joints, targets outside the frame, targets
                         exactly `radius` and `radius + 1` away from a hand pixel.
  fit_case()             sums written directly: counts on both sides of min_count and of 2^26, variances on both sides of
                         max_var, negative sums, an unreachable slot that holds sums.
  border_case()          a stump, one voting pixel and a table whose joints land on and next to every border of V4.
  wave_case()            a frame 64 pixels wide in which a wave's 64 lanes vote into one cell for joint 0, into 64 for joint 1.

`memo_walk` is refit_numpy.walk behind a cache, for the frozen arrays of these cases: votes_numpy's functions take it as their
`walk`, so that the eighteen runs over the adversarial frames walk every pixel once per scale."""
import functools

import numpy as np

import refit_cases as rc
import refit_numpy as rn
import votes_numpy as vn
import walk_cases as wc


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


_walks = {}


def memo_walk(frame, tree, D, x, y, scale):
    """refit_numpy.walk, remembered per (frame, tree, pixel, scale).  Only for arrays that stay alive and unchanged: the key
    is their address."""
    assert not frame.flags.writeable and not tree.flags.writeable, "memo_walk is for the frozen arrays of the cases"
    key = (frame.ctypes.data, frame.shape, tree.ctypes.data, D, x, y, float(scale))
    if key not in _walks:
        _walks[key] = rn.walk(frame, tree, D, x, y, scale)
    return _walks[key]


# ------------------------------------------------------------ the case worked by hand ------------------------------------------
HAND = dict(radius=3, min_count=1, max_var=3, shift=1)


def hand_case():
    """(depth [1, 4, 8], labels, targets [1, 1, 3], forest [1, 1, 9]).  Depth 64 everywhere but a 0 at (7, 0), so ox = dx.  The
    stump probes (x + 2, y) against (x, y) (offset 128 at depth 64), thresh 1: f = 0 goes left for x <= 5, the probe leaves the
    frame and f = 65471 goes right for x >= 6; both sides are leaf slots.  Hand pixels (x, y): (1, 1), (2, 1), (0, 3) left,
    (6, 2) right, (7, 0) without depth.  One joint at (4, 2), depth 70."""
    depth = np.full((1, 4, 8), 64, np.uint16)
    depth[0, 0, 7] = 0
    labels = np.zeros(depth.shape, np.uint16)
    for x, y in ((1, 1), (2, 1), (0, 3), (6, 2), (7, 0)):
        labels[0, y, x] = 1 + x                             # any label but 0 is "hand"
    targets = np.array([[[4, 2, 70]]], np.int32)
    forest = np.zeros((1, 1, 9), np.float32)
    forest[0, 0, :7] = [128., 0., 0., 0., 1., 0., 0.]
    return depth, labels, targets, forest


# ------------------------------------------------------------ targets for the adversarial frames ------------------------------
def hand_pixels(depth, labels):
    """(image, y, x) of the pixels rule V1 walks, in memory order."""
    return [tuple(int(v) for v in p) for p in np.argwhere((labels > 0) & (depth > 0) & (depth < 65535))]


@functools.lru_cache(maxsize=None)
def targets_for(J, radius, seed=77):
    """int32 [2, J, 3] for walk_cases.adversarial_frames(): joint 0 of image 0 sits exactly `radius` to the right of a hand pixel
    (so `radius + 1` from its left neighbour, a hand pixel too), joint 0 of image 1 `radius` below one; further joints are drawn
    inside and around the frame; with five joints and more one is absent per image (tz 0, 65535 and negative), one lies left of
    or above the frame and one `radius + 1` away along y from a hand pixel of the last row."""
    depth, labels = wc.adversarial_frames()
    n, H, W = depth.shape
    rng = np.random.default_rng(seed + 100 * J + radius)
    t = np.zeros((n, J, 3), np.int32)
    t[:, :, 0] = rng.integers(-5, W + 5, (n, J))
    t[:, :, 1] = rng.integers(-3, H + 3, (n, J))
    t[:, :, 2] = rng.integers(200, 3200, (n, J))
    px = hand_pixels(depth, labels)
    pair = next((i, y, x) for i, y, x in px if i == 0 and (0, y, x - 1) in px)      # a hand pixel with a hand pixel to its left
    t[0, 0, :2] = (pair[2] + radius, pair[1])
    below = next((i, y, x) for i, y, x in px if i == 1)
    t[1, 0, :2] = (below[2], below[1] + radius)
    if J >= 5:
        t[0, 1, 2], t[1, 1, 2], t[1, 2, 2] = 0, 65535, -4                          # absent
        t[0, 2, :2] = (-9, 4)                                                       # left of the frame
        t[1, 3, :2] = (W + 200, -7)                                                 # right of and above it
        last = next((i, y, x) for i, y, x in reversed(px) if i == 0)
        t[0, 4, :2] = (last[2], last[1] + radius + 1)                               # one too far for that pixel
    if J >= 16:
        t[0, 15] = (2 ** 31 - 1, -2 ** 31, 65534)                                  # the int32 range: dx needs 64 bits
        t[1, 15] = (-2 ** 31, 2 ** 31 - 1, 1)
    _freeze(t)
    return t


# ------------------------------------------------------------ sums written directly -------------------------------------------
FIT = dict(J=3, min_count=5, max_var=1000)


@functools.lru_cache(maxsize=None)
def fit_case():
    """(forest, sums, slots): the adversarial forest of walk_cases and sums uint64 [T, N, 2, 3, 5] that are zero but for the
    named entries `slots` = {name: (t, n, s, j)}, written on reachable leaf slots (`unreachable` excepted)."""
    _, _, forest, _ = wc.adversarial_case()
    T, N = forest.shape[:2]
    J, m, V = FIT["J"], FIT["min_count"], FIT["max_var"]
    reach = rn.reachable_nodes(forest)
    leaf = [(t, n, s) for t in range(T) for n in range(N) for s in (0, 1) if reach[t, n] and rn.is_leaf_slot(forest[t, n], s)]
    dead = [(t, n, s) for t in range(T) for n in range(N) for s in (0, 1) if not reach[t, n]]
    assert len(leaf) >= 12 and dead
    sums = np.zeros((T, N, 2, J, 5), np.uint64)
    u = lambda v: np.uint64(v & vn.M64)                     # noqa: E731
    entries = {
        "below_min_count": (m - 1, 4, 4, 4, 40),
        "at_min_count": (m, 5, 5, 5, 50),
        "below_2_26": ((1 << 26) - 1, 3 * ((1 << 26) - 1), 0, -7, 9 * ((1 << 26) - 1) + 5),      # mean 3, var 0
        "at_2_26": (1 << 26, 3 << 26, 0, -7, 9 << 26),
        "var_at_max": (8, 0, 0, 0, 8 * V + 7),              # floordiv gives V: kept, w = 256 - floordiv(256 V, V + 1) = 1
        "var_above_max": (8, 0, 0, 0, 8 * (V + 1)),         # V + 1: dropped for spread
        "negative_sums": (6, -7, -13, -40000, 6 * 9),       # floordiv(-7, 6) = -2, floordiv(-13, 6) = -3: var = max(0, 9 - 13) = 0
        "var_clamped": (8, 24, 0, 0, 1),                    # mx = 3, floordiv(1, 8) - 9 < 0: var = 0, w = 256
        "large_means": (9, 9 * ((1 << 18) - 1), -9 * ((1 << 18) - 1), 9 * 65533, 2 * 9 * ((1 << 18) - 1) ** 2 + 9 * 17),   # var 17
    }
    slots = {}
    for k, (name, e) in enumerate(entries.items()):
        t, n, s = leaf[k]
        j = k % J
        sums[t, n, s, j] = [u(v) for v in e]
        slots[name] = (t, n, s, j)
    t, n, s = dead[len(dead) // 2]
    sums[t, n, s, 1] = [u(v) for v in (100, 100, 100, 100, 100)]
    slots["unreachable"] = (t, n, s, 1)
    _freeze(sums)
    return forest, sums, slots


# ------------------------------------------------------------ votes on and next to every border -------------------------------
BORDER = dict(W=8, H=3, d=64, x=5, y=1)


def all_left_stump():
    """D = 1, C = 1: no offsets, f = 0 < 1, everything ends in the left leaf slot."""
    forest = np.zeros((1, 1, 9), np.float32)
    forest[0, 0, 4] = 1.
    return forest


def border_case():
    """(depth [1, 3, 8] of 64 everywhere, forest, votes int32 [1, 1, 2, 10, 4], gate_one, gate_two).  At depth 64 a vote moves
    by (mx, my) pixels exactly.  gate_one lets pixel (5, 1) alone take part: joints 0 and 1 land on vx = W - 1 and W, 2 and 3 on
    vy = -1 and 0, 4 to 7 on vz = 0, 1, 65534 and 65535; joint 8 stays on the pixel; joint 9 has w = 0.  gate_two lets (6, 2) and
    (1, 1) take part: for joint 8 two cells of equal weight, and the lower row-major index, (1, 1), wins."""
    m = BORDER
    depth = np.full((1, m["H"], m["W"]), m["d"], np.uint16)
    votes = np.zeros((1, 1, 2, 10, 4), np.int32)
    votes[0, 0, 0] = [(m["W"] - 1 - m["x"], 0, 0, 7), (m["W"] - m["x"], 0, 0, 7), (0, -m["y"] - 1, 0, 9), (0, -m["y"], 0, 9),
                      (0, 0, -m["d"], 11), (0, 0, 1 - m["d"], 11), (0, 0, 65534 - m["d"], 13), (0, 0, 65535 - m["d"], 13),
                      (0, 0, 6, 100), (1, 1, 1, 0)]
    votes[0, 0, 1] = (1, 1, 1, 256)                         # the right side: nothing ends there
    gate_one = np.zeros(depth.shape, np.uint16)
    gate_one[0, m["y"], m["x"]] = 3
    gate_two = np.zeros(depth.shape, np.uint16)
    gate_two[0, 2, 6] = gate_two[0, 1, 1] = 1
    return depth, all_left_stump(), votes, gate_one, gate_two


# ------------------------------------------------------------ a wave's 64 lanes on one cell, and on 64 --------------------------
def wave_case():
    """(depth [1, 2, 64] of 1000 everywhere, forest, votes int32 [1, 63, 2, 2, 4]).  refit_cases.column_tree(6, 1, 64) ends column
    x in its own slot of level 5.  Joint 0 of column x's slot points at column 32 -- mx = floordiv((32 - x) * 1000, 64), which
    V4 inverts exactly at this depth -- so the 64 lanes of the wave that holds a row vote into one cell; joint 1 points at the
    pixel itself, 64 cells for 64 lanes.  Weights differ from column to column, so a lost or doubled lane shows."""
    depth = np.full((1, 2, 64), 1000, np.uint16)
    forest = rc.column_tree(6, 1, 64)[None].copy()
    votes = np.zeros((1, 63, 2, 2, 4), np.int32)
    for x in range(64):
        n, s = 31 + (x >> 1), x & 1
        votes[0, n, s, 0] = (vn.offset(32 - x, 1000), 0, x - 20, 1 + x)
        votes[0, n, s, 1] = (0, 0, 3 * x, 256 - x)
    return depth, forest, votes
