"""The cases of tests/test_joint_votes.py: seeded numpy builders, cached and frozen, that the CPU tests and the GPU tests both
call, so that both see the same arrays.

  hand_case()            the D = 1 stump on one 8 x 4 frame of depth 64 whose sums, votes, cells and joint the test writes out.
  targets_for(...)       targets for the adversarial frames of walk_cases: absent joints, targets outside the frame, targets
                         exactly `radius` and `radius + 1` away from a hand pixel.
  fit_case()             sums written directly: counts on both sides of min_count and of 2^26, variances on both sides of
                         max_var, negative sums, an unreachable slot that holds sums.
  border_case()          a stump, one voting pixel and a table whose joints land on and next to every border of V4.
  wave_case()            a frame 64 pixels wide in which a wave's 64 lanes vote into one cell for joint 0, into 64 for joint 1.

  tie_case(name)         TIE_LAYOUTS: gates on a 20 x 40 frame of one depth that leave equal cells, and equal box sums, for V5's
                         tie rule: the lower index on the higher thread, one thread twice, boxes clipped by different borders.
  sum_case()             405 stumps on 144 x 144: the box sum of the whole grid is above 2^31 - 1; the accumulator in closed form.
  wide_case()            one row of 20000 pixels and a table written directly: 128 m + d on both sides of +-2^31, weights
                         outside 1..256.
  middle_case()          three stumps of which the second tells some hand pixels to go on at level D - 1.
  count_sweep_case(), fit_sweep_case(), modes_sweep_case()
                         more pixels, nodes and (frame, joint) pairs than one sweep of the kernels' grids takes.

EDITS names wrong readings of rules V1 to V5, `mutant(name)` loads tests/votes_numpy.py with that reading (tests/mutants.py),
`outputs(mod, name)` computes what the device test of case `name` compares, KILLS says which device case must notice which
reading, EQUIVALENT which readings no input can tell from the rule, and why.

`memo_walk` is refit_numpy.walk behind a cache, for the frozen arrays of these cases: votes_numpy's functions take it as their
`walk`, so that the eighteen runs over the adversarial frames walk every pixel once per scale."""
import functools

import numpy as np

import mutants
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
    entries = fit_entries(m, V)
    slots = {}
    for k, (name, e) in enumerate(entries.items()):
        t, n, s = leaf[k]
        j = k % J
        sums[t, n, s, j] = [_u64(v) for v in e]
        slots[name] = (t, n, s, j)
    t, n, s = dead[len(dead) // 2]
    sums[t, n, s, 1] = [_u64(v) for v in (100, 100, 100, 100, 100)]
    slots["unreachable"] = (t, n, s, 1)
    _freeze(sums)
    return forest, sums, slots


def _u64(v):
    return np.uint64(v & vn.M64)


def fit_entries(m, V):
    """Five words per name, for min_count m and max_var V."""
    return {
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


# ------------------------------------------------------------ equal cells and equal box sums ----------------------------------
TIES = dict(H=20, W=40, d=64, mz=6, w=100)


def _yx(*cells):
    """Cells of the 40-wide grid of shift 0, by flat index, as (y, x)."""
    return tuple((c // TIES["W"], c % TIES["W"]) for c in cells)


# name: (cell_shift, box, the voting pixels (y, x), the joint that rule V5 gives, worked by hand).  At shift 0 the grid has 800
# cells and thread t of k_votes_modes meets cells t, t + 256, t + 512 (and t + 768 for t < 32).  Every voting pixel adds 100 to
# its own cell, at vz = 70; a cell (cx, cy) of shift 0 has its centre at (16 cx + 8, 16 cy + 8).
TIE_LAYOUTS = {
    # threads 4 and 6 meet in the reduction's step s = 2: `ob >= s_best[tid]` would hand thread 4 the cell of thread 6
    "cells 4 and 6": (0, 0, _yx(4, 6), (72, 8, 70, 100)),
    # cell 100 = (2, 20) is thread 100's, cell 300 = (7, 20) thread 44's: the lower index is held by the higher thread
    "cells 100 and 300": (0, 0, _yx(100, 300), (328, 40, 70, 100)),
    # cell 44 = (1, 4) and cell 300: thread 44 meets the same sum at c and at c + 256
    "cells 44 and 300": (0, 0, _yx(44, 300), (72, 24, 70, 100)),
    "cells 44, 300 and 556": (0, 0, _yx(44, 300, 556), (72, 24, 70, 100)),                  # ... and at c + 512 = (13, 36)
    # (1, 10), (3, 2), (5, 7): the middle one in row-major order has the lowest column, so it is first in column-major order
    "three cells, the middle one leftmost": (0, 0, ((1, 10), (3, 2), (5, 7)), (168, 24, 70, 100)),
    # box 1.  Three pixels under the top border, three on the left one: S = 300 at (cx, cy) = (11, 0), (11, 1), (0, 10) and
    # (1, 10).  (11, 0) wins, its box clipped to rows 0..1: X = (168 + 200 + 184) / 3 = 184, Y = floor((8 + 8 + 24) / 3) = 13.
    # Column-major order takes (0, 10), whose box is clipped to columns 0..1.
    "box 1: equal sums under the top and on the left border": (0, 1, ((0, 10), (0, 12), (1, 11), (9, 0), (11, 0), (10, 1)), (184, 13, 70, 300)),
    # box 1.  S = 300 at (0, 10), (1, 10) on the left border and at (38, 11), (39, 11) on the right one, a row further down.
    # (0, 10) wins: X = floor((8 + 8 + 24) / 3) = 13, Y = (152 + 184 + 168) / 3 = 168.  One cell to the left of the winner's
    # box is, in memory, the last cell of the row above: (39, 10) holds a vote that the box must not take.
    "box 1: equal sums on the left and the right border": (0, 1, ((9, 0), (11, 0), (10, 1), (10, 39), (12, 39), (11, 38)), (13, 168, 70, 300)),
    # box 4.  (0, 0), (2, 3), (4, 1) in the top left corner: S = 300 for cx, cy in 0..4; (0, 0) wins with its box clipped to
    # 5 x 5 cells: X = floor((8 + 40 + 72) / 3) = 40, Y = floor((8 + 56 + 24) / 3) = 29.  (22, 19), (25, 18), (20, 17) under the
    # bottom border: S = 300 as well, later in both orders; the last tie is (29, 19).
    "box 4: equal sums in a corner and on the bottom border": (0, 4, ((0, 0), (3, 2), (1, 4), (19, 22), (18, 25), (17, 20)), (40, 29, 70, 300)),
    # shift 1: a cell holds up to four pixels.  Cell (0, 2) holds 400, the largest; cells (10, 6), (11, 6) and (10, 7) hold
    # 300 each.  Box 1: S = 900 first at (10, 6): X = floor((336 + 368 + 336) / 3) = 346, Y = floor((208 + 208 + 240) / 3) = 218.
    "box 1 at shift 1: the largest cell outside the winning box": (
        1, 1, ((4, 0), (4, 1), (5, 0), (5, 1), (12, 20), (12, 21), (13, 20), (12, 22), (13, 23), (12, 23), (14, 20), (15, 21), (14, 21)),
        (346, 218, 70, 900)),
    # ... box 4: the box of (7, 2) ends at row 6 and leaves out (10, 7): S = 600.  The first cell whose box holds all three is
    # (7, 3): rows 0..7 after clipping by the top border, columns 3..11; column 0 with its 400 stays outside.  The same joint.
    "box 4 at shift 1: the largest cell outside the winning box": (
        1, 4, ((4, 0), (4, 1), (5, 0), (5, 1), (12, 20), (12, 21), (13, 20), (12, 22), (13, 23), (12, 23), (14, 20), (15, 21), (14, 21)),
        (346, 218, 70, 900)),
}


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """(depth [1, 20, 40] of 64 everywhere, forest, votes int32 [1, 1, 2, 1, 4], gate, cell_shift, box): the one joint stays on
    the voting pixel, (0, 0, 6, 100), so the accumulator is what the gate draws."""
    m = TIES
    shift, box, pixels, _ = TIE_LAYOUTS[name]
    depth = np.full((1, m["H"], m["W"]), m["d"], np.uint16)
    votes = np.zeros((1, 1, 2, 1, 4), np.int32)
    votes[0, 0, 0, 0] = (0, 0, m["mz"], m["w"])
    gate = np.zeros(depth.shape, np.uint16)
    for y, x in pixels:
        gate[0, y, x] = 1
    forest = all_left_stump()
    _freeze(depth, votes, gate, forest)
    return depth, forest, votes, gate, shift, box


# ------------------------------------------------------------ a box sum above 2^31 - 1 ------------------------------------------
SUM = dict(T=405, H=144, W=144, d=1000, mz=7, shift=4)
SUM_BEST = 144 * 144 * 256 * 405                           # 2149908480: above 2^31 - 1, below 2^32
SUM_RUNS = ((4, 1), (0, 1), (4, SUM_BEST), (4, SUM_BEST + 1))               # (box, min_support)


def full_grid(H, W, T, d, mz, shift):
    """The accumulators (acc [1, 1, Ha, Wa], zacc) of T all-left stumps whose one joint is (0, 0, mz, 256), on a frame of depth
    d everywhere without a gate, in closed form: every pixel adds 256 per tree to its own cell, at vz = d + mz."""
    side = 1 << shift
    assert H % side == 0 and W % side == 0 and side * side * T * 256 < 1 << 32
    acc = np.full((1, 1, H >> shift, W >> shift), side * side * T * 256, np.uint32)
    return acc, acc.astype(np.uint64) * np.uint64(d + mz)


def sum_case(T=SUM["T"], H=SUM["H"], W=SUM["W"]):
    """(depth [1, H, W] of one depth, forest [T, 1, 9], votes int32 [T, 1, 2, 1, 4])."""
    depth = np.full((1, H, W), SUM["d"], np.uint16)
    forest = np.concatenate([all_left_stump()] * T)
    votes = np.zeros((T, 1, 2, 1, 4), np.int32)
    votes[:, 0, 0, 0] = (0, 0, SUM["mz"], 256)
    return depth, forest, votes


# ------------------------------------------------------------ 128 m + d on both sides of +-2^31 ---------------------------------
WIDE = dict(W=20000, J=12, shift=4)
# The pixels that vote, one per frame of the batch: (x, depth).  A vote at these depths moves by 2^31 / (2 d) = 16384 pixels at
# the least, hence the width; with cells of 16 pixels rule V5's restatement visits 1250 cells per (frame, joint), not 20000.
# The columns are chosen so that every vote of joints 0 and 1 lands in the LAST column of a cell, 15 (mod 16), and one column
# more is another cell: 15 + 16416, 31 + 16416, 19007 - 16416 and 19024 - 16417.  A quotient that is truncated where V4
# floors, or rounded up, is one more.
WIDE_PIXELS = ((15, 65407), (31, 65408), (19007, 65409), (19024, 65408))
# the table's joints (mx, w); my = mz = 0.  128 * 16776705 = 2^31 - 65408, 128 * 16777727 = 2^31 + 65408.
WIDE_JOINTS = (
    (16776705, 9),            # 128 m + d = 2^31 - 1 at d = 65407, 2^31 at d = 65408: both move by 16416 pixels
    (-16777727, 9),           # -2^31 + 1 at d = 65409 (-16416 pixels), -2^31 at d = 65408 (-16417 pixels)
    (25165824, 9),            # 3 * 2^30 + d: 24624 pixels, outside; read in 32 bits it is -2^30 + d, -8208 pixels: inside from 19024
    ((1 << 31) - 1, 9), (-(1 << 31) + 1, 9), (-(1 << 31), 9),              # millions of pixels away: dropped
    (0, 257), (0, -1), (0, -256), (0, (1 << 31) - 1), (0, -(1 << 31)),     # weights that are no vote
    (0, 256),                 # a vote on the pixel itself: the pixel takes part
)


@functools.lru_cache(maxsize=None)
def wide_case():
    """(depth [4, 1, 20000], forest, votes int32 [1, 1, 2, 12, 4], gate [4, 1, 20000]): frame i lets WIDE_PIXELS[i] alone vote."""
    m = WIDE
    depth = np.full((len(WIDE_PIXELS), 1, m["W"]), 1000, np.uint16)
    gate = np.zeros(depth.shape, np.uint16)
    for i, (x, d) in enumerate(WIDE_PIXELS):
        depth[:, 0, x] = d
        gate[i, 0, x] = 1
    votes = np.zeros((1, 1, 2, m["J"], 4), np.int32)
    for j, (mx, w) in enumerate(WIDE_JOINTS):
        votes[0, 0, 0, j] = (mx, 0, 0, w)
    forest = all_left_stump()
    _freeze(depth, gate, votes, forest)
    return depth, forest, votes, gate


# ------------------------------------------------------------ a fall-off in the second of three trees --------------------------
def middle_case():
    """hand_case()'s frame, labels and target under three stumps: the first and the third are hand_case()'s, the second has a
    "go on" flag on its left side, at level D - 1 = 0: the hand pixels with x <= 5 fall off there and must still sum, and
    vote, through the first and the third tree."""
    depth, labels, targets, stump = hand_case()
    forest = np.concatenate([stump, stump, stump])
    forest[1, 0, 5] = -1.
    forest[2, 0, 0] = 64.                                   # the third probes (x + 1, y): x = 6 goes left there
    return depth, labels, targets, forest


MIDDLE_FIT = dict(min_count=1, max_var=16)                  # the third tree's left slot has variance 5: it votes


# ------------------------------------------------------------ past one sweep of a grid ------------------------------------------
# forest_votes_hip.hip, lines 32 to 34: kThreads = 256, kMaxBlocks = 1024 (count and fit), kMaxModeBlocks = 65536 (modes)
SWEEP = 1024 * 256                                          # pixels of one sweep of k_votes_count, nodes of one of k_votes_fit
MODE_SWEEP = 65536                                          # (frame, joint) pairs of one sweep of k_votes_modes
COUNT_SWEEP = dict(n=2, H=367, W=401, J=2, radius=255, seed=91, drawn=40)


def count_sweep_flat():
    """The flat indices of the labelled pixels: the ends of the first sweep, both sides of the image boundary (which lies
    inside a wave: 367 * 401 = 147167 = 2299 * 64 + 31), the last pixel, and `drawn` seeded ones in each sweep."""
    m = COUNT_SWEEP
    pix, total = m["H"] * m["W"], m["n"] * m["H"] * m["W"]
    rng = np.random.default_rng(m["seed"])
    flat = [0, SWEEP - 1, SWEEP, pix - 2, pix - 1, pix, pix + 1, total - 1]
    flat += rng.choice(SWEEP, m["drawn"], replace=False).tolist() + (SWEEP + rng.choice(total - SWEEP, m["drawn"], replace=False)).tolist()
    return sorted(set(int(f) for f in flat))


@functools.lru_cache(maxsize=None)
def count_sweep_case():
    """(depth [2, 367, 401], labels, targets int32 [2, 2, 3], forest [1, 1, 9]): no label and no depth anywhere but at the
    pixels of count_sweep_flat().  The stump is hand_case()'s: it probes 128 / d pixels to the right against the pixel itself.
    Every third pixel gets its own depth written two pixels to its right, so that both leaf slots are used; one in seven has a
    label and no depth.  Joint 0 is within the radius of every pixel of the frame, joint 1 of a corner's."""
    m = COUNT_SWEEP
    depth = np.full((m["n"], m["H"], m["W"]), 65535, np.uint16)
    labels = np.zeros(depth.shape, np.uint16)
    at = [np.unravel_index(f, depth.shape) for f in count_sweep_flat()]
    ds = [(64, 100, 128, 333, 65534)[k % 5] for k in range(len(at))]
    for k, (i, y, x) in enumerate(at):
        if k % 3 == 0 and x + 2 < m["W"]:
            depth[i, y, x + 2] = ds[k]
    for k, (i, y, x) in enumerate(at):
        labels[i, y, x] = 1 + k % 9
        depth[i, y, x] = 0 if k % 7 == 5 else ds[k]
    targets = np.array([[[200, 183, 700], [30, 40, 900]], [[200, 183, 650], [380, 350, 1200]]], np.int32)
    forest = hand_case()[3]
    _freeze(depth, labels, targets, forest)
    return depth, labels, targets, forest


FIT_SWEEP = dict(T=5, D=16, min_count=5, max_var=1000, seed=17)


@functools.lru_cache(maxsize=None)
def fit_sweep_case():
    """(forest [5, 65535, 9], sums uint64 [5, 65535, 2, 1, 5], slots {name: (t, n, s, 0)}, leaf [(t, n, s)]).  327675 nodes.
    (votes_numpy.fit asks a slot's flag only where the node is reachable, and refit_numpy.reachable_nodes a parent's flag only
    where the parent is: 0.2 s for both at this size, so the restatement itself gives the expected table.)
    Every flag says "leaf slot" but for one "go on" path per tree from the root to level 15, drawn; the last tree's path starts
    to the right, so all of it from level 2 on lies past node 262144 of the forest (node 4 of tree 4).  The reachable leaf
    slots are the 15 sides next to a path and the two sides of its end: 17 a tree.  fit_entries' sums go on them tree by
    tree from the deepest up; `unreachable` is the other child of the last tree's path at level 3."""
    m = FIT_SWEEP
    T, D = m["T"], m["D"]
    N = (1 << D) - 1
    rng = np.random.default_rng(m["seed"])
    forest = np.zeros((T, N, 9), np.float32)
    forest[:, :, 4] = 1.
    dead = None
    for t in range(T):
        n = 0
        for level in range(D - 1):
            s = 1 if t == T - 1 and level == 0 else int(rng.integers(2))
            forest[t, n, 5 + s] = -1.
            if t == T - 1 and level == 3:
                dead = (t, 2 * n + 1 + (1 - s), 1)
            n = 2 * n + 1 + s
    leaf = [(int(t), int(n), s) for t, n in np.argwhere(rn.reachable_nodes(forest)) for s in (0, 1) if rn.is_leaf_slot(forest[t, n], s)]
    sums = np.zeros((T, N, 2, 1, 5), np.uint64)
    entries = fit_entries(m["min_count"], m["max_var"])
    slots = {}
    for t in range(T):
        own = [slot for slot in leaf if slot[0] == t][::-1]
        for k, (name, e) in enumerate(entries.items()):
            sums[own[k]][0] = [_u64(v) for v in e]
            slots[f"{name} in tree {t}"] = own[k] + (0,)
    sums[dead][0] = [_u64(v) for v in (100, 100, 100, 100, 100)]
    slots["unreachable"] = dead + (0,)
    _freeze(forest, sums)
    return forest, sums, slots, leaf


MODES = dict(frames=4097, J=16, seed=5)
# the 2 x 2 frames the batch is drawn from: depth 64 moves a vote by mx pixels, 128 by mx / 2 rounded half up, 640 by none
MODE_KINDS = np.array([[[64, 64], [64, 64]], [[128, 64], [0, 128]], [[640, 65535], [128, 64]], [[65535, 0], [0, 65535]],
                       [[64, 640], [640, 128]], [[3000, 3000], [64, 0]], [[128, 128], [128, 128]], [[0, 0], [0, 700]]], np.uint16)


@functools.lru_cache(maxsize=None)
def modes_sweep_case():
    """(depth [4097, 2, 2], forest, votes int32 [1, 1, 2, 16, 4], kind [4097]): 65552 (frame, joint) pairs.  Frame i is
    MODE_KINDS[kind[i]]; frames 0 and 4096, whose pairs one workgroup of a grid of 65536 handles one after the other, are of
    different kinds.  A frame's joints depend on that frame alone, so the restatement runs on the eight kinds."""
    m = MODES
    rng = np.random.default_rng(m["seed"])
    kind = rng.integers(0, len(MODE_KINDS), m["frames"])
    kind[0], kind[m["frames"] - 1] = 0, 6
    votes = np.zeros((1, 1, 2, m["J"], 4), np.int32)
    for j in range(m["J"]):
        votes[0, 0, 0, j] = ((0, 1, -1, 2)[j % 4], (0, 0, 1, -1, 1)[j % 5], 10 * j - 50, 1 + 15 * j)
    depth = np.ascontiguousarray(MODE_KINDS[kind])
    forest = all_left_stump()
    _freeze(depth, votes, forest, kind)
    return depth, forest, votes, kind


def vote_by_kind(mod, shift=0, box=0):
    """`mod.vote` of modes_sweep_case(): the eight kinds voted, then dealt out to the frames."""
    depth, forest, votes, kind = modes_sweep_case()
    return np.ascontiguousarray(mod.vote(MODE_KINDS, forest, votes, shift=shift, box=box)[kind])


# ------------------------------------------------------------ mutants ---------------------------------------------------------
def _i32(expr):
    """Source text: `expr` read as an int32, two's complement."""
    return f"((({expr}) + (1 << 31)) % (1 << 32) - (1 << 31))"



_VOTE = "return (128 * int(m) + int(d)) // (2 * int(d))"
_KEPT = "if not (0 <= vx < W and 0 <= vy < H and 1 <= vz <= 65534):"
_ACC = "acc[i, j, vy >> shift, vx >> shift] += np.uint32(w)"
_ZACC = "zacc[i, j, vy >> shift, vx >> shift] += np.uint64(w * vz)"
# a vote kept at vx == W or vy == H lands in the last cell of its row or column: the copy's index stays inside the array
_CLAMPED = [(_ACC, "acc[i, j, min(vy >> shift, acc.shape[2] - 1), min(vx >> shift, acc.shape[3] - 1)] += np.uint32(w)"),
            (_ZACC, "zacc[i, j, min(vy >> shift, acc.shape[2] - 1), min(vx >> shift, acc.shape[3] - 1)] += np.uint64(w * vz)")]
# a weight outside 1..256 that is taken for a vote is added as the uint32 it is read as
_WRAPPED = [(_ACC, "acc[i, j, vy >> shift, vx >> shift] += np.uint32(w & 0xffffffff)"),
            (_ZACC, "zacc[i, j, vy >> shift, vx >> shift] += np.uint64((w & 0xffffffff) * vz)")]
_MEANS = "mx, my, mz = (signed64(word[k]) // n for k in (1, 2, 3))"
_S = "S = int(acc[max(cy - box, 0):cy + box + 1, max(cx - box, 0):cx + box + 1].sum(dtype=np.uint64))"
_ROWS = "for yy in range(max(cy - box, 0), min(cy + box, Ha - 1) + 1):"
_COLS = "for xx in range(max(cx - box, 0), min(cx + box, Wa - 1) + 1):"
_JOINT = "return (sx // best, sy // best, sz // best, min(best, (1 << 31) - 1))"

EDITS = {
    # V1
    "absent read as tz < 0": [("return tz <= 0 or tz >= 65535", "return tz < 0 or tz >= 65535")],
    "absent read as tz > 65535": [("return tz <= 0 or tz >= 65535", "return tz <= 0 or tz > 65535")],
    "offset truncated towards 0": [("return (int(delta) * int(d)) // 64", "return abs(int(delta) * int(d)) // 64 * (1 if delta >= 0 else -1)")],
    "depth 65535 walked in the count": [("if d == 0 or d == NO_PIXEL:\n            tot[1] += 1", "if d == 0:\n            tot[1] += 1")],
    "radius read as >=": [("if abs(dx) > radius or abs(dy) > radius:", "if abs(dx) >= radius or abs(dy) >= radius:")],
    "radius along x only": [("if abs(dx) > radius or abs(dy) > radius:", "if abs(dx) > radius:")],
    "radius Euclidean": [("if abs(dx) > radius or abs(dy) > radius:", "if dx * dx + dy * dy > radius * radius:")],
    "oz sign": [("offset(dy, d), tz - d", "offset(dy, d), d - tz")],
    "squares of x only": [("(1, ox, oy, oz, ox * ox + oy * oy)", "(1, ox, oy, oz, ox * ox)")],
    "a fall-off ends the pixel's sums": [("tot[2] += 1\n                continue", "tot[2] += 1\n                break")],
    # V2
    "n <= min_count": [("if n < min_count or n >= 1 << 26:", "if n <= min_count or n >= 1 << 26:")],
    "n > 2^26": [("if n < min_count or n >= 1 << 26:", "if n < min_count or n > 1 << 26:")],
    "mean truncated": [(_MEANS, "mx, my, mz = (abs(signed64(word[k])) // n * (1 if signed64(word[k]) >= 0 else -1) for k in (1, 2, 3))")],
    "sums read unsigned": [(_MEANS, "mx, my, mz = (" + _i32("int(word[k]) // n") + " for k in (1, 2, 3))")],
    "variance as an absolute value": [("var = max(0, int(word[4]) // n - (mx * mx + my * my))", "var = abs(int(word[4]) // n - (mx * mx + my * my))")],
    "var >= max_var": [("if var > max_var:", "if var >= max_var:")],
    "weight over max_var, not max_var + 1": [("return 256 - (var * 256) // (max_var + 1)", "return 256 - (var * 256) // max(max_var, 1)")],
    "weight 255": [("return 256 - (var * 256) // (max_var + 1)", "return 255 - (var * 256) // (max_var + 1)")],
    "fit ignoring reachability": [("if not (reach[t, n] and is_leaf_slot(forest[t, n], s)):", "if not is_leaf_slot(forest[t, n], s):")],
    # V3, V4
    "vote rounded half down": [(_VOTE, "return -((int(d) - 128 * int(m)) // (2 * int(d)))")],
    "vote truncated": [(_VOTE, "return abs(64 * int(m)) // int(d) * (1 if m >= 0 else -1)")],
    "vote floored without the half": [(_VOTE, "return (64 * int(m)) // int(d)")],
    "128 m + d in 32 bits": [(_VOTE, "return " + _i32("128 * int(m) + int(d)") + " // (2 * int(d))")],
    "gate 65535 passes": [("int(gate[i, y, x]) in (0, NO_PIXEL):", "int(gate[i, y, x]) == 0:")],
    "depth 65535 votes in the cast": [("if d == 0 or d == NO_PIXEL:\n                    continue", "if d == 0:\n                    continue")],
    "a fall-off ends the pixel's votes": [("if at is None:\n                        continue", "if at is None:\n                        break")],
    "w >= 1 votes": [("if w < 1 or w > 256:", "if w < 1:")] + _WRAPPED,
    "negative w votes": [("if w < 1 or w > 256:", "if w == 0 or w > 256:")] + _WRAPPED,
    "vz 0 kept": [(_KEPT, _KEPT.replace("1 <= vz", "0 <= vz"))],
    "vz 65535 kept": [(_KEPT, _KEPT.replace("vz <= 65534", "vz <= 65535"))],
    "vx == W kept": [(_KEPT, _KEPT.replace("vx < W", "vx <= W"))] + _CLAMPED,
    "vy == H kept": [(_KEPT, _KEPT.replace("vy < H", "vy <= H"))] + _CLAMPED,
    "zacc weighted by d, not vz": [(_ZACC, _ZACC.replace("w * vz", "w * d"))],
    "reduce reading (x, y), not (x r, y r)": [("xd, yd = x * r, y * r", "xd, yd = x, y")],
    # V5
    "last tie wins": [("if S > best:", "if S >= best:")],
    "column-major ties": [("for cy in range(Ha):\n        for cx in range(Wa):", "for cx in range(Wa):\n        for cy in range(Ha):")],
    # (without a winner the copy takes cell (0, 0) and divides by 1, where a kernel would divide by 0)
    "min_support 0 is 0": [("if best < max(min_support, 1):", "if best < min_support:"), ("best, win = 0, None", "best, win = 0, (0, 0)"),
                           (_JOINT, _JOINT.replace("// best", "// max(best, 1)"))],
    "support <=": [("if best < max(min_support, 1):", "if best <= max(min_support, 1):")],
    "cell centre at +8 whatever the shift": [("sx += w * (16 * (xx << shift) + 8 * (1 << shift))", "sx += w * (16 * (xx << shift) + 8)"),
                                             ("sy += w * (16 * (yy << shift) + 8 * (1 << shift))", "sy += w * (16 * (yy << shift) + 8)")],
    # the columns of the centroid's box not clipped: in memory the cell left of column 0 is the last of the row above (the
    # copy's index stays inside the array)
    "centroid over an unclipped box": [(_COLS, "for xx in range(cx - box, cx + box + 1):"),
                                       ("w = int(acc[yy, xx])", "w = int(acc.reshape(-1)[min(max(yy * Wa + xx, 0), acc.size - 1)])"),
                                       ("sz += int(zacc[yy, xx])", "sz += int(zacc.reshape(-1)[min(max(yy * Wa + xx, 0), acc.size - 1)])")],
    "centroid over the winner alone": [(_ROWS, "for yy in range(cy, cy + 1):"), (_COLS, "for xx in range(cx, cx + 1):")],
    "S in 32 bits": [(_S, "S = " + _i32(_S[4:]))],
    "support not clamped": [(_JOINT, _JOINT.replace("min(best, (1 << 31) - 1)", "best & 0x7fffffff"))],
}
MUTANTS = tuple(EDITS)


@functools.lru_cache(maxsize=None)
def mutant(name=None):
    """tests/votes_numpy.py under one wrong reading; the unchanged copy without a name."""
    return mutants.load("votes_numpy", EDITS[name] if name else ())


# ------------------------------------------------------------ what the device tests compare -----------------------------------
ADV_FIT = dict(min_count=2, max_var=1 << 22)
ADV_PARAMS = ((1, 0), (1, 255), (5, 0), (5, 255), (16, 0), (16, 255))       # (J, radius) of test_adversarial_count_fit_cast
CELLS_AND_BOXES = ((0, 0), (0, 4), (2, 1), (2, 0), (4, 1), (4, 4))          # (shift, box) of test_cast_cells_and_boxes


@functools.lru_cache(maxsize=None)
def adv_table(J, radius):
    """(sums, votes) of the restatement for the adversarial case at scale 1.0 with targets_for(J, radius)."""
    depth, labels, forest, _ = wc.adversarial_case()
    sums, _ = vn.count(depth, labels, targets_for(J, radius), forest, 1., radius, walk=memo_walk)
    votes, _ = vn.fit(forest, sums, **ADV_FIT)
    _freeze(sums, votes)
    return sums, votes


def reduce_gate():
    """test_cast_reduce_gates_and_support's gate: the labels at the pixels a reduce of 2 reads, then 65535, 0 and 9."""
    _, labels = wc.adversarial_frames()
    n, H, W = labels.shape
    gate = np.ascontiguousarray(labels[:, :H // 2 * 2:2, :W // 2 * 2:2])
    gate[0, 0, :3] = (65535, 0, 9)
    return gate


def reads_differently(mod, fname):
    """Whether `mod`'s function `fname`, or a function of the module that it calls, has other code than votes_numpy's."""
    seen, todo = set(), [fname]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        a, b = getattr(mod, f).__code__, getattr(vn, f).__code__
        if (a.co_code, a.co_consts, a.co_names) != (b.co_code, b.co_consts, b.co_names):
            return True
        todo += [n for n in b.co_names if hasattr(getattr(vn, n, None), "__code__")]
    return False


_stages = {}


def _adv_stage(mod, stage, J=5, radius=255, shift=2, gate=None, r=1, rerun=False):
    """`count`, `fit` or `cast` of the adversarial case under `mod`, remembered: the six boxes and the three supports read
    three accumulators.  A copy that reads the stage as the restatement does (reads_differently) is not run: the
    restatement's own result serves, so a mutant costs the stage it changes.  `rerun` runs the copy whatever its code."""
    if not rerun and not reads_differently(mod, stage):
        mod = vn
    key = (id(mod), stage, J, radius, shift, None if gate is None else gate.tobytes(), r)
    if key not in _stages:
        depth, labels, forest, _ = wc.adversarial_case()
        if stage == "count":
            got = mod.count(depth, labels, targets_for(J, radius), forest, 1., radius, walk=memo_walk)
        elif stage == "fit":
            got = mod.fit(forest, adv_table(J, radius)[0], **ADV_FIT)
        else:
            got = mod.cast(depth, forest, adv_table(J, radius)[1], 1., gate, r, shift, memo_walk)
        _stages[key] = (mod, got)                           # (the module is kept: its id is the key)
    return _stages[key][1]


def outputs(mod, name, rerun=False):
    """What the GPU test of case `name` compares with the restatement, under the restatement module `mod`: a list of arrays.
    Each stage starts from the true restatement's result of the stage before, as the device's does while it is right; a
    test that compares the device with itself alone has none."""
    out = []
    cast = lambda *a, **k: _adv_stage(mod, "cast", *a, rerun=rerun, **k)      # noqa: E731
    with np.errstate(all="ignore"):
        if name == "hand_worked_case_on_the_device":
            depth, labels, targets, forest = hand_case()
            h = HAND
            sums, totals = vn.count(depth, labels, targets, forest, radius=h["radius"])
            votes, _ = vn.fit(forest, sums, h["min_count"], h["max_var"])
            out += list(mod.count(depth, labels, targets, forest, radius=h["radius"])) + list(mod.fit(forest, sums, h["min_count"], h["max_var"]))
            out += [mod.vote(depth, forest, votes, gate=labels, shift=h["shift"], box=box) for box in (0, 1)]
        elif name.startswith("adversarial_count_fit_cast"):
            J, radius = (int(v) for v in name[name.index("[") + 1:-1].split("-"))
            out += list(_adv_stage(mod, "count", J, radius, rerun=rerun)) + list(_adv_stage(mod, "fit", J, radius, rerun=rerun))
            out.append(mod.modes(*cast(J, radius), 2, 1, 1))
        elif name == "fit_on_sums_written_directly":
            forest, sums, _ = fit_case()
            for min_count, max_var in ((FIT["min_count"], FIT["max_var"]), (1, 0), (1, 1 << 38), (1 << 26, 17)):
                out += list(mod.fit(forest, sums, min_count, max_var))
        elif name.startswith("cast_cells_and_boxes"):
            shift, box = (int(v) for v in name[name.index("[") + 1:-1].split("-"))
            out.append(mod.modes(*cast(shift=shift), shift, box, 1))
        elif name == "cast_reduce_gates_and_support":
            gate = reduce_gate()
            nothing = np.zeros_like(gate)
            nothing[:, ::2] = 65535
            best = int(vn.modes(*_adv_stage(vn, "cast"), 2, 1, 1)[..., 3].max())
            out += [mod.modes(*cast(gate=gate, r=2), 2, 1, 1), mod.modes(*cast(gate=nothing, r=2), 2, 1, 1)]
            out += [mod.modes(*cast(), 2, 1, support) for support in (best, best + 1)]
        elif name == "votes_on_and_next_to_every_border":
            depth, forest, votes, gate_one, gate_two = border_case()
            out += [mod.vote(depth, forest, votes, gate=g, shift=0, box=0) for g in (gate_one, gate_two)]
        elif name in ("more_frames_than_the_workspace_holds", "a_table_outlives_a_refit_of_the_pdfs"):
            out.append(mod.modes(*cast(), 2, 1, 1))
        elif name == "a_wave_on_one_cell_and_on_64_cells":
            depth, forest, votes = wave_case()
            out += [mod.vote(depth, forest, votes, shift=shift, box=box) for shift, box in ((0, 0), (0, 1), (2, 1))]
        elif name.startswith("mode_ties"):
            depth, forest, votes, gate, shift, box = tie_case(name[name.index("[") + 1:-1])
            out.append(mod.vote(depth, forest, votes, gate=gate, shift=shift, box=box))
        elif name == "box_sums_above_2_31":
            m = SUM
            acc, zacc = full_grid(m["H"], m["W"], m["T"], m["d"], m["mz"], m["shift"])
            out += [mod.modes(acc, zacc, m["shift"], box, support) for box, support in SUM_RUNS]
        elif name == "votes_that_need_64_bits_and_weights_that_are_none":
            depth, forest, votes, gate = wide_case()
            out.append(mod.vote(depth, forest, votes, gate=gate, shift=WIDE["shift"], box=0))
        elif name == "min_support_0":
            depth, forest, votes, gate_one, _ = border_case()
            out.append(mod.vote(depth, forest, votes, gate=gate_one, shift=0, box=0, min_support=0))
        elif name == "a_fall_off_in_a_middle_tree":
            depth, labels, targets, forest = middle_case()
            sums, _ = vn.count(depth, labels, targets, forest, radius=HAND["radius"])
            votes, _ = vn.fit(forest, sums, **MIDDLE_FIT)
            out += list(mod.count(depth, labels, targets, forest, radius=HAND["radius"])) + list(mod.fit(forest, sums, **MIDDLE_FIT))
            out += [mod.vote(depth, forest, votes, gate=labels, shift=HAND["shift"], box=box) for box in (0, 1)]
        elif name == "count_past_one_sweep":
            depth, labels, targets, forest = count_sweep_case()
            out += list(mod.count(depth, labels, targets, forest, radius=COUNT_SWEEP["radius"]))
        elif name == "fit_past_one_sweep":
            forest, sums, _, _ = fit_sweep_case()
            out += list(mod.fit(forest, sums, FIT_SWEEP["min_count"], FIT_SWEEP["max_var"]))
        elif name == "modes_past_one_sweep":
            out.append(vote_by_kind(mod))
        elif name not in DEVICE_ALONE:
            raise KeyError(name)
    return out


# GPU tests that compare the device with itself, or need the device to make their inputs: no reading can change what they see
DEVICE_ALONE = ("add_in_one_call_against_one_image_per_call", "table_save_and_load", "end_to_end_on_rendered_hands")

# device case (the GPU test's name without `test_`, then its parameters) -> exactly the readings that change what it compares
_RADIUS_0 = ("depth 65535 walked in the count", "radius read as >=", "radius along x only", "oz sign", "n <= min_count", "weight 255",
             "fit ignoring reachability", "zacc weighted by d, not vz", "cell centre at +8 whatever the shift", "centroid over the winner alone")
_RADIUS_255 = ("offset truncated towards 0", "depth 65535 walked in the count", "radius read as >=", "radius Euclidean", "oz sign",
               "squares of x only", "n <= min_count", "mean truncated", "sums read unsigned", "weight 255", "fit ignoring reachability")
_ABSENT = ("absent read as tz < 0", "absent read as tz > 65535", "radius along x only")
_PLAIN_CAST = ("vote truncated", "vote floored without the half", "zacc weighted by d, not vz")       # of the adversarial frames
_SHIFTED = ("cell centre at +8 whatever the shift",)
_WINNER = ("centroid over the winner alone",)
_NO_PIXEL = ("depth 65535 votes in the cast",)
_TIE = ("zacc weighted by d, not vz", "last tie wins")
_FIT = ("n <= min_count", "n > 2^26", "mean truncated", "sums read unsigned", "variance as an absolute value", "var >= max_var",
        "weight over max_var, not max_var + 1", "weight 255")
_HAND = ("radius read as >=", "radius Euclidean", "oz sign", "squares of x only", "n <= min_count", "weight over max_var, not max_var + 1",
         "weight 255", "vy == H kept", "zacc weighted by d, not vz") + _SHIFTED + _WINNER
KILLS = {
    "hand_worked_case_on_the_device": _HAND,
    "adversarial_count_fit_cast[1-0]": _RADIUS_0,
    "adversarial_count_fit_cast[1-255]": _RADIUS_255,
    "adversarial_count_fit_cast[5-0]": _RADIUS_0 + ("mean truncated",),
    "adversarial_count_fit_cast[5-255]": _RADIUS_255 + _ABSENT + _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER,
    "adversarial_count_fit_cast[16-0]": _RADIUS_0 + ("absent read as tz < 0",),
    "adversarial_count_fit_cast[16-255]": _RADIUS_255 + _ABSENT + _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER + (
        "vote rounded half down", "vz 0 kept", "vx == W kept", "vy == H kept", "last tie wins"),
    "add_in_one_call_against_one_image_per_call": (),
    "fit_on_sums_written_directly": _FIT + ("fit ignoring reachability",),
    "cast_cells_and_boxes[0-0]": _PLAIN_CAST + ("vx == W kept", "vy == H kept", "last tie wins"),
    "cast_cells_and_boxes[0-4]": _PLAIN_CAST + _NO_PIXEL + _WINNER + ("vy == H kept", "last tie wins"),
    "cast_cells_and_boxes[2-1]": _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER,
    "cast_cells_and_boxes[2-0]": _PLAIN_CAST + _SHIFTED,
    "cast_cells_and_boxes[4-1]": _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER + ("vx == W kept", "vy == H kept"),
    "cast_cells_and_boxes[4-4]": _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER + ("vx == W kept", "vy == H kept", "centroid over an unclipped box"),
    "cast_reduce_gates_and_support": _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER + (
        "gate 65535 passes", "reduce reading (x, y), not (x r, y r)", "support <="),
    "votes_on_and_next_to_every_border": _TIE + ("vz 0 kept", "vz 65535 kept", "vx == W kept"),
    "more_frames_than_the_workspace_holds": _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER,
    "a_wave_on_one_cell_and_on_64_cells": _PLAIN_CAST + _SHIFTED + _WINNER + ("last tie wins",),
    "table_save_and_load": (),
    "end_to_end_on_rendered_hands": (),
    "mode_ties[cells 4 and 6]": _TIE,
    "mode_ties[cells 100 and 300]": _TIE,
    "mode_ties[cells 44 and 300]": _TIE,
    "mode_ties[cells 44, 300 and 556]": _TIE,
    "mode_ties[three cells, the middle one leftmost]": _TIE + ("column-major ties",),
    "mode_ties[box 1: equal sums under the top and on the left border]": _TIE + _WINNER + ("column-major ties",),
    "mode_ties[box 1: equal sums on the left and the right border]": _TIE + _WINNER + ("centroid over an unclipped box",),
    "mode_ties[box 4: equal sums in a corner and on the bottom border]": _TIE + _WINNER + ("centroid over an unclipped box",),
    "mode_ties[box 1 at shift 1: the largest cell outside the winning box]": ("zacc weighted by d, not vz",) + _SHIFTED + _WINNER,
    "mode_ties[box 4 at shift 1: the largest cell outside the winning box]": ("zacc weighted by d, not vz",) + _SHIFTED + _WINNER,
    "box_sums_above_2_31": _SHIFTED + _WINNER + ("last tie wins", "support <=", "S in 32 bits", "support not clamped"),
    "votes_that_need_64_bits_and_weights_that_are_none": _SHIFTED + ("vote truncated", "128 m + d in 32 bits", "w >= 1 votes", "negative w votes"),
    "min_support_0": ("vz 0 kept", "vz 65535 kept", "vx == W kept", "zacc weighted by d, not vz", "min_support 0 is 0"),
    "a_fall_off_in_a_middle_tree": _HAND + ("a fall-off ends the pixel's sums", "a fall-off ends the pixel's votes", "last tie wins"),
    "count_past_one_sweep": ("offset truncated towards 0", "radius along x only", "radius Euclidean", "oz sign", "squares of x only"),
    "fit_past_one_sweep": _FIT + ("fit ignoring reachability",),
    "modes_past_one_sweep": ("vote rounded half down", "vote truncated", "vote floored without the half", "depth 65535 votes in the cast",
                             "vx == W kept", "vy == H kept", "zacc weighted by d, not vz", "last tie wins", "column-major ties", "support <="),
    "a_table_outlives_a_refit_of_the_pdfs": _PLAIN_CAST + _NO_PIXEL + _SHIFTED + _WINNER,
}
# readings that no input can tell from the rule: none.  Every reading tried is met by a case above.
EQUIVALENT = {}
