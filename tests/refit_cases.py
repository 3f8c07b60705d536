"""The hand-made cases of tests/test_refit.py: frames and forests built so that every rule of the leaf refit (R1 to R3 of
include/rdf_labels.h) is met by some pixel or slot, and the digit-coded leaf ids that let an EVALUATOR say which leaf slot a
pixel reaches."""
import importlib

import numpy as np

import refit_numpy as rn

NO_PIXEL = 65535


def _synth():
    return importlib.import_module("3d-beats_amd.synth")


# ------------------------------------------------------------ the case worked by hand ------------------------------------------
def hand_case():
    """One tree of two levels (three nodes), C = 3, on one 4 x 3 frame.  Every count and PDF is written out in the test.
        root: probes (x + 1, y) and (x, y) at depth 1000 (offsets 1000 and 0), thresh 50: du - dv < 50 goes left, to node 1
              (flag -1); the right side is a leaf slot.
        node 1: probes (x, y + 1) and (x, y), thresh 0; both sides leaf slots.   node 2: unreachable, stale bytes."""
    C = 3
    depth = np.array([[[1000, 1000, 1100, 1000],
                       [ 950,  900,    0, 1000],
                       [1000, 1000, 1000, 65535]]], np.uint16)
    labels = np.array([[[1, 2, 1, 2],
                        [0, 1, 2, 7],
                        [2, 0, 1, 1]]], np.uint16)
    tree = np.zeros((3, 7 + 2 * C), np.float32)
    tree[0, :7] = [1000., 0., 0., 0., 50., -1., 0.]
    tree[0, 7:] = [.5, .25, .25, .125, .125, .75]
    tree[1, :7] = [0., 1000., 0., 0., 0., 0., 0.]
    tree[1, 7:] = [0., 1., 0., 0., 0., 1.]
    tree[2, :] = 0.375                                   # never reached: flags 0.375 floor to 0
    return depth, labels, tree[None].copy(), C


# ------------------------------------------------------------ forests ---------------------------------------------------------
def trained_like(T, D, C, first=0, leaf_prob=0.3, min_leaf_level=1):
    s = _synth()
    return np.stack([s.trained_like_tree(first + k, D, C, leaf_prob, min(min_leaf_level, D - 1)) for k in range(T)])


def chain_tree(D, C):
    """Every pixel goes left at every level (no offsets: f = 0 < 1) and ends in the left leaf slot of level D - 1."""
    tree = np.zeros(((1 << D) - 1, 7 + 2 * C), np.float32)
    tree[:, 4] = 1.
    tree[:, 5:7] = -1.
    tree[(1 << (D - 1)) - 1:, 5:7] = 0.
    tree[:, 7:] = 1. / C
    return tree


def column_tree(D, C, width):
    """A full tree that sorts the pixels of a frame of depth 1000 everywhere by their column: node g of level j owns the
    columns from lo = g * (width >> j) on and asks whether the pixel lo + half columns to the left, half = width >> (j + 1),
    is still inside the frame.  u probes the pixel itself (1000), v that pixel: outside the left border (65535) iff x < lo +
    half, so f = -64535 < -30000 goes left for the lower half of the columns and f = 0 goes right.  With width = 2^D column x
    ends in slot (node x >> 1 of level D - 1, side x & 1): 2^D slots for 2^D columns."""
    tree = np.zeros(((1 << D) - 1, 7 + 2 * C), np.float32)
    tree[:, 5:7] = -1.
    tree[(1 << (D - 1)) - 1:, 5:7] = 0.
    tree[:, 7:] = 1. / C
    for j in range(D):
        for g in range(1 << j):
            tree[(1 << j) - 1 + g, :5] = [0., 0., -1000. * (g * (width >> j) + (width >> (j + 1))), 0., -30000.]
    return tree


# ------------------------------------------------------------ the main case --------------------------------------------------
MAIN = dict(n=2, H=9, W=70, T=3, D=4, C=5)


def main_case(seed=0):
    """2 images of 70 x 9 (neither a multiple of 8 nor of 64), T3/D4/C5 trees of synth.trained_like_tree with these roots and
    plants.  What the frames and trees contain is checked by test_main_case_meets_every_rule."""
    m = MAIN
    rng = np.random.default_rng(1234 + seed)
    depth = rng.integers(400, 1201, (m["n"], m["H"], m["W"])).astype(np.uint16)
    labels = rng.integers(0, m["C"] + 2, depth.shape).astype(np.uint16)         # 0 .. C + 1: ids 5 and 6 are unknown
    labels[rng.random(depth.shape) < 0.35] = 0
    labels[:, 3, 8:20] = 0                                # a run of 64 and more unlabelled pixels ends somewhere
    depth[:, 2:7, 40] = 0                                 # a column of zeros for probes to land on, unlabelled ...
    labels[:, 2:7, 40] = 0
    depth[0, 1, 5], labels[0, 1, 5] = 0, 2                # ... and depth 0 and 65535 under a label
    depth[1, 7, 66], labels[1, 7, 66] = NO_PIXEL, 3
    depth[1, 0, 0], labels[1, 0, 0] = 0, 1
    labels[0, 0, 0], labels[1, 8, 69] = 4, 1              # the first and the last pixel take part
    forest = trained_like(m["T"], m["D"], m["C"], first=40)
    # roots: every walk passes them.  At depth 400..1200 an offset of 3000 is 2 to 7 pixels
    forest[0, 0, :5] = [-3000., 0., 0., -5000., 10.]      # u off the left border, v off the top one (image 1: not image 0's rows)
    forest[1, 0, :5] = [4000., 0., 0., 4000., -10.]       # u off the right border (no wrap into the next row), v off the bottom
    forest[2, 0, :5] = [2500., 0., -2500., 0., 100.]      # both probes in the row: some land on the zero column
    forest[:, 0, 5:7] = -1.
    forest[2, 1, 4] = np.nan                              # a NaN threshold: everything goes right
    forest[2, 1, 6] = 0.
    forest[1, 1, 5], forest[1, 1, 6] = -0.5, 0.5          # floor(-0.5) = -1 goes on, floor(0.5) = 0 is a leaf slot
    forest[0, 2, :5] = [2000., 0., 0., 0., 0.]            # a neighbour nearer than the pixel itself: left,
    forest[0, 2, 5] = -1.                                 # on to level 2 ...
    forest[0, 5, :5] = [0., 0., 0., 0., 1.]               # ... where f = 0 < 1 goes left ...
    forest[0, 5, 5] = -1.
    forest[0, 11, :5] = [0., 0., 0., 0., 1.]              # ... and at level D - 1 the flag still says go on: off the tree
    forest[0, 11, 5] = -1.
    return depth, labels, forest


# ------------------------------------------------------------ digit-coded leaf ids --------------------------------------------
def n_digits(n_slots, C):
    k = 1
    while (C - 1) ** k < n_slots:
        k += 1
    return k


def digit_trees(tree, C):
    """Copies of one tree [N, E], C >= 3, one per digit position: slot k = 2n + s carries, as a one-hot PDF, digit p of k
    written in base C - 1 with the digits 1 .. C - 1.  An evaluator's label at a pixel is then that digit of the slot the
    pixel reached, and 0 (no PDF entry above 0) when it reached none."""
    assert C >= 3
    N = tree.shape[0]
    slots = np.arange(2 * N)
    out = []
    for p in range(n_digits(2 * N, C)):
        digit = 1 + (slots // (C - 1) ** p) % (C - 1)
        t = tree.copy()
        t[:, 7:] = 0.
        pdf = np.zeros((2 * N, C), np.float32)
        pdf[slots, digit] = 1.
        t[:, 7:] = pdf.reshape(N, 2 * C)
        out.append(t)
    return out


def slots_from_digits(label_maps, C):
    """label_maps: one evaluated label map per digit position (65535 where nothing was evaluated).  Returns (evaluated,
    fell_off, slot): bool, bool and int64 maps; slot is valid where evaluated and not fell_off."""
    maps = [m.astype(np.int64) for m in label_maps]
    evaluated = maps[0] != NO_PIXEL
    for m in maps:
        assert np.array_equal(m != NO_PIXEL, evaluated)
    zero = [m == 0 for m in maps]
    fell = evaluated & np.logical_and.reduce(zero)
    assert np.array_equal(evaluated & np.logical_or.reduce(zero), fell), "a slot's digits are all 1 .. C - 1 or all 0"
    slot = sum((np.where(evaluated & ~fell, m, 1) - 1) * (C - 1) ** p for p, m in enumerate(maps))
    return evaluated, fell, slot


def counts_from_slots(evaluated, fell, slot, labels, N, C):
    """np.bincount of (slot, label) over the live pixels as uint64 [N, 2, C], and the number of live pixels that fell off."""
    live = evaluated & (labels > 0) & (labels < C)
    hit = live & ~fell
    flat = np.bincount(slot[hit] * C + labels[hit].astype(np.int64), minlength=2 * N * C)
    return flat.astype(np.uint64).reshape(N, 2, C), int((live & fell).sum())


# ------------------------------------------------------------ apply -----------------------------------------------------------
def apply_case():
    """The main case's forest and counts with plants for rule R3.  Returns (forest, counts, chosen) where chosen = (t, n, s) is
    a reachable leaf slot with S >= 2 whose old PDF holds a NaN and a stale value."""
    depth, labels, forest = main_case()
    counts, _ = rn.count(depth, labels, forest)
    reach = rn.reachable_nodes(forest)
    chosen = None
    for n in range(forest.shape[1]):
        for s in (0, 1):
            if reach[1, n] and rn.is_leaf_slot(forest[1, n], s) and int(counts[1, n, s].sum()) >= 2 and chosen is None:
                chosen = (1, n, s)
    assert chosen is not None
    t, n, s = chosen
    C = MAIN["C"]
    forest[t, n, 7 + s * C] = np.nan
    forest[t, n, 7 + s * C + 1] = 123.25                  # a stale entry, as the trainer's one-hot rule leaves them
    forest[2, 14, :] = np.arange(17, dtype=np.float32) - 3.   # an unreachable node's bytes (node 1 of tree 2 is a leaf on its right)
    return forest, counts, chosen
