"""The hand-made cases of tests/test_prune.py: forests and counts built so that every rule of the pruning (P1 to P4 of
include/rdf_labels.h) is met by some node.  plan and apply take counts directly, so most cases set them here and need no
frames."""
import numpy as np

import refit_cases as rc
import refit_numpy as rn


# ------------------------------------------------------------ the case worked by hand ------------------------------------------
HAND_COST = 1


def hand_case():
    """One tree of three levels (seven nodes), C = 3, pruned with cost_per_leaf = 1.  Every number is written out in the test.
        root 0: both sides go on, to nodes 1 and 2.
        node 1: left goes on to node 3, right is a leaf slot whose PDF holds a stale 2.0 on the class no pixel has.
        node 2: left is a leaf slot whose PDF starts with a NaN, right goes on to node 6.
        nodes 3 and 6: leaves on both sides.   nodes 4 and 5: unreachable, stale bytes."""
    C = 3
    tree = np.zeros((7, 7 + 2 * C), np.float32)
    cnt = np.zeros((7, 2, C), np.uint64)
    tree[:, :5] = np.arange(35, dtype=np.float32).reshape(7, 5) + 0.5       # features: never read, must keep their bytes
    tree[0, 5:7] = [-1., -1.]
    tree[1, 5:7] = [-1., 0.]
    tree[1, 10:13] = [0., 2., 1.]
    cnt[1, 1] = [0, 0, 5]
    tree[2, 5:7] = [0., -1.]
    tree[2, 7:10] = [np.nan, .5, .5]
    cnt[2, 0] = [0, 1, 1]
    tree[3, 7:13] = [0., 1., 0., .2, .3, .5]
    cnt[3, 0], cnt[3, 1] = [0, 3, 1], [0, 1, 2]
    tree[4], tree[5] = 0.375, -7.25                                        # never reached
    tree[6, 7:13] = [0., 1., 0., 0., 0., 1.]
    cnt[6, 0], cnt[6, 1] = [0, 6, 0], [0, 0, 4]
    return tree[None].copy(), cnt[None].copy(), C


# ------------------------------------------------------------ the column tree of the issue ------------------------------------
def column_case(seed=3, rows=5, noise=0.2):
    """column_tree(5, 4, 32) with random leaf PDFs on a frame of depth 1000 whose labels depend on x >> 3 (four runs of eight
    columns, the four sides of level 1) with 20 % of them redrawn.  Returns (depth, labels, forest)."""
    D, C, W = 5, 4, 32
    rng = np.random.default_rng(seed)
    tree = rc.column_tree(D, C, W)
    last = (1 << (D - 1)) - 1
    pdf = rng.random((tree.shape[0] - last, 2, C)).astype(np.float32)
    tree[last:, 7:] = (pdf / pdf.sum(axis=2, keepdims=True, dtype=np.float32)).reshape(-1, 2 * C)
    depth = np.full((1, rows, W), 1000, np.uint16)
    labels = np.broadcast_to(1 + (np.arange(W) >> 3) % 3, (1, rows, W)).astype(np.uint16)
    redraw = rng.random(labels.shape) < noise
    labels = np.where(redraw, rng.integers(1, C, labels.shape), labels).astype(np.uint16)
    return depth, labels, tree[None].copy()


# ------------------------------------------------------------ forests and counts ----------------------------------------------
def reachable_leaf_slots(forest):
    reach = rn.reachable_nodes(forest)
    return [(t, n, s) for t in range(forest.shape[0]) for n in range(forest.shape[1]) for s in (0, 1)
            if reach[t, n] and rn.is_leaf_slot(forest[t, n], s)]


def random_counts(forest, rng, good=0.45, empty=0.25, high=12, slots=None):
    """Counts in the reachable leaf slots only (what rule R2 leaves): a `good` share of the slots holds pixels of the class its
    PDF answers with and at times one of another, an `empty` share holds none, the rest a few of any class.  No pixel has
    label 0 -- but with C = 2 class 0 takes part: one class alone would leave nothing to decide."""
    import prune_numpy as pn
    T, D, C = rn.dims(forest)
    lo = 0 if C == 2 else 1
    counts = np.zeros((T, forest.shape[1], 2, C), np.uint64)
    for t, n, s in reachable_leaf_slots(forest) if slots is None else slots:
        r = rng.random()
        if r < good:
            k = max(pn.argmax_e(forest[t, n, 7 + s * C:7 + (s + 1) * C]), lo)
            counts[t, n, s, k] = rng.integers(3, high)
            counts[t, n, s, lo + rng.integers(0, C - lo)] += rng.integers(0, 2)
        elif r < 1. - empty:
            counts[t, n, s, lo:] = rng.integers(0, 4, C - lo)
    return counts


MAIN = dict(T=3, D=6, C=5, seed=12)
# (cost_per_leaf, min_count, max_levels): the error rule alone with a price, a minimum support, a depth limit
MAIN_PARAMS = [(1, 0, 6), (0, 0, 6), (0, 14, 6), (2, 0, 3)]


def main_case():
    """T3/D6/C5 trees of synth.trained_like_tree with random counts and these plants; tree 2 has no pixel at all.  What the
    case contains is checked by test_main_case_meets_every_rule.  Returns (forest, counts)."""
    m = MAIN
    C = m["C"]
    rng = np.random.default_rng(4321 + m["seed"])
    forest = rc.trained_like(m["T"], m["D"], C, first=60, leaf_prob=0.25)
    counts = random_counts(forest, rng)
    counts[2] = 0
    reach = rn.reachable_nodes(forest)
    # flags that floor to -1 and to 0, and a NaN (a leaf slot): the structure stays
    assert forest[1, 0, 5] == -1.
    forest[1, 0, 5] = -0.5
    leaf = [(t, n, s) for t, n, s in reachable_leaf_slots(forest) if t == 1]
    forest[1, leaf[0][1], 5 + leaf[0][2]] = 0.5
    forest[1, leaf[1][1], 5 + leaf[1][2]] = np.nan
    # old PDFs: one with a NaN in front, one of zeros (k* = 0: every pixel is an error), one with a stale entry above the true maximum
    full = [(t, n, s) for t, n, s in reachable_leaf_slots(forest) if t == 0 and int(counts[t, n, s].sum()) >= 3]
    (t, n, s), z, st = full[0], full[1], full[2]
    forest[t, n, 7 + s * C] = np.nan
    forest[z[0], z[1], 7 + z[2] * C:7 + (z[2] + 1) * C] = 0.
    k = int(np.argmax(counts[st]))
    forest[st[0], st[1], 7 + st[2] * C + (k % (C - 1)) + 1] = 123.25
    # a "go on" at level D - 1 under a node that stays: the first reachable node of the last level in tree 0 falls off to the left
    last = (1 << (m["D"] - 1)) - 1
    n = last + int(np.argmax(reach[0, last:]))
    assert reach[0, n]
    forest[0, n, 5] = -1.
    counts[0, n, 0] = 0
    # an unreachable node with stale bytes and stale counts
    n = int(np.argmin(reach[1]))
    assert not reach[1, n]
    forest[1, n] = np.arange(7 + 2 * C, dtype=np.float32) - 3.
    counts[1, n] = 7
    return forest, counts


def chain_case(D=12, C=3):
    """One tree of depth 12 in which one root-to-leaf chain is all that is reachable below level 1: every node of the chain
    goes on to the left and has a leaf slot on its right; the nodes beside it hold stale bytes.  The right slots alternate
    between two classes that their PDFs answer rightly, so with cost_per_leaf = 0 nothing but the chain's end collapses."""
    N = (1 << D) - 1
    tree = np.full((N, 7 + 2 * C), 0.625, np.float32)                       # stale everywhere: flags floor to 0
    counts = np.zeros((1, N, 2, C), np.uint64)
    for j in range(D):
        n = (1 << j) - 1                                                    # the leftmost node of level j
        tree[n, :5] = [0., 0., 0., 0., 1.]
        tree[n, 5:7] = [-1. if j < D - 1 else 0., 0.]
        k = 1 + j % 2
        tree[n, 7:] = 0.
        tree[n, 7 + C + k] = 1.
        counts[0, n, 1, k] = 5 + j
        if j == D - 1:
            tree[n, 7 + k] = 1.
            counts[0, n, 0, k] = 2
    return tree[None].copy(), counts


def _sparse_leaf_slots(forest):
    import prune_numpy as pn
    return [(t, n, s) for t, n in pn.reachable_order(forest) for s in (0, 1) if rn.is_leaf_slot(forest[t, n], s)]


DEEP = dict(T=520, D=11, C=3)


def deep_subtrees_case():
    """T520/D11/C3: with more than 512 trees only level 0 is the one workgroup's, and each of the 1040 nodes of level 1 roots a
    subtree of ten levels that one workgroup of 256 threads sweeps: 512 nodes, eight waves and two trips of the 256 threads at
    its last level.  Every record starts as stale bytes.
        tree 0: both subtrees nearly full (a side is a leaf with probability 0.03 from level 2 on): all waves live, with holes;
        tree 1: a sparse tree (probability 0.2): live lanes next to unreachable ones, waves that leave, levels that end early;
        tree 2: nearly full, but node 1's left side is a leaf slot: the left half of its subtree's levels is unreachable -- at
                the last level the whole first trip of the 256 threads -- with the trained records still there, stale;
        tree 519, the last: nearly full, the root's left side a leaf slot: only the last workgroup's subtree lives;
        every 40th tree: the root goes on to node 1, whose sides are leaf slots: a subtree that ends at its root;
        the rest: a root with two leaf slots, subtrees that never start.
    Returns (forest, counts)."""
    m = DEEP
    T, D, C = m["T"], m["D"], m["C"]
    s = rc._synth()
    rng = np.random.default_rng(520)
    N = (1 << D) - 1
    forest = np.full((T, N, 7 + 2 * C), 0.625, np.float32)
    forest[:, 0, 5:7] = 0.
    forest[:, 0, 7:] = rng.random((T, 2 * C)).astype(np.float32)
    for t, prob in ((0, 0.03), (1, 0.2), (2, 0.03), (T - 1, 0.03)):
        forest[t] = s.trained_like_tree(900 + t, D, C, prob, 2)
    forest[2, 1, 5] = 0.
    forest[2, 1, 7:7 + C] = [0.25, 0.5, 0.25]
    forest[T - 1, 0, 5] = 0.
    forest[T - 1, 0, 7:7 + C] = [0.125, 0.125, 0.75]
    for t in range(40, T - 1, 40):
        forest[t, 0, 5] = -1.
        forest[t, 1, 5:7] = 0.
        forest[t, 1, 7:] = rng.random(2 * C).astype(np.float32)
    counts = random_counts(forest, rng, slots=_sparse_leaf_slots(forest))
    return forest, counts


WIDE = dict(T=16385, D=2, C=2)


def wide_forest_case():
    """T16385/D2/C2: 32770 subtrees of one node, more workgroups than one row of a launch's grid (32768) holds, so the last
    two sit in a second row.  Every 1000th tree and the last three go on from the root on both sides; the rest are a root with
    two leaf slots.  Returns (forest, counts)."""
    m = WIDE
    T, D, C = m["T"], m["D"], m["C"]
    rng = np.random.default_rng(16385)
    forest = np.full((T, 3, 7 + 2 * C), 0.625, np.float32)
    forest[:, :, 5:7] = 0.
    forest[:, :, 7:] = rng.random((T, 3, 2 * C)).astype(np.float32)
    deep = list(range(0, T, 1000)) + [T - 3, T - 2, T - 1]
    forest[deep, 0, 5:7] = -1.
    slots = [(t, n, s) for t in deep for n in (1, 2) for s in (0, 1)] + [(t, 0, s) for t in range(1, T, 997) for s in (0, 1)]
    counts = random_counts(forest, rng, slots=slots)
    return forest, counts


def huge_counts(forest, rng):
    """Counts near 2^40 in every reachable leaf slot, none of them exact in fp32."""
    T, D, C = rn.dims(forest)
    counts = np.zeros((T, forest.shape[1], 2, C), np.uint64)
    for t, n, s in reachable_leaf_slots(forest):
        counts[t, n, s, 1:] = (np.uint64(1) << np.uint64(40)) + rng.integers(0, 1 << 33, C - 1).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    return counts
