"""Plain numpy restatement of the leaf refit, rules R1 to R3 of include/rdf_labels.h: `count` (the walk of every labelled
pixel to its leaf slot), `subtree_sums` and `apply` (counts to PDFs).  Written for reading, one pixel and one slot at a time;
the kernels of forest_refit_hip.hip must match it bit for bit.  tests/test_refit.py pins it to a case worked by hand and pins
its walk to the oracle's evaluator."""
import numpy as np

NO_PIXEL = 65535
KEEP, ANCESTOR = 0, 1


def dims(forest):
    T, N, E = forest.shape
    D = int(N + 1).bit_length() - 1
    assert (1 << D) - 1 == N and E >= 9 and (E - 7) % 2 == 0, forest.shape
    return T, D, (E - 7) // 2


def floor_i32(v):
    """float32 -> int: floor, saturated to int32, NaN -> 0."""
    v = np.float32(v)
    if np.isnan(v):
        return 0
    f = np.floor(np.float64(v))
    return int(min(max(f, -2147483648.), 2147483647.))


def wrap_i32(v):
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def is_leaf_slot(rec, s):
    return floor_i32(rec[5 + s]) != -1


def probe(frame, x, y):
    h, w = frame.shape
    if x < 0 or x >= w or y < 0 or y >= h:         # per axis: no wrap into the next row or image
        return np.float32(NO_PIXEL)
    return np.float32(frame[y, x])


def walk(frame, tree, D, x, y, scale):
    """(node, side) of the leaf slot the pixel reaches, or None when it falls off level D - 1."""
    d = np.float32(frame[y, x])
    scale = np.float32(scale)
    g = 0
    for j in range(D):
        n = (1 << j) - 1 + g
        rec = tree[n]
        with np.errstate(all="ignore"):
            q = [floor_i32(np.float32(np.float32(scale * rec[k]) / d)) for k in range(4)]
            f = probe(frame, wrap_i32(x + q[0]), wrap_i32(y + q[1])) - probe(frame, wrap_i32(x + q[2]), wrap_i32(y + q[3]))
            s = 0 if f < rec[4] else 1                  # NaN goes right
        if is_leaf_slot(rec, s):
            return n, s
        g = 2 * g + s
    return None


def count(depth, labels, forest, scale=1., counts=None, totals=None):
    """Rules R1 and R2.  Adds onto counts uint64 [T, N, 2, C] and totals uint64 [4] (made zero when not given); returns both."""
    T, D, C = dims(forest)
    n_img, h, w = depth.shape
    assert labels.shape == depth.shape and depth.dtype == labels.dtype == np.uint16 and forest.dtype == np.float32
    counts = np.zeros((T, forest.shape[1], 2, C), np.uint64) if counts is None else counts
    totals = np.zeros(4, np.uint64) if totals is None else totals
    one = np.uint64(1)
    for i, y, x in zip(*np.nonzero(labels)):
        l, d = int(labels[i, y, x]), int(depth[i, y, x])
        if l >= C:
            totals[1] += one
        elif d == 0 or d == NO_PIXEL:
            totals[2] += one
        else:
            totals[0] += one
            for t in range(T):
                at = walk(depth[i], forest[t], D, int(x), int(y), scale)
                if at is None:
                    totals[3] += one
                else:
                    counts[t, at[0], at[1], l] += one
    return counts, totals


def reachable_nodes(forest):
    """bool [T, N]: the root, and every child whose parent is reachable and flags "go on" (-1) towards it."""
    T, D, _ = dims(forest)
    reach = np.zeros(forest.shape[:2], bool)
    reach[:, 0] = True
    for t in range(T):
        for n in range((1 << (D - 1)) - 1):             # the nodes that have children
            for s in (0, 1):
                reach[t, 2 * n + 1 + s] = reach[t, n] and not is_leaf_slot(forest[t, n], s)
    return reach


def subtree_sums(forest, counts):
    """uint64 [T, N, C]: per node the class counts of the leaf slots below it, both sides: a leaf slot gives its own counts,
    a "go on" side its child's sums, and at level D - 1 nothing."""
    T, D, C = dims(forest)
    N = forest.shape[1]
    sub = np.zeros((T, N, C), np.uint64)
    for t in range(T):
        for n in range(N - 1, -1, -1):
            for s in (0, 1):
                if is_leaf_slot(forest[t, n], s):
                    sub[t, n] += counts[t, n, s]
                elif 2 * n + 1 + s < N:
                    sub[t, n] += sub[t, 2 * n + 1 + s]
    return sub


def _pdf(cnt):
    """(float)cnt[c] / (float)sum: uint64 -> float32 rounds to nearest even (numpy's conversion does), one float32 divide."""
    return cnt.astype(np.float32) / np.float32(cnt.sum(dtype=np.uint64))


def apply(forest, counts, min_count=1, fallback=KEEP):
    """Rule R3.  Returns (the new forest, report uint64 [4] = own, ancestor, kept, reachable leaf slots)."""
    assert min_count >= 1 and fallback in (KEEP, ANCESTOR)
    T, D, C = dims(forest)
    out = forest.copy()
    reach = reachable_nodes(forest)
    sub = subtree_sums(forest, counts)
    report = np.zeros(4, np.uint64)
    for t in range(T):
        for n in range(forest.shape[1]):
            if not reach[t, n]:
                continue
            for s in (0, 1):
                if not is_leaf_slot(forest[t, n], s):
                    continue
                report[3] += np.uint64(1)
                src, which = None, 2
                if int(counts[t, n, s].sum(dtype=np.uint64)) >= min_count:
                    src, which = counts[t, n, s], 0
                elif fallback == ANCESTOR:
                    a = n
                    while True:
                        if int(sub[t, a].sum(dtype=np.uint64)) >= min_count:
                            src, which = sub[t, a], 1
                            break
                        if a == 0:
                            break
                        a = (a - 1) // 2
                report[which] += np.uint64(1)
                if src is not None:
                    out[t, n, 7 + s * C:7 + (s + 1) * C] = _pdf(src)
    return out, report
