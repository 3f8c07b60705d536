"""Plain numpy restatement of reduced-error pruning, rules P1 to P4 of include/rdf_labels.h: `plan` (the errors, the leaf
counts and the collapse decision of every node, bottom-up, and the report) and `apply` (the collapsed subtrees folded into
their parents' sides, top-down).  Written for reading, one node at a time, in Python integers; the kernels of
forest_prune_hip.hip must match it bit for bit in forest bytes, counts, report and collapse decisions.  The walk, the flags,
reachability and the subtree sums are refit_numpy's.  tests/test_prune.py pins this file to a case worked by hand."""
import numpy as np

import refit_numpy as rn


def level(n):
    return int(n + 1).bit_length() - 1


def argmax_e(pdf):
    """The evaluator's argmax: start at 0.0f, strict >, the first index wins, NaN never wins, none above 0
    gives class 0."""
    best, k = np.float32(0.), 0
    for c, v in enumerate(pdf):
        if v > best:
            best, k = v, c
    return k


def slot_error(rec, cnt, s, C):
    """Rule P1: the pixels of the slot that its current PDF labels wrongly."""
    k = argmax_e(rec[7 + s * C:7 + (s + 1) * C])
    return sum(int(v) for v in cnt) - int(cnt[k])


class Plan:
    """What rule P2 computes per node ([T, N] lists of Python integers, bool arrays) and the report of rule P4."""


def reachable_order(forest):
    """[(t, n)] of the reachable nodes only, every parent before its children: for forests of a million nodes of which a few
    thousand are reachable.  The same set as refit_numpy.reachable_nodes."""
    T, D, _ = rn.dims(forest)
    N = forest.shape[1]
    order = [(t, 0) for t in range(T)]
    for t, n in order:                                      # (the list grows while it is read)
        for s in (0, 1):
            if 2 * n + 1 + s < N and not rn.is_leaf_slot(forest[t, n], s):
                order.append((t, 2 * n + 1 + s))
    return order


def plan(forest, counts, cost_per_leaf=0, min_count=0, max_levels=None, sparse=False):
    """Rules P1, P2 and P4.  sparse: visit the reachable nodes only (reachable_order) and sum their subtrees on the way, where
    the plain form visits every node and takes refit_numpy's reachability and subtree sums; what a node that is not reachable
    gets (collapse False, sums 0) is compared with nothing.  The two forms agree on every reachable node."""
    T, D, C = rn.dims(forest)
    N = forest.shape[1]
    max_levels = D if max_levels is None else int(max_levels)
    cost_per_leaf, min_count = int(cost_per_leaf), int(min_count)
    assert 0 <= cost_per_leaf < 2 ** 32 and min_count >= 0 and 1 <= max_levels <= D
    assert counts.shape == (T, N, 2, C) and counts.dtype == np.uint64
    p = Plan()
    p.params = (cost_per_leaf, min_count, max_levels)
    if sparse:
        order = reachable_order(forest)
        p.sub = np.zeros((T, N, C), np.uint64)
        p.reach_before = np.zeros((T, N), bool)
        p.reach_before[tuple(np.array(order).T)] = True
    else:
        order = [(t, n) for t in range(T) for n in range(N)]
        p.sub = rn.subtree_sums(forest, counts)
        p.reach_before = rn.reachable_nodes(forest)
    p.err = [[0] * N for _ in range(T)]
    p.errB = [[0] * N for _ in range(T)]
    p.leaves = [[0] * N for _ in range(T)]
    p.leavesB = [[0] * N for _ in range(T)]
    p.collapse = np.zeros((T, N), bool)
    for t, a in reversed(order):                        # every child before its parent
        for s in (0, 1):
            c = 2 * a + 1 + s
            if rn.is_leaf_slot(forest[t, a], s):
                e = eB = slot_error(forest[t, a], counts[t, a, s], s, C)
                l = lB = 1
                if sparse:
                    p.sub[t, a] += counts[t, a, s]
            elif c < N:
                if sparse:
                    p.sub[t, a] += p.sub[t, c]
                eB, lB = p.errB[t][c], p.leavesB[t][c]
                if p.collapse[t, c]:
                    e, l = _err_leaf(p.sub[t, c]), 1
                else:
                    e, l = p.err[t][c], p.leaves[t][c]
            else:                                       # a "go on" at level D - 1: walks fall off
                e = eB = l = lB = 0
            p.err[t][a] += e
            p.errB[t][a] += eB
            p.leaves[t][a] += l
            p.leavesB[t][a] += lB
        Z = _total(p.sub[t, a])
        p.collapse[t, a] = a != 0 and (level(a) >= max_levels or Z < min_count or
                                       _err_leaf(p.sub[t, a]) <= p.err[t][a] + cost_per_leaf * max(p.leaves[t][a] - 1, 0))
    # the top-down half of the plan: which nodes stay reachable, which "go on" sides become leaf slots
    p.reach_after = np.zeros((T, N), bool)
    p.reach_after[:, 0] = True
    turned = 0
    for t, n in order:                                      # every parent before its children
        for s in (0, 1):
            c = 2 * n + 1 + s
            if c < N and p.reach_after[t, n] and not rn.is_leaf_slot(forest[t, n], s):
                if p.collapse[t, c]:
                    turned += 1
                else:
                    p.reach_after[t, c] = True
    deepest = level(int(np.nonzero(p.reach_after)[1].max()))
    p.report = np.array([sum(p.leavesB[t][0] for t in range(T)), sum(p.leaves[t][0] for t in range(T)), turned, deepest + 1,
                         sum(p.errB[t][0] for t in range(T)), sum(p.err[t][0] for t in range(T)),
                         sum(_total(p.sub[t, 0]) for t in range(T)), int(p.reach_after.sum())], np.uint64)
    return p


def _total(cnt):
    return sum(int(v) for v in cnt)


def _err_leaf(cnt):
    return _total(cnt) - max(int(v) for v in cnt)


def apply(forest, counts, p):
    """Rule P3.  Returns (the new forest, the new counts)."""
    T, D, C = rn.dims(forest)
    N = forest.shape[1]
    out, cnt = forest.copy(), counts.copy()
    out[~p.reach_after] = np.float32(0.)                    # every node that is not reachable any more
    cnt[~p.reach_after] = 0
    for t, n in np.argwhere(p.reach_after).tolist():
        for s in (0, 1):
            c = 2 * n + 1 + s
            if rn.is_leaf_slot(forest[t, n], s) or c >= N or not p.collapse[t, c]:
                continue
            out[t, n, 5 + s] = np.float32(0.)
            a = c
            while _total(p.sub[t, a]) < 1 and a != 0:
                a = (a - 1) // 2
            pdf = rn._pdf(p.sub[t, a]) if _total(p.sub[t, a]) >= 1 else np.zeros(C, np.float32)
            out[t, n, 7 + s * C:7 + (s + 1) * C] = pdf
            cnt[t, n, s] = p.sub[t, c]
    return out, cnt


def prune(forest, counts, cost_per_leaf=0, min_count=0, max_levels=None, sparse=False):
    p = plan(forest, counts, cost_per_leaf, min_count, max_levels, sparse)
    out, cnt = apply(forest, counts, p)
    return out, cnt, p


def truncated(forest, depth):
    """The first 2^depth - 1 records of each tree."""
    return np.ascontiguousarray(forest[:, :(1 << depth) - 1])


def tree_errors(depth, labels, tree, scale=1.):
    """Per tree alone: the walked pixels (rule R1) that the leaf slot they reach labels wrongly by the row-E argmax of its
    PDF, and the walks that fell off.  Returns (errors, fell_off)."""
    D = int(tree.shape[0] + 1).bit_length() - 1
    C = (tree.shape[1] - 7) // 2
    errors = fell = 0
    for i, y, x in zip(*np.nonzero(labels)):
        l, d = int(labels[i, y, x]), int(depth[i, y, x])
        if l >= C or d == 0 or d == rn.NO_PIXEL:
            continue
        at = rn.walk(depth[i], tree, D, int(x), int(y), scale)
        if at is None:
            fell += 1
        elif argmax_e(tree[at[0], 7 + at[1] * C:7 + (at[1] + 1) * C]) != l:
            errors += 1
    return errors, fell
