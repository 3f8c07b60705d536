"""numpy restatement of 3d-beats' decision-tree trainer.  TEST INFRASTRUCTURE ONLY.

Follows /root/reference/src/decision_tree.py:444-600 (DecisionTreeTrainer.train: level-synchronous loop
over proposal blocks, node blocks and image blocks) and /root/reference/src/cuda/tree_train.cu:
  evaluate_random_features :4-64     per (pixel, proposal): count the pixel's label in the child it falls into
  gini helpers             :66-97    fp32 arithmetic on uint64 counts
  pick_best_features       :99-236   best proposal per active node, node record, child counts
  get_active_nodes_next_level :238-273, copy_pixel_groups :275-324
and decision_tree.py:353-371 (random proposals from the global numpy RNG).

Parity unpinned by reference fixtures.  Two places where this restatement has to *define* the semantics:
  * fp32 expressions are evaluated as written, one rounding per operation (nvcc may contract `p += p_i*p_i`
    into an fma, so near-tied gains can rank differently on the reference's own hardware);
  * the reference appends next-level nodes with an atomic counter, i.e. in scheduler order; the order has no
    effect on the trained tree, and here it is ascending.
Stale PDF entries left behind when a later proposal block overwrites a node (tree_train.cu:204-223) are
reproduced: nothing is cleared.

The stages of a level -- count_children, pick_best, next_active, update_pixels -- are functions of arrays, so that a test
can drive one of them with inputs of its own (tests/test_training_stages.py); train_tree calls them in the trainer's order.
"""
import numpy as np

FEATURE_MAGNITUDE_MAX = 14.
FEATURE_THRESHOLD_MAX = 11.
F32 = np.float32


def make_random_features(n):
    """decision_tree.py:353-371, same draws from the global numpy RNG in the same order."""
    out = []
    for _ in range(n):
        offs = []
        for _ in range(2):
            th = np.random.uniform(0, np.pi * 2)
            mag = np.power(np.e, np.random.uniform(0, FEATURE_MAGNITUDE_MAX))
            offs.append(np.array([np.cos(th), np.sin(th)]) * mag)
        thr = np.random.choice([-1, 1]) * np.power(np.e, np.random.uniform(0, FEATURE_THRESHOLD_MAX))
        out.append((offs[0][0], offs[0][1], offs[1][0], offs[1][1], thr))
    return np.array(out, dtype=np.float32)


def _floor_sat_i32(q):
    with np.errstate(invalid="ignore"):
        f = np.floor(q.astype(np.float32)).astype(np.float64)
    f = np.where(np.isnan(f), 0.0, f)
    return np.clip(f, -2147483648.0, 2147483647.0).astype(np.int64)


def _wrap(a):
    return ((a + 2**31) % 2**32) - 2**31


def compute_feature(depth, img, y, x, u, v):
    """decision_tree_common.hpp:8-28 with uv_scale = 1 for pixel arrays (img, y, x) and one feature (u, v)."""
    n, h, w = depth.shape
    d = depth[img, y, x]
    df = d.astype(np.float32)
    with np.errstate(all="ignore"):
        ox = _floor_sat_i32(F32(u[0]) / df); oy = _floor_sat_i32(F32(u[1]) / df)
        px = _floor_sat_i32(F32(v[0]) / df); py = _floor_sat_i32(F32(v[1]) / df)

    def get(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        out = np.full(xx.shape, 65535, dtype=np.uint16)
        out[ok] = depth[img[ok], yy[ok], xx[ok]]
        return out.astype(np.float32)

    f = get(_wrap(y + oy), _wrap(x + ox)) - get(_wrap(y + py), _wrap(x + px))
    return np.where(d == 0, F32(0), f).astype(np.float32)


def _gini_impurity(c):
    s = F32(np.uint64(c.sum()))
    p = F32(0)
    for ci in c:
        with np.errstate(all="ignore"):
            p_i = F32(np.uint64(ci)) / s
            p = F32(p + F32(p_i * p_i))
    return F32(F32(1) - p)


def _gini_gain(pc, lc, rc):
    with np.errstate(all="ignore"):
        p_sum = F32(np.uint64(pc.sum()))
        p_imp = _gini_impurity(pc)
        rem = F32(F32(F32(F32(np.uint64(lc.sum())) / p_sum) * _gini_impurity(lc)) +
                  F32(F32(F32(np.uint64(rc.sum())) / p_sum) * _gini_impurity(rc)))
        return F32(p_imp - rem)


def _cutoff(counts, total, thresh=F32(0.999)):
    for i, c in enumerate(counts):
        with np.errstate(all="ignore"):
            if F32(F32(np.uint64(c)) * F32(1)) / F32(np.uint64(total)) >= thresh:
                return i
    return -1


def _f32_of_counts(a):
    """(float)count for an array of uint64 counts: one correctly rounded conversion each, as the scalar F32(np.uint64(c))."""
    return np.asarray(a, dtype=np.uint64).astype(np.float32)


def _gini_gain_block(pc, lc, rc):
    """_gini_gain for whole arrays: pc [..., C] broadcast against lc, rc [..., C] -> float32 [...].  float32 numpy
    element-wise operations in the order _gini_gain writes them, one rounding per operation."""
    def impurity(c):
        s = _f32_of_counts(c.sum(axis=-1, dtype=np.uint64))
        p = np.zeros(s.shape, np.float32)
        for k in range(c.shape[-1]):
            p_i = _f32_of_counts(c[..., k]) / s
            p = p + p_i * p_i
        return F32(1) - p

    with np.errstate(all="ignore"):
        p_sum = _f32_of_counts(pc.sum(axis=-1, dtype=np.uint64))
        p_imp = impurity(pc)
        rem = ((_f32_of_counts(lc.sum(axis=-1, dtype=np.uint64)) / p_sum) * impurity(lc) +
               (_f32_of_counts(rc.sum(axis=-1, dtype=np.uint64)) / p_sum) * impurity(rc))
        g = p_imp - rem
    assert g.dtype == np.float32
    return g


def block_gains(pc, lc, rc, vectorised=True):
    """Gain of every proposal of one node block: pc uint64 [n, C], lc and rc uint64 [n, P, C] -> float32 [n, P], 0 where a
    side is empty (tree_train.cu:150-160).  vectorised=False walks the scalar _gini_gain; the two agree bit for bit."""
    ls, rs = lc.sum(axis=-1, dtype=np.uint64), rc.sum(axis=-1, dtype=np.uint64)
    assert (ls + rs == pc.sum(axis=-1, dtype=np.uint64)[:, None]).all()
    if vectorised:
        g = _gini_gain_block(pc[:, None, :], lc, rc)
    else:
        g = np.zeros(ls.shape, np.float32)
        for i in range(lc.shape[0]):
            for j in range(lc.shape[1]):
                if ls[i, j] and rs[i, j]:
                    g[i, j] = _gini_gain(pc[i], lc[i, j], rc[i, j])
    return np.where((ls == 0) | (rs == 0), F32(0), g).astype(np.float32)


def first_best(g):
    """The scan of tree_train.cu:146-163: strict > from (-1, proposal 0), i.e. the first proposal of the largest gain."""
    best_g, best_j = F32(-1), 0
    for j, gj in enumerate(g):
        if gj > best_g:
            best_g, best_j = gj, j
    return best_g, best_j


def count_children(depth, labels_or_pixel_lists, node, props, start, end, NB, C):
    """evaluate_random_features: counts[j][child - start][label] over the pixels whose node is live (>= 0), whose label is
    below C and whose two children lie in [start, end).  Either `labels` [n, h, w] with `node` [n, h, w], or the pixel
    lists (img, y, x, label) with `node` per listed pixel.  Returns uint64 [P, NB, C]."""
    depth = np.ascontiguousarray(depth, dtype=np.uint16)
    node = np.asarray(node).astype(np.int64)
    if isinstance(labels_or_pixel_lists, tuple):
        img, yy, xx, lab = (np.asarray(a).astype(np.int64) for a in labels_or_pixel_lists)
    else:
        labels = np.asarray(labels_or_pixel_lists)
        assert labels.shape == depth.shape == node.shape
        img, yy, xx = np.nonzero(node >= 0)
        lab = labels[img, yy, xx].astype(np.int64)
        node = node[img, yy, xx]
    P = props.shape[0]
    elig = (node >= 0) & (node * 2 >= start) & (node * 2 + 1 < end) & (lab < C)
    counts = np.zeros((P, NB, C), dtype=np.uint64)
    ii, ey, ex, en, el = img[elig], yy[elig], xx[elig], node[elig], lab[elig]
    for j in range(P):
        f = compute_feature(depth, ii, ey, ex, props[j, 0:2], props[j, 2:4])
        with np.errstate(invalid="ignore"):
            child = np.where(f < props[j, 4], en * 2, en * 2 + 1) - start
        np.add.at(counts[j], (child, el), 1)
    return counts


def pick_best(active, node_counts, counts, props, tree, next_counts, best_gain, level, D, start, end, vectorised=True):
    """pick_best_features for one proposal block and one node block; updates tree [nodes, 7 + 2C], next_counts [nodes, C]
    and best_gain [n_active] in place, as the kernel does.  Nothing is cleared: entries that this block does not write
    keep what they held."""
    C = node_counts.shape[1]
    level_base = (1 << level) - 1
    active = np.asarray(active).astype(np.int64)
    inside = np.nonzero((active * 2 >= start) & (active * 2 + 1 < end))[0]
    if inside.size == 0 or props.shape[0] == 0:
        return
    par = active[inside]
    lc_all = counts[:, par * 2 - start, :].transpose(1, 0, 2)         # [n, P, C]
    rc_all = counts[:, par * 2 + 1 - start, :].transpose(1, 0, 2)
    gains = block_gains(node_counts[par], lc_all, rc_all, vectorised)
    for n, i in enumerate(inside):
        parent = int(par[n])
        l_child, r_child = parent * 2, parent * 2 + 1
        pc = node_counts[parent]
        p_sum = int(pc.sum())
        best_g, best_j = first_best(gains[n])
        if not best_g > best_gain[i]:
            continue
        best_gain[i] = best_g
        lc, rc = lc_all[n, best_j], rc_all[n, best_j]
        ls, rs = int(lc.sum()), int(rc.sum())
        rec = tree[level_base + parent]
        rec[0:5] = props[best_j]
        if best_g <= 0:
            rec[5] = rec[6] = 0.0
            for k in range(C):
                with np.errstate(all="ignore"):
                    p = F32(F32(np.uint64(pc[k])) * F32(1)) / F32(np.uint64(p_sum))
                rec[7 + k] = rec[7 + C + k] = p
            continue
        for side, cc, cs, child in ((0, lc, ls, l_child), (1, rc, rs, r_child)):
            cut = _cutoff(cc, cs)
            if cut > -1:
                rec[5 + side] = 0.0
                rec[7 + side * C + cut] = 1.0
            elif level == D - 1:
                rec[5 + side] = 0.0
                for k in range(C):
                    with np.errstate(all="ignore"):
                        rec[7 + side * C + k] = F32(F32(np.uint64(cc[k])) * F32(1)) / F32(np.uint64(cs))
            else:
                rec[5 + side] = -1.0
                next_counts[child] = cc


def next_active(tree, active, level, C):
    """get_active_nodes_next_level, in ascending order of the parents: the children whose flag is -1."""
    tree = np.asarray(tree).reshape(-1, 7 + 2 * C)
    level_base = (1 << level) - 1
    nxt = []
    for parent in active:
        rec = tree[level_base + int(parent)]
        if rec[5] == -1.0:
            nxt.append(int(parent) * 2)
        if rec[6] == -1.0:
            nxt.append(int(parent) * 2 + 1)
    return np.array(nxt, dtype=np.int64)


def update_pixels(depth, node, tree, level, C):
    """copy_pixel_groups: the next level's node of every pixel, `node` [n, h, w] with -1 = not live.  A pixel goes left
    when its feature is below the threshold (never with a NaN threshold) and is retired unless that side's flag is -1."""
    depth = np.ascontiguousarray(depth, dtype=np.uint16)
    tree = np.asarray(tree).reshape(-1, 7 + 2 * C)
    level_base = (1 << level) - 1
    node = np.asarray(node).astype(np.int64)
    out = node.copy()
    img, yy, xx = np.nonzero(node >= 0)
    cur = node[img, yy, xx]
    for parent in np.unique(cur):
        sel = cur == parent
        rec = tree[level_base + parent]
        f = compute_feature(depth, img[sel], yy[sel], xx[sel], rec[0:2], rec[2:4])
        with np.errstate(invalid="ignore"):
            left = f < rec[4]
        status = np.where(left, _floor_sat_i32(np.array([rec[5]]))[0], _floor_sat_i32(np.array([rec[6]]))[0])
        out[img[sel], yy[sel], xx[sel]] = np.where(status != -1, -1, parent * 2 + np.where(left, 0, 1))
    return out


def train_tree(depth, labels, num_classes, max_depth, proposal_blocks_per_level, proposals_per_block,
               max_next_nodes_per_block=1 << 17, proposal_fn=make_random_features):
    """Returns the trained tree, float32 [2^D - 1, 7 + 2C] (level-order, tree_train.cu record layout)."""
    depth = np.ascontiguousarray(depth, dtype=np.uint16)
    labels = np.ascontiguousarray(labels, dtype=np.uint16)
    C, D = num_classes, max_depth
    E = 7 + 2 * C
    tree = np.zeros(((1 << D) - 1, E), dtype=np.float32)
    node = np.where(labels > 0, 0, -1).astype(np.int64)  # nodes_by_pixel; -1 = unlabelled or retired
    max_leaf = 1 << D
    node_counts = np.zeros((max_leaf, C), dtype=np.uint64)
    np.add.at(node_counts[0], labels[labels > 0].astype(np.int64), 1)
    next_counts = node_counts.copy()                     # cu_array.to_gpu(self.node_counts) twice (:399-400)
    active = np.array([0], dtype=np.int64)
    for level in range(D):
        if active.size == 0:
            break
        best_gain = np.full(active.size, -1.0, dtype=np.float32)
        for _ in range(proposal_blocks_per_level):
            props = proposal_fn(proposals_per_block)
            max_next = 1 << (level + 1)
            if max_next > max_next_nodes_per_block:
                blocks = [(i * max_next_nodes_per_block, (i + 1) * max_next_nodes_per_block)
                          for i in range(max_next // max_next_nodes_per_block)]
            else:
                blocks = [(0, max_next)]
            NB = min(max_next, max_next_nodes_per_block)
            for start, end in blocks:
                counts = count_children(depth, labels, node, props, start, end, NB, C)
                pick_best(active, node_counts, counts, props, tree, next_counts, best_gain, level, D, start, end)
        nxt = next_active(tree, active, level, C)
        if level == D - 1:
            break
        node_counts = next_counts.copy()
        node = update_pixels(depth, node, tree, level, C)
        active = nxt
    return tree
