"""The cases of tests/test_posterior.py, built from seeds: the case worked by hand, the parity cases (the smallest shapes at
which the posterior kernel can go wrong: widths on both sides of a wave, one to five rows, every class-capacity bound, a
depth-12 forest whose leaves begin at level 9), a hand-made forest of awkward PDFs, the two-layer stack of the layered tests with
the thresholds at which its gates reject, and the maps of the confidence counts' striding launches."""
import importlib

import numpy as np

NO_PIXEL = 65535


def _synth():
    return importlib.import_module("3d-beats_amd.synth")


# ------------------------------------------------------------ the case worked by hand ------------------------------------------
def hand_case():
    """T = 2, D = 2, C = 3 on one 4 x 4 frame; every sum, label and confidence is written out in the test.
        tree 0  root: probes (x + 1, y) and (x, y) at depth 1000 (offsets 1000 and 0), thresh 50: du - dv < 50 goes left, on to
                node 1 (flag -1); the right side is a leaf slot, one-hot for class 1.
                node 1: probes (x, y + 1) and (x, y), thresh 50: left is a leaf slot [.5, .5, 0]; right says "go on" at the last
                level: the walk falls off and adds nothing.
        tree 1  root: probes (x - 1, y) and (x, y), thresh 50: left is an all-zero leaf, right the leaf [.25, .25, .5]."""
    C = 3
    depth = np.array([[[1000, 1000, 1100, 1000],
                       [1000, 1000, 1000, 1000],
                       [1000, 1200,    0, 65535],
                       [1000, 1000, 1000, 1000]]], np.uint16)
    forest = np.zeros((2, 3, 7 + 2 * C), np.float32)
    forest[0, 0, :7] = [1000., 0., 0., 0., 50., -1., 0.]
    forest[0, 0, 7:] = [0., 0., 0., 0., 1., 0.]
    forest[0, 1, :7] = [0., 1000., 0., 0., 50., 0., -1.]
    forest[0, 1, 7:] = [.5, .5, 0., 0., 0., 0.]
    forest[1, 0, :7] = [-1000., 0., 0., 0., 50., 0., 0.]
    forest[1, 0, 7:] = [0., 0., 0., .25, .25, .5]
    return depth, forest


# ------------------------------------------------------------ frames and forests ------------------------------------------------
def live_rows(idx, n, h, w):
    """n frames of h x w cut out of synth.live_frame(idx + i, 48, w) (background 65535, an ellipse of surface, holes of 0): the
    h consecutive rows with the most pixels to evaluate, so that a frame of one to five rows is not all background."""
    out = np.empty((n, h, w), np.uint16)
    for i in range(n):
        big = _synth().live_frame(idx + i, 48, w)
        valid = ((big != 0) & (big != NO_PIXEL)).sum(axis=1)
        y0 = int(np.argmax([valid[y:y + h].sum() for y in range(48 - h + 1)]))
        out[i] = big[y0:y0 + h]
    return out


def single_pixel(n, h, w, at):
    """All background but one pixel with a depth."""
    out = np.full((n, h, w), NO_PIXEL, np.uint16)
    out[(0,) + at] = 900
    return out


def trained_like(T, D, C, first):
    """synth.trained_like_tree with leaves from level 1 on, and offsets of about five pixels along the row at the frames' depths (about 4000) so
    that probes land inside the frame, on the background, on holes and outside."""
    s = _synth()
    forest = np.stack([s.trained_like_tree(first + k, D, C, 0.3, min(1, D - 1)) for k in range(T)])
    forest[:, :, 0:4:2] *= 20.
    forest[:, :, 1:4:2] /= 50.                           # (the frames are a few rows high: rows y and y - 1)
    forest[:, :, 4] /= 20.
    return forest


def deep_forest(T, D, C, first):
    """trained_like's offsets and thresholds on trees whose leaves begin at level 9: every walk goes nine levels down at least,
    through the levels at which the node index (1 << j) - 1 + g and the record offset n * E grow."""
    s = _synth()
    forest = np.stack([s.trained_like_tree(first + k, D, C, 0.3, min(9, D - 1)) for k in range(T)])
    forest[:, :, 0:4:2] *= 20.
    forest[:, :, 1:4:2] /= 50.
    forest[:, :, 4] /= 20.
    return forest


def walk_ends(depth, forest, labels_reduce=1, scale=1.):
    """[(image, y, x, tree, node, side)] of every walk of the evaluated label pixels (no filter); node and side are None for
    a walk that falls off level D - 1."""
    import refit_numpy as rn
    T, D, _ = rn.dims(forest)
    r = int(labels_reduce)
    out = []
    for i in range(depth.shape[0]):
        for y in range(0, (depth.shape[1] // r) * r, r):
            for x in range(0, (depth.shape[2] // r) * r, r):
                if depth[i, y, x] in (0, NO_PIXEL):
                    continue
                for t in range(T):
                    at = rn.walk(depth[i], forest[t], D, x, y, scale)
                    out.append((i, y, x, t) + (at if at is not None else (None, None)))
    return out


def level_of(node):
    return int(node + 1).bit_length() - 1


def plant_fall_off(depth, forest, labels_reduce=1, scale=1.):
    """The first walk (in walk_ends' order) that ends in a leaf slot of level D - 1 is told to go on there: it falls off the
    tree at depth.  Changes `forest` in place; returns (image, y, x, tree, node, side) of the plant."""
    D = level_of(forest.shape[1])
    for i, y, x, t, n, s in walk_ends(depth, forest, labels_reduce, scale):
        if n is not None and level_of(n) == D - 1:
            forest[t, n, 5 + s] = -1.
            return i, y, x, t, n, s
    raise AssertionError("no walk ends on the last level")


def sharp_forest(T, D, C, first, hot_share=0.4):
    """trained_like with the leaf PDFs a well-trained tree has: cubed and normalised again, and four leaf slots in ten one-hot
    (the trainer's rule above 0.999 purity), so that confidences reach from below a half up to 65535."""
    forest = trained_like(T, D, C, first)
    rng = np.random.default_rng(first)
    pdf = forest[:, :, 7:].reshape(T, -1, 2, C)
    cubed = pdf * pdf * pdf
    total = cubed.sum(axis=3, keepdims=True, dtype=np.float32)
    cubed = np.where(total > 0, cubed / np.where(total > 0, total, np.float32(1)), np.float32(0)).astype(np.float32)
    one_hot = (np.arange(C) == pdf.argmax(axis=3)[..., None]).astype(np.float32)
    hot = (rng.random(pdf.shape[:3]) < hot_share)[..., None] & (total > 0)
    forest[:, :, 7:] = np.where(hot, one_hot, cubed).reshape(T, -1, 2 * C)
    return forest


def awkward_forest():
    """T = 2, D = 2, C = 3 with PDFs no trainer writes: negative entries (a share above 1: the confidence clamps), NaN, +inf,
    an all-zero leaf, and a "go on" flag on the last level.  Probes one pixel to the right, below and to the left at depths
    around 4000."""
    C = 3
    forest = np.zeros((2, 3, 7 + 2 * C), np.float32)
    forest[0, 0, :7] = [6000., 0., 0., 0., 0., -1., 0.]
    forest[0, 0, 7:] = [0., 0., 0., -1., 0., 2.]
    forest[0, 1, :7] = [0., 6000., 0., 0., 0., 0., -1.]
    forest[0, 1, 7:] = [np.inf, 0., 0., 7., 7., 7.]          # (the right side says "go on": its PDF is never read)
    forest[1, 0, :7] = [-6000., 0., 0., 0., 0., 0., 0.]
    forest[1, 0, 7:] = [0., 0., 0., .25, np.nan, .5]
    return forest


def filter_image(seed, shape, filter_class):
    rng = np.random.default_rng(seed)
    f = rng.choice(np.array([0, filter_class, filter_class, filter_class, NO_PIXEL], np.uint16), size=shape)
    return f.astype(np.uint16)


# id: n, H, W, r, scale, T, D, C, filter class or None, pre-fill, forest kind, frame kind
PARITY = {
    "w1":        (1, 1, 1, 1, 1.0, 1, 1, 1, None, NO_PIXEL, "trained", "single"),
    "w63":       (1, 2, 63, 1, 0.5, 2, 2, 2, None, 0, "trained", "live"),
    "w64_n3":    (3, 3, 64, 1, 1.0, 5, 6, 4, 2, NO_PIXEL, "trained", "live"),
    "w65":       (1, 4, 65, 1, 1.0, 1, 6, 5, None, 0, "trained", "live"),
    "w130_r2":   (3, 5, 130, 2, 0.5, 2, 6, 8, 2, 0, "sharp", "live"),
    "w130_c9":   (1, 5, 130, 1, 1.0, 5, 2, 9, None, NO_PIXEL, "trained", "live"),
    "w131_r3":   (1, 7, 131, 3, 1.0, 2, 6, 16, 3, NO_PIXEL, "trained", "live"),
    "awkward":   (1, 3, 65, 1, 1.0, 2, 2, 3, None, NO_PIXEL, "awkward", "live"),
    "single_r2": (1, 4, 130, 2, 1.0, 1, 1, 16, None, 0, "trained", "single"),
    "row_d1":    (3, 1, 64, 1, 0.5, 5, 1, 8, None, NO_PIXEL, "trained", "live"),
    "sharp":     (1, 5, 65, 1, 1.0, 2, 6, 5, None, NO_PIXEL, "sharp", "live"),
    # (sorted last: the seeds of the cases above are their places in the sorted list)
    "walk_d12":  (1, 5, 130, 1, 1.0, 2, 12, 5, None, NO_PIXEL, "deep", "live500"),
}


def parity_case(name):
    """(depth, forest, kwargs of posterior_numpy.posterior / get_posteriors_forest, pre-fill)."""
    n, h, w, r, scale, T, D, C, fclass, prefill, fkind, dkind = PARITY[name]
    seed = sorted(PARITY).index(name)
    depth = live_rows(500, n, h, w) if dkind == "live500" else live_rows(100 + 10 * seed, n, h, w) if dkind == "live" else single_pixel(n, h, w, (h - 1 - (h - 1) % r, (w - 1) - (w - 1) % r))
    forest = {"awkward": awkward_forest, "sharp": lambda: sharp_forest(T, D, C, 30 + 5 * seed),
              "trained": lambda: trained_like(T, D, C, 30 + 5 * seed), "deep": lambda: deep_forest(T, D, C, 30 + 5 * seed)}[fkind]()
    assert forest.shape == (T, (1 << D) - 1, 7 + 2 * C)
    if fkind == "deep":
        plant_fall_off(depth, forest, r, scale)
    filt = None if fclass is None else filter_image(seed, (n, h // r, w // r), fclass)
    return depth, forest, dict(labels_reduce=r, scale=scale, filter_images=filt, filter_class=fclass), prefill


# ------------------------------------------------------------ the layered stack -------------------------------------------------
LAYERED = dict(H=24, W=66, R=2)


def layered_case():
    """A two-layer filtered stack of HandModel.layered_config's shape (a C = 4 forest, then a C = 5 forest filtered on class 3 of
    the first) on frames of 66 x 24 at labels_reduce 2.  Returns (f0, f1, conditions, colors, frames uint16 [2, 24, 66])."""
    f0, f1 = sharp_forest(3, 5, 4, 60, 0.8), sharp_forest(3, 6, 5, 70, 0.8)
    # classes 0 and 3 change places: most pixels of these frames then get class 3 from the first layer, the one the second takes
    f0[:, :, 7:] = f0[:, :, 7:].reshape(3, -1, 2, 4)[..., [3, 1, 2, 0]].reshape(3, -1, 8)
    conditions = [[0, 1], [0, 2], [1, 3], [0, 3], [0, 4], [0, 5], [0, 6], [0, 7]]
    colors = [[10 * i, 255 - 10 * i, i, 255] for i in range(1, 8)]
    frames = np.stack([_synth().live_frame(300 + i, 48, LAYERED["W"])[12:12 + LAYERED["H"]] for i in range(2)])
    return f0, f1, conditions, colors, frames


# thresholds at which both gates of layered_case() reject and layer 0's gate changes what layer 1 evaluates (the conditions are
# asserted by test_posterior.test_the_gated_stack_case_meets_its_conditions)
LAYERED_GATE = (50000, 30000)
LAYERED_FILTER_CLASS = 3


def stack_answer(pn, oracle, case, frame, thresholds=None, scale=0.75, prefill_colors=0):
    """What a LayeredDecisionForest over layered_case()'s forests leaves for one frame, from the restatement `pn` gated per
    layer (thresholds None: no gate) and the oracle's composite: a dict of `labels` and `conf` (one [Hl, Wl] map a layer,
    confidence 0 where nothing was evaluated), `evaluated` (bool, a layer), `composite`, `hand` (the composite mirrored in x) and
    `colors` / `hand_colors` (RGBA of the composite / the mirrored one over `prefill_colors` bytes)."""
    f0, f1, conditions, colors, _ = case
    R = LAYERED["R"]
    t0, t1 = (0, 0) if thresholds is None else thresholds
    d3 = np.ascontiguousarray(frame)[None]
    l0, c0, _ = pn.posterior(d3, f0, R, scale, min_conf=t0)
    l1, c1, _ = pn.posterior(d3, f1, R, scale, filter_images=l0, filter_class=LAYERED_FILTER_CLASS, min_conf=t1)
    ev0, ev1 = pn.evaluated_mask(d3, R), pn.evaluated_mask(d3, R, l0, LAYERED_FILTER_CLASS)
    comp = np.full(l0.shape[1:], NO_PIXEL, np.uint16)
    assert oracle.composite([l0[0], l1[0]], conditions, comp) == 0
    hand = np.ascontiguousarray(comp[:, ::-1])

    def rgba(labels):
        out = np.full(labels.shape + (4,), prefill_colors, np.uint8)
        known = (labels >= 1) & (labels <= len(colors))
        out[known] = np.array(colors, np.uint8)[labels[known].astype(np.int64) - 1]
        return out
    return dict(labels=[l0[0], l1[0]], conf=[np.where(ev0[0], c0[0], 0).astype(np.uint16), np.where(ev1[0], c1[0], 0).astype(np.uint16)],
                evaluated=[ev0[0], ev1[0]], composite=comp, hand=hand, colors=rgba(comp), hand_colors=rgba(hand))


# ------------------------------------------------------------ the confidence counts' striding launches --------------------------
COUNTS_GRID_PIXELS = 512 * 256      # kCountBlocks workgroups of kThreads lanes: what one trip of k_confidence_counts covers
COUNTS_STRIDE = {
    "one_image":  dict(truth_shape=(1, 257, 511), r=1),        # 131327 label pixels: workgroup 0 alone makes a second trip
    "two_images": dict(truth_shape=(2, 258, 1022), r=2),       # [2, 129, 511] maps, 131838: a wave of the second trip spans the images
}


def counts_stride_maps(name, C=8):
    """(pred, conf, truth, r) with more label pixels than one trip of the counts kernel covers: pred 20 % 65535, truth 70 % zero (and
    never zero at the planted pixels), confidence 0 and 65535 planted at the first pixel, the last pixel and pixel 131072, and
    the two aligned waves from label pixel 131072 + 64 on without any truth."""
    n, h, w = COUNTS_STRIDE[name]["truth_shape"]
    r = COUNTS_STRIDE[name]["r"]
    hl, wl = h // r, w // r
    n_lpx = n * hl * wl
    rng = np.random.default_rng(n_lpx)
    pred = rng.integers(0, C, n_lpx).astype(np.uint16)
    pred[rng.random(n_lpx) < 0.2] = NO_PIXEL
    conf = rng.integers(0, 65536, n_lpx).astype(np.uint16)
    at = rng.integers(1, C, n_lpx).astype(np.uint16)              # the truth under each label pixel
    at[rng.random(n_lpx) < 0.7] = 0
    right = (rng.random(n_lpx) < 0.5) & (at > 0) & (pred != NO_PIXEL)
    pred[right] = at[right]
    planted = np.array([0, 1, COUNTS_GRID_PIXELS - 1, COUNTS_GRID_PIXELS, COUNTS_GRID_PIXELS + 1, n_lpx - 2, n_lpx - 1])
    conf[planted] = [0, 65535, 65535, 65535, 0, 0, 65535]
    at[planted] = [1, 2, 3, 1, 2, 3, 1]
    pred[planted] = [1, 2, 1, 1, 3, 3, 2]
    at[COUNTS_GRID_PIXELS + 64:COUNTS_GRID_PIXELS + 192] = 0
    truth = rng.integers(1, C, (n, h, w)).astype(np.uint16)       # off the sampled coordinates: never zero, never to be read
    truth[:, :hl * r:r, :wl * r:r] = at.reshape(n, hl, wl)
    return pred.reshape(n, hl, wl), conf.reshape(n, hl, wl), truth, r
