"""Integer restatement of the glove-colour labelling in include/rdf_labels.h, written from the reference's text
(src/cuda/points_ops.cu:39-63, 167-255; src/live_data_convert.py:156-204, 413-458): what the tests hold librdf_labels.so to,
bit for bit.  All sums are Python / int64 integers, so no order of addition enters."""
import numpy as np


def nearest_int(colors, image):
    """(index of the nearest colour, its squared distance) for every pixel of image uint8 [..., 3] against colors uint8
    [K, 3]: colour 0 first, then a strictly smaller distance wins (points_ops.cu:230-241) -- np.argmin keeps the first."""
    px = np.asarray(image, np.int32)[..., None, :]
    d = ((px - np.asarray(colors, np.int32)) ** 2).sum(-1)
    best = np.argmin(d, axis=-1)
    return best, np.take_along_axis(d, best[..., None], -1)[..., 0].astype(np.int64)


def nearest_f32(colors, image):
    """The same in the reference's arithmetic: float32 differences, squares and a running float32 sum over r, g, b."""
    px = np.asarray(image, np.uint8).astype(np.float32)[..., None, :]
    c = np.asarray(colors, np.uint8).astype(np.float32)
    d = np.zeros(px.shape[:-2] + (c.shape[0],), np.float32)
    for j in range(3):
        diff = px[..., j] - c[:, j]
        d = d + diff * diff
    best = np.zeros(d.shape[:-1], np.int64)
    bd = d[..., 0].copy()
    for i in range(1, c.shape[0]):
        less = d[..., i] < bd
        best[less] = i
        bd[less] = d[..., i][less]
    return best, bd


def skipped(image):
    """r + g + b == 0 (points_ops.cu:183, 228)."""
    return np.asarray(image, np.int64).sum(-1) == 0


def split_counts(colors, image):
    """int64 [K, 5]: pixels, sum r, sum g, sum b, sum cost per colour, over the pixels that are not skipped."""
    image = np.asarray(image, np.uint8).reshape(-1, 3)
    K = len(colors)
    keep = ~skipped(image)
    best, cost = nearest_int(colors, image[keep])
    px = image[keep].astype(np.int64)
    out = np.zeros((K, 5), np.int64)
    for k in range(K):
        mine = best == k
        out[k, 0] = int(mine.sum())
        out[k, 1:4] = px[mine].sum(0)
        out[k, 4] = int(cost[mine].sum())
    return out


def counts_as_reference(counts, onto=None):
    """The uint64 [K, 5] words the reference's kernel leaves: four integers and the bits of a double (points_ops.cu:244-249),
    added onto `onto` (same layout) when given."""
    out = np.zeros(counts.shape, np.uint64) if onto is None else np.array(onto, np.uint64)
    out[:, :4] += counts[:, :4].astype(np.uint64)
    out[:, 4] = (out[:, 4].view(np.float64) + counts[:, 4].astype(np.float64)).view(np.uint64)
    return out


def update(counts):
    """(sums / count).astype(uint8) (live_data_convert.py:193) = sum // count; an empty group -> (0, 0, 0)."""
    n = counts[:, 0:1]
    return np.where(n > 0, counts[:, 1:4] // np.maximum(n, 1), 0).astype(np.uint8)


def make_color_mapping(image, init, iterations):
    """init uint8 [tries, K, 3] -> (best colours uint8 [K, 3], best try, cost of every try float64 [tries], final colours of
    every try).  The cost of a try is that of its LAST assignment, against the colours before the last update (:189-197);
    a strictly smaller cost wins (:195)."""
    assert iterations >= 1
    tries = len(init)
    costs = np.zeros(tries, np.float64)
    finals = np.zeros(np.asarray(init).shape, np.uint8)
    best, best_try, best_cost = None, 0, np.inf
    for t in range(tries):
        colors = np.array(init[t], np.uint8)
        for _ in range(iterations):
            counts = split_counts(colors, image)
            cost = float(int(counts[:, 4].sum()))
            colors = update(counts)
        costs[t], finals[t] = cost, colors
        if cost < best_cost:
            best, best_try, best_cost = colors.copy(), t, cost
    return best, best_try, costs, finals


def apply_point_mapping(colors, image):
    """Every non-skipped pixel becomes its nearest colour (points_ops.cu:167-205)."""
    image = np.array(image, np.uint8)
    keep = ~skipped(image)
    best, _ = nearest_int(colors, image[keep])
    image[keep] = np.asarray(colors, np.uint8)[best]
    return image


def label_frame(mapping, image, depth=None, mask_labels=None, mask_label=None):
    """live_data_convert.py:413-458 -> (snapped colour image, labels uint16, labels_rgba, depth with 0 -> 65535 or None)."""
    mapping = np.asarray(mapping, np.uint8)
    image = np.array(image, np.uint8)
    if mask_labels is not None:
        image[np.asarray(mask_labels) != mask_label] = 0
    image = apply_point_mapping(mapping, image)
    labels = np.zeros(image.shape[:2], np.uint16)
    for i in range(len(mapping)):                      # a later i overwrites: the highest matching index stands
        labels[np.all(image == mapping[i], axis=2)] = i + 1
    rgba = np.zeros(image.shape[:2] + (4,), np.uint8)
    rgba[..., :3] = image
    rgba[np.any(image > 0, axis=2), 3] = 255
    if depth is not None:
        depth = np.array(depth, np.uint16)
        depth[depth == 0] = 65535
    return image, labels, rgba, depth


def depths_from_points(depth, pts):
    """w > 0 -> depth = (uint16)z: truncated towards zero, clamped to [0, 65535], NaN -> 0 (points_ops.cu:59-62)."""
    depth = np.array(depth, np.uint16)
    pts = np.asarray(pts, np.float32).reshape(depth.shape + (4,))
    z = np.trunc(pts[..., 2].astype(np.float64))
    z = np.where(np.isnan(z), 0., np.clip(z, 0., 65535.)).astype(np.uint16)
    w = pts[..., 3] > 0
    depth[w] = z[w]
    return depth


def glove_scene(H, W, palette, noise, seed=0, holes=0.0):
    """A synthetic glove frame: blobs painted with the palette's colours plus per-channel noise in [-noise, noise], on black.
    Returns (colour uint8 [H, W, 3], painted class uint16 [H, W]: 0 background, k + 1 for palette[k])."""
    rng = np.random.default_rng(seed)
    palette = np.asarray(palette, np.int64)
    K = len(palette)
    yy, xx = np.mgrid[:H, :W]
    painted = np.zeros((H, W), np.uint16)
    for k in range(K):
        cx, cy = (0.15 + 0.7 * (k + 0.5) / K) * W, (0.35 + 0.3 * ((k * 7) % 5) / 4) * H
        m = ((xx - cx) / (0.42 * W / K)) ** 2 + ((yy - cy) / (0.22 * H)) ** 2 <= 1.
        painted[m & (painted == 0)] = k + 1
    if holes:
        painted[rng.random((H, W)) < holes] = 0
    color = np.zeros((H, W, 3), np.int64)
    on = painted > 0
    color[on] = palette[painted[on] - 1] + rng.integers(-noise, noise + 1, (int(on.sum()), 3))
    return np.clip(color, 0, 255).astype(np.uint8), painted
