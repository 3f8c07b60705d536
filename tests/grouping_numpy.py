"""CPU restatement of the hand-group chain (rdf_hand_groups; the reference's shrink_image -> CppGrouping().make_groups ->
write_pixel_groups_to_stencil_image -> grow_groups), written from the contract in include/rdf_hip.h: components from
scipy.ndimage.label with the 4-connected structure, statistics in numpy with the fp32 arithmetic the contract names."""
import numpy as np
from scipy import ndimage

_FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def shrink(depth, level):
    f = 1 << level
    hm, wm = depth.shape[0] // f, depth.shape[1] // f
    return np.ascontiguousarray(depth[:hm * f:f, :wm * f:f])


def components(mm):
    """int32 [Hm, Wm]: each foreground pixel's component as its minimum raster index, -1 for background."""
    lab, n = ndimage.label(mm != 0, structure=_FOUR)
    out = np.full(mm.shape, -1, np.int32)
    if n:
        flat = lab.reshape(-1)
        idx = np.arange(flat.size)
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat, idx)
        out.reshape(-1)[flat > 0] = first[flat[flat > 0]]
    return out


def make_groups(mm, pct_thresh):
    """(g_info float32 [2, 3], stencil uint16 [Hm, Wm], comps int32 [Hm, Wm]) of one shrunk frame."""
    hm, wm = mm.shape
    comps = components(mm)
    g_info = np.zeros((2, 3), np.float32)
    stencil = np.zeros(mm.shape, np.uint16)
    flat = comps.reshape(-1)
    fg = flat >= 0
    idx = np.nonzero(fg)[0]
    r = flat[fg]
    size = np.bincount(r, minlength=flat.size)
    sum_x = np.bincount(r, weights=None if idx.size == 0 else (idx % wm), minlength=flat.size).astype(np.int64)
    sum_y = np.bincount(r, weights=None if idx.size == 0 else (idx // wm), minlength=flat.size).astype(np.int64)
    best = [None, None]
    p = np.float32(hm * wm)
    pct = np.float32(pct_thresh)
    for root in np.nonzero(size)[0]:   # ascending root = the order the reference's raster scan meets the components
        n = int(size[root])
        if np.float32(n) / p <= pct:
            continue
        cx = np.float32(int(sum_x[root])) / np.float32(n)
        cy = np.float32(int(sum_y[root])) / np.float32(n)
        side = 0 if cx < np.float32(wm) / np.float32(2) else 1
        if best[side] is None or n > best[side][0]:
            best[side] = (n, cx, cy, root)
    for side in (0, 1):
        if best[side] is not None:
            size, cx, cy, root = best[side]
            g_info[side] = (np.float32(size), cx, cy)
            stencil[comps == root] = side + 1
    return g_info, stencil, comps


def grow(stencil):
    """grow_groups: own value if nonzero, else the first nonzero of left, right, up, down (outside = 0)."""
    s = stencil
    pad = np.zeros((s.shape[0] + 2, s.shape[1] + 2), s.dtype)
    pad[1:-1, 1:-1] = s
    out = s.copy()
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        nb = pad[1 + dy:pad.shape[0] - 1 + dy, 1 + dx:pad.shape[1] - 1 + dx]
        take = (out == 0) & (nb != 0)
        out[take] = nb[take]
    return out


def write_stencil(coords, num_coords, dims):
    st = np.zeros(dims, np.uint16)
    c = coords[:num_coords]
    st[c[:, 0], c[:, 1]] = c[:, 2]
    return st


def coords_of(stencil):
    """(y, x, group) rows: group 1 then group 2, each in raster order."""
    rows = []
    for g in (1, 2):
        ys, xs = np.nonzero(stencil == g)
        rows.append(np.stack([ys, xs, np.full(ys.shape, g)], 1))
    return np.concatenate(rows).astype(np.int32)


def hand_groups(depth, level, pct_thresh):
    """The whole chain for one frame: (groups uint16 [Hm, Wm], g_info float32 [2, 3], comps int32, coords int32 [k, 3])."""
    mm = shrink(depth, level)
    g_info, stencil, comps = make_groups(mm, pct_thresh)
    return grow(stencil), g_info, comps, coords_of(stencil)
