"""Plain restatement of the joint votes, rules V1 to V5 of include/rdf_labels.h: `count` (offsets towards the joints summed per
leaf slot), `fit` (sums to votes), `cast` (votes into accumulators) and `modes` (accumulators to joints).  Written for reading,
one pixel and one slot at a time with Python ints; the kernels of forest_votes_hip.hip must match it bit for bit.  The forest's
shape, the walk, the leaf-slot test and reachability are refit_numpy's.  tests/test_joint_votes.py pins it to a case worked by
hand and pins every rounding rule on literals."""
import numpy as np

from refit_numpy import dims, is_leaf_slot, reachable_nodes, walk

NO_PIXEL = 65535
MAX_JOINTS, MAX_RADIUS = 16, 255
M64 = (1 << 64) - 1


def signed64(v):
    """A uint64 word read as two's complement."""
    v = int(v)
    return v - (1 << 64) if v >> 63 else v


def absent(tz):
    return tz <= 0 or tz >= 65535


def offset(delta, d):
    """V1: floordiv(delta * d, 64).  Python's // is the floor division."""
    return (int(delta) * int(d)) // 64


def count(depth, labels, targets, forest, scale=1., radius=MAX_RADIUS, sums=None, totals=None, walk=walk):
    """Rule V1.  Adds onto sums uint64 [T, N, 2, J, 5] and totals uint64 [4] (made zero when not given); returns both.  `walk`:
    refit_numpy's, or the same behind a cache (votes_cases.memo_walk)."""
    T, D, _ = dims(forest)
    n_img, h, w = depth.shape
    J = targets.shape[1]
    assert labels.shape == depth.shape and depth.dtype == labels.dtype == np.uint16 and forest.dtype == np.float32
    assert targets.shape == (n_img, J, 3) and targets.dtype == np.int32 and 1 <= J <= MAX_JOINTS and 0 <= radius <= MAX_RADIUS
    sums = np.zeros((T, forest.shape[1], 2, J, 5), np.uint64) if sums is None else sums
    totals = np.zeros(4, np.uint64) if totals is None else totals
    tot = [int(v) for v in totals]
    for i, y, x in zip(*np.nonzero(labels)):
        i, y, x = int(i), int(y), int(x)
        d = int(depth[i, y, x])
        if d == 0 or d == NO_PIXEL:
            tot[1] += 1
            continue
        tot[0] += 1
        for t in range(T):
            at = walk(depth[i], forest[t], D, x, y, scale)
            if at is None:
                tot[2] += 1
                continue
            for j in range(J):
                tx, ty, tz = (int(v) for v in targets[i, j])
                if absent(tz):
                    continue
                dx, dy = tx - x, ty - y
                if abs(dx) > radius or abs(dy) > radius:
                    continue
                ox, oy, oz = offset(dx, d), offset(dy, d), tz - d
                word = sums[t, at[0], at[1], j]
                for k, v in enumerate((1, ox, oy, oz, ox * ox + oy * oy)):
                    word[k] = np.uint64((int(word[k]) + v) & M64)              # the signed sums wrap as two's complement
                tot[3] += 1
    totals[:] = [np.uint64(v) for v in tot]
    return sums, totals


def weight(var, max_var):
    """V2: 256 - floordiv(var * 256, max_var + 1) for 0 <= var <= max_var: 256 at var 0, 1 at var == max_var."""
    return 256 - (var * 256) // (max_var + 1)


def fit_entry(word, min_count, max_var):
    """V2 for one (slot, joint): ((mx, my, mz, w), which) with which 1 a vote, 2 dropped for support, 3 dropped for spread."""
    n = int(word[0])
    if n < min_count or n >= 1 << 26:
        return (0, 0, 0, 0), 2
    mx, my, mz = (signed64(word[k]) // n for k in (1, 2, 3))
    assert all(-(1 << 31) <= m < 1 << 31 for m in (mx, my, mz)), "sums that rule V1 cannot have made"
    var = max(0, int(word[4]) // n - (mx * mx + my * my))
    if var > max_var:
        return (0, 0, 0, 0), 3
    return (mx, my, mz, weight(var, max_var)), 1


def fit(forest, sums, min_count, max_var):
    """Rule V2.  Returns (votes int32 [T, N, 2, J, 4], report uint64 [4])."""
    assert min_count >= 1 and 0 <= max_var <= 1 << 38
    T, N = forest.shape[:2]
    J = sums.shape[3]
    votes = np.zeros((T, N, 2, J, 4), np.int32)
    report = [0, 0, 0, 0]
    reach = reachable_nodes(forest)
    for t in range(T):
        for n in range(N):
            for s in (0, 1):
                if not (reach[t, n] and is_leaf_slot(forest[t, n], s)):
                    continue
                report[0] += 1
                for j in range(J):
                    votes[t, n, s, j], which = fit_entry(sums[t, n, s, j], min_count, max_var)
                    report[which] += 1
    return votes, np.array(report, np.uint64)


def vote_pixels(m, d):
    """V4: floordiv(128 * m + d, 2 * d), the inverse of V1's normalisation rounded half up."""
    return (128 * int(m) + int(d)) // (2 * int(d))


def grid(dim, shift):
    return ((dim - 1) >> shift) + 1 if dim > 0 else 0


def cast(depth, forest, votes, scale=1., gate=None, r=1, shift=2, walk=walk):
    """Rules V3 and V4.  Returns (acc uint32 [n_img, J, Ha, Wa], zacc uint64 alike)."""
    T, D, _ = dims(forest)
    n_img, H, W = depth.shape
    J = votes.shape[3]
    Hl, Wl = H // r, W // r
    assert Hl * Wl * T * 256 < 1 << 32
    acc = np.zeros((n_img, J, grid(H, shift), grid(W, shift)), np.uint32)
    zacc = np.zeros(acc.shape, np.uint64)
    for i in range(n_img):
        for y in range(Hl):
            for x in range(Wl):
                if gate is not None and int(gate[i, y, x]) in (0, NO_PIXEL):
                    continue
                xd, yd = x * r, y * r
                d = int(depth[i, yd, xd])
                if d == 0 or d == NO_PIXEL:
                    continue
                for t in range(T):
                    at = walk(depth[i], forest[t], D, xd, yd, scale)
                    if at is None:
                        continue
                    for j in range(J):
                        mx, my, mz, w = (int(v) for v in votes[t, at[0], at[1], j])
                        if w < 1 or w > 256:
                            continue
                        vx, vy, vz = xd + vote_pixels(mx, d), yd + vote_pixels(my, d), d + mz
                        if not (0 <= vx < W and 0 <= vy < H and 1 <= vz <= 65534):
                            continue
                        acc[i, j, vy >> shift, vx >> shift] += np.uint32(w)
                        zacc[i, j, vy >> shift, vx >> shift] += np.uint64(w * vz)
    return acc, zacc


def mode(acc, zacc, shift, box, min_support):
    """Rule V5 for one (frame, joint): acc, zacc [Ha, Wa] -> (X, Y, Z, support)."""
    Ha, Wa = acc.shape
    best, win = 0, None
    for cy in range(Ha):
        for cx in range(Wa):
            S = int(acc[max(cy - box, 0):cy + box + 1, max(cx - box, 0):cx + box + 1].sum(dtype=np.uint64))    # clipped to the grid
            if S > best:                                            # strictly: the first cell in row-major order stays
                best, win = S, (cy, cx)
    if best < max(min_support, 1):
        return (-1, -1, 0, 0)
    cy, cx = win
    sx = sy = sz = 0
    for yy in range(max(cy - box, 0), min(cy + box, Ha - 1) + 1):
        for xx in range(max(cx - box, 0), min(cx + box, Wa - 1) + 1):
            w = int(acc[yy, xx])
            sx += w * (16 * (xx << shift) + 8 * (1 << shift))
            sy += w * (16 * (yy << shift) + 8 * (1 << shift))
            sz += int(zacc[yy, xx])
    return (sx // best, sy // best, sz // best, min(best, (1 << 31) - 1))


def modes(acc, zacc, shift=2, box=1, min_support=1):
    """Rule V5.  Returns joints int32 [n_img, J, 4]."""
    n_img, J = acc.shape[:2]
    out = np.zeros((n_img, J, 4), np.int32)
    for i in range(n_img):
        for j in range(J):
            out[i, j] = mode(acc[i, j], zacc[i, j], shift, box, min_support)
    return out


def vote(depth, forest, votes, scale=1., gate=None, r=1, shift=2, box=1, min_support=1, walk=walk):
    """Rules V3 to V5: what rdf_labels_votes_cast writes into joints_out."""
    return modes(*cast(depth, forest, votes, scale, gate, r, shift, walk), shift, box, min_support)
