"""CPU restatement of the depth front end (include/rdf_frontend.h): the RANSAC plane of CalibratedPlane and the per-frame
chain deproject -> transform -> filter_points_by_plane -> remove_missing_3d_points_from_depth_image -> gaussian_depth_filter,
in float32 numpy with the operation order the header states (each line one fp32 rounding; numpy never contracts)."""
import numpy as np

F = np.float32
NAN = F(np.nan)


def mat_row(r, x, y, z, w):
    """Row r (4 floats) of M times (x, y, z, w) in glm 0.9.9's order: (Mul0 + Mul1) + (Mul2 + Mul3)."""
    r = np.asarray(r, np.float32)
    return (r[0] * x + r[1] * y) + (r[2] * z + r[3] * w)


def transform_xyzw(M, x, y, z, w):
    M = np.asarray(M, np.float32).reshape(4, 4)
    return [mat_row(M[i], x, y, z, w) for i in range(4)]


def _normalize(v):
    x, y, z = v
    s = F(1) / np.sqrt((x * x + y * y) + z * z)
    return (x * s, y * s, z * s)


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


# ------------------------------------------------------------------ the plane ------------------------------------------------
def draw_index(u, dim_x, dim_y):
    """r = floor((u * dim_x) * dim_y) in fp32, or -1 for a miss (r < 0 or r >= dim_x * dim_y)."""
    v = np.floor((F(u) * F(dim_x)) * F(dim_y))
    return int(v) if v >= 0 and v < dim_x * dim_y else -1


def plane_candidates(rand, pts, dim_x, dim_y, start_mat=None):
    """(candidates float32 [G, 16], counts int32 [G]: 0 valid, -1 invalid) -- rdf_make_plane_candidates."""
    rand = np.asarray(rand, np.float32)
    P = np.asarray(pts, np.float32).reshape(-1, 4)
    G, N = rand.shape[0], int(dim_x) * int(dim_y)
    cand = np.full((G, 16), NAN, np.float32)
    counts = np.full(G, -1, np.int32)
    v = np.floor((rand * F(dim_x)) * F(dim_y)).astype(np.float64)
    hit = (v >= 0) & (v < N)
    r = np.where(hit, v, 0).astype(np.int64)
    take = hit & (P[r, 2] > 0)
    rank = np.cumsum(take, 1)
    ok = rank[:, -1] >= 3
    idx = [np.argmax(take & (rank == k + 1), 1) for k in range(3)]
    Q = [P[r[np.arange(G), j], :3] for j in idx]         # [G, 3] each: the first three points taken
    with np.errstate(all="ignore"):
        sub = lambda a, b: tuple(a[:, k] - b[:, k] for k in range(3))     # noqa: E731
        v0 = _normalize(sub(Q[1], Q[0]))
        v1 = _normalize(sub(Q[2], Q[0]))
        za = _normalize(_cross(v0, v1))
        xa = v0
        ya = _normalize(_cross(za, xa))
        z0, o1 = np.zeros(G, np.float32), np.ones(G, np.float32)
        M = np.stack([xa[0], ya[0], za[0], -Q[0][:, 0],
                      xa[1], ya[1], za[1], -Q[0][:, 1],
                      xa[2], ya[2], za[2], -Q[0][:, 2],
                      z0, z0, z0, o1], 1).astype(np.float32)
    cand[ok] = M[ok]
    counts[ok] = 0
    if start_mat is not None and G:
        cand[0] = np.asarray(start_mat, np.float32).reshape(16)
        counts[0] = 0
    return cand, counts


def plane_inliers(pts, cand, T, counts=None, chunk=64):
    """counts + the number of points with w == 1 and |z'| < T per candidate (a candidate without inliers keeps its count).
    torch on the CPU does the arithmetic when it is importable (the same float32 operations, one per line, many threads)."""
    P = np.asarray(pts, np.float32).reshape(-1, 4)
    P = P[P[:, 3] == 1]
    cand = np.asarray(cand, np.float32).reshape(-1, 16)
    G = cand.shape[0]
    out = np.zeros(G, np.int64)
    T = F(T)
    try:
        import torch
        # every point here has w == 1, and M23 * 1 == M23 exactly; |z'| < T is z' < T && z' > -T, NaN included
        x, y, z = (torch.from_numpy(np.ascontiguousarray(P[:, k]))[None, :] for k in range(3))
        for a in range(0, G, chunk):
            m = torch.from_numpy(np.ascontiguousarray(cand[a:a + chunk, 8:12]))
            zz = torch.mul(x, m[:, 0:1])
            zz.add_(torch.mul(y, m[:, 1:2]))
            t = torch.mul(z, m[:, 2:3])
            t.add_(m[:, 3:4])
            zz.add_(t)
            out[a:a + chunk] = (zz.abs_() < float(T)).sum(1).numpy()
    except ImportError:
        with np.errstate(all="ignore"):
            for a in range(0, G, chunk):
                m = cand[a:a + chunk, 8:12]
                zz = mat_row(m.T[:, :, None], P[None, :, 0], P[None, :, 1], P[None, :, 2], P[None, :, 3])
                out[a:a + chunk] = ((zz < T) & (zz > -T)).sum(1)
    base = np.zeros(G, np.int32) if counts is None else np.asarray(counts, np.int32).copy()
    return np.where(out > 0, base + out, base).astype(np.int32)


def plane_select(cand, counts, plane_in=None):
    """(plane float32 [16], best, best_count, c float64 [4], status) -- rdf_plane_select.  status 0 ok, 1 no plane (then
    plane is plane_in unchanged)."""
    cand = np.asarray(cand, np.float32).reshape(-1, 16)
    counts = np.asarray(counts, np.int32)
    best = int(np.argmax(counts))
    M = cand[best].copy()
    with np.errstate(all="ignore"):
        t = (-M[11]) / M[10]
        c = np.asarray(M.reshape(4, 4), np.float64) @ np.array([0., 0., t, 1.])
    ok = counts[best] > 0 and abs(c[2]) < 0.001
    plane = np.zeros(16, np.float32) if plane_in is None else np.asarray(plane_in, np.float32).reshape(16).copy()
    if ok:
        M[3] = M[3] + -F(c[0])
        M[7] = M[7] + -F(c[1])
        plane = M
    return plane, best, int(counts[best]), c, 0 if ok else 1


def calibrate(rand, pts, dim_x, dim_y, T, start_mat=None, plane_in=None):
    cand, counts = plane_candidates(rand, pts, dim_x, dim_y, start_mat)
    counts = plane_inliers(pts, cand, T, counts)
    return plane_select(cand, counts, plane_in) + (cand, counts)


# ------------------------------------------------------------------ per frame ------------------------------------------------
def deproject(depth, ppx, ppy, f, pts=None):
    """pts float32 [n, H, W, 4]; pixels with d == 0 keep what `pts` held (zeros when None)."""
    depth = np.asarray(depth)
    shp = depth.shape
    out = np.zeros(shp + (4,), np.float32) if pts is None else np.asarray(pts, np.float32).reshape(shp + (4,)).copy()
    H, W = shp[-2:]
    yy, xx = np.mgrid[:H, :W]
    d = depth.astype(np.float32)
    with np.errstate(all="ignore"):
        px = (d * (xx.astype(np.float32) - F(ppx))) / F(f)
        py = (d * (yy.astype(np.float32) - F(ppy))) / F(f)
    p = np.stack(np.broadcast_arrays(px, py, d, np.ones_like(d)), -1)
    m = depth > 0
    out[m] = p[m]
    return out


def transform(pts, M):
    pts = np.asarray(pts, np.float32).copy()
    m = pts[..., 3] == 1
    with np.errstate(all="ignore"):
        q = transform_xyzw(M, pts[..., 0], pts[..., 1], pts[..., 2], pts[..., 3])
    for k in range(4):
        pts[..., k] = np.where(m, q[k], pts[..., k])
    return pts


def filter_by_plane(pts, T):
    pts = np.asarray(pts, np.float32).copy()
    pts[(pts[..., 3] == 1) & (pts[..., 2] > -F(T))] = 0
    return pts


def remove_missing(pts, depth):
    depth = np.asarray(depth).copy()
    depth[np.asarray(pts)[..., 3] == 0] = 0
    return depth


def float2uint_rd(v):
    q = np.floor(np.asarray(v, np.float32)).astype(np.float64)
    q = np.where(np.isnan(q) | (q < 0), 0, np.minimum(q, 4294967295.0))
    return q.astype(np.uint32)


def gaussian(depth, weights):
    """gaussian_depth_filter of one or more frames [.., H, W] uint16 with float32 weights [k, k]."""
    depth = np.asarray(depth)
    w = np.asarray(weights, np.float32)
    k = w.shape[0]
    h = k // 2
    H, W = depth.shape[-2:]
    pad = np.zeros(depth.shape[:-2] + (H + 2 * h, W + 2 * h), np.uint16)
    pad[..., h:h + H, h:h + W] = depth
    inb = np.zeros((H + 2 * h, W + 2 * h), bool)
    inb[h:h + H, h:h + W] = True
    w0 = np.zeros(depth.shape, np.float32)
    wn = np.zeros(depth.shape, np.float32)
    s = np.zeros(depth.shape, np.float32)
    for dy in range(k):
        for dx in range(k):
            d = pad[..., dy:dy + H, dx:dx + W]
            ok = inb[dy:dy + H, dx:dx + W]
            wt = w[dy, dx]
            zero = ok & (d == 0)
            non = ok & (d != 0)
            w0 = np.where(zero, w0 + wt, w0)
            wn = np.where(non, wn + wt, wn)
            s = np.where(non, s + d.astype(np.float32) * wt, s)
    with np.errstate(all="ignore"):
        q = float2uint_rd(s / wn)
    return np.where(w0 > wn, 0, q.astype(np.uint16)).astype(np.uint16)


def chain(depth, ppx, ppy, f, M, T, weights=None):
    """The five stand-alone kernels in the app's order (3d_bz.py:163-212), pts starting from zeros: (depth_out, pts)."""
    pts = deproject(depth, ppx, ppy, f)
    pts = filter_by_plane(transform(pts, M), T)
    d = remove_missing(pts, depth)
    if weights is not None:
        d = gaussian(d, weights)
    return d, pts


def frame_front(depth, ppx, ppy, f, M, T, weights=None):
    """rdf_frame_front, per pixel as the header states: (depth_out, pts_out)."""
    depth = np.asarray(depth)
    p = deproject(depth, ppx, ppy, f)
    with np.errstate(all="ignore"):
        q = np.stack(transform_xyzw(M, p[..., 0], p[..., 1], p[..., 2], p[..., 3]), -1)
    gone = (depth == 0) | ((q[..., 3] == 1) & (q[..., 2] > -F(T)))
    pts = np.where(gone[..., None], F(0), q).astype(np.float32)
    clean = np.where(gone | (q[..., 3] == 0), 0, depth).astype(np.uint16)
    return (gaussian(clean, weights) if weights is not None else clean), pts
