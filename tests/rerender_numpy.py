"""CPU restatement of the re-render (include/rdf_labels.h, rdf_rerender and rdf_points_center): the six rules in numpy,
float32 where the header says fp32 (one rounding per operation; numpy never contracts), int64 where it says integer.
`rerender` returns what the kernels write plus the number of fragments that reached each pixel's depth test, which the
kernels do not keep and the fill-rule tests need."""
import numpy as np

F = np.float32
SUB, HALF, MAX_SNAPPED = 256, 128, float(1 << 20)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def vertices(pts, M, f, ppx, ppy):
    """Rules 2 and 3 for every point: (X, Y int64, z' float32, has_point, drawable), each [H, W]."""
    pts = np.asarray(pts, np.float32)
    m = np.asarray(M, np.float32).reshape(4, 4)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    with np.errstate(all="ignore"):
        xt, yt, zt = (((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3))
        fx = np.floor(((F(f) * xt) / zt + F(ppx)) * F(SUB) + F(0.5))
        fy = np.floor(((F(f) * yt) / zt + F(ppy)) * F(SUB) + F(0.5))
        ok = (zt > 0) & (np.abs(fx) <= F(MAX_SNAPPED)) & (np.abs(fy) <= F(MAX_SNAPPED))
    X = np.where(ok, fx, 0).astype(np.int64)
    Y = np.where(ok, fy, 0).astype(np.int64)
    return X, Y, zt.astype(np.float32), pts[..., 3] > 0, ok


def mesh(has_point):
    """Rule 1: (ids uint64 [T], corner indices int64 [T, 3] into the flattened frame) of every triangle of an existing quad."""
    H, W = has_point.shape
    if H < 2 or W < 2:
        return np.zeros(0, np.uint64), np.zeros((0, 3), np.int64)
    quad = has_point[:-1, :-1] & has_point[:-1, 1:] & has_point[1:, :-1] & has_point[1:, 1:]
    y, x = np.nonzero(quad)
    at = y * W + x
    ids = 2 * (y * (W - 1) + x)
    tri0 = np.stack([at, at + 1, at + W], 1)
    tri1 = np.stack([at + 1, at + W, at + W + 1], 1)
    ids = np.concatenate([ids, ids + 1]).astype(np.uint64)
    order = np.argsort(ids, kind="stable")
    return ids[order], np.concatenate([tri0, tri1])[order]


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def fragments(X, Y, z, drawable, ids, tris, W, H, zmin, zmax):
    """Rules 4 and 5: every fragment that reaches the depth test, as a dict of arrays [N]: pix (j * W + i), tri (index
    into ids / tris), z, q0..q2, s."""
    Xf, Yf, zf, ok = X.reshape(-1), Y.reshape(-1), z.reshape(-1), drawable.reshape(-1)
    tri = np.nonzero(ok[tris].all(1))[0] if len(tris) else np.zeros(0, np.int64)
    vx, vy, vz = Xf[tris[tri]], Yf[tris[tri]], zf[tris[tri]]            # [T, 3]
    area = _edge(vx[:, 0], vy[:, 0], vx[:, 1], vy[:, 1], vx[:, 2], vy[:, 2])
    keep = area != 0
    tri, vx, vy, vz, sgn = tri[keep], vx[keep], vy[keep], vz[keep], np.sign(area[keep])
    need = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = sgn * (vx[:, b] - vx[:, a]), sgn * (vy[:, b] - vy[:, a])
        need.append(np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, 1))
    i0 = np.maximum(0, (vx.min(1) - HALF + SUB - 1) >> 8)
    i1 = np.minimum(W - 1, (vx.max(1) - HALF) >> 8)
    j0 = np.maximum(0, (vy.min(1) - HALF + SUB - 1) >> 8)
    j1 = np.minimum(H - 1, (vy.max(1) - HALF) >> 8)
    out = {k: [] for k in ("pix", "tri", "z", "q0", "q1", "q2", "s")}
    nx, ny = i1 - i0 + 1, j1 - j0 + 1
    for dj in range(int(ny.max()) if len(tri) else 0):
        rows = np.nonzero((ny > dj) & (nx > 0))[0]
        for di in range(int(nx[rows].max()) if len(rows) else 0):
            sel = rows[nx[rows] > di]
            i, j = i0[sel] + di, j0[sel] + dj
            px, py = i * SUB + HALF, j * SUB + HALF
            e = []
            inside = np.ones(len(sel), bool)
            for k in range(3):
                a, b = (k + 1) % 3, (k + 2) % 3
                ek = sgn[sel] * _edge(vx[sel, a], vy[sel, a], vx[sel, b], vy[sel, b], px, py)
                inside &= ek >= need[k][sel]
                e.append(ek)
            sel, i, j = sel[inside], i[inside], j[inside]
            w = [ek[inside].astype(np.float32) for ek in e]
            q = [w[k] / vz[sel, k] for k in range(3)]
            s = (q[0] + q[1]) + q[2]
            zz = ((w[0] + w[1]) + w[2]) / s
            ok_z = (zz >= F(zmin)) & (zz <= F(zmax))
            out["pix"].append((j * W + i)[ok_z])
            out["tri"].append(tri[sel][ok_z])
            out["z"].append(zz[ok_z])
            for k in range(3):
                out[f"q{k}"].append(q[k][ok_z])
            out["s"].append(s[ok_z])
    dt = {"pix": np.int64, "tri": np.int64}
    return {k: (np.concatenate(v) if v else np.zeros(0)).astype(dt.get(k, np.float32)) for k, v in out.items()}


def depth_key(z, tri_id):
    """Rule 6: (bits(z) << 32) | triangle id, uint64."""
    bits = np.asarray(z, np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | np.asarray(tri_id, np.uint64)


def resolve(n_px, pix, z, tri_id):
    """Rule 6 on an explicit fragment list: per pixel, the index of the fragment that wins (-1 where there is none)."""
    pix = np.asarray(pix, np.int64)
    key = depth_key(z, tri_id)
    best = np.full(n_px, EMPTY, np.uint64)
    np.minimum.at(best, pix, key)
    winner = np.full(n_px, -1, np.int64)
    won = np.nonzero(key == best[pix])[0]
    # several fragments of one pixel with one key would be the same triangle twice: the first stands
    winner[pix[won][::-1]] = won[::-1]
    return winner


def rerender(pts, color, M, f, ppx, ppy, zmin=50., zmax=50000.):
    """(depth uint16 [H, W], colour uint8 [H, W, 3], fragments per pixel int64 [H, W])."""
    pts = np.asarray(pts, np.float32)
    color = np.asarray(color, np.uint8)
    H, W = pts.shape[:2]
    X, Y, z, has, ok = vertices(pts, M, f, ppx, ppy)
    ids, tris = mesh(has)
    fr = fragments(X, Y, z, ok, ids, tris, W, H, zmin, zmax)
    count = np.bincount(fr["pix"], minlength=H * W).reshape(H, W)
    depth = np.zeros(H * W, np.uint16)
    out = np.zeros((H * W, 3), np.uint8)
    winner = resolve(H * W, fr["pix"], fr["z"], ids[fr["tri"]])
    px = np.nonzero(winner >= 0)[0]
    w = winner[px]
    depth[px] = np.minimum(np.trunc(fr["z"][w]), F(65535)).astype(np.uint16)
    corner = color.reshape(-1, 3)[tris[fr["tri"][w]]].astype(np.float32)        # [n, 3 corners, 3 channels]
    q0, q1, q2, s = fr["q0"][w], fr["q1"][w], fr["q2"][w], fr["s"][w]
    for ch in range(3):
        c = ((q0 * corner[:, 0, ch] + q1 * corner[:, 1, ch]) + q2 * corner[:, 2, ch]) / s
        out[px, ch] = np.minimum(F(255), np.floor(c + F(0.5))).astype(np.uint8)
    return depth.reshape(H, W), out.reshape(H, W, 3), count


def center_sums(pts):
    """rdf_points_center's value up to the order of the fp64 additions: numpy's float64 sums of the four components."""
    return np.asarray(pts, np.float32).reshape(-1, 4).astype(np.float64).sum(0)
