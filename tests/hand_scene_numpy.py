"""CPU restatement of rdf_hand_scene_render (include/rdf_labels.h): rules V, 3 to 6, T, E and H in numpy, float32 where the
header says fp32 (one rounding per operation; numpy never contracts), int64 / uint32 where it says integer.  Coverage,
depth and the depth test are rerender_numpy's `fragments` and `resolve`: the rules are rdf_rerender's own.
`render` returns what the kernels write plus, per frame, what the scene tests ask about: the fragments that reached the
depth test and the table's depth."""
import numpy as np

from rerender_numpy import EMPTY, HALF, MAX_SNAPPED, SUB, depth_key, fragments, resolve  # noqa: F401

F = np.float32
U32 = np.uint32
FRAME_STEP = 0x9E3779B9


def vertices(verts, vert_part, tforms, f, ppx, ppy):
    """Rule V and rule 3 for every vertex of one frame (tforms float32 [n_parts, 12]): (X, Y int64, z' float32, drawable).
    A vertex whose part is out of range is not drawable, so every triangle that uses it is dropped."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    part = np.asarray(vert_part, np.int64).reshape(-1)
    tforms = np.asarray(tforms, np.float32).reshape(-1, 12)
    known = (part >= 0) & (part < len(tforms))
    m = tforms[np.where(known, part, 0)] if len(tforms) else np.zeros((len(verts), 12), np.float32)
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    with np.errstate(all="ignore"):
        xt, yt, zt = (((m[:, 4 * r] * x + m[:, 4 * r + 1] * y) + m[:, 4 * r + 2] * z) + m[:, 4 * r + 3] for r in range(3))
        fx = np.floor(((F(f) * xt) / zt + F(ppx)) * F(SUB) + F(0.5))
        fy = np.floor(((F(f) * yt) / zt + F(ppy)) * F(SUB) + F(0.5))
        ok = known & (zt > 0) & (np.abs(fx) <= F(MAX_SNAPPED)) & (np.abs(fy) <= F(MAX_SNAPPED))
    X = np.where(ok, fx, 0).astype(np.int64)
    Y = np.where(ok, fy, 0).astype(np.int64)
    return X, Y, zt.astype(np.float32), ok


def mix(x):
    """The 32-bit mixing function of rule H, on uint32 arrays (wrapping)."""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def hashes(seed, n, n_px):
    """(hash, hash') of rule H for every pixel of frame n."""
    base = mix(np.array([(int(seed) + int(n) * FRAME_STEP) & 0xFFFFFFFF], np.uint64))[0]
    h = mix(np.arange(n_px, dtype=np.uint64) ^ np.uint64(base))
    return h, mix(h.astype(np.uint64) ^ np.uint64(0x85EBCA6B))


def table_depth(table, W, H, f, ppx, ppy, zmin, zmax):
    """Rule T for one frame: (zt float32 [H * W], there bool [H * W])."""
    nx, ny, nz, d = (F(v) for v in np.asarray(table, np.float32).reshape(4))
    j, i = np.mgrid[:H, :W]
    rx = ((i.astype(np.float32) + F(0.5)) - F(ppx)) / F(f)
    ry = ((j.astype(np.float32) + F(0.5)) - F(ppy)) / F(f)
    t = ((nx * rx + ny * ry) + nz).reshape(-1)
    with np.errstate(all="ignore"):
        zt = (d / t).astype(np.float32)
        there = (t > 0) & (zt >= F(zmin)) & (zt <= F(zmax))
    return zt, there


def _u16(z):
    return np.minimum(np.trunc(z), F(65535)).astype(np.uint16)


def rasterise(W, H, verts, vert_part, tris, part_tforms, f, ppx, ppy, zmin=50., zmax=50000.):
    """Rules V and 3 to 6 for every frame: a list of {"fr": the fragments that reached the depth test (pix, tri = index
    into tris, z), "winner": per pixel the index into fr of the fragment that won, or -1}.  It does not depend on labels,
    table, holes or noise, so one call serves every such variant of a scene."""
    part_tforms = np.asarray(part_tforms, np.float32)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    n_verts = len(np.asarray(verts).reshape(-1, 3))
    ids = np.nonzero(((tris >= 0) & (tris < n_verts)).all(1))[0]            # the others are dropped, not read
    out = []
    for n in range(part_tforms.shape[0]):
        X, Y, z, ok = vertices(verts, vert_part, part_tforms[n], f, ppx, ppy)
        with np.errstate(all="ignore"):
            fr = fragments(X, Y, z, ok, ids.astype(np.uint64), tris[ids], W, H, zmin, zmax)
        fr["tri"] = ids[fr["tri"]]
        out.append({"fr": fr, "winner": resolve(W * H, fr["pix"], fr["z"], fr["tri"])})
    return out


def render(W, H, verts, vert_part, tris, tri_label, part_tforms, table, f, ppx, ppy, zmin=50., zmax=50000., empty_depth=65535,
           seed=0, hole_threshold=0, noise_amp=0, geometry=None):
    """(depth uint16 [N, H, W], labels uint16 [N, H, W], info): info[n] = rasterise's record of frame n (`geometry`, when
    it has been computed before) plus "zt", "table": rule T, and "mesh": bool [H * W], the pixels that show the mesh
    before holes."""
    part_tforms = np.asarray(part_tforms, np.float32)
    N = part_tforms.shape[0]
    tri_label = np.asarray(tri_label, np.uint16).reshape(-1)
    n_px = W * H
    if geometry is None:
        geometry = rasterise(W, H, verts, vert_part, tris, part_tforms, f, ppx, ppy, zmin, zmax)
    depth = np.empty((N, n_px), np.uint16)
    labels = np.empty((N, n_px), np.uint16)
    info = []
    for n in range(N):
        fr, winner = geometry[n]["fr"], geometry[n]["winner"]
        mesh = winner >= 0
        zm = np.zeros(n_px, np.float32)
        zm[mesh] = fr["z"][winner[mesh]]
        lab = np.zeros(n_px, np.uint16)
        lab[mesh] = tri_label[fr["tri"][winner[mesh]]]
        zt, there = np.zeros(n_px, np.float32), np.zeros(n_px, bool)
        if table is not None:
            zt, there = table_depth(np.asarray(table, np.float32).reshape(-1, 4)[n], W, H, f, ppx, ppy, zmin, zmax)
        mesh = mesh & ~(there & ~(zm <= zt))
        shows_table = there & ~mesh
        drawn = mesh | shows_table
        d = np.where(mesh, _u16(zm), np.where(shows_table, _u16(np.where(there, zt, 0)), 0)).astype(np.int64)
        lab = np.where(mesh, lab, 0).astype(np.uint16)
        h, h2 = hashes(seed, n, n_px)
        if hole_threshold:
            drawn = drawn & ~(h < U32(hole_threshold))
        if noise_amp > 0:
            d = np.clip(d + (h2 % U32(2 * noise_amp + 1)).astype(np.int64) - noise_amp, 1, 65534)
        depth[n] = np.where(drawn, d, empty_depth).astype(np.uint16)
        labels[n] = np.where(drawn, lab, 0)
        info.append({"fr": fr, "winner": winner, "zt": zt, "table": there, "mesh": mesh})
    return depth.reshape(N, H, W), labels.reshape(N, H, W), info
