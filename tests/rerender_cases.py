"""Inputs of the re-render's device tests (tests/test_rerender.py), and of the rasteriser cases that tests/test_hand_scene.py
runs a second time as a mesh: seeded and hand-placed numpy builders that the CPU tests (do the cases bite?) and the GPU tests
(rdf_rerender against tests/rerender_numpy.py) both call, so that both see the same arrays.

`case`       the scenes the re-render has been compared on from the start: an ellipse of points with holes and a depth step
             under five transforms, at each of SIZES.
GRID_CASES   small point grids placed on the screen by hand, one rule of include/rdf_labels.h each (GRID_CASES).  Focal
             length 64, principal points that are multiples of 1/256 and depths that are powers of two: deprojection,
             projection, snapping and the perspective division are exact, and where a case carries "depth" that image was
             worked out by hand and is a literal.  `as_mesh` turns a grid into rdf_hand_scene_render's arguments.

MUTANTS names wrong readings of the rules, `mutant(name)` loads tests/rerender_numpy.py with that reading (tests/mutants.py),
KILLS says which device case must notice which, EQUIVALENT which readings no input can tell from the rule, and why."""
import functools
import importlib

import numpy as np

import frontend_numpy as fnp
import mutants
import rerender_numpy as rn

F = np.float32
EYE = np.identity(4, np.float32)
FOCAL = 64.
ULP_UP = lambda v: float(np.nextafter(F(v), F(np.inf)))         # noqa: E731
ULP_DOWN = lambda v: float(np.nextafter(F(v), F(0)))            # noqa: E731


def make_transform(*a, **kw):
    return importlib.import_module("3d-beats_amd.rerender").SceneRerender.make_transform(*a, **kw)


# ------------------------------------------------------------------ the scenes of the first device test ----------------------
SIZES = ((33, 17), (70, 130), (130, 70))


def plane(tilt_deg=25., spin_deg=40., t=(3000., -7000., 10000.)):
    """An orthonormal plane matrix (rotation about x, then about z) with translations of up to 10^4, float32."""
    a, b = np.deg2rad(tilt_deg), np.deg2rad(spin_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    P = np.identity(4)
    P[:3, :3] = rz @ rx
    P[:3, 3] = t
    return P.astype(np.float32)


def scene(W, H, seed):
    """An ellipse of valid points with holes and a depth step on an empty background, random colours: (pts, colour, cam)."""
    rng = np.random.default_rng(seed)
    f, ppx, ppy = F(W), F((W - 1) / 2 + 0.3), F((H - 1) / 2 - 0.2)
    yy, xx = np.mgrid[:H, :W]
    ell = ((xx - W / 2) / (0.42 * W)) ** 2 + ((yy - H / 2) / (0.40 * H)) ** 2 <= 1.
    d = np.where(xx > 0.55 * W, 800 + 2 * yy + xx % 5, 600 + (3 * xx + yy) % 11 + yy)
    d = np.where(ell, d, 0)
    d[rng.random((H, W)) < 0.03] = 0
    pts = fnp.deproject(d.astype(np.uint16), ppx, ppy, f)
    color = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    return pts, color, (float(f), float(ppx), float(ppy))


def transforms(pts):
    P = plane(20., 0., (0., 30., 650.))
    s = rn.center_sums(fnp.transform(pts, P))
    c = s[:3] / s[3]
    return [("identity", EYE),
            ("scale 0.8 with skew", make_transform(P, c, 0.8, (0.05, -0.1, 0.02))),
            ("scale 1.25", make_transform(P, c, 1.25)),
            ("rotated and pushed out of the frame", make_transform(P, c, 1., (0., 0., 0.), 0.3, (210., 40., 0.))),
            ("partly beyond zmax", np.diag([70., 70., 70., 1.]).astype(np.float32))]


_cases = {}


def case(W, H):
    """Scene, transforms and the restatement's images for one size, computed once."""
    if (W, H) not in _cases:
        pts, color, cam = scene(W, H, W * 1000 + H)
        _cases[W, H] = (pts, color, cam, [(name, M, rn.rerender(pts, color, M, *cam)) for name, M in transforms(pts)])
    return _cases[W, H]


# ------------------------------------------------------------------ point grids placed by hand -------------------------------
def grid(W, H, cam, placed, seed=0):
    """(pts float32 [H, W, 4], colour uint8 [H, W, 3]) of a W x H frame whose point (row, col) sits at the camera-space
    point that the identity projects to the screen position (sx, sy) at depth z, for `placed` = {(row, col): (sx, sy, z)};
    every other point has w = 0.  Random colours."""
    f, ppx, ppy = (F(v) for v in cam)
    pts = np.zeros((H, W, 4), np.float32)
    for (r, c), (sx, sy, z) in placed.items():
        pts[r, c] = ((F(sx) - ppx) * F(z) / f, (F(sy) - ppy) * F(z) / f, z, 1.)
    color = np.random.default_rng(1000 + seed).integers(0, 256, (H, W, 3)).astype(np.uint8)
    return pts, color


def lattice(xs, ys, z):
    """{(row, col): (xs[col], ys[row], z)}: a fronto-parallel lattice."""
    return {(r, c): (sx, sy, z) for r, sy in enumerate(ys) for c, sx in enumerate(xs)}


def as_mesh(pts):
    """The grid as rdf_hand_scene_render's mesh, rule 1's triangles in rule 1's order so that an index into tris is the
    re-render's triangle id: (verts [H * W, 3], vert_part zeros, tris int32 [2 (W - 1)(H - 1), 3], tri_label = 1 + id % 250).
    The triangles of a quad that rule 1 does not make are (0, 0, 0): no area, dropped."""
    H, W = pts.shape[:2]
    j, i = np.mgrid[:H, :W]
    at = (j[:-1, :-1] * W + i[:-1, :-1]).reshape(-1)
    tris = np.stack([np.stack([at, at + 1, at + W], 1), np.stack([at + 1, at + W, at + W + 1], 1)], 1)
    has = pts[..., 3] > 0
    quad = (has[:-1, :-1] & has[:-1, 1:] & has[1:, :-1] & has[1:, 1:]).reshape(-1)
    tris[~quad] = 0
    tris = tris.reshape(-1, 3)
    label = (1 + np.arange(len(tris)) % 250).astype(np.uint16)
    return pts[..., :3].reshape(-1, 3).copy(), np.zeros(W * H, np.int32), tris.astype(np.int32), label


def _f32(*bits):
    return np.array(bits, np.uint32).view(np.float32)


# The fma case.  Point A and the transform's rows were found by a seeded search on the CPU over random points and rows
# whose z term is large (m2 * z near 3e5, taken back by m3): with every operation rounded, A snaps to X = 640, the centre
# of pixel column 2; with the multiply-adds of ((m0 * x + m1 * y) + m2 * z) contracted it snaps to 643.  m1 = 0 and row 2
# has no x or y term, so the point below A (same x and z) snaps to the same X under either reading: A's quad has a
# vertical left edge through the centres of column 2, which the fill rule draws -- and a contracting kernel would not.
FMA_A = _f32(0xC01BD6E4, 0xC095EB37, 0x429788B8)                                    # (x, y, z) of A
FMA_ROWS = _f32(0x3F7E4A86, 0, 0x4529D45D, 0xC8490D99, 0, 0x3F800000, 0, 0, 0, 0, 0x3F724744, 0x3F94B5AC)
FMA_X, FMA_X_CONTRACTED = 640, 643

# The summation-order case: four points far outside an 8 x 8 frame (edge functions beyond 2^24: the sums of w round) at
# depths that are no powers of two (the q round), found by a seeded search on the CPU for a frame in which one stored
# depth differs under w0 + (w1 + w2) and one under q0 + (q1 + q2).  (x, y, z, w) of p00, p01, p10, p11.
SUM_POINTS = (0xC960D220, 0xC934BDF0, 0x46A97375, 0x3F800000, 0x49D3B1E3, 0xC92CF129, 0x46FC39A4, 0x3F800000,
              0xC9C4C5AB, 0x49E7787B, 0x471F4B7B, 0x3F800000, 0x4A1AA11A, 0x4A00B374, 0x471C5787, 0x3F800000)


def _fma_grid():
    x, y, z = (float(v) for v in FMA_A)
    M = np.identity(4, np.float32)
    M[:3] = FMA_ROWS.reshape(3, 4)
    pts = np.zeros((8, 8, 4), np.float32)
    pts[0, 0] = (x, y, z, 1.)
    pts[1, 0] = (x, y + FMA_DY, z, 1.)
    pts[0, 1] = (x + FMA_DX, y, z, 1.)
    pts[1, 1] = (x + FMA_DX, y + FMA_DY, z, 1.)
    return pts, M


FMA_DX, FMA_DY = 5., 9.            # the quad's extent in model units: some three pixels by five at A's depth
FMA_CAM = (FOCAL, 3.5, 3.25)
SUM_CAM = (FOCAL, 3.75, 4.5)

LIMIT = 4096.                        # 2^20 / 256: the screen position that snaps to 2^20
CAM8 = (FOCAL, 0., 0.)               # of the 8 x 8 cases: sx - ppx is sx


def _limit_placed(axis, sign, past):
    """One quad whose triangle 0 has a vertex snapped to sign * 2^20 (+ sign when `past`) on `axis` and covers the 8 x 8
    frame; its fourth point is behind the camera, so triangle 1 is dropped either way."""
    far = sign * (LIMIT + (1 / 256 if past else 0.))
    if sign > 0:        # (-1, -1), (far, -1), (-1, 20): the long edge passes the frame's far corner at 19.9
        tri = [(-1., -1.), (far, -1.), (-1., 20.)]
    else:               # (far, -1), (9, -1), (9, 20)
        tri = [(far, -1.), (9., -1.), (9., 20.)]
    if axis == "y":
        tri = [(b, a) for a, b in tri]
        tri = [tri[0], tri[2], tri[1]]          # p01 and p10 change places with the axes: the same winding on the screen
    placed = {(0, 0): tri[0] + (64.,), (0, 1): tri[1] + (64.,), (1, 0): tri[2] + (64.,), (1, 1): (4., 4., -64.)}
    return placed


def _grid_cases():
    out = {}

    def add(name, W, H, cam, placed, M=EYE, zmin=50., zmax=50000., depth=None, seed=None, pts=None):
        p, color = grid(W, H, cam, placed or {}, len(out) if seed is None else seed)
        if pts is not None:
            p = pts
        for a in (p, color):
            a.setflags(write=False)
        out[name] = {"W": W, "H": H, "cam": cam, "pts": p, "color": color, "M": np.asarray(M, np.float32), "zmin": zmin, "zmax": zmax,
                     "depth": None if depth is None else np.asarray(depth, np.uint16)}

    # 2 x 2 quads whose every edge passes through pixel centres: columns 2.5, 6.5, 10.5 and rows 3.5, 7.5, 11.5.  Column
    # 2 (a left edge on the silhouette) and row 3 (a top edge on it) are drawn, column 10 and row 11 (right, bottom) are
    # not; column 6 and row 7 (shared by two quads) are drawn once.  The quads' diagonals pass through centres as well.
    want = np.zeros((16, 16), np.uint16)
    want[3:11, 2:10] = 512
    add("edges on pixel centres", 16, 16, (FOCAL, 7.5, 7.25), lattice((2.5, 6.5, 10.5), (3.5, 7.5, 11.5), 512.), depth=want)
    # five columns of points folded back on themselves in x at one depth: quads 0 and 3, and 1 and 2, of each row of quads
    # cover the same pixels with the same z bits (512 exactly: every q is w / 512, exact).  The lower id's colour shows.
    want = np.zeros((16, 16), np.uint16)
    want[2:10, 2:10] = 512           # centres i + 0.5 in (2.25, 10.25) and j + 0.5 in (1.75, 9.75)
    add("folded back at one depth", 16, 16, (FOCAL, 7.5, 7.25), lattice((2.25, 6.25, 10.25, 6.25, 2.25), (1.75, 5.75, 9.75), 512.),
        depth=want)
    # a surface that fills the 8 x 8 frame at depth 64, against depth ranges that end on it and one float beside it
    fill = lattice((-1., 4., 9.), (-1., 4., 9.), 64.)
    full, none = np.full((8, 8), 64, np.uint16), np.zeros((8, 8), np.uint16)
    add("surface at zmin", 8, 8, CAM8, fill, zmin=64., zmax=128., depth=full)
    add("surface at zmax", 8, 8, CAM8, fill, zmin=32., zmax=64., depth=full)
    add("surface one float below zmin", 8, 8, CAM8, fill, zmin=ULP_UP(64.), zmax=128., depth=none)
    add("surface one float above zmax", 8, 8, CAM8, fill, zmin=32., zmax=ULP_DOWN(64.), depth=none)
    for axis in "xy":
        for sign in (1, -1):
            s = "+" if sign > 0 else "-"
            add(f"{axis} snapped to {s}2^20", 8, 8, CAM8, _limit_placed(axis, sign, False), depth=full)
            add(f"{axis} snapped to {s}(2^20 + 1)", 8, 8, CAM8, _limit_placed(axis, sign, True), depth=none)
    pts, M = _fma_grid()
    add("rows that a contraction would snap elsewhere", 8, 8, FMA_CAM, None, M=M, pts=pts, seed=77)
    pts = np.zeros((8, 8, 4), np.float32)
    pts[:2, :2] = _f32(*SUM_POINTS).reshape(2, 2, 4)
    add("sums that another order would round elsewhere", 8, 8, SUM_CAM, None, pts=pts, seed=78)
    return out


GRID_CASES = _grid_cases()


@functools.lru_cache(maxsize=None)
def grid_want(name):
    """The restatement's (depth, colour, fragments per pixel) of a grid case."""
    c = GRID_CASES[name]
    return rn.rerender(c["pts"], c["color"], c["M"], *c["cam"], c["zmin"], c["zmax"])


# ------------------------------------------------------------------ mutants ---------------------------------------------------
# Wrong readings of rules 3 to 6 in rerender_numpy.fragments / resolve / depth_key, which hand_scene_numpy draws with too.
FRAGMENT_EDITS = {
    "no fill rule: every edge in": [("need.append(np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, 1))", "need.append(np.where(dy == dy, 0, 1))")],
    "no fill rule: every edge out": [("need.append(np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, 1))", "need.append(np.where(dy == dy, 1, 0))")],
    "left edge read as D.Y > 0": [("np.where((dy < 0) | (", "np.where((dy > 0) | (")],
    "top edge read as D.X < 0": [("(dy == 0) & (dx > 0)", "(dy == 0) & (dx < 0)")],
    "zmin exclusive": [("(zz >= F(zmin))", "(zz > F(zmin))")],
    "zmax exclusive": [("(zz <= F(zmax))", "(zz < F(zmax))")],
    "no depth range": [("ok_z = (zz >= F(zmin)) & (zz <= F(zmax))", "ok_z = zz == zz")],
    "w summed in another order": [("zz = ((w[0] + w[1]) + w[2]) / s", "zz = (w[0] + (w[1] + w[2])) / s")],
    "q summed in another order": [("s = (q[0] + q[1]) + q[2]", "s = q[0] + (q[1] + q[2])")],
    "box one pixel short on the right": [("i1 = np.minimum(W - 1, (vx.max(1) - HALF) >> 8)", "i1 = np.minimum(W - 1, ((vx.max(1) - HALF) >> 8) - 1)")],
    "box one pixel short at the top": [("j0 = np.maximum(0, (vy.min(1) - HALF + SUB - 1) >> 8)", "j0 = np.maximum(0, ((vy.min(1) - HALF + SUB - 1) >> 8) + 1)")],
    "column 0 outside the box": [("i0 = np.maximum(0, (vx.min(1) - HALF + SUB - 1) >> 8)", "i0 = np.maximum(1, (vx.min(1) - HALF + SUB - 1) >> 8)")],
    "depth ties to the highest id": [("return (bits << np.uint64(32)) | np.asarray(tri_id, np.uint64)",
                                      "return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(tri_id, np.uint64))")],
    "farthest fragment wins": [("bits = np.asarray(z, np.float32).view(np.uint32).astype(np.uint64)",
                                "bits = np.uint64(0xFFFFFFFF) - np.asarray(z, np.float32).view(np.uint32).astype(np.uint64)")],
    "one winding only": [("keep = area != 0", "keep = area > 0")],
    "a triangle of area 0 kept": [("keep = area != 0", "keep = area == area")],
}
# Wrong readings of rules 2 and 3 in the lines that rerender_numpy.vertices and hand_scene_numpy.vertices spell alike.
VERTEX_EDITS = {
    "snap by truncation": [("fx = np.floor(", "fx = np.trunc("), ("fy = np.floor(", "fy = np.trunc(")],
    "snap without the + 0.5": [("+ F(ppx)) * F(SUB) + F(0.5))", "+ F(ppx)) * F(SUB))"), ("+ F(ppy)) * F(SUB) + F(0.5))", "+ F(ppy)) * F(SUB))")],
    "|X| <= 2^20 read as <": [("(np.abs(fx) <= F(MAX_SNAPPED))", "(np.abs(fx) < F(MAX_SNAPPED))")],
    "|Y| <= 2^20 read as <": [("(np.abs(fy) <= F(MAX_SNAPPED))", "(np.abs(fy) < F(MAX_SNAPPED))")],
    "no limit on |X|": [("(np.abs(fx) <= F(MAX_SNAPPED))", "(fx == fx)")],
    "no limit on |Y|": [("(np.abs(fy) <= F(MAX_SNAPPED))", "(fy == fy)")],
    "z' >= 0 drawable": [("(zt > 0)", "(zt >= 0)")],
    "behind the camera drawable": [("(zt > 0)", "(zt != 0)")],
}
# The rows of rule 2, spelled for rerender_numpy.vertices (hand_scene_cases has hand_scene_numpy's spelling).
ROW_EDITS = {
    "vertex rows contracted": [("xt, yt, zt = (((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3))",
                                "xt, yt, zt = (_fma(m[r, 2], z, _fma(m[r, 0], x, m[r, 1] * y)) + m[r, 3] for r in range(3))")],
}
# Wrong readings of what the re-render alone has: rule 1, the colour and the stored depth.
OWN_EDITS = {
    "a quad of three points": [("has_point[:-1, :-1] & has_point[:-1, 1:] & has_point[1:, :-1] & has_point[1:, 1:]",
                                "has_point[:-1, :-1] & has_point[:-1, 1:] & has_point[1:, :-1]")],
    "triangle 1 from p00": [("tri1 = np.stack([at + 1, at + W, at + W + 1], 1)", "tri1 = np.stack([at, at + W, at + W + 1], 1)")],
    "depth rounded": [('np.minimum(np.trunc(fr["z"][w]), F(65535))', 'np.minimum(np.floor(fr["z"][w] + F(0.5)), F(65535))')],
    "colour truncated": [("np.minimum(F(255), np.floor(c + F(0.5)))", "np.minimum(F(255), np.floor(c))")],
    "colour corners in another order": [("q1 * corner[:, 1, ch]) + q2 * corner[:, 2, ch]", "q1 * corner[:, 2, ch]) + q2 * corner[:, 1, ch]")],
}
EDITS = {**FRAGMENT_EDITS, **VERTEX_EDITS, **ROW_EDITS, **OWN_EDITS}
MUTANTS = tuple(EDITS)

# No input tells these from the rule: the re-render draws the same image under either reading.
EQUIVALENT = {
    "z' >= 0 drawable": "z' = +-0 makes (f * x') / z' an infinity or (x' = 0, or NaN) a NaN, the snapped value with it, and "
                        "neither passes |X| <= 2^20: the vertex is not drawable under either reading.  The smallest subnormal "
                        "is > 0 under both.",
    "a triangle of area 0 kept": "sgn is 0, so every e_k is 0 and every edge direction D is (0, 0): neither left nor top, "
                                 "e_k >= 1 is asked and no pixel is covered.",
}


@functools.lru_cache(maxsize=None)
def mutant(name=None):
    """tests/rerender_numpy.py under one wrong reading; the unchanged copy without a name."""
    return mutants.load("rerender_numpy", EDITS[name] if name else ())


def rerender_of(mod, c):
    """(depth, colour) of a grid case under the module `mod`."""
    return mod.rerender(c["pts"], c["color"], c["M"], *c["cam"], c["zmin"], c["zmax"])[:2]


# device case -> the mutants it must kill.  "scenes 33 x 17" is the first device test at its smallest size; every other key
# is a GRID_CASES name.
KILLS = {
    "scenes 33 x 17": ("no fill rule: every edge out", "snap without the + 0.5",
                       "depth rounded", "colour truncated", "a quad of three points", "box one pixel short on the right",
                       "box one pixel short at the top", "one winding only", "farthest fragment wins", "no depth range",
                       "triangle 1 from p00", "colour corners in another order", "column 0 outside the box"),
    "edges on pixel centres": ("top edge read as D.X < 0", "no fill rule: every edge in", "no fill rule: every edge out",
                               "left edge read as D.Y > 0"),
    "folded back at one depth": ("depth ties to the highest id", "one winding only"),
    "surface at zmin": ("zmin exclusive", "column 0 outside the box"),
    "surface at zmax": ("zmax exclusive", "snap by truncation"),
    "surface one float below zmin": ("no depth range",),
    "surface one float above zmax": ("no depth range",),
    "x snapped to +2^20": ("|X| <= 2^20 read as <",),
    "x snapped to -2^20": ("|X| <= 2^20 read as <",),
    "y snapped to +2^20": ("|Y| <= 2^20 read as <",),
    "y snapped to -2^20": ("|Y| <= 2^20 read as <",),
    "x snapped to +(2^20 + 1)": ("no limit on |X|",),
    # (its fourth point is behind the camera, and truncation brings -(2^20 + 1) + 0.5 back to -2^20)
    "x snapped to -(2^20 + 1)": ("no limit on |X|", "behind the camera drawable", "snap by truncation"),
    "y snapped to +(2^20 + 1)": ("no limit on |Y|",),
    "y snapped to -(2^20 + 1)": ("no limit on |Y|",),
    "rows that a contraction would snap elsewhere": ("vertex rows contracted",),
    "sums that another order would round elsewhere": ("w summed in another order", "q summed in another order"),
}
