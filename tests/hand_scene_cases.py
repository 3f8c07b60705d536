"""The hand-built scenes of tests/test_hand_scene.py: a small mesh of three parts placed so that every rule of
rdf_hand_scene_render decides some pixel.  Positions are given on the screen and turned into model points at depths that
are powers of two with a focal length of 64, so that where it matters (the shared edge) projection and snapping are exact.

Triangles, by name (TRI maps a name to its indices in `tris`):
  quad     two triangles of part 0, labels 6 and 7, from 30 % outside the frame on every side: clipped by all four borders;
           896 deep on the left and 1152 on the right, so it dips under a table 1000 deep
  edge     two triangles of part 1 at depth 512, labels 1 and 2, that share the vertical edge x = 8.5 from y = 2.25 to 11.75:
           the centres of pixels (8, 2..11) lie on it (frame 0, where part 1 is not moved)
  tie      one triangle of part 1 at depth 512 twice, labels 3 and 4: the lower index wins every pixel
  behind   a triangle of part 2, label 5: frame 0 puts part 2 behind the camera, later frames in front
  bad      triangles that must be dropped without being read: a vertex index of n_verts, one of -1, and a vertex whose
           part is 99; label 9 appears nowhere
Frames differ in every part's transform and in the table, so a wrong frame stride or key-plane offset shows.

`case`              the scene at the SIZES, one and MAX_FRAMES frames, under every row of VARIANTS.
`many_frames_case`  the same mesh at 16 x 13 in 65541 frames that cycle through seven settings of the transforms and tables
                    (`part_tforms_cycle`, `tables_cycle`): more frames than k_hand_raster's grid has rows.
`OWN_CASES`         one rule of T, E and H each on a 16 x 16 frame; `grid_case` draws rerender_cases.GRID_CASES as meshes.

MUTANTS names wrong readings of the rules, `mutant(name)` loads tests/hand_scene_numpy.py with that reading (tests/mutants.py),
KILLS says which device case must notice which, EQUIVALENT which readings no input can tell from the rule, and why."""
import functools

import numpy as np

import hand_scene_numpy as hs
import mutants
import rerender_cases as rc

F = np.float32
FOCAL = 64.
SIZES = ((33, 17), (70, 130))
MAX_FRAMES = 3
EDGE_COLUMN, EDGE_ROWS = 8, range(2, 12)
TRI = {"quad": (0, 1), "edge": (2, 3), "tie": (4, 5), "behind": (6,), "bad": (7, 8, 9)}
# (name, table, empty_depth, hole_threshold, noise_amp)
VARIANTS = (("plain dataset frame", False, 65535, 0, 0),
            ("camera frame with table, holes and noise", True, 0, 1 << 30, 5),
            ("no table, holes and noise, empty 0", False, 0, 1 << 31, 40),
            ("table, clean, empty 65535", True, 65535, 0, 0))
SEED = 20240607


def camera(W, H):
    return FOCAL, (W - 1) / 2. + 0.25, (H - 1) / 2. - 0.25


def _affine(rot_z=0., scale=1., shift=(0., 0., 0.)):
    c, s = np.cos(rot_z) * scale, np.sin(rot_z) * scale
    return np.array([c, -s, 0., shift[0], s, c, 0., shift[1], 0., 0., scale, shift[2]], np.float32)


def mesh(W, H):
    """(verts float32 [V, 3], vert_part int32 [V], tris int32 [T, 3], tri_label uint16 [T])."""
    f, ppx, ppy = camera(W, H)

    def at(sx, sy, z):      # the model point that the identity projects to screen (sx, sy) at depth z
        return ((sx - ppx) * z / f, (sy - ppy) * z / f, z)
    verts = [at(-0.3 * W, -0.3 * H, 896.), at(1.3 * W, -0.3 * H, 1152.), at(-0.3 * W, 1.3 * H, 896.), at(1.3 * W, 1.3 * H, 1152.),
             at(8.5, 2.25, 512.), at(8.5, 11.75, 512.), at(3., 6., 512.), at(13., 7., 512.),
             at(15.2, 2.1, 512.), at(24.7, 3.3, 512.), at(18.4, 12.9, 512.),
             at(20., 6., 512.), at(27., 8., 512.), at(22., 13., 640.),
             at(5., 5., 512.)]
    part = [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 99]
    n = len(verts)
    tris = [(0, 1, 2), (1, 2, 3), (4, 5, 6), (5, 4, 7), (8, 9, 10), (8, 9, 10), (11, 12, 13),
            (4, 5, n), (-1, 5, 6), (4, 7, 14)]
    label = [6, 7, 1, 2, 3, 4, 5, 9, 9, 9]
    return np.array(verts, np.float32), np.array(part, np.int32), np.array(tris, np.int32), np.array(label, np.uint16)


def part_tforms():
    """float32 [3 frames, 3 parts, 12]."""
    return np.stack([
        np.stack([_affine(), _affine(), _affine(shift=(0., 0., -2048.))]),
        np.stack([_affine(0.05, 1., (40., -25., 30.)), _affine(0.1, 1., (12., 9., 20.)), _affine()]),
        np.stack([_affine(-0.08, 0.9, (-60., 35., 80.)), _affine(0., 1., (-25., 10., -60.)), _affine(0.3, 1.1, (-70., 20., 5.))]),
    ])


def tables():
    """float32 [3, 4]: facing the camera at depth 1000 in frame 0, tilted in the others."""
    return np.array([(0., 0., 1., 1000.), (0.1, -0.05, 1., 990.), (-0.07, 0.12, 0.98, 1015.)], np.float32)


# ------------------------------------------------------------------ more frames than the grid has rows ------------------------
# k_hand_raster strides frames over gridDim.y, capped at 65535: six frames more make the loop body run twice.  Frame n has
# the transforms (and the table) of setting n % 7, and 65535 % 7 = 1 (the three settings above would not do: 65535 % 3 = 0),
# so a kernel that indexed by row of the grid, not by frame, would draw another setting.  No holes and no noise: a frame
# then does not depend on its index.
MANY_N, MANY_PERIOD, MANY_ROWS = 65541, 7, 65535
MANY_SIZE = (16, 13)


def part_tforms_cycle(p=MANY_PERIOD):
    """float32 [p frames, 3 parts, 12]: p distinct settings; part 2 is behind the camera in settings 0 and 4."""
    out = []
    for k in range(p):
        behind = k % 4 == 0
        out.append(np.stack([_affine(0.03 * k - 0.1, 1. + 0.02 * k, (10. * k - 30., 6. * k - 20., 25. * k - 40.)),
                             _affine(0.05 * k, 1., (4. * k - 10., 3. * k - 8., 30. - 12. * k)),
                             _affine(shift=(0., 0., -2048.)) if behind else _affine(0.1 * k, 1., (-60. - 5. * k, -20. + 4. * k, 10. * k))]))
    return np.stack(out)


def tables_cycle(p=MANY_PERIOD):
    """float32 [p, 4]: the table nearer than part of the quad in every setting, tilted another way in each."""
    return np.array([(0.03 * k - 0.09, 0.1 - 0.04 * k, 1., 1040. - 15. * k) for k in range(p)], np.float32)


# (name, table, empty_depth)
MANY_VARIANTS = (("without a table", False, 65535), ("with the cycling tables", True, 0))


def many_frames_case():
    """{"cam", "mesh", "tforms" [7, 3, 12], "tables" [7, 4], "index": int [MANY_N] = n % 7,
    "want": {variant name: (depth, labels, info) of the 7 settings}}, computed once."""
    if "many" not in _cases:
        W, H = MANY_SIZE
        cam, m, t, tb = camera(W, H), mesh(W, H), part_tforms_cycle(), tables_cycle()
        geometry = hs.rasterise(W, H, m[0], m[1], m[2], t, *cam)
        want = {name: hs.render(W, H, *m, t, tb if with_table else None, *cam, empty_depth=empty, geometry=geometry)
                for name, with_table, empty in MANY_VARIANTS}
        _cases["many"] = {"cam": cam, "mesh": m, "tforms": t, "tables": tb, "index": np.arange(MANY_N) % MANY_PERIOD, "want": want}
    return _cases["many"]


_cases = {}


def case(W, H):
    """The scene at one size, computed once and shared: {"cam", "mesh", "tforms", "tables", "geometry" (rasterise of the
    three frames), "want": {(n_frames, variant name): (depth, labels, info)}}."""
    if (W, H) not in _cases:
        cam, m, t = camera(W, H), mesh(W, H), part_tforms()
        geometry = hs.rasterise(W, H, m[0], m[1], m[2], t, *cam)
        want = {}
        for n_frames in (1, MAX_FRAMES):
            for name, with_table, empty, holes, noise in VARIANTS:
                want[n_frames, name] = hs.render(W, H, *m, t[:n_frames], tables()[:n_frames] if with_table else None, *cam,
                                                 empty_depth=empty, seed=SEED, hole_threshold=holes, noise_amp=noise,
                                                 geometry=geometry[:n_frames])
        _cases[W, H] = {"cam": cam, "mesh": m, "tforms": t, "tables": tables(), "geometry": geometry, "want": want}
    return _cases[W, H]


# ------------------------------------------------------------------ one rule each ---------------------------------------------
# OWN_CASES: what rdf_hand_scene_render has beyond the shared rasteriser (rules T, E and H) on a 16 x 16 frame with focal
# length 64, one mesh quad at depth 512 (screen 2.5 .. 10.5 by 3.5 .. 11.5: pixels 2 .. 9 by 3 .. 10, its edges on pixel
# centres) and tables that face the camera, (0, 0, 1, d): t = 1 and zt = d exactly at every pixel.  The rasteriser's own
# cases are rerender_cases.GRID_CASES, drawn here as meshes (`grid_case`).
OWN_SIZE, OWN_CAM = (16, 16), (FOCAL, 7.5, 7.25)
QUAD_PIXELS = (slice(3, 11), slice(2, 10))


def _own_mesh():
    pts, _ = rc.grid(16, 16, OWN_CAM, rc.lattice((2.5, 10.5), (3.5, 11.5), 512.))
    return rc.as_mesh(pts)


def _facing(*d):
    return np.array([(0., 0., 1., v) for v in d], np.float32)


def _own_cases():
    out = {}

    def add(name, tables, zmin=50., zmax=50000., empty=0, seed=SEED, holes=0, noise=0):
        out[name] = {"W": 16, "H": 16, "cam": OWN_CAM, "mesh": _own_mesh(), "tables": tables, "zmin": zmin, "zmax": zmax, "empty": empty,
                     "tforms": np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (len(tables), 1, 1)),
                     "seed": seed, "holes": holes, "noise": noise}
    add("quad coplanar with the table", _facing(512.))
    add("tables at the ends of the depth range", _facing(1024., rc.ULP_UP(1024.), 256., rc.ULP_DOWN(256.)), zmin=256., zmax=1024., empty=7)
    # the threshold is the hash of one drawn pixel of frame 0, the median one: it stays, every pixel with a smaller hash goes
    h = hs.hashes(SEED, 0, 256)[0]
    add("hole threshold on a pixel's own hash", _facing(1024., 1024.), holes=int(np.sort(h)[128]))
    add("noise against both clamps", _facing(2., 65533.), zmin=1., zmax=70000., noise=5)
    return out


OWN_CASES = _own_cases()


def grid_case(name):
    """rerender_cases.GRID_CASES[name] as rdf_hand_scene_render's arguments: no table, empty depth 0, one frame."""
    c = rc.GRID_CASES[name]
    return {"W": c["W"], "H": c["H"], "cam": c["cam"], "mesh": rc.as_mesh(c["pts"]), "tables": None, "zmin": c["zmin"], "zmax": c["zmax"],
            "empty": 0, "tforms": np.ascontiguousarray(c["M"][:3]).reshape(1, 1, 12), "seed": 0, "holes": 0, "noise": 0,
            "depth": c["depth"]}


def render_of(mod, c):
    """(depth, labels) of an OWN_CASES or grid_case record under the module `mod`."""
    with np.errstate(all="ignore"):
        return mod.render(c["W"], c["H"], *c["mesh"], c["tforms"], c["tables"], *c["cam"], c["zmin"], c["zmax"], c["empty"], c["seed"],
                          c["holes"], c["noise"])[:2]


_wants = {}


def want_of(name):
    """The restatement's (depth, labels) of a case of OWN_CASES or, as "grid: <name>", of rerender_cases.GRID_CASES."""
    if name not in _wants:
        _wants[name] = render_of(hs, grid_case(name[6:]) if name.startswith("grid: ") else OWN_CASES[name])
    return _wants[name]


# ------------------------------------------------------------------ mutants ---------------------------------------------------
# rerender_cases.FRAGMENT_EDITS reach this restatement through the functions it imports; VERTEX_EDITS apply to its own
# `vertices`, which spells rule 3 as rerender_numpy does.  Its own spelling of rule 2's rows and rules V, T, E and H:
OWN_EDITS = {
    "vertex rows contracted": [("xt, yt, zt = (((m[:, 4 * r] * x + m[:, 4 * r + 1] * y) + m[:, 4 * r + 2] * z) + m[:, 4 * r + 3] for r in range(3))",
                                "xt, yt, zt = (_fma(m[:, 4 * r + 2], z, _fma(m[:, 4 * r], x, m[:, 4 * r + 1] * y)) + m[:, 4 * r + 3] for r in range(3))")],
    "a part out of range read as part 0": [("ok = known & (zt > 0)", "ok = (zt > 0)")],
    "table against mesh tie read as <": [("~(zm <= zt)", "~(zm < zt)")],
    "table zmin exclusive": [("(zt >= F(zmin))", "(zt > F(zmin))")],
    "table zmax exclusive": [("(zt <= F(zmax))", "(zt < F(zmax))")],
    "table without a depth range": [("there = (t > 0) & (zt >= F(zmin)) & (zt <= F(zmax))", "there = (t > 0) & (zt == zt)")],
    "table t >= 0": [("there = (t > 0) &", "there = (t >= 0) &")],
    "table ray without the + 0.5": [("(i.astype(np.float32) + F(0.5))", "i.astype(np.float32)"), ("(j.astype(np.float32) + F(0.5))", "j.astype(np.float32)")],
    "table of frame 0 in every frame": [(".reshape(-1, 4)[n]", ".reshape(-1, 4)[0]")],
    "hole test read as <=": [("(h < U32(hole_threshold))", "(h <= U32(hole_threshold))")],
    "a hole keeps its label": [("labels[n] = np.where(drawn, lab, 0)", "labels[n] = lab")],
    "hash ignores the frame": [("h, h2 = hashes(seed, n, n_px)", "h, h2 = hashes(seed, 0, n_px)")],
    "noise clamped at 0": [("- noise_amp, 1, 65534)", "- noise_amp, 0, 65534)")],
    "noise clamped at 65535": [("- noise_amp, 1, 65534)", "- noise_amp, 1, 65535)")],
    "noise on an empty pixel": [("depth[n] = np.where(drawn, d, empty_depth)", "depth[n] = np.where(drawn | (noise_amp > 0), d, empty_depth)")],
    "stored depth rounded": [("np.minimum(np.trunc(z), F(65535))", "np.minimum(np.floor(z + F(0.5)), F(65535))")],
}
EDITS = {**OWN_EDITS, **rc.VERTEX_EDITS}
MUTANTS = tuple(rc.FRAGMENT_EDITS) + tuple(EDITS)

EQUIVALENT = {
    "z' >= 0 drawable": rc.EQUIVALENT["z' >= 0 drawable"],
    "a triangle of area 0 kept": rc.EQUIVALENT["a triangle of area 0 kept"],
    "table t >= 0": "t = +-0 makes zt = d / t an infinity, or a NaN where d is 0 or NaN: zt <= zmax fails for +inf and NaN, "
                    "zmin <= zt for -inf, so there is no table at that pixel under either reading.",
}


@functools.lru_cache(maxsize=None)
def mutant(name=None):
    """tests/hand_scene_numpy.py under one wrong reading; without a name the unchanged copy, drawing with an unchanged copy
    of rerender_numpy's functions."""
    r = rc.mutant(name if name in rc.FRAGMENT_EDITS else None)
    mod = mutants.load("hand_scene_numpy", EDITS.get(name, ()) if name else (), fragments=r.fragments, resolve=r.resolve,
                       depth_key=r.depth_key)
    # an edit of rules T, E or H stands in `render` and `table_depth` alone: `rasterise` is the restatement's, text for text
    mod.RASTERISES_ALIKE = name in OWN_EDITS and name not in ("vertex rows contracted", "a part out of range read as part 0")
    return mod


# device case -> the mutants it must kill.  "scene 33 x 17" is the hand-built scene under every row of VARIANTS;
# "grid: <name>" a rasteriser case of rerender_cases.GRID_CASES as a mesh; every other key is one of OWN_CASES.
KILLS = {
    "scene 33 x 17": ("no fill rule: every edge in", "no fill rule: every edge out", "left edge read as D.Y > 0",
                      "q summed in another order", "box one pixel short on the right", "box one pixel short at the top",
                      "column 0 outside the box", "depth ties to the highest id", "farthest fragment wins", "one winding only",
                      "a part out of range read as part 0", "table ray without the + 0.5", "table of frame 0 in every frame",
                      "a hole keeps its label", "hash ignores the frame", "noise on an empty pixel", "stored depth rounded",
                      "snap by truncation", "snap without the + 0.5"),
    "grid: edges on pixel centres": ("top edge read as D.X < 0", "no fill rule: every edge in", "no fill rule: every edge out",
                                     "left edge read as D.Y > 0"),
    "grid: folded back at one depth": ("depth ties to the highest id",),
    "grid: surface at zmin": ("zmin exclusive",),
    "grid: surface at zmax": ("zmax exclusive",),
    "grid: surface one float below zmin": ("no depth range",),
    "grid: surface one float above zmax": ("no depth range",),
    "grid: x snapped to +2^20": ("|X| <= 2^20 read as <",),
    "grid: x snapped to -2^20": ("|X| <= 2^20 read as <",),
    "grid: y snapped to +2^20": ("|Y| <= 2^20 read as <",),
    "grid: y snapped to -2^20": ("|Y| <= 2^20 read as <",),
    "grid: x snapped to +(2^20 + 1)": ("no limit on |X|",),
    "grid: x snapped to -(2^20 + 1)": ("no limit on |X|", "behind the camera drawable"),
    "grid: y snapped to +(2^20 + 1)": ("no limit on |Y|",),
    "grid: y snapped to -(2^20 + 1)": ("no limit on |Y|",),
    "grid: rows that a contraction would snap elsewhere": ("vertex rows contracted",),
    "grid: sums that another order would round elsewhere": ("w summed in another order", "q summed in another order"),
    "quad coplanar with the table": ("table against mesh tie read as <",),
    "tables at the ends of the depth range": ("table zmin exclusive", "table zmax exclusive", "table without a depth range"),
    "hole threshold on a pixel's own hash": ("hole test read as <=",),
    "noise against both clamps": ("noise clamped at 0", "noise clamped at 65535"),
}
