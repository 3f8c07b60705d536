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
                    (`part_tforms_cycle`, `tables_cycle`): more frames than k_hand_raster's grid has rows."""
import numpy as np

import hand_scene_numpy as hs

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
