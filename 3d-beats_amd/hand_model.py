"""An articulated hand as a labelled triangle mesh: what HandSceneRenderer (hand_scene.py, rdf_hand_scene_render) draws.

The reference makes its training sets by rendering a rigged hand in Blender (datagen/); nothing of that is used here.  This
hand is 16 rigid parts -- a palm and five fingers (thumb, index, middle, ring, pinky) of three phalanges -- each a closed
capped cylinder of elliptical section, and a pose is 26 numbers.  Pure numpy, no device; everything is deterministic.

Spaces.  A part's vertices are in PART space: the cylinder's axis is +y, from the joint at the origin to the next joint at
(0, length, 0).  HAND space has the wrist at the origin, the palm along +y, the back of the hand towards +z and the thumb on
the -x side (a right hand seen from above); fingers flex towards -z.  PLANE space is the table's: z is the height above the
table (the space CalibratedPlane's matrix maps camera points into).  Lengths are in depth units, `units_per_mm` per
millimetre: 10 for the D415's 0.1 mm unit (rs_util.py:28-33).

Dimensions (mm), plausible for an adult hand, this module's own:
  palm      95 long (wrist to knuckles), 84 wide, 26 thick
  finger    base (x, y) on the palm   rest splay   phalanx lengths   phalanx radii
  thumb     (-40, 25)                  55 deg       44, 32, 28        11, 10, 9
  index     (-30, 95)                   8 deg       42, 25, 22        9.5, 8.5, 7.5
  middle    (-10, 98)                   0 deg       46, 28, 23        9.5, 8.5, 7.5
  ring      ( 10, 95)                  -8 deg       43, 27, 22        9, 8, 7
  pinky     ( 29, 88)                 -18 deg       33, 19, 20        8, 7, 6.5
A phalanx's cylinder starts half a radius before its joint, inside its parent, so that a flexed joint shows no gap.

Pose (float64 [26]): wrist x, y, z in plane space (depth units); yaw, pitch, roll (radians; hand -> plane is
T(wrist) Rz(yaw) Rx(pitch) Ry(roll), so a negative pitch lowers the fingers); then per finger a spread angle (added to the
rest splay, about z) and three flexion angles (about the phalanx's own x axis, positive towards the palm side).  A finger
is a planar chain: phalanx k points along (0, cos a_k, -sin a_k) in the finger's plane, a_k the sum of its first k + 1
flexions, and hangs off the end of phalanx k - 1.
"""
import numpy as np

FINGERS = ("thumb", "index", "middle", "ring", "pinky")
N_PARTS = 16
POSE_SIZE = 26
PALM = 0

PALM_LENGTH, PALM_HALF_WIDTH, PALM_HALF_THICKNESS = 95., 42., 13.
FINGER_BASE = ((-40., 25.), (-30., 95.), (-10., 98.), (10., 95.), (29., 88.))
FINGER_REST_SPLAY = tuple(np.deg2rad(v) for v in (55., 8., 0., -8., -18.))
PHALANX_LENGTH = ((44., 32., 28.), (42., 25., 22.), (46., 28., 23.), (43., 27., 22.), (33., 19., 20.))
PHALANX_RADIUS = ((11., 10., 9.), (9.5, 8.5, 7.5), (9.5, 8.5, 7.5), (9., 8., 7.), (8., 7., 6.5))
PALM_SIDES, PALM_RINGS, FINGER_SIDES, FINGER_RINGS = 12, 5, 8, 2

# what sample_poses draws from, uniformly: (low, high); lengths in mm, angles in radians
SAMPLE_RANGES = {"x": (-60., 60.), "y": (-110., -30.), "height": (60., 140.), "yaw": (-0.6, 0.6), "pitch": (-0.3, 0.2),
                 "roll": (-0.35, 0.35), "spread": (-0.12, 0.12), "flexion": (0., 0.6)}
# Hand shapes, what shape_poses draws a finger's angles from: shape -> finger -> ((spread low, high), (flexion low, high)), the
# flexion range for each of the finger's three joints.  An extended finger flexes at most 0.25 a joint, a curled one at least
# 1.0 (three joints of 1.0 to 1.45 fold the tip back onto the palm); the thumb, which folds across the palm, curls less.
_OUT, _CURLED, _THUMB_IN = ((-0.12, 0.12), (0., 0.25)), ((-0.05, 0.05), (1.0, 1.45)), ((-0.05, 0.05), (0.55, 0.9))
SHAPES = {
    "open":  {"thumb": _OUT, "index": _OUT, "middle": _OUT, "ring": _OUT, "pinky": _OUT},
    "fist":  {"thumb": _THUMB_IN, "index": _CURLED, "middle": _CURLED, "ring": _CURLED, "pinky": _CURLED},
    "point": {"thumb": _THUMB_IN, "index": _OUT, "middle": _CURLED, "ring": _CURLED, "pinky": _CURLED},
    # thumb and index bent towards each other, the other three extended
    "pinch": {"thumb": ((-0.3, -0.15), (0.35, 0.55)), "index": ((-0.05, 0.05), (0.5, 0.75)), "middle": _OUT, "ring": _OUT,
              "pinky": _OUT},
}
REST_FLEXION = 0.25             # press_sequence: every joint of a resting finger
PRESS_SPEED_MM = 4.             # press_sequence: the tip's descent per frame

# fine: 1 palm, 2 finger (proximal and middle phalanges), 3..7 the fingertips (distal phalanges) thumb..pinky
LABEL_COLORS = ((200, 200, 200, 255), (90, 90, 220, 255), (230, 60, 60, 255), (240, 160, 40, 255), (230, 220, 50, 255),
                (60, 200, 80, 255), (200, 60, 210, 255))


def part_index(finger, phalanx):
    """Part number of a finger's phalanx (0 proximal .. 2 distal); the palm is part 0."""
    f = FINGERS.index(finger) if isinstance(finger, str) else int(finger)
    assert 0 <= f < 5 and 0 <= int(phalanx) < 3
    return 1 + 3 * f + int(phalanx)


def _cylinder(rx, rz, y0, y1, sides, rings):
    """A closed capped cylinder about the y axis: (verts float64 [V, 3], tris int32 [T, 3]).  Two cap centres, then
    rings + 1 rings of `sides` vertices; every edge is shared by two triangles that run along it in opposite directions."""
    ang = 2. * np.pi * np.arange(sides) / sides
    verts = [(0., y0, 0.), (0., y1, 0.)]
    for r in range(rings + 1):
        y = y0 + (y1 - y0) * r / rings
        verts += [(rx * np.cos(a), y, rz * np.sin(a)) for a in ang]
    tris = []
    at = lambda r, s: 2 + r * sides + s % sides       # noqa: E731
    for s in range(sides):
        tris.append((0, at(0, s), at(0, s + 1)))
        tris.append((1, at(rings, s + 1), at(rings, s)))
        for r in range(rings):
            a, b, c, d = at(r, s), at(r, s + 1), at(r + 1, s), at(r + 1, s + 1)
            tris += [(a, d, b), (a, c, d)]          # counter-clockwise seen from outside
    return np.array(verts, np.float64), np.array(tris, np.int32)


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = np.identity(4)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _shift(v):
    m = np.identity(4)
    m[:3, 3] = v
    return m


_MIRROR = np.diag([-1., 1., 1., 1.])


class HandModel:
    def __init__(self, units_per_mm=10., mirrored=False):
        """mirrored: the other hand -- the same mesh with x negated (and each triangle's order reversed, so that the
        winding stays outward) on the mirrored skeleton."""
        self.units_per_mm = float(units_per_mm)
        self.is_mirrored = bool(mirrored)
        u = self.units_per_mm
        verts, parts, tris, tri_part = [], [], [], []
        n = 0
        for p in range(N_PARTS):
            if p == PALM:
                v, t = _cylinder(PALM_HALF_WIDTH * u, PALM_HALF_THICKNESS * u, 0., PALM_LENGTH * u, PALM_SIDES, PALM_RINGS)
            else:
                f, k = divmod(p - 1, 3)
                r, length = PHALANX_RADIUS[f][k] * u, PHALANX_LENGTH[f][k] * u
                v, t = _cylinder(r, r, -0.5 * r, length, FINGER_SIDES, FINGER_RINGS)
            if mirrored:
                v = v * (-1., 1., 1.)
                t = t[:, ::-1]
            verts.append(v)
            parts.append(np.full(len(v), p, np.int32))
            tris.append(t + n)
            tri_part.append(np.full(len(t), p, np.int32))
            n += len(v)
        self.verts = np.concatenate(verts).astype(np.float32)
        self.vert_part = np.concatenate(parts)
        self.tris = np.ascontiguousarray(np.concatenate(tris), np.int32)
        self.tri_part = np.concatenate(tri_part)
        self.tip_parts = np.array([part_index(f, 2) for f in range(5)], np.int32)
        # the end point of each fingertip in its distal phalanx's part space
        self.tip_points = np.array([(0., PHALANX_LENGTH[f][2] * u, 0.) for f in range(5)], np.float64)

    def mirrored(self):
        return HandModel(self.units_per_mm, not self.is_mirrored)

    # ------------------------------------------------------------------ pose ------------------------------------------------
    def rest_pose(self, wrist=(0., 0., 0.)):
        pose = np.zeros(POSE_SIZE, np.float64)
        pose[:3] = wrist
        return pose

    def _hand_from_part(self, pose):
        """float64 [16, 4, 4] of one pose: part space -> hand space, the kinematic chain."""
        u = self.units_per_mm
        out = np.empty((N_PARTS, 4, 4), np.float64)
        out[PALM] = np.identity(4)
        for f in range(5):
            spread, flex = pose[6 + 4 * f], pose[7 + 4 * f:10 + 4 * f]
            m = _shift((FINGER_BASE[f][0] * u, FINGER_BASE[f][1] * u, 0.)) @ _rot("z", FINGER_REST_SPLAY[f] + spread)
            for k in range(3):
                if k:
                    m = m @ _shift((0., PHALANX_LENGTH[f][k - 1] * u, 0.))      # hangs off the end of the one before
                m = m @ _rot("x", -flex[k])
                out[part_index(f, k)] = m
        if self.is_mirrored:
            out = _MIRROR @ out @ _MIRROR
        return out

    @staticmethod
    def _plane_from_hand(pose):
        return _shift(pose[:3]) @ _rot("z", pose[3]) @ _rot("x", pose[4]) @ _rot("y", pose[5])

    def part_matrices(self, poses, cam_from_plane=None):
        """float64 [N, 16, 4, 4]: part space -> camera space (plane space when cam_from_plane is None) of every pose."""
        poses = np.asarray(poses, np.float64).reshape(-1, POSE_SIZE)
        cam = np.identity(4) if cam_from_plane is None else np.asarray(cam_from_plane, np.float64).reshape(4, 4)
        out = np.empty((len(poses), N_PARTS, 4, 4), np.float64)
        for i, pose in enumerate(poses):
            out[i] = (cam @ self._plane_from_hand(pose)) @ self._hand_from_part(pose)
        return out

    def part_transforms(self, poses, cam_from_plane=None):
        """float32 [N, 16, 12]: rows 0..2 of part_matrices, composed in float64 and cast once -- the part_tforms of
        rdf_hand_scene_render.  cam_from_plane: the inverse of the table plane's matrix (plane space -> camera space)."""
        m = self.part_matrices(poses, cam_from_plane)
        return np.ascontiguousarray(m[:, :, :3, :].reshape(len(m), N_PARTS, 12).astype(np.float32))

    def fingertips(self, poses, cam_from_plane=None):
        """float64 [N, 5, 3]: the end points of the five fingertips."""
        m = self.part_matrices(poses, cam_from_plane)[:, self.tip_parts]
        tip = np.concatenate([self.tip_points, np.ones((5, 1))], 1)        # on the part's axis: its own mirror image
        return np.einsum("nfij,fj->nfi", m, tip)[..., :3]

    def sample_poses(self, n, rng, ranges=None):
        """n poses drawn uniformly from SAMPLE_RANGES (overridden entry by entry by `ranges`) with a numpy Generator: one
        rng.random((n, 26)) call, so the same seed gives the same poses.  The default ranges put the wrist below the middle
        of the view of a camera that looks down its plane space's -z (y = -110..-30 mm, so that the fingers cross the
        centre) at 60..140 mm above the table."""
        return self._draw_poses(n, rng, ranges, None)

    def shape_poses(self, shape, n, rng, ranges=None):
        """sample_poses with every finger's spread and flexion ranges taken from SHAPES[shape] (a name, or a table entry of
        its form): the wrist and the hand's angles come from SAMPLE_RANGES and `ranges` as they do there; one
        rng.random((n, 26)) call, the same seed gives the same poses, and a mirrored model gives the mirror images."""
        return self._draw_poses(n, rng, ranges, SHAPES[shape] if isinstance(shape, str) else shape)

    def shape_dataset_poses(self, num_images, rng, shapes=tuple(SHAPES), ranges=None):
        """The poses of a shape dataset (HandSceneRenderer.make_shape_dataset): frame n is of shape shapes[n % len(shapes)].
        One shape_poses call per shape, in the order of `shapes`, for the frames of that shape.  Returns (poses float64
        [num_images, 26], shape indices int32 [num_images])."""
        shapes = tuple(shapes)
        assert shapes and all(s in SHAPES for s in shapes), shapes
        num_images = int(num_images)
        index = (np.arange(num_images) % len(shapes)).astype(np.int32)
        poses = np.empty((num_images, POSE_SIZE), np.float64)
        for k, shape in enumerate(shapes):
            at = np.flatnonzero(index == k)
            poses[at] = self.shape_poses(shape, len(at), rng, ranges)
        return poses, index

    def _draw_poses(self, n, rng, ranges, fingers):
        r = dict(SAMPLE_RANGES)
        r.update(ranges or {})
        u = self.units_per_mm
        lo = np.empty(POSE_SIZE)
        hi = np.empty(POSE_SIZE)
        for k, name in enumerate(("x", "y", "height")):
            lo[k], hi[k] = r[name][0] * u, r[name][1] * u
        for k, name in enumerate(("yaw", "pitch", "roll")):
            lo[3 + k], hi[3 + k] = r[name]
        for f in range(5):
            spread, flexion = (r["spread"], r["flexion"]) if fingers is None else fingers[FINGERS[f]]
            lo[6 + 4 * f], hi[6 + 4 * f] = spread
            lo[7 + 4 * f:10 + 4 * f], hi[7 + 4 * f:10 + 4 * f] = flexion
        poses = lo + (hi - lo) * rng.random((int(n), POSE_SIZE))
        if self.is_mirrored:
            poses[:, (0, 3, 5)] *= -1.         # the other hand's poses are the mirror images of this hand's
        return poses

    def _tip_height(self, pose, finger):
        return self.fingertips(pose[None])[0, finger, 2]

    def press_sequence(self, n_frames, finger, wrist=(0., 0., 450.), speed_mm=PRESS_SPEED_MM, yaw=0.):
        """float64 [n_frames, 26]: a resting hand (every flexion REST_FLEXION, wrist at `wrist`, depth units) whose one
        finger presses: the end point of its tip goes down by speed_mm per frame, by flexing the knuckle alone, until it is
        one tip radius above the table (the skin touches), stays there, and comes back the same way; frame k is as far
        down as frame n_frames - 1 - k.  The knuckle angle is found by bisection on the tip's height, in float64."""
        f = FINGERS.index(finger) if isinstance(finger, str) else int(finger)
        u = self.units_per_mm
        rest = self.rest_pose(wrist)
        rest[3] = yaw
        for g in range(5):
            rest[7 + 4 * g:10 + 4 * g] = REST_FLEXION
        top, touch = self._tip_height(rest, f), PHALANX_RADIUS[f][2] * u
        assert top > touch, "the resting tip is already on the table"

        def height(a):
            p = rest.copy()
            p[7 + 4 * f] = a
            return self._tip_height(p, f)
        poses = np.repeat(rest[None], int(n_frames), 0)
        for k in range(int(n_frames)):
            want = max(touch, top - min(k, n_frames - 1 - k) * speed_mm * u)
            lo, hi = REST_FLEXION, 0.5 * np.pi          # the tip only goes down between these
            assert height(hi) <= want, "the table is out of this finger's reach: lower the wrist"
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if height(mid) > want else (lo, mid)
            poses[k, 7 + 4 * f] = hi if want > touch else lo      # never below the table
        return poses

    # ------------------------------------------------------------------ labels ----------------------------------------------
    @staticmethod
    def label_table(scheme="fine"):
        """uint16 [16]: part -> id.  'fine': 1 palm, 2 finger, 3..7 the fingertips thumb..pinky.  The two layers of a
        LayeredDecisionForest: 'coarse' (1 palm, 2 finger, 3 tip) and 'tips' (1..5 the fingertips, 0 elsewhere: the second
        layer is trained and run on the pixels of the coarse class 3 only)."""
        t = np.zeros(N_PARTS, np.uint16)
        for f in range(5):
            for k in range(3):
                p = part_index(f, k)
                t[p] = {"fine": 3 + f if k == 2 else 2, "coarse": 3 if k == 2 else 2, "tips": 1 + f if k == 2 else 0}[scheme]
        t[PALM] = 0 if scheme == "tips" else 1
        return t

    @staticmethod
    def id_to_color(scheme="fine"):
        """{id: [r, g, b, 255]} without id 0, for dataset.write_dataset."""
        if scheme == "fine":
            return {i + 1: list(c) for i, c in enumerate(LABEL_COLORS)}
        if scheme == "coarse":
            return {i + 1: list(LABEL_COLORS[i]) for i in range(3)}
        return {i + 1: list(LABEL_COLORS[2 + i]) for i in range(5)}

    @staticmethod
    def layered_config(coarse_model, tips_model):
        """The config of a LayeredDecisionForest over a 'coarse' and a 'tips' forest (paths or DecisionForest objects)
        whose composite is the 'fine' scheme: coarse 1 and 2 are final, coarse 3 defers to the second layer's 1..5, which
        become 3..7."""
        conditions = [[0, 1], [0, 2], [1, 3]] + [[0, 3 + f] for f in range(5)]
        return {"layers": [{"model": coarse_model}, {"model": tips_model, "filter_model": 0, "filter_model_class": 3}],
                "conditions": conditions, "label_colors": [list(c) for c in LABEL_COLORS]}
