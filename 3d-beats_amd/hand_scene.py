"""Labelled depth frames of the articulated hand of hand_model.py, rendered on the device (librdf_labels.so:
rdf_hand_scene_render): the package's own training sets and raw camera sequences, from a seed.  The reference renders a
rigged hand in Blender for this (datagen/) and ships no recordings.

`HandSceneRenderer.render` draws a batch of poses -- one hand (16 parts) or two (32: a right hand, then its mirror image) --
into device depth and label images, two launches per chunk of `max_frames` on the current stream, nothing read back.
`make_dataset` writes a directory that DecisionTreeDatasetConfig, train_forest and score_saved_model read as any other,
`make_shape_dataset` one whose frames are labelled by the hand's shape (hand_model.SHAPES), for a shape.ShapeVoter's forest;
`camera_sequence` gives raw frames with the table under the hand, the input of BeatsSession.run_sequence.  With `sensor=` (a
StereoSensor) all three draw a clean left and a clean right frame and report what the stereo camera makes of them, in place of
rule H's holes and noise.  The rasteriser's rules are in include/rdf_labels.h.
"""
import os

import numpy as np

from . import _lib
from .dataset import SHAPES_FILE, TARGETS_FILE, write_dataset
from .device import DeviceArray, device_ptr, get_runtime, to_device
from .hand_model import N_PARTS, POSE_SIZE, SHAPES, HandModel

# make_shape_dataset: the colour of shape k's label, 1 + k (at most as many shapes as a ShapeVoter's forest has classes but 0)
SHAPE_COLORS = tuple((40 + 14 * k, 250 - 13 * k, (97 * k) % 256, 255) for k in range(15))
Z_NEAR, Z_FAR = 50., 50000.         # SceneRerender's planes
FRAME_SEED_STEP = 0x9E3779B9        # rule H: frame n under seed s is frame 0 under seed s + n * this


def look_down_plane(height, tilt=0.):
    """The table plane's matrix (camera space -> plane space, as CalibratedPlane's) for a camera `height` depth units above
    the plane-space origin that looks down, tilted by `tilt` radians about its x axis: image x is plane x, image y is
    plane -y."""
    c, s = np.cos(tilt), np.sin(tilt)
    m = np.identity(4)
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = -c, s, -s, -c         # Rx(tilt) diag(1, -1, -1)
    m[2, 3] = height
    return m


def table_of_plane(plane):
    """(nx, ny, nz, d) of rdf_hand_scene_render for the plane z = 0 of plane space, with d >= 0."""
    plane = np.asarray(plane, np.float64).reshape(4, 4)
    t = np.array([plane[2, 0], plane[2, 1], plane[2, 2], -plane[2, 3]])
    return (-t if t[3] < 0 else t).astype(np.float32)


class HandSceneRenderer:
    def __init__(self, depth_dims, intrinsics, model=None, z_near=Z_NEAR, z_far=Z_FAR, max_frames=64):
        """depth_dims = (DIM_Y, DIM_X); intrinsics = (focal, ppx, ppy) of the depth camera; model: a HandModel (the right
        hand; its mirror image is the left).  The key workspace holds max_frames frames: longer batches go in chunks."""
        self._rt = get_runtime()
        self._lb = _lib.load("labels")
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.f, self.ppx, self.ppy = (float(np.float32(v)) for v in np.asarray(intrinsics, np.float64).reshape(-1)[:3])
        self.z_near, self.z_far = float(z_near), float(z_far)
        self.max_frames = int(max_frames)
        assert self.max_frames >= 1
        self.model = model or HandModel()
        self.left_model = self.model.mirrored()
        r, l = self.model, self.left_model
        # one hand, and two: the left hand's vertices, parts and triangles behind the right hand's
        self._mesh = {N_PARTS: (r.verts, r.vert_part, r.tris, r.tri_part),
                      2 * N_PARTS: (np.concatenate([r.verts, l.verts]), np.concatenate([r.vert_part, l.vert_part + N_PARTS]),
                                    np.concatenate([r.tris, l.tris + len(r.verts)]), np.concatenate([r.tri_part, l.tri_part]))}
        self._mesh_cu, self._labels_cu = {}, {}
        # the key buffer starts out empty (every byte 0xFF) and every call leaves it so
        n = int(self._lb.rdf_hand_scene_workspace_bytes(self.max_frames, self.DIM_X, self.DIM_Y))
        self._keys = DeviceArray((max(n, 8),), np.uint8).fill(0xFF)

    def _device_mesh(self, n_parts):
        if n_parts not in self._mesh_cu:
            verts, vert_part, tris, _ = self._mesh[n_parts]
            self._mesh_cu[n_parts] = (to_device(verts.astype(np.float32)), to_device(vert_part.astype(np.int32)),
                                      to_device(tris.astype(np.int32)))
        return self._mesh_cu[n_parts]

    def tri_labels(self, n_parts, labels):
        """uint16 [n_tris] of a scheme's name ('fine', 'coarse', 'tips') or of an explicit part -> id table (16 entries, used
        for both hands, or n_parts)."""
        table = HandModel.label_table(labels) if isinstance(labels, str) else np.asarray(labels, np.uint16).reshape(-1)
        assert table.size in (N_PARTS, n_parts), table.shape
        return table[self._mesh[n_parts][3] % table.size].astype(np.uint16)

    def transforms(self, poses, plane, left_poses=None):
        """float32 [N, 16 or 32, 12]: the part_tforms of `poses` (and of the left hand's `left_poses`) for a camera whose
        table plane is `plane` (camera space -> plane space)."""
        cam_from_plane = np.linalg.inv(np.asarray(plane, np.float64).reshape(4, 4))
        t = self.model.part_transforms(poses, cam_from_plane)
        if left_poses is None:
            return t
        left = self.left_model.part_transforms(left_poses, cam_from_plane)
        assert len(left) == len(t)
        return np.ascontiguousarray(np.concatenate([t, left], 1))

    def fingertip_targets(self, poses, plane, left_poses=None):
        """Host int32 [N, 5 or 10, 3] = (tx, ty, tz): where the end points of the fingertips of `poses` (thumb..pinky, then the
        left hand's of `left_poses`) fall in the image of a camera whose table plane is `plane` -- the targets of
        VoteFitter.add.  HandModel.fingertips in camera space, projected with this renderer's own focal length and principal
        point in float64: tx = floor(f X / Z + ppx), ty alike, tz = round(Z) (numpy's rint).  (tx, ty) may lie outside the frame.  tz = 0, the
        joint is absent, when Z is outside [z_near, z_far] or tz outside 1..65534."""
        cam_from_plane = np.linalg.inv(np.asarray(plane, np.float64).reshape(4, 4))
        tips = self.model.fingertips(poses, cam_from_plane)
        if left_poses is not None:
            left = self.left_model.fingertips(left_poses, cam_from_plane)
            assert len(left) == len(tips)
            tips = np.concatenate([tips, left], 1)
        X, Y, Z = tips[..., 0], tips[..., 1], tips[..., 2]
        seen = (Z >= self.z_near) & (Z <= self.z_far)
        Zs = np.where(seen, Z, 1.)
        tz = np.rint(Zs)
        seen &= (tz >= 1.) & (tz <= 65534.)
        lim = float(2 ** 31 - 1)
        out = np.zeros(tips.shape, np.int32)
        out[..., 0] = np.clip(np.floor(self.f * X / Zs + self.ppx), -lim, lim)
        out[..., 1] = np.clip(np.floor(self.f * Y / Zs + self.ppy), -lim, lim)
        out[..., 2] = np.where(seen, tz, 0.)
        out[~seen, :2] = 0
        return out

    def render(self, part_tforms, labels='fine', table=None, empty_depth=65535, seed=0, hole_rate=0., noise_amp=0,
               depth_out=None, labels_out=None, sensor=None):
        """part_tforms: host float32 [N, 16, 12] (one hand) or [N, 32, 12] (two).  labels: see tri_labels.  table: None, or
        (nx, ny, nz, d) in camera space as [4] or [N, 4].  empty_depth: 65535 for dataset frames, 0 for raw camera frames.
        hole_rate: the share of drawn pixels dropped (threshold hole_rate * 2^32 of rule H); noise_amp: depth units.
        sensor: a StereoSensor of this frame size; the clean frame and the same scene from a camera moved by the sensor's
        baseline along +x go through sensor.sense (seed is then the IR noise's), which replaces rule H: hole_rate and
        noise_amp must be zero.
        Returns device (depth uint16 [N, H, W], labels uint16 [N, H, W]); every pixel of both is written.  Frame n of a
        long batch gets the same image whatever max_frames is."""
        if sensor is not None:
            return self._render_through(sensor, part_tforms, labels, table, empty_depth, seed, hole_rate, noise_amp, depth_out,
                                        labels_out)
        t = np.ascontiguousarray(part_tforms, np.float32)
        assert t.ndim == 3 and t.shape[1] in self._mesh and t.shape[2] == 12, t.shape
        N, P = int(t.shape[0]), int(t.shape[1])
        H, W = self.DIM_Y, self.DIM_X
        verts, vert_part, tris = self._device_mesh(P)
        key = (P, labels if isinstance(labels, str) else np.asarray(labels, np.uint16).tobytes())
        if key not in self._labels_cu:
            self._labels_cu[key] = to_device(self.tri_labels(P, labels))
        tri_label = self._labels_cu[key]
        if table is not None:
            table = np.ascontiguousarray(np.broadcast_to(np.asarray(table, np.float32).reshape(-1, 4), (N, 4)))
        depth_out = DeviceArray((N, H, W), np.uint16) if depth_out is None else depth_out
        labels_out = DeviceArray((N, H, W), np.uint16) if labels_out is None else labels_out
        for o in (depth_out, labels_out):
            assert np.dtype(o.dtype) == np.uint16 and int(np.prod(o.shape)) == N * H * W, (o.shape, o.dtype)
        threshold = min(int(float(hole_rate) * 4294967296.), 0xFFFFFFFF) if hole_rate > 0. else 0
        d0, l0 = device_ptr(depth_out), device_ptr(labels_out)
        for a in range(0, N, self.max_frames):
            b = min(N - a, self.max_frames)
            t_cu = to_device(t[a:a + b])
            table_cu = to_device(table[a:a + b]) if table is not None else None
            rc = self._lb.rdf_hand_scene_render(
                b, W, H, int(verts.shape[0]), verts.ptr, vert_part.ptr, int(tris.shape[0]), tris.ptr, tri_label.ptr, P,
                t_cu.ptr, table_cu.ptr if table_cu is not None else None, self.f, self.ppx, self.ppy, self.z_near, self.z_far,
                int(empty_depth), (int(seed) + a * FRAME_SEED_STEP) & 0xFFFFFFFF, threshold, int(noise_amp), self._keys.ptr,
                d0 + a * H * W * 2, l0 + a * H * W * 2, self._rt.stream())
            _lib.check(self._lb, rc, "rdf_hand_scene_render")
        for o in (self._keys, depth_out, labels_out):
            if hasattr(o, "mark_dirty"):
                o.mark_dirty()
        return depth_out, labels_out

    def _render_through(self, sensor, part_tforms, labels, table, empty_depth, seed, hole_rate, noise_amp, depth_out, labels_out):
        if hole_rate or noise_amp:
            raise ValueError("a sensor replaces holes and noise: hole_rate and noise_amp must be zero with sensor=")
        assert (sensor.DIM_Y, sensor.DIM_X) == (self.DIM_Y, self.DIM_X), "the sensor is of another frame size"
        t = np.ascontiguousarray(part_tforms, np.float32)
        # the right camera sits at x = +B: every point's x is B less in its space.  float64, cast once
        right = t.astype(np.float64)
        right[:, :, 3] -= sensor.baseline
        right_table = None
        if table is not None:
            right_table = np.asarray(table, np.float32).reshape(-1, 4).astype(np.float64)
            right_table[:, 3] -= right_table[:, 0] * sensor.baseline
            right_table = right_table.astype(np.float32)
        depth_l, labels_l = self.render(t, labels, table, empty_depth)
        depth_r, _ = self.render(right.astype(np.float32), labels, right_table, empty_depth)
        return sensor.sense(depth_l, labels_l, depth_r, seed, empty_depth, depth_out, labels_out)

    def make_dataset(self, dataset_dir, num_images, seed, labels='fine', plane=None, two_hands=False, ranges=None,
                     hole_rate=0., noise_amp=0, sensor=None, targets=False):
        """Sample `num_images` poses from `seed` (HandModel.sample_poses), render them in dataset convention -- no table,
        background depth 65535, label 0 = none -- and write `dataset_dir` with dataset.write_dataset and the scheme's
        id_to_color.  plane: the camera's table plane; default look_down_plane(550 mm).  sensor: see render.  targets=True also writes
        `targets.npy` to the directory: int32 [N, 5 or 10, 3], the fingertip_targets of the sampled poses for `plane` -- what
        dataset.read_targets and dataset.fit_votes_saved_model read; without it the directory is what it always was.  Returns
        the host (depth, labels)."""
        rng = np.random.default_rng(seed)
        plane = look_down_plane(550. * self.model.units_per_mm) if plane is None else plane
        poses = self.model.sample_poses(num_images, rng, ranges)
        left = None
        if two_hands:       # the hands' wrists 220 mm apart
            shift = np.zeros(POSE_SIZE)
            shift[0] = 110. * self.model.units_per_mm
            left = self.left_model.sample_poses(num_images, rng, ranges) - shift
            poses = poses + shift
        depth, lab = self.render(self.transforms(poses, plane, left), labels, None, 65535, int(seed) & 0xFFFFFFFF, hole_rate,
                                 noise_amp, sensor=sensor)
        depth, lab = depth.get(), lab.get()
        scheme = labels if isinstance(labels, str) else 'fine'
        write_dataset(dataset_dir, depth, lab, HandModel.id_to_color(scheme))
        if targets:
            np.save(os.path.join(dataset_dir, TARGETS_FILE), self.fingertip_targets(poses, plane, left))
        return depth, lab

    def make_shape_dataset(self, dataset_dir, num_images, seed, shapes=tuple(SHAPES), plane=None, ranges=None, hole_rate=0.,
                           noise_amp=0, sensor=None):
        """A training set for a SHAPE forest (shape.ShapeVoter): frame n shows one hand of shape shapes[n % len(shapes)]
        (HandModel.shape_dataset_poses from `seed`), rendered as make_dataset renders, and every hand pixel of it carries the
        label 1 + n % len(shapes), 0 elsewhere.  Written with dataset.write_dataset, one colour per shape, and `shapes.npy`,
        int32 [N], the shape index of every frame (dataset.read_shapes); train_forest trains on the directory as on any
        other.  Returns the host (depth, labels, shape indices)."""
        shapes = tuple(shapes)
        assert 1 <= len(shapes) <= len(SHAPE_COLORS), f"1 .. {len(SHAPE_COLORS)} shapes"
        rng = np.random.default_rng(seed)
        plane = look_down_plane(550. * self.model.units_per_mm) if plane is None else plane
        poses, index = self.model.shape_dataset_poses(num_images, rng, shapes, ranges)
        depth, lab = self.render(self.transforms(poses, plane), 'fine', None, 65535, int(seed) & 0xFFFFFFFF, hole_rate,
                                 noise_amp, sensor=sensor)
        depth, lab = depth.get(), lab.get()
        lab = np.where(lab != 0, (1 + index)[:, None, None], 0).astype(np.uint16)
        write_dataset(dataset_dir, depth, lab, {1 + k: SHAPE_COLORS[k] for k in range(len(shapes))})
        np.save(os.path.join(dataset_dir, SHAPES_FILE), index)
        return depth, lab, index

    def camera_sequence(self, poses, plane, left_poses=None, hole_rate=0., noise_amp=0, seed=0, labels='fine', labels_out=None,
                        sensor=None):
        """Raw camera frames of `poses` [N, 26] (and the left hand's `left_poses`) over the table of `plane`: the table is
        drawn, empty pixels and holes are 0 -- device uint16 [N, H, W], what BeatsSession.run_sequence takes.  The truth
        labels go to `labels_out` when given.
        Half a pixel: the renderer samples pixel (i, j) at (i + 0.5, j + 0.5), while deproject_points places pixel x at
        sx = x.  A caller who wants the front end to deproject these frames onto the rendered geometry builds this object
        with (ppx + 0.5, ppy + 0.5)."""
        depth, _ = self.render(self.transforms(poses, plane, left_poses), labels, table_of_plane(plane), 0, seed, hole_rate,
                               noise_amp, labels_out=labels_out, sensor=sensor)
        return depth
