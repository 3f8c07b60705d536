"""A colour-glove recording to a training set: the reference's converter (src/live_data_convert.py) without
its camera, window and GL.

`RecordingConverter.convert(frames)` takes (depth uint16 [H, W], colour uint8 [H, W, 3]) pairs, the colour already aligned
to the depth, and writes what `DecisionTreeDatasetConfig` and `dataset.train_forest` read: `{i:08d}_labels.png`,
`{i:08d}_labels_rgba.png`, `{i:08d}_depth.png` and `config.json`.  Per frame it makes the reference's calls in the
reference's order (tick(), :319-458): deproject_points, the table plane on the first and on every 20th frame
(CalibratedPlane), transform_points into the plane, filter_points_by_plane, transform_points back with the host's
np.linalg.inv of the plane, the depth cleared and rebuilt by depths_from_points, the optional Gaussian (k = 15), the optional
mask forest, the colour mapping on the first frame, and ColorLabeler.label_frame.  Everything up to the PNG encoder stays
on the stream; one copy per output image ends the frame.

With `rerender=True` every frame is also re-rendered as the reference's rerender_image does it (:207-282): the frame's points
as a triangle mesh, scaled, skewed, rotated or shifted at random about the scene's centre in plane space (not on the first
two frames), drawn back into a new depth and a new aligned colour image that replace the frame's for the labelling.  The
reference draws through OpenGL; here it is SceneRerender's software rasteriser (its rules: include/rdf_labels.h), the centre
is summed on the device, and one 32-byte copy of it per frame reaches the host, which composes the matrix.  As in the
reference the re-rendered depth comes from the points, so it replaces the Gaussian-filtered image too.
Out of scope: make_triangles as a kernel of its own (nothing here consumes an index buffer), reading .bag files and
rs.align, and the host-side depth_rgba debug PNG.
One deviation: the points buffer is cleared every frame.  The reference never clears it, so where this frame has no depth
reading, points of earlier frames (on the first frame, uninitialised memory) are transformed again and written into the
rebuilt depth.
"""
import json
import os

import numpy as np

from .calibrated_plane import CalibratedPlane
from .color_labels import ColorLabeler
from .cuda.points_ops import PointsOps
from .device import DeviceArray
from .engine.buffer import GpuBuffer
from .rerender import SceneRerender

FRAMES_PER_RECOMPUTE_PLANE = 20
GAUSSIAN_K_SIZE = 15
FIRST_AUGMENTED_FRAME = 3        # "dont randomly transform 1st frame": frame_count > 2 (live_data_convert.py:251-261)


def draw_augmentation(rng, frame_count, scale_variance, scale_skew_variance, rotate_variance, translate_variance):
    """One frame's random transform, drawn in the reference's order (live_data_convert.py:262-265): scale ~ N(1, .), skew x 3,
    rotate, translate x 3 ~ N(0, .).  Frames before the third draw with zero variances, which still advances `rng`.  (The
    reference makes a fresh, unseeded default_rng() for every draw; here all draws come from the converter's one generator.)
    Returns (scale, skew [3], rotate, translate [3])."""
    if frame_count < FIRST_AUGMENTED_FRAME:
        scale_variance = scale_skew_variance = rotate_variance = translate_variance = 0.
    scale = rng.normal(1, scale_variance, 1)[0]
    skew = rng.normal(0, scale_skew_variance, 3)
    rotate = rng.normal(0., rotate_variance, 1)[0]
    translate = rng.normal(0., translate_variance, 3)
    return scale, skew, rotate, translate


class RecordingConverter:
    def __init__(self, out_path, depth_dims, intrinsics, num_colors, plane_z_threshold, mask_model=None, mask_label=None,
                 gaussian_noise=0., max_images=None, num_random_guesses=25000, num_tries=8, num_iterations=32, seed=None,
                 rerender=False, scale_variance=0.1, scale_skew_variance=0., rotate_variance=0., translate_variance=0.,
                 augment_seed=None):
        """depth_dims = (DIM_Y, DIM_X); intrinsics = (focal, ppx, ppy) of the depth camera; num_colors = --colors;
        plane_z_threshold = --plane_z_threshold; mask_model (a DecisionForest or the path of its .npy) with mask_label;
        gaussian_noise = --gaussian_noise (applied above 0.1, as there); max_images = --max_images.  seed: of the plane's
        random draws.  rerender: re-render every frame with a random transform of these variances (the defaults are the
        reference's, :64-67), drawn from default_rng(augment_seed)."""
        assert (mask_model is None) == (mask_label is None), "mask_model and mask_label are both required if using mask"
        self.OUT_PATH = out_path
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        f, ppx, ppy = (float(v) for v in np.asarray(intrinsics, np.float64).reshape(-1)[:3])
        self.FOCAL = np.float32(f)
        self.PP = np.array([ppx, ppy], dtype=np.float32)
        self.PLANE_Z_THRESHOLD = float(plane_z_threshold)
        self.gaussian_noise = float(gaussian_noise or 0)
        self.MAX_IMAGES = max_images if max_images is not None else np.inf
        self.MASK_LABEL = mask_label
        self.mask_model = None
        if mask_model is not None:
            from .decision_tree import DecisionForest, DecisionTreeEvaluator
            self.mask_model = DecisionForest.load(mask_model) if isinstance(mask_model, (str, os.PathLike)) else mask_model
            self.decision_tree_evaluator = DecisionTreeEvaluator()
            self.mask_labels_gpu = GpuBuffer((1, self.DIM_Y, self.DIM_X), dtype=np.uint16)
        self.points_ops = PointsOps()
        self.calibrated_plane = CalibratedPlane(num_random_guesses, self.PLANE_Z_THRESHOLD, seed)
        self.labeler = ColorLabeler(num_colors, num_tries, num_iterations)
        self.depth_gpu = GpuBuffer((1, self.DIM_Y, self.DIM_X), dtype=np.uint16)
        self.depth_gpu_2 = GpuBuffer((1, self.DIM_Y, self.DIM_X), dtype=np.uint16)
        self.pts_gpu = GpuBuffer((self.DIM_Y, self.DIM_X, 4), dtype=np.float32)
        self.color_gpu = GpuBuffer((self.DIM_Y, self.DIM_X, 3), dtype=np.uint8)
        self.labels_gpu = DeviceArray((self.DIM_Y, self.DIM_X), np.uint16)
        self.labels_rgba_gpu = DeviceArray((self.DIM_Y, self.DIM_X, 4), np.uint8)
        self.rerender = bool(rerender)
        if self.rerender:
            self.SCALE_VARIANCE, self.SCALE_SKEW_VARIANCE = float(scale_variance), float(scale_skew_variance)
            self.ROTATE_VARIANCE, self.TRANSLATE_VARIANCE = float(rotate_variance), float(translate_variance)
            self.augment_rng = np.random.default_rng(augment_seed)
            self.scene_rerender = SceneRerender((self.DIM_Y, self.DIM_X), (self.FOCAL, self.PP[0], self.PP[1]))
            self.depth_rerendered_gpu = GpuBuffer((1, self.DIM_Y, self.DIM_X), dtype=np.uint16)
            self.color_rerendered_gpu = GpuBuffer((self.DIM_Y, self.DIM_X, 3), dtype=np.uint8)
            self.obj_tform = None            # the last frame's transform
        self.frame_count = 0
        self.color_mapping = None

    def _path(self, name):
        return os.path.join(self.OUT_PATH, f'{str(self.frame_count - 1).zfill(8)}_{name}.png')

    def tick(self, depth, color, init_colors=None):
        """One frame.  Returns False once max_images frames are written.  init_colors: the first frame's starting colours
        (ColorLabeler.make_color_mapping), None to draw them."""
        from PIL import Image
        if self.frame_count >= self.MAX_IMAGES:
            return False
        self.frame_count += 1
        W, H, n_px = self.DIM_X, self.DIM_Y, self.DIM_X * self.DIM_Y
        po, cp = self.points_ops, self.calibrated_plane
        dims = np.array([1, W, H, -1], dtype=np.int32)
        self.depth_gpu.cu().set(np.ascontiguousarray(depth, np.uint16).reshape(1, H, W))
        self.pts_gpu.cu().fill(0)
        po.deproject_points(dims, self.PP, self.FOCAL, self.depth_gpu.cu(), self.pts_gpu.cu())
        if not cp.is_set() or self.frame_count % FRAMES_PER_RECOMPUTE_PLANE == 0:
            cp.make(self.pts_gpu, (W, H))
        po.transform_points(np.int32(n_px), self.pts_gpu.cu(), cp.get_mat())
        cp.filter_points_by_plane(np.int32(n_px), np.float32(self.PLANE_Z_THRESHOLD), self.pts_gpu.cu())
        if self.rerender:
            self.scene_rerender.center(self.pts_gpu.cu())     # while the points are in plane space; read after the uploads
        po.transform_points(np.int32(n_px), self.pts_gpu.cu(), np.linalg.inv(cp.get_mat()))
        self.depth_gpu.cu().fill(np.uint16(0))
        po.depths_from_points(dims, self.depth_gpu.cu(), self.pts_gpu.cu())
        if self.gaussian_noise > 0.1:
            po.gaussian_depth_filter(self.depth_gpu, self.depth_gpu_2, sigma=self.gaussian_noise, k_size=GAUSSIAN_K_SIZE)
            self.depth_gpu.cu().set(self.depth_gpu_2.cu())
        self.color_gpu.cu().set(np.ascontiguousarray(color, np.uint8).reshape(H, W, 3))
        depth_gpu, color_gpu = self.depth_gpu, self.color_gpu
        if self.rerender:
            depth_gpu, color_gpu = self._rerender_image()
        mask = None
        if self.mask_model is not None:
            # (the reference turns 65535 back into 0 after the forest and into 65535 again before it saves: the same image)
            po.convert_0s_to_maxuint(n_px, depth_gpu.cu())
            self.mask_labels_gpu.cu().fill(np.uint16(0))
            self.decision_tree_evaluator.get_labels_forest(self.mask_model, depth_gpu.cu(), self.mask_labels_gpu.cu())
            mask = self.mask_labels_gpu.cu()
        if not self.labeler.is_set():
            if mask is not None:
                self.labeler.mask_color_image(color_gpu.cu(), mask, self.MASK_LABEL)
            self.color_mapping = self.labeler.make_color_mapping(color_gpu.cu(), init_colors)
        self.labeler.label_frame(color_gpu.cu(), depth_gpu.cu(), mask, self.MASK_LABEL if mask is not None else None,
                                 self.labels_gpu, self.labels_rgba_gpu)
        Image.fromarray(self.labels_gpu.get()).save(self._path('labels'))
        Image.fromarray(self.labels_rgba_gpu.get()).save(self._path('labels_rgba'))
        Image.fromarray(depth_gpu.cu().get()[0]).save(self._path('depth'))
        return True

    def _rerender_image(self):
        """rerender_image (live_data_convert.py:207-282): the frame's points and colours, moved by a random transform about the
        scene's centre, drawn into the second pair of buffers.  Returns (depth, colour) for the rest of the frame."""
        sums = self.scene_rerender.center_cu.get()
        center = sums[:3] / sums[3] if sums[3] != 0 else np.zeros(3)          # (no point left: nothing is drawn either way)
        scale, skew, rotate, translate = draw_augmentation(self.augment_rng, self.frame_count, self.SCALE_VARIANCE,
                                                           self.SCALE_SKEW_VARIANCE, self.ROTATE_VARIANCE,
                                                           self.TRANSLATE_VARIANCE)
        self.obj_tform = SceneRerender.make_transform(self.calibrated_plane.get_mat(), center, scale, skew, rotate, translate)
        self.scene_rerender.run(self.pts_gpu.cu(), self.color_gpu.cu(), self.obj_tform, self.depth_rerendered_gpu.cu(),
                                self.color_rerendered_gpu.cu())
        return self.depth_rerendered_gpu, self.color_rerendered_gpu

    def finish(self):
        """config.json, the entry point into the dataset (live_data_convert.py:284-298)."""
        obj = {'img_dims': [self.DIM_X, self.DIM_Y], 'num_images': self.frame_count,
               'id_to_color': self.labeler.id_to_color()}
        with open(os.path.join(self.OUT_PATH, 'config.json'), 'w') as fh:
            fh.write(json.dumps(obj))
        return obj

    def convert(self, frames, init_colors=None):
        """Every (depth, colour) pair of `frames`, up to max_images, then config.json.  Returns the number of frames written."""
        os.makedirs(self.OUT_PATH, exist_ok=True)
        for depth, color in frames:
            if not self.tick(depth, color, init_colors):
                break
        self.finish()
        return self.frame_count
